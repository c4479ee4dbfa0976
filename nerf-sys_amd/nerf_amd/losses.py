"""Loss head — nerfs/losses.py:10-32 + nerfs/color_space.py:4-66 of the reference.

``compute_mse_loss(P, model, data, ...)`` keeps the reference signature (P.ray_samples,
P.chunk_points, P.color_space) and adds the canonical coarse+fine term when P.n_importance > 0.
The fused training engine (trainer.py) computes the same loss inside the compositing kernel.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .ray_rendering import render_rays


def linear_to_srgb(x):
    x = x.clamp(0, 1)
    return torch.where(x <= 0.0031308, 12.92 * x, 1.055 * x.pow(1 / 2.4) - 0.055)


def srgb_to_linear(x):
    return torch.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055).pow(2.4))


def color_space_transformer(pred_linear, gt_tensor, color_space: str):
    cs = str(color_space).lower()
    pred32 = pred_linear.to(torch.float32)
    gt32 = gt_tensor.to(torch.float32).clamp(0, 1)
    if cs == "linear":
        pred, gt = pred32.clamp(0, 1), srgb_to_linear(gt32).clamp(0, 1)
    elif cs == "srgb":
        pred, gt = linear_to_srgb(pred32).clamp(0, 1), gt32.clamp(0, 1)
    elif cs == "identity":
        if (gt32.max() > 1) or (gt32.min() < 0):
            raise ValueError("GT out of [0,1]; identity mode assumes normalized linear GT.")
        pred, gt = pred32, gt32
    else:
        raise ValueError(f"Invalid color_space={color_space!r}; use 'linear'|'srgb'|'identity'")
    return pred.to(pred_linear.dtype), gt.to(pred_linear.dtype)


def compute_mse_loss(P, model, data, params=None, active_module=None, reduction="mean", **render_kwargs):
    """nerfs/losses.py:10-32; with P.n_importance > 0 the loss is MSE(fine) + MSE(coarse) (canonical NeRF).
    ``render_kwargs`` pass through to render_rays (e.g. the parity tests' injected jitter u_strat / u_pdf)."""
    gt_rgb, rays = data["rgbs"], data["rays"]
    n_imp = int(getattr(P, "n_importance", 0) or 0)
    out = render_rays(model, rays, ray_samples=P.ray_samples, params=params, active_module=active_module,
                      chunk=P.chunk_points, n_importance=n_imp, return_extras=True, **render_kwargs)
    pred_rgb, extras = out[0], out[-1]
    cs = getattr(P, "color_space", "linear")
    a, b = color_space_transformer(pred_rgb, gt_rgb, cs)
    loss = F.mse_loss(a, b, reduction=reduction)
    if n_imp > 0:
        a, b = color_space_transformer(extras["rgb_coarse"], gt_rgb, cs)
        loss = loss + F.mse_loss(a, b, reduction=reduction)
    return loss


def compute_fim_loss(P, model, data, params=None, active_module=None, *, grad_buffer=None, update_fisher=False,
                     clamp_factor=5, **_):
    """nerfs/losses.py:35-151 as the reference runs it: one render_rays pass (P.ray_samples, no importance pass) and
    the per-ray MSE mean (:67-73) — which the reference returns, because no module defines ``fisher_store`` /
    ``fim_loss`` (:75-78).  ``model.submodules[active_module]`` is resolved first, as the reference
    does (:75), so a call without an active module fails there too.  A model that does carry a Fisher store is refused:
    the Fisher-weighted branch (:79-151) is out of scope."""
    gt_rgb, rays = data["rgbs"], data["rays"]
    pred = render_rays(model, rays, ray_samples=P.ray_samples, params=params, active_module=active_module,
                       chunk=P.chunk_points)[0]
    a, b = color_space_transformer(pred, gt_rgb, getattr(P, "color_space", "linear"))
    base_loss = F.mse_loss(a, b, reduction="none").mean(dim=-1).mean()
    expert_module = model.submodules[active_module]  # noqa: F841  (losses.py:75)
    if not hasattr(model, "fisher_store") or not hasattr(model, "fim_loss"):
        return base_loss
    raise NotImplementedError("the Fisher-weighted loss (nerfs/losses.py:79-151) is out of scope (SURVEY §2 row 4)")


def psnr(mse: float) -> float:
    import math
    return -10.0 * math.log10(max(float(mse), 1e-8))


def image_psnr(pred_linear, gt_u8_or_srgb, color_space: str = "linear") -> float:
    """Full-image PSNR as the reference evaluates it (pipelines/online_stage/runtime_adapt.py:150-157):
    the rendered image is linear, the ground truth is 8-bit sRGB, and both are brought into
    ``color_space`` (the training colour space, args.py:98-102) by color_space_transformer."""
    gt = gt_u8_or_srgb.float() / 255.0 if gt_u8_or_srgb.dtype == torch.uint8 else gt_u8_or_srgb.float()
    a, b = color_space_transformer(pred_linear.float(), gt.to(pred_linear.device), color_space)
    return psnr(F.mse_loss(a, b).item())


def image_ssim(pred_linear, gt_u8_or_srgb, color_space: str = "linear") -> float:
    """Full-image SSIM beside image_psnr (runtime_adapt.py:158: pytorch_msssim.ssim, data_range=1, on the same
    colour-space-transformed pair), mean of the three channels; measured by the HIP kernel behind metrics.image_metrics."""
    from .metrics import image_metrics
    return float(image_metrics(pred_linear, gt_u8_or_srgb.to(pred_linear.device), color_space)["ssim"][0])
