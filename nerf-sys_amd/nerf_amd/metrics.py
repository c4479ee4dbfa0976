"""Image quality of rendered views — the PSNR and SSIM of runtime_evaluate (pipelines/online_stage/runtime_adapt.py:
24-210, metrics at :150-158), measured by one HIP kernel per batch of images (csrc/metrics.hip) and kept on the device.

The rendered image is linear, the ground truth is 8-bit sRGB (uint8, or the same values as floats in [0,1]); both are
brought into ``color_space`` as losses.color_space_transformer does.  SSIM is pytorch_msssim.ssim with its defaults and
data_range=1, per channel.  LPIPS is not measured."""
from __future__ import annotations

import torch

from . import kernels as K


def image_metrics(pred_linear, gt, color_space: str = "linear") -> dict:
    """pred_linear, gt: (H,W,3) or (N,H,W,3) device tensors -> {"mse": (N,), "psnr": (N,), "ssim": (N,),
    "ssim_channels": (N,3)} device tensors; psnr = -10 log10(max(mse, 1e-8)) as losses.psnr, ssim = mean of the three
    channels.  The ground truth is clamped to [0,1] in every colour space, as color_space_transformer clamps it.
    Nothing is read on the host, with one exception: ``identity`` with a float ground truth keeps
    color_space_transformer's refusal of values outside [0,1] (a ValueError), which has to look at the data."""
    if isinstance(gt, torch.Tensor) and gt.dtype != torch.uint8:
        gt = gt.float()
        if str(color_space).lower() == "identity" and gt.is_cuda and gt.numel() and (
                (gt.max() > 1) or (gt.min() < 0)):
            raise ValueError("GT out of [0,1]; identity mode assumes normalized linear GT.")
    if isinstance(pred_linear, torch.Tensor) and pred_linear.is_cuda:
        pred_linear = pred_linear.float().contiguous()
        if isinstance(gt, torch.Tensor) and gt.is_cuda:
            gt = gt.contiguous()
    out = K.image_metrics(pred_linear, gt, str(color_space).lower())
    mse = out[:, 0]
    return {"mse": mse, "psnr": -10.0 * torch.log10(mse.clamp_min(1e-8)), "ssim": out[:, 1:].mean(dim=1),
            "ssim_channels": out[:, 1:]}


def evaluate_views(model, poses, images, *, H: int, W: int, fx: float, fy: float, cx: float, cy: float,
                   color_space: str = "linear", **render_image_kwargs) -> dict:
    """Phase B of runtime_evaluate: render_image for every pose, PSNR and SSIM of every view against ``images``
    (V,H,W,3; uint8 sRGB or floats), accumulated on the device and read once at the end.
    Returns {"psnr": mean, "ssim": mean, "per_view": [{"psnr": .., "ssim": ..}, ...]} as Python floats."""
    from .ray_rendering import render_image
    n = int(poses.shape[0])
    if int(images.shape[0]) != n:
        raise ValueError(f"{n} poses but {int(images.shape[0])} images")
    device = next(model.parameters()).device
    acc = torch.empty((n, 2), dtype=torch.float32, device=device)
    with torch.no_grad():
        for v in range(n):
            img, _, _ = render_image(model, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, c2w=poses[v], **render_image_kwargs)
            m = image_metrics(img, images[v].to(device), color_space)
            acc[v, 0], acc[v, 1] = m["psnr"][0], m["ssim"][0]
    rows = acc.tolist()  # the one host read
    per_view = [{"psnr": p, "ssim": s} for p, s in rows]
    return {"psnr": sum(r["psnr"] for r in per_view) / max(n, 1), "ssim": sum(r["ssim"] for r in per_view) / max(n, 1),
            "per_view": per_view}
