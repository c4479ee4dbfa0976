"""Plain references for the fused Instant-NGP MLP (csrc/ngp.hip) -- CPU only, no project kernels.

``plan_reference`` restates the host-side ``make_plan`` (packed layout, backward LDS plan, weight-gradient block
count) so that a test can state which kernel path a configuration reaches *before* it runs: the
``ngp_bwd_kernel<NSB>`` instantiation, and whether the bias-gradient partials have room in LDS (``bsum >= 0``) or
every layer's bias gradient is summed by one wave in registers (``bsum < 0``).

``mlp_reference`` evaluates ``[rgb | sigma]`` from the *named* tensors of ``oracle.ngp_oracle.ngp_param_shapes``
and an already-encoded position (``enc``), so ``in_dim`` and ``sh_levels`` are free of any hash grid.  It is built
from the oracle's own pieces (``_lin``, ``_TruncExp``, ``sh_encode``, ``freq_encode``), runs in float64 by
default, is differentiable by autograd, and can hand back the pre-activation of every ReLU unit.

``kink_free_rows`` picks the rows whose ReLU pre-activations all stay away from 0: there an fp32 kernel and the
fp64 reference take the same side of every ReLU, so their gradients differ by rounding only.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from oracle import ngp_oracle as NO

MAX_LAYERS = 12          # NGP_MAX_LAYERS
MAX_WGRAD_BLOCKS = 32    # NGP_MAX_SB
BWD_ROWS = 32            # NGP_BROWS
DIR_DIMS = (1, 4, 9, 16, 25, 27)   # SH levels 1..5, or the frequency encoding (3 + 3 * 2 * 4)

Layer = namedtuple("Layer", "K N Kpad Npad w_off b_off")
Plan = namedtuple("Plan", "layers total smem_floats bsum wgrad_blocks slots_per_wave nsb head")


# The named configurations of the edge tests: (in_dim, hidden, sigma_depth, geo, colour hidden, colour depth,
# dir_mode (0 SH, 1 frequency), sh_levels) and the path each must reach: (layers, ngp_bwd_kernel<NSB>, bsum < 0).
Config = namedtuple("Config", "in_dim hidden sigma_depth geo color_hidden color_depth dir_mode sh_levels")
CONFIGS = {
    "tiny": Config(2, 1, 1, 0, 1, 1, 0, 4),            # width-1 layers, geo 0 (empty tensors)
    "nodepth": Config(8, 33, 0, 0, 17, 0, 0, 4),       # 2 layers: the head is layer 0, rgb reads cin
    "sd0": Config(16, 33, 0, 7, 17, 1, 0, 4),          # the head writes d_enc
    "wide_in": Config(64, 17, 1, 31, 33, 1, 0, 4),     # Kpad 64 / Npad 32 first layer, geo 31
    "in40": Config(40, 64, 2, 15, 64, 2, 0, 4),        # production widths, in_dim > 32
    "freq31": Config(16, 24, 1, 31, 40, 1, 1, 4),      # 31 + 27 = 58 colour inputs
    "near_sh3": Config(32, 64, 2, 15, 64, 2, 0, 3),    # one field away from the production shape ...
    "near_geo14": Config(32, 64, 2, 14, 64, 2, 0, 4),
    "near_in33": Config(33, 64, 2, 15, 64, 2, 0, 4),
    "sh1": Config(16, 32, 1, 15, 32, 1, 0, 1),         # dir_dim 1
    "sh5": Config(16, 32, 1, 15, 32, 1, 0, 5),         # dir_dim 25
    "nsb8": Config(32, 64, 4, 15, 64, 3, 0, 4),        # 28 weight-gradient blocks
    "nsb8_in64": Config(64, 64, 3, 15, 64, 3, 0, 4),   # 26 blocks
    "twelve": Config(16, 32, 5, 15, 32, 5, 0, 4),      # NGP_MAX_LAYERS
    "mix": Config(32, 64, 3, 15, 32, 3, 0, 4),         # 64 -> 32 width change
    "prod": Config(32, 64, 2, 15, 64, 2, 0, 4),        # the production shape itself (compile-time kernels)
}
EXPECTED_PATH = {
    "tiny": (4, 4, False), "nodepth": (2, 4, False), "sd0": (3, 4, False), "wide_in": (4, 4, False),
    "in40": (6, 6, False), "freq31": (4, 4, False), "near_sh3": (6, 4, False), "near_geo14": (6, 4, False),
    "near_in33": (6, 6, False), "sh1": (4, 4, False), "sh5": (4, 4, False), "nsb8": (9, 8, True),
    "nsb8_in64": (8, 8, True), "twelve": (12, 4, True), "mix": (8, 4, False), "prod": (6, 4, False),
}
# shapes make_plan rejects, as plan_reference arguments
REJECTED = {
    "hidden65": (16, 65, 2, 15, 64, 2, 16),
    "in65": (65, 64, 2, 15, 64, 2, 16),
    "geo32": (32, 64, 2, 32, 64, 2, 16),
    "layers13": (16, 32, 6, 15, 32, 5, 16),
    "twelve_wide": (16, 64, 5, 15, 64, 5, 16),  # 12 layers of width 64: 40 weight-gradient blocks > 32
}


def config_dir_dim(c):
    return c.sh_levels * c.sh_levels if c.dir_mode == 0 else 27


def config_plan(c):
    return plan_reference(c.in_dim, c.hidden, c.sigma_depth, c.geo, c.color_hidden, c.color_depth, config_dir_dim(c))


def pad32(x):
    return (x + 31) // 32 * 32


def plan_reference(in_dim, hidden, sigma_depth, geo, color_hidden, color_depth, dir_dim):
    """make_plan(save = true) of csrc/ngp.hip, or None for a shape it rejects."""
    if not (1 <= in_dim <= 64 and 1 <= hidden <= 64 and 1 <= color_hidden <= 64):
        return None
    if geo < 0 or geo + 1 > 32 or sigma_depth < 0 or color_depth < 0:
        return None
    if dir_dim not in DIR_DIMS or geo + dir_dim > 64:
        return None
    nl = sigma_depth + color_depth + 2
    if nl > MAX_LAYERS:
        return None
    head = sigma_depth
    layers, o, last = [], 0, in_dim
    for l in range(nl):
        if l < head:
            N, K = hidden, last
        elif l == head:
            N, K = 1 + geo, last
        elif l < nl - 1:
            N, K = color_hidden, (geo + dir_dim if l == head + 1 else last)
        else:
            N, K = 3, (geo + dir_dim if l == head + 1 else last)
        Np, Kp = pad32(N), pad32(K)
        w_off = o
        o += Np * Kp
        b_off = o
        o += Np
        layers.append(Layer(K, N, Kp, Np, w_off, b_off))
        if l < head:
            last = hidden
        elif l > head:
            last = color_hidden
    total = o
    # backward LDS plan (floats): enc tile, cin tile, two gradient tiles, d sigma_raw, one tile per saved activation
    s = BWD_ROWS * (pad32(in_dim) + 4)
    s += BWD_ROWS * (pad32(geo + dir_dim) + 4)
    s += 2 * BWD_ROWS * 68
    s += BWD_ROWS
    for l, L in enumerate(layers):
        if l != head and l != nl - 1:
            s += BWD_ROWS * (L.Npad + 4)
    bsum = -1
    if (s + 4 * nl * 64) * 4 <= 80 * 1024:
        bsum = s
        s += 4 * nl * 64
    if s * 4 > 160 * 1024:
        return None
    nblk = sum((L.Npad // 32) * (L.Kpad // 32) for L in layers)
    per_wave = (nblk + 3) // 4
    if 4 * per_wave > MAX_WGRAD_BLOCKS:
        return None
    nsb = 4 if per_wave <= 4 else 6 if per_wave <= 6 else 8
    return Plan(tuple(layers), total, s, bsum, nblk, per_wave, nsb, head)


def dir_encode(d, dir_mode, sh_levels=4):
    """MetaNGP._enc_dir: d / clamp_min(|d|, 1e-9), then the SH encoder (which normalises again) or the frequency
    encoder (which does not)."""
    dn = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-9)
    return NO.sh_encode(dn, sh_levels) if dir_mode == 0 else NO.freq_encode(dn, 4)


def mlp_reference(named, enc, x_d, *, sigma_depth, color_depth, dir_mode, sh_levels, sigmoid, dtype=torch.float64,
                  return_preacts=False):
    """[rgb | sigma] (M, 4) of the MetaNGP MLP on encoded positions enc (M, in_dim) and x_d (M, 6) (columns 3..5:
    the view direction).  ``named`` maps ngp_param_shapes' names to tensors; tensors that already have ``dtype`` are
    used as they are, so autograd reaches them.  return_preacts: also the list of every ReLU layer's pre-activation
    (M, width), trunk first."""
    p = {k: (v if v.dtype == dtype else v.to(dtype)) for k, v in named.items()}
    h = enc.to(dtype)
    pre = []
    for i in range(sigma_depth):
        z = NO._lin(h, p, f"sigma_trunk.{i}.linear")
        pre.append(z)
        h = torch.relu(z)
    sigma = NO._TruncExp.apply(NO._lin(h, p, "sigma_head"))
    geo = NO._lin(h, p, "geo_head")
    c = torch.cat([geo, dir_encode(x_d[..., 3:6].to(dtype), dir_mode, sh_levels)], -1)
    for j in range(color_depth):
        z = NO._lin(c, p, f"color_mlp.{j}.linear")
        pre.append(z)
        c = torch.relu(z)
    c = NO._lin(c, p, f"color_mlp.{color_depth}")
    out = torch.cat([torch.sigmoid(c) if sigmoid else c, sigma], -1)
    return (out, pre) if return_preacts else out


def kink_free_rows(preacts, margin, rows=None):
    """Indices of the rows whose every ReLU pre-activation has |z| >= margin.  A net without a ReLU layer has no
    pre-activations to tell the row count from: pass ``rows``, and every row is kept."""
    if not preacts and rows is None:
        raise ValueError("kink_free_rows: no ReLU layer, pass the row count as rows=")
    ok = torch.ones(preacts[0].shape[0] if preacts else rows, dtype=torch.bool)
    for z in preacts:
        if z.shape[-1]:
            ok &= (z.detach().abs() >= margin).all(dim=-1)
    return torch.nonzero(ok).reshape(-1)


def draw_case(cfg, M, seed, *, sigmoid=True, dirs=None, head_bias=None, sigma_up=1.0, margin=1e-4):
    """One seeded test case for configuration ``cfg`` (a Config), entirely on the CPU: nn.Linear-scale weights per
    named tensor (fp32), enc ~ U(-1, 1), unnormalised normal directions, an upstream gradient ~ N(0, 1) (its sigma
    column times ``sigma_up``), and the float64 reference of the forward and of every gradient.

    ReLU kinks are handled here, before any kernel runs: 2 M candidate rows are drawn and the first M whose float64
    pre-activations all have |z| >= margin are kept; fewer than M survivors is an AssertionError.
    dirs = "edges": candidate row i gets the direction 0 (i % 4 == 0), one of length 1e-12 (1) or 1e3 (2).
    head_bias: sigma_head.bias is set to it (saturated trunc_exp)."""
    g = torch.Generator().manual_seed(seed)
    dd = config_dir_dim(cfg)
    shapes = NO.ngp_param_shapes(cfg.in_dim, cfg.hidden, cfg.sigma_depth, cfg.geo, cfg.color_hidden, cfg.color_depth,
                                 dd)
    named, fan_in = {}, 1
    for name, shp in shapes.items():
        if len(shp) == 2:
            fan_in = shp[1]
        bound = 1.0 / fan_in ** 0.5
        named[name] = (torch.rand(shp, generator=g) * 2 - 1) * bound
    if head_bias is not None:
        named["sigma_head.bias"].fill_(head_bias)
    P = 2 * M
    enc = torch.rand(P, cfg.in_dim, generator=g) * 2 - 1
    d = torch.randn(P, 3, generator=g)
    if dirs == "edges":
        u = torch.nn.functional.normalize(d, dim=-1)
        i = torch.arange(P)
        d = torch.where((i % 4 == 0)[:, None], torch.zeros_like(d), d)
        d = torch.where((i % 4 == 1)[:, None], u * 1e-12, d)
        d = torch.where((i % 4 == 2)[:, None], u * 1e3, d)
    x_d = torch.cat([torch.rand(P, 3, generator=g), d], -1)
    kw = dict(sigma_depth=cfg.sigma_depth, color_depth=cfg.color_depth, dir_mode=cfg.dir_mode,
              sh_levels=cfg.sh_levels, sigmoid=sigmoid)
    with torch.no_grad():
        _, pre = mlp_reference(named, enc, x_d, return_preacts=True, **kw)
    keep = kink_free_rows(pre, margin, rows=P)
    assert keep.numel() >= M, f"only {keep.numel()} of {P} candidate rows are kink free, need {M}"
    survival = keep.numel() / max(P, 1)
    keep = keep[:M]
    enc, x_d = enc[keep].contiguous(), x_d[keep].contiguous()
    gup = torch.randn(M, 4, generator=g)
    gup[:, 3] *= sigma_up
    w64 = {k: v.double().requires_grad_(True) for k, v in named.items()}
    e64 = enc.double().requires_grad_(True)
    out = mlp_reference(w64, e64, x_d, **kw)
    gr = torch.autograd.grad((out * gup.double()).sum(), [e64] + list(w64.values()))
    case = dict(cfg=cfg, M=M, sigmoid=sigmoid, named=named, enc=enc, x_d=x_d, gup=gup, out=out.detach(),
                d_enc=gr[0], grads=dict(zip(w64, gr[1:])), survival=survival, kw=kw)
    return namedtuple("Case", case)(**case)
