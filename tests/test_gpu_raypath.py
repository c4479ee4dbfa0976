"""The ray-side kernels between the two MLP passes against the fp64 oracle (run on an MI355X: -m gpu).

Covered: csrc/composite.hip (forward, fused loss head, analytic backward), csrc/sample_pdf.hip and the stratified,
build_xd and freq_encode kernels of csrc/rays.hip, at the sizes where the code takes another path:
  composite   spl_for(S) picks SPL = 1, 2, 3, 4, 8, 16 samples per lane; S_GRID holds the first, the last and a ragged S
              of every instance, N_GRID the ray counts around the 16-ray forward block and the 4-ray backward block.
  sample_pdf  P = 1, 2, 4, 8 values per lane at S + n_imp <= 64, 128, 256, 512; the cdf scan runs in chunks of 64
              interior weights (B = S - 2) and hands a carry from chunk to chunk; S = 256 is the largest S.
  rays        256 threads per block over n*S (n*D) elements; linspace01 switches its evaluation at s = S / 2.

References: oracle/nerf_oracle.py called with fp64 tensors (gradients by autograd through it).  The inputs are fp32
values; the fp64 run sees exactly the same numbers.

Tolerance (compositing, loss head, stratified, build_xd, freq_encode): none is hard-coded.  Each case runs the same
oracle on the CPU in fp32, measures e_host = max |fp32 - fp64| per output family and allows the kernel
max(4 * e_host, 4 ulp at max |ref|) in the same norm.  The gradient is judged in two families, the rgb channels and
the sigma channel, each on its own scale.  Where the reference gradient is exactly zero by a clamp mask the kernel's
must be exactly zero.

sample_pdf: the fp32 oracle reproduces the kernel's rounding points (fp64 accumulation, cdf rounded once), so the
primary check is 4 ulp of max |t| (4 * 2^-23 * 8) against it on identical u.  The fp64 oracle is the independent
check: den < 1e-5 -> 1 is a true discontinuity, so every element must be within 1e-4 and 99.8 % within 1e-5;
test_pdf_fp32_oracle_meets_the_fp64_caps pins on the CPU that the fp32 oracle itself meets these caps on the same
inputs.  det=True draws u = linspace(0, 1, n_imp) evaluated from both ends (linspace01); the upper half 1 - step * k
may or may not be contracted to one fma by the compiler, so the test accepts the oracle on either of the two u
(the build measured below contracts it).  A fourth mode, "tie", plants u on entries of the fp32 cdf (exact ties of
searchsorted(right=True)); a tie exists only in fp32, so that mode is held to the fp32 oracle alone.

Two places where a correct kernel cannot meet 4 x e_host of the CPU's fp32 run, and what the tests do there:
  exp, S > 256 (SPL 8 and 16).  T is a product of S values of expf.  On the probe's 12541 arguments in (-0.02, 0) the
    device's expf had a mean error of -0.10 ulp (sigma 0.29, worst 0.64), the CPU's 0.00 ulp (sigma 0.29, worst
    0.55): both good to an ulp, but over S factors the device's mean error adds up to S * 0.1 ulp while the CPU's
    grows like sqrt(S).  At S = 1000 the kernel's depth was 6.5e-6 from fp64, the CPU's fp32 oracle 1.2e-6, and the
    same CPU oracle with exp alone taken from the device (torch.exp on the GPU) 5.8e-6, 1.2e-6 from the kernel.  So
    for S > 256 e_host is measured on that oracle (_host_exp); up to S = 256 it stays the CPU's.
  e_i - Q_i in the backward, on the ray that is transparent up to its opaque last sample: d sigma_i there is
    delta_i (e_i - 0.9999999 e_{S-1}) with both dL/dw of size 10 and rounded in fp32 before they cancel, next to a
    largest gradient of 1.7.  A CPU evaluation of the kernel's formula in plain fp32 gives the kernel's figures to
    all printed digits (7.714e-07 at S = 2, 1.968e-07 at S = 193) where autograd's order happened to give 6.1e-08 and
    3.4e-08.  On that ray alone the 4 ulp are counted at the size of the operands (_sigma_operands).

Measured on an MI355X (worst kernel error against fp64 per family; e_host of the same cases; "used" = the largest
err / allowed of any case, 1.00 is the limit):
  forward, SPL 1-4 (S <= 256)   rgb 1.9e-7 (e_host up to 1.8e-7), depth 8.2e-7 (4.9e-7), weights 6.8e-8 (6.7e-8),
                                acc 2.7e-7 (1.5e-7); used at most 0.79 (depth, S = 256, n = 4)
  forward, SPL 8 (257..512)     rgb 5.0e-7 (4.4e-7), depth 2.6e-6 (2.2e-6), weights 7.0e-8, acc 7.9e-7 (6.7e-7); used
                                at most 0.93 (depth, S = 511, n = 1: e_host 6.5e-8, the 4 ulp floor decides)
  forward, SPL 16 (513..1024)   rgb 1.7e-6 (1.8e-6), depth 1.1e-5 (1.1e-5), weights 1.2e-7, acc 3.1e-6 (3.2e-6); used
                                at most 0.58
  backward, rgb channels        1.4e-8 .. 2.4e-7 on max |ref| 1 .. 3, equal to e_host in most cases; used at most 0.38
  backward, sigma channel       SPL 1: up to 2.2e-6 (S = 2, 3 where sigma delta is large; e_host the same); SPL 2-4: up
                                to 3.0e-7; SPL 8: 2.8e-7; SPL 16: 1.1e-6 (e_host 1.2e-6); used at most 1.00 (S = 192,
                                n = 17, all gradients, scale 0.7: 6.326e-8 of 6.351e-8 allowed), next 0.83
  d bg through autograd         4.2e-8 .. 6.9e-6 (e_host 7.4e-6), used at most 0.69
  loss head                     loss_sum 1.3e-7 (e_host 1.1e-7) on 0.75 + loss, d_rgb 2.2e-7 (2.3e-7, srgb); used
                                at most 0.46
  stratified (u given)          8.7e-7, equal to e_host in every case; counter RNG at most 0.92 ulp outside its stratum
  build_xd                      5.2e-7 (e_host 9.4e-7); freq_encode 6.6e-8 (3.6e-8), used at most 0.28
  sample_pdf                    at most 4.8e-7 (one ulp of t) from the fp32 oracle in all 66 cases; against fp64 at
                                worst 9.1e-5 and 99.968 % within 1e-5, the fp32 oracle's own figures on the CPU
  sample_pdf counter RNG        mean - 1/2 within 0.8 sigma, variance - 1/12 within 2.1 sigma; one-hot: 99.73 % inside
                                the hot bin (99.49 % required)
The whole module takes 4 s.

Found by test_ray_kernels_accept_an_empty_batch and test_sample_pdf_arguments: nerf_sample_pdf, nerf_sample_stratified,
nerf_build_xd, nerf_freq_encode, nerf_clamp_near_far and nerf_rays_ndc refused an empty batch (torch gives an empty
tensor a NULL pointer and they looked at the pointers first); found by test_freq_encode[*-0-False]: nerf_freq_encode
refused L = 0 without the input columns, an output with no element, for the same reason.
"""
import contextlib
import functools
import itertools
import math
from collections import Counter
from types import SimpleNamespace
from unittest import mock

import pytest
import torch

from oracle import nerf_oracle as O

gpu = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
MARGIN = 4.0


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


def _ulp(m):
    """Spacing of fp32 numbers at magnitude m."""
    return 2.0 ** (math.frexp(m)[1] - 24) if m > 0 else 2.0 ** -149


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _check(family, what, got, ref, host, operands=None):
    """got within max(4 e_host, 4 ulp at max |ref|) of the fp64 ref, in the max norm over the tensor; never from got
    itself.  ``operands`` (per element, from the fp64 reference): the magnitude of the operands of a cancelling
    subtraction behind that element; there the 4 ulp are counted at that magnitude where it is the larger."""
    got, host = got.detach().cpu().double(), host.detach().double()
    assert got.shape == ref.shape == host.shape, (family, what, got.shape, ref.shape)
    if ref.numel() == 0:
        return
    assert torch.isfinite(got).all(), f"{family} {what}: not finite"
    e_host = (host - ref).abs().max().item()
    mx = ref.abs().max().item()
    bound = MARGIN * max(e_host, _ulp(mx))
    diff = (got - ref).abs()
    err = diff.max().item()
    allowed = torch.full_like(ref, bound)
    if operands is not None:
        allowed = torch.maximum(allowed, MARGIN * 2.0 ** (torch.floor(torch.log2(operands.clamp_min(1e-30))) - 23))
    worst = (diff / allowed).max().item()
    print(f"RAYPATH {family} | {what} | err {err:.3e} host {e_host:.3e} bound {bound:.3e} max|ref| {mx:.3e} "
          f"used {worst:.2f}")
    assert worst <= 1.0, (f"{family} {what}: err {err:.3e}, {worst:.2f} x what is allowed (bound {bound:.3e}, "
                          f"e_host {e_host:.3e}, max|ref| {mx:.3e})")


@contextlib.contextmanager
def _host_exp(S, dtype=torch.float32):
    """What the fp32 host oracle uses for exp.  Up to S = 256: the CPU's.  Above (SPL 8 and 16): the device's expf,
    through torch.exp on the GPU, because T is a product of S values of exp and the two exp differ in their mean
    error (module docstring); every other operation of the host oracle stays on the CPU."""
    if S <= 256 or dtype != torch.float32:
        yield
        return
    cpu_exp = torch.exp

    def exp(x):
        return cpu_exp(x.to(DEV)).cpu() if x.dtype == torch.float32 and not x.is_cuda else cpu_exp(x)

    with mock.patch.object(torch, "exp", exp):
        yield


# ================================================================== 1 / 2. compositing

S_GRID = [2, 3, 63, 64, 65, 128, 129, 192, 193, 256, 257, 511, 512, 513, 1000, 1024]
S_PER_SPL = [3, 65, 192, 256, 511, 1000]  # one S of every composite_*_kernel<SPL>: SPL 1, 2, 3, 4, 8, 16
N_GRID = [1, 3, 4, 5, 15, 16, 17, 33]
N_DEFAULT = 19


def _spl(S):
    need = (S + 63) // 64
    return next(k for k in (1, 2, 3, 4, 8, 16) if need <= k)


def test_grid_covers_every_template_instance():
    assert sorted({_spl(S) for S in S_PER_SPL}) == [1, 2, 3, 4, 8, 16]
    for spl in (1, 2, 3, 4, 8, 16):
        ss = [S for S in S_GRID if _spl(S) == spl]
        assert max(ss) == 64 * spl and any(S % 64 for S in ss), spl


@functools.lru_cache(maxsize=None)
def _comp_case(S, n, with_bg, scale):
    """Inputs (fp32), the fp64 oracle and the fp32 host oracle of one compositing case; shared and never modified."""
    g = _gen(1, S, n, with_bg, scale * 10)
    t = torch.sort(torch.rand(n, S, generator=g) * 4 + 2, -1)[0]
    rs = torch.empty(n, S, 4)
    rs[..., :3] = torch.rand(n, S, 3, generator=g) * 1.4 - 0.2
    rs[..., 3] = (torch.rand(n, S, generator=g) * 3.0 - 0.5) * (256.0 / S)
    # special rays 1..6 (ray 0 is always a plain random ray)
    if n > 1:
        rs[1, :, 3] = 0.0                      # transparent
    if n > 2:
        rs[2, :, 3] = 1e5                      # alpha clamp at 1 - 1e-7, T underflow
    if n > 3:
        j = (S - 1) // 2
        t[3, j + 1] = t[3, j]                  # two equal neighbours: delta clamp at 1e-4
    if n > 4:
        t[4, S - 1] = t[4, S - 2]              # last two equal: the copied last interval is the clamp
    if n > 5:
        rs[5, :, 3] = 0.0
        rs[5, S - 1, 3] = 1e5                  # opaque only in its last sample
    if n > 6:
        rs[6, :, 3] = 0.0
        rs[6, 0, 3] = 1e5                      # opaque only in its first sample
    bg = torch.rand(n, 3, generator=g) if with_bg else None
    ref = O.volume_render(rs.double(), t.double(), None if bg is None else bg.double(), scale)
    with _host_exp(S):
        host = O.volume_render(rs, t, bg, scale)
    return SimpleNamespace(S=S, n=n, scale=scale, t=t, rs=rs, bg=bg, ref=ref, host=host,
                           what=f"S={S} n={n} bg={int(with_bg)} scale={scale}")


def _alt(i):
    """bg on/off and sigma_scale alternate over the ray-count grid."""
    return bool(i % 2), (1.0, 0.7)[(i // 2) % 2]


FWD_CASES = ([(S, N_DEFAULT, bg, sc) for S in S_GRID for bg in (False, True) for sc in (1.0, 0.7)]
             + [(S, n, *_alt(i)) for S in S_PER_SPL for i, n in enumerate(N_GRID)])


def _on(x):
    return None if x is None else x.to(DEV)


@gpu
@pytest.mark.parametrize("S,n,with_bg,scale", FWD_CASES)
def test_composite_forward(K, S, n, with_bg, scale):
    c = _comp_case(S, n, with_bg, scale)
    out = K.composite_fwd(c.rs.to(DEV), c.t.to(DEV), _on(c.bg), scale)
    for name, a, r, h in zip(("rgb", "depth", "weights", "acc"), out, c.ref, c.host):
        _check(f"fwd {name} SPL{_spl(S)}", c.what, a, r, h)


FLAGS_ALL = list(itertools.product((False, True), repeat=3))
BWD_CASES = ([(S, N_DEFAULT, bg, sc, fl) for S in S_GRID for bg in (False, True) for sc in (1.0, 0.7)
              for fl in (FLAGS_ALL if S in S_PER_SPL else [(False,) * 3, (True,) * 3])]
             + [(S, n, *_alt(i), (True,) * 3) for S in S_PER_SPL for i, n in enumerate(N_GRID)])


def _upstream(c):
    g = _gen(2, c.S, c.n)
    return (torch.randn(c.n, 3, generator=g), torch.randn(c.n, generator=g), torch.randn(c.n, generator=g),
            torch.randn(c.n, c.S, generator=g) * 0.1)


def _oracle_grad(c, up, flags, dtype, want_bg=False):
    """d/d rgb_sigma (and d/d bg) of sum(rgb g_rgb) [+ sum(depth g_depth)] [+ sum(acc g_acc)] [+ sum(w g_w)]."""
    rs = c.rs.to(dtype).clone().requires_grad_(True)
    bg = None if c.bg is None else c.bg.to(dtype).clone().requires_grad_(want_bg)
    g_rgb, g_d, g_a, g_w = (x.to(dtype) for x in up)
    with _host_exp(c.S, dtype):
        rgb, depth, w, acc = O.volume_render(rs, c.t.to(dtype), bg, c.scale)
        L = (rgb * g_rgb).sum()
        if flags[0]:
            L = L + (depth * g_d).sum()
        if flags[1]:
            L = L + (acc * g_a).sum()
        if flags[2]:
            L = L + (w * g_w).sum()
        return torch.autograd.grad(L, [rs, bg] if want_bg else [rs])


def _sigma_operands(c, up, flags):
    """d sigma_i = scale delta_i e_s,i T_i (e_i - Q_i) with e_i = dL/dw_i and Q_i = sum_{k>i} e_k alpha_k prod f_j, a
    convex mean of the later e_k (times at most 1).  Returns scale delta e_s T (|e_i| + max_{k>i} |e_k|) in fp64: the
    size of what that subtraction cancels.  On the ray that is transparent up to its opaque last sample it leaves
    e_i - e_{S-1} of two dL/dw of size 10, each rounded in fp32, where the largest gradient of the case is below 2."""
    rs, t = c.rs.double(), c.t.double()
    delta = (t[:, 1:] - t[:, :-1]).clamp_min(1e-4)
    delta = torch.cat([delta, delta[:, -1:]], 1)
    e_s = torch.exp(-rs[..., 3].clamp_min(0.0) * c.scale * delta)
    f = 1.0 - (1.0 - e_s).clamp(0.0, 1.0 - 1e-7) + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(f[:, :1]), f], 1), 1)[:, :-1]
    g_rgb, g_d, g_a, g_w = (x.double() for x in up)
    e = (rs[..., :3].clamp(0.0, 1.0) * g_rgb[:, None, :]).sum(-1)
    if flags[0]:
        e = e + g_d[:, None] * t
    ga = g_a if flags[1] else torch.zeros_like(g_a)
    if c.bg is not None:
        ga = ga - (g_rgb * c.bg.double()).sum(-1)
    e = (e + ga[:, None] + (g_w if flags[2] else 0.0)).abs()
    later = torch.cummax(e.flip(1), 1)[0].flip(1)
    later = torch.cat([later[:, 1:], torch.zeros_like(later[:, :1])], 1)
    ops = c.scale * delta * e_s * T * (e + later)
    ops[torch.arange(c.n) != 5] = 0.0  # only the ray built to cancel: transparent up to its opaque last sample
    return ops


def _check_grad(c, d, ref, host, what, up, flags):
    """rgb channels and sigma channel each on its own scale, then the exact zeros of the clamp masks."""
    d = d.detach().cpu().view(c.n, c.S, 4)
    _check(f"bwd d_rgb SPL{_spl(c.S)}", what, d[..., :3], ref[..., :3], host[..., :3])
    _check(f"bwd d_sigma SPL{_spl(c.S)}", what, d[..., 3], ref[..., 3], host[..., 3], _sigma_operands(c, up, flags))
    out_rgb = (c.rs[..., :3] < 0) | (c.rs[..., :3] > 1)
    neg = c.rs[..., 3] < 0
    delta = (c.t[:, 1:] - c.t[:, :-1]).double().clamp_min(1e-4)
    delta = torch.cat([delta, delta[:, -1:]], 1)
    sat = c.rs[..., 3].double().clamp_min(0) * c.scale * delta >= 20.0  # exp(-20) = 2e-9: clamped in fp32 and fp64
    assert c.n * c.S < 64 or (out_rgb.any() and neg.any() and (sat.any() or c.n < 3))
    for mask, got_ch, ref_ch, name in ((out_rgb, d[..., :3], ref[..., :3], "rgb outside [0, 1]"),
                                       (neg, d[..., 3], ref[..., 3], "sigma < 0"),
                                       (sat, d[..., 3], ref[..., 3], "alpha at its clamp")):
        assert not ref_ch[mask].any(), f"{what}: the reference gradient is not zero where {name}"
        assert not got_ch[mask].any(), f"{what}: gradient not exactly zero where {name}"


@gpu
@pytest.mark.parametrize("S,n,with_bg,scale,flags", BWD_CASES)
def test_composite_backward(K, S, n, with_bg, scale, flags):
    c = _comp_case(S, n, with_bg, scale)
    up = _upstream(c)
    ref, = _oracle_grad(c, up, flags, F64)
    host, = _oracle_grad(c, up, flags, torch.float32)
    opt = [_on(x) if f else None for x, f in zip(up[1:], flags)]
    d = K.composite_bwd(c.rs.to(DEV), c.t.to(DEV), _on(c.bg), up[0].to(DEV), opt[0], opt[1], opt[2], scale)
    assert d.shape == c.rs.shape
    _check_grad(c, d, ref, host, f"{c.what} g_depth={int(flags[0])} g_acc={int(flags[1])} g_w={int(flags[2])}", up,
                flags)


@gpu
@pytest.mark.parametrize("S", S_PER_SPL)
def test_volume_render_autograd(K, S):
    """ray_rendering.volume_render end to end: VolumeRenderFn's argument order, d rgb_sigma and d bg."""
    from nerf_amd.ray_rendering import volume_render
    c = _comp_case(S, N_DEFAULT, True, 0.7)
    up = _upstream(c)
    ref = _oracle_grad(c, up, (True,) * 3, F64, want_bg=True)
    host = _oracle_grad(c, up, (True,) * 3, torch.float32, want_bg=True)
    rs = c.rs.to(DEV).requires_grad_(True)
    bg = c.bg.to(DEV).requires_grad_(True)
    out = volume_render(rs, c.t.to(DEV), bg, sigma_scale=0.7)
    for name, a, r, h in zip(("rgb", "depth", "weights", "acc"), out, c.ref, c.host):
        _check(f"fwd {name} SPL{_spl(S)}", f"autograd {c.what}", a, r, h)
    g = [x.to(DEV) for x in up]
    L = (out[0] * g[0]).sum() + (out[1] * g[1]).sum() + (out[3] * g[2]).sum() + (out[2] * g[3]).sum()
    d_rs, d_bg = torch.autograd.grad(L, [rs, bg])
    _check_grad(c, d_rs, ref[0], host[0], f"autograd {c.what}", up, (True,) * 3)
    _check("bwd d_bg", f"autograd {c.what}", d_bg, ref[1], host[1])


# ================================================================== 3. fused loss head

LOSS_N = [1, 15, 16, 17, 33]
LOSS_S = [64, 300]
LOSS_IN = 0.75  # what loss_sum holds before the call


@functools.lru_cache(maxsize=None)
def _loss_inputs(S, n):
    g = _gen(3, S, n)
    t = torch.sort(torch.rand(n, S, generator=g) * 4 + 2, -1)[0]
    rs = torch.empty(n, S, 4)
    rs[..., :3] = torch.rand(n, S, 3, generator=g) * 1.4 - 0.2
    rs[..., 3] = (torch.rand(n, S, generator=g) * 3.0 - 0.5) * (64.0 / S)
    bg = torch.rand(n, 3, generator=g) * 2.2 - 0.6   # shifts rgb_map out of [0, 1] on the less opaque rays
    gt = torch.rand(n, 3, generator=g) * 1.2 - 0.1
    gt[0] = torch.tensor([0.03, 0.05, 0.6])           # both sides of the 0.04045 knee
    if n > 2:  # two transparent rays: rgb_map = bg exactly, on both sides of the 0.0031308 knee and outside [0, 1]
        rs[1, :, 3] = 0.0
        rs[2, :, 3] = -0.25
        bg[1] = torch.tensor([0.002, 0.004, 0.5])
        bg[2] = torch.tensor([-0.3, 1.4, 0.0031])
        gt[1] = torch.tensor([0.0404, 0.0405, 0.5])
        gt[2] = torch.tensor([0.2, 0.9, -0.05])
    inv_count = torch.tensor(1.0 / (3 * (2 * n + 1)), dtype=torch.float32).item()  # as if n were part of a batch
    return SimpleNamespace(S=S, n=n, t=t, rs=rs, bg=bg, gt=gt, inv_count=inv_count)


def _loss_oracle(c, cs, dtype):
    with _host_exp(c.S, dtype):
        rgb = O.volume_render(c.rs.to(dtype), c.t.to(dtype), c.bg.to(dtype))[0].detach().requires_grad_(True)
    loss = O.mse_loss(rgb, c.gt.to(dtype), cs)
    g, = torch.autograd.grad(loss, rgb)
    k = torch.tensor(3 * c.n * c.inv_count, dtype=dtype)
    return (torch.tensor(LOSS_IN, dtype=dtype) + loss.detach() * k).reshape(1), g * k, rgb.detach()


@gpu
@pytest.mark.parametrize("cs", ["linear", "srgb", "identity"])
@pytest.mark.parametrize("n", LOSS_N)
@pytest.mark.parametrize("S", LOSS_S)
def test_composite_loss_head(K, S, n, cs):
    c = _loss_inputs(S, n)
    ref, host = _loss_oracle(c, cs, F64), _loss_oracle(c, cs, torch.float32)
    p = ref[2]
    if n > 2:  # the premises: both dp branches and both sides of both knees are live
        assert (p < -1e-3).any() and (p > 1 + 1e-3).any() and ((p > 1e-3) & (p < 1 - 1e-3)).any()
        assert ((p > 0) & (p < 0.0031308)).any() and (c.gt.clamp(0, 1) < 0.04045).any()
    loss_sum = torch.full((1,), LOSS_IN, device=DEV)
    out = K.composite_fwd(c.rs.to(DEV), c.t.to(DEV), c.bg.to(DEV), gt=c.gt.to(DEV), color_space=cs,
                          inv_count=c.inv_count, loss_sum=loss_sum)
    assert out[4] is loss_sum
    what = f"S={S} n={n} {cs}"
    _check("loss rgb", what, out[0], ref[2], host[2])
    _check(f"loss loss_sum {cs}", what, out[4], ref[0], host[0])
    _check(f"loss d_rgb {cs}", what, out[5], ref[1], host[1])
    if cs != "identity":
        outside = (p < -1e-5) | (p > 1 + 1e-5)
        assert not ref[1][outside].any() and not out[5].cpu()[outside].any(), "d_rgb not zero where rgb_map is clamped"


# ================================================================== 4. compositing arguments

def _sentinel(*shape):
    return torch.full(shape, 7.0, device=DEV)


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(bool((x == 7.0).all()) for x in ts)


@gpu
@pytest.mark.parametrize("S", [1, 1025])
def test_composite_refuses_S(K, S):
    n = 3
    rs, t = torch.rand(n, S, 4, device=DEV), torch.rand(n, S, device=DEV).sort(-1)[0]
    outs = (_sentinel(n, 3), _sentinel(n), _sentinel(n, S), _sentinel(n))
    with pytest.raises(ValueError, match="nerf_composite_fwd"):
        K.composite_fwd(rs, t, outs=outs)
    d = _sentinel(n, S, 4)
    with pytest.raises(ValueError, match="nerf_composite_bwd"):
        K.composite_bwd(rs, t, None, torch.ones(n, 3, device=DEV), out=d)
    assert _untouched(d, *outs)


@gpu
def test_composite_refuses_misaligned(K):
    n, S = 3, 5
    buf = torch.rand(n * S * 4 + 4, device=DEV)
    rs = buf[1:1 + n * S * 4].view(n, S, 4)
    assert rs.is_contiguous() and rs.data_ptr() % 16 == 4
    t = torch.rand(n, S, device=DEV).sort(-1)[0]
    outs = (_sentinel(n, 3), _sentinel(n), _sentinel(n, S), _sentinel(n))
    with pytest.raises(RuntimeError, match="aligned"):
        K.composite_fwd(rs, t, outs=outs)
    d = _sentinel(n, S, 4)
    with pytest.raises(RuntimeError, match="aligned"):
        K.composite_bwd(rs, t, None, torch.ones(n, 3, device=DEV), out=d)
    dbuf = _sentinel(n * S * 4 + 4)
    with pytest.raises(RuntimeError, match="aligned"):  # an aligned input with a misaligned gradient buffer
        K.composite_bwd(buf[:n * S * 4].view(n, S, 4), t, None, torch.ones(n, 3, device=DEV),
                        out=dbuf[1:1 + n * S * 4].view(n, S, 4))
    assert _untouched(d, dbuf, *outs)


@gpu
def test_composite_refuses_loss_arguments(K):
    from nerf_amd._lib import lib, ptr, stream
    n, S = 3, 5
    rs, t = torch.rand(n, S, 4, device=DEV), torch.rand(n, S, device=DEV).sort(-1)[0]
    gt = torch.rand(n, 3, device=DEV)
    outs = (_sentinel(n, 3), _sentinel(n), _sentinel(n, S), _sentinel(n))
    loss = _sentinel(1)
    with pytest.raises(ValueError, match="color_space"):
        K.composite_fwd(rs, t, gt=gt, color_space="xyz", loss_sum=loss, outs=outs)

    def raw(cs, loss_sum, d_rgb):
        return lib().nerf_composite_fwd(ptr(rs), ptr(t), None, n, S, 1.0, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                        ptr(outs[3]), ptr(gt), cs, 1.0, ptr(loss_sum), ptr(d_rgb), stream())

    d_rgb = _sentinel(n, 3)
    assert raw(3, loss, d_rgb) == -3 and raw(-1, loss, d_rgb) == -3   # NERF_E_ENUM
    assert raw(0, loss, None) == -1 and raw(0, None, d_rgb) == -1     # gt without room for d_rgb / the sum
    assert _untouched(loss, d_rgb, *outs)
    assert raw(0, loss, d_rgb) == 0                                    # the well-formed call goes through
    assert not _untouched(loss) and not _untouched(d_rgb)


@gpu
def test_composite_empty_batch(K):
    from nerf_amd.ray_rendering import volume_render
    S = 5
    rs, t = torch.zeros(0, S, 4, device=DEV), torch.zeros(0, S, device=DEV)
    shapes = [(0, 3), (0,), (0, S), (0,)]
    assert [tuple(x.shape) for x in K.composite_fwd(rs, t)] == shapes
    loss = torch.full((1,), LOSS_IN, device=DEV)
    out = K.composite_fwd(rs, t, torch.zeros(0, 3, device=DEV), gt=torch.zeros(0, 3, device=DEV), loss_sum=loss,
                          inv_count=1.0)
    assert [tuple(x.shape) for x in out[:4]] == shapes and out[5].shape == (0, 3) and out[4].item() == LOSS_IN
    assert K.composite_bwd(rs, t, None, torch.zeros(0, 3, device=DEV)).shape == (0, S, 4)
    rsg = rs.clone().requires_grad_(True)
    res = volume_render(rsg, t, torch.zeros(0, 3, device=DEV))
    g, = torch.autograd.grad(res[0].sum() + res[2].sum(), rsg)
    assert g.shape == (0, S, 4)


# ================================================================== 5. sample_pdf

PDF_PAIRS = [(3, 1), (3, 61), (3, 62), (34, 30), (64, 64), (65, 63), (66, 62), (66, 190), (67, 189), (128, 128),
             (130, 126), (130, 127), (194, 62), (256, 1), (256, 256), (64, 128), (66, 63)]
PDF_MODES = ["u", "det", "edge"]
PDF_N = 37
# (S, n_imp) -> seed offset, for the pairs whose fp32 oracle broke the fp64 caps on the CPU at offset 0 (the first
# offset that passes test_pdf_fp32_oracle_meets_the_fp64_caps in all modes).  What breaks them is the top of the cdf:
# u = 1 (det) or 1 - 2^-24 (edge) on a ray whose last bin is below the den < 1e-5 rule lands on edge[S-2] or one bin
# lower according to the last bit of cdf[S-2], in fp32 and in fp64 alike.
PDF_SEED = {(34, 30): 2, (64, 64): 5, (65, 63): 2, (66, 62): 10, (66, 190): 10, (67, 189): 4, (128, 128): 30,
            (130, 126): 3, (130, 127): 1, (194, 62): 29, (256, 256): 25, (66, 63): 21}
PDF_TOL32 = 4 * 2.0 ** -23 * 8
U_MAX = 1.0 - 2.0 ** -24  # the largest float below 1


def test_pdf_pairs_sit_on_the_thresholds():
    tot = {S + n for S, n in PDF_PAIRS}
    assert {64, 65, 128, 129, 256, 257, 512} <= tot
    B = {S - 2 for S, _ in PDF_PAIRS}
    assert {1, 62, 63, 64, 65, 128, 192, 254} <= B and max(S for S, _ in PDF_PAIRS) == 256


def _linspace01(n, fused):
    """csrc linspace01 on the host: step * s below the middle, 1 - step * (n - 1 - s) from it on; ``fused`` rounds
    the upper half once (the product kept exact, as one fma does) instead of twice."""
    if n == 1:
        return torch.zeros(1)
    step = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n - 1), dtype=torch.float32)
    s = torch.arange(n, dtype=torch.float32)
    back = (n - 1) - s
    hi = (1.0 - step.double() * back.double()).float() if fused else 1.0 - step * back
    return torch.where(torch.arange(n) < n // 2, step * s, hi)


def _cdf32(t, w):
    """The cdf of the fp32 oracle (oracle.sample_pdf's first lines): where a u may tie with an entry."""
    ww = w[:, 1:-1] + 1e-5
    pdf = ww / ww.double().sum(-1, keepdim=True).float()
    return torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)


@functools.lru_cache(maxsize=None)
def _pdf_case(S, n_imp, mode):
    n, B = PDF_N, S - 2
    g = _gen(5, S, n_imp, PDF_SEED.get((S, n_imp), 0))
    t = torch.sort(torch.rand(n, S, generator=g) * 4 + 2, -1)[0]
    w = torch.rand(n, S, generator=g) ** 4
    w[0] = 0.0                                   # all zero: a uniform pdf of 1e-5 floors
    w[1] = 0.0
    w[1, 1 + B // 2] = 0.5 + torch.rand(1, generator=g).item()   # one-hot
    w[2, :1 + B // 2] = 0.0                      # first half zero
    w[3] = 0.0
    w[3, S - 2] = 1.0                            # all mass in the last interior bin
    u = None
    if mode != "det":
        u = torch.rand(n, n_imp, generator=g)
    if mode in ("edge", "tie"):
        if n_imp == 1:
            u[0::2, 0], u[1::2, 0] = 0.0, U_MAX
        else:
            u[:, 0], u[:, -1] = 0.0, U_MAX
    if mode == "tie":  # u equal to cdf entries: searchsorted(right=True) must step over them
        cdf = _cdf32(t, w)
        NC = S - 1
        u[:, 1] = cdf[:, max(1, NC // 4)]
        u[:, 2] = cdf[:, NC - 1]
        u[:, 3] = cdf[:, NC // 2]
    if mode == "det":
        us = [_linspace01(n_imp, f).expand(n, n_imp).contiguous() for f in (False, True)]
    else:
        us = [u]
    r32 = [O.hierarchical_t_vals(t, w, n_imp, u=x) for x in us]
    r64 = [O.hierarchical_t_vals(t.double(), w.double(), n_imp, u=x.double()) for x in us]
    return SimpleNamespace(S=S, n_imp=n_imp, t=t, w=w, u=u, det=mode == "det", r32=r32, r64=r64)


def _caps64(x, r64):
    d = (x.double() - r64).abs()
    return d.max().item(), (d <= 1e-5).double().mean().item()


@pytest.mark.parametrize("mode", PDF_MODES)
@pytest.mark.parametrize("S,n_imp", PDF_PAIRS)
def test_pdf_fp32_oracle_meets_the_fp64_caps(S, n_imp, mode):
    """CPU only, the premise of the fp64 check below: on these inputs the fp32 oracle itself stays within 1e-4 of
    the fp64 oracle everywhere and within 1e-5 on 99.8 % of the elements."""
    c = _pdf_case(S, n_imp, mode)
    for a, b in zip(c.r32, c.r64):
        worst, frac = _caps64(a, b)
        print(f"RAYPATH pdf premise | S={S} n_imp={n_imp} {mode} | worst {worst:.3e} within1e-5 {frac:.5f}")
        assert worst <= 1e-4 and frac >= 0.998, (worst, frac)


def _fine_rows(out, t):
    """Per row the multiset difference out - t on the bit patterns; every coarse t must be in out bitwise."""
    ob, tb = out.contiguous().view(torch.int32).tolist(), t.contiguous().view(torch.int32).tolist()
    fine = []
    for r, (orow, trow) in enumerate(zip(ob, tb)):
        have, want = Counter(orow), Counter(trow)
        assert not (want - have), f"row {r}: a coarse t is missing from the merged output"
        fine.append(torch.tensor(sorted((have - want).elements()), dtype=torch.int32).view(torch.float32))
    return fine


def _pdf_properties(out, t, n_imp):
    assert out.shape == (t.shape[0], t.shape[1] + n_imp) and torch.isfinite(out).all()
    assert (out[:, 1:] >= out[:, :-1]).all(), "a row is not sorted"
    assert (out >= t[:, :1]).all() and (out <= t[:, -1:]).all(), "a sample left [t_0, t_{S-1}]"
    fine = _fine_rows(out, t)
    assert all(f.numel() == n_imp for f in fine)
    return fine


def _run_pdf(K, c, **kw):
    return K.sample_pdf(c.t.to(DEV), c.w.to(DEV), c.n_imp, u=_on(c.u), det=c.det, **kw).cpu()


@gpu
@pytest.mark.parametrize("S,n_imp,mode", [(S, n, m) for S, n in PDF_PAIRS for m in PDF_MODES + ["tie"]
                                          if m != "tie" or n >= 4])
def test_sample_pdf_vs_oracle(K, S, n_imp, mode):
    c = _pdf_case(S, n_imp, mode)
    out = _run_pdf(K, c)
    _pdf_properties(out, c.t, n_imp)
    errs = [(out.double() - r.double()).abs().max().item() for r in c.r32]
    k = min(range(len(errs)), key=errs.__getitem__)
    print(f"RAYPATH pdf fp32 oracle | S={S} n_imp={n_imp} {mode} | err {errs[k]:.3e} tol {PDF_TOL32:.3e}"
          + (f" (u = linspace01 {'fused' if k else 'plain'}; other {errs[1 - k]:.3e})" if c.det else ""))
    assert errs[k] <= PDF_TOL32, (errs, PDF_TOL32)
    if mode == "tie":
        return  # a u on a cdf entry is a tie only in fp32: the fp64 oracle may sit one bin away
    worst, frac = _caps64(out, c.r64[k])
    print(f"RAYPATH pdf fp64 oracle | S={S} n_imp={n_imp} {mode} | worst {worst:.3e} within1e-5 {frac:.5f}")
    assert worst <= 1e-4 and frac >= 0.998, (worst, frac)


@gpu
@pytest.mark.parametrize("S,n_imp", [(3, 62), (66, 190), (256, 256)])
def test_sample_pdf_rng_is_a_function_of_seed_and_ray(K, S, n_imp):
    """u=None, det=False: the trainer's path.  Same rows for every ray, so rays differ only through the RNG."""
    n = PDF_N
    t = torch.linspace(2.0, 6.0, S).expand(n, S).contiguous()
    w = (torch.rand(1, S, generator=_gen(6, S)) ** 2).expand(n, S).contiguous()
    a, b, c = (K.sample_pdf(t.to(DEV), w.to(DEV), n_imp, seed=s).cpu() for s in (11, 11, 12))
    fa, fc = _pdf_properties(a, t, n_imp), _pdf_properties(c, t, n_imp)
    assert _bits(a, b), "the same seed gave other bits"
    assert all(not torch.equal(x, y) for x, y in zip(fa, fc)), "another seed gave the same samples on a ray"
    assert all(not torch.equal(fa[i], fa[j]) for i in range(n) for j in range(i)), "two rays drew the same samples"


@gpu
@pytest.mark.parametrize("S,n_imp,n", [(64, 128, 37), (256, 256, 19), (130, 126, 38)])
def test_sample_pdf_rng_is_uniform(K, S, n_imp, n):
    """linspace t and equal weights: the inverse cdf is the straight line from mid_0 to mid_{S-2}, so the fine
    samples rescaled to [0, 1] are the u themselves.  For N = n * n_imp independent U(0, 1): the mean has sigma
    sqrt(1 / (12 N)); mean((u - 1/2)^2) has mean 1/12 and variance (1/80 - 1/144) / N, sigma = sqrt(1 / (180 N))."""
    t = torch.linspace(2.0, 6.0, S).expand(n, S).contiguous()
    w = torch.ones(n, S)
    out = K.sample_pdf(t.to(DEV), w.to(DEV), n_imp, seed=2024).cpu()
    fine = torch.cat(_pdf_properties(out, t, n_imp)).double()
    mids = 0.5 * (t[0, 1:] + t[0, :-1]).double()
    v = (fine - mids[0]) / (mids[-1] - mids[0])
    N = n * n_imp
    assert v.numel() == N and v.min() >= -1e-6 and v.max() <= 1 + 1e-6
    s_mean, s_var = math.sqrt(1.0 / (12 * N)), math.sqrt(1.0 / (180 * N))
    mean, var = v.mean().item(), ((v - 0.5) ** 2).mean().item()
    print(f"RAYPATH pdf rng | S={S} n_imp={n_imp} N={N} | mean-1/2 {mean - 0.5:+.2e} (sigma {s_mean:.2e}) "
          f"var-1/12 {var - 1 / 12:+.2e} (sigma {s_var:.2e})")
    assert abs(mean - 0.5) <= 5 * s_mean and abs(var - 1.0 / 12) <= 5 * s_var


@gpu
def test_sample_pdf_rng_follows_a_one_hot_pdf(K):
    """One weight of 1 among zeros: the other B - 1 bins hold 1e-5 / (1 + B 1e-5) each, so the expected fraction
    outside the hot bin is below B * 1e-5; N = 148 * 256 draws put its count (about 96) far above Poisson noise."""
    S, n_imp, n, k = 256, 256, 148, 100
    B = S - 2
    t = torch.sort(torch.rand(1, S, generator=_gen(7)) * 4 + 2, -1)[0].expand(n, S).contiguous()
    w = torch.zeros(n, S)
    w[:, k] = 1.0
    out = K.sample_pdf(t.to(DEV), w.to(DEV), n_imp, seed=5).cpu()
    fine = torch.cat(_pdf_properties(out, t, n_imp))
    mids = 0.5 * (t[0, 1:] + t[0, :-1])
    inside = ((fine >= mids[k - 1]) & (fine <= mids[k])).double().mean().item()
    print(f"RAYPATH pdf rng | one-hot S={S} | inside {inside:.6f} required {1 - 2 * B * 1e-5:.6f}")
    assert inside >= 1 - 2 * B * 1e-5
    assert inside < 1.0, "no sample at all outside the hot bin: the 1e-5 floor is gone"


@gpu
def test_sample_pdf_arguments(K):
    def call(S, n_imp, n=3):
        t = torch.rand(n, S, device=DEV).sort(-1)[0]
        return K.sample_pdf(t, torch.rand(n, S, device=DEV), n_imp, det=True)

    for S, n_imp in ((2, 4), (257, 4), (256, 257), (3, 510), (64, 0)):
        with pytest.raises(ValueError, match="nerf_sample_pdf"):
            call(S, n_imp)
    assert call(256, 256).shape == (3, 512)
    assert call(64, 32, n=0).shape == (0, 96)
    assert K.sample_pdf(torch.zeros(0, 5, device=DEV), torch.zeros(0, 5, device=DEV), 3, seed=1).shape == (0, 8)


# ================================================================== 6. stratified, build_xd, freq_encode

STRAT_S = [1, 2, 3, 64, 65, 192]
STRAT_N = [1, 255, 257]


@functools.lru_cache(maxsize=None)
def _rays(n):
    g = _gen(8, n)
    near = torch.rand(n, generator=g) * 2 + 0.5
    far = near + 1 + torch.rand(n, generator=g) * 4
    return torch.cat([torch.randn(n, 6, generator=g), near[:, None], far[:, None]], 1)


@gpu
@pytest.mark.parametrize("randomized", [False, True])
@pytest.mark.parametrize("n", STRAT_N)
@pytest.mark.parametrize("S", STRAT_S)
def test_stratified_vs_oracle(K, S, n, randomized):
    rays = _rays(n)
    u = torch.rand(n, S, generator=_gen(9, S, n)) if randomized else None
    if randomized:
        u[0, 0], u[-1, -1] = 0.0, U_MAX
    got = K.sample_stratified(rays.to(DEV), S, randomized, _on(u))
    ref = O.stratified_t_vals(rays[:, 6].double(), rays[:, 7].double(), S, randomized,
                              None if u is None else u.double())
    host = O.stratified_t_vals(rays[:, 6], rays[:, 7], S, randomized, u)
    _check("stratified", f"S={S} n={n} randomized={int(randomized)}", got, ref, host)
    if not randomized:
        got = got.cpu()
        assert _bits(got[:, 0], rays[:, 6]), "t_0 is not near"
        assert S == 1 or _bits(got[:, -1], rays[:, 7]), "t_{S-1} is not far"


@gpu
@pytest.mark.parametrize("S", STRAT_S)
def test_stratified_linspace_is_evaluated_from_both_ends(K, S):
    """near = 0, far = 1 returns linspace01 itself.  Its lower half is step * s, its upper half 1 - step * (S-1-s):
    0 and 1 exactly at the ends and, with step * k rounded (plain) or kept exact (one fma), the mirror image
    of the lower half.  An evaluation from the near end alone drifts off it (at 27 of 32 places at S = 64)."""
    rays = torch.zeros(3, 8)
    rays[:, 7] = 1.0
    got = K.sample_stratified(rays.to(DEV), S, False).cpu()
    assert _bits(got[0], got[1]) and _bits(got[1], got[2])
    tl = got[0]
    assert tl[0].item() == 0.0 and (S == 1 or tl[-1].item() == 1.0)
    assert S < 3 or (tl[1:] > tl[:-1]).all()
    cands = [_linspace01(S, f) for f in (False, True)]
    assert any(_bits(tl, c) for c in cands), (tl - cands[0]).abs().max().item()


@gpu
@pytest.mark.parametrize("n", STRAT_N)
@pytest.mark.parametrize("S", STRAT_S)
def test_stratified_rng_stays_in_its_stratum(K, S, n):
    rays = _rays(n)
    a, b, c = (K.sample_stratified(rays.to(DEV), S, True, None, seed=s).cpu() for s in (21, 21, 22))
    assert _bits(a, b), "the same seed gave other bits"
    t = O.stratified_t_vals(rays[:, 6].double(), rays[:, 7].double(), S, False)
    mids = 0.5 * (t[:, :-1] + t[:, 1:])
    low, high = torch.cat([t[:, :1], mids], 1), torch.cat([mids, t[:, -1:]], 1)
    ulp = 2.0 ** (torch.floor(torch.log2(high)) - 23)
    slack = torch.maximum((low - a.double()) / ulp, (a.double() - high) / ulp).max().item()
    print(f"RAYPATH stratified rng | S={S} n={n} | worst excursion {slack:+.2f} ulp (allowed 2)")
    assert slack <= 2.0
    if S > 1:
        assert not torch.equal(a, c), "another seed gave the same samples"
        uu = ((a.double() - low) / (high - low))[:, 1:-1] if S > 2 else None
        if uu is not None and uu.numel() >= 1000:  # U(0,1): the mean's sigma is sqrt(1 / (12 N))
            assert abs(uu.mean().item() - 0.5) <= 5 * math.sqrt(1.0 / (12 * uu.numel()))


XD_SHAPES = [(1, 1), (3, 5), (37, 65), (255, 3), (19, 257)]


@gpu
@pytest.mark.parametrize("n,S", XD_SHAPES)
def test_build_xd(K, n, S):
    assert (n * S) % 256
    rays = _rays(n)
    t = torch.sort(torch.rand(n, S, generator=_gen(10, n, S)) * 4 + 2, -1)[0]
    xd = K.build_xd(rays.to(DEV), t.to(DEV)).cpu()
    assert xd.shape == (n * S, 6)
    o, d = rays[:, None, :3], rays[:, None, 3:6]
    ref = (o.double() + d.double() * t.double()[..., None]).reshape(-1, 3)
    host = (o + d * t[..., None]).reshape(-1, 3)
    _check("build_xd", f"n={n} S={S}", xd[:, :3], ref, host)
    assert _bits(xd[:, 3:], d.expand(n, S, 3).reshape(-1, 3)), "the direction columns are not copies"


# n so that n * D lands on 1, 255 and 257 where D divides them, else on the nearest multiples on either side of 256
FREQ_N = {1: [1, 255, 257], 3: [1, 85, 86], 6: [1, 42, 43]}


@gpu
@pytest.mark.parametrize("inc", [True, False])
@pytest.mark.parametrize("L", [0, 1, 4, 10])
@pytest.mark.parametrize("D", [1, 3, 6])
def test_freq_encode(K, D, L, inc):
    for n in FREQ_N[D]:
        x = torch.rand(n, D, generator=_gen(11, n, D, L)) * 8 - 4
        x[0, 0] = 4.0
        got = K.freq_encode(x.to(DEV), L, inc).cpu()
        od = D * (2 * L + int(inc))
        assert got.shape == (n, od)
        if inc:
            assert _bits(got[:, :D], x), "the input columns are not copies"
        if L == 0:
            continue
        xe = x.double()[..., None] * 2.0 ** torch.arange(L, dtype=F64)   # exact in fp32 too
        assert torch.equal(xe.float().double(), xe)
        ref = torch.cat([torch.cos(xe), torch.sin(xe)], -1).reshape(n, -1)
        host = O.freq_encode(x, L, False)
        _check("freq_encode", f"D={D} L={L} inc={int(inc)} n={n}", got[:, D if inc else 0:], ref, host)


@gpu
def test_ray_kernels_accept_an_empty_batch(K):
    rays = torch.zeros(0, 8, device=DEV)
    for randomized in (False, True):
        assert K.sample_stratified(rays, 7, randomized, seed=3).shape == (0, 7)
    assert K.sample_stratified(rays, 7, True, torch.zeros(0, 7, device=DEV)).shape == (0, 7)
    assert K.build_xd(rays, torch.zeros(0, 7, device=DEV)).shape == (0, 6)
    assert K.freq_encode(torch.zeros(0, 3, device=DEV), 10).shape == (0, 63)
    assert K.freq_encode(torch.zeros(0, 5, 3, device=DEV), 4, False).shape == (0, 5, 24)
    r, valid = K.clamp_near_far(rays, 0.5, 4.0)
    assert r.shape == (0, 8) and valid.shape == (0,) and valid.dtype == torch.bool
    assert K.rays_ndc(rays, 8, 8, 10.0).shape == (0, 8)


@gpu
def test_ray_kernels_still_refuse_a_null_pointer(K):
    """n = 0 is answered before the pointers are looked at; with n > 0 a NULL buffer is still an error."""
    from nerf_amd._lib import lib, ptr, stream
    L, n, S = lib(), 3, 5
    rays, t = ptr(torch.zeros(n, 8, device=DEV)), ptr(torch.zeros(n, S, device=DEV))
    x, st = ptr(torch.zeros(n, 3, device=DEV)), stream()
    big = ptr(torch.zeros(n * S * 8, device=DEV))
    E_ARG = -1
    assert L.nerf_sample_stratified(None, n, S, 0, None, 0, big, st) == E_ARG
    assert L.nerf_sample_stratified(rays, n, S, 0, None, 0, None, st) == E_ARG
    assert L.nerf_build_xd(rays, None, n, S, big, st) == E_ARG and L.nerf_build_xd(rays, t, n, S, None, st) == E_ARG
    assert L.nerf_freq_encode(None, n, 3, 2, 1, big, 15, st) == E_ARG
    assert L.nerf_freq_encode(x, n, 3, 2, 1, None, 15, st) == E_ARG
    assert L.nerf_clamp_near_far(None, n, 1, 0.5, 1, 4.0, 1e-6, 0.0, None, st) == E_ARG
    assert L.nerf_rays_ndc(None, n, 8, 8, 10.0, 1.0, big, st) == E_ARG
    assert L.nerf_rays_ndc(rays, n, 8, 8, 10.0, 1.0, None, st) == E_ARG
    assert L.nerf_sample_pdf(None, t, n, S, 4, None, 1, 0, big, st) == E_ARG
    assert L.nerf_sample_pdf(t, t, n, S, 4, None, 1, 0, None, st) == E_ARG
    # the scalar checks come first, also for an empty batch
    assert L.nerf_sample_pdf(None, None, 0, 2, 4, None, 1, 0, None, st) == E_ARG
    assert L.nerf_sample_stratified(None, 0, 0, 0, None, 0, None, st) == E_ARG
    assert L.nerf_freq_encode(None, 0, 3, 2, 1, None, 14, st) == E_ARG
