"""nerf_grad_sqnorm / nerf_adam / nerf_adam_dstep / FlatAdam against a plain fp64 Adam (run on an MI355X: -m gpu).

The sizes sit on the kernels' own edges (csrc/adam.hip): sqnorm_kernel's two-float4 loop needs n > 1,048,576 and
falls back to a scalar loop when g is not 16-byte aligned; adam_kernel<true>'s non-temporal two-float4 loop needs
n > 4,194,304; adam_kernel<false> runs when any of p/g/m/v is not 16-byte aligned; segment edges fall inside float4
groups.

Reference: ``adam_ref`` below, torch's single-tensor Adam with L2 weight decay restated in float64.  Gradients are
g = sign(p0) * (1 + rand) on every step, so g*scale + wd*p never cancels and fp32 Adam stays well-conditioned.

Tolerance: none is hard-coded.  Each case measures e_ref = max |fp32 - ref64| / (1 + |ref64|) over p from torch's CPU
fp32 torch.optim.Adam (+ clip_grad_norm_) on the same inputs, or from adam_ref run in float32 where torch cannot
express the case (segments, a given start state), and allows the kernel 4 * e_ref * (1 + |ref64|) per element; m and
v likewise against their own fp64 values, relative to max |ref| of the tensor.  grad_sqnorm: relative error
(ceil(n / 262144) + 32) * 2^-24 (the additions one thread chains, plus the wave / block / partial sums; all terms
positive), and exactly 4.0 for a single 2.0 among zeros.

Measured on an MI355X (e_ref of the fp32 host run; worst kernel error in the same units; allowed is 4 x e_ref):
  adam, one segment, 4 clipped steps     p: e_ref 8.8e-9 (n = 3) .. 1.5e-7 (n = 4,194,304), kernel = 1.00 x e_ref at
                                            every size (the kernel's p is torch's fp32 p)
                                         m: e_ref 4.4e-8 .. 1.5e-7 up to n = 10007, kernel at most 1.32 x (n = 1023);
                                            1.0e-5 .. 3.7e-5 from n = 4,194,304 (torch's fp32 clip norm), kernel 1.8e-7
                                         v: e_ref 5.0e-8 .. 2.6e-7 up to n = 10007, kernel at most 2.51 x (n = 7);
                                            2.1e-5 .. 7.5e-5 from n = 4,194,304, kernel 2.9e-7
  scalar kernel, n = 10007 / 4,194,308   p 1.16e-7 / 1.48e-7 (1.00 x), m at most 0.89 x, v at most 1.05 x
  segments (wd 0.01, steps 3-4)          p 7.7e-8 .. 8.8e-8, m 5.8e-8 .. 7.6e-8, v 1.3e-7 .. 1.4e-7, kernel 1.00 x
  weight decay 0.01                      p 8.9e-8 .. 4.6e-7, m 1.1e-7 .. 3.6e-7, v 8.8e-8 .. 5.5e-7; kernel at most
                                            1.38 x (v, n = 4099, clip)
  bias correction, steps 1 .. 100000     p 3.9e-8 .. 4.1e-8, m 3.6e-8 .. 3.8e-8, v 6.9e-8 .. 7.1e-8, kernel at most
                                            1.02 x; host- and device-counted steps came out bitwise equal
  FlatAdam, 285 parameters, 5 steps      e_ref 8.5e-8 .. 1.2e-7, kernel 1.00 x (host- and device-counted)
  shard convention, W = 2 / 3            p 9.8e-8 / 1.1e-7 (1.00 x), m 9.4e-8 / 9.6e-8 (0.93 x), v 1.1e-7 / 1.5e-7
                                            (1.21 x)
  grad_sqnorm                            relative error at most 7.7e-8 (n = 1023, unaligned); 2.0e-6 .. 2.7e-6 allowed

Found by test_sqnorm_value[0-*]: nerf_grad_sqnorm refused an empty gradient (torch gives an empty tensor a NULL
pointer); it now writes 256 zeros.
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B1, B2, EPS = 0.9, 0.999, 1e-8
MARGIN = 4.0


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


# ------------------------------------------------------------------ the reference


def adam_ref(p, m, v, s, g, lr, mask, wd=0.0, max_norm=0.0, dtype=torch.float64):
    """One step of torch's single-tensor Adam (L2 weight decay, clip first) in ``dtype``; ``lr`` per element,
    elements outside ``mask`` keep p, m and v."""
    p, m, v, g, lr = (t.to(dtype) for t in (p, m, v, g, lr))
    scale = min(max_norm / (float(torch.linalg.vector_norm(g)) + 1e-6), 1.0) if max_norm > 0 else 1.0
    gi = g * scale + wd * p
    bc1, bc2 = 1.0 - B1 ** s, 1.0 - B2 ** s
    m2 = m + (1.0 - B1) * (gi - m)
    v2 = v * B2 + (1.0 - B2) * gi * gi
    p2 = p - (lr / bc1) * m2 / (v2.sqrt() / math.sqrt(bc2) + EPS)
    return torch.where(mask, p2, p), torch.where(mask, m2, m), torch.where(mask, v2, v)


def _torch_adam(p0, grads, lr, wd, clip, dtype):
    pt = p0.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [pt], "lr": lr}], betas=(B1, B2), eps=EPS, weight_decay=wd)
    for g in grads:
        pt.grad = g.to(dtype).clone()
        if clip > 0:
            torch.nn.utils.clip_grad_norm_([pt], clip)
        opt.step()
    st = opt.state[pt]
    return pt.detach(), st["exp_avg"], st["exp_avg_sq"]


def _e_ref(lo, ref):
    """(e_p, e_m, e_v) of an fp32 run against the fp64 one: p relative to 1 + |ref|, m and v to max |ref|."""
    ep = ((lo[0].double() - ref[0]).abs() / (1.0 + ref[0].abs())).max().item()
    em, ev = (((lo[i].double() - ref[i]).abs().max() / ref[i].abs().max()).item() for i in (1, 2))
    return ep, em, ev


@functools.lru_cache(maxsize=None)
def _case(n, offs=None, lrs=(2e-3,), wd=0.0, clip=1.0, s0=1, steps=4, start="zero", zero_from=None):
    """Inputs, the fp64 result and the measured fp32 error of one case (computed once, shared, never modified)."""
    offs = (0, n) if offs is None else offs
    gen = torch.Generator().manual_seed(1000003 * len(offs) + n + s0)
    p0 = torch.randn(n, generator=gen)
    sgn = torch.where(p0 >= 0, 1.0, -1.0)
    grads = [sgn * (1.0 + torch.rand(n, generator=gen)) for _ in range(steps)]
    if start == "zero":
        m0, v0 = torch.zeros(n), torch.zeros(n)
    else:
        m0, v0 = torch.randn(n, generator=gen), torch.rand(n, generator=gen)
    if zero_from is not None:  # the zero padding of a sharded flat buffer
        for t in [p0, m0, v0] + grads:
            t[zero_from:] = 0
    lr = torch.zeros(n, dtype=torch.float64)
    mask = torch.zeros(n, dtype=torch.bool)
    for i, x in enumerate(lrs):
        lr[offs[i]:offs[i + 1]] = x
        mask[offs[i]:offs[i + 1]] = True
    ref, lo = (p0, m0, v0), (p0, m0, v0)
    for k, g in enumerate(grads):
        ref = adam_ref(*ref, s0 + k, g, lr, mask, wd, clip)
    if offs == (0, n) and start == "zero" and s0 == 1 and zero_from is None:
        lo = _torch_adam(p0, grads, lrs[0], wd, clip, torch.float32)
    else:
        for k, g in enumerate(grads):
            lo = adam_ref(*lo, s0 + k, g, lr, mask, wd, clip, dtype=torch.float32)
    return SimpleNamespace(n=n, offs=offs, lrs=lrs, wd=wd, clip=clip, s0=s0, p0=p0, m0=m0, v0=v0, grads=grads,
                           mask=mask, ref=ref, e=_e_ref(lo, ref))


# ------------------------------------------------------------------ running the kernels


def _dev(t, off=0):
    """A device copy of t that starts ``off`` floats into its allocation (off = 1: not 16-byte aligned)."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    view = buf[off:off + t.numel()]
    view.copy_(t)
    assert (view.data_ptr() % 16 == 0) == (off % 4 == 0) or t.numel() == 0
    return view


def _run(K, c, mis=(0, 0, 0, 0), dstep=False, clip=None, grads=None):
    """The case's steps through grad_sqnorm + adam; ``mis`` = float offsets of the p, g, m, v views."""
    clip = c.clip if clip is None else clip
    p, m, v = _dev(c.p0, mis[0]), _dev(c.m0, mis[2]), _dev(c.v0, mis[3])
    g = _dev(c.p0, mis[1])
    sd = torch.full((1,), c.s0 - 1, dtype=torch.int64, device=DEV) if dstep else None
    for k, gr in enumerate(c.grads if grads is None else grads):
        g.copy_(gr)
        parts, mx = (K.grad_sqnorm(g), float(clip)) if clip > 0 else (None, 0.0)
        if dstep:
            sd.add_(1)
        K.adam(p, g, m, v, list(c.offs), list(c.lrs), sd if dstep else c.s0 + k, (B1, B2), EPS, c.wd, parts, mx)
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu()


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(c, got, what, other=None):
    """got (p, m, v) within MARGIN * e_ref of the case's fp64 result (of ``other`` where given: same allowance)."""
    bad = []
    for i, name in enumerate("pmv"):
        r = c.ref[i]
        x = got[i].double()
        y = r if other is None else other[i].double()
        scale = (1.0 + r.abs()) if i == 0 else r.abs().max()
        err = ((x - y).abs() / scale).max().item()
        print(f"{what} {name}: e_ref {c.e[i]:.3e} err {err:.3e} ({err / c.e[i] if c.e[i] else float('inf'):.2f} x)")
        if not ((x - y).abs() <= MARGIN * c.e[i] * scale).all():
            bad.append(f"{name}: err {err:.3e} > {MARGIN} * e_ref {c.e[i]:.3e}")
    assert not bad, f"{what}: " + "; ".join(bad)


def test_reference_is_torch_adam_in_fp64():
    """adam_ref restates torch.optim.Adam + clip_grad_norm_: in float64 the two agree to rounding."""
    for wd, clip in ((0.0, 1.0), (0.01, 1.0), (0.01, 0.0)):
        c = _case(10007, wd=wd, clip=clip)
        t = _torch_adam(c.p0, c.grads, c.lrs[0], wd, clip, torch.float64)
        for a, b in zip(t, c.ref):
            assert (a - b).abs().max().item() <= 1e-13 * (1.0 + b.abs().max().item())


# ------------------------------------------------------------------ A. grad_sqnorm

SQ_SIZES = [0, 1, 3, 4, 5, 1023, 1048576, 1048580, 2097152, 2097152 + 4003, 3 * 1048576 + 7]


@functools.lru_cache(maxsize=None)
def _sq_data():
    return torch.randn(max(SQ_SIZES) + 1, generator=torch.Generator().manual_seed(7))


@pytest.fixture(scope="module")
def sq_dev(K):
    return _sq_data().to(DEV), torch.zeros(max(SQ_SIZES) + 1, device=DEV)


def _sqnorm(K, g):
    parts = torch.full((256,), float("nan"), device=DEV)
    out = K.grad_sqnorm(g, parts)
    assert out is parts
    return parts.cpu()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SQ_SIZES)
def test_sqnorm_value(K, sq_dev, n, off):
    g = sq_dev[0][off:off + n]
    assert n == 0 or (g.data_ptr() % 16 == 0) == (off == 0)
    parts = _sqnorm(K, g)
    assert torch.isfinite(parts).all()
    assert _bits(parts, _sqnorm(K, g)), "two calls on the same data differ"
    if n == 0:
        assert not parts.any()
        return
    ref = _sq_data()[off:off + n].double().square().sum().item()
    err = abs(parts.double().sum().item() - ref) / ref
    tol = (math.ceil(n / 262144) + 32) * 2.0 ** -24
    print(f"sqnorm n={n} off={off}: rel err {err:.3e} (allowed {tol:.3e})")
    assert err <= tol


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SQ_SIZES[1:])
def test_sqnorm_single_element_exact(K, sq_dev, n, off):
    """One 2.0 among zeros sums to exactly 4.0 wherever it sits: no element is dropped or read twice."""
    g = sq_dev[1][off:off + n]
    for idx in sorted({0, 3, 4 * (n // 4) - 1, 4 * (n // 4), n - 1, 4 * 262144}):
        if not 0 <= idx < n:
            continue
        g[idx] = 2.0
        parts = _sqnorm(K, g)
        g[idx] = 0.0
        assert torch.isfinite(parts).all()
        assert parts.double().sum().item() == 4.0, (n, off, idx, parts.double().sum().item())


# ------------------------------------------------------------------ B. adam / adam_dstep

LOOP_SIZES = [1, 2, 3, 4, 5, 7, 1023, 1025, 10007, 4194304, 4194308, 8388608 + 4003]


@pytest.mark.parametrize("n", LOOP_SIZES)
def test_adam_loops(K, n):
    """4 clipped steps from zero state, one segment: the float4 loop, its unrolled non-temporal form, the tail."""
    c = _case(n)
    _check(c, _run(K, c), f"adam n={n}")


@pytest.mark.parametrize("mis", [(1, 1, 1, 1), (0, 0, 1, 0)], ids=["all-offset", "m-offset"])
@pytest.mark.parametrize("n", [10007, 4194308])
def test_adam_scalar_path(K, n, mis):
    """Any pointer off 16-byte alignment selects adam_kernel<false>.  Both paths call the same adam_elem, but not
    bit for bit: of the 13 inlined copies in adam_kernel<true> the compiler leaves two with m and v as separate
    multiplies and adds (packed v_pk_mul_f32) and contracts the rest, and the one in adam_kernel<false>, to fma.  So
    the two paths are held to each other within the reference tolerance, not bitwise."""
    c = _case(n)
    got = _run(K, c, mis=mis)
    _check(c, got, f"adam scalar n={n} mis={mis}")
    _check(c, got, f"adam scalar n={n} mis={mis} vs float4", other=_run(K, c))


N_SEG = 4194308 + 13
SEG_TABLES = {
    "eight": ((3, 10, 11, 11, 4099, 1048577, 2097154, 4194305, N_SEG - 2),
              tuple(1e-4 * 100.0 ** (i / 7.0) for i in range(8)), N_SEG),
    "shard": ((0, 0, 33333, 100032, 100032), (1e-2, 3e-3, 1e-3, 1e-4), 100032),
    "inside": ((6, N_SEG - 7), (2e-3,), N_SEG),
}


@pytest.mark.parametrize("dstep", [False, True], ids=["host-step", "device-step"])
@pytest.mark.parametrize("table", list(SEG_TABLES))
def test_adam_segments(K, table, dstep):
    """Segment edges inside float4 groups, empty and one-element segments, and everything outside left alone."""
    offs, lrs, n = SEG_TABLES[table]
    c = _case(n, offs, lrs, wd=0.01, s0=3, steps=2, start="rand")
    got = _run(K, c, dstep=dstep)
    _check(c, got, f"adam segments {table} dstep={dstep}")
    out = ~c.mask
    assert out.sum().item() == n - (offs[-1] - offs[0])
    for name, a, b in zip("pmv", got, (c.p0, c.m0, c.v0)):
        assert _bits(a[out], b[out]), f"{name}: an element outside every segment changed"


@pytest.mark.parametrize("clip", [1.0, 0.0], ids=["clip", "noclip"])
@pytest.mark.parametrize("n", [4099, 8388608 + 4003])
def test_adam_weight_decay(K, n, clip):
    c = _case(n, wd=0.01, clip=clip, lrs=(1e-2,))
    _check(c, _run(K, c), f"adam wd n={n} clip={clip}")


@pytest.mark.parametrize("n", [4099, 10007])
def test_adam_clip_identities(K, n):
    c = _case(n)
    assert max(float(g.norm()) for g in c.grads) < 1e3
    for name, a, b in zip("pmv", _run(K, c, clip=1e6), _run(K, c, clip=0.0)):
        assert _bits(a, b), f"{name}: a max_norm above the norm is not the unclipped step"
    zeros = [torch.zeros(n)] * 4
    for clip in (1.0, 0.0):
        p, m, v = _run(K, c, clip=clip, grads=zeros)
        assert _bits(p, c.p0), "a zero gradient moved p"
        assert not m.any() and not v.any()


@pytest.mark.parametrize("s", [1, 2, 10, 1000, 100000])
def test_adam_bias_correction(K, s):
    """One step at step count s from a random state, counted on the host (nerf_adam) and on the device (dstep)."""
    c = _case(10007, s0=s, steps=1, start="rand")
    host, dev = _run(K, c), _run(K, c, dstep=True)
    _check(c, host, f"adam step={s} host")
    _check(c, dev, f"adam step={s} device")
    _check(c, host, f"adam step={s} host vs device", other=dev)


def test_adam_argument_checks(K):
    n = 1023
    c = _case(n)
    p, g, m, v = _dev(c.p0), _dev(c.grads[0]), _dev(c.m0), _dev(c.v0)
    bad = [
        ("nine segments", list(range(0, 1000, 100)), [1e-3] * 9, 1),
        ("decreasing offsets", [0, 500, 400, n], [1e-3] * 3, 1),
        ("off[-1] > n", [0, n + 1], [1e-3], 1),
        ("off[0] < 0", [-1, n], [1e-3], 1),
        ("step 0", [0, n], [1e-3], 0),
    ]
    for what, offs, lrs, step in bad:
        with pytest.raises(ValueError, match="nerf_adam"):
            K.adam(p, g, m, v, offs, lrs, step)
        torch.cuda.synchronize()
        assert _bits(p.cpu(), c.p0), what
    K.adam(p, g, m, v, [0, n], [1e-3], 1)  # the well-formed call goes through
    assert not _bits(p.cpu(), c.p0)


# ------------------------------------------------------------------ C. FlatAdam, single rank

SHAPES = [(7, 3), (5,), (129, 2), (1,)]
GROUP_OF = [0, 1, 1, 2]
GROUP_LR = [1e-2, 3e-3, 1e-3]


def _groups(ps):
    return [{"params": [p for p, k in zip(ps, GROUP_OF) if k == gi], "lr": lr} for gi, lr in enumerate(GROUP_LR)]


@functools.lru_cache(maxsize=None)
def _flat_case(clip, wd, steps=5):
    gen = torch.Generator().manual_seed(11)
    p0 = [torch.randn(s, generator=gen) for s in SHAPES]
    grads = [[torch.where(p >= 0, 1.0, -1.0) * (1.0 + torch.rand(p.shape, generator=gen)) for p in p0]
             for _ in range(steps)]

    def run(dtype):
        ps = [p.to(dtype).clone().requires_grad_(True) for p in p0]
        opt = torch.optim.Adam(_groups(ps), betas=(B1, B2), eps=EPS, weight_decay=wd)
        for gs in grads:
            for p, g in zip(ps, gs):
                p.grad = g.to(dtype).clone()
            if clip:
                torch.nn.utils.clip_grad_norm_(ps, clip)
            opt.step()
        return torch.cat([p.detach().reshape(-1) for p in ps])

    ref, lo = run(torch.float64), run(torch.float32)
    e = ((lo.double() - ref).abs() / (1.0 + ref.abs())).max().item()
    return SimpleNamespace(p0=p0, grads=grads, ref=ref, e=e)


def _inside(t, buf):
    return buf.data_ptr() <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= buf.data_ptr() + 4 * buf.numel()


def _flat_run(c, clip, wd, dstep):
    from nerf_amd.optim import FlatAdam
    ps = [torch.nn.Parameter(p.to(DEV)) for p in c.p0]
    opt = FlatAdam(_groups(ps), betas=(B1, B2), eps=EPS, weight_decay=wd, grad_clip=clip)
    assert opt.seg_off == [0, 21, 284, 285] and opt.seg_lr == GROUP_LR
    assert torch.equal(opt.flat.cpu(), torch.cat([p.reshape(-1) for p in c.p0]))
    if dstep:
        opt.device_step()
    for k, gs in enumerate(c.grads, 1):
        for p, g in zip(ps, gs):
            p.grad.copy_(g)
        assert torch.equal(opt.grad.cpu(), torch.cat([g.reshape(-1) for g in gs]))
        opt.step()
        for p in ps:
            assert _inside(p, opt.flat) and _inside(p.grad, opt.grad)
        opt.zero_grad()
        assert not any(p.grad.any().item() for p in ps) and not opt.grad.any().item()
        assert opt.step_count == k
    torch.cuda.synchronize()
    return torch.cat([p.detach().reshape(-1) for p in ps]).cpu(), opt


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [1.0, None])
def test_flat_adam_matches_torch(K, clip, wd):
    c = _flat_case(clip, wd)
    got, _ = _flat_run(c, clip, wd, dstep=False)
    err = ((got.double() - c.ref).abs() / (1.0 + c.ref.abs())).max().item()
    print(f"FlatAdam clip={clip} wd={wd}: e_ref {c.e:.3e} err {err:.3e}")
    assert ((got.double() - c.ref).abs() <= MARGIN * c.e * (1.0 + c.ref.abs())).all(), (err, c.e)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [1.0, None])
def test_flat_adam_device_step(K, clip, wd):
    c = _flat_case(clip, wd)
    host, _ = _flat_run(c, clip, wd, dstep=False)
    got, opt = _flat_run(c, clip, wd, dstep=True)
    assert opt.step_dev.item() == len(c.grads) == opt.step_count
    tol = MARGIN * c.e * (1.0 + c.ref.abs())
    err = ((got.double() - c.ref).abs() / (1.0 + c.ref.abs())).max().item()
    print(f"FlatAdam device step clip={clip} wd={wd}: e_ref {c.e:.3e} err {err:.3e}")
    assert ((got.double() - c.ref).abs() <= tol).all(), (err, c.e)
    assert ((got.double() - host.double()).abs() <= tol).all()


@pytest.mark.parametrize("W", [2, 3])
def test_flat_adam_shard_convention(K, W):
    """FlatAdam._step_sharded's calls without a process group: per-rank slices, partials added block by block,
    offsets clipped to the slice; the slices together are the whole-buffer step and the padding stays zero."""
    n, seg_off, lrs = 100003, (0, 30001, 70002, 100003), (1e-2, 3e-3, 1e-3)
    S = -(-n // (W * 64)) * 64
    c = _case(S * W, seg_off, lrs, wd=0.01, steps=3, zero_from=n)
    p, m, v, g = _dev(c.p0), _dev(c.m0), _dev(c.v0), _dev(c.p0)
    for k, gr in enumerate(c.grads, 1):
        g.copy_(gr)
        parts = torch.zeros(256, device=DEV)
        for r in range(W):
            parts += K.grad_sqnorm(g[r * S:(r + 1) * S])
        for r in range(W):
            sl = slice(r * S, (r + 1) * S)
            seg = [min(max(o - r * S, 0), S) for o in seg_off]
            K.adam(p[sl], g[sl], m[sl], v[sl], seg, list(lrs), k, (B1, B2), EPS, c.wd, parts, 1.0)
    torch.cuda.synchronize()
    got = (p.cpu(), m.cpu(), v.cpu())
    _check(c, got, f"shard convention W={W}")
    for t in got:
        assert not t[n:].any(), "the zero padding moved"
