"""The occupancy-grid kernels (csrc/occ.hip) at their wave, tile and level edges, through the C entry points, against
the references of tests/occ_reference.py (checked on the CPU by tests/test_occ_reference.py).  Run on an MI355X: -m gpu.

Integer work, the seeded draws and the dyadic march family are compared as bytes; compositing, its backward, the cell
points and the packed points are compared with float64 under the bounds derived in occ_reference's docstring, and each
such test prints its worst error / bound before it asserts <= 1; threshold decisions (visibility, invisible cells) are
compared exactly outside the derived margins.  Every output buffer is pre-filled with a sentinel and everything the
kernel should not write must keep it."""
import ctypes

import numpy as np
import pytest
import torch

import occ_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32
U64 = ctypes.c_uint64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _api():
    from nerf_amd._lib import lib, ptr, stream
    return lib(), ptr, stream


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _full(shape, value, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device=DEV)


def _padded(a, value):
    """a on the device with one sentinel row behind it (never empty, so never a null pointer)."""
    a = np.ascontiguousarray(a)
    pad = np.full((1,) + a.shape[1:], value, dtype=a.dtype)
    return _d(np.concatenate([a, pad]))


def _grid(g):
    from nerf_amd.occupancy import NerfOccGrid
    s = NerfOccGrid()
    s.levels, s.resolution = g["L"], g["R"]
    for i, v in enumerate(g["roi"]):
        s.roi[i] = float(v)
    return s


def _addr(s):
    return ctypes.c_void_p(ctypes.addressof(s))


def _keeps(t, n, value):
    return bool((t[n:] == value).all())


# ================================================================================================= single march

def _march_args(case, stratified, u, seed, **over):
    _, ptr, _ = _api()
    keep = dict(g=_grid(case), bin=_d(case["bin"]), rays=_d(case["rays"]), u=None if u is None else _d(u))
    a = dict(near=case["near_plane"], far=case["far_plane"], step=case["step"], cone=case["cone"],
             max_steps=case["max_steps"])
    a.update(over)
    args = (_addr(keep["g"]), ptr(keep["bin"]), ptr(keep["rays"]), case["rays"].shape[0], a["near"], a["far"],
            a["step"], a["cone"], int(stratified), ptr(keep["u"]), U64(seed), a["max_steps"])
    return args, keep


def _march(case, stratified=None, u=None, seed=0):
    """Count pass, host scan, write pass -> (counts (N), ray_idx, t0, t1 (M + 8, sentinel past M))."""
    L, ptr, stream = _api()
    if stratified is None:
        stratified, u = case["u"] is not None, case["u"]
    args, keep = _march_args(case, stratified, u, seed)
    N = case["rays"].shape[0]
    counts = _full(N + 2, R.ISENT, I32)
    assert L.nerf_occ_march(*args, ptr(counts), None, None, None, None, stream()) == 0
    cnt = counts.cpu().numpy()
    assert (cnt[N:] == R.ISENT).all() and (cnt[:N] >= 0).all()
    offs = R.exclusive_scan(cnt[:N])
    M = int(offs[-1])
    ri, t0, t1 = _full(M + 8, R.ISENT, I32), _full(M + 8, R.SENT), _full(M + 8, R.SENT)
    doffs = _d(offs)
    assert L.nerf_occ_march(*args, None, ptr(doffs), ptr(ri), ptr(t0), ptr(t1), stream()) == 0
    torch.cuda.synchronize()
    del keep
    return cnt[:N], ri.cpu().numpy(), t0.cpu().numpy(), t1.cpu().numpy()


def _check_packed(got, want, what, limit=None):
    """got: arrays with a sentinel tail; want: (counts, ray_idx, t0, t1) of the reference.  With limit (a clamped
    capacity) only the first min(limit, M) entries are written."""
    ri, t0, t1 = got
    _, rri, r0, r1 = want
    M = len(rri)
    m = M if limit is None else min(limit, M)
    assert np.array_equal(ri[:m], rri[:m]), what
    assert R.same_bits(t0[:m], r0[:m].astype(np.float32)) and R.same_bits(t1[:m], r1[:m].astype(np.float32)), what
    assert (ri[m:] == R.ISENT).all() and (t0[m:] == R.SENT).all() and (t1[m:] == R.SENT).all(), what


@pytest.mark.parametrize("i", range(len(R.MARCH_CASES)))
def test_march_dyadic_bitwise(i):
    """Counts, ray indices, t0 and t1 of every ray equal to the reference's, as bytes: L = 1, 2, 3; cube, flat and
    off-centre ROI; empty, full and random grids; explicit jitter; a binding max_steps; N = 1, 127, 128, 129."""
    want = R.march_expected(i)
    cnt, ri, t0, t1 = _march(R.march_case(i))
    bad = np.flatnonzero(cnt != want[0])
    assert bad.size == 0, (R.MARCH_CASES[i], bad[:8].tolist(), cnt[bad[:8]].tolist(), want[0][bad[:8]].tolist())
    _check_packed((ri, t0, t1), want, R.MARCH_CASES[i])


@pytest.mark.parametrize("i", range(len(R.CONE_CASES)))
def test_march_cone_one_step_checks(i):
    """cone > 0 on generic rays: the kernel's own samples checked one step at a time (occ_reference.cone_checks)."""
    case = R.cone_case(i)
    cnt, ri, t0, t1 = _march(case)
    M = int(cnt.sum())
    assert np.array_equal(ri[:M], np.repeat(np.arange(case["N"]), cnt).astype(np.int32))
    assert (ri[M:] == R.ISENT).all() and (t0[M:] == R.SENT).all() and (t1[M:] == R.SENT).all()
    res = R.cone_checks(case, cnt, t0[:M], t1[:M])
    share = res["left_out"] / (res["left_out"] + res["checked"])
    print(f"cone march {i}: {M} samples, {res['checked']} checks, left out {share:.4%}, failed {res['failed'][:6]}")
    assert res["failed"] == [] and share <= 0.02 and M > 2000


def test_march_seeded_jitter_is_the_restated_stream():
    """stratified with u == NULL draws nerf_uniform(seed, 0x0CC, r): the same bytes as passing that u."""
    case = R.march_case(0)
    N = case["rays"].shape[0]
    for seed in (0, 7, 2 ** 63 + 12345):
        a = _march(case, True, None, seed)
        b = _march(case, True, R.uniforms(seed, 0x0CC, N), seed + 1)      # the seed is unused when u is given
        for x, y in zip(a, b):
            assert R.same_bits(x, y), seed
    plain = _march(case, False, None, 0)
    assert not R.same_bits(a[2], plain[2])


def test_march_error_returns():
    L, ptr, stream = _api()
    case = R.march_case(3)
    counts, offs = _full(4, R.ISENT, I32), torch.zeros(2, dtype=I32, device=DEV)
    ri, t0 = _full(8, R.ISENT, I32), _full(8, R.SENT)
    tail = (ptr(counts), None, None, None, None, stream())
    for over in (dict(step=0.0), dict(step=-1.0), dict(step=float("nan")), dict(max_steps=0)):
        args, keep = _march_args(case, False, None, 0, **over)
        assert L.nerf_occ_march(*args, *tail) == -1, over
    for bad in (dict(L=0), dict(L=9), dict(R=0), dict(R=513), dict(roi=[-1, -1, -1, 1, -1, 1])):
        args, keep = _march_args(dict(case, **bad), False, None, 0)
        assert L.nerf_occ_march(*args, *tail) == -1, bad
    args, keep = _march_args(case, False, None, 0)
    assert L.nerf_occ_march(*args, None, None, None, None, None, stream()) == -1
    assert L.nerf_occ_march(*args, None, ptr(offs), None, ptr(t0), ptr(t0), stream()) == -1
    assert L.nerf_occ_march(*args, None, ptr(offs), ptr(ri), None, ptr(t0), stream()) == -1
    assert L.nerf_occ_march(*args, None, ptr(offs), ptr(ri), ptr(t0), None, stream()) == -1
    assert L.nerf_occ_march(args[0], None, *args[2:], *tail) == -1
    assert L.nerf_occ_march(*args[:3], 0, *args[4:], None, None, None, None, None, stream()) == 0      # N = 0
    torch.cuda.synchronize()
    assert _keeps(counts, 0, R.ISENT) and _keeps(ri, 0, R.ISENT) and _keeps(t0, 0, R.SENT)


# ================================================================================================= multi-expert march

class _Multi:
    """Host-side arguments of the multi-expert entry points for a list of experts."""

    def __init__(self, experts, rays, run, stratified=0, seed=0):
        from nerf_amd.occupancy import NerfOccGrid
        _, ptr, _ = _api()
        K = len(experts)
        self.K, self.N = K, rays.shape[0]
        self.grids = (NerfOccGrid * K)()
        for k, e in enumerate(experts):
            self.grids[k].levels, self.grids[k].resolution = e["L"], e["R"]
            for i, v in enumerate(e["roi"]):
                self.grids[k].roi[i] = float(v)
        self.bins = [_d(e["bin"]) for e in experts]
        self.barr = (ctypes.c_void_p * K)(*[b.data_ptr() for b in self.bins])
        self.boxes = (ctypes.c_float * (6 * K))(*[float(v) for e in experts for v in e["box"]])
        self.steps = (ctypes.c_float * K)(*[float(e["step"]) for e in experts])
        self.rays = _d(rays)
        self.head = (self.grids, self.barr, self.boxes, self.steps, K, ptr(self.rays), self.N, run["near_plane"],
                     run["far_plane"], run["cone"], int(stratified), U64(seed), run["max_steps"])

    def counts(self, stage_cap=None, dseed=None):
        L, ptr, stream = _api()
        KN = self.K * self.N
        counts = _full(KN + 2, R.ISENT, I32)
        if stage_cap is None:
            rc = L.nerf_occ_march_multi(*self.head, ptr(counts), None, None, None, None, stream())
        else:
            self.cap = stage_cap
            self.stage = _full(2 * KN * stage_cap + 2, R.SENT)
            tail = (ptr(counts), ptr(self.stage), stage_cap, None, None, None, None)
            if dseed is None:
                rc = L.nerf_occ_march_multi_staged(*self.head, *tail, stream())
            else:
                rc = L.nerf_occ_march_multi_staged_dseed(*self.head, *tail, ptr(dseed[0]), U64(dseed[1]), stream())
        assert rc == 0
        self.dcounts = counts
        cnt = counts.cpu().numpy()
        assert (cnt[KN:] == R.ISENT).all()
        if stage_cap is not None:
            assert _keeps(self.stage, 2 * KN * stage_cap, R.SENT)
        return cnt[:KN]

    def write(self, offs, size, staged=False, dseed=None):
        L, ptr, stream = _api()
        ri, t0, t1 = _full(size, R.ISENT, I32), _full(size, R.SENT), _full(size, R.SENT)
        doffs = _d(np.asarray(offs, dtype=np.int32))
        out = (ptr(doffs), ptr(ri), ptr(t0), ptr(t1))
        if not staged:
            rc = L.nerf_occ_march_multi(*self.head, None, *out, stream())
        elif dseed is None:
            rc = L.nerf_occ_march_multi_staged(*self.head, ptr(self.dcounts), ptr(self.stage), self.cap, *out, stream())
        else:
            rc = L.nerf_occ_march_multi_staged_dseed(*self.head, ptr(self.dcounts), ptr(self.stage), self.cap, *out,
                                                     ptr(dseed[0]), U64(dseed[1]), stream())
        assert rc == 0
        torch.cuda.synchronize()
        return ri.cpu().numpy(), t0.cpu().numpy(), t1.cpu().numpy()


def test_march_multi_dyadic_bitwise():
    """K = 2 grids built from structs, boxes that some rays miss, graze along a face or start inside."""
    experts, rays, run = R.multi_case()
    want = R.multi_expected()
    m = _Multi(experts, rays, run)
    cnt = m.counts()
    bad = np.flatnonzero(cnt != want[0])
    assert bad.size == 0, (bad[:8].tolist(), cnt[bad[:8]].tolist(), want[0][bad[:8]].tolist())
    M = int(cnt.sum())
    _check_packed(m.write(R.exclusive_scan(cnt), M + 8), want, "multi")


@pytest.mark.parametrize("cap", R.STAGE_CAPS)
def test_march_staged_and_clamped_offsets(cap):
    """The staged march (count pass keeps cap segments per pair, write pass copies them and marches only the longer
    pairs) against the same reference, then with the offsets clamped to a capacity C as the sync-free container step
    does: the first min(C, M) samples are the unclamped ones and nothing is written behind them.  The plain
    multi-expert write pass obeys the same clamp."""
    experts, rays, run = R.multi_case()
    want = R.multi_expected()
    m = _Multi(experts, rays, run)
    cnt = m.counts(stage_cap=cap)
    assert np.array_equal(cnt, want[0])
    assert (cnt > cap).any() == (cap < 512)
    offs = R.exclusive_scan(cnt).astype(np.int64)
    M = int(offs[-1])
    _check_packed(m.write(offs, M + 8, staged=True), want, ("staged", cap))
    for C in R.clamp_capacities(cnt, cap):
        clamped = np.minimum(offs, C)
        _check_packed(m.write(clamped, M + 8, staged=True), want, ("staged", cap, C), limit=C)
        _check_packed(m.write(clamped, M + 8, staged=False), want, ("plain", cap, C), limit=C)


def test_march_multi_jitter_streams_and_device_seed():
    """Expert k jitters with the stream 0x0CC00 + k: rays that start inside both (full) grids emit their first sample
    at fl(near + u step_k).  The _dseed entry with *step_dev = s is the plain call with seed + s * seed_mul."""
    L, ptr, stream = _api()
    experts = [dict(e, bin=R.march_binary(e, "full", 0)) for e in R.MULTI_EXPERTS]
    N = 67
    rs = np.random.RandomState(5)
    rays = np.zeros((N, 8), dtype=np.float32)
    rays[:, :3] = [0.25, 0.0, 0.0] + (rs.rand(N, 3) - 0.5) * 0.25            # inside both grids and both boxes
    d = rs.randn(N, 3)
    rays[:, 3:6] = 0.25 * d / np.linalg.norm(d, axis=1, keepdims=True)   # short: the first step stays inside
    rays[:, 7] = 9.0
    run = dict(near_plane=R.NEAR_PLANE, far_plane=R.FAR_PLANE, max_steps=64, cone=0.0)
    seed, mul, s = 0x1234567890ABCDEF, 0x9E3779B97F4A7C15, 3
    m = _Multi(experts, rays, run, stratified=1, seed=seed)
    cnt = m.counts()
    assert (cnt > 0).all()
    offs = R.exclusive_scan(cnt)
    ri, t0, t1 = m.write(offs, int(offs[-1]) + 8)
    for k, e in enumerate(experts):
        u = R.uniforms(seed, 0x0CC00 + k, N).astype(np.float64)
        first = (R.NEAR_PLANE + u * e["step"]).astype(np.float32)
        assert R.same_bits(t0[offs[k * N:(k + 1) * N]], first), k
    # device-side seed
    step_dev = torch.tensor([s], dtype=torch.int64, device=DEV)
    a = _Multi(experts, rays, run, stratified=1, seed=seed)
    ca = a.counts(stage_cap=3, dseed=(step_dev, mul))
    b = _Multi(experts, rays, run, stratified=1, seed=(seed + s * mul) % 2 ** 64)
    cb = b.counts(stage_cap=3)
    assert np.array_equal(ca, cb)
    offs = R.exclusive_scan(ca)
    wa = a.write(offs, int(offs[-1]) + 8, staged=True, dseed=(step_dev, mul))
    wb = b.write(offs, int(offs[-1]) + 8, staged=True)
    for x, y in zip(wa, wb):
        assert R.same_bits(x, y)
    tail = (ptr(a.dcounts), ptr(a.stage), 3, None, None, None, None)
    assert L.nerf_occ_march_multi_staged_dseed(*a.head, *tail, None, U64(mul), stream()) == -1


# ================================================================================================= packed compositing

def _packed_dev(case):
    return dict(rs=_padded(case["rs"], R.SENT), t0=_padded(case["t0"], R.SENT), t1=_padded(case["t1"], R.SENT),
                offs=_d(case["offs"]), bg=_d(case["bg"]), g_rgb=_d(case["g_rgb"]), g_depth=_d(case["g_depth"]),
                g_acc=_d(case["g_acc"]), g_w=_padded(case["g_w"], R.SENT))


@pytest.mark.parametrize("name", list(R.PACKED_CASES))
def test_packed_forward_backward_vs_float64(name):
    """Ray lengths 0, 1, 63 .. 65, 127 .. 129, 192, 300 and N = 1, 3, 4, 5, 37 (four rays per block), with and
    without bg, g_depth, g_acc and g_weights; all-empty and trailing empty rays; a saturated ray and a sigma = 0 ray."""
    L, ptr, stream = _api()
    case = R.packed_case(name)
    N, M = case["N"], case["M"]
    dv = _packed_dev(case)
    worst = {}
    for with_bg in (True, False):
        w, rgb = _full(M + 1, R.SENT), _full((N + 1, 3), R.SENT)
        dep, acc = _full(N + 1, R.SENT), _full(N + 1, R.SENT)
        assert L.nerf_packed_composite_fwd(ptr(dv["rs"]), ptr(dv["t0"]), ptr(dv["t1"]), ptr(dv["offs"]), N,
                                           ptr(dv["bg"]) if with_bg else None, ptr(rgb), ptr(dep), ptr(acc), ptr(w),
                                           stream()) == 0
        v, e = R.packed_forward(case, with_bg)
        got = dict(w=w, rgb=rgb, depth=dep, acc=acc)
        for k in v:
            n = M if k == "w" else N
            assert _keeps(got[k], n, R.SENT), (name, k)
            worst["fwd " + k] = max(worst.get("fwd " + k, 0.0), R.worst_ratio(got[k][:n], v[k], e[k]))
        if name == "saturated":
            wc = w.cpu().numpy()
            a, b, c = (int(x) for x in case["offs"][:3])
            T = np.exp(-(np.cumsum(case["rs"][a:b, 3].astype(np.float64) * 0.001)))      # dt >= 0.001
            assert (wc[a:b][1:][T[:-1] < 2.0 ** -160] == 0).all() and (wc[b:c] == 0).all()
    for flags in ((True, True, True, True), (False, False, False, False), (True, False, True, False),
                  (False, True, False, True)):
        drs = _full((M + 1, 4), R.SENT)
        opt = [ptr(dv[k]) if f else None for k, f in zip(("bg", "g_depth", "g_acc", "g_w"), flags)]
        assert L.nerf_packed_composite_bwd(ptr(dv["rs"]), ptr(dv["t0"]), ptr(dv["t1"]), ptr(dv["offs"]), N, opt[0],
                                           ptr(dv["g_rgb"]), opt[1], opt[2], opt[3], ptr(drs), stream()) == 0
        val, err = R.packed_backward(case, *flags)
        assert _keeps(drs, M, R.SENT), (name, flags)
        worst["bwd rgb"] = max(worst.get("bwd rgb", 0.0), R.worst_ratio(drs[:M, :3], val[:, :3], err[:, :3]))
        worst["bwd sigma"] = max(worst.get("bwd sigma", 0.0), R.worst_ratio(drs[:M, 3], val[:, 3], err[:, 3]))
    print(f"packed {name}: worst error / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_packed_alignment_and_zero_rays():
    L, ptr, stream = _api()
    case = R.packed_case("N3")
    N, M = case["N"], case["M"]
    dv = _packed_dev(case)
    flat = _full(4 * M + 8, 0.5)
    off1 = ctypes.c_void_p(flat.data_ptr() + 4)
    outs = [_full((N, 3), R.SENT), _full(N, R.SENT), _full(N, R.SENT), _full(M, R.SENT)]
    head = (ptr(dv["t0"]), ptr(dv["t1"]), ptr(dv["offs"]), N)
    assert L.nerf_packed_composite_fwd(off1, *head, None, *[ptr(o) for o in outs], stream()) == -2
    drs = _full((M + 1, 4), R.SENT)
    assert L.nerf_packed_composite_bwd(off1, *head, None, ptr(dv["g_rgb"]), None, None, None, ptr(drs), stream()) == -2
    assert L.nerf_packed_composite_bwd(ptr(dv["rs"]), *head, None, ptr(dv["g_rgb"]), None, None, None,
                                       ctypes.c_void_p(drs.data_ptr() + 4), stream()) == -2
    assert L.nerf_packed_composite_fwd(ptr(dv["rs"]), *head[:3], 0, None, None, None, None, None, stream()) == 0
    assert L.nerf_packed_composite_fwd(ptr(dv["rs"]), *head[:3], -1, None, *[ptr(o) for o in outs], stream()) == -1
    torch.cuda.synchronize()
    assert all(_keeps(o, 0, R.SENT) for o in outs) and _keeps(drs, 0, R.SENT)


# ================================================================================================= visibility, compaction

def _vis_runs(N):
    yield dict(eps=R.VIS_EPS, athr=R.VIS_ATHR)
    yield dict(eps=R.VIS_EPS, athr=0.0)
    for group in sorted({1, 3, N}):
        yield dict(eps=R.VIS_EPS, athr=R.VIS_ATHR, groups=R.vis_group_thresholds(-(-N // group), group), group=group)


@pytest.mark.parametrize("name", ["N37", "all_lengths", "N5", "N4", "N3", "N1", "trailing_empty", "saturated"])
def test_visibility_and_compaction(name):
    """nerf_packed_visibility and _groups (group sizes 1, 3, N; thresholds above, below, at and under 0) equal to the
    float64 decision outside the derived margins; then nerf_packed_compact with and without counts, as bytes."""
    L, ptr, stream = _api()
    case = R.packed_case(name)
    N, M = case["N"], case["M"]
    dv = _packed_dev(case)
    sig = _padded(case["rs"][:, 3], R.SENT)
    ri = np.repeat(np.arange(N), np.diff(case["offs"])).astype(np.int32)
    dri = _padded(ri, R.ISENT)
    left = total = 0
    for kw in _vis_runs(N):
        keep = _full(M + 1, R.ISENT, I32)
        head = (ptr(dv["t0"]), ptr(dv["t1"]), ptr(sig), ptr(dv["offs"]), N)
        if "groups" in kw:
            dg = _d(kw["groups"])
            assert L.nerf_packed_visibility_groups(*head, kw["group"], kw["eps"], kw["athr"], ptr(dg), ptr(keep),
                                                   stream()) == 0
        else:
            assert L.nerf_packed_visibility(*head, kw["eps"], kw["athr"], ptr(keep), stream()) == 0
        want, decided = R.visibility(case, **kw)
        got = keep.cpu().numpy()
        assert got[M] == R.ISENT and np.isin(got[:M], (0, 1)).all()
        assert np.array_equal(got[:M][decided].astype(bool), want[decided]), (name, kw.get("group"))
        left += int((~decided).sum())
        total += M
        # compaction of what the device kept
        pos, rri, r0, r1, rc = R.compact(got[:M], ri, case["t0"], case["t1"], N)
        m = len(rri)
        dpos = _d(pos)
        for with_counts in (True, False):
            ro, t0o, t1o = _full(M + 1, R.ISENT, I32), _full(M + 1, R.SENT), _full(M + 1, R.SENT)
            cnt = torch.zeros(N + 1, dtype=I32, device=DEV)
            cnt[N] = R.ISENT
            assert L.nerf_packed_compact(ptr(keep), ptr(dpos), M, ptr(dri), ptr(dv["t0"]), ptr(dv["t1"]), ptr(ro),
                                         ptr(t0o), ptr(t1o), ptr(cnt) if with_counts else None, stream()) == 0
            assert np.array_equal(ro.cpu().numpy()[:m], rri) and _keeps(ro, m, R.ISENT)
            assert R.same_bits(t0o[:m], r0) and R.same_bits(t1o[:m], r1)
            assert _keeps(t0o, m, R.SENT) and _keeps(t1o, m, R.SENT)
            assert np.array_equal(cnt.cpu().numpy()[:N], rc if with_counts else np.zeros(N, np.int32))
            assert int(cnt[N]) == R.ISENT
    print(f"visibility {name}: {left} of {total} decisions left out")
    assert left <= 0.01 * total
    assert L.nerf_packed_visibility_groups(ptr(dv["t0"]), ptr(dv["t1"]), ptr(sig), ptr(dv["offs"]), N, 0, 1e-2, 0.0,
                                           ptr(sig), ptr(dri), stream()) == -1
    assert L.nerf_packed_visibility_groups(ptr(dv["t0"]), ptr(dv["t1"]), ptr(sig), ptr(dv["offs"]), N, 1, 1e-2, 0.0,
                                           None, ptr(dri), stream()) == -1


def test_packed_points_and_device_count():
    """nerf_packed_points over M and nerf_packed_points_n over *m_dev in {0, 1, 255, 256, 257, capacity, more}."""
    L, ptr, stream = _api()
    case = R.packed_case("N5")
    cap = R.POINT_CAPACITY
    rs = np.random.RandomState(3)
    rays = rs.randn(case["N"], 8).astype(np.float32)
    ri = np.repeat(np.arange(case["N"]), np.diff(case["offs"])).astype(np.int32)[:cap]
    t0, t1 = case["t0"][:cap], case["t1"][:cap]
    x, bound, dirs = R.packed_points(rays, ri, t0, t1)
    drays, dri, dt0, dt1 = _d(rays), _d(ri), _d(t0), _d(t1)
    worst = 0.0
    for count in R.POINT_COUNTS + [cap, cap + 1000]:
        n = min(count, cap)
        for by_device in (False, True):
            if count > cap and not by_device:
                continue
            xd = _full((cap + 1, 6), R.SENT)
            if by_device:
                m_dev = torch.tensor([count], dtype=I32, device=DEV)
                rc = L.nerf_packed_points_n(ptr(drays), ptr(dri), ptr(dt0), ptr(dt1), cap, ptr(m_dev), ptr(xd), stream())
            else:
                rc = L.nerf_packed_points(ptr(drays), ptr(dri), ptr(dt0), ptr(dt1), n, ptr(xd), stream())
            assert rc == 0 and _keeps(xd, n, R.SENT), (count, by_device)
            if n:
                worst = max(worst, R.worst_ratio(xd[:n, :3], x[:n], bound[:n]))
                assert R.same_bits(xd[:n, 3:].contiguous(), dirs[:n]), (count, by_device)
    print(f"packed points: worst error / bound {worst:.4f}")
    assert worst <= 1.0
    assert L.nerf_packed_points_n(ptr(drays), ptr(dri), ptr(dt0), ptr(dt1), cap, None, ptr(xd), stream()) == -1


@pytest.mark.parametrize("n", R.ELEMENTWISE_N)
def test_ray_counts_and_scan(n):
    L, ptr, stream = _api()
    rs = np.random.RandomState(n % 1000)
    N = max(1, n // 7)
    ri = np.sort(rs.randint(0, N, n)).astype(np.int32)
    counts = _full(N + 1, R.ISENT, I32)
    dri = _d(ri)
    assert L.nerf_ray_counts(ptr(dri), n, N, ptr(counts), stream()) == 0
    want = R.ray_counts(ri, N)
    assert np.array_equal(counts.cpu().numpy()[:N], want) and int(counts[N]) == R.ISENT
    out = _full(N + 8, R.ISENT, I32)
    wsb = int(L.nerf_scan_workspace_bytes(N))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dc = _d(want)
    assert L.nerf_exclusive_scan_i32(ptr(dc), N, ptr(out), ptr(ws), wsb, stream()) == 0
    assert np.array_equal(out.cpu().numpy()[:N + 1], R.exclusive_scan(want)) and _keeps(out, N + 1, R.ISENT)


# ================================================================================================= occupancy update chain

@pytest.mark.parametrize("n", R.ELEMENTWISE_N)
def test_update_threshold_binarize(n):
    L, ptr, stream = _api()
    rs = np.random.RandomState(n % 1000 + 1)
    total = 2 * n + 3
    occs = (rs.rand(total) ** 2).astype(np.float32)
    occs[rs.rand(total) < 0.2] = -1.0
    cells = rs.permutation(total)[:n].astype(np.int32)                  # distinct cells
    cells[rs.rand(n) < 0.1] = -1
    vals = (rs.rand(n) * 1.2).astype(np.float32)
    docc, dcells, dvals = _padded(occs, R.SENT), _d(cells), _d(vals)
    assert L.nerf_occ_update(ptr(docc), ptr(dcells), ptr(dvals), n, 0.95, stream()) == 0
    want = R.occ_update(occs, cells, vals, 0.95)
    assert R.same_bits(docc[:total], want) and float(docc[total]) == R.SENT
    assert ((occs == -1) == (want == -1)).all()
    # threshold over n cells, in the three kinds, binding and not binding
    nf = int(L.nerf_occ_threshold_floats())
    assert nf >= 4 + 2 * 3 * 256
    for kind in ("visible", "some_invisible", "all_invisible"):
        o = R.threshold_input(n, kind)
        do = _padded(o, R.SENT)
        for occ_thre in (0.01, 1e9):
            thre = _full(nf + 2, R.SENT)
            assert L.nerf_occ_threshold(ptr(do), n, occ_thre, ptr(thre), stream()) == 0
            got = thre.cpu().numpy()
            w0, w1 = R.threshold64(o, occ_thre)
            assert R.ulp_apart(got[0], w0) and R.ulp_apart(got[1], w1), (kind, occ_thre, got[:2], w0, w1)
            assert (got[2:4] == R.SENT).all() and (got[nf:] == R.SENT).all()
            if kind == "all_invisible":
                assert got[0] == 0.0 and got[1] == -1.0
            b = _full(n + 1, 7, torch.uint8)
            assert L.nerf_occ_binarize(ptr(do), n, ptr(thre), ptr(b), stream()) == 0
            assert np.array_equal(b.cpu().numpy()[:n], R.binarize(o, got[0])) and int(b[n]) == 7


def test_update_duplicated_cell_takes_one_of_its_values():
    L, ptr, stream = _api()
    occs = np.array([0.5, 0.25, -1.0, 0.0], dtype=np.float32)
    cells = np.array([1, 1, 2, 2, 3], dtype=np.int32)
    vals = np.array([0.75, 0.5, 3.0, 4.0, 0.125], dtype=np.float32)
    docc, dcells, dvals = _d(occs), _d(cells), _d(vals)
    assert L.nerf_occ_update(ptr(docc), ptr(dcells), ptr(dvals), 5, 0.5, stream()) == 0
    got = docc.cpu().numpy()
    assert got[0] == 0.5 and got[1] in (0.75, 0.5) and got[2] == -1.0 and got[3] == 0.125


@pytest.mark.parametrize("k", range(len(R.CELL_GRIDS)))
def test_cell_points(k):
    L, ptr, stream = _api()
    g = R.CELL_GRIDS[k]
    worst = 0.0
    for n in (1, 255, 257):
        cells = R.cell_points_input(g, max(n, 3), k)[:n]
        x = _full((n + 1, 3), R.SENT)
        gs, dcells = _grid(g), _d(cells)
        assert L.nerf_occ_cell_points(_addr(gs), ptr(dcells), n, U64(21), ptr(x), stream()) == 0
        ref, bound, lo, hi = R.cell_points(g, cells, 21)
        got = x.cpu().numpy()
        assert (got[n] == R.SENT).all()
        live = cells >= 0
        assert (got[:n][~live] == ref[~live]).all()                      # empty slots: the ROI centre exactly
        assert ((got[:n] >= lo) & (got[:n] <= hi)).all()
        if live.any():
            worst = max(worst, R.worst_ratio(got[:n][live], ref[live], bound[live]))
    print(f"cell points L={g['L']}: worst error / bound {worst:.4f}")
    assert worst <= 1.0


def _sample_cells(flags, L_, cpl, n, seed):
    L, ptr, stream = _api()
    pos = R.exclusive_scan(flags)
    occ_list = np.flatnonzero(flags).astype(np.int32)
    dl, dp = _padded(occ_list, R.ISENT), _d(pos)
    cells = _full(L_ * 2 * n + 1, R.ISENT, I32)
    assert L.nerf_occ_sample_cells(ptr(dl), ptr(dp), L_, cpl, n, U64(seed), ptr(cells), stream()) == 0
    got = cells.cpu().numpy()
    assert got[-1] == R.ISENT
    return got[:-1], R.sample_cells_reference(occ_list, pos[::cpl], cpl, n, seed)


@pytest.mark.parametrize("R_", [16, 64])
def test_sample_cells_bitwise(R_):
    """Both halves of the draw, as bytes, at 16^3 and 64^3 cells per level with fewer than, exactly and more than n
    occupied cells: the draws of every grid up to R = 256 are what they have always been."""
    cpl, n = R_ ** 3, 100
    for occ0, occ1 in ((n // 2, 3 * n), (n, n + 1), (0, cpl)):
        flags = np.concatenate([R.sample_cells_input(cpl, occ0, 1), R.sample_cells_input(cpl, occ1, 2)])
        got, want = _sample_cells(flags, 2, cpl, n, 0xABCDEF0123)
        assert np.array_equal(got, want), (R_, occ0, occ1, np.flatnonzero(got != want)[:8])


def test_sample_cells_large_grid_reaches_every_cell():
    """cells_per_level = 2^27 (R = 512): a 24-bit uniform times the range is always a multiple of 8.  Every residue
    of the uniform cells mod 8 must occur, and the draws are the restated wide draw."""
    L, ptr, stream = _api()
    cpl, n = 1 << 27, 4096
    pos = torch.zeros(cpl + 1, dtype=I32, device=DEV)
    occ_list = _full(4, R.ISENT, I32)
    cells = _full(2 * n + 1, R.ISENT, I32)
    assert L.nerf_occ_sample_cells(ptr(occ_list), ptr(pos), 1, cpl, n, U64(5), ptr(cells), stream()) == 0
    got = cells.cpu().numpy()
    del pos
    assert got[-1] == R.ISENT and (got[n:2 * n] == -1).all()
    uni = got[:n]
    assert uni.min() >= 0 and uni.max() < cpl
    assert sorted(set((uni % 8).tolist())) == list(range(8))
    assert np.array_equal(uni, [R.draw_below(5, 0x51, j, cpl) for j in range(n)])


# ================================================================================================= mark invisible

@pytest.mark.parametrize("which", R.INVIS_CAMERAS)
@pytest.mark.parametrize("k", range(len(R.INVIS_GRIDS)))
def test_mark_invisible(k, which):
    """Visible cells keep what they held (values and earlier -1 alike), the others become -1; cells within the derived
    margin of near_plane or of the image border may go either way."""
    L, ptr, stream = _api()
    g = R.INVIS_GRIDS[k]
    n = g["L"] * g["R"] ** 3
    K, c2w = R.invisible_cameras(which)
    rs = np.random.RandomState(k)
    occs = rs.rand(n).astype(np.float32)
    occs[::11] = -1.0
    docc = _padded(occs, R.SENT)
    gs = _grid(g)
    dK, dc = (_d(K), _d(c2w)) if len(K) else (None, None)
    assert L.nerf_occ_mark_invisible(_addr(gs), ptr(dK), ptr(dc), len(K), R.INVIS_W, R.INVIS_H, R.INVIS_NEAR, ptr(docc),
                                     stream()) == 0
    got = docc.cpu().numpy()
    vis, decided = R.mark_invisible(g, K, c2w, R.INVIS_W, R.INVIS_H, R.INVIS_NEAR)
    assert got[n] == R.SENT
    assert R.same_bits(got[:n][vis], occs[vis]) and (got[:n][decided & ~vis] == -1.0).all()
    und = ~decided
    assert ((got[:n][und] == -1.0) | (got[:n][und] == occs[und])).all()
    print(f"mark_invisible grid {k} {which}: visible {vis.mean():.3f}, left out {und.mean():.4%}")
    assert und.mean() <= 0.02
    if which == "none":
        assert L.nerf_occ_mark_invisible(_addr(gs), None, None, 1, 8, 8, 0.1, ptr(docc), stream()) == -1
        assert L.nerf_occ_mark_invisible(_addr(gs), None, None, 0, 0, 8, 0.1, ptr(docc), stream()) == -1
