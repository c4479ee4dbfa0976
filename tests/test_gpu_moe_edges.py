"""The MoE container kernels (csrc/moe.hip) at their block, wave and capacity edges, through the C entry points, against
the plain-torch CPU references of tests/moe_reference.py (checked on the CPU by tests/test_moe_reference.py).
Run on an MI355X: -m gpu.

Integer and fp32-restatable operations are compared exactly; operations through a divide, a square root or expf are
compared with a float64 reference under the bound derived in moe_reference's docstring, and each such test prints
the worst ratio of error to bound before it asserts ratio <= 1.  Every output buffer is pre-filled with a sentinel
and everything the kernel should not write must keep it."""
import ctypes

import pytest
import torch

import moe_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _api():
    from nerf_amd._lib import lib, ptr, stream
    return lib(), ptr, stream


def _d(t):
    return t.to(DEV).contiguous()


def _full(shape, value, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device=DEV)


def _i32(*v):
    return torch.tensor(v, dtype=I32, device=DEV)


# ================================================================================================= dispatch

def _dispatch(W, K, eps, count=None):
    """-> (offsets (K+1), idx (M K, sentinel where unwritten)) on the CPU."""
    L, ptr, stream = _api()
    M = W.shape[0]
    offs = _full(K + 1, R.ISENT, I32)
    idx = _full(max(M * K, 1), R.ISENT, I32)
    wsb = int(L.nerf_moe_dispatch_workspace_bytes(M, K))
    assert wsb >= -(-M // 256) * K * 4 + 128
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    if count is None:
        rc = L.nerf_moe_dispatch(ptr(W), M, K, eps, ptr(offs), ptr(idx), ptr(ws), wsb, stream())
    else:
        m_dev = _i32(count)
        rc = L.nerf_moe_dispatch_n(ptr(W), M, ptr(m_dev), K, eps, ptr(offs), ptr(idx), ptr(ws), wsb, stream())
    assert rc == 0
    return offs.cpu(), idx.cpu()


def _check_dispatch(got, ref, what):
    (offs, idx), (roffs, ridx) = got, ref
    assert torch.equal(offs, roffs), what
    n = int(roffs[-1])
    assert torch.equal(idx[:n], ridx), what
    assert bool((idx[n:] == R.ISENT).all()), what             # nothing written past offsets[K]


@pytest.mark.parametrize("K", R.DISPATCH_K)
@pytest.mark.parametrize("M", R.DISPATCH_M)
def test_dispatch_vs_nonzero_order(M, K):
    """M = 65793 is 257 blocks + 1 row: the scan's threads own runs of 2 blocks (the carry between the runs), the
    trailing threads own none, and the write kernel's fourth-wave prefix runs at scale."""
    for eps in R.DISPATCH_EPS:
        W = R.dispatch_weights(M, K, eps)
        _check_dispatch(_dispatch(_d(W), K, eps), R.dispatch_reference(W, eps), (M, K, eps))


@pytest.mark.parametrize("count", R.DISPATCH_COUNTS)
def test_dispatch_device_count(count):
    """nerf_moe_dispatch_n at capacity 65793: rows at and past the count hold weights above eps and route nowhere; a
    count above the capacity acts as the capacity."""
    cap, eps = R.DISPATCH_CAP, 1e-8
    for K in ((3, 32) if count == 257 else (3,)):
        W = R.dispatch_weights(cap, K, eps).clone()
        W[min(count, cap):] = 0.5
        _check_dispatch(_dispatch(_d(W), K, eps, count=count), R.dispatch_reference(W, eps, count=count), (count, K))


def test_dispatch_zero_rows_and_errors():
    L, ptr, stream = _api()
    for K in (1, 32):
        offs = _full(K + 3, R.ISENT, I32)
        assert L.nerf_moe_dispatch(None, 0, K, 0.0, ptr(offs), None, None, 0, stream()) == 0
        assert offs.cpu().tolist() == [0] * (K + 1) + [R.ISENT] * 2
    W = _d(R.dispatch_weights(257, 3, 0.0))
    offs, idx = _full(40, R.ISENT, I32), _full(257 * 33, R.ISENT, I32)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    m = _i32(100)
    assert L.nerf_moe_dispatch(ptr(W), 257, 33, 0.0, ptr(offs), ptr(idx), ptr(ws), ws.numel(), stream()) == -1
    assert L.nerf_moe_dispatch_n(ptr(W), 257, ptr(m), 33, 0.0, ptr(offs), ptr(idx), ptr(ws), ws.numel(), stream()) == -1
    assert L.nerf_moe_dispatch_n(ptr(W), 257, None, 3, 0.0, ptr(offs), ptr(idx), ptr(ws), ws.numel(), stream()) == -1
    need = 2 * 3 * 4 + 32 * 4                                     # 2 blocks' counts and the totals
    short = need - 3 * 4                                          # one block's counts too small
    assert L.nerf_moe_dispatch(ptr(W), 257, 3, 0.0, ptr(offs), ptr(idx), ptr(ws), short, stream()) == -4
    assert L.nerf_moe_dispatch_n(ptr(W), 257, ptr(m), 3, 0.0, ptr(offs), ptr(idx), ptr(ws), short, stream()) == -4
    assert L.nerf_moe_dispatch(ptr(W), 257, 3, 0.0, ptr(offs), ptr(idx), ptr(ws), need, stream()) == 0
    torch.cuda.synchronize()
    assert bool((offs == R.ISENT).sum() == 40 - 4)                # the refused calls wrote nothing, the last one K + 1


# ================================================================================================= gather & co.

@pytest.mark.parametrize("cols", R.GATHER_COLS)
def test_gather_rows_pitches(cols):
    L, ptr, stream = _api()
    g = R.gen(cols)
    src = torch.randn(97, cols + 2, generator=g)
    dsrc = _d(src)
    for n in R.rows_at_block_edge(cols):
        idx = torch.randint(0, 97, (n,), generator=g).to(I32)
        dst = torch.full((n + 2, cols + 1), R.SENT)
        out, didx = _d(dst), _d(idx)
        assert L.nerf_gather_rows(ptr(dsrc), cols + 2, ptr(didx), n, cols, ptr(out), cols + 1, stream()) == 0
        assert R.same_bits(out, R.gather_reference(src, idx, n, cols, dst)), (cols, n)


@pytest.mark.parametrize("cols,cap", [(6, R.GATHER_CAP), (1, 300), (4, 65)])
def test_gather_rows_device_range(cols, cap):
    """nerf_gather_rows_rng: 200,000 x 6 elements are more than the 4096 x 256 threads of its bounded grid (the
    grid-stride loop); an empty or reversed range leaves the destination untouched, a range longer than the capacity
    is clamped to it."""
    L, ptr, stream = _api()
    g = R.gen(100 + cols)
    src = torch.randn(4096, 8, generator=g)
    idx = torch.randint(0, 4096, (cap + 7,), generator=g).to(I32)
    dsrc, didx = _d(src), _d(idx)
    dst = torch.full((cap + 1, cols + 1), R.SENT)
    for rng, n, first in R.rng_cases(cap):
        out, drng = _d(dst), _i32(*rng)
        assert L.nerf_gather_rows_rng(ptr(dsrc), 8, ptr(didx), ptr(drng), cap, cols, ptr(out), cols + 1,
                                      stream()) == 0
        assert R.same_bits(out, R.gather_reference(src, idx[first:], n, cols, dst)), (cols, rng)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_flag_compact_and_scatter_counts(n):
    L, ptr, stream = _api()
    flags, pos = R.flags_input(n)
    idx, dflags, dpos = _full(n + 2, R.ISENT, I32), _d(flags), _d(pos)
    assert L.nerf_flag_compact(ptr(dflags), ptr(dpos), n, ptr(idx), stream()) == 0
    ref = flags.nonzero().squeeze(1).to(I32)
    assert torch.equal(idx.cpu()[:ref.numel()], ref) and bool((idx.cpu()[ref.numel():] == R.ISENT).all())
    g = R.gen(200 + n)
    hit = torch.randperm(2 * n + 3, generator=g)[:n].sort().values.to(I32)
    cnt_k = torch.randint(0, 1000, (n,), generator=g).to(I32)
    cnt, dhit, dcnt_k = _full(2 * n + 3, R.ISENT, I32), _d(hit), _d(cnt_k)
    assert L.nerf_scatter_counts(ptr(dhit), ptr(dcnt_k), n, ptr(cnt), stream()) == 0
    want = torch.full((2 * n + 3,), R.ISENT, dtype=I32)
    want[hit.long()] = cnt_k
    assert torch.equal(cnt.cpu(), want)


# ================================================================================================= mix

@pytest.mark.parametrize("K", R.MIX_K)
@pytest.mark.parametrize("C", R.MIX_C)
def test_mix_bitwise(C, K):
    """nerf_moe_combine in expert order gives the bits of the fp32 out = out + y * w (no fma contraction), and
    nerf_moe_combine_bwd those of dout * w."""
    L, ptr, stream = _api()
    for M in R.rows_at_block_edge(C):
        for one_hot in (False, True):
            W, sels, ys = R.mix_case(M, C, K, one_hot)
            dW = _d(W)
            out = torch.zeros(M + 1, C, device=DEV)
            out[M] = R.SENT
            dout = torch.randn(M, C, generator=R.gen(M + C + K))
            ddout = _d(dout)
            for k, (sel, y) in enumerate(zip(sels, ys)):
                n = sel.numel()
                dsel, dy_in = _d(sel), _d(y)
                assert L.nerf_moe_combine(ptr(dy_in), n, C, ptr(dsel), ptr(dW), K, k, ptr(out), stream()) == 0
                dy = _full((n + 1, C), R.SENT)
                assert L.nerf_moe_combine_bwd(ptr(ddout), n, C, ptr(dsel), ptr(dW), K, k, ptr(dy), stream()) == 0
                want = torch.cat([R.mix_bwd_reference(W, sel, k, dout), torch.full((1, C), R.SENT)])
                assert R.same_bits(dy, want), (M, C, K, one_hot, k)
            want = torch.cat([R.mix_reference(W, sels, ys, C), torch.full((1, C), R.SENT)])
            assert R.same_bits(out, want), (M, C, K, one_hot)


# ================================================================================================= blend

def _blend_device(case, ranged):
    """s, c after all experts through nerf_moe_blend, or through nerf_moe_blend_rng on the packed expert-major idx
    with one capacity-sized y buffer."""
    L, ptr, stream = _api()
    M, K = case["M"], case["K"]
    dW = _d(case["W"])
    s, c = torch.zeros(M + 1, device=DEV), torch.zeros(M + 1, 3, device=DEV)
    s[M], c[M] = R.SENT, R.SENT
    packed = _d(torch.cat(case["sels"] + [torch.zeros(1, dtype=I32)]))
    off = 0
    for k, (sel, y) in enumerate(zip(case["sels"], case["ys"])):
        n = sel.numel()
        if ranged:
            cap = M
            buf, drng = _full((cap, 4), R.SENT), _i32(off, off + n)
            buf[:n] = _d(y)
            assert L.nerf_moe_blend_rng(ptr(buf), cap, ptr(packed), ptr(drng), ptr(dW), K, k, ptr(s), ptr(c),
                                        stream()) == 0
        else:
            dy_in, dsel = _d(y), _d(sel)
            assert L.nerf_moe_blend(ptr(dy_in), n, ptr(dsel), ptr(dW), K, k, ptr(s), ptr(c), stream()) == 0
        off += n
    return s, c


@pytest.mark.parametrize("shift", range(5))
@pytest.mark.parametrize("K", R.BLEND_K)
def test_blend_accumulate_finish_backward(K, shift):
    """Accumulation: bits of the fp32 restatement (host-sized and ranged).  Finish: 2^-23 relative on rgb, sigma exact,
    rows past a device count untouched.  Backward: float64 autograd under (3 K + 9) 2^-23 sum |terms|, the s = 0 row
    (not live, gradients of order 1e12) and the s == 1e-12f row (live) included; the ranged form gives the same bits."""
    L, ptr, stream = _api()
    case = R.blend_case(K, shift)
    M = case["M"]
    rs_, rc_ = R.blend_accumulate(case)
    s, c = _blend_device(case, False)
    for ranged in (False, True):
        s2, c2 = (s, c) if not ranged else _blend_device(case, True)
        assert R.same_bits(s2[:M], rs_) and R.same_bits(c2[:M], rc_), (K, shift, ranged)
        assert float(s2[M]) == R.SENT and bool((c2[M] == R.SENT).all())
    rs = _full((M + 1, 4), R.SENT)
    assert L.nerf_moe_blend_finish(ptr(s), ptr(c), M, ptr(rs), stream()) == 0
    ratio, sigma_exact = R.finish_ratio(rs[:M].cpu(), rs_, rc_)
    print(f"blend finish K={K} shift={shift}: worst |rgb - rgb64| / (2^-23 |rgb64|) = {ratio:.4f}")
    assert ratio <= 1.0 and sigma_exact and bool((rs[M] == R.SENT).all())
    for count in (0, 1, 257, M, M + 1000):
        rn, m_dev = _full((M + 1, 4), R.SENT), _i32(count)
        assert L.nerf_moe_blend_finish_n(ptr(s), ptr(c), M, ptr(m_dev), ptr(rn), stream()) == 0
        n = min(count, M)
        assert R.same_bits(rn[:n], rs[:n]) and bool((rn[n:] == R.SENT).all()), count
    # backward, fed with the device's own saved s and mix as in the product
    g = R.blend_upstream(M)
    dg, dW = _d(g), _d(case["W"])
    ref, bound = R.blend_bwd_autograd(case, g), R.blend_bwd_bound(case, g)
    packed = _d(torch.cat(case["sels"] + [torch.zeros(1, dtype=I32)]))
    worst, off = 0.0, 0
    for k, (sel, y) in enumerate(zip(case["sels"], case["ys"])):
        n = sel.numel()
        dy, dy_in, dsel = _full((n + 1, 4), R.SENT), _d(y), _d(sel)
        assert L.nerf_moe_blend_bwd(ptr(dy_in), n, ptr(dsel), ptr(dW), K, k, ptr(s), ptr(rs), ptr(dg), ptr(dy),
                                    stream()) == 0
        assert bool((dy[n] == R.SENT).all()) and bool(torch.isfinite(dy).all())
        worst = max(worst, R.worst_ratio(dy[:n], ref[k], bound[k]))
        buf, dy2, drng = _full((M, 4), R.SENT), _full((M, 4), R.SENT), _i32(off, off + n)
        buf[:n] = dy_in
        assert L.nerf_moe_blend_bwd_rng(ptr(buf), M, ptr(packed), ptr(drng), ptr(dW), K, k, ptr(s), ptr(rs), ptr(dg),
                                        ptr(dy2), stream()) == 0
        assert R.same_bits(dy2[:n], dy[:n]) and bool((dy2[n:] == R.SENT).all()), k
        off += n
    print(f"blend backward K={K} shift={shift}: worst error / ({R.BLEND_BWD_K(K)} 2^-23 sum|terms|) = {worst:.4f}")
    assert worst <= 1.0


def test_blend_device_range_edges():
    """nerf_moe_blend_rng / nerf_moe_blend_bwd_rng with the full, shifted, empty, reversed and over-long ranges."""
    L, ptr, stream = _api()
    cap, M, K, k = 257, 600, 4, 2
    g = R.gen(301)
    idx = torch.randperm(M, generator=g)[:cap + 7].to(I32)       # distinct rows: a launch never meets a row twice
    y = torch.cat([torch.rand(cap, 3, generator=g), torch.rand(cap, 1, generator=g) + 0.1], 1)
    W = torch.rand(M, K, generator=g) + 0.05
    s0, c0 = torch.rand(M, generator=g) + 0.5, torch.rand(M, 3, generator=g)
    rs = R.blend_finish_fp32(s0, c0)
    up = R.blend_upstream(M)
    dy_, didx, dW, ds0, drs, dup = _d(y), _d(idx), _d(W), _d(s0), _d(rs), _d(up)
    for rng, n, first in R.rng_cases(cap):
        sel = idx[first:first + n]
        s, c = _d(s0), _d(c0)
        drng = _i32(*rng)
        assert L.nerf_moe_blend_rng(ptr(dy_), cap, ptr(didx), ptr(drng), ptr(dW), K, k, ptr(s), ptr(c), stream()) == 0
        i = sel.long()
        ws = W[i, k] * y[:n, 3]
        ws_s, ws_c = s0.clone(), c0.clone()
        ws_s[i] = ws_s[i] + ws
        ws_c[i] = ws_c[i] + ws[:, None] * y[:n, :3]
        assert R.same_bits(s, ws_s) and R.same_bits(c, ws_c), rng
        dy = _full((cap + 1, 4), R.SENT)
        assert L.nerf_moe_blend_bwd_rng(ptr(dy_), cap, ptr(didx), ptr(drng), ptr(dW), K, k, ptr(ds0), ptr(drs),
                                        ptr(dup), ptr(dy), stream()) == 0
        want, dsel = _full((cap + 1, 4), R.SENT), _d(sel)         # the host-sized backward on the same rows
        assert L.nerf_moe_blend_bwd(ptr(dy_), n, ptr(dsel), ptr(dW), K, k, ptr(ds0), ptr(drs), ptr(dup), ptr(want),
                                    stream()) == 0
        assert R.same_bits(dy, want), rng
        assert bool((dy[n:] == R.SENT).all()) and (n == 0 or bool((dy[:n] != R.SENT).any())), rng


# ================================================================================================= segment union

def _union_run(inp, layout):
    L, ptr, stream = _api()
    K, segs = inp["K"], inp["segs"]
    N = len(segs)
    packed = R.union_pack(segs, K)
    keep = []
    if layout == "separate":
        t0d, t1d, ofd = [_d(p[0]) for p in packed], [_d(p[1]) for p in packed], [_d(p[2]) for p in packed]
        keep = [t0d, t1d, ofd]
        # an expert without any segment: a one-element array (never read) in place of a null pointer
        t0d = [t if t.numel() else _full(1, R.SENT) for t in t0d]
        t1d = [t if t.numel() else _full(1, R.SENT) for t in t1d]
        p0, p1, po = [t.data_ptr() for t in t0d], [t.data_ptr() for t in t1d], [t.data_ptr() for t in ofd]
        keep += [t0d, t1d]
    else:  # one shared packed array, offsets (K N + 1) expert-major, expert k's slice starting at k N
        t0a, t1a = _d(torch.cat([p[0] for p in packed])), _d(torch.cat([p[1] for p in packed]))
        base, offs = 0, []
        for p in packed:
            offs.append(p[2][:-1] + base)
            base += int(p[2][-1])
        ofa = _d(torch.cat(offs + [torch.tensor([base], dtype=I32)]))
        keep = [t0a, t1a, ofa]
        p0, p1 = [t0a.data_ptr()] * K, [t1a.data_ptr()] * K
        po = [ofa[k * N:].data_ptr() for k in range(K)]
    a0, a1, ao = [(ctypes.c_void_p * K)(*p) for p in (p0, p1, po)]
    counts = _full(N + 2, R.ISENT, I32)
    assert L.nerf_segments_union(a0, a1, ao, K, N, ptr(counts), None, None, None, None, stream()) == 0
    counts = counts.cpu()
    total = int(counts[:N].sum())
    off = torch.zeros(N + 1, dtype=I32)
    off[1:] = torch.cumsum(counts[:N], 0).to(I32)
    ri, t0, t1 = _full(total + 64, R.ISENT, I32), _full(total + 64, R.SENT), _full(total + 64, R.SENT)
    doff = _d(off)
    assert L.nerf_segments_union(a0, a1, ao, K, N, None, ptr(doff), ptr(ri), ptr(t0), ptr(t1), stream()) == 0
    torch.cuda.synchronize()
    del keep
    return counts, ri.cpu(), t0.cpu(), t1.cpu()


@pytest.mark.parametrize("layout", ["separate", "shared"])
@pytest.mark.parametrize("K", R.UNION_K)
def test_segments_union_both_algorithms(K, layout):
    """About 40 rays in one launch with 0 .. 4098 boundary entries: the LDS bitonic path up to 2048, the sequential
    merge on lane 0 above; counts, ray indices, t0 and t1 exactly those of torch.unique per ray."""
    inp = R.union_input(K)
    N = len(inp["segs"])
    rc, rri, rt0, rt1 = R.union_reference(inp["segs"])
    # the reference must not depend on the count pass it is compared with
    counts, ri, t0, t1 = _union_run(inp, layout)
    assert torch.equal(counts[:N], rc) and counts[N:].tolist() == [R.ISENT] * 2
    n = int(rc.sum())
    assert torch.equal(ri[:n], rri) and R.same_bits(t0[:n], rt0) and R.same_bits(t1[:n], rt1)
    assert bool((ri[n:] == R.ISENT).all()) and bool((t0[n:] == R.SENT).all()) and bool((t1[n:] == R.SENT).all())
    if inp["pair"]:
        lo, hi = inp["pair"]                                     # the same boundaries through both algorithms
        off = torch.cumsum(rc, 0) - rc
        a, b, m = int(off[lo]), int(off[hi]), int(rc[lo])
        assert int(counts[lo]) == int(counts[hi]) == m
        assert R.same_bits(t0[a:a + m], t0[b:b + m]) and R.same_bits(t1[a:a + m], t1[b:b + m])


def test_segments_union_expert_limit():
    L, ptr, stream = _api()
    t = _full(4, 1.0)
    off = torch.zeros(3, dtype=I32, device=DEV)
    arr = (ctypes.c_void_p * 9)(*([t.data_ptr()] * 9))
    ofs = (ctypes.c_void_p * 9)(*([off.data_ptr()] * 9))
    counts = _full(2, R.ISENT, I32)
    assert L.nerf_segments_union(arr, arr, ofs, 9, 2, ptr(counts), None, None, None, None, stream()) == -1
    assert L.nerf_segments_union(arr, arr, ofs, 0, 2, ptr(counts), None, None, None, None, stream()) == -1
    assert L.nerf_segments_union(arr, arr, ofs, 8, 2, ptr(counts), None, None, None, None, stream()) == 0
    assert counts.cpu().tolist() == [0, 0]


# ================================================================================================= AABB prefilter

def _hits(rays, box):
    L, ptr, stream = _api()
    n = rays.shape[0]
    hit, drays = _full(n + 2, R.ISENT, I32), _d(rays)
    assert L.nerf_rays_aabb_hit(ptr(drays), n, (ctypes.c_float * 6)(*box), ptr(hit), stream()) == 0
    hit = hit.cpu()
    assert hit[n:].tolist() == [R.ISENT] * 2
    return hit[:n]


@pytest.mark.parametrize("N", R.AABB_N)
def test_aabb_prefilter_random(N):
    rays = R.aabb_rays()[:N]
    keep = R.aabb_keep(rays, R.AABB_BOX)
    want = (R.aabb_margin64(rays, R.AABB_BOX) > 0).to(I32)
    hit = _hits(rays, R.AABB_BOX)
    assert bool(((hit == 0) | (hit == 1)).all())
    assert torch.equal(hit[keep], want[keep])


def test_aabb_prefilter_constructed():
    rays, want = R.aabb_exact_rays()
    got = _hits(rays, R.AABB_EXACT_BOX)
    assert torch.equal(got, want), (got != want).nonzero().squeeze(1).tolist()


# ================================================================================================= routing

def _route(x, cen, margin, c2d, count=None):
    """x: a device view (M, 3) whose row pitch is x.stride(0)."""
    L, ptr, stream = _api()
    M, K = x.shape[0], cen.shape[0]
    W = _full((M + 1, K), R.SENT)
    c = (ctypes.c_float * (3 * K))(*cen.reshape(-1).tolist())
    if count is None:
        rc = L.nerf_moe_route(ptr(x), x.stride(0), M, c, K, int(c2d), margin, ptr(W), stream())
    else:
        m_dev = _i32(count)
        rc = L.nerf_moe_route_n(ptr(x), x.stride(0), M, ptr(m_dev), c, K, int(c2d), margin, ptr(W), stream())
    assert rc == 0
    W = W.cpu()
    assert bool((W[M] == R.SENT).all())
    return W[:M]


def _pitched(pts, pitch):
    buf = _full((pts.shape[0], pitch), R.SENT)
    buf[:, :3] = _d(pts)
    return buf[:, :3]


@pytest.mark.parametrize("c2d", [0, 1])
@pytest.mark.parametrize("K", R.ROUTE_K)
def test_route_vs_float64(K, c2d):
    pts, cen = R.route_input(K)
    worst = worst_left = 0.0
    for margin in R.ROUTE_SOFT + R.ROUTE_HARD:
        for M in R.ROUTE_M:
            for pitch in (3, 6):
                got = _route(_pitched(pts[:M], pitch), cen, margin, c2d)
                ratio, zero_ok, left = R.route_ratio(got, pts[:M], cen, margin, bool(c2d))
                assert ratio <= 1.0 and zero_ok, (K, c2d, margin, M, pitch, ratio)
                if M == 4099:
                    assert left <= 0.005
                    worst_left = max(worst_left, left)
                worst = max(worst, ratio)
    print(f"routing K={K} cluster_2d={c2d}: worst |w - w64| / ((K + 8) 2^-24 w64) = {worst:.4f}, "
          f"largest share of rows left out {worst_left:.4%}")


@pytest.mark.parametrize("c2d", [0, 1])
def test_route_constructed_rows(c2d):
    for margin in R.ROUTE_SOFT + R.ROUTE_HARD:
        got = _route(_d(R.ROUTE_EXACT_PTS), R.ROUTE_EXACT_CEN, margin, c2d)
        for r, row in enumerate(R.route_exact_expect(margin, bool(c2d))):
            if row is not None:
                assert R.same_bits(got[r], torch.tensor(row, dtype=torch.float32)), (c2d, margin, r, got[r].tolist())


@pytest.mark.parametrize("count", R.ROUTE_COUNTS)
def test_route_device_count(count):
    """nerf_moe_route_n: rows below the count as nerf_moe_route, rows at and past it all zero."""
    for K, margin, c2d in ((3, 1.05, 1), (32, 1.0, 0)):
        pts, cen = R.route_input(K)
        x = _pitched(pts, 6)
        n = min(count, pts.shape[0])
        got = _route(x, cen, margin, c2d, count=count)
        assert R.same_bits(got[:n], _route(x, cen, margin, c2d)[:n]) and bool((got[n:] == 0).all()), (K, count)


# ================================================================================================= background MLP

def _bg_fwd(d, w, H):
    L, ptr, stream = _api()
    N = d.shape[0]
    out = _full((N + 1, 3), R.SENT)
    assert L.nerf_bg_mlp_fwd(ptr(d), d.stride(0), N, ptr(w), H, ptr(out), stream()) == 0
    assert bool((out[N] == R.SENT).all())
    return out[:N]


def _bg_bwd(d, w, H, g):
    L, ptr, stream = _api()
    N, P = d.shape[0], 20 * H + 3
    wsb = int(L.nerf_bg_mlp_workspace_bytes(N, H))
    assert wsb >= -(-max(N, 1) // 64) * P * 4
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dw = _full(P + 2, R.SENT)
    assert L.nerf_bg_mlp_bwd(ptr(d) if N else None, max(d.stride(0), 3), N, ptr(w), H, ptr(g) if N else None, ptr(dw),
                             ptr(ws), wsb, stream()) == 0
    assert dw[P:].tolist() == [R.SENT] * 2
    return dw[:P]


def _rays_view(d, pitch):
    """Directions at columns 3 .. 5 of ray rows of 8 floats (read in place), or packed (N, 3)."""
    if pitch == 3:
        return _d(d)
    buf = _full((d.shape[0], 8), R.SENT)
    buf[:, 3:6] = _d(d)
    return buf[:, 3:6]


@pytest.mark.parametrize("H", R.BG_H)
def test_bg_mlp_vs_float64(H):
    """Forward and packed weight gradient at H = 1, 32, 64 (BG_MAXH), N around the 64-ray block and the 256-thread
    workgroup, pitch 3 and 8, norms 1e-6 .. 1e3 and the zero vector."""
    dirs, _ = R.bg_directions(H)
    w = R.bg_weights(H)
    dw_ = _d(w)
    worst_f = worst_b = 0.0
    for N in R.BG_N:
        d, g = dirs[:N], R.bg_upstream(N)
        ref, bound = R.bg_fwd_bound(d, w, H)
        gref, gbound = R.bg_bwd_bound(d, w, H, g)
        outs, grads = [], []
        for pitch in (3, 8):
            dv = _rays_view(d, pitch)
            outs.append(_bg_fwd(dv, dw_, H).cpu())
            grads.append(_bg_bwd(dv, dw_, H, _d(g)).cpu())
            rf, rb = R.worst_ratio(outs[-1], ref, bound), R.worst_ratio(grads[-1], gref, gbound)
            assert rf <= 1.0 and rb <= 1.0, (H, N, pitch, rf, rb)
            worst_f, worst_b = max(worst_f, rf), max(worst_b, rb)
        assert R.same_bits(outs[0], outs[1]) and R.same_bits(grads[0], grads[1]), (H, N)
    print(f"background MLP H={H}: worst forward error / bound = {worst_f:.4f}, worst d_w error / bound = {worst_b:.4f}")


@pytest.mark.parametrize("H", R.BG_H)
def test_bg_mlp_bwd_deterministic_and_block_edge(H):
    dirs, _ = R.bg_directions(H)
    w = _d(R.bg_weights(H))
    g = R.bg_upstream(321)
    d321 = _d(dirs[:321])
    a, b = _bg_bwd(d321, w, H, _d(g)).cpu(), _bg_bwd(d321, w, H, _d(g)).cpu()
    assert R.same_bits(a, b)                                      # one slab per block, summed in order
    g65 = g[:65].clone()
    g65[64] = 0.0                                 # a 65th ray with a zero upstream gradient: a second block
    a, b = _bg_bwd(_d(dirs[:64]), w, H, _d(g[:64])).cpu(), _bg_bwd(_d(dirs[:65]), w, H, _d(g65)).cpu()
    assert R.same_bits(a, b)
    z = _bg_bwd(torch.zeros(0, 3, device=DEV), w, H, torch.zeros(0, 3, device=DEV))
    assert bool((z == 0).all())                                   # N = 0 zeroes d_w


def test_bg_mlp_errors():
    L, ptr, stream = _api()
    d, g = _d(R.bg_directions(32)[0][:65]), _d(R.bg_upstream(65))
    w = _d(R.bg_weights(64))
    out, dw = _full((65, 3), R.SENT), _full(20 * 64 + 3, R.SENT)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    for H in (0, 65):
        assert L.nerf_bg_mlp_fwd(ptr(d), 3, 65, ptr(w), H, ptr(out), stream()) == -1
        assert L.nerf_bg_mlp_bwd(ptr(d), 3, 65, ptr(w), H, ptr(g), ptr(dw), ptr(ws), ws.numel(), stream()) == -1
        assert int(L.nerf_bg_mlp_workspace_bytes(65, H)) == -1
    assert L.nerf_bg_mlp_fwd(ptr(d), 2, 65, ptr(w), 32, ptr(out), stream()) == -1
    short = (2 - 1) * (20 * 32 + 3) * 4                           # 65 rays are two slabs: one slab short
    assert L.nerf_bg_mlp_bwd(ptr(d), 3, 65, ptr(w), 32, ptr(g), ptr(dw), ptr(ws), short, stream()) == -4
    assert L.nerf_bg_mlp_bwd(ptr(d), 3, 65, ptr(w), 32, ptr(g), ptr(dw), ptr(ws), 2 * short, stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == R.SENT).all()) and bool((dw[643:] == R.SENT).all())
