"""The hash-grid table gradient on the device (-m gpu) where samples share cells: hash_bwd_kernel<F>,
hash_bwd_f2_kernel, hash_bwd_f2_agg_kernel (nerf_hash_encode_bwd) and the scatter inside ngp_bwd_prod_kernel<*, HB>
(nerf_ngp_bwd_hash, nerf_ngp_bwd_hash_n) against the float64 accumulation of the same fp32 terms in
tests/hash_scatter_reference.py, entry by entry, within k 2^-23 sum|t| (derived there; nothing here is measured).

The inputs are ray-major, t-sorted samples plus one point 40 times and the clamp / grid-node edge points
(hash_scatter_reference.build_input); tests/test_hash_scatter_reference.py checks on the CPU that they put runs of 2
to 16 lanes, full 16-lane runs and cells continuing across the 16-sample, tile and workgroup boundaries in front of the
segmented scan.  Every gradient is accumulated into a non-zero base; an entry no sample touches must keep its bits."""
import ctypes
import functools

import pytest
import torch

import hash_scatter_reference as H
from oracle import ngp_oracle as NO

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = float(torch.tensor(1e-6, dtype=torch.float32))
AABB = [v for p in H.BOX for v in p]


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import ngp
    return ngp


def _grid(N, grid, F, interp):
    levels, log2_T, mn, mx = grid
    res = H.resolutions(grid)
    assert torch.equal(N.level_resolutions(levels, mn, mx)[0], res)
    g = N.NerfHashGrid()
    g.levels, g.features_per_level, g.log2_hashmap_size, g.interpolation = levels, F, log2_T, N._INTERP[interp]
    for i, r in enumerate(res.tolist()):
        g.resolutions[i] = int(r)
    return g, res


def _judge(what, got, ref, base):
    """The per-entry bound, the untouched entries' bits and no NaN; prints the worst ratio to the bound."""
    sum64, abs64, count = ref
    assert not torch.isnan(got).any(), what
    ratio, untouched = H.bound_ratio(got, sum64, abs64, count, base)
    print(f"{what}: worst |got - sum64| / (k 2^-23 sum|t|) = {ratio:.4f}, largest k {int(count.max())}, "
          f"{int((count > 0).sum())} of {count.numel()} entries touched")
    assert untouched, f"{what}: an entry no sample touches changed"
    assert ratio <= 1.0, f"{what}: {ratio} bounds away from the float64 sum"
    return ratio


def _two_launch(N, what, x_dev, grid, F, interp, aabb=AABB, seed=0, forward=True):
    """nerf_hash_encode_bwd on x_dev (M, >= 3; any row pitch) into a non-zero base against the reference, and
    nerf_hash_encode on the same points against the fp32 oracle, bit for bit, with a wider out_stride too."""
    g, res = _grid(N, grid, F, interp)
    levels, log2_T = grid[0], grid[1]
    M, od, rows = x_dev.shape[0], levels * F, levels * 2 ** log2_T
    gen = torch.Generator().manual_seed(1000 + seed)
    d_out = torch.randn(M, od, generator=gen)
    base = torch.randn(rows, F, generator=gen) * 1e-3
    x_cpu = x_dev[:, :3].cpu()
    box = None if aabb is None else H.BOX
    got = base.to(DEV)
    assert N.hash_encode_bwd(g, x_dev, d_out.to(DEV), rows, aabb, EPS, d_table=got) is got
    torch.cuda.synchronize()
    ref = H.scatter_reference(x_cpu, d_out, res, log2_T, F, interp, box, EPS)
    _judge(what, got.cpu(), ref, base)
    if forward:
        table = torch.rand(rows, F, generator=gen) - 0.5
        want = NO.hash_encode(table, H.unit_points(x_cpu, box, EPS), res, log2_T, F, interp)
        out = N.hash_encode(g, table.to(DEV), x_dev, aabb, EPS)
        assert torch.equal(out.cpu(), want), what
        wide = N.hash_encode(g, table.to(DEV), x_dev, aabb, EPS, out_stride=od + 4).cpu()
        assert torch.equal(wide[:, :od], want) and not wide[:, od:].any(), what
    return ref


def _x(M=None, **kw):
    x = H.build_input(**kw)
    return x[:M if M is not None else x.shape[0]].to(DEV)


# ------------------------------------------------------------------------------------------- two-launch path

@pytest.mark.parametrize("interp", ["Linear", "Smoothstep"])
@pytest.mark.parametrize("grid,M", H.AGG_GRIDS, ids=[f"L{g[0]}-T{g[1]}" for g, _ in H.AGG_GRIDS])
def test_agg_kernel(N, grid, M, interp):
    """hash_bwd_f2_agg_kernel (F = 2, Linear / Smoothstep), from a 2^14 table down to a 2-entry one where the eight
    corners of a cell collide (that one at M = 65, which keeps k <= 647)."""
    _two_launch(N, f"agg L{grid[0]} 2^{grid[1]} {interp} M={M}", _x(M), grid, 2, interp, seed=grid[0])


@pytest.mark.parametrize("M", H.RAGGED_M)
def test_agg_kernel_ragged(N, M):
    """M at the edges of the 16-sample sub-sequence and the 64-sample workgroup: the lanes past M hold no sample."""
    _two_launch(N, f"agg ragged M={M}", _x(M), H.GRID_L8, 2, "Linear", seed=M)


def test_nearest_f2(N):
    """hash_bwd_f2_kernel; the resolutions include odd ones, where the box centre rounds half to even."""
    assert any(int(r) % 2 for r in H.resolutions(H.NEAREST_GRID))
    _two_launch(N, "nearest F=2", _x(), H.NEAREST_GRID, 2, "Nearest", seed=1)


@pytest.mark.parametrize("interp", ["Linear", "Nearest"])
@pytest.mark.parametrize("F", H.GENERIC_F)
def test_generic_kernel(N, F, interp):
    """hash_bwd_kernel<F>, F = 1, 4, 8, on a 64-entry table."""
    _two_launch(N, f"generic F={F} {interp}", _x(), H.GENERIC_GRID, F, interp, seed=10 + F)


def test_pitches(N):
    """x as the first three columns of (M, 6) rows, d_out in rows of pitch L F + 4 whose pad columns are NaN."""
    g, res = _grid(N, H.GRID_L8, 2, "Linear")
    x6 = _x()
    M, od, rows = x6.shape[0], 16, 8 * 2 ** 12
    gen = torch.Generator().manual_seed(77)
    d_out = torch.randn(M, od, generator=gen)
    base = torch.randn(rows, 2, generator=gen) * 1e-3
    buf = torch.full((M, od + 4), float("nan"))
    buf[:, :od] = d_out
    buf, got = buf.to(DEV), base.to(DEV)
    x = x6[:, :3]
    assert x.stride(0) == 6 and x.data_ptr() == x6.data_ptr()
    N.check(N.lib().nerf_hash_encode_bwd(N._addr(g), N.ptr(x), 6, M, (ctypes.c_float * 6)(*AABB), EPS, N.ptr(buf),
                                         od + 4, N.ptr(got), N.stream()), "nerf_hash_encode_bwd")
    torch.cuda.synchronize()
    _judge("pitches", got.cpu(), H.scatter_reference(x.cpu(), d_out, res, 12, 2, "Linear", H.BOX, EPS), base)


def test_no_box(N):
    """aabb = None: the points are unit-cube coordinates already, no clamp."""
    _two_launch(N, "no box", H.unit_input().to(DEV), H.GRID_L8, 2, "Linear", aabb=None, seed=3)


def test_guard_rows(N):
    """d_table as a view into a larger buffer: the 64 rows before and after it keep their bits."""
    g, res = _grid(N, H.GRID_L8, 2, "Smoothstep")
    x = _x()
    rows = 8 * 2 ** 12
    gen = torch.Generator().manual_seed(78)
    d_out = torch.randn(x.shape[0], 16, generator=gen)
    big = torch.randn(rows + 128, 2, generator=gen) * 1e-3
    big[:64], big[-64:] = 12345.678, -8765.4321
    dev = big.to(DEV)
    N.hash_encode_bwd(g, x, d_out.to(DEV), rows, AABB, EPS, d_table=dev[64:64 + rows])
    torch.cuda.synchronize()
    out = dev.cpu()
    assert not torch.isnan(out).any()
    assert torch.equal(out[:64].view(torch.int32), big[:64].view(torch.int32))
    assert torch.equal(out[-64:].view(torch.int32), big[-64:].view(torch.int32))
    _judge("guard rows", out[64:64 + rows], H.scatter_reference(x[:, :3].cpu(), d_out, res, 12, 2, "Smoothstep",
                                                                 H.BOX, EPS), big[64:64 + rows])


# ------------------------------------------------------------------------------------------------ fused path

@functools.lru_cache(maxsize=None)
def _expert(levels, interp):
    """The production expert of test_bwd_hash_fused_vs_pair."""
    from nerf_amd.ngp import InstantNGP
    torch.manual_seed(12)
    grid = H.fused_grid(levels)
    net = InstantNGP(scene_box=torch.tensor(H.BOX), hidden=64, sigma_depth=2, color_hidden=64, color_depth=2,
                     dir_encoding="spherical",
                     hash_enc_conf=dict(levels=levels, features_per_level=2, log2_hashmap_size=grid[1],
                                        min_res=grid[2], max_res=grid[3], interpolation=interp)).to(DEV)
    with torch.no_grad():
        net.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    assert torch.equal(net.xyz_encoder.level_resolutions.cpu(), H.resolutions(grid))
    assert net._aabb_host == AABB and net._eps == EPS
    return net


def _pair(N, net, x_d, gout):
    """enc, and nerf_ngp_bwd's d_enc and d_w on clean (M, .) inputs; the CPU scatter of that d_enc is the reference."""
    w, tab = net.packed().detach(), net.xyz_encoder.hash_table.detach()
    enc = N.hash_encode(net.xyz_encoder.grid, tab, x_d, AABB, EPS)
    d_enc, d_w = N.ngp_bwd(net.net_struct, w, enc, x_d, gout)
    return w, enc, d_enc, d_w


def _fused(N, what, levels, interp, x_d, seed=0):
    net = _expert(levels, interp)
    grid = H.fused_grid(levels)
    M = x_d.shape[0]
    gen = torch.Generator().manual_seed(2000 + seed)
    gout = torch.randn(M, 4, generator=gen).to(DEV)
    base = torch.randn(levels * 2 ** grid[1], 2, generator=gen) * 1e-3
    w, enc, d_enc, dw_p = _pair(N, net, x_d, gout)
    got = base.to(DEV)
    dw_f = N.ngp_bwd_hash(net.net_struct, net.xyz_encoder.grid, w, enc, x_d, gout, got, AABB, EPS)
    torch.cuda.synchronize()
    assert dw_f is not None, f"{what}: no fused kernel for this shape"
    assert torch.equal(dw_f.cpu(), dw_p.cpu()), what
    ref = H.scatter_reference(x_d[:, :3].cpu(), d_enc.cpu(), H.resolutions(grid), grid[1], 2, interp, H.BOX, EPS)
    return _judge(what, got.cpu(), ref, base)


@pytest.mark.parametrize("interp", ["Linear", "Smoothstep"])
@pytest.mark.parametrize("levels", H.FUSED_LEVELS)
def test_fused_levels(N, levels, interp):
    """L = 16 and L = 8 fill both level halves / one; L = 5 and L = 9 mask lanes by l2 < L (L = 5: waves 2 and 3 issue
    nothing; L = 9: they hold one level).  All four are production plans (the enc tile is padded to 32 columns), so
    the fused kernel takes them."""
    _fused(N, f"fused L={levels} {interp}", levels, interp, _x(), seed=levels)


@pytest.mark.parametrize("M", H.FUSED_M)
def test_fused_ragged(N, M):
    """M at the edges of the 16-row halves and the 32-row tile."""
    _fused(N, f"fused M={M}", 16, "Linear", _x(M), seed=M)


@pytest.mark.parametrize("shift", H.FUSED_SHIFTS)
def test_fused_repeat_across_rows_and_tiles(N, shift):
    """The 40-fold repeat from row 8 of a tile (across rows 15 | 16) and from row 24 (across the tile boundary)."""
    _fused(N, f"fused shift={shift}", 16, "Linear", _x(shift=shift), seed=shift)


def test_fused_two_tiles_per_workgroup(N):
    """514 tiles on at most 512 workgroups: some walk a second tile (with another prefetched input tile)."""
    x = _x(H.FUSED_BIG["M"], R=H.FUSED_BIG["R"], S=H.FUSED_BIG["S"])
    assert x.shape[0] == H.FUSED_BIG["M"]
    _fused(N, "fused M=16421", 8, "Linear", x, seed=5)


@pytest.mark.parametrize("n", H.N_ROWS)
def test_device_sized_entry_point(N, n):
    """nerf_ngp_bwd_hash_n: capacity 96, the row count rng[1] - rng[0] read on the device (200 clamps to the
    capacity), NaN in every row past it.  d_table against the reference of the first n rows; d_w bitwise nerf_ngp_bwd's
    on those rows (the same tiles in the same workgroup order; a workgroup without a tile adds a zero slab)."""
    net = _expert(16, "Smoothstep")
    grid = H.fused_grid(16)
    cap, nn = H.N_CAP, min(n, H.N_CAP)
    gen = torch.Generator().manual_seed(3000 + n)
    base = torch.randn(16 * 2 ** grid[1], 2, generator=gen) * 1e-3
    w = net.packed().detach()
    x_d = torch.full((cap, 6), float("nan"), device=DEV)
    enc = torch.full((cap, 32), float("nan"), device=DEV)
    gout = torch.full((cap, 4), float("nan"), device=DEV)
    if nn:
        x_d[:nn] = _x(nn)
        gout[:nn] = torch.randn(nn, 4, generator=gen).to(DEV)
        _, e, d_enc, dw_p = _pair(N, net, x_d[:nn].contiguous(), gout[:nn].contiguous())
        enc[:nn] = e
    rng = torch.tensor([H.N_LO, H.N_LO + n], dtype=torch.int32, device=DEV)
    got = base.to(DEV)
    d_w = torch.full_like(w, float("nan"))
    ws = N.ngp_workspace(net.net_struct, cap, x_d.device)
    N.check(N.lib().nerf_ngp_bwd_hash_n(N._addr(net.net_struct), N._addr(net.xyz_encoder.grid), N.ptr(w), N.ptr(enc),
                                        enc.stride(0), N.ptr(x_d), cap, N.ptr(rng), N.ptr(gout),
                                        (ctypes.c_float * 6)(*AABB), EPS, N.ptr(got), N.ptr(d_w), 0, N.ptr(ws),
                                        ws.numel(), N.stream()), "nerf_ngp_bwd_hash_n")
    torch.cuda.synchronize()
    assert torch.isfinite(d_w).all() and not torch.isnan(got).any()
    if nn == 0:
        assert torch.equal(got.cpu().view(torch.int32), base.view(torch.int32))
        assert not d_w.any()
        return
    ref = H.scatter_reference(x_d[:nn, :3].cpu(), d_enc.cpu(), H.resolutions(grid), grid[1], 2, "Smoothstep", H.BOX,
                              EPS)
    _judge(f"bwd_hash_n n={n}", got.cpu(), ref, base)
    assert torch.equal(d_w, dw_p)
