"""The table-gradient yardstick on the CPU alone (tests/hash_scatter_reference.py): agreement with fp32 autograd
through the oracle's hash_encode, a known answer, run_stats on hand-built sequences, and the conditions the inputs of
tests/test_gpu_hash_scatter.py must meet to reach the run aggregation at all (merged share, a full 16-lane run, a
cell continuing across a 16-sample boundary) and to keep the per-entry bound sharp (k <= 647)."""
import pytest
import torch

import hash_scatter_reference as H
from oracle import ngp_oracle as NO

CASES = H.position_cases()


def _autograd_table_grad(x, d_out, res, log2_T, F, interp, aabb, eps=1e-6):
    table = torch.zeros(res.numel() * 2 ** log2_T, F, requires_grad=True)
    box = torch.tensor(aabb)
    x01 = ((x - box[0]) / (box[1] - box[0])).clamp(eps, 1.0 - eps)
    y = NO.hash_encode(table, x01, res, log2_T, F, interp)
    (y * d_out).sum().backward()
    return table.grad


def test_clamp_bounds_match_torch():
    """The kernels clamp to the fp32 difference 1.0f - eps, the oracle to the double 1 - eps rounded to fp32: the same
    fp32 number for the eps in use."""
    for eps in (1e-6, 0.0):
        hi = torch.tensor(1.0) - torch.tensor(eps, dtype=torch.float32)
        assert float(hi) == float(torch.tensor(1.0 - eps, dtype=torch.float32))
        assert torch.equal(H.unit_points(H.build_input(), H.BOX, eps),
                           ((H.build_input()[:, :3] + 1.5) / 3.0).clamp(eps, 1.0 - eps))


@pytest.mark.parametrize("F", [1, 2, 4])
@pytest.mark.parametrize("interp", ["Linear", "Smoothstep", "Nearest"])
def test_reference_agrees_with_autograd(interp, F):
    """torch's index_put backward adds the same fp32 terms in its own order: it lies within the bound of sum64, and an
    entry nothing touches is exactly 0."""
    grid = H.NEAREST_GRID if interp == "Nearest" else H.GRID_L8
    res = H.resolutions(grid)
    x = H.build_input()[:, :3]
    g = torch.Generator().manual_seed(7 + F)
    d_out = torch.randn(x.shape[0], grid[0] * F, generator=g)
    sum64, abs64, count = H.scatter_reference(x, d_out, res, grid[1], F, interp, H.BOX)
    ref = _autograd_table_grad(x, d_out, res, grid[1], F, interp, H.BOX)
    ratio, untouched = H.bound_ratio(ref, sum64, abs64, count)
    print(f"{interp} F={F}: autograd fp32 vs sum64, worst ratio to the bound {ratio:.3f}, max k {int(count.max())}")
    assert untouched
    assert ratio <= 1.0
    assert int(count.sum()) == x.shape[0] * grid[0] * (1 if interp == "Nearest" else 8)
    # the bound has teeth: dropping one sample's terms is seen
    sum_d, _, _ = H.scatter_reference(x[1:], d_out[1:], res, grid[1], F, interp, H.BOX)
    assert H.bound_ratio(sum_d.float(), sum64, abs64, count)[0] > 1.0


def test_known_answer_cell_centre():
    """One sample at the centre of a cell of a one-level grid: every corner weight is 1/2, so each of the eight corners
    receives g / 8 exactly (a table large enough that the eight corners do not collide)."""
    res = torch.tensor([4], dtype=torch.int32)
    x = torch.tensor([[0.375, 0.625, 0.125]])  # s = (1.5, 2.5, 0.5)
    g = torch.tensor([[3.0, -5.0]])
    for interp in ("Linear", "Smoothstep"):  # smoothstep(1/2) = 1/2
        sum64, abs64, count = H.scatter_reference(x, g, res, 10, 2, interp)
        rows = [int(NO.hash_index(torch.tensor(1 + dx), torch.tensor(2 + dy), torch.tensor(dz), 10))
                for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
        assert len(set(rows)) == 8
        assert sorted(torch.nonzero(count).flatten().tolist()) == sorted(rows)
        assert torch.equal(count[rows], torch.ones(8, dtype=torch.int64))
        assert torch.equal(sum64[rows], (g.double() / 8).expand(8, 2))
        assert torch.equal(abs64[rows], (g.double().abs() / 8).expand(8, 2))
    sum64, _, count = H.scatter_reference(x, g, res, 10, 2, "Nearest")  # round half to even: (2, 2, 0)
    row = int(NO.hash_index(torch.tensor(2), torch.tensor(2), torch.tensor(0), 10))
    assert torch.nonzero(count).flatten().tolist() == [row] and torch.equal(sum64[row], g[0].double())


def test_bound_ratio_base_and_untouched():
    sum64 = torch.tensor([[1.0], [0.0], [0.0]], dtype=torch.float64)
    abs64 = torch.tensor([[3.5], [0.0], [0.0]], dtype=torch.float64)
    count = torch.tensor([2, 0, 1])
    base = torch.tensor([[0.5], [0.25], [0.0]])
    got = torch.tensor([[1.5], [0.25], [0.0]])
    assert H.bound_ratio(got, sum64, abs64, count, base) == (0.0, True)
    got[0, 0] += 3 * 2.0 ** -23 * 4.0  # exactly the bound (12 ulps of 1.5): k = 2 + 1, sum|t| = 3.5 + 0.5
    assert H.bound_ratio(got, sum64, abs64, count, base) == (1.0, True)
    got[1, 0] = -0.25
    assert H.bound_ratio(got, sum64, abs64, count, base)[1] is False
    got[1, 0], got[2, 0] = 0.25, 1e-30  # an entry whose terms are all zero must be met exactly
    assert H.bound_ratio(got, sum64, abs64, count, base)[0] == float("inf")
    got[2, 0] = float("nan")
    assert H.bound_ratio(got, sum64, abs64, count, base)[0] == float("inf")


def test_run_stats_by_hand():
    a = torch.cat([torch.full((16,), 5), torch.arange(100, 116)])
    s = H.run_stats(a)
    assert (s.longest_run, s.longest_in_group, s.crosses_group) == (16, 16, False)
    assert s.merged_share == 15 / 32
    b = torch.arange(32) + 100
    b[14:19] = 7
    s = H.run_stats(b)
    assert (s.longest_run, s.longest_in_group, s.crosses_group) == (5, 3, True)
    assert s.merged_share == 3 / 32  # 15 merges into 14; 17 and 18 into 16; 16 starts a group
    # two columns are two sequences: the statistics are taken over both
    s = H.run_stats(torch.stack([a, b], 1))
    assert (s.longest_run, s.longest_in_group, s.crosses_group) == (16, 16, True)
    assert s.merged_share == 18 / 64
    assert H.run_stats(torch.zeros(0, 3, dtype=torch.int64)).longest_run == 0


def test_input_layout():
    x = H.build_input()
    assert x.shape == (H.BASE_M, 6) and x.dtype == torch.float32
    start = 8 * 40
    assert start % H.GROUP == 0 and start % H.TILE == 0
    assert torch.equal(x[start:start + H.REPEAT, :3], torch.tensor(H.REPEAT_POINT).expand(H.REPEAT, 3))
    p = H.unit_points(x, H.BOX)
    e = p[start + H.REPEAT:]
    lo, hi = float(torch.tensor(1e-6)), float(torch.tensor(1.0) - torch.tensor(1e-6))
    assert e[0].tolist() == [0.5, 0.5, 0.5]
    assert e[1].tolist() == [lo] * 3 and e[2].tolist() == [hi] * 3
    assert e[3].tolist() == [hi, H.NODE_K[0] / 2048.0, H.NODE_K[1] / 2048.0]  # outside in x; grid nodes in y and z
    for s in H.FUSED_SHIFTS:  # the repeat from row 8 / 24 of a tile
        xs = H.build_input(shift=s)
        assert xs.shape[0] == H.BASE_M + s
        assert torch.equal(xs[start + s:start + s + H.REPEAT, :3], torch.tensor(H.REPEAT_POINT).expand(H.REPEAT, 3))
    assert H.FUSED_SHIFTS == [8, 24]  # rows 8..15 | 16..31 | next tile 0..15, and rows 24..31 | next tile 0..31
    assert -(-H.FUSED_BIG["M"] // H.TILE) > 512  # more tiles than the fused backward ever launches workgroups
    u = H.unit_input()
    assert float(u[:, :3].min()) >= 0.0 and float(u[:, :3].max()) < 1.0


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_inputs_reach_the_regime(case):
    """Every input of tests/test_gpu_hash_scatter.py, from the reference alone.  The inputs that hold the whole
    40-fold repeat are held to all four conditions.  The others are prefixes of the base input (ragged M, the
    device-sized calls); a prefix cannot hold more than it is long, so each is held to what its length allows: a
    merged share >= 0.25 from M = 15, a full 16-lane run from M = 16, a run across a group boundary from M = 17 (the
    first samples of a ray share their coarse cells)."""
    name, x, grid, interp, aabb = case
    M = x.shape[0]
    rows, _ = H.scatter_terms(x, None, H.resolutions(grid), grid[1], 1, interp, aabb)
    s = H.run_stats(rows)
    k = torch.bincount(rows.reshape(-1))
    print(f"{name}: M={M} merged share {s.merged_share:.3f}, longest run {s.longest_run} ({s.longest_in_group} in a "
          f"group), crosses a group boundary: {s.crosses_group}, largest k {int(k.max())}")
    if M >= 15:
        assert s.merged_share >= 0.25
    if M >= 16:
        assert s.longest_in_group == H.GROUP
    if M >= 17:
        assert s.crosses_group
    if name == "fused-big":
        # 16421 samples x 8 corners fall on the ~200 nodes a resolution-8 level has inside the ray bundle: k <= 647
        # cannot hold at the two coarsest levels (largest k 3464).  The bound stays valid there; it stays sharp on
        # the six levels from resolution 26 on, which hold 99.8 % of the touched entries.
        assert float((k[k > 0] <= H.K_MAX).sum()) >= 0.99 * float((k > 0).sum())
        T = 2 ** grid[1]
        assert int(k[2 * T:].max()) <= H.K_MAX
    else:
        assert int(k.max()) <= H.K_MAX and int(k.max()) ** 2 * H.U23 <= 0.05
