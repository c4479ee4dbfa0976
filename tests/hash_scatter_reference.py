"""Plain-torch CPU reference of the hash-grid table gradient (csrc/ngp.hip: hash_bwd_kernel<F>, hash_bwd_f2_kernel,
hash_bwd_f2_agg_kernel and the scatter inside ngp_bwd_prod_kernel<*, HB = true>) — TEST INFRASTRUCTURE ONLY.

The operation: every sample adds, per level, eight corner terms (one for Nearest) to the table-gradient row its corner
hashes to.  The reference computes each term in fp32 with the kernels' operations, one rounding each and in the
kernels' order, so the k terms of an entry are the same fp32 numbers on both sides, and accumulates them in float64.
Only the order of the kernels' fp32 additions is then free (atomics, and the run aggregation that sums the lanes of
one cell before the atomic), so the standard summation bound holds per entry:

    |got - sum64| <= (k - 1) 2^-24 sum|t|  + O(2^-48)          and the tests allow      k 2^-23 sum|t|,

more than twice the first-order bound.  A base the kernel accumulates into counts as one more term.  An entry no
sample touches (k = 0) must come back as it was, bit for bit.

run_stats() describes, from the same indices, what the run aggregation sees: the lanes of one (feature, x-corner)
sub-sequence are the 16 consecutive samples m = 16 j .. 16 j + 15 (a wave of hash_bwd_f2_agg_kernel; rows
16 (wave & 1) .. + 15 of a 32-row tile in the fused kernel), and a lane merges into its predecessor when both hold the
same entry.

build_input() and the case tables below are the inputs of tests/test_gpu_hash_scatter.py; tests/
test_hash_scatter_reference.py checks on the CPU that they reach the regime they are meant for."""
import functools
from collections import namedtuple

import torch

from oracle import ngp_oracle as NO

U23 = 2.0 ** -23
GROUP = 16   # samples per run-aggregation sub-sequence
TILE = 32    # rows per tile of the fused backward
K_MAX = 647  # k^2 2^-23 <= 0.05: one lost term of average size |t| = abs64 / k is then >= 20 bounds away


# ------------------------------------------------------------------------------------------------ the operation

def unit_points(x, aabb=None, eps=1e-6):
    """load_x01: (x - mn) / ext clamped to [eps, 1 - eps], every operation in fp32 (1 - eps is the fp32 difference);
    without a box the points are taken as they are."""
    x = x[:, :3].float()
    if aabb is None:
        return x.clone()
    aabb = torch.as_tensor(aabb, dtype=torch.float32).reshape(2, 3)
    e = torch.tensor(eps, dtype=torch.float32)
    v = (x - aabb[0]) / (aabb[1] - aabb[0])
    return torch.minimum(torch.maximum(v, e), torch.tensor(1.0, dtype=torch.float32) - e)


def scatter_terms(x, d_out, res, log2_T, F, interpolation, aabb=None, eps=1e-6):
    """-> (rows (M, L, C) int64, terms (M, L, C, F) fp32): sample m adds terms[m, l, c] to table-gradient row
    rows[m, l, c] (level offset included).  C = 8 corners, bits x = 4, y = 2, z = 1 (C = 1 for Nearest).  d_out may
    be None: only the rows are returned then (terms is None)."""
    res = torch.as_tensor(res)
    L, T = res.numel(), 2 ** log2_T
    p = unit_points(x, aabb, eps)
    s = p[:, None, :] * res.to(torch.float32).view(1, L, 1)  # (M, L, 3)
    offs = (torch.arange(L, dtype=torch.int64) * T).view(1, L)
    g = None if d_out is None else d_out[:, :L * F].float().reshape(-1, L, F)
    if interpolation == "Nearest":
        i = torch.round(s).to(torch.int64)  # half to even, as rintf
        rows = (NO.hash_index(i[..., 0], i[..., 1], i[..., 2], log2_T) + offs)[..., None]
        return rows, None if g is None else g[:, :, None, :].clone()
    assert interpolation in ("Linear", "Smoothstep"), interpolation
    fl = torch.floor(s)
    w = s - fl
    if interpolation == "Smoothstep":
        w = (w * w) * (3.0 - 2.0 * w)
    u = 1.0 - w
    i0 = fl.to(torch.int64)
    rows, terms = [], []
    for c in range(8):
        dx, dy, dz = (c >> 2) & 1, (c >> 1) & 1, c & 1
        rows.append(NO.hash_index(i0[..., 0] + dx, i0[..., 1] + dy, i0[..., 2] + dz, log2_T) + offs)
        if g is not None:
            wx = (w if dx else u)[..., 0:1]
            wy = (w if dy else u)[..., 1:2]
            wz = (w if dz else u)[..., 2:3]
            terms.append(((g * wz) * wy) * wx)
    return torch.stack(rows, -1), None if g is None else torch.stack(terms, 2)


def scatter_reference(x, d_out, res, log2_T, F, interpolation, aabb=None, eps=1e-6):
    """-> (sum64 (L T, F) float64, abs64 (L T, F) float64 = sum |term|, count (L T,) int64 = k) per table entry."""
    rows, terms = scatter_terms(x, d_out, res, log2_T, F, interpolation, aabb, eps)
    n = torch.as_tensor(res).numel() * 2 ** log2_T
    flat = rows.reshape(-1)
    t64 = terms.double().reshape(-1, F)
    sum64 = torch.zeros(n, F, dtype=torch.float64).index_add_(0, flat, t64)
    abs64 = torch.zeros(n, F, dtype=torch.float64).index_add_(0, flat, t64.abs())
    return sum64, abs64, torch.bincount(flat, minlength=n)


def entry_counts(x, res, log2_T, interpolation, aabb=None, eps=1e-6):
    """k per table entry from the positions alone."""
    rows, _ = scatter_terms(x, None, res, log2_T, 1, interpolation, aabb, eps)
    return torch.bincount(rows.reshape(-1), minlength=torch.as_tensor(res).numel() * 2 ** log2_T)


def bound_ratio(got, sum64, abs64, count, base=None):
    """-> (worst |got - (base + sum64)| / bound over the touched entries, untouched entries bit-identical to the base).
    bound = k 2^-23 sum|t|, a non-zero base counting as one more term in k and in sum|t|.  An entry whose bound is 0
    (every term 0) must be met exactly: its ratio is 0 then, inf otherwise."""
    got = got.detach().cpu()
    k = count.double()[:, None].expand_as(sum64)
    ref, mag = sum64, abs64
    if base is not None:
        base = base.detach().cpu()
        ref, mag, k = ref + base.double(), mag + base.double().abs(), k + 1.0
    zero = torch.zeros_like(got) if base is None else base
    hit = (count > 0)[:, None].expand_as(sum64)
    err = torch.nan_to_num((got.double() - ref).abs()[hit], nan=float("inf"), posinf=float("inf"))
    bound = (k * U23 * mag)[hit]
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
    untouched = bool(torch.equal(got[~hit].view(torch.int32), zero[~hit].view(torch.int32)))
    return (float(ratio.max()) if ratio.numel() else 0.0), untouched


# ------------------------------------------------------------------------------------------------ run statistics

RunStats = namedtuple("RunStats", "merged_share longest_run longest_in_group crosses_group")


def run_stats(rows, group=GROUP):
    """rows (M, ...) int64: one index sequence along dim 0 per trailing position (level, corner).
    merged_share: the share of (sample, position) pairs whose index equals the previous sample's inside one group of
    `group` consecutive samples (the lanes that do not issue an atomic); longest_run: the longest stretch of equal
    consecutive indices; longest_in_group: the same with runs cut at the group boundaries (what one scan sums, at most
    `group`); crosses_group: some run continues from the last sample of a group into the first of the next."""
    M = rows.shape[0]
    if M == 0:
        return RunStats(0.0, 0, 0, False)
    rows = rows.reshape(M, -1)
    m = torch.arange(M).view(M, 1)
    same = torch.zeros_like(rows, dtype=torch.bool)
    same[1:] = rows[1:] == rows[:-1]
    first = (m % group == 0).expand_as(same)

    def longest(head):
        start = torch.where(head, m.expand_as(rows), torch.zeros_like(rows))
        return int((m - torch.cummax(start, 0).values + 1).max())

    merged = same & ~first
    return RunStats(float(merged.sum()) / merged.numel(), longest(~same), longest(~same | first),
                    bool((same & first).any()))


# ------------------------------------------------------------------------------------------------ the inputs

BOX = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
STEP, T0 = 3.0 / 256.0, 1.4
REPEAT = 40
REPEAT_POINT = (0.31, -0.22, 0.67)
NODE_K = (1552, 400)  # x01 = k / 2048: grid nodes of every power-of-two level up to 128 as well (k is a multiple of 16)


def rays(n, seed):
    """_rays of tests/test_gpu_occ.py: origins near (0.1, -3, 0.2), directions around +y."""
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.1, -3.0, 0.2]) + torch.randn(n, 3, generator=g) * 0.1
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g) * 0.35 + torch.tensor([0.0, 1.0, 0.0]), dim=-1)
    return o, d


def edge_points():
    """The box centre (x01 = 0.5: a node at even resolutions, the half-way rounding case of Nearest at odd ones), both
    box corners (the clamp at eps and 1 - eps), and a point outside the box in x (clamped to 1 - eps) whose y and z sit
    at x01 = k / 2048 exactly (-1.5 + 3 k / 2048 and the division by 3 are exact in fp32)."""
    ky, kz = NODE_K
    return torch.tensor([[0.0, 0.0, 0.0], [-1.5, -1.5, -1.5], [1.5, 1.5, 1.5],
                         [2.25, -1.5 + 3.0 * ky / 2048.0, -1.5 + 3.0 * kz / 2048.0]], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def build_input(R=8, S=40, shift=0, seed=3):
    """(M, 6) fp32 [x, d], M = R S + shift + 44, ray-major: R rays of S samples at t = 1.4 + 3 j / 256, `shift` more
    samples of one further ray, one point 40 times (from row R S + shift: with R S a multiple of 16 and shift = 0 the
    repeat fills one 16-sample group, then another, and ends in the middle of the third), the four edge points.
    Columns 3..5 are the ray directions (unit vectors for the edge rows).  Do not modify the result: it is cached."""
    o, d = rays(R + 1, seed)
    t = T0 + STEP * torch.arange(S, dtype=torch.float32)
    x = (o[:R, None, :] + d[:R, None, :] * t[None, :, None]).reshape(-1, 3)
    dd = d[:R, None, :].expand(R, S, 3).reshape(-1, 3)
    xs = o[R] + d[R] * t[:shift, None]
    rep = torch.tensor(REPEAT_POINT, dtype=torch.float32).expand(REPEAT, 3)
    e = edge_points()
    tail_d = d[R].expand(shift + REPEAT + e.shape[0], 3)
    return torch.cat([torch.cat([x, xs, rep, e], 0), torch.cat([dd, tail_d], 0)], 1).contiguous()


def unit_input(M=364):
    """The base input mapped into [0, 1) for the calls without a box: (x + 1.5) / 3, the outside coordinate folded
    back inside."""
    p = unit_points(build_input()[:M], BOX, 1e-6)
    return torch.cat([p.clamp(0.0, 0.999), build_input()[:M, 3:]], 1).contiguous()


BASE_M = 364

# (levels, log2_T, min_res, max_res)
GRID_L16, GRID_L8, GRID_L5, GRID_L1 = (16, 14, 16, 2048), (8, 12, 8, 128), (5, 4, 4, 64), (1, 1, 4, 4)
AGG_GRIDS = [(GRID_L16, BASE_M), (GRID_L8, BASE_M), (GRID_L5, BASE_M), (GRID_L1, 65)]  # (grid, M)
RAGGED_M = [1, 15, 16, 17, 63, 64, 65]
NEAREST_GRID = (8, 10, 4, 300)   # tag c of tests/test_gpu_ngp.py's HCFG at F = 2: odd resolutions among them
GENERIC_GRID = (4, 6, 4, 64)     # F = 1, 4, 8
GENERIC_F = [1, 4, 8]

# the fused kernel: the production expert of test_bwd_hash_fused_vs_pair, log2_T = 14, min_res 8, max_res 512
FUSED_LEVELS = [16, 8, 5, 9]
FUSED_M = [1, 15, 16, 17, 31, 32, 33, BASE_M]
FUSED_SHIFTS = [8, 24]  # the repeat from row 8 / 24 of its tile: across rows 15 | 16, and across the tile boundary
FUSED_BIG = dict(R=257, S=64, M=16421)  # 514 tiles: with at most 512 workgroups some walk two
N_CAP, N_LO, N_ROWS = 96, 7, [0, 1, 33, 96, 200]


def fused_grid(levels):
    return (levels, 14, 8, 512)


def resolutions(grid):
    return NO.hash_resolutions(grid[0], grid[2], grid[3])[0]


def position_cases():
    """Every (name, x (M, 3), grid, interpolation, aabb) whose scatter tests/test_gpu_hash_scatter.py
    checks against scatter_reference with the per-entry bound."""
    base = build_input()
    out = []
    for grid, M in AGG_GRIDS:
        for interp in ("Linear", "Smoothstep"):
            out.append((f"agg-L{grid[0]}-{interp}", base[:M, :3], grid, interp, BOX))
    for M in RAGGED_M:
        out.append((f"ragged-{M}", base[:M, :3], GRID_L8, "Linear", BOX))
    out.append(("nearest", base[:, :3], NEAREST_GRID, "Nearest", BOX))
    for interp in ("Linear", "Nearest"):
        out.append((f"generic-{interp}", base[:, :3], GENERIC_GRID, interp, BOX))
    out.append(("pitches", base[:, :3], GRID_L8, "Linear", BOX))
    out.append(("no-box", unit_input()[:, :3], GRID_L8, "Linear", None))
    out.append(("guard-rows", base[:, :3], GRID_L8, "Smoothstep", BOX))
    for levels in FUSED_LEVELS:
        for interp in ("Linear", "Smoothstep"):
            out.append((f"fused-L{levels}-{interp}", base[:, :3], fused_grid(levels), interp, BOX))
    for M in FUSED_M:
        out.append((f"fused-M{M}", base[:M, :3], fused_grid(16), "Linear", BOX))
    for s in FUSED_SHIFTS:
        out.append((f"fused-shift{s}", build_input(shift=s)[:, :3], fused_grid(16), "Linear", BOX))
    big = build_input(R=FUSED_BIG["R"], S=FUSED_BIG["S"])[:FUSED_BIG["M"], :3]
    out.append(("fused-big", big, fused_grid(8), "Linear", BOX))
    for n in [n for n in N_ROWS if n > 0]:
        out.append((f"fused-n{n}", base[:min(n, N_CAP), :3], fused_grid(16), "Smoothstep", BOX))
    return out
