"""References and deterministic inputs for the occupancy-grid kernels (csrc/occ.hip) — TEST INFRASTRUCTURE ONLY.
tests/test_gpu_occ_edges.py compares the kernels with these through the C entry points; tests/test_occ_reference.py
checks on the CPU that the references are right, that the shipped inputs meet the conditions stated here and that
the bounds have teeth.  u = 2^-24 is the unit roundoff of fp32; every count is to first order in u.

EXACT FAMILIES (compared as bytes).  The counter RNG (nerf_mix64 / nerf_uniform) is restated in Python integers, so
every seeded draw is known: uniform() is the 24-bit integer over 2^24, an exact float.  exclusive scan, ray counts,
compaction, binarize are integer work.  occ_update on distinct cells is max(o * decay, v): one fp32 multiply and a
max.  sample_cells is draw_below(): for a range up to 2^24 one fp32 multiply of the uniform with the range, a
truncation and a clamp; above 2^24 the high 64 bits of (64-bit mix) * range.

DYADIC MARCH FAMILY.  occ.o is built with fma contraction on, so a general fp32 restatement of the marcher cannot
match bytes.  The family's inputs make every operation of the marcher exact in fp32 instead: cone = 0, step a power of
two, origins on the 1/32 lattice, direction components from {0, +-1, +-1/2, +-1/4}, near / far / u dyadic, ROI centre
dyadic, ROI half sizes powers of two, R a power of two.  All of t, mid, the points, the cell arithmetic and the
skip (te - t) / dt then live on a lattice of 2^-9 below 2^4: 13 bits.  march_ray() run in Python floats is therefore
the kernel's exact output, and run in numpy float32 (test_occ_reference) it gives the same bytes.  The level of a point
is taken from the exponent in the float run (exact) and from ceil(log2f(s)) in the float32 run, as the kernel does.
The family meets midpoints exactly on cell faces, s exactly 1, 2 and 4, zero direction components, starts inside the
grid and rays that miss.  Seeded jitter (24-bit u) is not dyadic enough: t = near + u * step rounds once it passes a
power of two.  It is checked by comparing the kernel with itself (u passed explicitly) and, for the multi-expert
streams, on the first sample of rays that start inside a full grid, whose t0 is the single rounding
fl(near + u * step).

PACKED COMPOSITING (packed_fwd_kernel / packed_bwd_kernel) against float64 on the same fp32 inputs.  Per sample k of a
ray, with c = k // 64 the number of chunk carries before it and I_k the inclusive sum of sigma dt:
  dt = t1 - t0 (1), sdt = sigma dt (1): 2u relative; the wave scan adds positive terms over a depth of 6, the carry
  S adds one rounding per earlier chunk, S + inc and (.) - sdt one each: the exclusive sum E_k is within
      dE_k = (10 + c) u I_k                                     (absolute: the subtraction cancels)
  T_k = expf(-E_k): expf within 1 ulp = 2u:     dT_k = T_k (dE_k + 2u) + tiny
  alpha_k = 1 - expf(-sdt): the argument carries 2u sdt, expf 2u, the subtraction u:
      dalpha_k = e^-sdt (2u + 2u sdt) + u alpha_k
  w_k = T_k alpha_k (1):                        dw_k = T_k dalpha_k + alpha_k dT_k + u w_k + tiny
  tiny = 2^-126 covers results the device flushes below the normal range (saturated rays).
  rgb_c = sum_k w_k c_k: one fma per chunk in a lane, a butterfly of depth 6, with nch chunks
      drgb_c = sum_k |c_k| dw_k + (nch + 7) u sum_k |w_k c_k|   (+ |bg_c| (dacc + 2u) + 2u |rgb_c| with a background)
  depth the same with t_mid = (t0 + t1) / 2 (1 more rounding), acc with c_k = 1.
Backward, g_k = <g_rgb, c_k> + g_depth t_mid + (g_acc - <g_rgb, bg>) + g_w,k: at most 8 roundings on any path through
its (mixed-sign) terms: dg_k = 8u G_k, G_k the sum of the absolute values of the terms.
  d rgb_c,k = w_k g_c (1):                      |g_c| dw_k + u |w_k g_c|
  q_k = g_k w_k:                                e_k = |g_k| dw_k + w_k dg_k + u |q_k|
  tot = sum q (nch + 6 additions), inclusive prefix (6 + c + 1): each within A = sum_k e_k + (nch + 7) u sum_k |q_k|
  suffix = tot - prefix (1): 2A + u |suffix| -- absolute in u sum |g_k w_k|, not relative: the subtraction cancels
  T_next = expf(-I_k):                          dTn_k = Tn_k ((9 + c) u I_k + 2u) + tiny
  dsdt = g_k T_next - suffix (2), d sigma = dsdt dt (dt: 1, product: 1):
      dsigma_k = dt (Tn_k dg_k + |g_k| dTn_k + 2A + u (|g_k Tn_k| + |suffix|) + 3u |dsdt|) + tiny
The tests allow twice these first-order counts (the slack the MoE bounds take) and print the worst error / bound.
Observed on an MI355X: see OBSERVED below.

VISIBILITY.  keep = T_k >= eps and (athr <= 0 or alpha_k >= athr), athr = min(alpha_thre, group threshold) (exact).
A sample is left out of the comparison only where |T_k - eps| <= 2 dT_k or |alpha_k - athr| <= 2 dalpha_k; all others
must be equal.

CELL POINTS.  f = (ci + uniform) / R (1 + 1), mn = c - h 2^l, extent = 2 h 2^l, x = mn + f extent (2, or 1 as an fma):
|x - x64| <= 4u (|mn| + |extent|).  f <= (ci + 1) / R and rounding is monotone, so with dyadic faces the point lies
in the closed box of its cell.  Empty slots (-1) give the ROI centre exactly.

MARK INVISIBLE.  Cell centre x_a: 4u (|c_a| + extent_a); d = x - t (1); camera coordinates are three products and two
additions: e_cam = sum_i |R_i| (dx_i + u |d_i|) + 3u sum_i |R_i d_i|; pixel u = (k . cam) / zc:
  dnum = sum_i |k_i| e_i + 3u sum_i |k_i cam_i|,  du = (dnum + |u| e_z) / |zc| + u |u|.
A camera's verdict on a cell is ambiguous where zc is within 2 e_z of near_plane, or u (v) within 2 du (2 dv) of 0 or
W (H).  A cell some camera surely sees is visible; otherwise a cell with an ambiguous camera is left out.

THRESHOLD.  fp64 mean of the cells >= 0 and of all cells; the kernel sums in fp64 in another order and casts:
equal after the cast to within 1 ulp of fp32.

CONE MARCH (cone > 0, generic rays).  fp32 drift is real, so two long marches are not compared: cone_checks() takes
the kernel's own output one step at a time (the step length, the occupied cell of each midpoint, the float64 marcher
from each t1 to the next t0 or to the end, and from the ray's start to its first sample).  A check is left out only
where a float64 decision lies within twice the error of ONE evaluation of its threshold; the count of roundings is in
cone_replay's and _cell64's docstrings.  Over a run of skipped cells the kernel's t is not observable, so its error
is carried along (et) and widens the margins of that run only.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
F32 = np.float32
SENT = -12345.5
ISENT = -7777

# worst error / bound ratios measured on an MI355X over all cases (tests/test_gpu_occ_edges.py prints them per case);
# no visibility decision and no cell of mark_invisible fell inside its margin there.
OBSERVED = {"fwd w": 0.1523, "fwd rgb": 0.0921, "fwd depth": 0.0910, "fwd acc": 0.0914, "bwd rgb": 0.1524,
            "bwd sigma": 0.0531, "packed points": 0.3942, "cell points": 0.2083}

RAY_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 192, 300]
PACKED_N = [1, 3, 4, 5, 37]
ELEMENTWISE_N = [1, 255, 256, 257, 65535, 65536, 65537]
MARCH_N = [1, 127, 128, 129]


def same_bits(a, b):
    a, b = np.ascontiguousarray(_np(a)), np.ascontiguousarray(_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ================================================================================================= counter RNG

_M = (1 << 64) - 1


def mix64(z):
    z &= _M
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & _M
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & _M
    return z ^ (z >> 31)


def bits64(seed, a, b):
    return mix64(seed * 0x9e3779b97f4a7c15 + mix64(a * 0xd1b54a32d192ed03 + b))


def uniform(seed, a, b):
    """nerf_uniform: 24 bits over 2^24, exact as a float (and as a float32)."""
    return (bits64(seed, a, b) >> 40) / 16777216.0


def uniforms(seed, a, n):
    return np.array([uniform(seed, a, b) for b in range(n)], dtype=F32)


def draw_below(seed, a, b, rng):
    if rng <= 1 << 24:
        r = int(F32(uniform(seed, a, b)) * F32(rng))
        return min(r, rng - 1)
    return (bits64(seed, a, b) * rng) >> 64


def draw_below_24bit_only(seed, a, b, rng):
    """The draw before the wide path existed: what the large-grid test must tell from draw_below."""
    r = int(F32(uniform(seed, a, b)) * F32(rng))
    return min(r, rng - 1)


def sample_cells_reference(occ_list, level_base, cpl, n, seed, draw=draw_below):
    """nerf_occ_sample_cells: level_base[l] = pos[l * cpl] (L + 1 entries).  -> int32 (L * 2n)."""
    L = len(level_base) - 1
    out = np.empty(L * 2 * n, dtype=np.int32)
    for l in range(L):
        base, c = int(level_base[l]), int(level_base[l + 1]) - int(level_base[l])
        for j in range(n):
            out[l * 2 * n + j] = l * cpl + draw(seed, 0x51 + l, j, cpl)
        for k in range(n):
            if c <= n:
                v = occ_list[base + k] if k < c else -1
            else:
                v = occ_list[base + draw(seed, 0xA3 + l, k, c)]
            out[l * 2 * n + n + k] = v
    return out


def sample_cells_input(cpl, n_occ, seed):
    """One level's int32 flags with n_occ occupied cells."""
    rs = np.random.RandomState(seed)
    flags = np.zeros(cpl, dtype=np.int32)
    flags[rs.permutation(cpl)[:n_occ]] = 1
    return flags


# ================================================================================================= integer families

def exclusive_scan(x):
    x = _np(x).astype(np.int64)
    return np.concatenate([[0], np.cumsum(x)]).astype(np.int32)


def ray_counts(ri, N):
    return np.bincount(_np(ri).astype(np.int64), minlength=N).astype(np.int32)


def compact(keep, ri, t0, t1, N):
    """-> (pos, ri_o, t0_o, t1_o, counts) of nerf_packed_compact fed with pos = exclusive scan of keep."""
    keep = _np(keep).astype(bool)
    return (exclusive_scan(keep), _np(ri)[keep], _np(t0)[keep], _np(t1)[keep],
            np.bincount(_np(ri)[keep].astype(np.int64), minlength=N).astype(np.int32))


def occ_update(occs, cells, vals, decay):
    """On distinct cells: occs[id] = max(o * decay, v) where o >= 0; -1 cells and -1 slots untouched."""
    out = _np(occs).astype(F32).copy()
    d = F32(decay)
    for c, v in zip(_np(cells).tolist(), _np(vals).astype(F32)):
        if c >= 0 and out[c] >= 0:
            out[c] = max(out[c] * d, v)
    return out


def binarize(occs, thre0):
    return (_np(occs).astype(F32) > F32(thre0)).astype(np.uint8)


def threshold64(occs, occ_thre):
    o = _np(occs).astype(np.float64)
    vis = o[o >= 0]
    mean = F32(vis.mean()) if vis.size else F32(0)
    return min(mean, F32(occ_thre)), F32(o.mean())


def ulp_apart(a, b):
    a, b = F32(a), F32(b)
    return a == b or np.nextafter(a, b) == b


def threshold_input(n, kind):
    rs = np.random.RandomState(n % 9973 + len(kind))
    o = (rs.rand(n) ** 3).astype(F32)
    if kind == "all_invisible":
        o[:] = -1
    elif kind == "some_invisible":
        o[rs.rand(n) < 0.3] = -1
        o[n - 1] = 0.75                                         # the last element is visible: the tail counts
    return o


# ================================================================================================= march

def make_grid(L, R, roi, F=float):
    """Grid as the host's make_grid (fp32), its numbers then taken into F."""
    r = [F32(v) for v in roi]
    c = [F32(0.5) * (r[a] + r[3 + a]) for a in range(3)]
    h = [F32(0.5) * (r[3 + a] - r[a]) for a in range(3)]
    return dict(L=L, R=R, c=[F(v) for v in c], h=[F(v) for v in h], roi=[float(v) for v in r])


def _level(F, s):
    if not s > 1:
        return 0
    if F is float:
        m, e = math.frexp(s)
        return e - 1 if m == 0.5 else e
    return int(math.ceil(np.log2(s)))                           # ceilf(log2f(s)), as the kernel


def cell_of(F, G, p):
    """-> (id, level, cmin, csz) or None outside the outermost level."""
    R = G["R"]
    s = F(0.0)
    for a in range(3):
        s = max(s, abs(p[a] - G["c"][a]) / G["h"][a])
    l = _level(F, s)
    if l >= G["L"]:
        return None
    scale = F(1 << l)
    ci, cmin, csz = [], [], []
    for a in range(3):
        mn = G["c"][a] - G["h"][a] * scale
        sz = F(2.0) * G["h"][a] * scale
        k = int(math.floor((p[a] - mn) / sz * F(R)))
        k = 0 if k < 0 else (R - 1 if k >= R else k)
        ci.append(k)
        csz.append(sz / F(R))
        cmin.append(mn + F(k) * csz[a])
    return l * R ** 3 + (ci[0] * R + ci[1]) * R + ci[2], l, cmin, csz


E12 = float(F32(1e-12))


def march_ray(F, G, binr, o, d, t, tf, step, cone, max_steps, fault=None):
    """march_ray of occ.hip in the arithmetic F (float or numpy.float32), one rounding per operation.
    fault: None | "skip_k_minus_1" | "skip_k_plus_1" | "mid_at_t" (planted, for the teeth tests)."""
    eps, big = F(E12), F(1 << (G["L"] - 1))
    for a in range(3):
        lo, hi = G["c"][a] - G["h"][a] * big, G["c"][a] + G["h"][a] * big
        if abs(d[a]) < eps:
            if o[a] < lo or o[a] > hi:
                tf = F(-1.0)
            continue
        ta, tb = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
        t, tf = max(t, min(ta, tb)), min(tf, max(ta, tb))
    out, it = [], 0
    while t < tf and it < max_steps:
        it += 1
        dt = min(max(t * cone, step), F(F32(1e10)))
        mid = t + F(0.5) * dt
        if mid >= tf:
            break
        at = t if fault == "mid_at_t" else mid
        cell = cell_of(F, G, [o[a] + d[a] * at for a in range(3)])
        if cell is None:
            break
        cid, _, cmin, csz = cell
        if binr[cid]:
            out.append((t, t + dt))
            t = t + dt
        else:
            te = math.inf
            for a in range(3):
                if abs(d[a]) > eps:
                    te = min(te, ((cmin[a] + csz[a] if d[a] > 0 else cmin[a]) - o[a]) / d[a])
            if te == math.inf:
                break
            k = math.ceil((te - t) / dt)
            if fault == "skip_k_minus_1":
                k -= 1
            if fault == "skip_k_plus_1":
                k += 1
            t = t + F(max(1, k)) * dt
    return out


def box_hit(F, ray, box):
    """The multi-expert box prefilter of march_multi_kernel."""
    tmin, tmax = -math.inf, math.inf
    big = F(1.0) / F(F32(1e-9))
    for a in range(3):
        dd = ray[3 + a]
        inv = F(1.0) / dd if abs(dd) > F(F32(1e-9)) else big
        ta, tb = (F(F32(box[a])) - ray[a]) * inv, (F(F32(box[3 + a])) - ray[a]) * inv
        tmin, tmax = max(tmin, min(ta, tb)), min(tmax, max(ta, tb))
    return min(tmax, ray[7]) > max(tmin, ray[6])


def march(case, F=float, fault=None):
    """nerf_occ_march on a case of march_case(): -> (counts int32 (N), ray_idx int32, t0, t1 in F as float64)."""
    return march_multi([case], case["rays"], case, F, fault)


def march_multi(experts, rays, run, F=float, fault=None):
    """nerf_occ_march_multi: experts = dicts with grid, bin, step (and box, except for the single march); run holds
    near_plane, far_plane, max_steps, u (explicit jitter, single march only) or seed (multi) or neither.
    counts are expert-major (K N); samples follow in that order with ray_idx = r."""
    N = rays.shape[0]
    counts, ri, t0, t1 = [], [], [], []
    for k, e in enumerate(experts):
        G = make_grid(e["L"], e["R"], e["roi"], F)
        step = F(F32(e["step"]))
        for r in range(N):
            ry = [F(v) for v in rays[r]]
            segs = []
            if "box" not in e or box_hit(F, ry, e["box"]):
                t, tf = max(F(F32(run["near_plane"])), ry[6]), min(F(F32(run["far_plane"])), ry[7])
                if run.get("u") is not None:
                    t = t + F(run["u"][r]) * step
                elif run.get("seed") is not None:
                    t = F(F32(float(t) + uniform(run["seed"], 0x0CC00 + k, r) * float(step)))
                segs = march_ray(F, G, e["bin"], ry[:3], ry[3:6], t, tf, step, F(F32(run.get("cone", 0.0))),
                                 run["max_steps"], fault)
            counts.append(len(segs))
            ri += [r] * len(segs)
            t0 += [float(s[0]) for s in segs]
            t1 += [float(s[1]) for s in segs]
    return (np.array(counts, dtype=np.int32), np.array(ri, dtype=np.int32), np.array(t0, dtype=np.float64),
            np.array(t1, dtype=np.float64))


MARCH_GRIDS = {
    "cube1": dict(L=1, R=16, roi=[-1, -1, -1, 1, 1, 1], step=1 / 16),
    "flat2": dict(L=2, R=16, roi=[-1, -0.5, 0, 1, 0.5, 0.5], step=1 / 16),
    "off2": dict(L=2, R=8, roi=[0.5, -1.5, -0.25, 1.5, -0.5, 0.75], step=1 / 32),
    "cube3": dict(L=3, R=8, roi=[-1, -1, -1, 1, 1, 1], step=1 / 8),
}
NEAR_PLANE, FAR_PLANE = 0.25, 12.0
# (grid, binary, N, explicit u, max_steps)
MARCH_CASES = [
    ("cube1", "random", 129, False, 4096), ("cube1", "full", 128, True, 4096), ("cube1", "empty", 127, False, 4096),
    ("cube1", "random", 1, False, 4096), ("flat2", "random", 129, True, 4096), ("flat2", "full", 127, False, 4096),
    ("flat2", "random", 128, False, 5), ("off2", "random", 129, False, 4096), ("off2", "full", 128, True, 7),
    ("cube3", "random", 129, True, 4096), ("cube3", "full", 127, False, 4096), ("cube3", "empty", 128, True, 4096),
    ("cube3", "random", 128, False, 6),
]
_Q = [0.0, 0.25, 0.5, 1.0]


def _quant(x):
    """|x| in [0, 1] -> the nearest of {0, 1/4, 1/2, 1}."""
    return min(_Q, key=lambda q: abs(q - x))


def dyadic_rays(g, N, seed):
    """(N, 8) float32 rays of the dyadic family for grid g: of every 8 rays, 2 start inside the grid, 1 points away
    (a miss), 2 are parallel to an axis (one of them along the grid's outermost face), 3 start outside aimed at a
    lattice point of the ROI."""
    rs = np.random.RandomState(seed)
    G = make_grid(g["L"], g["R"], g["roi"])
    c, h = np.array(G["c"]), np.array(G["h"])
    H = h * 2 ** (g["L"] - 1)
    rays = np.zeros((N, 8), dtype=np.float64)
    for r in range(N):
        kind = r % 8
        target = c + h * rs.randint(-8, 9, 3) / 8.0
        a0, side = rs.randint(3), rs.choice([-1.0, 1.0])
        if kind < 2:
            o = c + np.round(H * rs.randint(-8, 9, 3) / 8.0 * 32) / 32
        else:
            o = c + np.round(H * rs.randint(-10, 11, 3) / 8.0 * 32) / 32
            o[a0] = c[a0] + side * (H[a0] + rs.randint(1, 65) / 32.0)
        delta = target - o
        if kind in (3, 4):                                      # parallel to axis a0, through the ROI
            o[np.arange(3) != a0] = target[np.arange(3) != a0]
            if kind == 4:                                       # along the outermost face: s = 2^(L-1) all the way
                a1 = (a0 + 1) % 3
                o[a1] = c[a1] + rs.choice([-1.0, 1.0]) * H[a1]
            d = np.zeros(3)
            d[a0] = -side * rs.choice([0.25, 0.5, 1.0])
        else:
            m = np.abs(delta).max()
            d = np.array([np.sign(x) * _quant(abs(x) / m) for x in delta]) if m > 0 else np.array([1.0, 0.5, 0.0])
            if kind == 2:
                d = -d
        if not d.any():
            d[a0] = 1.0
        rays[r, :3], rays[r, 3:6] = o, d
        rays[r, 6], rays[r, 7] = (0.0, 0.5)[rs.randint(2)], (16.0, 16.0, 16.0, 5.0)[rs.randint(4)]
    out = rays.astype(F32)
    assert (out.astype(np.float64) == rays).all()
    return out


def march_binary(g, kind, seed):
    n = g["L"] * g["R"] ** 3
    if kind == "empty":
        return np.zeros(n, dtype=np.uint8)
    if kind == "full":
        return np.ones(n, dtype=np.uint8)
    return (np.random.RandomState(seed).rand(n) < 0.4).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def march_case(i):
    name, kind, N, with_u, max_steps = MARCH_CASES[i]
    g = MARCH_GRIDS[name]
    case = dict(g, name=name, kind=kind, N=N, bin=march_binary(g, kind, 100 + i), rays=dyadic_rays(g, N, 200 + i),
                near_plane=NEAR_PLANE, far_plane=FAR_PLANE, max_steps=max_steps, cone=0.0,
                u=(np.arange(N) * 5 % 8 / 8.0).astype(F32) if with_u else None)
    return case


@functools.lru_cache(maxsize=None)
def march_expected(i):
    return march(march_case(i))


# two experts side by side along x, different grids and steps; boxes a little smaller than the grids' outer boxes
MULTI_EXPERTS = [
    dict(L=2, R=8, roi=[-1, -0.5, -0.5, 0, 0.5, 0.5], step=1 / 16, box=[-1.5, -1, -1, 0.5, 1, 1]),
    dict(L=1, R=16, roi=[0, -1, -1, 2, 1, 1], step=1 / 32, box=[0, -1, -1, 2, 1, 1]),
]
MULTI_N = 129
STAGE_CAPS = [1, 3, 512]


@functools.lru_cache(maxsize=None)
def multi_case():
    """Of every 8 rays: one along +x on the face y = 1 of both boxes (the prefilter's y slab is [-2e9, 0]: dropped),
    one along +x on the face y = -1 (slab [0, 2e9]: kept, marched along the level face s = 2 of expert 0 and the
    outer face of expert 1), one starting inside box 1; the rest generic, some missing either box."""
    experts = [dict(e, bin=march_binary(e, "random", 300 + k)) for k, e in enumerate(MULTI_EXPERTS)]
    rays = dyadic_rays(dict(L=2, R=8, roi=[-1, -1, -1, 2, 1, 1]), MULTI_N, 310)
    for r in range(0, MULTI_N - 2, 8):
        rays[r, :6] = [-3.0, 1.0, (r % 16) / 16.0 - 0.5, 1.0, 0.0, 0.0]
        rays[r + 1, :6] = [-3.0, -1.0, (r % 16) / 16.0 - 0.5, 1.0, 0.0, 0.0]
        rays[r + 2, :3] = [0.5 + (r % 32) / 32.0, (r % 8) / 8.0 - 0.5, 0.25]
        rays[r + 2, 6] = 0.0
    run = dict(near_plane=NEAR_PLANE, far_plane=FAR_PLANE, max_steps=4096, cone=0.0)
    return experts, rays, run


@functools.lru_cache(maxsize=None)
def multi_expected():
    experts, rays, run = multi_case()
    return march_multi(experts, rays, run)


def clamp_capacities(counts, cap):
    """Capacities for the clamped-offset tests, from the unclamped counts (K N) and a stage cap: 0, 1, the middle of
    a staged pair (1 < count <= cap), the middle of an overflowing pair (count > cap), a pair boundary, M, M + 5.
    Kinds that do not occur for this cap are left out."""
    offs = exclusive_scan(counts).astype(np.int64)
    M = int(offs[-1])
    out = {0, 1, M, M + 5}
    staged = [j for j in range(len(counts)) if 1 < counts[j] <= cap and offs[j] > 0]
    over = [j for j in range(len(counts)) if counts[j] > max(cap, 1) and offs[j] > 0]
    edge = [j for j in range(len(counts)) if counts[j] > 0 and 0 < offs[j] < M]
    if staged:
        j = staged[len(staged) // 2]
        out.add(int(offs[j] + counts[j] // 2))
    if over:
        j = over[len(over) // 2]
        out.add(int(offs[j] + counts[j] // 2))
    if edge:
        out.add(int(offs[edge[len(edge) // 2]]))
    return sorted(out)


# ================================================================================================= packed compositing

def packed_lengths(N, shift=0):
    return [RAY_LENGTHS[(r * 3 + shift + N) % len(RAY_LENGTHS)] for r in range(N)]


PACKED_CASES = {f"N{N}": packed_lengths(N) for N in PACKED_N}
PACKED_CASES.update({
    "all_lengths": list(RAY_LENGTHS),
    "trailing_empty": [64, 129, 0, 0, 0],
    "all_empty": [0, 0, 0],
    "saturated": [129, 65, 5],          # ray 0 saturates (sigma 1e4), ray 1 has sigma = 0 throughout
})


@functools.lru_cache(maxsize=None)
def packed_case(name):
    lens = PACKED_CASES[name]
    N, M = len(lens), sum(lens)
    rs = np.random.RandomState(1000 + sum(map(ord, name)))
    offs = exclusive_scan(lens)
    dt = (rs.rand(M) * 0.05 + 1e-3)
    t0 = np.zeros(M)
    for r in range(N):
        a, b = offs[r], offs[r + 1]
        t0[a:b] = 2.0 + np.cumsum(dt[a:b]) - dt[a:b]
    t0 = t0.astype(F32)
    t1 = (t0 + dt).astype(F32)
    rsig = np.concatenate([rs.rand(M, 3), np.exp(rs.randn(M, 1) * 2)], 1).astype(F32)
    if name == "saturated":
        rsig[offs[0]:offs[1], 3] = 1e4
        rsig[offs[1]:offs[2], 3] = 0.0
    return dict(name=name, N=N, M=M, offs=offs, t0=t0, t1=t1, rs=rsig, bg=rs.rand(N, 3).astype(F32),
                g_rgb=rs.randn(N, 3).astype(F32), g_depth=rs.randn(N).astype(F32), g_acc=rs.randn(N).astype(F32),
                g_w=rs.randn(M).astype(F32))


def _ray_terms(case, r, fault=None):
    """float64 per-sample quantities of ray r and their forward bounds."""
    a, b = int(case["offs"][r]), int(case["offs"][r + 1])
    t0, t1 = case["t0"][a:b].astype(np.float64), case["t1"][a:b].astype(np.float64)
    sig = case["rs"][a:b, 3].astype(np.float64)
    dt = t1 - t0
    sdt = sig * dt
    I = np.cumsum(sdt)
    E = I - sdt
    if fault == "inclusive_T":
        E = I
    if fault == "no_carry":                                      # the sum restarts at every 64-sample chunk
        k = np.arange(b - a)
        first = (k // 64) * 64
        E = E - np.where(first > 0, I[np.maximum(first - 1, 0)], 0.0)
    c = np.arange(b - a) // 64
    T, ex = np.exp(-E), np.exp(-sdt)
    al = 1.0 - ex
    w = T * al
    dE = (10 + c) * U * I
    dT = T * (dE + 2 * U) + TINY
    dal = ex * (2 * U + 2 * U * sdt) + U * al
    dw = T * dal + al * dT + U * w + TINY
    Tn = np.exp(-I)
    dTn = Tn * ((9 + c) * U * I + 2 * U) + TINY
    return dict(a=a, b=b, dt=dt, tm=0.5 * (t0 + t1), I=I, T=T, al=al, w=w, dT=dT, dal=dal, dw=dw, Tn=Tn, dTn=dTn,
                nch=max(1, -(-(b - a) // 64)))


def packed_forward(case, with_bg=True, fault=None):
    """-> value and bound (twice the first-order count) of weights (M), rgb (N, 3), depth (N), acc (N)."""
    N, M = case["N"], case["M"]
    v = dict(w=np.zeros(M), rgb=np.zeros((N, 3)), depth=np.zeros(N), acc=np.zeros(N))
    e = dict(w=np.zeros(M), rgb=np.zeros((N, 3)), depth=np.zeros(N), acc=np.zeros(N))
    for r in range(N):
        q = _ray_terms(case, r, fault)
        a, b, n = q["a"], q["b"], q["nch"] + 7
        col = case["rs"][a:b, :3].astype(np.float64)
        v["w"][a:b], e["w"][a:b] = q["w"], q["dw"]
        v["rgb"][r] = (q["w"][:, None] * col).sum(0)
        e["rgb"][r] = (q["dw"][:, None] * col).sum(0) + n * U * (q["w"][:, None] * col).sum(0) + TINY
        v["depth"][r] = (q["w"] * q["tm"]).sum()
        e["depth"][r] = (q["dw"] * q["tm"]).sum() + (n + 1) * U * v["depth"][r] + TINY
        v["acc"][r] = q["w"].sum()
        e["acc"][r] = q["dw"].sum() + n * U * v["acc"][r] + TINY
        if with_bg:
            bg = case["bg"][r].astype(np.float64)
            e["rgb"][r] += bg * (e["acc"][r] + 2 * U) + 2 * U * (v["rgb"][r] + bg)
            v["rgb"][r] = v["rgb"][r] + (1.0 - v["acc"][r]) * bg
    return v, {k: 2 * x for k, x in e.items()}


def packed_backward(case, with_bg=True, with_depth=True, with_acc=True, with_gw=True, fault=None):
    """-> value and bound (twice the first-order count) of d_rgb_sigma (M, 4)."""
    N, M = case["N"], case["M"]
    val, err = np.zeros((M, 4)), np.zeros((M, 4))
    for r in range(N):
        q = _ray_terms(case, r)
        a, b = q["a"], q["b"]
        if a == b:
            continue
        col = case["rs"][a:b, :3].astype(np.float64)
        g = case["g_rgb"][r].astype(np.float64)
        gd = float(case["g_depth"][r]) if with_depth else 0.0
        ga = float(case["g_acc"][r]) if with_acc else 0.0
        gw = case["g_w"][a:b].astype(np.float64) if with_gw else np.zeros(b - a)
        bgdot, bgabs = 0.0, 0.0
        if with_bg:
            bg = case["bg"][r].astype(np.float64)
            bgdot, bgabs = float((g * bg).sum()), float(np.abs(g * bg).sum())
        gk = (col * g).sum(1) + gd * q["tm"] + (ga - bgdot) + gw
        Gk = (col * np.abs(g)).sum(1) + abs(gd) * q["tm"] + abs(ga) + bgabs + np.abs(gw)
        dg = 8 * U * Gk
        w, dw = q["w"], q["dw"]
        qk = gk * w
        ek = np.abs(gk) * dw + w * dg + U * np.abs(qk)
        A = ek.sum() + (q["nch"] + 7) * U * np.abs(qk).sum()
        prefix = np.cumsum(qk)
        if fault == "no_carry":
            k = np.arange(b - a)
            first = (k // 64) * 64
            prefix = prefix - np.where(first > 0, prefix[np.maximum(first - 1, 0)], 0.0)
        suffix = qk.sum() - prefix
        dsdt = gk * q["Tn"] - suffix
        val[a:b, :3] = w[:, None] * g
        err[a:b, :3] = dw[:, None] * np.abs(g) + U * np.abs(val[a:b, :3]) + TINY
        val[a:b, 3] = dsdt * q["dt"]
        err[a:b, 3] = q["dt"] * (q["Tn"] * dg + np.abs(gk) * q["dTn"] + 2 * A
                                 + U * (np.abs(gk * q["Tn"]) + np.abs(suffix)) + 3 * U * np.abs(dsdt)) + TINY
    return val, 2 * err


def packed_autograd(case, with_bg=True, with_depth=True, with_acc=True, with_gw=True):
    """d_rgb_sigma by float64 autograd through an independent composite (torch cumsum per ray)."""
    rs = torch.tensor(case["rs"], dtype=torch.float64, requires_grad=True)
    t0, t1 = torch.tensor(case["t0"], dtype=torch.float64), torch.tensor(case["t1"], dtype=torch.float64)
    loss = rs.sum() * 0
    for r in range(case["N"]):
        a, b = int(case["offs"][r]), int(case["offs"][r + 1])
        sdt = rs[a:b, 3] * (t1[a:b] - t0[a:b])
        T = torch.exp(-(torch.cumsum(sdt, 0) - sdt))
        w = T * (1 - torch.exp(-sdt))
        acc = w.sum()
        rgb = (w[:, None] * rs[a:b, :3]).sum(0)
        if with_bg:
            rgb = rgb + (1 - acc) * torch.tensor(case["bg"][r], dtype=torch.float64)
        loss = loss + (rgb * torch.tensor(case["g_rgb"][r], dtype=torch.float64)).sum()
        if with_depth:
            loss = loss + float(case["g_depth"][r]) * (w * 0.5 * (t0[a:b] + t1[a:b])).sum()
        if with_acc:
            loss = loss + float(case["g_acc"][r]) * acc
        if with_gw:
            loss = loss + (w * torch.tensor(case["g_w"][a:b], dtype=torch.float64)).sum()
    loss.backward()
    return rs.grad.numpy()


def worst_ratio(got, ref, bound):
    got = _np(got).astype(np.float64)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all()
    return float((np.abs(got - ref) / bound).max())


# ================================================================================================= visibility

VIS_EPS = 1e-2
VIS_ATHR = 0.05


def vis_group_thresholds(n_groups, seed):
    """Per-group thresholds above and below the global one, at 0 and below 0, cyclically."""
    vals = [0.2, 0.01, 0.0, -1.0, VIS_ATHR]
    return np.array([vals[(g + seed) % len(vals)] for g in range(n_groups)], dtype=F32)


def visibility(case, eps, athr, groups=None, group=1, fault=None):
    """-> (keep bool (M), decided bool (M)): the float64 decision and where it is outside the bound."""
    M = case["M"]
    keep, decided = np.zeros(M, dtype=bool), np.zeros(M, dtype=bool)
    eps, athr = float(F32(eps)), F32(athr)
    for r in range(case["N"]):
        q = _ray_terms(case, r)
        a, b = q["a"], q["b"]
        th = athr
        if groups is not None:
            th = min(athr, groups[r if fault == "group_by_ray" else r // group])
        th = float(th)
        kT, dT_ok = q["T"] >= eps, np.abs(q["T"] - eps) > 2 * q["dT"]
        if th <= 0:
            keep[a:b], decided[a:b] = kT, dT_ok
        else:
            ka, da_ok = q["al"] >= th, np.abs(q["al"] - th) > 2 * q["dal"]
            keep[a:b] = kT & ka
            # surely dropped if either test surely fails; surely kept only if both surely pass
            decided[a:b] = (dT_ok & ~kT) | (da_ok & ~ka) | (dT_ok & da_ok)
    return keep, decided


# ================================================================================================= packed points

POINT_COUNTS = [0, 1, 255, 256, 257]
POINT_CAPACITY = 300


def packed_points(rays, ri, t0, t1):
    """x = o + d * t_mid with t_mid = 0.5 (t0 + t1) in float64 -> (x (M, 3), bound (M, 3), directions float32 (M, 3)).
    t_mid rounds once, the product and the sum once each (or once together as an fma), so positions are compared
    under 2u (|o| + 2 |d t_mid|); the directions are copies."""
    rr = _np(rays)[_np(ri).astype(np.int64)]
    r64 = rr.astype(np.float64)
    tm = 0.5 * (_np(t0).astype(np.float64) + _np(t1).astype(np.float64))
    x = r64[:, :3] + r64[:, 3:6] * tm[:, None]
    bound = 2 * U * (np.abs(r64[:, :3]) + 2 * np.abs(r64[:, 3:6] * tm[:, None])) + TINY
    return x, bound, rr[:, 3:6].copy()


# ================================================================================================= cell points

CELL_GRIDS = [dict(L=1, R=16, roi=[-1, -1, -1, 1, 1, 1]), dict(L=2, R=8, roi=[-1, -0.5, 0, 1, 0.5, 0.5]),
              dict(L=3, R=4, roi=[0.5, -1.5, -0.25, 1.5, -0.5, 0.75])]


def cell_points_input(g, n, seed):
    rs = np.random.RandomState(seed)
    total = g["L"] * g["R"] ** 3
    cells = rs.randint(0, total, n).astype(np.int32)
    cells[::7] = -1
    cells[1], cells[2] = 0, total - 1
    return cells


def cell_points(g, cells, seed):
    """-> (x float64 (n, 3), bound (n, 3), lo, hi (n, 3) the cell's closed box; the ROI centre for empty slots)."""
    G = make_grid(g["L"], g["R"], g["roi"])
    R, cpl = g["R"], g["R"] ** 3
    c, h = np.array(G["c"]), np.array(G["h"])
    n = len(cells)
    x, bound, lo, hi = (np.zeros((n, 3)) for _ in range(4))
    for i, cid in enumerate(_np(cells).tolist()):
        if cid < 0:
            x[i], lo[i], hi[i] = c, c, c
            continue
        l, q = divmod(cid, cpl)
        ci = np.array([q // (R * R), (q // R) % R, q % R], dtype=np.float64)
        un = np.array([uniform(seed, i, a) for a in range(3)])
        mn, ext = c - h * 2 ** l, 2 * h * 2 ** l
        x[i] = mn + (ci + un) / R * ext
        bound[i] = 4 * U * (np.abs(mn) + np.abs(ext))
        lo[i], hi[i] = mn + ci / R * ext, mn + (ci + 1) / R * ext
    return x, bound, lo, hi


# ================================================================================================= mark invisible

INVIS_W, INVIS_H, INVIS_NEAR = 64, 48, 0.25
INVIS_GRIDS = [dict(L=1, R=16, roi=[-1, -1, -1, 1, 1, 1]), dict(L=3, R=8, roi=[-1, -0.5, 0, 1, 0.5, 0.5])]


def _rot(axis, deg):
    t = math.radians(deg)
    cs, sn = math.cos(t), math.sin(t)
    m = {0: [[1, 0, 0], [0, cs, -sn], [0, sn, cs]], 1: [[cs, 0, sn], [0, 1, 0], [-sn, 0, cs]],
         2: [[cs, -sn, 0], [sn, cs, 0], [0, 0, 1]]}[axis]
    return np.array(m)


def invisible_cameras(which):
    """-> (K (n, 3, 3), c2w (n, 3, 4)) float32.  which: "front" one axis-aligned camera at z = -2 looking down +z (a little off the axis: on it whole rows
    of cell centres project exactly onto the image border);
    "rotated" two cameras turned about y and x; "behind" a camera looking away from the grid (sees nothing);
    "inside" a camera at the ROI centre (zc crosses near_plane inside the grid; u, v cross 0, W, H);
    "none" no camera."""
    Kmat = np.array([[40.0, 0, INVIS_W / 2], [0, 40.0, INVIS_H / 2], [0, 0, 1]])
    cams = {
        "front": [(np.eye(3), [0.011, -0.007, -2.0])],
        "rotated": [(_rot(1, 25.0) @ _rot(0, -10.0), [-2.0, 0.5, -3.0]), (_rot(0, 40.0), [0.25, 2.5, -2.0])],
        "behind": [(_rot(1, 180.0), [0.0, 0.0, -4.0])],
        "inside": [(_rot(2, 15.0), [0.03, 0.02, 0.26])],
        "none": [],
    }[which]
    n = len(cams)
    K, c2w = np.zeros((n, 3, 3), dtype=F32), np.zeros((n, 3, 4), dtype=F32)
    for i, (Rm, t) in enumerate(cams):
        K[i] = Kmat
        c2w[i, :, :3], c2w[i, :, 3] = Rm, t
    return K, c2w


INVIS_CAMERAS = ["front", "rotated", "behind", "inside", "none"]


def mark_invisible(g, K, c2w, W, H, near):
    """-> (visible bool (cells), decided bool (cells)) in float64 from the fp32 K and c2w."""
    G = make_grid(g["L"], g["R"], g["roi"])
    R, L = g["R"], g["L"]
    c, h = np.array(G["c"]), np.array(G["h"])
    near = float(F32(near))
    idx = np.stack(np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij"), -1).reshape(-1, 3)
    xs, dxs = [], []
    for l in range(L):
        ext = 2 * h * 2 ** l
        xs.append(c - h * 2 ** l + (idx + 0.5) / R * ext)
        dxs.append(np.broadcast_to(4 * U * (np.abs(c) + ext), (idx.shape[0], 3)))
    x, dx = np.concatenate(xs), np.concatenate(dxs)
    sure, maybe = np.zeros(len(x), dtype=bool), np.zeros(len(x), dtype=bool)
    for i in range(K.shape[0]):
        P, k = c2w[i].astype(np.float64), K[i].astype(np.float64)
        d = x - P[:, 3]
        dd = dx + U * np.abs(d)
        cam = d @ P[:, :3]                                        # R^T (x - t): column j of R dotted with d
        ecam = dd @ np.abs(P[:, :3]) + 3 * U * (np.abs(d) @ np.abs(P[:, :3]))
        zc, ez = cam[:, 2], ecam[:, 2]
        amb = np.abs(zc - near) <= 2 * ez
        cam_yes, cam_no = (zc > near) & ~amb, ~(zc > near) & ~amb
        zs = np.where(np.abs(zc) > 0, zc, 1.0)
        for row, lim in ((0, float(W)), (1, float(H))):
            num = cam @ k[row]
            dnum = ecam @ np.abs(k[row]) + 3 * U * (np.abs(cam) @ np.abs(k[row]))
            p = num / zs
            dp = (dnum + np.abs(p) * ez) / np.abs(zs) + U * np.abs(p)
            inside = (p >= 0) & (p < lim)
            amb = (np.abs(p) <= 2 * dp) | (np.abs(p - lim) <= 2 * dp)
            cam_yes &= inside & ~amb
            cam_no |= ~inside & ~amb
        sure |= cam_yes
        maybe |= ~(cam_yes | cam_no)
    return sure, sure | ~maybe


# ================================================================================================= cone march

# (L, R, roi, cone, density, seed)
CONE_CASES = [
    (2, 16, [-1, -1, -1, 1, 1, 1], 1 / 256, 0.5, 1),
    (3, 8, [-1, -0.5, 0, 1, 0.5, 0.5], 0.004, 0.3, 2),
    (1, 16, [-1, -1, -1, 1, 1, 1], 0.01, 0.5, 3),
]
CONE_N = 200


@functools.lru_cache(maxsize=None)
def cone_case(i):
    """Generic rays (normalised fp32 directions, nothing on a lattice) from around (0.1, -3, 0.2) towards +y."""
    L, R_, roi, cone, density, seed = CONE_CASES[i]
    rs = np.random.RandomState(500 + seed)
    o = np.array([0.1, -3.0, 0.2]) + rs.randn(CONE_N, 3) * 0.1
    d = rs.randn(CONE_N, 3) * 0.35 + np.array([0.0, 1.0, 0.0])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((CONE_N, 1), 0.5), np.full((CONE_N, 1), 6.0)], 1).astype(F32)
    g = dict(L=L, R=R_, roi=roi, step=float(F32(2.0 * 3 ** 0.5 / 256)))
    return dict(g, N=CONE_N, bin=(rs.rand(L * R_ ** 3) < density).astype(np.uint8), rays=rays, near_plane=0.0,
                far_plane=1e10, max_steps=4096, cone=float(F32(cone)), u=None)


def _cell64(G, p, dp):
    """Cell of p in float64 -> (id or None outside, cmin, csz, ambiguous).  dp: bound on the kernel's error in p.
    s_a = |p_a - c_a| / h_a carries dp_a / h_a + 2u s_a; ceil(log2f(s)) may be off within 4u s of a power of two.
    The cell coordinate q_a = (p_a - mn_a) / sz_a R carries (dp_a + u |mn_a|) / sz_a R + 3u q_a.  A decision
    within twice its error of a level face or a cell face is ambiguous."""
    L, R_ = G["L"], G["R"]
    s, ds = 0.0, 0.0
    for a in range(3):
        sa = abs(p[a] - G["c"][a]) / G["h"][a]
        if sa >= s:
            s, ds = sa, dp[a] / G["h"][a] + 2 * U * sa
        ds = max(ds, dp[a] / G["h"][a] + 2 * U * sa)
    amb = any(abs(s - 2.0 ** j) <= 2 * (ds + 4 * U * s) for j in range(L))
    l = _level(float, s)
    if l >= L:
        return None, None, None, amb
    scale = float(1 << l)
    ci, cmin, csz = [], [], []
    for a in range(3):
        mn, sz = G["c"][a] - G["h"][a] * scale, 2.0 * G["h"][a] * scale
        q = (p[a] - mn) / sz * R_
        dq = (dp[a] + U * abs(mn)) / sz * R_ + 3 * U * abs(q)
        n = round(q)
        if 0 < n < R_ and abs(q - n) <= 2 * dq:
            amb = True
        k = min(max(int(math.floor(q)), 0), R_ - 1)
        ci.append(k)
        csz.append(sz / R_)
        cmin.append(mn + k * sz / R_)
    return l * R_ ** 3 + (ci[0] * R_ + ci[1]) * R_ + ci[2], cmin, csz, amb


def _clip64(G, o, d, t, tf):
    big = float(1 << (G["L"] - 1))
    for a in range(3):
        lo, hi = G["c"][a] - G["h"][a] * big, G["c"][a] + G["h"][a] * big
        if abs(d[a]) < E12:
            if o[a] < lo or o[a] > hi:
                tf = -1.0
            continue
        ta, tb = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
        t, tf = max(t, min(ta, tb)), min(tf, max(ta, tb))
    return t, tf


def cone_replay(G, binr, o, d, t, et, tf, step, cone):
    """The float64 marcher from t (known to the kernel within et) to its next emitted sample.
    -> ("emit", t, et) | ("end", t, et) | ("ambiguous", t, et).
    One evaluation of the kernel rounds: dt = fl(t cone) (u), mid = t + dt / 2 (u, an fma): emid = et (1 + cone / 2)
    + 1.5u mid; p_a = o_a + d_a mid (u, an fma): dp_a = |d_a| emid + u |p_a|; tf = (face - o) / d: 2u |tf|;
    te_a = (face_a - o_a) / d_a with face = mn + k csz (3u (|cmin| + csz)): dte = (dface + u |face - o|) / |d| + u |te|;
    x = (te - t) / dt: dx = (dte + et + u |te - t|) / dt + |x| (2u + et / t); t' = t + k dt (an fma):
    et' = et + k dt (u + et / t) + u t'."""
    etf = 2 * U * abs(tf)
    while True:
        dt = min(max(t * cone, step), 1e10)
        mid = t + 0.5 * dt
        emid = et * (1 + 0.5 * cone) + 1.5 * U * abs(mid)
        if abs(mid - tf) <= 2 * (emid + etf):
            return "ambiguous", t, et
        if mid >= tf:
            return "end", t, et
        p = [o[a] + d[a] * mid for a in range(3)]
        dp = [abs(d[a]) * emid + U * abs(p[a]) for a in range(3)]
        cid, cmin, csz, amb = _cell64(G, p, dp)
        if amb:
            return "ambiguous", t, et
        if cid is None:
            return "end", t, et
        if binr[cid]:
            return "emit", t, et
        te, dte = math.inf, 0.0
        for a in range(3):
            if abs(d[a]) > E12:
                face = cmin[a] + csz[a] if d[a] > 0 else cmin[a]
                ta = (face - o[a]) / d[a]
                dte = max(dte, (3 * U * (abs(cmin[a]) + csz[a]) + U * abs(face - o[a])) / abs(d[a]) + U * abs(ta))
                te = min(te, ta)
        x = (te - t) / dt
        dx = (dte + et + U * abs(te - t)) / dt + abs(x) * (2 * U + et / max(t, 1e-30))
        n = round(x)
        if n >= 1 and abs(x - n) <= 2 * dx:
            return "ambiguous", t, et
        k = max(1, math.ceil(x))
        t2 = t + k * dt
        et = et + k * dt * (U + et / max(t, 1e-30)) + U * abs(t2)
        t = t2


def cone_checks(case, counts, t0, t1):
    """The one-step checks of a cone march's own output (counts (N), packed fp32 t0 / t1):
      dt        t1[i] is within 1 ulp of fl(t0[i] + clamp(t0[i] cone, step, 1e10));
      occupied  the cell of the sample's midpoint, in float64 from t0[i], is occupied;
      next      the float64 marcher from t1[i] emits next at t0[i + 1] (exactly when no cell is skipped, else within
                twice the accumulated bound), or ends if i is the ray's last sample;
      first     the same from the ray's start to its first sample (or to the end for a ray without samples).
    occupied / next / first are left out where a decision of the replay is ambiguous (cone_replay).
    -> dict(failed=[(check, ray, sample)], left_out, checked)."""
    G = make_grid(case["L"], case["R"], case["roi"])
    step, cone = float(F32(case["step"])), float(F32(case["cone"]))
    offs = exclusive_scan(counts).astype(np.int64)
    failed, left, checked = [], 0, 0
    t0, t1 = _np(t0).astype(np.float64), _np(t1).astype(np.float64)

    def follow(what, r, j, start, et, tf, want):
        nonlocal left, checked
        kind, t, e = cone_replay(G, case["bin"], o, d, start, et, tf, step, cone)
        if kind == "ambiguous":
            left += 1
            return
        checked += 1
        if want is None:
            ok = kind == "end"
        else:
            ok = kind == "emit" and (t == want if e == et == 0.0 else abs(t - want) <= 2 * e)
        if not ok:
            failed.append((what, r, j))

    for r in range(case["N"]):
        ry = [float(v) for v in case["rays"][r]]
        o, d = ry[:3], ry[3:6]
        a, b = int(offs[r]), int(offs[r + 1])
        ts, tf = _clip64(G, o, d, max(float(F32(case["near_plane"])), ry[6]), min(float(F32(case["far_plane"])), ry[7]))
        follow("first", r, -1, ts, 2 * U * abs(ts), tf, t0[a] if b > a else None)
        for j in range(a, b):
            checked += 1
            dt = min(max(t0[j] * cone, step), 1e10)
            if not ulp_apart(t1[j], F32(t0[j] + dt)):
                failed.append(("dt", r, j - a))
            mid = t0[j] + 0.5 * dt
            emid = 1.5 * U * abs(mid)
            p = [o[k] + d[k] * mid for k in range(3)]
            cid, _, _, amb = _cell64(G, p, [abs(d[k]) * emid + U * abs(p[k]) for k in range(3)])
            if amb:
                left += 1
            else:
                checked += 1
                if cid is None or not case["bin"][cid]:
                    failed.append(("occupied", r, j - a))
            follow("next", r, j - a, t1[j], 0.0, tf, t0[j + 1] if j + 1 < b else None)
    return dict(failed=failed, left_out=left, checked=checked)
