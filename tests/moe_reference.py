"""Plain-torch CPU references and deterministic inputs for the MoE container kernels (csrc/moe.hip) — TEST
INFRASTRUCTURE ONLY.  tests/test_gpu_moe_edges.py compares the kernels with these; tests/test_moe_reference.py checks
on the CPU that the references are right, that the inputs reach the edges they are built for and that the bounds
have teeth.

Exact operations (dispatch, gather, flag compaction, count scatter, mix, blend accumulation, segment union, the
constructed prefilter rays) are restated in integers or in fp32 with the kernels' operations in the kernels' order and
compared as bytes.  Operations that pass through a divide, a square root or expf are restated in float64 on the same
fp32 inputs and compared under a bound derived here by counting roundings; u = 2^-24 is the unit roundoff of fp32
(round to nearest, correctly rounded divide and sqrt), and every count is to first order in u.

ROUTING (route_kernel, soft weights).  Per centroid: three subtractions d_a = p_a - c_a (1 rounding each; float64
subtracts the same fp32 inputs exactly), three squares (1 each), two additions: a term of the sum carries at most
2 + 1 + 2 = 5 roundings, all terms are positive, so the sum is within 5u; the square root halves that and rounds
once: dist within 3.5u.  The reciprocal adds one: inv_k within 4.5u.  den adds K positive terms in sequence
(K - 1 roundings).  w_k = inv_k / den (1 rounding) gives, with e_j the relative error of inv_j,

    dw_k / w_k = (1 - w_k) e_k - sum_{j != k} w_j e_j - (additions) + (quotient)
    |dw_k| / w_k <= (9 (1 - w_k) + K) u.

The tests assert (K + 8) u.  The count above reaches that for w_k >= 1/9 and exceeds it by less than one u
below (and only with every rounding of the chain in one direction and all the weight of den on its first two terms);
the fp32 restatement on the CPU stays below 5 u for every K up to 32, so the bound is loose, yet far below the 1 / K
a dropped expert costs.  Masked-out weights are exactly 0.  The margin mask and the argmin are discontinuous, so rows
near a decision are left out (route_keep).

BLEND FINISH (blend_finish_kernel).  rgb = c / max(s, 1e-12f): one rounding of the float64 quotient of the same fp32
s and c; the tests allow 2^-23 = 2u relative.  The sigma channel max(s, 1e-12f) is exact.

BLEND BACKWARD (blend_bwd_kernel) against float64 autograd of rs = cat(c / s.clamp_min(t), s.clamp_min(t)),
t = float32(1e-12), from the same fp32 rows.  The kernel reads the saved fp32 s and mix = c / sn.  With rgb, sigma and
W non-negative every sum below has positive terms, so the errors are relative:
    s     K products, K - 1 additions                      <= K u
    c     2 products per term, K - 1 additions             <= (K + 1) u
    mix   c / sn, one more rounding                        <= (2 K + 2) u
  d rgb_c = ((w sigma) / sn) g_c: 3 roundings + s                        -> (K + 3) u |term|
  d sigma = g_w w + (w gdot) / sn, gdot = sum_c g_c (rgb_c - mix_c):
    rgb_c - mix_c: (2 K + 2) u |mix_c| + 1 u |rgb_c - mix_c|            <= (2 K + 3) u (|rgb_c| + |mix_c|)
    times g_c (1), the two additions of gdot (2), times w (1), / sn (1 + K for s), the final addition (1)
                                                                        -> (3 K + 9) u per unit of
    w / sn sum_c |g_c| (|rgb_c| + |mix_c|); the g_w w term carries 2 u.
The tests allow BLEND_BWD_K(K) 2^-23 = (3 K + 9) 2^-23 times the sum of the absolute values of the terms, twice the
first-order count.  A row with s = 0 is not live (the clamp passes no gradient and mix drops out of gdot): its
gradients are of order 1e12 and obey the same bound; a row with s == t exactly is live (>=).

BACKGROUND MLP (bg_fwd_kernel / bg_bwd_kernel) against float64 background_color / autograd.
  directions: squares (1 each) + 2 additions -> 3u, sqrt -> 2.5u, x / n -> 3.5u per component; the second
    normalisation sees components within 3.5u, its norm within 3.5 + 2.5 = 6u, its quotient 3.5 + 6 + 1 = 10.5u:
    C_D = 11.
  SH term e_i: a polynomial of degree g_i <= 3 in the components (g_i C_D), its fp32 constants (1 each), the
    operations on its longest path (0 for e_0, 1 at degree 1, 2 or 3 at degree 2, at most 5 at degree 3):
    |e_i - e_i64| <= R_SH[i] u A_i, R_SH = 1 | 13 x 3 | 25, 25, 27, 25, 26 | 39 x 7, and A_i the term evaluated with
    every monomial's absolute value.
  hidden s_j = sum_i W1_ji e_i + b1_j: a product (1), the additions that follow term i (16 - max(i, 1): the first
    is added to an exact 0) and the bias addition, N_ADD[i] = 18 - max(i, 1):
    Bh_j = u (sum_i (R_SH[i] + N_ADD[i]) |W1_ji| A_i + 2 |b1_j|); ReLU is 1-Lipschitz, so h_j is within Bh_j too.
  output o_c = sum_j W2_cj h_j + b2_c: Bo_c = sum_j |W2_cj| (Bh_j + (H + 2) u |h_j|) + 2 u |b2_c|.
  sigmoid: slope <= 1/4; expf (2u), the addition and the quotient (1 each) on a value <= 1:
    |out - out64| <= Bo_c / 4 + 4u.                                                      (bg_fwd_bound)
  backward, per ray: dz_c = g_c (sg (1 - sg)):  ddz_c = |g_c| (|1 - 2 sg| dsg + 3u sg (1 - sg)), dsg the forward
    bound; dh_j = mask sum_c W2_cj dz_c (1 product, 2 additions): ddh_j = sum_c |W2_cj| (ddz_c + 3u |dz_c|).
    Every d_w entry is a sum over the rays of products (1) added in ray order inside a 64-ray block (64) and then
    block by block (nblk): with n = 66 + nblk
      dW1_ji: sum_r ddh_rj A_ri + |dh_rj| R_SH[i] u A_ri + n u |dh_rj| A_ri
      db1_j : sum_r ddh_rj + n u |dh_rj|
      dW2_cj: sum_r ddz_rc |h_rj| + |dz_rc| Bh_rj + n u |dz_rc h_rj|
      db2_c : sum_r ddz_rc + n u |dz_rc|
    and the tests allow twice that (bg_bwd_bound).  A hidden unit whose float64 pre-activation lies within Bh_j of 0
    has an ambiguous mask: bg_directions() discards directions with such a unit within 64 Bh_j.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
U23 = 2.0 ** -23
T12 = float(np.float32(1e-12))   # the blend's clamp, as the kernel's 1e-12f
F32 = torch.float32
F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def rows_at_block_edge(cols):
    """Row counts n whose n * cols straddle the 256-thread block: the floor and ceiling of 255, 256, 257 over cols."""
    return sorted({max(1, v // cols) for v in (255, 256)} | {-(-v // cols) for v in (256, 257)})


# ================================================================================================= dispatch

DISPATCH_M = [1, 63, 64, 65, 255, 256, 257, 65536, 65537, 65793]
DISPATCH_K = [1, 3, 32]
DISPATCH_EPS = [0.0, 1e-8]
DISPATCH_CAP = 65793
DISPATCH_COUNTS = [0, 1, 255, 256, 257, DISPATCH_CAP, DISPATCH_CAP + 1000]


def owned_block(M):
    """The 256-row block one expert owns wholly: block 1 where it exists, else block 0 (None below 256 rows)."""
    return None if M < 256 else (1 if M >= 512 else 0)


def dispatch_special_rows(M, eps):
    """-> (row routed to no expert, row routed to all K), None where M has no room: the first rows outside
    owned_block(M) from row 2 on.  eps == 0 has only the first (its expert K-1 stays empty)."""
    free = [r for r in ((256, 257) if owned_block(M) == 0 else (2, 3)) if r < M]
    if eps == 0:
        return (free[0] if free else None), None
    return (free[1] if len(free) > 1 else None), (free[0] if free else None)


def dispatch_weights(M, K, eps):
    """Synthetic (M, K) fp32 weights, not from the router: about a third positive, the rest exactly eps, negative or
    0; W[M-1, K-1] == eps always (written last: at M = 256 it takes one row of the owned block from expert 0 when
    K = 1).  Expert 0 owns every row of owned_block(M).  The two requirements that exclude each other are split over
    eps: eps == 0 leaves expert K-1 (K > 1) without any row (so it owns none of the block either); eps > 0 routes
    one row to all K experts, and expert 1 owns none of the block.  dispatch_special_rows() names the row that
    routes nowhere and the row that routes everywhere."""
    g = gen(1000 * K + M % 997)
    e = float(np.float32(eps))
    cat = torch.randint(0, 6, (M, K), generator=g)
    pos = (torch.rand(M, K, generator=g) * 0.99 + 0.01).to(F32)
    W = torch.where(cat < 2, pos, torch.where(cat == 2, torch.full_like(pos, e),
                                              torch.where(cat == 3, -pos, torch.zeros_like(pos))))
    b = owned_block(M)
    if b is not None:
        W[256 * b:256 * (b + 1), 0] = pos[256 * b:256 * (b + 1), 0]
        if K > 1 and eps > 0:
            W[256 * b:256 * (b + 1), 1] = torch.where(cat[256 * b:256 * (b + 1), 1] < 3, e, -1.0)
    none_row, all_row = dispatch_special_rows(M, eps)
    if none_row is not None:
        W[none_row] = torch.where(cat[none_row] < 3, e, -0.5)
    if all_row is not None:
        W[all_row] = pos[all_row]
    if K > 1 and eps == 0:
        W[:, K - 1] = torch.where(cat[:, K - 1] < 3, e, -pos[:, K - 1])
    W[M - 1, K - 1] = e
    return W.contiguous()


def dispatch_reference(W, eps, count=None):
    """-> (offsets (K+1) int32, idx int32): per expert the rows with W[m, k] > eps (fp32 comparison, strict) in
    ascending order — torch.nonzero's — concatenated expert-major.  count: rows at and past min(count, M) route
    nowhere."""
    M, K = W.shape
    n = M if count is None else max(0, min(int(count), M))
    e = torch.tensor(eps, dtype=F32)
    sel = [(W[:n, k] > e).nonzero().squeeze(1).to(torch.int32) for k in range(K)]
    offs = torch.zeros(K + 1, dtype=torch.int32)
    offs[1:] = torch.cumsum(torch.tensor([s.numel() for s in sel]), 0).to(torch.int32)
    return offs, (torch.cat(sel) if sel else torch.zeros(0, dtype=torch.int32))


# ================================================================================================= gather & co.

GATHER_COLS = [1, 4, 6]
GATHER_CAP = 200000   # x 6 columns > 4096 x 256 elements: the grid-stride loop
SENT = -7.5           # sentinel of the float outputs
ISENT = -7


def rng_cases(cap):
    """(rng, rows the kernel handles, first idx entry): full, shifted, empty, reversed, clamped to the capacity."""
    return [((0, cap), cap, 0), ((7, 7 + cap), cap, 7), ((5, 5), 0, 5), ((9, 3), 0, 9), ((0, 3 * cap), cap, 0)]


def gather_reference(src, idx, n, cols, dst):
    """dst (rows, pitch) pre-filled: rows 0 .. n-1, columns 0 .. cols-1 take src[idx[i], :cols]."""
    out = dst.clone()
    out[:n, :cols] = src[idx[:n].long(), :cols]
    return out


def flags_input(n, seed=5):
    """flags with values 0, 1, 2, -1 (any non-zero counts), pos = exclusive scan of (flag != 0)."""
    f = torch.randint(-1, 3, (n,), generator=gen(seed + n)).to(torch.int32)
    nz = (f != 0).to(torch.int32)
    return f, (torch.cumsum(nz, 0) - nz).to(torch.int32)


# ================================================================================================= mix

MIX_C = [1, 4, 7]
MIX_K = [1, 3, 32]


def mix_case(M, C, K, one_hot, seed=11):
    """W (M, K): dense soft weights (every row to every expert: each launch covers M * C elements) or one-hot;
    sels per dispatch_reference; ys (n_k, C)."""
    g = gen(seed + 131 * M + 17 * C + K)
    if one_hot:
        W = torch.nn.functional.one_hot(torch.randint(0, K, (M,), generator=g), K).to(F32)
    else:
        W = torch.rand(M, K, generator=g) + 0.05
        W = (W / W.sum(1, keepdim=True)).to(F32)
    offs, idx = dispatch_reference(W, 0.0)
    sels = [idx[offs[k]:offs[k + 1]].contiguous() for k in range(K)]
    ys = [torch.randn(s.numel(), C, generator=g).to(F32) for s in sels]
    return W.contiguous(), sels, ys


def mix_reference(W, sels, ys, C):
    """fp32, out = out + y * w expert by expert (a product rounded, then a sum rounded: no fma)."""
    out = torch.zeros(W.shape[0], C, dtype=F32)
    for k, (sel, y) in enumerate(zip(sels, ys)):
        s = sel.long()
        out[s] = out[s] + y * W[s, k:k + 1]
    return out


def mix_bwd_reference(W, sel, k, dout):
    s = sel.long()
    return dout[s] * W[s, k:k + 1]


# ================================================================================================= blend

BLEND_K = [1, 4, 8]
BLEND_ROWS = [0, 1, 255, 256, 257]
BLEND_M = 300


def blend_case(K, shift, seed=23):
    """Expert k routes n_k = BLEND_ROWS[(k + shift) % 5] of BLEND_M rows (random ascending subsets, so rows are shared
    between experts and the order of the additions matters).  rgb in [0, 1), sigma in (0.05, 3), W in (0.05, 1).
    Row 0 is in every non-empty expert with sigma exactly 0 (s = 0: not live).  Row 1 is routed only by the first
    expert with n_k >= 2, with W = 1 and sigma = float32(1e-12) (s == the clamp exactly: live).
    -> dict(W, sels, ys, M, k1)."""
    g = gen(seed + 100 * K + shift)
    M = BLEND_M
    ns = [BLEND_ROWS[(k + shift) % 5] for k in range(K)]
    k1 = next((k for k in range(K) if ns[k] >= 2), None)
    W = torch.zeros(M, K, dtype=F32)
    sels, ys = [], []
    for k, n in enumerate(ns):
        forced = ([0] if n >= 1 else []) + ([1] if k == k1 else [])
        rest = (torch.randperm(M - 2, generator=g)[:n - len(forced)] + 2).sort().values
        sel = torch.cat([torch.tensor(forced, dtype=torch.int64), rest])
        y = torch.cat([torch.rand(n, 3, generator=g), torch.rand(n, 1, generator=g) * 2.95 + 0.05], 1).to(F32)
        W[sel, k] = (torch.rand(n, generator=g) * 0.95 + 0.05).to(F32)
        if n >= 1:
            y[0, 3] = 0.0
        if k == k1:
            y[1, 3] = T12
            W[1, k] = 1.0
        sels.append(sel.to(torch.int32))
        ys.append(y.contiguous())
    return dict(W=W, sels=sels, ys=ys, M=M, k1=k1, K=K)


def blend_accumulate(case):
    """fp32 restatement: ws = W * sigma; s += ws; c += ws * rgb, in expert order -> (s (M), c (M, 3))."""
    s = torch.zeros(case["M"], dtype=F32)
    c = torch.zeros(case["M"], 3, dtype=F32)
    for k, (sel, y) in enumerate(zip(case["sels"], case["ys"])):
        i = sel.long()
        ws = case["W"][i, k] * y[:, 3]
        s[i] = s[i] + ws
        c[i] = c[i] + ws[:, None] * y[:, :3]
    return s, c


def blend_finish64(s, c):
    """float64 quotient of the fp32 sums -> (M, 4) float64."""
    sn = s.double().clamp_min(T12)
    return torch.cat([c.double() / sn[:, None], sn[:, None]], 1)


def blend_finish_fp32(s, c):
    sn = torch.maximum(s, torch.tensor(T12, dtype=F32))
    return torch.cat([c / sn[:, None], sn[:, None]], 1)


def finish_ratio(rs, s, c):
    """-> (worst |rgb - rgb64| / (2^-23 |rgb64|), sigma channel exact)."""
    ref = blend_finish64(s, c)
    err = (rs[:, :3].double() - ref[:, :3]).abs()
    bound = U23 * ref[:, :3].abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
    return float(ratio.max()), same_bits(rs[:, 3], ref[:, 3].to(F32))


def BLEND_BWD_K(K):
    return 3 * K + 9


def blend_upstream(M, seed=31):
    return torch.randn(M, 4, generator=gen(seed)).to(F32)


def blend_bwd_autograd(case, g):
    """float64 autograd of rs = cat(c / s.clamp_min(t), s.clamp_min(t)) w.r.t. every expert's (rgb, sigma) rows."""
    ys = [y.double().requires_grad_(True) for y in case["ys"]]
    s = torch.zeros(case["M"], dtype=F64)
    c = torch.zeros(case["M"], 3, dtype=F64)
    for k, (sel, y) in enumerate(zip(case["sels"], ys)):
        i = sel.long()
        ws = case["W"][i, k].double() * y[:, 3]
        s = s.index_add(0, i, ws)
        c = c.index_add(0, i, ws[:, None] * y[:, :3])
    sn = s.clamp_min(T12)
    rs = torch.cat([c / sn[:, None], sn[:, None]], 1)
    (rs * g.double()).sum().backward()
    return [y.grad if y.grad is not None else torch.zeros_like(y) for y in ys]


def blend_bwd_restate(case, g, s, rs, dtype=F32, strict=False, drop_mix=False):
    """blend_bwd_kernel's arithmetic in `dtype` from the saved s (M) and rs (M, 4).  strict: live = s > t in place
    of >= ; drop_mix: gdot without the - mix term (the two mutations the bound must catch)."""
    out = []
    t = torch.tensor(T12, dtype=s.dtype)
    for k, (sel, y) in enumerate(zip(case["sels"], case["ys"])):
        i = sel.long()
        v = y.to(dtype)
        w = case["W"][i, k].to(dtype)
        live = (s[i] > t) if strict else (s[i] >= t)
        sn = torch.maximum(s[i], t).to(dtype)
        mix = torch.where(live[:, None], rs[i, :3].to(dtype), torch.zeros((), dtype=dtype))
        if drop_mix:
            mix = torch.zeros_like(mix)
        gg = g[i].to(dtype)
        dc = w * v[:, 3] / sn
        dsig = torch.where(live, gg[:, 3], torch.zeros((), dtype=dtype)) * w
        d = gg[:, :3] * (v[:, :3] - mix)
        gdot = d[:, 0] + d[:, 1] + d[:, 2]
        dsig = dsig + w * gdot / sn
        out.append(torch.cat([dc[:, None] * gg[:, :3], dsig[:, None]], 1))
    return out


def blend_bwd_bound(case, g):
    """Per expert (n_k, 4) float64: BLEND_BWD_K(K) 2^-23 sum |terms| from the float64 values."""
    s, c = blend_accumulate(case)
    rs = blend_finish64(s, c)
    t = T12
    out = []
    for k, (sel, y) in enumerate(zip(case["sels"], case["ys"])):
        i = sel.long()
        v, w, gg = y.double(), case["W"][i, k].double(), g[i].double()
        s64 = s[i].double()
        live = s64 >= t
        sn = s64.clamp_min(t)
        mix = torch.where(live[:, None], rs[i, :3], torch.zeros((), dtype=F64))
        t_rgb = (w * v[:, 3] / sn)[:, None] * gg[:, :3].abs()
        t_sig = torch.where(live, gg[:, 3].abs() * w, torch.zeros((), dtype=F64)) + \
            w / sn * (gg[:, :3].abs() * (v[:, :3].abs() + mix.abs())).sum(1)
        out.append(BLEND_BWD_K(case["K"]) * U23 * torch.cat([t_rgb, t_sig[:, None]], 1))
    return out


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; an element whose bound is 0 must be met exactly (inf otherwise); NaN counts as inf."""
    err = torch.nan_to_num((got.detach().cpu().double() - ref).abs(), nan=float("inf"), posinf=float("inf"))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
    return float(r.max()) if r.numel() else 0.0


# ================================================================================================= routing

ROUTE_K = [1, 3, 8, 32]
ROUTE_M = [1, 255, 256, 257, 4099]
ROUTE_SOFT = [1.05, 2.0]
ROUTE_HARD = [1.0, 0.9]
ROUTE_COUNTS = [0, 1, 257, 4099, 5000]


@functools.lru_cache(maxsize=None)
def route_input(K, seed=41):
    """-> (points (4099, 3) fp32 uniform in [-1.7, 1.7]^3, centroids (K, 3) fp32 uniform in the same cube)."""
    g = gen(seed + K)
    return ((torch.rand(4099, 3, generator=g) * 3.4 - 1.7).to(F32).contiguous(),
            (torch.rand(K, 3, generator=g) * 3.4 - 1.7).to(F32).contiguous())


def route_dist64(pts, cen, c2d):
    a = [1, 2] if c2d else [0, 1, 2]
    return (pts[:, None, a].double() - cen[None, :, a].double()).pow(2).sum(-1).sqrt()


def routing64(pts, cen, margin, c2d):
    """moe_oracle.routing in float64 on the fp32 inputs (the oracle casts to fp32 itself) -> (weights, mask) for
    margin > 1, else (one-hot weights, None)."""
    dist = route_dist64(pts, cen, c2d)
    if margin > 1.0:
        dist = dist.clamp_min(1e-6)
        inv = 1.0 / dist
        mask = dist <= margin * dist.min(1, keepdim=True).values
        inv = inv * mask
        return inv / inv.sum(1, keepdim=True).clamp_min(1e-6), mask
    return torch.nn.functional.one_hot(dist.argmin(1), cen.shape[0]).double(), None


def routing_fp32(pts, cen, margin, c2d):
    """route_kernel's arithmetic in fp32 torch ops."""
    d = [pts[:, None, a] - cen[None, :, a] for a in range(3)]
    s = d[1] * d[1] + d[2] * d[2]
    if not c2d:
        s = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    dist = s.sqrt()
    K = cen.shape[0]
    if margin > 1.0:
        dist = dist.clamp_min(1e-6)
        lim = torch.tensor(margin, dtype=F32) * dist.min(1, keepdim=True).values
        inv = torch.where(dist <= lim, 1.0 / dist, torch.zeros((), dtype=F32))
        den = torch.zeros(pts.shape[0], dtype=F32)
        for k in range(K):
            den = den + inv[:, k]
        return inv / den.clamp_min(1e-6)[:, None]
    return torch.nn.functional.one_hot(dist.argmin(1), K).to(F32)


def route_keep(pts, cen, margin, c2d):
    """Rows away from the discontinuities: soft, no float64 distance within 1e-5 (relative) of margin x nearest;
    hard, the two nearest distances at least 1e-6 (relative) apart."""
    dist = route_dist64(pts, cen, c2d)
    if margin > 1.0:
        dist = dist.clamp_min(1e-6)
        lim = margin * dist.min(1, keepdim=True).values
        return ~((dist - lim).abs() <= 1e-5 * lim).any(1)
    if cen.shape[0] == 1:
        return torch.ones(pts.shape[0], dtype=torch.bool)
    two = dist.topk(2, dim=1, largest=False).values
    return (two[:, 1] - two[:, 0]) >= 1e-6 * two[:, 1]


def route_ratio(got, pts, cen, margin, c2d):
    """-> (worst |w - w64| / ((K + 8) u w64) over the kept rows (hard: 0 if one-hot equal, inf otherwise), masked-out
    weights exactly 0, share of rows left out)."""
    got = got.detach().cpu()
    keep = route_keep(pts, cen, margin, c2d)
    ref, mask = routing64(pts, cen, margin, c2d)
    K = cen.shape[0]
    left = 1.0 - float(keep.double().mean()) if keep.numel() else 0.0
    if mask is None:
        ok = bool(torch.equal(got[keep].double(), ref[keep]))
        return (0.0 if ok else float("inf")), ok, left
    zero_ok = bool((got[keep][~mask[keep]] == 0).all())
    r = worst_ratio(got[keep], ref[keep], (K + 8) * U * ref[keep])
    return r, zero_ok, left


# constructed rows: centroids 0 and 1 mirror each other in y, 3 differs from 0 only in x (a tie under cluster_2d)
ROUTE_EXACT_CEN = torch.tensor([[0.5, 0.25, -0.5], [0.5, -0.25, -0.5], [-1.0, 1.0, 1.0], [-0.75, 0.25, -0.5]],
                               dtype=F32)
ROUTE_EXACT_PTS = torch.tensor([[-1.0, 1.0, 1.0],     # on centroid 2: the distance clamps to 1e-6, one-hot
                                [0.5, 0.0, -0.5],     # equidistant (0.25) from 0 and 1 (and from 3 under cluster_2d)
                                [0.125, 0.25, -0.5]],  # under cluster_2d on centroids 0 and 3 at once
                               dtype=F32)


def route_exact_expect(margin, c2d):
    """The fixed answers (fp32 rows) by the code's rules: first minimum for the hard route, equal weights for ties."""
    third = float(np.float32(4.0) / np.float32(12.0))
    if margin > 1.0:
        rows = [[0, 0, 1, 0],
                [third, third, 0, third] if c2d else [0.5, 0.5, 0, 0],
                [0.5, 0, 0, 0.5] if c2d else None]
    else:
        rows = [[0, 0, 1, 0], [1, 0, 0, 0], [1, 0, 0, 0] if c2d else None]
    return rows


# ================================================================================================= AABB prefilter

AABB_BOX = (-1.0, -0.5, -0.75, 1.25, 0.75, 0.875)
AABB_N = [1, 255, 256, 257]


@functools.lru_cache(maxsize=None)
def aabb_rays(n=257, seed=53):
    """(n, 8) fp32 rays [o, d, near, far]: origins in [-3, 3]^3, half the directions aimed at a point in [-1.5, 1.5]^3,
    half random; near in (0.05, 1), far in (2, 7)."""
    g = gen(seed)
    o = torch.rand(n, 3, generator=g) * 6 - 3
    aim = torch.rand(n, 3, generator=g) * 3 - 1.5 - o
    d = torch.where((torch.arange(n) % 2 == 0)[:, None], aim, torch.randn(n, 3, generator=g))
    d = torch.nn.functional.normalize(d, dim=-1)
    near = torch.rand(n, 1, generator=g) * 0.95 + 0.05
    far = torch.rand(n, 1, generator=g) * 5 + 2
    return torch.cat([o, d, near, far], 1).to(F32).contiguous()


def aabb_margin64(rays, box):
    """float64 restatement of _intersect_rays_aabb: min(tmax, far) - max(tmin, near); a hit iff > 0."""
    r = rays.double()
    lo, hi = torch.tensor(box[:3], dtype=F64), torch.tensor(box[3:], dtype=F64)
    d = r[:, 3:6]
    inv = torch.where(d.abs() > 1e-9, 1.0 / d, torch.full_like(d, 1e9))
    ta, tb = (lo - r[:, :3]) * inv, (hi - r[:, :3]) * inv
    tmin = torch.minimum(ta, tb).amax(-1)
    tmax = torch.maximum(ta, tb).amin(-1)
    return torch.minimum(tmax, r[:, 7]) - torch.maximum(tmin, r[:, 6])


def aabb_keep(rays, box):
    size = max(box[3] - box[0], box[4] - box[1], box[5] - box[2])
    return aabb_margin64(rays, box).abs() > 1e-5 * size


AABB_EXACT_BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
# (origin, direction, near, far, hit): every number exactly representable, the box is crossed at t in [2, 4] along +y
AABB_EXACT = [
    ((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), 0.5, 6.0, 1),      # zero components: 1e9 reciprocal, origin inside the slabs
    ((0.0, -3.0, 0.0), (-0.0, 1.0, -0.0), 0.5, 6.0, 1),    # -0.0 likewise
    ((2.0, -3.0, 0.0), (0.0, 1.0, 0.0), 0.5, 6.0, 0),      # outside the x slab, above
    ((-2.0, -3.0, 0.0), (0.0, 1.0, 0.0), 0.5, 6.0, 0),     # ... below
    ((2.0, -3.0, 0.0), (-0.0, 1.0, 0.0), 0.5, 6.0, 0),
    ((0.0, -3.0, -2.0), (0.0, 1.0, -0.0), 0.5, 6.0, 0),
    ((0.0, -3.0, 0.0), (1e-10, 1.0, 0.0), 0.5, 6.0, 1),    # |d| = 1e-10 <= 1e-9: the 1e9 reciprocal, either sign
    ((0.0, -3.0, 0.0), (-1e-10, 1.0, 0.0), 0.5, 6.0, 1),
    ((2.0, -3.0, 0.0), (1e-10, 1.0, 0.0), 0.5, 6.0, 0),
    ((2.0, -3.0, 0.0), (-1e-10, 1.0, 0.0), 0.5, 6.0, 0),
    ((-2.0, -3.0, 0.0), (-1e-10, 1.0, 0.0), 0.5, 6.0, 0),
    ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.5, 6.0, 1),       # origin inside the box: leaves at t = 1
    ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 2.0, 6.0, 0),       # ... but near is past the exit
    ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, 6.0, 0),       # ... near on the exit: strict
    ((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), 0.5, 1.5, 0),      # box wholly beyond far
    ((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), 0.5, 2.0, 0),      # far on the entry: strict
    ((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), 0.5, 2.5, 1),
    ((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), 4.5, 6.0, 0),      # box wholly before near
    ((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), 4.0, 6.0, 0),      # near on the exit: strict
    ((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), 3.5, 6.0, 1),
    ((1.0, -3.0, 0.0), (0.0, 1.0, 0.0), 0.5, 6.0, 0),      # in the face plane x = 1: the x interval ends at t = 0
    ((0.0, -3.0, 1.0), (0.0, 1.0, 0.0), 0.5, 6.0, 0),      # in the face plane z = 1
    ((-3.0, -1.0, 0.0), (1.0, 1.0, 0.0), 0.5, 6.0, 0),     # touches the edge x = -1, y = 1 at t = 2 only: strict
    ((-3.0, -1.5, 0.0), (1.0, 1.0, 0.0), 0.5, 6.0, 1),     # the same ray moved inside: t in [2, 2.5]
]


def aabb_exact_rays():
    rows = [list(o) + list(d) + [n, f] for o, d, n, f, _ in AABB_EXACT]
    return torch.tensor(rows, dtype=F32), torch.tensor([h for *_, h in AABB_EXACT], dtype=torch.int32)


# ================================================================================================= segment union

UNION_CAP = 2048
UNION_NB = [0, 2, 62, 64, 66, 126, 128, 130, 1022, 1024, 1026, 2046, 2048, 2050, 4098]
UNION_K = [1, 3, 8]
UNION_NEAR = 0.05
UNION_STEPS = (1.0 / 256.0, 0.0051)   # experts with even k march the first lattice, odd k the second


def lattice(step, n):
    """near + step * i for i = 0 .. n-1 in fp32: a product rounded, then a sum rounded."""
    return torch.tensor(step, dtype=F32) * torch.arange(n, dtype=F32) + torch.tensor(UNION_NEAR, dtype=F32)


def _chain(step, cells):
    lat = lattice(step, (max(cells) + 2) if len(cells) else 1)
    c = torch.tensor(cells, dtype=torch.int64)
    return lat[c], lat[c + 1]


def _cells(g, n, start=0):
    """n ascending cells from start on, about one in eight dropped (gaps)."""
    if n == 0:
        return []
    span = n + max(1, n // 8)
    keep = torch.randperm(span, generator=g)[:n].sort().values
    return (keep + start).tolist()


def _split(g, total, K):
    """total segments over K experts, every share random (shares of 0 included)."""
    if K == 1:
        return [total]
    cuts = torch.randint(0, total + 1, (K - 1,), generator=g).sort().values.tolist()
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


@functools.lru_cache(maxsize=None)
def union_input(K, seed=61):
    """-> dict(segs: per ray a list over the experts of (t0, t1) fp32 chains, tags: ray -> what it is for,
    pair: (ray <= UNION_CAP entries, ray > UNION_CAP entries) with the same distinct boundaries, or None for K = 1).
    Ray r < len(UNION_NB) totals UNION_NB[r] boundary entries; the 2050 ray is the 2048 ray plus one segment."""
    g = gen(seed + K)
    rays, tags = [], {}

    def random_ray(nb):
        shares = _split(g, nb // 2, K)
        starts = torch.randint(0, 40, (K,), generator=g).tolist()
        return [_chain(UNION_STEPS[k % 2], _cells(g, shares[k], starts[k])) for k in range(K)]

    for nb in UNION_NB:
        if nb == 2050:
            base = [(a.clone(), b.clone()) for a, b in rays[tags["nb2048"]]]
            k = max(range(K), key=lambda j: base[j][0].numel())
            a, b = _chain(UNION_STEPS[k % 2], [4000])   # past every cell of the 2048 ray (< 40 + 1024 * 9 / 8 + 1)
            base[k] = (torch.cat([base[k][0], a]), torch.cat([base[k][1], b]))
            rays.append(base)
        else:
            rays.append(random_ray(nb))
        tags[f"nb{nb}"] = len(rays) - 1
    empty = (torch.zeros(0, dtype=F32), torch.zeros(0, dtype=F32))
    # one segment with t0 == t1: one distinct boundary, no segment
    z = lattice(UNION_STEPS[0], 8)[5:6]
    rays.append([(z.clone(), z.clone())] + [empty] * (K - 1))
    tags["degenerate"] = len(rays) - 1
    # present in one expert only (the last)
    rays.append([empty] * (K - 1) + [_chain(UNION_STEPS[(K - 1) % 2], _cells(g, 70, 3))])
    tags["single"] = len(rays) - 1
    # every expert identical: short (LDS path for every K) and long (K * 2 * 300 entries: past the cap for K = 8)
    for name, n in (("same_short", 20), ("same_long", 300)):
        ch = _chain(UNION_STEPS[0], _cells(g, n, 1))
        rays.append([(ch[0].clone(), ch[1].clone()) for _ in range(K)])
        tags[name] = len(rays) - 1
    # the same distinct boundaries below and above the cap: one expert holds the chain / two experts hold it twice over
    pair = None
    if K >= 3:
        ch = _chain(UNION_STEPS[0], _cells(g, 600, 2))      # 1200 entries
        other = _chain(UNION_STEPS[1], _cells(g, 100, 0))   # 200 entries, another lattice
        lo = [empty] * K
        hi = [empty] * K
        lo[0], lo[1] = ch, other
        hi[0], hi[1], hi[K - 1] = ch, other, ch             # 1200 + 200 + 1200 = 2600 entries
        rays += [lo, hi]
        pair = (len(rays) - 2, len(rays) - 1)
    # interleaving lattices at sizes off the powers of two, to fill up to about 40 rays
    for nb in (6, 34, 190, 514, 700, 1500, 2052, 2600, 3000, 100, 258, 10, 12, 1100, 2044, 2056, 18, 4, 900):
        rays.append(random_ray(nb))
    return dict(segs=rays, tags=tags, pair=pair, K=K)


def union_nb(ray):
    return sum(2 * a.numel() for a, _ in ray)


def union_reference(segs):
    """Per ray torch.unique (sorted) of all t0 and t1, consecutive pairs -> (counts (N) int32, ri, t0, t1)."""
    counts, ri, t0, t1 = [], [], [], []
    for r, ray in enumerate(segs):
        b = torch.unique(torch.cat([torch.cat([a, c]) for a, c in ray]), sorted=True)
        n = max(b.numel() - 1, 0)
        counts.append(n)
        ri.append(torch.full((n,), r, dtype=torch.int32))
        t0.append(b[:n])
        t1.append(b[1:n + 1])
    return torch.tensor(counts, dtype=torch.int32), torch.cat(ri), torch.cat(t0), torch.cat(t1)


def union_merge_seq(ray, unique=True):
    """Python restatement of merge_seq (the sequential fallback): K-way merge of the 2K sorted lists, strict < so
    the first list wins a tie, exact-equality unique (unique=False: the mutation that keeps repeated boundaries)
    -> (t0 list, t1 list)."""
    lists = []
    for a, b in ray:
        lists += [a.tolist(), b.tolist()]
    pos = [0] * len(lists)
    prev, have, o0, o1 = 0.0, False, [], []
    while True:
        best, bi = float("inf"), -1
        for i, l in enumerate(lists):
            if pos[i] < len(l) and l[pos[i]] < best:
                best, bi = l[pos[i]], i
        if bi < 0:
            break
        pos[bi] += 1
        if unique and have and best == prev:
            continue
        if have:
            o0.append(prev)
            o1.append(best)
        prev, have = best, True
    return o0, o1


def union_pack(segs, K):
    """-> per expert (t0 (n_k), t1 (n_k), offsets (N+1) int32)."""
    out = []
    for k in range(K):
        n = [ray[k][0].numel() for ray in segs]
        offs = torch.zeros(len(segs) + 1, dtype=torch.int32)
        offs[1:] = torch.cumsum(torch.tensor(n), 0).to(torch.int32)
        out.append((torch.cat([ray[k][0] for ray in segs]), torch.cat([ray[k][1] for ray in segs]), offs))
    return out


# ================================================================================================= background MLP

BG_H = [1, 32, 64]
BG_N = [1, 63, 64, 65, 255, 256, 257, 321]
BG_RAYS = 64
C_D = 11
R_SH = torch.tensor([1.0] + [13.0] * 3 + [25.0, 25.0, 27.0, 25.0, 26.0] + [39.0] * 7, dtype=torch.float64)
N_ADD = torch.tensor([18.0 - max(i, 1) for i in range(16)], dtype=torch.float64)
BG_SPARE = 400    # directions drawn before the discards


def bg_weights(H, seed=71):
    """Packed W1 (H, 16) | b1 (H) | W2 (3, H) | b2 (3), fp32."""
    g = gen(seed + H)
    W1 = (torch.rand(H, 16, generator=g) * 2 - 1) * 0.5
    b1 = (torch.rand(H, generator=g) * 2 - 1) * 0.3
    W2 = (torch.rand(3, H, generator=g) * 2 - 1) * (1.5 / H ** 0.5)
    b2 = (torch.rand(3, generator=g) * 2 - 1) * 0.3
    return torch.cat([W1.reshape(-1), b1, W2.reshape(-1), b2]).to(F32).contiguous()


def bg_unpack(w, H):
    return w[:16 * H].view(H, 16), w[16 * H:17 * H], w[17 * H:20 * H].view(3, H), w[20 * H:20 * H + 3]


def _unit64(d):
    d = torch.nn.functional.normalize(d, dim=-1)                # eps 1e-12
    return d / d.norm(dim=-1, keepdim=True).clamp_min(1e-9)     # SHEncoder.forward's own


def sh16(d, absolute=False):
    """The 16 SH terms of unit directions in d's dtype (oracle sh_components, degree 3); absolute: every monomial
    by its absolute value (A_i of the bounds)."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    if absolute:
        x, y, z = x.abs(), y.abs(), z.abs()
    sg = 1.0 if absolute else -1.0
    xx, yy, zz = x * x, y * y, z * z
    one = torch.ones_like(x)
    return torch.stack([
        0.28209479177387814 * one, 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
        1.0925484305920792 * x * y, 1.0925484305920792 * y * z, 0.9461746957575601 * zz + sg * 0.31539156525251999,
        1.0925484305920792 * x * z, 0.5462742152960396 * (xx + sg * yy),
        0.5900435899266435 * y * (3 * xx + sg * yy), 2.890611442640554 * x * y * z,
        0.4570457994644658 * y * (5 * zz + sg * 1), 0.3731763325901154 * z * (5 * zz + sg * 3),
        0.4570457994644658 * x * (5 * zz + sg * 1), 1.445305721320277 * z * (xx + sg * yy),
        0.5900435899266435 * x * (xx + sg * 3 * yy)], -1)


def bg_forward64(d, w, H):
    """float64 forward with every intermediate the bounds need."""
    W1, b1, W2, b2 = [t.double() for t in bg_unpack(w, H)]
    dn = _unit64(d.double())
    e, A = sh16(dn), sh16(dn, absolute=True)
    pre = e @ W1.t() + b1
    h = torch.relu(pre)
    o = h @ W2.t() + b2
    Bh = U * ((A * (R_SH + N_ADD)) @ W1.abs().t() + 2 * b1.abs())
    Bo = (Bh + (H + 2) * U * h) @ W2.abs().t() + 2 * U * b2.abs()
    return dict(e=e, A=A, pre=pre, h=h, o=o, out=torch.sigmoid(o), Bh=Bh, Bo=Bo)


def bg_fwd_bound(d, w, H):
    """-> (out64 (N, 3), bound (N, 3)): Bo / 4 + 4u."""
    f = bg_forward64(d, w, H)
    return f["out"], f["Bo"] / 4 + 4 * U


def bg_forward_fp32(d, w, H):
    """bg_fwd_kernel's arithmetic in fp32 torch ops (the dot products in the kernel's order)."""
    W1, b1, W2, b2 = bg_unpack(w, H)
    x = d.to(F32)
    for clamp in (1e-12, 1e-9):
        n = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]).sqrt().clamp_min(clamp)
        x = x / n[:, None]
    e = sh16(x)
    s = torch.zeros(d.shape[0], H, dtype=F32)
    for i in range(16):
        s = s + W1[:, i][None, :] * e[:, i:i + 1]
    h = torch.relu(s + b1)
    o = torch.zeros(d.shape[0], 3, dtype=F32)
    for j in range(H):
        o = o + W2[:, j][None, :] * h[:, j:j + 1]
    o = o + b2
    return 1.0 / (1.0 + torch.exp(-o)), h


def bg_backward_fp32(d, w, H, gout):
    out, h = bg_forward_fp32(d, w, H)
    W1, b1, W2, b2 = bg_unpack(w, H)
    x = d.to(F32)
    for clamp in (1e-12, 1e-9):
        x = x / (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]).sqrt().clamp_min(clamp)[:, None]
    e = sh16(x)
    dz = gout * (out * (1.0 - out))
    dh = torch.where(h > 0, dz @ W2, torch.zeros((), dtype=F32))
    return torch.cat([(dh.t() @ e).reshape(-1), dh.sum(0), (dz.t() @ h).reshape(-1), dz.sum(0)])


def bg_upstream(N, seed=83):
    return torch.randn(max(N, 1), 3, generator=gen(seed)).to(F32)[:N].contiguous()


def bg_bwd_bound(d, w, H, gout):
    """-> (d_w64 (20 H + 3) by float64 autograd, bound (20 H + 3)); see the module docstring."""
    N = d.shape[0]
    w64 = w.double().requires_grad_(True)
    W1, b1, W2, b2 = bg_unpack(w64, H)
    dn = _unit64(d.double())
    out = torch.sigmoid(torch.relu(sh16(dn) @ W1.t() + b1) @ W2.t() + b2)
    (out * gout.double()).sum().backward()
    ref = w64.grad.clone()
    f = bg_forward64(d, w, H)
    W2a = bg_unpack(w, H)[2].double().abs()
    g, sg, h, A = gout.double().abs(), f["out"], f["h"], f["A"]
    dz = g * sg * (1 - sg)
    dsg = f["Bo"] / 4 + 4 * U
    ddz = g * ((1 - 2 * sg).abs() * dsg + 3 * U * sg * (1 - sg))
    mask = (f["pre"] > 0).double()
    dh = mask * ((gout.double() * sg * (1 - sg)) @ bg_unpack(w, H)[2].double()).abs()
    ddh = mask * ((ddz + 3 * U * dz) @ W2a)
    n = 66 + -(-N // BG_RAYS)
    bW1 = ddh.t() @ A + U * (dh.t() @ (A * (R_SH + n)))
    bb1 = ddh.sum(0) + n * U * dh.sum(0)
    bW2 = ddz.t() @ h + dz.t() @ f["Bh"] + n * U * (dz.t() @ h)
    bb2 = ddz.sum(0) + n * U * dz.sum(0)
    return ref, 2 * torch.cat([bW1.reshape(-1), bb1, bW2.reshape(-1), bb2])


@functools.lru_cache(maxsize=None)
def bg_directions(H, seed=89):
    """-> (directions (n, 3) fp32 with n >= max(BG_N), share discarded).  Drawn: unit vectors, vectors with norms
    log-uniform in [1e-6, 1e3], the zero vector at row 5 (never a norm between 0 and 1e-6); discarded: those with a
    hidden unit whose float64 pre-activation lies within 64 Bh of 0 (an ambiguous ReLU mask in the backward)."""
    g = gen(seed + H)
    u = torch.nn.functional.normalize(torch.randn(BG_SPARE, 3, generator=g), dim=-1)
    scale = 10.0 ** (torch.rand(BG_SPARE, 1, generator=g) * 9 - 6)
    d = torch.where((torch.arange(BG_SPARE) % 3 == 0)[:, None], u, u * scale).to(F32)
    d[5] = 0.0
    f = bg_forward64(d, bg_weights(H), H)
    ok = ~(f["pre"].abs() <= 64 * f["Bh"]).any(1)
    return d[ok].contiguous(), 1.0 - float(ok.double().mean())
