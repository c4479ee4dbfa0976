"""CPU checks of tests/moe_reference.py: the references are right (against the oracle, autograd and independent
restatements), the inputs reach the edges tests/test_gpu_moe_edges.py is meant for, each bounded reference evaluated
in fp32 on the CPU stays within its own bound, and the bounds catch the mutations they are there for."""
import pytest
import torch

import moe_reference as R
from golden_io import load
from oracle import moe_oracle as MO


# ------------------------------------------------------------------------------------------------ dispatch

@pytest.mark.parametrize("tag", ["soft", "hard"])
def test_dispatch_reference_is_the_oracles_selection(tag):
    """container_forward selects (w[:, k] > 0).nonzero() per expert: the reference with eps = 0 on the golden
    routing weights, and container_forward mixes exactly the rows the reference lists."""
    z = load("moe")
    W = z[f"{tag}_route"]
    offs, idx = R.dispatch_reference(W, 0.0)
    seen = []
    experts = [lambda x, k=k: (seen.append((k, x[:, 0].clone())), x[:, :4])[1] for k in range(W.shape[1])]
    margin, c2d = (1.05, True) if tag == "soft" else (1.0, False)   # the golden cases of tests/test_gpu_moe.py
    MO.container_forward(experts, z["x_d"], z["centroids"], margin, c2d)
    assert len(seen) > 0
    for k, x0 in seen:
        sel = idx[offs[k]:offs[k + 1]].long()
        assert torch.equal(z["x_d"][sel, 0], x0), k
        assert torch.equal(sel, (W[:, k] > 0).nonzero().squeeze(1))
    assert int(offs[-1]) == sum(x0.numel() for _, x0 in seen)


def test_dispatch_inputs_reach_their_edges():
    import numpy as np
    none_rows = all_rows = empty_experts = blocks = 0
    for eps in R.DISPATCH_EPS:
        e = float(np.float32(eps))
        for M in R.DISPATCH_M:
            for K in R.DISPATCH_K:
                W = R.dispatch_weights(M, K, eps)
                assert W.shape == (M, K) and W.dtype == torch.float32
                assert int((W == e).sum()) >= 1, (M, K, eps)           # equal to eps: excluded by the strict test
                offs, idx = R.dispatch_reference(W, eps)
                routed = (W > e)
                assert int(offs[-1]) == int(routed.sum())
                if M >= 63 and (K > 1 or M < 256 or M >= 512):   # K = 1: expert 0 owns all of M = 256, 257 but one row
                    assert bool((W < 0).any()) and bool(routed.any())
                none_rows += int((~routed.any(1)).sum() > 0)
                all_rows += int(routed.all(1).sum() > 0 and K > 1)
                empty_experts += int(K > 1 and (offs[1:] == offs[:-1]).any())
                b = R.owned_block(M)
                if M >= 512 and K > 1:
                    blk = routed[256 * b:256 * (b + 1)]
                    assert bool(blk[:, 0].all()) and bool((~blk).all(0).any()), (M, K, eps)
                    blocks += 1
                nr, ar = R.dispatch_special_rows(M, eps)
                if nr is not None and nr != M - 1:
                    assert not bool(routed[nr].any())
                if ar is not None and ar != M - 1:
                    assert bool(routed[ar].all())
    assert none_rows >= 40 and all_rows >= 10 and empty_experts >= 20 and blocks >= 12
    cap = R.DISPATCH_CAP
    assert -(-cap // 256) == 258 and -(-258 // 256) == 2          # chunk = 2: threads 129 .. 255 have empty runs
    assert 129 * 2 >= 258 and 130 * 2 > 258                        # b0 > nblk for the trailing threads


def test_dispatch_reference_counts():
    W = R.dispatch_weights(300, 3, 1e-8)
    full = R.dispatch_reference(W, 1e-8)
    assert all(torch.equal(a, b) for a, b in zip(full, R.dispatch_reference(W, 1e-8, count=1300)))
    offs, idx = R.dispatch_reference(W, 1e-8, count=0)
    assert int(offs.abs().sum()) == 0 and idx.numel() == 0
    offs, idx = R.dispatch_reference(W, 1e-8, count=257)
    assert int(idx.max()) < 257


# ------------------------------------------------------------------------------------------------ exact operations

def test_block_edge_rows():
    assert R.rows_at_block_edge(1) == [255, 256, 257]
    for cols in (4, 6, 7):
        ns = R.rows_at_block_edge(cols)
        assert min(ns) * cols <= 255 and max(ns) * cols >= 257, cols
    assert R.GATHER_CAP * 6 > 4096 * 256


def test_mix_reference_matches_index_add():
    """The oracle's out.index_add(0, sel, yk * w[sel, k]) in expert order gives the reference's bits."""
    for one_hot in (False, True):
        W, sels, ys = R.mix_case(64, 4, 3, one_hot)
        out = torch.zeros(64, 4)
        for k, (sel, y) in enumerate(zip(sels, ys)):
            out = out.index_add(0, sel.long(), y * W.index_select(0, sel.long())[:, k:k + 1])
        assert R.same_bits(out, R.mix_reference(W, sels, ys, 4))
    W, sels, ys = R.mix_case(64, 4, 3, False)
    assert all(s.numel() == 64 for s in sels)                     # dense: every launch covers M * C elements


def test_blend_inputs_reach_their_edges():
    seen = set()
    for K in R.BLEND_K:
        for shift in range(5):
            case = R.blend_case(K, shift)
            seen |= {s.numel() for s in case["sels"]}
            s, c = R.blend_accumulate(case)
            for sel in case["sels"]:
                assert sel.numel() == sel.unique().numel()       # one launch never meets a row twice
            if any(sel.numel() for sel in case["sels"]):
                assert float(s[0]) == 0.0                        # every sigma 0: not live
            if case["k1"] is not None:
                assert R.same_bits(s[1:2], torch.tensor([R.T12]))   # s == the clamp exactly: live
            assert bool((s[2:] > 1e-3).sum() > 0) or K == 1
    assert seen == set(R.BLEND_ROWS)


# ------------------------------------------------------------------------------------------------ union

@pytest.mark.parametrize("K", R.UNION_K)
def test_union_inputs_and_merge_restatement(K):
    inp = R.union_input(K)
    segs, tags = inp["segs"], inp["tags"]
    assert 35 <= len(segs) <= 45
    nbs = [R.union_nb(ray) for ray in segs]
    assert nbs[:len(R.UNION_NB)] == R.UNION_NB and all(nb % 2 == 0 for nb in nbs)
    assert max(nbs) > R.UNION_CAP and sum(nb > R.UNION_CAP for nb in nbs) >= 3
    counts, ri, t0, t1 = R.union_reference(segs)
    pos = 0
    for r, ray in enumerate(segs):
        assert len(ray) == K
        for a, b in ray:                                         # chains: sorted lists, t1[i] bit-identical to t0[i+1]
            assert bool((a[1:] > a[:-1]).all()) and bool((b[1:] > b[:-1]).all())
            if r != tags["degenerate"]:
                assert bool((b > a).all())
                joined = b[:-1] == a[1:]
                assert a.numel() < 8 or bool(joined.any())       # chains ...
                assert a.numel() < 64 or not bool(joined.all())  # ... with gaps
        o0, o1 = R.union_merge_seq(ray)
        n = int(counts[r])
        assert len(o0) == n
        assert torch.equal(torch.tensor(o0, dtype=torch.float32), t0[pos:pos + n])
        assert torch.equal(torch.tensor(o1, dtype=torch.float32), t1[pos:pos + n])
        if nbs[r] > R.UNION_CAP:                                 # teeth: the long rays do repeat boundaries
            assert len(R.union_merge_seq(ray, unique=False)[0]) > n
        pos += n
    assert int(counts[tags["degenerate"]]) == 0 and int(counts[tags["nb0"]]) == 0 and int(counts[tags["nb2"]]) == 1
    assert sum(a.numel() > 0 for a, _ in segs[tags["single"]]) == 1
    for name in ("same_short", "same_long"):
        ray = segs[tags[name]]
        assert all(torch.equal(ray[0][0], a) and torch.equal(ray[0][1], b) for a, b in ray)
        assert int(counts[tags[name]]) < R.union_nb(ray) // 2 or K == 1
    # the 2050 ray is the 2048 ray plus one segment
    a48, a50 = segs[tags["nb2048"]], segs[tags["nb2050"]]
    extra = sum(y[0].numel() - x[0].numel() for x, y in zip(a48, a50))
    assert extra == 1 and all(torch.equal(x[0], y[0][:x[0].numel()]) for x, y in zip(a48, a50))
    if K >= 3:
        lo, hi = inp["pair"]
        assert nbs[lo] <= R.UNION_CAP < nbs[hi]
        ulo = torch.unique(torch.cat([torch.cat(p) for p in segs[lo]]))
        uhi = torch.unique(torch.cat([torch.cat(p) for p in segs[hi]]))
        assert torch.equal(ulo, uhi) and int(counts[lo]) == int(counts[hi]) > 600
        # experts on different lattices interleave, experts on the same lattice share boundaries exactly
        big = segs[tags["nb4098"]]
        assert int(counts[tags["nb4098"]]) < 4098 // 2 * 2 - 1
        e0, e1, e2 = [torch.cat(p) for p in big[:3]]
        assert e0.numel() and e1.numel() and e2.numel()
        assert bool(torch.isin(e0, e2).any()) and bool(((e1 > e0.min()) & (e1 < e0.max()) & ~torch.isin(e1, e0)).any())


# ------------------------------------------------------------------------------------------------ routing

def test_routing64_is_the_oracle_in_float64():
    for K in R.ROUTE_K:
        pts, cen = R.route_input(K)
        for c2d in (False, True):
            for margin in R.ROUTE_SOFT + R.ROUTE_HARD:
                ref, mask = R.routing64(pts, cen, margin, c2d)
                w, hard = MO.routing(pts, cen, margin, c2d)
                keep = R.route_keep(pts, cen, margin, c2d)
                if w is None:
                    assert torch.equal(ref[keep].argmax(1), hard[keep])
                else:
                    assert torch.equal(mask[keep], w[keep] > 0)
                    assert float((w[keep].double() - ref[keep]).abs().max()) <= 1e-6


def test_routing_fp32_within_bound_and_few_rows_left_out():
    worst = 0.0
    for K in R.ROUTE_K:
        pts, cen = R.route_input(K)
        for c2d in (False, True):
            for margin in R.ROUTE_SOFT + R.ROUTE_HARD:
                for M in R.ROUTE_M:
                    got = R.routing_fp32(pts[:M], cen, margin, c2d)
                    ratio, zero_ok, left = R.route_ratio(got, pts[:M], cen, margin, c2d)
                    assert ratio <= 1.0 and zero_ok, (K, c2d, margin, M, ratio)
                    assert left <= 0.005 or M < 4099, (K, c2d, margin, M, left)
                    if M == 4099:
                        assert left <= 0.005
                    if margin > 1.0:
                        worst = max(worst, ratio * (K + 8))
    print(f"fp32 routing on the CPU: worst |w - w64| / w64 = {worst:.3f} x 2^-24")


def test_routing_bound_has_teeth():
    """A dropped expert (the last term missing from the denominator) and a single-precision slip of one ulp in one
    distance are both outside the bound."""
    K = 8
    pts, cen = R.route_input(K)
    ref, mask = R.routing64(pts, cen, 2.0, False)
    inv = torch.where(mask, 1.0 / R.route_dist64(pts, cen, False).clamp_min(1e-6), torch.zeros((), dtype=torch.float64))
    dropped = (inv / inv[:, :-1].sum(1, keepdim=True)).float()
    assert R.route_ratio(dropped, pts, cen, 2.0, False)[0] > 1e3
    rows = mask.sum(1) >= 2
    bumped = ref.float().clone()
    bumped[rows] = bumped[rows] * (1 + 4 * (K + 8) * 2.0 ** -24)
    assert R.route_ratio(bumped, pts, cen, 2.0, False)[0] > 1.0


def test_route_exact_rows():
    for c2d in (False, True):
        for margin in R.ROUTE_SOFT + R.ROUTE_HARD:
            got = R.routing_fp32(R.ROUTE_EXACT_PTS, R.ROUTE_EXACT_CEN, margin, c2d)
            ref, _ = R.routing64(R.ROUTE_EXACT_PTS, R.ROUTE_EXACT_CEN, margin, c2d)
            for r, row in enumerate(R.route_exact_expect(margin, c2d)):
                if row is not None:
                    assert R.same_bits(got[r], torch.tensor(row, dtype=torch.float32)), (c2d, margin, r)
                    assert float((ref[r] - torch.tensor(row, dtype=torch.float64)).abs().max()) <= 1e-7


# ------------------------------------------------------------------------------------------------ prefilter

def test_aabb_inputs():
    rays = R.aabb_rays()
    keep = R.aabb_keep(rays, R.AABB_BOX)
    for n in R.AABB_N:
        assert 1.0 - float(keep[:n].double().mean()) <= 0.01
    hit = R.aabb_margin64(rays, R.AABB_BOX) > 0
    assert 0.1 <= float(hit.double().mean()) <= 0.9                # both answers well represented
    ex, expect = R.aabb_exact_rays()
    assert torch.equal(ex.double().float(), ex)
    assert torch.equal((R.aabb_margin64(ex, R.AABB_EXACT_BOX) > 0).to(torch.int32), expect)
    d = ex[:, 3:6]
    assert bool((d == 0).any()) and bool(torch.signbit(d[d == 0]).any())
    assert bool(((d.abs() > 0) & (d.abs() < 1e-9)).any())


# ------------------------------------------------------------------------------------------------ blend

def _blend_all():
    return [R.blend_case(K, shift) for K in R.BLEND_K for shift in range(5)]


def test_blend_finish_fp32_within_bound():
    for case in _blend_all():
        s, c = R.blend_accumulate(case)
        ratio, sigma_exact = R.finish_ratio(R.blend_finish_fp32(s, c), s, c)
        assert ratio <= 1.0 and sigma_exact


def test_blend_bwd_restatement_autograd_and_teeth():
    worst = big = 0.0
    caught_strict = caught_mix = 0
    for case in _blend_all():
        g = R.blend_upstream(case["M"])
        ref = R.blend_bwd_autograd(case, g)
        bound = R.blend_bwd_bound(case, g)
        s, c = R.blend_accumulate(case)
        # the kernel's formula in float64 from the float64 sums is the autograd gradient
        s64 = torch.zeros(case["M"], dtype=torch.float64)
        c64 = torch.zeros(case["M"], 3, dtype=torch.float64)
        for k, (sel, y) in enumerate(zip(case["sels"], case["ys"])):
            ws = case["W"][sel.long(), k].double() * y[:, 3].double()
            s64.index_add_(0, sel.long(), ws)
            c64.index_add_(0, sel.long(), ws[:, None] * y[:, :3].double())
        rs64 = torch.cat([c64 / s64.clamp_min(R.T12)[:, None], s64.clamp_min(R.T12)[:, None]], 1)
        exact = R.blend_bwd_restate(case, g, s64, rs64, dtype=torch.float64)
        for a, b, bd in zip(exact, ref, bound):                  # (float64 roundings: 2^-29 of fp32's)
            assert bool(torch.isfinite(b).all())
            assert R.worst_ratio(a, b, bd) <= 1e-6
        rs = R.blend_finish_fp32(s, c)
        got = R.blend_bwd_restate(case, g, s, rs)
        strict = R.blend_bwd_restate(case, g, s, rs, strict=True)
        nomix = R.blend_bwd_restate(case, g, s, rs, drop_mix=True)
        for k in range(case["K"]):
            assert bool(torch.isfinite(got[k]).all())
            worst = max(worst, R.worst_ratio(got[k], ref[k], bound[k]))
        if case["k1"] is not None:
            caught_strict += max(R.worst_ratio(a, b, c_) for a, b, c_ in zip(strict, ref, bound)) > 1.0
        if any(sel.numel() > 1 for sel in case["sels"]):
            caught_mix += max(R.worst_ratio(a, b, c_) for a, b, c_ in zip(nomix, ref, bound)) > 1.0
        if any(sel.numel() for sel in case["sels"]):   # the s = 0 row: gradients of order 1e12 (times g . rgb)
            k0 = next(k for k, sel in enumerate(case["sels"]) if sel.numel())
            big = max(big, float(ref[k0][0, 3].abs()))
    print(f"fp32 blend backward on the CPU: worst error / bound = {worst:.4f}")
    assert worst <= 1.0 and big > 1e10
    n_k1 = sum(case["k1"] is not None for case in _blend_all())
    assert caught_strict == n_k1 > 0 and caught_mix >= n_k1


# ------------------------------------------------------------------------------------------------ background MLP

@pytest.mark.parametrize("H", R.BG_H)
def test_bg_references_and_bounds(H):
    d, discarded = R.bg_directions(H)
    assert discarded <= 0.05 and d.shape[0] >= max(R.BG_N)
    zero = (d == 0).all(1).nonzero()
    assert zero.numel() == 1 and int(zero) < 63
    norms = d.norm(dim=1)
    assert float(norms[norms > 0].min()) >= 0.9e-6 and float(norms.max()) <= 1.1e3
    assert float(norms[norms > 0].min()) < 1e-4 and float(norms.max()) > 10
    w = R.bg_weights(H)
    W1, b1, W2, b2 = R.bg_unpack(w, H)
    ref, bound = R.bg_fwd_bound(d, w, H)
    # the float64 forward is the oracle's background_color
    oracle64 = MO.background_color(d.double(), W1.double(), b1.double(), W2.double(), b2.double())
    assert float((ref - oracle64).abs().max()) < 1e-14
    assert float((ref.float() - MO.background_color(d, W1, b1, W2, b2)).abs().max()) < 1e-5
    got, _ = R.bg_forward_fp32(d, w, H)
    r = R.worst_ratio(got, ref, bound)
    print(f"fp32 background forward on the CPU, H = {H}: worst error / bound = {r:.4f}, "
          f"largest bound {float(bound.max()):.2e}")
    assert r <= 1.0 and float(bound.max()) < 2e-4
    # teeth: a single normalisation pass is the same function, a dropped SH term or hidden unit is not
    e_drop = w.clone()
    e_drop[15] = 0.0                                              # W1[0, 15]
    assert R.worst_ratio(R.bg_forward_fp32(d, e_drop, H)[0], ref, bound) > 1.0
    worst_b = 0.0
    for N in R.BG_N:
        g = R.bg_upstream(N)
        dref, dbound = R.bg_bwd_bound(d[:N], w, H, g)
        dgot = R.bg_backward_fp32(d[:N], w, H, g)
        r = R.worst_ratio(dgot, dref, dbound)
        assert r <= 1.0, (H, N, r)
        worst_b = max(worst_b, r)
        # teeth: the gradient without the ReLU mask, and with one ray's contribution missing
        if N >= 63:
            few = R.bg_backward_fp32(d[:N - 1], w, H, g[:N - 1])
            assert R.worst_ratio(few, dref, dbound) > 1.0
    print(f"fp32 background d_w on the CPU, H = {H}: worst error / bound = {worst_b:.4f}")
