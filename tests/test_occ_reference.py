"""CPU checks of tests/occ_reference.py: the references are right (against oracle/occ_oracle.py, float64 autograd
and fp32 restatements), the shipped inputs meet the conditions the reference's docstring states (the dyadic family
is exact in fp32, the left-out shares are small, the edges are reached) and the bounds and equalities catch the
faults they are there for."""
import numpy as np
import pytest
import torch

import occ_reference as R
from oracle import occ_oracle as OO


# ------------------------------------------------------------------------------------------------ RNG, cell draws

def test_rng_restatement_properties():
    u = R.uniforms(7, 0x0CC, 4096)
    assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert ((u.astype(np.float64) * 2 ** 24) % 1 == 0).all()            # 24 bits
    assert abs(float(u.mean()) - 0.5) < 0.02 and len(np.unique(u)) > 4000
    assert R.mix64(0) == 0 and R.mix64(1) == 0x5692161D100B05E5         # splitmix64's finaliser on 1
    assert R.uniform(1, 2, 3) != R.uniform(1, 3, 2) != R.uniform(2, 2, 3)


def test_draw_below_keeps_the_fp32_path_up_to_2_24_and_reaches_every_cell_above():
    for rng in (1, 7, 16 ** 3, 64 ** 3, (1 << 24) - 1, 1 << 24):
        for b in range(200):
            assert R.draw_below(5, 0x51, b, rng) == R.draw_below_24bit_only(5, 0x51, b, rng) < rng
    cpl = 1 << 27
    new = np.array([R.draw_below(5, 0x51, b, cpl) for b in range(4096)])
    old = np.array([R.draw_below_24bit_only(5, 0x51, b, cpl) for b in range(4096)])
    assert new.min() >= 0 and new.max() < cpl
    assert sorted(set(new % 8)) == list(range(8))
    assert set(old % 8) == {0}                      # the fault the large-grid GPU test is there for: 1 residue of 8
    # just above 2^24 and far from a power of two the wide draw stays in range and spreads
    for rng in ((1 << 24) + 1, 3 * (1 << 25) + 5):
        d = np.array([R.draw_below(9, 0xA3, b, rng) for b in range(2000)])
        assert d.min() >= 0 and d.max() < rng and d.max() > 0.9 * rng and d.min() < 0.1 * rng


def test_sample_cells_reference_halves():
    cpl, n = 16 ** 3, 100
    for n_occ in (n - 1, n, n + 1, 3 * n):
        flags = R.sample_cells_input(cpl, n_occ, n_occ)
        occ_list = np.flatnonzero(flags).astype(np.int32)
        out = R.sample_cells_reference(occ_list, [0, n_occ], cpl, n, 11)
        uni, occ = out[:n], out[n:]
        assert uni.min() >= 0 and uni.max() < cpl
        if n_occ <= n:
            assert (occ[:n_occ] == occ_list).all() and (occ[n_occ:] == -1).all()
        else:
            assert np.isin(occ, occ_list).all() and len(np.unique(occ)) > n // 2


# ------------------------------------------------------------------------------------------------ dyadic march

def _trace_march(monkeypatch, fn):
    """Runs fn() recording, for every cell lookup, whether s was a power of two and whether the point lay on a face."""
    seen = dict(s=set(), face=0, calls=0)
    orig = R.cell_of

    def spy(F, G, p):
        s = max(abs(p[a] - G["c"][a]) / G["h"][a] for a in range(3))
        if s in (1.0, 2.0, 4.0):
            seen["s"].add(float(s))
        out = orig(F, G, p)
        if out is not None:
            _, _, cmin, csz = out
            seen["face"] += any((p[a] - cmin[a]) / csz[a] in (0.0, 1.0) for a in range(3))
        seen["calls"] += 1
        return out

    monkeypatch.setattr(R, "cell_of", spy)
    res = fn()
    monkeypatch.setattr(R, "cell_of", orig)
    return res, seen


@pytest.mark.parametrize("i", range(len(R.MARCH_CASES)))
def test_dyadic_family_is_exact_in_fp32(i, monkeypatch):
    """The float32 run (ceil(log2f(s)) included) and the float run give the same samples on every ray, every t is a
    float32, and the case reaches the edges it is there for."""
    case = R.march_case(i)
    (c64, ri64, a64, b64), seen = _trace_march(monkeypatch, lambda: R.march(case))
    c32, ri32, a32, b32 = R.march(case, F=np.float32)
    assert (c64 == c32).all() and (ri64 == ri32).all() and (a64 == a32).all() and (b64 == b32).all()
    assert (a64.astype(np.float32) == a64).all() and (b64.astype(np.float32) == b64).all()
    assert (c64 == R.march_expected(i)[0]).all()
    name, kind, N, with_u, max_steps = R.MARCH_CASES[i]
    if kind == "empty":
        assert c64.sum() == 0
    if N >= 127:
        if kind != "empty":
            share = float((c64 == 0).mean())
            print(f"march case {i} {name}/{kind}: empty rays {share:.3f}")
            assert share <= 0.25
            assert seen["face"] > 0                                       # midpoints exactly on a cell face
            assert 2.0 ** (case["L"] - 1) in seen["s"]                    # along the outermost face
            if not with_u and max_steps > 100:                            # on the lattice: every level boundary
                assert seen["s"] >= {2.0 ** l for l in range(case["L"])}
        rays = case["rays"]
        assert (rays[:, 3:6] == 0).any(1).sum() >= N // 4 and ((rays[:, 3:6] != 0).sum(1) == 1).sum() >= N // 8
        if max_steps < 100:
            assert (R.march(dict(case, max_steps=4096))[0] != c64).mean() > 0.1   # max_steps binds
        if kind == "random" and max_steps > 100:
            assert (c64 == 0).any() and c64.max() > 8


def test_multi_family_is_exact_in_fp32_and_meets_the_prefilter_edges():
    experts, rays, run = R.multi_case()
    c64, ri64, a64, b64 = R.multi_expected()
    c32, ri32, a32, b32 = R.march_multi(experts, rays, run, F=np.float32)
    assert (c64 == c32).all() and (ri64 == ri32).all() and (a64 == a32).all() and (b64 == b32).all()
    assert (a64.astype(np.float32) == a64).all() and (b64.astype(np.float32) == b64).all()
    N = R.MULTI_N
    hit = np.array([[R.box_hit(float, [float(v) for v in rays[r]], e["box"]) for r in range(N)] for e in experts])
    hit32 = np.array([[R.box_hit(np.float32, list(rays[r]), e["box"]) for r in range(N)] for e in experts])
    assert (hit == hit32).all()
    assert not hit[:, 0::8][:, :-1].any()                                 # on the face y = 1: dropped
    assert hit[:, 1::8][:, :16].all()                                     # on the face y = -1: kept
    assert hit[1, 2::8][:16].all()                                        # starts inside box 1
    assert (~hit).any(1).all() and (hit[0] != hit[1]).any()               # each box missed; some rays hit one only
    c = c64.reshape(2, N)
    assert (c[:, 1::8][:, :16] > 0).any(1).all()                          # the face-grazing rays do emit samples
    assert (c[~hit] == 0).all()
    for cap in R.STAGE_CAPS:
        caps = R.clamp_capacities(c64, cap)
        assert len(caps) >= (6 if cap < 512 else 5), (cap, caps)          # at cap 512 nothing overflows


@pytest.mark.parametrize("i", [0, 5, 7, 10])
def test_dyadic_reference_is_the_oracles_march(i):
    case = R.march_case(i)
    assert case["u"] is None and case["max_steps"] == 4096
    rays = torch.tensor(case["rays"])
    near = torch.clamp(rays[:, 6], min=R.NEAR_PLANE)
    far = torch.clamp(rays[:, 7], max=R.FAR_PLANE)
    b = torch.tensor(case["bin"]).view(case["L"], case["R"], case["R"], case["R"]).bool()
    ri, t0, t1 = OO.march(rays[:, :3], rays[:, 3:6], near, far, b, case["roi"], case["R"], case["step"])
    counts, rri, r0, r1 = R.march_expected(i)
    assert np.array_equal(ri.numpy(), rri) and np.array_equal(t0.numpy(), r0.astype(np.float32))
    assert np.array_equal(t1.numpy(), r1.astype(np.float32))


@pytest.mark.parametrize("fault,share", [("skip_k_minus_1", 0.2), ("mid_at_t", 0.2)])
def test_march_equality_has_teeth(fault, share):
    """A skip of k - 1 lattice steps re-tests the empty cell it should leave, which never changes the samples of a
    ray but costs an iteration: it shows where max_steps binds.  A midpoint tested at t changes the samples."""
    i = 6 if fault == "skip_k_minus_1" else 0
    good, bad = R.march_expected(i), R.march(R.march_case(i), fault=fault)
    n = min(len(good[2]), len(bad[2]))
    differs = (good[0] != bad[0])
    if n:
        per_ray = np.zeros(len(good[0]), dtype=bool)
        neq = np.flatnonzero(good[2][:n] != bad[2][:n])
        per_ray[np.unique(good[1][neq])] = True
        differs |= per_ray
    print(f"{fault}: rays that differ {differs.mean():.3f}")
    assert differs.mean() >= share


# ------------------------------------------------------------------------------------------------ packed compositing

def _fp32_composite(case, with_bg):
    """Sequential fp32 evaluation (numpy float32 cumsum): one legal order of the kernel's arithmetic."""
    N, M, f = case["N"], case["M"], np.float32
    w, rgb, dep, acc = np.zeros(M, f), np.zeros((N, 3), f), np.zeros(N, f), np.zeros(N, f)
    for r in range(N):
        a, b = case["offs"][r], case["offs"][r + 1]
        sdt = case["rs"][a:b, 3] * (case["t1"][a:b] - case["t0"][a:b])
        E = np.cumsum(sdt, dtype=f) - sdt
        w[a:b] = np.exp(-E, dtype=f) * (f(1) - np.exp(-sdt, dtype=f))
        rgb[r] = (w[a:b, None] * case["rs"][a:b, :3]).sum(0, dtype=f)
        dep[r] = (w[a:b] * (f(0.5) * (case["t0"][a:b] + case["t1"][a:b]))).sum(dtype=f)
        acc[r] = w[a:b].sum(dtype=f)
        if with_bg:
            rgb[r] = rgb[r] + (f(1) - acc[r]) * case["bg"][r]
    return dict(w=w, rgb=rgb, depth=dep, acc=acc)


@pytest.mark.parametrize("name", list(R.PACKED_CASES))
def test_packed_reference_vs_oracle_autograd_and_fp32(name):
    case = R.packed_case(name)
    N, M = case["N"], case["M"]
    ri = torch.repeat_interleave(torch.arange(N), torch.tensor(np.diff(case["offs"]).astype(np.int64)))
    for with_bg in (True, False):
        v, e = R.packed_forward(case, with_bg)
        t = lambda k: torch.tensor(case[k], dtype=torch.float64)
        ref = OO.render_packed(t("rs"), t("t0"), t("t1"), ri, N, t("bg") if with_bg else None)
        for k, o in zip(("rgb", "depth", "w", "acc"), ref):
            assert np.allclose(v[k], o.numpy(), rtol=1e-12, atol=1e-300), (name, k)
        got = _fp32_composite(case, with_bg)
        for k in v:
            assert R.worst_ratio(got[k], v[k], e[k]) <= 1.0, (name, with_bg, k)
    for flags in ((True, True, True, True), (False, False, False, False), (True, False, True, False)):
        val, err = R.packed_backward(case, *flags)
        auto = R.packed_autograd(case, *flags)
        scale = np.abs(auto).max() if M else 1.0
        assert np.abs(val - auto).max(initial=0.0) <= 1e-11 * max(scale, 1.0), (name, flags)
        assert (err > 0).all() or M == 0


@pytest.mark.parametrize("fault", ["no_carry", "inclusive_T"])
def test_packed_bounds_have_teeth(fault):
    """Dropping the chunk carry (every ray longer than 64) or an inclusive transmittance moves the weights, the
    outputs and the sigma gradients by more than 100 times their bounds."""
    for name in ("all_lengths", "N5"):
        case = R.packed_case(name)
        v, e = R.packed_forward(case)
        bad, _ = R.packed_forward(case, fault=fault)
        ratios = {k: R.worst_ratio(bad[k], v[k], e[k]) for k in v}
        print(f"{fault} {name}: forward error / bound {ratios}")
        assert min(ratios.values()) >= 100.0
        if fault == "no_carry":
            val, err = R.packed_backward(case)
            badv, _ = R.packed_backward(case, fault=fault)
            r = R.worst_ratio(badv[:, 3], val[:, 3], err[:, 3])
            print(f"{fault} {name}: d sigma error / bound {r:.1f}")
            assert r >= 100.0


# ------------------------------------------------------------------------------------------------ visibility

def _vis_runs(case):
    N = case["N"]
    yield "plain", dict(eps=R.VIS_EPS, athr=R.VIS_ATHR)
    yield "plain0", dict(eps=R.VIS_EPS, athr=0.0)
    for group in sorted({1, 3, N}):
        n_groups = -(-N // group)
        yield f"group{group}", dict(eps=R.VIS_EPS, athr=R.VIS_ATHR, groups=R.vis_group_thresholds(n_groups, group),
                                    group=group)


def test_visibility_reference_and_left_out_share():
    worst = 0.0
    for name in ("N37", "all_lengths", "N5", "saturated"):
        case = R.packed_case(name)
        N = case["N"]
        ri = torch.repeat_interleave(torch.arange(N), torch.tensor(np.diff(case["offs"]).astype(np.int64)))
        t = lambda k: torch.tensor(case[k], dtype=torch.float64)
        for tag, kw in _vis_runs(case):
            keep, decided = R.visibility(case, **kw)
            worst = max(worst, 1.0 - decided.mean())
            if "groups" not in kw:
                ref = OO.visibility(t("t0"), t("t1"), t("rs")[:, 3], ri, N, float(np.float32(kw["eps"])),
                                    float(np.float32(kw["athr"])))
                assert np.array_equal(keep, ref.numpy()), (name, tag)
            if name == "N37":
                assert 0.05 < keep.mean() < 0.95, (tag, keep.mean())      # both outcomes are common
    print(f"visibility: largest share left out {worst:.4%}")
    assert worst <= 0.01


def test_visibility_group_index_has_teeth():
    """A threshold indexed by r instead of r / group changes the decision of at least 50 decided samples."""
    case = R.packed_case("N37")
    groups = R.vis_group_thresholds(37, 3)                                # long enough to be indexed by r
    keep, decided = R.visibility(case, R.VIS_EPS, R.VIS_ATHR, groups, 3)
    bad, _ = R.visibility(case, R.VIS_EPS, R.VIS_ATHR, groups, 3, fault="group_by_ray")
    n = int(((keep != bad) & decided).sum())
    print(f"group threshold by ray: {n} decided samples differ")
    assert n >= 50


# ------------------------------------------------------------------------------------------------ occupancy update chain

def test_update_threshold_binarize_references():
    occs = np.array([0.5, -1.0, 0.0, 0.25, 1.0], dtype=np.float32)
    out = R.occ_update(occs, np.array([0, 1, -1, 3], dtype=np.int32), np.array([0.1, 9, 9, 0.9], dtype=np.float32), 0.95)
    assert out.tolist() == [float(np.float32(0.5) * np.float32(0.95)), -1.0, 0.0, float(np.float32(0.9)), 1.0]
    for n in R.ELEMENTWISE_N:
        for kind in ("visible", "some_invisible", "all_invisible"):
            o = R.threshold_input(n, kind)
            t0, t1 = R.threshold64(o, 0.01)
            ref = o[o >= 0].astype(np.float64).mean() if (o >= 0).any() else 0.0
            assert float(t0) == min(float(np.float32(ref)), float(np.float32(0.01)))
            assert R.ulp_apart(t1, np.float32(o.astype(np.float64).sum() / n))
            if kind == "all_invisible":
                assert float(t0) == 0.0 and float(t1) == -1.0
            assert R.binarize(o, t0).sum() == (o > t0).sum()
    assert R.ulp_apart(1.0, np.nextafter(np.float32(1), np.float32(2))) and not R.ulp_apart(1.0, 1.0 + 2.0 ** -22)
    o = R.threshold_input(257, "visible")
    assert R.threshold64(o, 1e9)[0] == np.float32(o.astype(np.float64).mean())          # occ_thre not binding


def test_cell_points_reference_lies_in_its_cell():
    for k, g in enumerate(R.CELL_GRIDS):
        cells = R.cell_points_input(g, 257, k)
        x, bound, lo, hi = R.cell_points(g, cells, 21)
        assert ((x >= lo) & (x <= hi)).all() and (cells == -1).sum() > 30
        assert (bound[cells >= 0] > 0).all() and (bound[cells >= 0] < 1e-5).all()
        G = R.make_grid(g["L"], g["R"], g["roi"])
        assert (x[cells < 0] == np.array(G["c"])).all()
        assert (lo.astype(np.float32) == lo).all() and (hi.astype(np.float32) == hi).all()   # dyadic faces


# ------------------------------------------------------------------------------------------------ mark invisible

def test_mark_invisible_reference_and_left_out_share():
    worst = 0.0
    for g in R.INVIS_GRIDS:
        n = g["L"] * g["R"] ** 3
        shares = {}
        for which in R.INVIS_CAMERAS:
            K, c2w = R.invisible_cameras(which)
            vis, decided = R.mark_invisible(g, K, c2w, R.INVIS_W, R.INVIS_H, R.INVIS_NEAR)
            assert vis.shape == (n,) and not (vis & ~decided).any()
            worst = max(worst, 1.0 - decided.mean())
            shares[which] = float(vis.mean())
        assert shares["none"] == 0.0 and shares["behind"] == 0.0
        assert 0.02 < shares["front"] < 1.0 and 0.02 < shares["rotated"] < 1.0 and 0.0 < shares["inside"] < 0.9
    # the axis-aligned camera in closed form: |x / (z + 2)| < 32 / 40 and |y / (z + 2)| < 24 / 40
    g = R.INVIS_GRIDS[0]
    K, c2w = R.invisible_cameras("front")
    vis, decided = R.mark_invisible(g, K, c2w, R.INVIS_W, R.INVIS_H, R.INVIS_NEAR)
    c = (np.arange(16) + 0.5) / 16 * 2 - 1
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    tx, ty = float(np.float32(0.011)), float(np.float32(-0.007))
    u, v = 40 * (X - tx) / (Z + 2) + 32, 40 * (Y - ty) / (Z + 2) + 24
    want = ((u >= 0) & (u < 64) & (v >= 0) & (v < 48)).reshape(-1)
    assert np.array_equal(vis[decided], want[decided])
    print(f"mark_invisible: largest share left out {worst:.4%}")
    assert worst <= 0.02


def test_shape_lists_are_covered_and_small():
    assert {c[2] for c in R.MARCH_CASES} >= set(R.MARCH_N) and max(c[2] for c in R.MARCH_CASES) <= 256
    assert {g["L"] for g in R.MARCH_GRIDS.values()} == {1, 2, 3}
    grids = list(R.MARCH_GRIDS.values()) + R.MULTI_EXPERTS + R.CELL_GRIDS + R.INVIS_GRIDS
    grids += [dict(L=c[0], R=c[1]) for c in R.CONE_CASES]
    assert max(g["L"] * g["R"] ** 3 for g in grids) <= 3 * 16 ** 3 and R.MULTI_N <= 256 and R.CONE_N <= 256
    lens = set()
    for N in R.PACKED_N:
        assert len(R.PACKED_CASES[f"N{N}"]) == N
        lens |= set(R.PACKED_CASES[f"N{N}"])
    assert lens >= set(R.RAY_LENGTHS) and set(R.PACKED_CASES["all_lengths"]) == set(R.RAY_LENGTHS)


def test_integer_references():
    assert R.exclusive_scan([3, 0, 2]).tolist() == [0, 3, 3, 5]
    assert R.ray_counts([0, 0, 2], 4).tolist() == [2, 0, 1, 0]
    pos, ri, t0, t1, cnt = R.compact([1, 0, 1, 1], [0, 0, 1, 3], [1., 2., 3., 4.], [2., 3., 4., 5.], 4)
    assert pos.tolist() == [0, 1, 1, 2, 3] and ri.tolist() == [0, 1, 3] and t0.tolist() == [1., 3., 4.]
    assert cnt.tolist() == [1, 1, 0, 1]
    x, bound, d = R.packed_points(np.array([[1, 2, 3, .5, 0, -1, 0, 9]], dtype=np.float32), [0, 0], [1., 2.], [2., 4.])
    assert x.tolist() == [[1.75, 2.0, 1.5], [2.5, 2.0, 0.0]] and d.tolist() == [[.5, 0, -1]] * 2 and (bound > 0).all()


# ------------------------------------------------------------------------------------------------ cone march

@pytest.mark.parametrize("i", range(len(R.CONE_CASES)))
def test_cone_checks_hold_for_an_fp32_march_and_have_teeth(i):
    """The fp32 run of the marcher (one legal rounding of the kernel's arithmetic), replayed against its own
    fp32-rounded output, passes every one-step check with at most 2 % of them left out; a midpoint tested at t and a
    skip of k + 1 lattice steps each fail at least 100 checks."""
    case = R.cone_case(i)
    counts, _, t0, t1 = R.march(case, F=np.float32)
    assert counts.sum() > 2000 and (t0.astype(np.float32) == t0).all()
    res = R.cone_checks(case, counts, t0, t1)
    share = res["left_out"] / (res["left_out"] + res["checked"])
    print(f"cone case {i}: {counts.sum()} samples, {res['checked']} checks, left out {share:.4%}")
    assert res["failed"] == [] and share <= 0.02
    for fault in ("mid_at_t", "skip_k_plus_1"):
        c, _, a, b = R.march(case, F=np.float32, fault=fault)
        bad = R.cone_checks(case, c, a, b)
        print(f"cone case {i} {fault}: {len(bad['failed'])} of {bad['checked']} checks fail")
        assert len(bad["failed"]) >= 100
    # a step length one fp32 step too long on one sample is seen
    t1b = t1.astype(np.float32).copy()
    t1b[5] = np.nextafter(np.nextafter(t1b[5], np.float32(99)), np.float32(99))
    ray = int(np.searchsorted(np.cumsum(counts), 5, side="right"))
    assert ("dt", ray, 5 - int(R.exclusive_scan(counts)[ray])) in R.cone_checks(case, counts, t0, t1b)["failed"]
