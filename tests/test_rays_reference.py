"""CPU checks of tests/rays_reference.py: the references are right (against oracle/nerf_oracle.py in float64, float32
for the clamp, and against literals worked out apart from the reference), and the inputs that tests/test_gpu_ray_front.py
runs on meet the conditions its exact comparisons rest on: no ray or pixel inside a decision margin, both outcomes
common in every dataset case, the exact AABB family exact in float32, and an NDC tolerance measured here."""
import numpy as np
import pytest
import torch

import rays_reference as R
from oracle import nerf_oracle as O

F64 = torch.float64


def _t(a, dtype=F64):
    return torch.tensor(np.asarray(a), dtype=dtype)


# ------------------------------------------------------------------------------------------------ pick_pixels

def test_pick_pixels_hand_computed():
    """z and k of three (p, seed) pairs, from a separate C evaluation of the kernel's expression with a 128-bit
    product; the triples are k split by hand."""
    assert R.mix64(0) == 0 and R.mix64(1) == 0x5692161D100B05E5         # splitmix64's finaliser on 1
    lit = ((0, 0, 0x58016DF76F315627, 36, (1, 0, 1), 1650104703, (1, 1252, 24703)),
           (256, 1, 0xCD64042802D06E37, 84, (2, 2, 4), 3851075407, (2, 16276, 35407)),
           (123456789, R.M64, 0x95548AE870B5ED78, 61, (1, 5, 1), 2799942085, (1, 29998, 22085)))
    for p, seed, z, k, triple, k_big, triple_big in lit:
        assert R.mix64(seed * R.GOLDEN + R.mix64(p + R.PIX_STREAM)) == z
        assert (z * 105) >> 64 == k and (z * 4800000000) >> 64 == k_big
        assert R.pick_one(p, seed, 3, 7, 5) == triple
        assert R.pick_one(p, seed, 3, 40000, 40000) == triple_big
    assert R.pick_pixels(257, 3, 7, 5, 1)[256].tolist() == [2, 2, 4]
    assert R.pick_pixels(4, 1, 1, 1, 99).tolist() == [[0, 0, 0]] * 4
    assert R.pick_pixels(0, 3, 7, 5, 1).shape == (0, 3)


def test_pick_pixels_seed_arithmetic():
    assert R.pick_seed(5) == 5 and R.pick_seed(-1) == R.M64
    assert R.pick_seed(R.M64, 1, 1) == 0
    assert R.pick_seed(7, -1, 3) == (7 - 3) % 2 ** 64                   # -1 is 2^64 - 1
    assert R.pick_seed(7, 1 << 40, R.GOLDEN) == (7 + (R.GOLDEN << 40)) % 2 ** 64
    a = R.pick_pixels(64, 3, 7, 5, 7, step=-1, seed_mul=3)
    assert np.array_equal(a, R.pick_pixels(64, 3, 7, 5, 4)) and not np.array_equal(a, R.pick_pixels(64, 3, 7, 5, 7))


def test_pick_pixels_large_total():
    """tot = 3 * 40000 * 40000 > 2^32: in-range triples that use the whole range."""
    pix = R.pick_pixels(2000, 3, 40000, 40000, 12345)
    assert pix.min() >= 0 and pix[:, 0].max() == 2 and pix[:, 1:].max() < 40000
    assert pix[:, 1].max() > 39000 and pix[:, 2].max() > 39000 and set(pix[:, 0].tolist()) == {0, 1, 2}
    k = pix[:, 0].astype(np.int64) * 1600000000 + pix[:, 1].astype(np.int64) * 40000 + pix[:, 2]
    assert (k > 2 ** 32).sum() > 100


def test_pick_pixels_chi_square():
    """2^16 draws over 3 * 7 * 5 = 105 cells: chi-square under the 99.9 % quantile of 104 degrees of freedom
    (153.2, Wilson-Hilferty: 104 (1 - 2 / 936 + 3.0902 sqrt(2 / 936))^3 = 153.2)."""
    n = 1 << 16
    pix = R.pick_pixels(n, 3, 7, 5, 2024).astype(np.int64)
    cells = np.bincount(pix[:, 0] * 35 + pix[:, 1] * 5 + pix[:, 2], minlength=105)
    chi2 = float(((cells - n / 105) ** 2 / (n / 105)).sum())
    print(f"pick_pixels chi-square over 105 cells: {chi2:.1f}")
    assert cells.min() > 0 and chi2 < 153.2


# ------------------------------------------------------------------------------------------------ rays against the oracle

def _oracle_rays(H, W, K, center, c2w, aabb=None, near=None, far=None, max_bound=1e10, invalid=1e10):
    dirs = O.get_ray_directions(H, W, *[float(np.float32(v)) for v in K], center, dtype=F64)
    box = None if aabb is None else _t(aabb).view(2, 3)
    return O.get_rays(dirs, _t(c2w), box, near, far, float(np.float32(max_bound)),
                      float(np.float32(invalid))).reshape(-1, 8).numpy()


@pytest.mark.parametrize("H,W", R.DENSE_SHAPES)
@pytest.mark.parametrize("center", [True, False])
def test_ray_dirs_is_the_oracles(H, W, center):
    K, poses = R.dense_camera(H, W)
    g = np.arange(H * W)
    o, d = R.ray_dirs(H, W, *K, center, poses[0], g // W, g % W)
    ref = _oracle_rays(H, W, K, center, poses[0], near=1.0, far=2.0)
    assert np.abs(o - ref[:, :3]).max() == 0 and np.abs(d - ref[:, 3:6]).max() < 1e-14
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 2e-7           # the float32 pose is orthonormal to 2^-24
    o2, d2 = R.ray_dirs(H, W, *K, center, poses[[0] * len(g)], g // W, g % W)     # one pose per pixel
    assert np.array_equal(o, o2) and np.array_equal(d, d2)


def _generic_aabb_rays():
    poses, pix = R.aabb_case()
    H, W = R.AABB_HW
    o, d = R.ray_dirs(H, W, *R.AABB_K, True, poses[pix[:, 0]], pix[:, 1], pix[:, 2])
    return poses, pix, o.astype(np.float32), d.astype(np.float32)       # what the kernel hands the slab test


@pytest.mark.parametrize("max_bound,invalid", R.AABB_BOUNDS)
def test_aabb_is_the_oracles_and_clear_of_the_margin(max_bound, invalid):
    poses, pix, o, d = _generic_aabb_rays()
    near, far, gap, tmax = R.aabb_near_far(o, d, R.AABB_BOX, max_bound, invalid, with_tmax=True)
    n, f = O.ray_aabb_intersect(_t(o), _t(d), _t(R.AABB_BOX).view(2, 3), R.EPS_DIR, float(np.float32(max_bound)),
                                float(np.float32(invalid)))
    assert np.array_equal(near, n.numpy()) and np.array_equal(far, f.numpy())
    # through the whole of get_rays as well, on one pose
    H, W = R.AABB_HW
    ref = _oracle_rays(H, W, R.AABB_K, True, poses[1], R.AABB_BOX, max_bound=max_bound, invalid=invalid)
    g = np.arange(H * W)
    o1, d1 = R.ray_dirs(H, W, *R.AABB_K, True, poses[1], g // W, g % W)
    n1, f1, _ = R.aabb_near_far(o1, d1, R.AABB_BOX, max_bound, invalid)
    assert np.allclose(n1, ref[:, 6], rtol=1e-12, atol=0) and np.allclose(f1, ref[:, 7], rtol=1e-12, atol=0)
    # input conditions
    assert not R.in_margin(gap, tmax).any(), np.flatnonzero(R.in_margin(gap, tmax))
    valid = gap > 0
    by_pose = [valid[pix[:, 0] == k] for k in range(3)]
    print(f"aabb max_bound {max_bound}: valid {valid.mean():.3f}, per pose {[round(float(v.mean()), 3) for v in by_pose]}")
    assert not by_pose[2].any()                                         # looking away
    if max_bound == 1e10:
        assert by_pose[0].all() and 0.2 < by_pose[1].mean() < 0.8 and (near[valid & (pix[:, 0] == 0)] == 0).all()
    if max_bound == 1.0:
        assert not by_pose[1].any() and (far[valid] == 1.0).sum() > 10 and (far[valid] < 1.0).sum() > 10
        assert (near[~valid] == -1.0).all() and (far[~valid] == -1.0).all()
    if max_bound == 3.0:
        assert (far[valid & (pix[:, 0] == 1)] == 3.0).sum() > 10


def test_aabb_exact_family():
    """Each literal of AABB_EXACT is what the float64 reference and a float32 step-by-step evaluation give, the
    direction is +-e_axis with a -0.0 component, and the family holds the `<=` cases (gap == 0)."""
    zero_gap = 0
    for name, axis, sign, origin, max_bound, invalid, near, far in R.AABB_EXACT:
        d = R.exact_dir(axis, sign)
        M = R.exact_pose(axis, sign, origin)
        o64, d64 = R.ray_dirs(1, 1, 1.0, 1.0, 0.5, 0.5, True, M, [0], [0])
        assert np.array_equal(d64[0], d.astype(np.float64)) and np.array_equal(o64[0], np.float64(origin)), name
        assert np.signbit(d).sum() >= 1 and np.signbit(d[(axis + 1) % 3]) and d[(axis + 1) % 3] == 0, name
        n64, f64, gap = R.aabb_near_far(d * 0 + np.float32(origin), d, R.EXACT_BOX, max_bound, invalid)
        n32, f32 = R.slab_fp32(origin, d, R.EXACT_BOX, max_bound, invalid)
        assert (float(n64), float(f64)) == (near, far) == (float(n32), float(f32)), (name, n64, f64, n32, f32)
        zero_gap += int(gap == 0)
        # the oracle in float32 agrees bit for bit as well
        n, f = O.ray_aabb_intersect(_t([origin], torch.float32), _t([d], torch.float32),
                                    _t(R.EXACT_BOX, torch.float32).view(2, 3), 1e-8, max_bound, invalid)
        assert (float(n), float(f)) == (near, far), name
    assert zero_gap >= 3


def test_clamp_is_the_oracles_in_float32():
    for n in R.CLAMP_N:
        rays = R.clamp_rays(n)
        for hn, nv, hf, fv in R.CLAMP_OVERRIDES:
            for invalid in R.CLAMP_INVALID:
                a, b, ok = R.clamp_near_far(rays[:, 6], rays[:, 7], hn, nv, hf, fv, R.CLAMP_EPS, invalid)
                override = (nv if hn else None, fv if hf else None) if (hn or hf) else None
                out, valid = O.clamp_rays_near_far(torch.tensor(rays), override, R.CLAMP_EPS, invalid)
                assert np.array_equal(ok, valid.numpy()), (n, hn, nv, hf, fv)
                assert R.same_bits(a, out[:, 6].numpy()) and R.same_bits(b, out[:, 7].numpy()), (n, hn, nv, hf, fv)
                if not (hn or hf):
                    assert R.same_bits(a, rays[:, 6]) and R.same_bits(b, rays[:, 7])
    # the rows the table is there for
    sp = R.clamp_specials()
    a, b, ok = R.clamp_near_far(sp[:, 0], sp[:, 1], 1, 0.5, 1, 4.0, R.CLAMP_EPS, np.inf)
    assert not ok[:3].any() and np.isinf(a[:3]).all() and np.isinf(b[:3]).all()             # NaN rows: invalid
    assert ok[3:6].tolist() == [False, False, True]                    # far == near + eps, one ulp under, one over
    _, _, ok0 = R.clamp_near_far(sp[:, 0], sp[:, 1], 0, 0.0, 0, 0.0, R.CLAMP_EPS, np.inf)
    # near = 16: near + eps rounds up to the next float32, which is far; near >= 32: it rounds back to near
    assert ok0[6:10].tolist() == [False, False, True, True]
    assert np.float32(16) + np.float32(R.CLAMP_EPS) == sp[6, 1] and np.float32(32) + np.float32(R.CLAMP_EPS) == 32
    assert ok0[10:17].sum() == 0 and ok[10] and ok[11]                  # +-inf rows; -inf near / inf far overridden


@pytest.mark.parametrize("n,c", R.NDC_CASES)
def test_ndc_is_the_oracles(n, c):
    H, W, focal, near_plane = R.NDC_CONFIGS[c]
    rays = R.ndc_rays_input(n, c)
    ref = O.ndc_rays(H, W, float(np.float32(focal)), float(np.float32(near_plane)), _t(rays)).numpy()
    got = R.ndc(rays, H, W, focal, near_plane)
    assert np.allclose(got, ref, rtol=1e-13, atol=1e-13)
    assert (got[:, 6] == 0).all() and (got[:, 7] == 1).all()
    on_plane = rays[:, 2] == -np.float32(near_plane)
    assert on_plane.sum() >= (n + 4) // 5 and (rays[:, 5] < 0).sum() >= n // 2 and ((rays[:, 5] > 0).sum() >= n // 2)
    assert np.allclose(got[on_plane, 2], -1.0, rtol=0, atol=1e-15)      # t = 0: o stays on the near plane


def test_ndc_tolerance_is_measured():
    """The float32 oracle against the float64 reference, per column relative to max |ref|: the measurement is what
    NDC_REL_ERR records, and four times it stays under the 1e-5 the suite used before."""
    worst = np.zeros(6)
    for n, c in R.NDC_CASES:
        H, W, focal, near_plane = R.NDC_CONFIGS[c]
        rays = R.ndc_rays_input(n, c)
        f32 = O.ndc_rays(H, W, focal, near_plane, torch.tensor(rays)).numpy().astype(np.float64)
        ref = R.ndc(rays, H, W, focal, near_plane)
        worst = np.maximum(worst, np.abs(f32 - ref)[:, :6].max(0) / np.abs(ref[:, :6]).max(0))
        assert (f32[:, 6] == 0).all() and (f32[:, 7] == 1).all()
    print("ndc float32 error / max |ref| per column:", " ".join(f"{w:.3e}" for w in worst))
    rec = np.array(R.NDC_REL_ERR)
    assert (worst <= rec).all() and (rec <= 2 * worst + 2.0 ** -24).all()        # recorded, and not padded
    assert (4 * rec < 1e-5).all()
    tol = R.ndc_tolerance(ref)
    assert tol.shape == (6,) and (tol >= R.T_TOL * np.abs(ref[:, :6]).max(0)).all()


# ------------------------------------------------------------------------------------------------ dataset build

def _oracle_dataset(case):
    """The kept rows by the oracle in float64, image by image (get_rays + clamp + mask), concatenated."""
    rows, idx = [], []
    for k in range(case["n_images"]):
        rays = torch.tensor(_oracle_rays(case["H"], case["W"], case["intr"][k], case["center"], case["c2w"][k],
                                         case["aabb"], max_bound=R.DATASET_BOUND, invalid=R.DATASET_BOUND))
        rays, valid = O.clamp_rays_near_far(rays, case["override"], R.DATASET_EPS, float("inf"))
        keep = valid.numpy() & (case["masks"][k].reshape(-1) != 0)
        rows.append(rays.numpy()[keep])
        idx += [int(case["image_index"][k])] * int(keep.sum())
    return np.concatenate(rows), np.array(idx, dtype=np.int32)


@pytest.mark.parametrize("i", range(len(R.DATASET_CASES)))
def test_dataset_case(i):
    case, exp = R.dataset_expected(i)
    n = case["n_images"] * 35
    flags = exp["flags"]
    rows, idx = _oracle_dataset(case)
    assert rows.shape == exp["rays"].shape and np.array_equal(idx, exp["idx"])
    assert np.allclose(rows, exp["rays"], rtol=1e-12, atol=1e-13)
    assert np.array_equal(exp["pos"], np.concatenate([[0], np.cumsum(flags)])) and exp["bounds"][-1] == flags.sum()
    assert len(exp["bounds"]) == case["n_images"] + 1 and exp["rgb"].dtype == np.float32
    px = case["images"].reshape(n, 3)[flags == 1]
    assert np.array_equal(exp["rgb"], (torch.tensor(px).float() / 255.0).numpy())
    kp = exp["kept_pixels"]
    assert np.array_equal((kp[:, 0] * 5 + kp[:, 1]) * 7 + kp[:, 2], np.flatnonzero(flags))
    assert (np.diff(case["image_index"]) == -3).all()
    # input conditions: nothing inside a decision margin, both outcomes common
    hit, keep = R.in_margin(exp["hit_gap"], exp["hit_scale"]), R.in_margin(exp["keep_gap"], exp["keep_scale"])
    assert not hit.any() and not keep.any(), (np.flatnonzero(hit), np.flatnonzero(keep))
    assert np.array_equal(flags == 1, exp["keep_gap"] > 0)
    share = float(flags.mean())
    print(f"dataset case {i} {R.DATASET_CASES[i]}: kept {share:.3f} of {n}")
    if case["keep"] == "random":
        assert 0.2 <= share <= 0.8
    elif case["keep"] == "last_pixel":
        assert flags.sum() == 1 and flags[-1] == 1
    else:
        assert flags.sum() == 0
    # the special images do what they are there for
    lay, per_image = case["layout"], flags.reshape(case["n_images"], 35).sum(1)
    for k in lay["masked"] + lay["miss"] + lay["nan_t"] + lay["nan_r"]:
        assert per_image[k] == 0
    unmasked = case["masks"].reshape(case["n_images"], 35).sum(1)
    for k in lay["miss"] + lay["nan_t"] + lay["nan_r"]:
        assert unmasked[k] > 20
    for k in lay["miss"]:
        assert (exp["hit_gap"].reshape(-1, 35)[k] < -1).all()
    for k in lay["nan_t"] + lay["nan_r"]:
        assert np.isnan(exp["hit_gap"].reshape(-1, 35)[k]).all()


def test_dataset_cases_cover_the_edges():
    cases = [R.dataset_expected(i) for i in range(len(R.DATASET_CASES))]
    assert {c["n_images"] for c, _ in cases} == {1, 8, 59}
    assert 8 * 35 > 256 and 59 * 35 > 2048 > 58 * 35
    for n_images in (8, 59):
        mine = [(c, e) for c, e in cases if c["n_images"] == n_images and c["keep"] == "random"]
        assert {c["center"] for c, _ in mine} == {True, False}
        assert {c["override"] for c, _ in mine} >= set(R.DS_OVERRIDES)
        lays = [c["layout"] for c, _ in mine]
        last, mid = n_images - 1, n_images // 2
        assert any(0 in l["masked"] for l in lays) and any(mid in l["masked"] for l in lays)
        assert any(last in l["masked"] for l in lays)
        assert any(0 in l["miss"] for l in lays) and any(last in l["miss"] for l in lays)
        assert any(l["nan_t"] for l in lays) and any(l["nan_r"] for l in lays)
    # overrides change the outcome: the far and the near override each drop or rewrite rays of the plain case
    by = {(c["n_images"], tuple(sorted(c["layout"]["masked"])), c["override"]): e for c, e in cases
          if c["keep"] == "random" and "shared" not in c}
    assert any(e["rays"][:, 6].min() == 0.5 for (_, _, o), e in by.items() if o == (0.5, 4.0))
    assert any(e["rays"][:, 7].max() == 4.0 for (_, _, o), e in by.items() if o == (None, 4.0))
