"""The ray front of csrc/rays.hip (pick_pixels, rays_gen with its AABB slab test, clamp_near_far, rays_ndc and the
two-pass dataset build) against the references of tests/rays_reference.py (checked on the CPU by
tests/test_rays_reference.py, which also shows that no input lies inside a decision margin).  Run on an MI355X: -m gpu.

Integer work, keep / hit decisions, colours, origins and the clamp are compared exactly; directions with float64 under
2e-6, slab distances with float64 on the kernel's own o, d under 4 * 2^-24 * max(1, |t|), NDC under the per-column
tolerance measured on the CPU.  Direct calls pre-fill what lies behind each output with a sentinel that must survive.

Every pixel triple handed to rays_gen is in range: the kernel trusts them.

NaN.  C's fmaxf / fminf return the other operand when one is NaN; torch.maximum / torch.minimum and amax / clamp in the
reference propagate it.  Found by this file, on an MI355X, with the kernels on fmaxf / fminf throughout:
  test_clamp_near_far           the row (near, far) = (NaN, 2) with near_override = 0.5 came back valid with near = 0.5
                                (rows 0, 230 / 232 of every n; the reference says invalid, near = far = invalid_value);
  test_aabb_nan_pose            a NaN in the pose's translation gave near = 0, far = 12 .. 16 (the slab of that axis was
                                skipped) where the reference gives NaN, NaN;
  test_dataset_build[5..24]     every case with a NaN-pose image kept 28 .. 40 of its pixels, with NaN origins or
                                directions, where the reference keeps none;
  test_pick_pixels_*            n = 0 was refused (-1): torch gives an empty tensor a NULL pointer and the entry points
                                looked at pix_out first.
clamp_ray and aabb_slab now propagate NaN (max_nan / min_nan in csrc/rays.hip, fmaxf / fminf for every other operand,
so all other outputs keep their bits), and nerf_pick_pixels / _dseed take an empty batch.

Measured on an MI355X after that: directions at most 1.3e-7 from float64 (2e-6 allowed); slab distances at most 0.47 of
their bound; NDC at most 0.50 of the column tolerance; everything else exact.  The whole module takes 3 s."""
import ctypes

import numpy as np
import pytest
import torch

import rays_reference as R

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


def _K():
    from nerf_amd import kernels
    return kernels


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _full(shape, value, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device=DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _in_range(pix, n_poses, H, W):
    pix = np.asarray(pix)
    return bool((pix >= 0).all() and (pix[:, 0] < n_poses).all() and (pix[:, 1] < H).all() and (pix[:, 2] < W).all())


def _check_od(rays, o_ref, d_ref, what):
    """Origins bitwise the pose column, directions within DIR_TOL of float64."""
    assert R.same_bits(rays[:, :3], np.asarray(o_ref, dtype=np.float32)), what
    err = float(np.abs(rays[:, 3:6].astype(np.float64) - d_ref).max())
    assert err <= R.DIR_TOL, (what, err)
    return err


def _check_t(got, ref, what):
    """near / far columns against float64 values: exact where the reference is a constant (invalid, a clamp, an
    override), T_TOL * max(1, |t|) elsewhere; inf and the invalid constants must match exactly."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), what
    ratio = np.abs(got[fin] - ref[fin]) / (R.T_TOL * np.maximum(1.0, np.abs(ref[fin])))
    worst = float(ratio.max(initial=0.0))
    assert worst <= 1.0, (what, worst)
    return worst


# ================================================================================================= pick_pixels

@pytest.mark.parametrize("shape", R.PICK_SHAPES)
def test_pick_pixels_is_the_restated_stream(shape):
    """Every triple equal to the Python-integer reference: n around the 256-thread block, totals of 1, 105, 600 and
    4.8e9 > 2^32 (only the (n,3) output is allocated), seeds 0, 1, 2^63 and 2^64 - 1."""
    K = _K()
    n_images, H, W = shape
    for n in R.PICK_N:
        for seed in R.PICK_SEEDS:
            got = _np(K.pick_pixels(n, n_images, H, W, seed, DEV))
            want = R.pick_pixels(n, n_images, H, W, seed)
            assert got.dtype == np.int32 and np.array_equal(got, want), (shape, n, seed, np.flatnonzero(got != want)[:8])
            if shape == (1, 1, 1):
                assert not got.any()
    assert K.pick_pixels(0, n_images, H, W, 5, DEV).shape == (0, 3)


@pytest.mark.parametrize("mul", R.PICK_MULS)
def test_pick_pixels_device_seed(mul):
    """step_dev in {0, 1, 2^40, -1}: the stream is (seed + step * mul) mod 2^64, read on the device."""
    K = _K()
    n_images, H, W = 3, 7, 5
    for step in R.PICK_STEPS:
        step_dev = torch.tensor([step], dtype=torch.int64, device=DEV)
        for n in (1, 257):
            got = _np(K.pick_pixels(n, n_images, H, W, R.PICK_BASE_SEED, DEV, step_dev=step_dev, seed_mul=mul))
            host = _np(K.pick_pixels(n, n_images, H, W, R.pick_seed(R.PICK_BASE_SEED, step, mul), DEV))
            want = R.pick_pixels(n, n_images, H, W, R.PICK_BASE_SEED, step, mul)
            assert np.array_equal(got, host) and np.array_equal(got, want), (step, mul, n)
    big = _np(K.pick_pixels(257, 3, 40000, 40000, R.PICK_BASE_SEED, DEV, step_dev=step_dev, seed_mul=mul))
    assert np.array_equal(big, R.pick_pixels(257, 3, 40000, 40000, R.PICK_BASE_SEED, -1, mul))
    assert K.pick_pixels(0, 3, 7, 5, 1, DEV, step_dev=step_dev, seed_mul=mul).shape == (0, 3)


# ================================================================================================= rays_gen

@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("H,W", R.DENSE_SHAPES)
def test_rays_gen_dense(H, W, center):
    """H * W = 1, 257, 259 (a 3-thread tail block) and 256; c2w as (3,4), (4,4) and (n,4,4): the dense path uses
    pose 0 in each."""
    K = _K()
    Kin, poses = R.dense_camera(H, W)
    g = np.arange(H * W)
    o_ref, d_ref = R.ray_dirs(H, W, *Kin, center, poses[0], g // W, g % W)
    near, far = R.DENSE_NEAR_FAR
    p44 = np.concatenate([poses, np.broadcast_to(np.float32([0, 0, 0, 1]), (3, 1, 4))], 1)
    outs = []
    for c2w in (poses[0], p44[0], p44):
        rays = _np(K.rays_gen(_d(c2w), H, W, *Kin, near=near, far=far, center_pixels=center))
        assert rays.shape == (H * W, 8)
        err = _check_od(rays, np.broadcast_to(poses[0][:, 3], (H * W, 3)), d_ref, (H, W, center, c2w.shape))
        assert R.same_bits(rays[:, 6], np.full(H * W, near, np.float32)), "near is the float32 of the constant"
        assert R.same_bits(rays[:, 7], np.full(H * W, far, np.float32))
        outs.append(rays)
    assert R.same_bits(outs[0], outs[1]) and R.same_bits(outs[0], outs[2])
    print(f"dense {H}x{W} center={center}: worst direction error {err:.2e}")


@pytest.mark.parametrize("n", R.BATCH_N)
def test_rays_gen_batch(n):
    """(image, row, col) triples over three poses and three 5x7 images, (0,0,0) and the last pixel of the last image
    among them: colours exact, origins bitwise, directions within 2e-6."""
    K = _K()
    H, W = R.BATCH_HW
    Kin, poses = R.dense_camera(H, W)
    for pix, images in R.batch_case(n):
        assert len(pix) == n and _in_range(pix, 3, H, W)
        for center in (True, False):
            rays, rgb = K.rays_gen(_d(poses), H, W, *Kin, pix=_d(pix), near=2.0, far=6.0, center_pixels=center,
                                   images_u8=_d(images))
            rays, rgb = _np(rays), _np(rgb)
            o_ref, d_ref = R.ray_dirs(H, W, *Kin, center, poses[pix[:, 0]], pix[:, 1], pix[:, 2])
            _check_od(rays, o_ref, d_ref, (n, center))
            want = images[pix[:, 0], pix[:, 1], pix[:, 2]].astype(np.float32) / np.float32(255)
            assert R.same_bits(rgb, want), (n, center)
            assert (rays[:, 6] == 2.0).all() and (rays[:, 7] == 6.0).all()


@pytest.mark.parametrize("max_bound,invalid", R.AABB_BOUNDS)
def test_rays_gen_aabb_generic(max_bound, invalid):
    """257 rays of a camera inside the box, one outside looking in and one outside looking away; the slab test in
    float64 on the kernel's own o, d; the same set of invalid rays; max_bound and invalid other than the defaults."""
    K = _K()
    H, W = R.AABB_HW
    poses, pix = R.aabb_case()
    assert _in_range(pix, 3, H, W)
    rays = _np(K.rays_gen(_d(poses), H, W, *R.AABB_K, pix=_d(pix), aabb=_d(np.float32(R.AABB_BOX)),
                          aabb_max_bound=max_bound, aabb_invalid=invalid))
    o_ref, d_ref = R.ray_dirs(H, W, *R.AABB_K, True, poses[pix[:, 0]], pix[:, 1], pix[:, 2])
    _check_od(rays, o_ref, d_ref, "aabb")
    near, far, gap = R.aabb_near_far(rays[:, :3], rays[:, 3:6], R.AABB_BOX, max_bound, invalid)
    iv = np.float32(invalid)
    got_invalid = (rays[:, 6] == iv) & (rays[:, 7] == iv)
    assert np.array_equal(got_invalid, ~(gap > 0)), np.flatnonzero(got_invalid != ~(gap > 0))
    worst = max(_check_t(rays[:, 6], near, "near"), _check_t(rays[:, 7], far, "far"))
    print(f"aabb max_bound {max_bound}: {int(got_invalid.sum())} of {len(pix)} invalid, worst error / bound {worst:.3f}")
    assert 0 < got_invalid.sum() < len(pix)


def test_rays_gen_aabb_exact():
    """1x1 images looking exactly along an axis from power-of-two origins at a power-of-two box: near and far bitwise
    the expected values, with origins inside, on a face, along an edge, parallel to a slab inside and outside it,
    and with the box behind; one direction component is -0.0."""
    K = _K()
    box = _d(np.float32(R.EXACT_BOX))
    for name, axis, sign, origin, max_bound, invalid, near, far in R.AABB_EXACT:
        M = R.exact_pose(axis, sign, origin)
        rays = _np(K.rays_gen(_d(M), 1, 1, 1.0, 1.0, 0.5, 0.5, aabb=box, center_pixels=True, aabb_max_bound=max_bound,
                              aabb_invalid=invalid))
        assert rays.shape == (1, 8)
        assert R.same_bits(rays[0, :3], np.float32(origin)), name
        assert R.same_bits(rays[0, 3:6], R.exact_dir(axis, sign)), (name, rays[0, 3:6])
        assert R.same_bits(rays[0, 6:], np.float32([near, far])), (name, rays[0, 6:], near, far)


def test_aabb_nan_pose():
    """A NaN in the pose's translation or rotation reaches near and far as NaN (the reference's amax / clamp propagate
    it), so clamp_near_far and the dataset build call the ray invalid."""
    K = _K()
    H, W = 3, 5
    Kin, poses = R.dense_camera(H, W)
    for where in ((0, 3), (1, 1)):
        M = poses[0].copy()
        M[where] = np.nan
        rays = K.rays_gen(_d(M), H, W, *Kin, aabb=_d(np.float32([-9, -9, -9, 9, 9, 9])))
        got = _np(rays)
        assert np.isnan(got[:, 6]).all() and np.isnan(got[:, 7]).all(), (where, got[:, 6:])
        for near in (None, 0.5):
            out, valid = K.clamp_near_far(rays, near, None if near is None else 4.0)
            assert not _np(valid).any(), (where, near)
            if near is not None:
                assert np.isinf(_np(out)[:, 6:]).all()


# ================================================================================================= clamp_near_far

@pytest.mark.parametrize("n", R.CLAMP_N)
def test_clamp_near_far(n):
    """Rays and valid equal to the float32 reference for every override combination and invalid value: far == near +
    eps and one ulp either side, near + eps rounding back to near, +-inf, and NaN in near, in far and in both (a NaN
    stays NaN through the override and the ray is invalid).  With neither override the rays come back bit for bit."""
    K = _K()
    L, ptr, stream = _api()
    rays = R.clamp_rays(n)
    assert np.isnan(rays[0, 6]) and (n == 1 or np.isnan(rays[-R.clamp_specials().shape[0]:, 6:]).any())
    drays = _d(rays)
    for hn, nv, hf, fv in R.CLAMP_OVERRIDES:
        for invalid in R.CLAMP_INVALID:
            a, b, ok = R.clamp_near_far(rays[:, 6], rays[:, 7], hn, nv, hf, fv, R.CLAMP_EPS, invalid)
            out, valid = K.clamp_near_far(drays, nv if hn else None, fv if hf else None, R.CLAMP_EPS, invalid)
            out, valid = _np(out), _np(valid)
            what = (n, hn, nv, hf, fv, invalid)
            assert np.array_equal(valid, ok), (what, np.flatnonzero(valid != ok)[:8], rays[valid != ok][:8, 6:])
            assert R.same_bits(out[:, :6], rays[:, :6]), what
            assert R.same_bits(out[:, 6], a) and R.same_bits(out[:, 7], b), (what, out[:4, 6:], a[:4], b[:4])
            if not (hn or hf):
                assert R.same_bits(out, rays), what
            # valid_out = NULL: accepted, and the rays are rewritten all the same
            raw = _d(np.concatenate([rays, np.full((1, 8), R.SENT, np.float32)]))
            assert L.nerf_clamp_near_far(ptr(raw), n, hn, nv, hf, fv, R.CLAMP_EPS, invalid, None, stream()) == 0
            raw = _np(raw)
            assert R.same_bits(raw[:n], out) and (raw[n] == R.SENT).all(), what
    assert R.same_bits(_np(drays), rays)                                 # the wrapper works on a copy


# ================================================================================================= rays_ndc

@pytest.mark.parametrize("n,c", R.NDC_CASES)
def test_rays_ndc(n, c):
    """Rays down -z and +z and origins on the near plane, at the reference setting and at a tiny odd one; columns 6
    and 7 exactly 0 and 1, the others within max(4 x the float32 oracle's measured error, 4 * 2^-24) of the column's
    max |ref|.  The output is a tensor of its own."""
    K = _K()
    H, W, focal, near_plane = R.NDC_CONFIGS[c]
    rays = R.ndc_rays_input(n, c)
    drays = _d(rays)
    out = K.rays_ndc(drays, H, W, focal, near_plane)
    assert out.data_ptr() != drays.data_ptr() and R.same_bits(_np(drays), rays)
    got = _np(out).astype(np.float64)
    ref = R.ndc(rays, H, W, focal, near_plane)
    assert (got[:, 6] == 0).all() and (got[:, 7] == 1).all()
    ratio = np.abs(got - ref)[:, :6].max(0) / R.ndc_tolerance(ref)
    print(f"ndc n={n} config {c}: error / tolerance per column " + " ".join(f"{r:.3f}" for r in ratio))
    assert (ratio <= 1.0).all(), ratio


# ================================================================================================= dataset build

class _MD:
    """What nerf_amd.data.build_run reads of an ImageMetadata."""

    def __init__(self, case, k):
        self.H, self.W = case["H"], case["W"]
        self.c2w = torch.from_numpy(case["c2w"][k])
        self.intrinsics = torch.from_numpy(case["intr"][k])
        self.image_index = int(case["image_index"][k])


def _check_rows(case, exp, rays, rgb, idx, what):
    """Kept rows (numpy) against the reference: count, order, ids and colours exact, o bitwise, d within 2e-6,
    near / far by the float64 slab test on the row's own o, d followed by the float32 clamp."""
    total = int(exp["flags"].sum())
    assert rays.shape == (total, 8) and rgb.shape == (total, 3) and idx.shape == (total,), what
    assert np.array_equal(idx, exp["idx"]), what
    assert R.same_bits(rgb, exp["rgb"]), what
    if total == 0:
        return
    _check_od(rays, exp["rays"][:, :3], exp["rays"][:, 3:6], what)      # ascending pixel order: row r is kept pixel r
    near, far, gap = R.aabb_near_far(rays[:, :3], rays[:, 3:6], case["aabb"], R.DATASET_BOUND, R.DATASET_BOUND)
    assert (gap > 0).all(), what
    hn, nv, hf, fv = R.override_args(case["override"])
    a, b, ok = R.clamp_near_far(near, far, hn, nv, hf, fv, R.DATASET_EPS, np.inf)
    assert ok.all(), what
    _check_t(rays[:, 6], a, what)
    _check_t(rays[:, 7], b, what)
    if hn and np.isfinite(nv):
        assert (rays[:, 6][exp["rays"][:, 6] == nv] == np.float32(nv)).all(), what
    if hf:
        assert (rays[:, 7][exp["rays"][:, 7] == fv] == np.float32(fv)).all(), what


def _direct(case, exp):
    """Count pass and write pass through the C entry point with sentinels behind every output."""
    L, ptr, stream = _api()
    H, W, n_img = case["H"], case["W"], case["n_images"]
    n = n_img * H * W
    hn, nv, hf, fv = R.override_args(case["override"])
    keep = dict(c2w=_d(case["c2w"].reshape(n_img, 12)), intr=_d(case["intr"]), ids=_d(case["image_index"]),
                aabb=_d(np.float32(case["aabb"])), images=_d(case["images"]), masks=_d(case["masks"]))
    args = (ptr(keep["c2w"]), ptr(keep["intr"]), ptr(keep["ids"]), n_img, H, W, int(case["center"]), ptr(keep["aabb"]),
            hn, nv, hf, fv, ptr(keep["images"]), ptr(keep["masks"]))
    flags = _full(n + 8, R.ISENT, I32)
    assert L.nerf_dataset_rays(*args, ptr(flags), None, None, None, None, stream()) == 0
    got = _np(flags)
    assert (got[n:] == R.ISENT).all()
    bad = np.flatnonzero(got[:n] != exp["flags"])
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), exp["hit_gap"][bad[:8]], exp["keep_gap"][bad[:8]])
    total = int(exp["pos"][-1])
    rays, rgb, idx = _full((total + 8, 8), R.SENT), _full((total + 8, 3), R.SENT), _full(total + 8, R.ISENT, I32)
    if total:
        pos = _d(exp["pos"])
        assert L.nerf_dataset_rays(*args, None, ptr(pos), ptr(rays), ptr(rgb), ptr(idx), stream()) == 0
    torch.cuda.synchronize()
    del keep
    rays, rgb, idx = _np(rays), _np(rgb), _np(idx)
    assert (rays[total:] == R.SENT).all() and (rgb[total:] == R.SENT).all() and (idx[total:] == R.ISENT).all()
    return rays[:total], rgb[:total], idx[:total]


@pytest.mark.parametrize("i", range(len(R.DATASET_CASES)))
def test_dataset_build(i):
    """Runs of 1, 8 (280 pixels: two blocks) and 59 (2065 pixels: past the 2048-element scan tile) 5x7 images with
    per-image poses and intrinsics, descending ids, random masks, fully masked, missing and NaN-pose images first, in
    the middle and last, one case that keeps its last pixel alone and one that keeps nothing; every override.  Through
    the C entry point (flags exact, sentinels kept) and through nerf_amd.data.build_run (boundaries, kept ids)."""
    from nerf_amd.data import build_run
    case, exp = R.dataset_expected(i)
    what = R.DATASET_CASES[i]
    rays, rgb, idx = _direct(case, exp)
    _check_rows(case, exp, rays, rgb, idx, what)
    run = [(_MD(case, k), case["images"][k], torch.from_numpy(case["masks"][k]).bool())
           for k in range(case["n_images"])]
    r2, c2, i2, kept = build_run(run, _d(np.float32(case["aabb"])), case["center"], case["override"],
                                 torch.device(DEV))
    bounds = exp["bounds"]
    want_kept = [int(case["image_index"][k]) for k in range(case["n_images"]) if bounds[k + 1] > bounds[k]]
    assert kept == want_kept, what
    assert r2.shape == (int(bounds[-1]), 8) and i2.dtype == I32
    assert R.same_bits(_np(r2), rays) and R.same_bits(_np(c2), rgb) and np.array_equal(_np(i2), idx), what
    # per-image boundaries: the rows of image k are bounds[k] .. bounds[k + 1]
    ids = np.repeat(case["image_index"], np.diff(bounds))
    assert np.array_equal(idx, ids), what
    if case["keep"] == "nothing":
        assert kept == [] and r2.shape[0] == 0 and c2.shape == (0, 3) and i2.shape == (0,)
    if case["keep"] == "last_pixel":
        assert kept == [int(case["image_index"][-1])] and r2.shape[0] == 1


@pytest.mark.parametrize("i", [j for j, c in enumerate(R.DATASET_CASES) if c.get("shared_intrinsics")])
def test_dataset_and_batch_generator_give_the_same_bits(i):
    """make_ray and clamp_ray are shared: rays_gen on the kept pixels followed by clamp_near_far with the override is
    the dataset's rows bit for bit."""
    K = _K()
    case, exp = R.dataset_expected(i)
    rows, _, _ = _direct(case, exp)
    pix = exp["kept_pixels"]
    assert len(pix) > 50 and _in_range(pix, case["n_images"], case["H"], case["W"])
    assert (case["intr"] == case["intr"][0]).all()
    fx, fy, cx, cy = (float(v) for v in case["intr"][0])
    rays = K.rays_gen(_d(case["c2w"]), case["H"], case["W"], fx, fy, cx, cy, pix=_d(pix),
                      aabb=_d(np.float32(case["aabb"])), center_pixels=case["center"])
    hn, nv, hf, fv = R.override_args(case["override"])
    out, valid = K.clamp_near_far(rays, nv if hn else None, fv if hf else None)
    assert _np(valid).all()
    assert R.same_bits(_np(out), rows), np.flatnonzero((_np(out) != rows).any(1))[:8]


def test_dataset_no_images():
    L, ptr, stream = _api()
    flags = _full(8, R.ISENT, I32)
    assert L.nerf_dataset_rays(None, None, None, 0, 5, 7, 1, None, 0, 0.0, 0, 0.0, None, None, ptr(flags), None, None,
                               None, None, stream()) == 0
    torch.cuda.synchronize()
    assert (_np(flags) == R.ISENT).all()


# ================================================================================================= refusals

def test_refusals_return_before_any_launch():
    L, ptr, stream = _api()
    H, W = 5, 7
    c2w = _d(R.dense_camera(H, W)[1])
    rays, rgb = _full((H * W + 1, 8), R.SENT), _full((H * W, 3), R.SENT)
    images = torch.zeros((3, H, W, 3), dtype=torch.uint8, device=DEV)
    tail = (H, W, 9.0, 9.0, 3.5, 2.5, 1, 2.0, 6.0, None, 1e10, 1e10)
    # pix = NULL and n != H * W
    assert L.nerf_rays_gen(ptr(c2w), 3, None, H * W - 1, *tail, None, ptr(rays), None, stream()) == -1
    # images without rgb_out
    assert L.nerf_rays_gen(ptr(c2w), 3, None, H * W, *tail, ptr(images), ptr(rays), None, stream()) == -1
    # rays_out off by 4 bytes
    off = ctypes.c_void_p(rays.data_ptr() + 4)
    assert L.nerf_rays_gen(ptr(c2w), 3, None, H * W, *tail, None, off, None, stream()) == -2
    # dataset: write pass with a misaligned out_rays, count pass without flags
    case, exp = R.dataset_expected(0)
    n = case["n_images"] * H * W
    keep = dict(c2w=_d(case["c2w"].reshape(-1, 12)), intr=_d(case["intr"]), ids=_d(case["image_index"]),
                aabb=_d(np.float32(case["aabb"])), images=_d(case["images"]), masks=_d(case["masks"]))
    args = (ptr(keep["c2w"]), ptr(keep["intr"]), ptr(keep["ids"]), case["n_images"], H, W, 1, ptr(keep["aabb"]),
            0, 0.0, 0, 0.0, ptr(keep["images"]), ptr(keep["masks"]))
    pos, idx = _d(exp["pos"]), _full(n, R.ISENT, I32)
    assert L.nerf_dataset_rays(*args, None, ptr(pos), off, ptr(rgb), ptr(idx), stream()) == -2
    assert L.nerf_dataset_rays(*args, None, None, None, None, None, stream()) == -1
    # pick_pixels with H = 0
    pix = _full((4, 3), R.ISENT, I32)
    assert L.nerf_pick_pixels(4, 3, 0, 7, U64(1), ptr(pix), stream()) == -1
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert L.nerf_pick_pixels_dseed(4, 3, 0, 7, U64(1), U64(1), ptr(step), ptr(pix), stream()) == -1
    torch.cuda.synchronize()
    assert (_np(rays) == R.SENT).all() and (_np(rgb) == R.SENT).all() and (_np(idx) == R.ISENT).all()
    assert (_np(pix) == R.ISENT).all()
