"""Plain references of the ray front of csrc/rays.hip (pick_pixels, rays_gen with its AABB slab test, clamp_near_far,
rays_ndc and the two-pass dataset build), and the inputs the GPU tests of tests/test_gpu_ray_front.py run on.  numpy
and Python integers only; nothing here imports nerf_amd.  tests/test_rays_reference.py checks all of it on the CPU.

What is compared how
  pick_pixels       Python integers modulo 2^64: exact.
  directions        float64 on the float32 inputs; the kernel must be within DIR_TOL = 2e-6 absolute (about 17 * 2^-24
                    worst case for subtract, divide, norm, divide and a 3-term rotation with orthonormal R).
  AABB near / far   float64 slab test on the kernel's own float32 o, d; T_TOL * max(1, |t|) = 4 * 2^-24 * max(1, |t|):
                    subtract, reciprocal and multiply are each correctly rounded.  The hit / miss decision is compared
                    exactly: aabb_near_far returns a signed gap (below) and the shipped inputs keep every ray out of
                    the margin MARGIN * max(1, |tmax|) around gap = 0.
  clamp_near_far    numpy float32, op for op: exact, NaN and inf rows included.
  rays_ndc          float64; per-column tolerance from the float32 oracle's own error, see NDC_REL_ERR.
  dataset build     flags, scan, boundaries, image ids and colours exact; ray columns as above.

The signed gap.  With tmin, tmax the slab interval before the clamp to [0, max_bound], a ray is valid iff
tmax > tmin and tmax > 0 and tmin < max_bound (the clamp is monotone, so clamped tmax <= clamped tmin exactly when one
of the three fails).  gap is the smallest of the three slacks (tmax - tmin, tmax, max_bound - tmin): positive for a
valid ray, where it is tmax - tmin unless a clamp binds sooner, and otherwise minus the largest deficit, i.e. how far the
ray is from becoming valid.  Exactly representable cases (AABB_EXACT) sit at gap = 0 on purpose and are judged bitwise.
"""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
PIX_STREAM = 0x632BE59BD9B4E019

EPS_DIR = float(np.float32(1e-8))          # the slab test's replacement for |d| < eps
DIR_TOL = 2e-6
T_TOL = 4.0 * 2.0 ** -24
MARGIN = 1e-4
DATASET_BOUND = float(np.float32(1e10))    # max_bound = invalid of the dataset build
DATASET_EPS = float(np.float32(1e-6))
SENT = -777.25                             # float sentinel; ISENT its int32 counterpart
ISENT = -0x35014542

# rays_ndc: largest |float32 oracle - float64| per column over all NDC_CASES, divided by the column's max |ref|, as
# measured by test_rays_reference.py::test_ndc_tolerance_is_measured (it asserts the measurement stays at or under
# these).  The GPU tolerance of a column is max(4 * this, 4 * 2^-24) * max |ref|; columns 6 and 7 are exact.
NDC_REL_ERR = (4.2e-7, 4.8e-7, 9.6e-7, 4.0e-7, 4.0e-7, 4.8e-7)


# ------------------------------------------------------------------------------------------------ pick_pixels

def mix64(z):
    """nerf_mix64: splitmix64's finaliser."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def pick_seed(seed, step=None, seed_mul=0):
    """(seed + step * seed_mul) mod 2^64; a negative step counts as its uint64 bit pattern."""
    if step is not None:
        seed = seed + (step & M64) * seed_mul
    return seed & M64


def pick_one(p, seed, n_images, H, W):
    z = mix64(seed * GOLDEN + mix64(p + PIX_STREAM))
    k = (z * (n_images * H * W)) >> 64
    hw = H * W
    return k // hw, (k % hw) // W, k % W


def pick_pixels(n, n_images, H, W, seed, step=None, seed_mul=0):
    s = pick_seed(seed, step, seed_mul)
    return np.array([pick_one(p, s, n_images, H, W) for p in range(n)], dtype=np.int32).reshape(n, 3)


# ------------------------------------------------------------------------------------------------ rays

def ray_dirs(H, W, fx, fy, cx, cy, center, c2w, rows, cols):
    """Origin and rotated unit direction (float64) of pixels (rows, cols); c2w (3,4), or (n,3,4) one pose per pixel.
    The intrinsics are taken as the float32 numbers the C entry point receives."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
    M = np.asarray(c2w, dtype=np.float64)
    i = np.asarray(cols, dtype=np.float64) + (0.5 if center else 0.0)
    j = np.asarray(rows, dtype=np.float64) + (0.5 if center else 0.0)
    v = np.stack([(i - cx) / fx, -(j - cy) / fy, -np.ones_like(i)], -1)
    v = v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-12)
    M = np.broadcast_to(M, v.shape[:-1] + (3, 4))
    d = np.einsum("nrc,nc->nr", M[:, :, :3], v)
    return M[:, :, 3].copy(), d


def aabb_near_far(o, d, aabb, max_bound, invalid, with_tmax=False):
    """float64 slab test -> (near, far, gap); gap as in the module docstring (> 0 iff valid).  A NaN anywhere in a
    ray gives near = far = NaN (torch's amax / clamp propagate it) and gap = NaN.  with_tmax adds the clamped tmax
    before the invalid rewrite, the scale of the decision margin."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    box = np.asarray(aabb, dtype=np.float64).reshape(2, 3)
    max_bound = float(np.float32(max_bound))
    with np.errstate(invalid="ignore", over="ignore"):
        rd = np.where(np.abs(d) < EPS_DIR, np.where(d >= 0, EPS_DIR, -EPS_DIR), d)
        inv = 1.0 / rd
        t0, t1 = (box[0] - o) * inv, (box[1] - o) * inv
        tmin, tmax = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)      # numpy's propagate NaN too
        slack = np.minimum(np.minimum(tmax - tmin, tmax), max_bound - tmin)
        near, far = np.clip(tmin, 0.0, max_bound), np.clip(tmax, 0.0, max_bound)
        bad = far <= near
    nan = np.isnan(tmin) | np.isnan(tmax)
    assert np.array_equal(bad | nan, ~(slack > 0))
    iv = float(np.float32(invalid))
    out = np.where(bad, iv, near), np.where(bad, iv, far), np.where(nan, np.nan, slack)
    return out + (np.where(nan, 1.0, far),) if with_tmax else out


def in_margin(gap, scale):
    """True where a decision is too close to call: |gap| <= MARGIN * max(1, |scale|).  NaN gaps are decided."""
    with np.errstate(invalid="ignore"):
        return np.abs(gap) <= MARGIN * np.maximum(1.0, np.abs(scale))


def clamp_near_far(near, far, has_near, nv, has_far, fv, eps, invalid):
    """numpy float32, op for op -> (near, far, valid).  np.maximum / np.minimum propagate NaN, as torch's do."""
    f = np.float32
    a, b = np.asarray(near, dtype=f).copy(), np.asarray(far, dtype=f).copy()
    with np.errstate(invalid="ignore"):
        if has_near:
            a = np.maximum(a, f(nv))
        if has_far:
            b = np.minimum(b, f(fv))
        ok = np.isfinite(a) & np.isfinite(b) & (b > a + f(eps))
    if has_near or has_far:
        a, b = np.where(ok, a, f(invalid)), np.where(ok, b, f(invalid))
    return a.astype(f), b.astype(f), ok


def ndc(rays, H, W, focal, near_plane):
    r = np.asarray(rays, dtype=np.float64)
    focal, near_plane = float(np.float32(focal)), float(np.float32(near_plane))
    o, d = r[:, :3], r[:, 3:6]
    t = -(near_plane + o[:, 2]) / d[:, 2]
    o = o + t[:, None] * d
    ax, ay = -1.0 / (W / (2.0 * focal)), -1.0 / (H / (2.0 * focal))
    z = np.zeros(len(r))
    return np.stack([ax * o[:, 0] / o[:, 2], ay * o[:, 1] / o[:, 2], 1.0 + 2.0 * near_plane / o[:, 2],
                     ax * (d[:, 0] / d[:, 2] - o[:, 0] / o[:, 2]), ay * (d[:, 1] / d[:, 2] - o[:, 1] / o[:, 2]),
                     -2.0 * near_plane / o[:, 2], z, z + 1.0], -1)


def exclusive_scan(x):
    return np.concatenate([[0], np.cumsum(np.asarray(x, dtype=np.int64))]).astype(np.int32)


def dataset_rows(c2w, intr, image_index, H, W, center, aabb, has_near, nv, has_far, fv, images, masks):
    """The dataset build of a run, pixel by pixel in order.  Returns a dict: flags (n), pos (n + 1), rays (kept, 8)
    float64, rgb (kept, 3) float32, idx (kept), bounds (n_images + 1), and per pixel hit_gap (the slab test's signed
    gap, its scale hit_scale) and keep_gap (far - near - eps after the override, its scale keep_scale).  keep_gap is
    +-inf where the decision is not a comparison of computed numbers: masked pixels, NaN rays, and rays the slab test
    rejected (near = far = 1e10 bit for bit, or 1e10 against the override: hit_gap is their margin)."""
    c2w = np.asarray(c2w, dtype=np.float32).reshape(-1, 3, 4)
    intr = np.asarray(intr, dtype=np.float32).reshape(-1, 4)
    n_img, hw = len(c2w), H * W
    n = n_img * hw
    g = np.arange(n)
    im, q = g // hw, g % hw
    rows, cols = q // W, q % W
    o = np.empty((n, 3))
    d = np.empty((n, 3))
    for k in range(n_img):
        s = slice(k * hw, (k + 1) * hw)
        o[s], d[s] = ray_dirs(H, W, *intr[k], center, c2w[k], rows[s], cols[s])
    near, far, hit_gap, hit_scale = aabb_near_far(o, d, aabb, DATASET_BOUND, DATASET_BOUND, with_tmax=True)
    a, b = near.copy(), far.copy()
    if has_near:
        a = np.maximum(a, float(np.float32(nv)))
    if has_far:
        b = np.minimum(b, float(np.float32(fv)))
    with np.errstate(invalid="ignore"):
        keep_gap = b - a - DATASET_EPS
        ok = np.isfinite(a) & np.isfinite(b) & (keep_gap > 0)
    unmasked = np.ones(n, dtype=bool) if masks is None else np.asarray(masks).reshape(n) != 0
    flags = (ok & unmasked).astype(np.int32)
    undecidable = ~unmasked | np.isnan(keep_gap) | ~(hit_gap > 0)
    keep_gap = np.where(undecidable, np.where(flags == 1, np.inf, -np.inf), keep_gap)
    if has_near or has_far:
        a, b = np.where(ok, a, np.inf), np.where(ok, b, np.inf)
    pos = exclusive_scan(flags)
    kept = flags == 1
    px = np.asarray(images, dtype=np.uint8).reshape(n, 3)[kept]
    return dict(flags=flags, pos=pos, kept_pixels=np.stack([im, rows, cols], -1)[kept].astype(np.int32),
                rays=np.concatenate([o, d, a[:, None], b[:, None]], -1)[kept],
                rgb=px.astype(np.float32) / np.float32(255), idx=np.asarray(image_index, dtype=np.int32)[im[kept]],
                bounds=pos[::hw].copy(), hit_gap=hit_gap, hit_scale=hit_scale, keep_gap=keep_gap,
                keep_scale=np.where(np.isfinite(b), b, 1.0))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ================================================================================================= inputs

def rotation(axis, angle):
    """Rodrigues' rotation, rounded to float32: a generic orthonormal matrix (to 2^-24)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(np.float32)


def look_at(eye, target, roll=0.0):
    """c2w (3,4) float32 of a camera at eye whose -z axis points at target."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = eye - target
    z /= np.linalg.norm(z)
    up = np.array([np.sin(roll) * 0.3, 0.2, 1.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], 1), eye[:, None]], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ pick_pixels

PICK_N = (1, 255, 256, 257)
PICK_SHAPES = ((1, 1, 1), (3, 7, 5), (2, 1, 300), (3, 40000, 40000))
PICK_SEEDS = (0, 1, 1 << 63, M64)
PICK_STEPS = (0, 1, 1 << 40, -1)
PICK_MULS = (1, GOLDEN)
PICK_BASE_SEED = 0x1234567890ABCDEF

# ------------------------------------------------------------------------------------------------ rays_gen

DENSE_SHAPES = ((1, 1), (1, 257), (7, 37), (16, 16))
DENSE_NEAR_FAR = (0.1, 7.5)                    # 0.1 is not a float32: the kernel must hand back float32(0.1)
BATCH_N = (1, 255, 257)
BATCH_HW = (5, 7)


def dense_camera(H, W):
    """Non-square intrinsics, off-centre principal point, three generic poses (the dense path uses pose 0)."""
    K = (1.75 * W + 0.375, 1.25 * W + 2.5, 0.5 * W + 1.75, 0.5 * H - 0.625)
    poses = np.stack([np.concatenate([rotation(ax, an), np.array(t, dtype=np.float32)[:, None]], 1)
                      for ax, an, t in (((1, 2, 3), 0.7, (0.3, -1.2, 2.5)), ((-2, 1, 0.5), 2.1, (4, 5, 6)),
                                        ((0, 1, -1), -1.3, (-7, 8, -9)))]).astype(np.float32)
    return K, poses


def batch_case(n):
    """-> list of (pix (n,3), images (3,5,7,3) uint8): pixel triples of three 5x7 images, holding (0,0,0) and the last
    pixel of the last image (n = 1: one batch for each)."""
    H, W = BATCH_HW
    images = np.random.RandomState(11).randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    first, last = (0, 0, 0), (2, H - 1, W - 1)
    if n == 1:
        return [(np.array([first], dtype=np.int32), images), (np.array([last], dtype=np.int32), images)]
    pix = pick_pixels(n, 3, H, W, 77 + n)
    pix[0], pix[-1] = last, first
    return [(pix, images)]


# ------------------------------------------------------------------------------------------------ AABB, generic

AABB_BOX = (-1.0, -1.5, -0.75, 1.0, 1.25, 1.5)
AABB_N = 257
AABB_HW = (16, 16)
AABB_K = (9.0, 11.0, 8.25, 7.5)                # wide enough that the camera outside sees past the box
AABB_BOUNDS = ((1e10, 1e10), (1.0, -1.0), (3.0, 0.0))      # (max_bound, invalid)
AABB_SEED = 5


def aabb_case():
    """-> (poses (3,3,4), pix (257,3)): a camera inside the box, one outside looking in, one outside looking away."""
    eye = (3.0, 0.6, 0.3)
    poses = np.stack([np.concatenate([rotation((1, -1, 2), 0.9), np.array([[0.2], [-0.3], [0.1]], np.float32)], 1),
                      look_at(eye, (0.1, 0.0, 0.2), 0.4),
                      look_at(eye, (5.9, 1.2, 0.4), 0.4)])
    return poses, pick_pixels(AABB_N, 3, *AABB_HW, AABB_SEED)


# ------------------------------------------------------------------------------------------------ AABB, exact

EXACT_BOX = (-1.0, -2.0, -4.0, 1.0, 2.0, 4.0)
BIG = float(np.float32(1e10))
# (name, direction axis, sign, origin, max_bound, invalid, near, far): a 1x1 image with the principal point on the
# pixel centre looks exactly along -z of the camera; the pose is a signed permutation, so d = sign * e_axis and, with
# origins and box at powers of two, every fp32 operation that reaches near / far is exact.
AABB_EXACT = (
    ("inside", 0, +1, (0.5, 0.25, -1.0), BIG, BIG, 0.0, 0.5),
    ("inside, -y", 1, -1, (0.5, 0.25, -1.0), BIG, BIG, 0.0, 2.25),
    ("ahead", 0, +1, (-3.0, 0.5, 1.0), BIG, BIG, 2.0, 4.0),
    ("on the entry face", 0, +1, (-1.0, 0.5, 1.0), BIG, BIG, 0.0, 2.0),
    ("on the exit face, leaving: tmax == tmin == 0", 0, +1, (1.0, 0.5, 1.0), BIG, BIG, BIG, BIG),
    ("on the entry face, leaving", 0, -1, (-1.0, 0.5, 1.0), BIG, -1.0, -1.0, -1.0),
    ("parallel and inside, far cut by max_bound", 2, +1, (0.0, 1.0, 0.0), 2.0, BIG, 0.0, 2.0),
    ("parallel and inside, both cut by max_bound", 2, +1, (0.0, 1.0, -8.0), 2.0, -1.0, -1.0, -1.0),
    ("parallel and inside, near under max_bound", 2, +1, (0.0, 1.0, -8.0), 8.0, -1.0, 4.0, 8.0),
    ("parallel and outside, above", 0, +1, (0.0, 4.0, 0.0), BIG, BIG, BIG, BIG),
    ("parallel and outside, below", 0, +1, (0.0, -4.0, 0.0), BIG, 0.0, 0.0, 0.0),
    ("along an upper edge from its corner: tmax == tmin == 0", 0, +1, (-1.0, 2.0, 4.0), BIG, BIG, BIG, BIG),
    ("along an upper edge, from outside", 0, +1, (-4.0, 2.0, 4.0), BIG, BIG, BIG, BIG),
    ("along a lower edge: the eps replacement keeps it", 0, +1, (-4.0, -2.0, -4.0), BIG, BIG, 3.0, 5.0),
    ("box behind", 0, +1, (4.0, 0.0, 0.0), BIG, BIG, BIG, BIG),
    ("box behind, -z", 2, -1, (0.0, 0.0, -16.0), BIG, -1.0, -1.0, -1.0),
)


def exact_pose(axis, sign, origin):
    """c2w (3,4) whose third column is -sign * e_axis; row (axis + 1) % 3 is (-1, 0, 0), which makes that component
    of d the sum of three -0.0 products: a -0.0 direction component."""
    M = np.zeros((3, 4), dtype=np.float32)
    M[axis, 2] = -sign
    M[(axis + 1) % 3, 0] = -1.0
    M[(axis + 2) % 3, 1] = 1.0
    M[:, 3] = origin
    return M


def exact_dir(axis, sign):
    """The direction the kernel's arithmetic gives for exact_pose, signed zeros included."""
    d = np.zeros(3, dtype=np.float32)
    d[axis] = sign
    d[(axis + 1) % 3] = -0.0
    return d


def slab_fp32(o, d, aabb, max_bound, invalid):
    """aabb_slab in float32, step by step (one ray)."""
    f = np.float32
    o, d, box = np.asarray(o, f), np.asarray(d, f), np.asarray(aabb, f).reshape(2, 3)
    eps = f(1e-8)
    rd = np.where(np.abs(d) < eps, np.where(d >= 0, eps, -eps), d).astype(f)
    inv = (f(1) / rd).astype(f)
    t0, t1 = ((box[0] - o).astype(f) * inv).astype(f), ((box[1] - o).astype(f) * inv).astype(f)
    tmin = np.clip(np.minimum(t0, t1).max(), f(0), f(max_bound))
    tmax = np.clip(np.maximum(t0, t1).min(), f(0), f(max_bound))
    if tmax <= tmin:
        return f(invalid), f(invalid)
    return f(tmin), f(tmax)


# ------------------------------------------------------------------------------------------------ clamp_near_far

CLAMP_N = (1, 255, 257)
CLAMP_EPS = 1e-6
CLAMP_INVALID = (float("inf"), 0.0, -1.0)
NINF = float("-inf")
# (has_near, near_v, has_far, far_v); -inf as near is the dataset's (None, None)
CLAMP_OVERRIDES = ((0, 0.0, 0, 0.0), (1, 0.5, 0, 0.0), (0, 0.0, 1, 4.0), (1, 0.5, 1, 4.0), (1, NINF, 0, 0.0),
                   (1, NINF, 1, 4.0))


def clamp_specials():
    """(near, far) rows at the edges of the decision; all of them at or above near_v = 0.5 where that matters."""
    f = np.float32
    inf, nan = f("inf"), f("nan")
    e = f(1.0) + f(CLAMP_EPS)                                   # fl(1 + eps)
    rows = [(nan, 2.0), (1.0, nan), (nan, nan),                 # NaN in near, in far, in both (row 0 serves n = 1)
            (1.0, e), (1.0, np.nextafter(e, f(0))), (1.0, np.nextafter(e, f(9))),
            (16.0, np.nextafter(f(16), f(99))), (32.0, 32.0), (32.0, np.nextafter(f(32), f(99))),
            (2.0 ** 20, 2.0 ** 20 + 0.125),
            (-inf, 2.0), (1.0, inf), (inf, inf), (-inf, inf), (inf, -inf), (1.0, -inf), (-inf, -inf),
            (0.25, 0.5), (0.25, np.nextafter(f(0.5) + f(CLAMP_EPS), f(9))), (3.0, 5.0), (4.0, 4.5),
            (3.9999995, 8.0), (0.0, 0.0), (2.0, 1.0), (1e10, 1e10)]
    return np.array(rows, dtype=f)


def clamp_rays(n):
    """(n,8) float32: random rays; the special rows stand first and again at the end (across the 256-thread block
    boundary when n = 257)."""
    rs = np.random.RandomState(100 + n)
    rays = rs.randn(n, 8).astype(np.float32)
    rays[:, 6] = rs.rand(n) * 5
    rays[:, 7] = rays[:, 6] + rs.rand(n) * 3 - 0.5              # some far < near
    sp = clamp_specials()
    k = min(n, len(sp))
    rays[:k, 6:] = sp[:k]
    if n > 2 * len(sp):
        rays[n - len(sp):, 6:] = sp
    return rays


# ------------------------------------------------------------------------------------------------ rays_ndc

NDC_N = (1, 255, 257)
NDC_CONFIGS = ((756, 1008, 815.0, 1.0), (5, 9, 3.5, 0.25))     # H, W, focal, near_plane
NDC_CASES = tuple((n, c) for c in range(len(NDC_CONFIGS)) for n in NDC_N)


def ndc_rays_input(n, c):
    """(n,8) float32: unit directions down -z (even rows) and +z (odd rows) with |d_z| >= 0.3, origins with
    |o_z| <= 8 near_plane; every fifth origin lies on the near plane (t = 0)."""
    near_plane = NDC_CONFIGS[c][3]
    rs = np.random.RandomState(1000 * c + n)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, :2] = rs.randn(n, 2) * 2 * near_plane
    rays[:, 2] = (rs.rand(n) * 16 - 8) * near_plane
    rays[::5, 2] = -near_plane
    d = rs.randn(n, 3) * 0.5
    d[:, 2] = (0.6 + rs.rand(n)) * np.where(np.arange(n) % 2 == 0, -1, 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3:6] = d
    rays[:, 6:] = rs.rand(n, 2)
    assert (np.abs(rays[:, 2]) <= 8 * near_plane).all() and (np.abs(rays[:, 5]) >= 0.3).all()
    return rays


def ndc_tolerance(ref):
    """Per-column absolute tolerance (6) for a float64 reference block."""
    scale = np.abs(ref[:, :6]).max(0)
    return np.maximum(4.0 * np.array(NDC_REL_ERR), T_TOL) * scale


# ------------------------------------------------------------------------------------------------ dataset build

DS_HW = (5, 7)
DS_BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
DS_OVERRIDES = (None, (0.5, 4.0), (None, 4.0), (0.5, None), (None, None))
DS_DISTANCES = (2.5, 0.3, 5.5, 2.0, 3.25, 1.5)     # camera distances: 0.3 is inside the box, 5.5 beyond far = 4
DS_SEED = 10


def override_args(override):
    """nerf_amd.data._override_args restated: (has_near, near_v, has_far, far_v)."""
    if override is None:
        return 0, 0.0, 0, 0.0
    no, fo = override
    return 1, (NINF if no is None else float(no)), (0 if fo is None else 1), (0.0 if fo is None else float(fo))


def _dataset_layout(n_images, layout):
    """Which images are fully masked, miss the box, or carry a NaN pose."""
    if n_images == 1 or layout == "plain":
        return dict(masked=[], miss=[], nan_t=[], nan_r=[])
    last, mid = n_images - 1, n_images // 2
    if layout == "A":
        return dict(masked=[0], miss=[last], nan_t=[2], nan_r=[5])
    return dict(masked=[mid, last], miss=[0], nan_t=[], nan_r=[3])


def dataset_case(n_images, layout="plain", center=True, override=None, shared_intrinsics=False, keep="random"):
    """A run of n_images 5x7 images around DS_BOX: per-image poses (distances cycle through DS_DISTANCES) and
    intrinsics, descending non-contiguous image ids, random masks.  keep = "last_pixel" masks everything but the last
    pixel of the last image (whose camera stands inside the box), keep = "nothing" masks everything."""
    H, W = DS_HW
    rs = np.random.RandomState(DS_SEED + 17 * n_images + (0 if layout == "plain" else ord(layout)))
    lay = _dataset_layout(n_images, layout)
    c2w, intr = [], []
    for i in range(n_images):
        dist = DS_DISTANCES[i % len(DS_DISTANCES)]
        if keep == "last_pixel" and i == n_images - 1:
            dist = 0.3
        v = rs.randn(3)
        eye = dist * v / np.linalg.norm(v)
        M = look_at(eye, rs.randn(3) * 0.15, rs.rand())
        if i in lay["miss"]:
            M = look_at(eye + 40.0, eye + 80.0, 0.1)            # far away, looking further away
        if i in lay["nan_t"]:
            M[0, 3] = np.nan
        if i in lay["nan_r"]:
            M[1, 1] = np.nan
        c2w.append(M)
        k = 0 if shared_intrinsics else i
        intr.append((4.0 + 0.25 * (k % 5), 3.5 + 0.125 * (k % 7), 3.5 + 0.1 * (k % 3), 2.5 - 0.05 * (k % 4)))
    images = rs.randint(0, 256, (n_images, H, W, 3)).astype(np.uint8)
    masks = (rs.rand(n_images, H, W) < 0.85).astype(np.uint8)
    for i in lay["masked"]:
        masks[i] = 0
    if keep != "random":
        masks[:] = 0
    if keep == "last_pixel":
        masks[-1, -1, -1] = 1
    return dict(n_images=n_images, H=H, W=W, center=bool(center), override=override, aabb=DS_BOX, layout=lay,
                c2w=np.stack(c2w).astype(np.float32), intr=np.array(intr, dtype=np.float32),
                image_index=(100 - 3 * np.arange(n_images)).astype(np.int32), images=images, masks=masks, keep=keep)


def _dataset_case_list():
    out = []
    for n_images, layouts in ((1, ("plain",)), (8, ("A", "B")), (59, ("A", "B"))):
        for li, layout in enumerate(layouts):
            for oi, override in enumerate(DS_OVERRIDES):
                out.append(dict(n_images=n_images, layout=layout, center=(oi + li) % 2 == 0, override=override))
    out.append(dict(n_images=8, layout="plain", center=True, override=(0.5, 4.0), keep="last_pixel"))
    out.append(dict(n_images=8, layout="plain", center=False, override=None, keep="nothing"))
    out.append(dict(n_images=8, layout="plain", center=True, override=None, shared_intrinsics=True))
    out.append(dict(n_images=8, layout="plain", center=False, override=(0.5, 4.0), shared_intrinsics=True))
    out.append(dict(n_images=8, layout="plain", center=True, override=(None, None), shared_intrinsics=True))
    return out


DATASET_CASES = _dataset_case_list()
_expected = {}


def dataset_expected(i):
    """(case, dataset_rows of it), computed once and shared; callers must not modify it."""
    if i not in _expected:
        case = dataset_case(**DATASET_CASES[i])
        hn, nv, hf, fv = override_args(case["override"])
        _expected[i] = (case, dataset_rows(case["c2w"], case["intr"], case["image_index"], case["H"], case["W"],
                                           case["center"], case["aabb"], hn, nv, hf, fv, case["images"],
                                           case["masks"]))
    return _expected[i]
