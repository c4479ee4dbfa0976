"""The generic (plan-driven) fused Instant-NGP MLP kernels of csrc/ngp.hip -- ngp_fwd_kernel, ngp_density_kernel,
ngp_bwd_kernel<4|6|8>, ngp_wt_kernel, ngp_reduce_kernel<true|false> -- across widths, depths and weight-gradient
slot counts, against the float64 reference of tests/ngp_mlp_reference.py.  Run on an MI355X: -m gpu.

The tests call the low-level wrappers (ngp_fwd, ngp_density, ngp_bwd, ngp_workspace) with a raw NerfNgpNet and an
NgpLayout built from ngp_param_shapes, so in_dim and sh_levels are free of any hash grid.  Every case that claims a
path (ngp_bwd_kernel<8>, bsum < 0, 12 layers, not the production kernels) asserts it through plan_reference before
the kernel runs.  ReLU kinks are removed on the reference side only (draw_case keeps the first M of 2 M candidate
rows whose float64 pre-activations all have |z| >= 1e-4, and fails when fewer than M survive); no row is dropped
after looking at kernel output.

Bounds (those of test_ngp_production_backward_kernel): forward within 2e-5 * max(1, |ref|inf) of float64, every
gradient tensor within 1e-5 * max(1, |ref|inf).  A plain fp32 CPU evaluation of the same reference sits at <= 1e-7
(forward) and <= 1.1e-6 (gradients) of float64 on these cases.

Worst errors observed on an MI355X, as a fraction of the bound's scale max(1, |ref|inf):
  forward (25 cases)                 1.1e-7 of 2e-5  (wide_in, M = 31); density bitwise the forward's sigma
  backward (25 cases)                1.8e-6 of 1e-5  (nsb8_in64, sigma_head.bias)
  tile loop, M = 16417 (256 CUs)     forward 8.9e-8; gradients 5.1e-6 of 1e-5 (twelve, sigma_head.weight; the fp32
                                     CPU evaluation of that case is 1.8e-5 from float64, nsb8 1.4e-6, mix 6.2e-7)
  pads and poison                    pads exactly 0; gradients 4.2e-7 (bitwise the unpoisoned call's)
  direction edges                    forward 6.6e-8, gradients 2.5e-7
  saturated head +100                sigma 5.9e-8 relative of 1e-5 (FLT_MAX against the exact FLT_MAX (1 + 5.9e-8));
                                     gradients 2.4e-7.  Before ngp_trunc_exp capped the overflow: sigma = +inf
  saturated head -100                sigma 2.0e-48 absolute of 1e-37
  module level                       forward 1.2e-7, gradients 1.3e-6 (wide_in, sigma_trunk.0.linear.weight)
"""
import ctypes
import functools
import math

import pytest
import torch

from oracle import ngp_oracle as NO
import ngp_mlp_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL, GRAD_TOL = 2e-5, 1e-5
EDGE_M = (1, 31, 32, 33, 63, 64, 65)   # around the forward's 64-row and the backward's 32-row tiles
LINEAR_RGB = ("nodepth", "wide_in", "nsb8")   # ids that also run with use_sigmoid_rgb = 0
CASES = ([(t, 97, True) for t in R.CONFIGS if t != "prod"] + [(t, 97, False) for t in LINEAR_RGB]
         + [("wide_in", m, True) for m in EDGE_M])
CASE_IDS = [f"{t}-{m}-{'sigmoid' if s else 'linear'}" for t, m, s in CASES]


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import ngp
    return ngp


def _net(N, cfg, sigmoid=True, generic=0):
    net = N.NerfNgpNet()
    net.in_dim, net.hidden, net.sigma_depth, net.geo_feat_dim = cfg.in_dim, cfg.hidden, cfg.sigma_depth, cfg.geo
    net.color_hidden, net.color_depth, net.dir_encoding, net.sh_levels = (cfg.color_hidden, cfg.color_depth,
                                                                          cfg.dir_mode, cfg.sh_levels)
    net.use_sigmoid_rgb, net.generic_kernels = int(sigmoid), int(generic)
    return net


def _layout(N, cfg, net):
    shapes = NO.ngp_param_shapes(cfg.in_dim, cfg.hidden, cfg.sigma_depth, cfg.geo, cfg.color_hidden, cfg.color_depth,
                                 R.config_dir_dim(cfg))
    return N.NgpLayout(net, shapes, cfg.sigma_depth, cfg.color_depth), shapes


@functools.lru_cache(maxsize=None)
def _case(tag, M, sigmoid=True, **kw):
    """The seeded inputs and the float64 reference of one case, computed once and shared (never modified)."""
    seed = 1000 * list(R.CONFIGS).index(tag) + M % 997 + (0 if sigmoid else 500)
    return R.draw_case(R.CONFIGS[tag], M, seed, sigmoid=sigmoid, **kw)


def _assert_path(tag):
    """The configuration reaches the path its id claims (layers, ngp_bwd_kernel<NSB>, bsum sign), by the Python
    restatement of make_plan -- asserted before any kernel runs."""
    p = R.config_plan(R.CONFIGS[tag])
    assert p is not None and (len(p.layers), p.nsb, p.bsum < 0) == R.EXPECTED_PATH[tag], tag
    return p


class _Gpu:
    """A case on the device: the raw net, its layout, the packed weights and the inputs."""

    def __init__(self, N, cs, generic=0):
        self.N, self.cs = N, cs
        self.net = _net(N, cs.cfg, cs.sigmoid, generic)
        self.layout, self.shapes = _layout(N, cs.cfg, self.net)
        self.w = self.layout.pack_raw([cs.named[n].to(DEV) for n in self.layout.names])
        self.enc, self.x_d, self.gup = cs.enc.to(DEV), cs.x_d.to(DEV), cs.gup.to(DEV)

    def fwd(self, enc=None):
        return self.N.ngp_fwd(self.net, self.w, self.enc if enc is None else enc, self.x_d)

    def density(self, enc=None):
        return self.N.ngp_density(self.net, self.w, self.enc if enc is None else enc)

    def bwd(self, **kw):
        enc = kw.pop("enc", self.enc)
        return self.N.ngp_bwd(self.net, self.w, enc, self.x_d, self.gup, **kw)

    def named_grads(self, d_w):
        flat = d_w.index_select(0, self.layout.device_index(d_w.device)).cpu()
        out, o = {}, 0
        for n in self.layout.names:
            k = int(torch.Size(self.shapes[n]).numel())
            out[n] = flat[o:o + k].view(self.shapes[n])
            o += k
        return out

    def pad_mask(self):
        m = torch.ones(self.layout.total, dtype=torch.bool)
        m[self.layout.index] = False
        return m


def _rel(got, ref):
    """max |got - ref| / max(1, |ref|inf) -- the error in units of the bounds' scale"""
    if ref.numel() == 0:
        assert got.numel() == 0
        return 0.0
    return float((got.detach().double().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def _check_fwd(what, out, cs):
    assert out.shape == cs.out.shape
    e = _rel(out, cs.out)
    print(f"[ngp-edges] {what} forward {e:.2e} (bound {FWD_TOL:.0e})")
    assert e <= FWD_TOL, f"{what}: forward {e:.3e}"
    return e


def _check_grads(what, g, d_enc, d_w, cs):
    in_dim = cs.cfg.in_dim
    worst = ("d_enc", _rel(d_enc[:, :in_dim], cs.d_enc))
    got = g.named_grads(d_w)
    errs = {n: _rel(got[n], cs.grads[n]) for n in g.layout.names}
    errs["d_enc"] = worst[1]
    name = max(errs, key=errs.get)
    print(f"[ngp-edges] {what} gradients {errs[name]:.2e} at {name} (bound {GRAD_TOL:.0e})")
    bad = {n: e for n, e in errs.items() if not e <= GRAD_TOL}
    assert not bad, f"{what}: {bad}"
    return errs[name]


# ------------------------------------------------------------------------------------------ 1. layout

@pytest.mark.parametrize("tag", list(R.CONFIGS))
def test_layout_equals_plan_reference(N, tag):
    cfg = R.CONFIGS[tag]
    p = _assert_path(tag)
    net = _net(N, cfg)
    layout, shapes = _layout(N, cfg, net)
    assert layout.total == p.total
    want = []
    for L in p.layers:
        want += [(L.w_off, L.Npad, L.Kpad), (L.b_off, L.Npad, 1)]
    assert [tuple(int(v) for v in t) for t in layout.tensors_table] == want
    # the named tensors' positions are distinct and inside their layers' live (N x K) corners
    idx = layout.index
    assert idx.numel() == sum(L.K * L.N + L.N for L in p.layers) == idx.unique().numel()
    live = torch.zeros(p.total, dtype=torch.bool)
    for L in p.layers:
        rows = torch.arange(L.N).view(-1, 1) * L.Kpad + torch.arange(L.K).view(1, -1)
        live[L.w_off + rows.reshape(-1)] = True
        live[L.b_off:L.b_off + L.N] = True
    assert bool(live[idx].all()) and int(live.sum()) == idx.numel()
    assert layout.color_start == p.layers[p.head + 1].w_off
    bytes_ = int(N.lib().nerf_ngp_workspace_bytes(ctypes.c_void_p(ctypes.addressof(net)), 1))
    assert bytes_ == 2 * p.total * 4 + 256   # one workgroup's slab + the W^T image


# ------------------------------------------------------------------------------------------ 2. forward

@pytest.mark.parametrize("tag,M,sigmoid", CASES, ids=CASE_IDS)
def test_forward_vs_fp64(N, tag, M, sigmoid):
    _assert_path(tag)
    cs = _case(tag, M, sigmoid)
    g = _Gpu(N, cs)
    out = g.fwd()
    sig = g.density()
    torch.cuda.synchronize()
    _check_fwd(f"{tag} M={M} sigmoid={int(sigmoid)}", out, cs)
    # the density kernel runs the same trunk code: bitwise the forward's sigma
    assert torch.equal(sig, out[:, 3])
    if tag.startswith("near_"):
        # one field away from the production shape: the generic kernels must serve it, so forcing them
        # (generic_kernels = 1) changes nothing
        g1 = _Gpu(N, cs, generic=1)
        assert torch.equal(g1.fwd(), out) and torch.equal(g1.density(), sig)


@pytest.mark.parametrize("tag", ["near_sh3", "near_geo14", "prod"])
def test_one_launch_entry_points_only_for_production(N, tag):
    """The fused encode + MLP entry points answer NERF_E_UNSUPPORTED (before they look at a buffer) for the shapes
    next to production whose packed layout equals production's, and NERF_OK for production itself."""
    cfg = R.CONFIGS[tag]
    p, prod = _assert_path(tag), R.config_plan(R.CONFIGS["prod"])
    assert p.total == prod.total and [L[2:] for L in p.layers] == [L[2:] for L in prod.layers]
    net = _net(N, cfg)
    grid = N.NerfHashGrid()
    grid.levels, grid.features_per_level, grid.log2_hashmap_size, grid.interpolation = 16, 2, 8, 1
    for i in range(16):
        grid.resolutions[i] = 4 + i
    L, a = N.lib(), lambda s: ctypes.c_void_p(ctypes.addressof(s))
    st = N.stream()
    rcs = (L.nerf_ngp_fwd_enc(a(net), a(grid), None, None, None, 0, None, 0.0, None, 32, None, st),
           L.nerf_ngp_density_enc(a(net), a(grid), None, None, None, 3, 0, None, 0.0, None, st),
           L.nerf_ngp_bwd_hash(a(net), a(grid), None, None, 32, None, 0, None, None, 0.0, None, ctypes.c_void_p(16), 1,
                               None, 0, st))
    assert rcs == ((0, 0, 0) if tag == "prod" else (N.E_UNSUPPORTED,) * 3)


# ------------------------------------------------------------------------------------------ 3. backward

@pytest.mark.parametrize("tag,M,sigmoid", CASES, ids=CASE_IDS)
def test_backward_vs_fp64(N, tag, M, sigmoid):
    _assert_path(tag)
    cs = _case(tag, M, sigmoid)
    g = _Gpu(N, cs)
    d_enc, d_w = g.bwd()
    torch.cuda.synchronize()
    _check_grads(f"{tag} M={M} sigmoid={int(sigmoid)}", g, d_enc, d_w, cs)
    assert bool((d_w.cpu()[g.pad_mask()] == 0).all()), "non-zero gradient at a pad position"
    if tag.startswith("near_"):
        d_enc1, d_w1 = _Gpu(N, cs, generic=1).bwd()
        assert torch.equal(d_enc1, d_enc) and torch.equal(d_w1, d_w)


# ------------------------------------------------------------------------------------------ 4. tile loop

@pytest.mark.parametrize("tag", ["nsb8", "twelve", "mix"])
def test_backward_tile_loop(N, tag):
    """M = 32 (2 CU) + 33 rows: 2 CU workgroups, of which the first visit two tiles, the rest one, and the last tile
    holds one row -- the smallest M at which accw, bacc and bsum accumulate across tiles."""
    p = _assert_path(tag)
    if tag == "nsb8":
        assert p.nsb == 8 and p.bsum < 0 and p.slots_per_wave == 7
    if tag == "twelve":
        assert len(p.layers) == 12 and p.bsum < 0   # layers 8..11 -> bacc[2]
    if tag == "mix":
        assert p.bsum >= 0
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    M = 32 * (2 * cu) + 33
    assert 2 * cu < math.ceil(M / 32) < 4 * cu and M % 32 == 1
    cs = _case(tag, M)
    g = _Gpu(N, cs)
    out = g.fwd()
    d_enc, d_w = g.bwd()
    d_enc2, d_w2 = g.bwd()
    torch.cuda.synchronize()
    _check_fwd(f"{tag} tile loop M={M}", out, cs)
    _check_grads(f"{tag} tile loop M={M}", g, d_enc, d_w, cs)
    assert torch.equal(d_w, d_w2) and torch.equal(d_enc, d_enc2)   # slabs + ordered reduce: deterministic
    assert bool((d_w.cpu()[g.pad_mask()] == 0).all())


# ------------------------------------------------------------------------------------------ 5. pads and poison

@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("tag", ["nodepth", "wide_in", "nsb8", "prod"])
def test_pads_zero_and_poison_ignored(N, tag, generic):
    """Adam runs over the whole packed buffer, so a pad gradient must be exactly 0; the slabs and d_w are
    write-only outputs (every packed float written once), enc columns past in_dim are never read and d_enc columns
    past in_dim never written."""
    _assert_path(tag)
    M = 97
    cs = _case(tag, M)
    g = _Gpu(N, cs, generic)
    in_dim, nan = cs.cfg.in_dim, float("nan")
    d_enc0, d_w0 = g.bwd()
    out0, sig0 = g.fwd(), g.density()
    _check_grads(f"{tag} generic={generic} M={M}", g, d_enc0, d_w0, cs)
    ws = N.ngp_workspace(g.net, M, torch.device(DEV, torch.cuda.current_device()))
    ws.fill_(255)   # every float of the slabs and of the W^T image: a NaN (0xffffffff)
    assert bool(torch.isnan(ws[:ws.numel() // 4 * 4].view(torch.float32)).all())
    enc = torch.full((M, in_dim + 5), nan, device=DEV)
    enc[:, :in_dim] = g.enc
    assert enc.stride(0) == in_dim + 5
    d_enc = torch.full_like(enc, nan)
    d_w = torch.full((g.layout.total,), nan, device=DEV)
    ws2 = N.ngp_workspace(g.net, M, torch.device(DEV, torch.cuda.current_device()))
    assert ws2.data_ptr() == ws.data_ptr()   # the poisoned buffer is the one the backward gets
    g.bwd(enc=enc, d_enc=d_enc, d_w=d_w, accumulate=False)
    torch.cuda.synchronize()
    pads = g.pad_mask()
    d_w_c = d_w.cpu()
    assert bool((d_w_c[pads] == 0).all()), "non-zero gradient at a pad position"
    assert bool(torch.isfinite(d_w_c[~pads]).all())
    assert torch.equal(d_w, d_w0)
    assert torch.equal(d_enc[:, :in_dim], d_enc0)
    assert bool(torch.isnan(d_enc[:, in_dim:]).all())
    assert torch.equal(g.fwd(enc=enc), out0) and torch.equal(g.density(enc=enc), sig0)


# ------------------------------------------------------------------------------------------ 6. entry-point arguments

@pytest.mark.parametrize("tag", ["wide_in", "prod"])
def test_accumulate_and_unaligned_d_w(N, tag):
    cs = _case(tag, 97)
    g = _Gpu(N, cs)
    total = g.layout.total
    _, fresh = g.bwd()
    preset = torch.randn(total, generator=torch.Generator().manual_seed(5)).to(DEV)
    acc = preset.clone()
    g.bwd(d_w=acc, accumulate=True)
    want = preset + fresh
    assert bool(((acc - want).abs() <= 2.0 ** -23 * want.abs()).all())   # one fp32 rounding of the sum
    assert torch.equal(acc.cpu()[g.pad_mask()], preset.cpu()[g.pad_mask()])
    # a d_w that is not 16-byte aligned takes the scalar-store reduce: the same values bitwise
    buf = torch.full((total + 1,), float("nan"), device=DEV)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4
    g.bwd(d_w=view, accumulate=False)
    assert torch.equal(view, fresh) and bool(torch.isnan(buf[0]))
    buf[1:] = preset
    g.bwd(d_w=view, accumulate=True)
    assert torch.equal(view, acc)


def test_workspace_and_stride_checks(N, monkeypatch):
    cs = _case("wide_in", 97)
    g = _Gpu(N, cs)
    M, total = 97, g.layout.total
    a = ctypes.c_void_p(ctypes.addressof(g.net))
    need = int(N.lib().nerf_ngp_workspace_bytes(a, M)) - 256
    assert need == (math.ceil(M / 32) + 1) * total * 4   # 4 workgroups' slabs + the W^T image
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    d_enc, d_w = torch.empty_like(g.enc), torch.empty(total, device=DEV)

    def raw(nbytes):
        return N.lib().nerf_ngp_bwd(a, N.ptr(g.w), N.ptr(g.enc), g.enc.stride(0), N.ptr(g.x_d), M, N.ptr(g.gup),
                                    N.ptr(d_enc), N.ptr(d_w), 0, N.ptr(ws), nbytes, N.stream())

    assert raw(need - 1) == -4   # NERF_E_WORKSPACE
    assert raw(need) == 0
    torch.cuda.synchronize()
    assert torch.equal(d_w, g.bwd()[1])
    # ... surfaced as the wrapper's error
    monkeypatch.setattr(N, "ngp_workspace", lambda net, M, device: ws[:need - 1])
    with pytest.raises(RuntimeError, match="workspace too small"):
        g.bwd()
    monkeypatch.undo()
    # enc_stride < in_dim: NERF_E_ARG from every entry point
    short = g.enc[:, :cs.cfg.in_dim - 1].contiguous()
    assert short.stride(0) == cs.cfg.in_dim - 1
    for call in (lambda: g.fwd(enc=short), lambda: g.density(enc=short),
                 lambda: g.bwd(enc=short, d_enc=torch.empty_like(g.enc))):
        with pytest.raises(ValueError, match="invalid argument"):
            call()


@pytest.mark.parametrize("tag", ["wide_in", "prod"])
def test_zero_rows(N, tag):
    cs = _case(tag, 97)
    g = _Gpu(N, cs)
    e0 = torch.empty((0, cs.cfg.in_dim), device=DEV)
    x0, g0 = torch.empty((0, 6), device=DEV), torch.empty((0, 4), device=DEV)
    d_w = torch.full((g.layout.total,), float("nan"), device=DEV)
    N.ngp_bwd(g.net, g.w, e0, x0, g0, d_w=d_w, accumulate=False)
    assert bool((d_w == 0).all())
    d_w.fill_(3.0)
    N.ngp_bwd(g.net, g.w, e0, x0, g0, d_w=d_w, accumulate=True)
    assert bool((d_w == 3.0).all())
    assert N.ngp_fwd(g.net, g.w, e0, x0).shape == (0, 4) and N.ngp_density(g.net, g.w, e0).shape == (0,)


# ------------------------------------------------------------------------------------------ 7. directions

@pytest.mark.parametrize("tag", ["freq31", "sh5"])
def test_direction_edges(N, tag):
    """Rows with d = 0, |d| = 1e-12 (below the 1e-9 clamp of the first normalisation) and |d| = 1e3."""
    _assert_path(tag)
    cs = _case(tag, 97, True, dirs="edges")
    n = cs.x_d[:, 3:6].norm(dim=-1)
    assert int((n == 0).sum()) >= 10 and int(((n > 0) & (n < 1e-9)).sum()) >= 10 and int((n > 999).sum()) >= 10
    g = _Gpu(N, cs)
    out = g.fwd()
    d_enc, d_w = g.bwd()
    torch.cuda.synchronize()
    _check_fwd(f"{tag} direction edges", out, cs)
    _check_grads(f"{tag} direction edges", g, d_enc, d_w, cs)


# ------------------------------------------------------------------------------------------ 8. saturated head

@pytest.mark.parametrize("bias", [100.0, -100.0])
@pytest.mark.parametrize("tag,generic", [("sd0", 0), ("prod", 0), ("prod", 1)])
def test_saturated_sigma_head(N, tag, generic, bias):
    """sigma_head.bias = +-100: sigma_raw is far outside trunc_exp's clamp (+-88.72) on every row.  High side: sigma
    finite and within 1e-5 relative (the clamp constant rounded to fp32 moves exp by <= 4e-6 relative); the gradients,
    with the sigma upstream scaled by 1e-36, against the reference.  Low side: sigma within 1e-37 absolute.
    (Before ngp_trunc_exp capped the overflow, the high side gave sigma = +inf: fp32(88.722839111) > ln(FLT_MAX).)
    The production shape runs too, on its compile-time kernels and on the generic ones: they share the expression."""
    _assert_path(tag)
    cs = _case(tag, 97, True, head_bias=bias, sigma_up=1e-36)
    g = _Gpu(N, cs, generic)
    out = g.fwd()
    sig = g.density()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and torch.equal(sig, out[:, 3])
    e_rgb = float((out[:, :3].double().cpu() - cs.out[:, :3]).abs().max())
    assert e_rgb <= FWD_TOL, e_rgb
    s, ref = out[:, 3].double().cpu(), cs.out[:, 3]
    if bias > 0:
        assert float(ref.min()) > 3.0e38
        e = float(((s - ref).abs() / ref).max())
        print(f"[ngp-edges] {tag} generic={generic} saturated head +100: sigma relative {e:.2e} (bound 1e-05)")
        assert e <= 1e-5, e
        d_enc, d_w = g.bwd()
        torch.cuda.synchronize()
        assert float(cs.grads["sigma_head.bias"].abs().max()) > 1.0   # the sigma branch dominates the gradients
        _check_grads(f"{tag} generic={generic} saturated head +100", g, d_enc, d_w, cs)
        # a saturated row with a zero upstream gradient contributes 0, not 0 * inf = NaN
        g.gup = torch.zeros_like(g.gup)
        d_enc0, d_w0 = g.bwd()
        assert bool((d_w0 == 0).all()) and bool((d_enc0 == 0).all())
    else:
        assert float(ref.max()) < 3.0e-39
        e = float((s - ref).abs().max())
        print(f"[ngp-edges] {tag} generic={generic} saturated head -100: sigma absolute {e:.2e} (bound 1e-37)")
        assert e <= 1e-37, e


# ------------------------------------------------------------------------------------------ 9. module level

MODULES = {
    "nodepth": dict(hidden=33, geo_feat_dim=0, sigma_depth=0, color_depth=0, color_hidden=17,
                    hash_enc_conf=dict(levels=4, features_per_level=2, log2_hashmap_size=10, min_res=4, max_res=32)),
    "wide_in": dict(hidden=17, geo_feat_dim=31, sigma_depth=1, color_depth=1, color_hidden=33,
                    hash_enc_conf=dict(levels=16, features_per_level=4, log2_hashmap_size=9, min_res=4, max_res=64)),
}


@pytest.mark.parametrize("tag", list(MODULES))
def test_module_forward_backward_vs_oracle(N, tag):
    """InstantNGP with a non-default shape end to end (hash grid, pack, generic kernels, table scatter) against
    NO.ngp_forward in float64.  Rows are chosen kink free from the float64 oracle's pre-activations."""
    kw = MODULES[tag]
    cfg = R.CONFIGS[tag]
    hc = kw["hash_enc_conf"]
    assert hc["levels"] * hc["features_per_level"] == cfg.in_dim
    assert (kw["hidden"], kw["sigma_depth"], kw["geo_feat_dim"], kw["color_hidden"], kw["color_depth"]) == cfg[1:6]
    _assert_path(tag)
    torch.manual_seed(17)
    box = torch.tensor([[-1.0, -2.0, -0.5], [1.5, 1.0, 2.0]])
    net = N.InstantNGP(scene_box=box, dir_encoding="spherical", **kw)
    with torch.no_grad():
        net.xyz_encoder.hash_table.uniform_(-1.0, 1.0)
    assert net.layout.total == R.config_plan(cfg).total
    w = {n: p.detach().double().clone().requires_grad_(True) for n, p in net.named_parameters()}
    table = w.pop("xyz_encoder.hash_table")
    res, _ = NO.hash_resolutions(hc["levels"], hc["min_res"], hc["max_res"])
    M = 97
    gen = torch.Generator().manual_seed(23)
    pool = torch.cat([box[0] + torch.rand(2 * M, 3, generator=gen) * (box[1] - box[0]),
                      torch.randn(2 * M, 3, generator=gen)], -1)
    with torch.no_grad():
        x01 = ((pool[:, :3].double() - box[0].double()) / (box[1] - box[0]).double()).clamp(1e-6, 1 - 1e-6)
        enc = NO.hash_encode(table, x01, res, hc["log2_hashmap_size"], hc["features_per_level"])
        _, pre = R.mlp_reference(w, enc, pool, sigma_depth=cfg.sigma_depth, color_depth=cfg.color_depth, dir_mode=0,
                                 sh_levels=4, sigmoid=True, return_preacts=True)
    keep = R.kink_free_rows(pre, 1e-4, rows=2 * M)
    assert keep.numel() >= M
    x_d = pool[keep[:M]].contiguous()
    gup = torch.randn(M, 4, generator=gen)
    ref = NO.ngp_forward(w, table, x_d.double(), box.double(), res, hc["log2_hashmap_size"],
                         hc["features_per_level"], sigma_depth=cfg.sigma_depth, color_depth=cfg.color_depth)
    rg = torch.autograd.grad((ref * gup.double()).sum(), list(w.values()) + [table])
    net = net.to(DEV)
    out = net(x_d.to(DEV))
    (out * gup.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    e = _rel(out, ref.detach())
    print(f"[ngp-edges] module {tag} forward {e:.2e} (bound {FWD_TOL:.0e})")
    assert e <= FWD_TOL
    params = dict(net.named_parameters())
    errs = {n: _rel(params[n].grad, r) for n, r in zip(list(w) + ["xyz_encoder.hash_table"], rg)}
    name = max(errs, key=errs.get)
    print(f"[ngp-edges] module {tag} gradients {errs[name]:.2e} at {name} (bound {GRAD_TOL:.0e})")
    assert all(v <= GRAD_TOL for v in errs.values()), errs


@pytest.mark.parametrize("tag", list(R.REJECTED))
def test_module_rejects_unsupported_shapes(N, tag):
    in_dim, hidden, sd, geo, ch, cd, _ = R.REJECTED[tag]
    assert R.plan_reference(*R.REJECTED[tag]) is None
    # in_dim is the hash grid's levels x features per level: 65 = 13 x 5
    levels, F = {16: (8, 2), 32: (16, 2), 65: (13, 5)}[in_dim]
    box = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    with pytest.raises(ValueError, match="unsupported MetaNGP configuration"):
        N.InstantNGP(scene_box=box, hidden=hidden, sigma_depth=sd, geo_feat_dim=geo, color_hidden=ch, color_depth=cd,
                     hash_enc_conf=dict(levels=levels, features_per_level=F, log2_hashmap_size=4, min_res=2,
                                        max_res=8))
