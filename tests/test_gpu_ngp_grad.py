"""Gradients w.r.t. the sample positions on the HIP path: nerf_hash_encode_bwd_x (any grid), the fused
nerf_ngp_density_grad_enc (production shape) and the surface built on them (HashGridEncoder backward,
InstantNGP.density_grad / normals / density with x.requires_grad).  Run on an MI355X: -m gpu.

The reference is the fp32 CPU oracle's autograd (oracle/ngp_oracle.py), not fp64: the kernels share the oracle's fp32
cell arithmetic bit for bit, and an fp64 run puts a few samples per ten thousand into another cell at resolution 2048.
Gradient bar as in test_gpu_ngp.py: |got - ref| <= 1e-4 max(1, max|ref|).  The measured maxima stand beside each
bound (MI355X, the figures of the run that accompanied this file)."""
import pytest
import torch

import ngp_grad_cases as C
from golden_io import load
from oracle import ngp_oracle as NO
from test_gpu_ngp import HCFG, MCFG, _ngp_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _err(a, b):
    return (a.detach().float().cpu() - b.detach().float().cpu()).abs().max().item() if a.numel() else 0.0


def _bar(ref):
    return 1e-4 * max(1.0, ref.abs().max().item() if ref.numel() else 0.0)


@pytest.fixture(scope="module")
def z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load("ngp")


@pytest.fixture(scope="module")
def N():
    from nerf_amd import ngp
    return ngp


def _grid(N, L, F, log2T, mn, mx, interp):
    return N.HashGridEncoder(levels=L, features_per_level=F, log2_hashmap_size=log2T, min_res=mn, max_res=mx,
                             interpolation=interp).grid


def _oracle_hash_dx(table, x, gup, cfg, aabb=None, eps=1e-6):
    """autograd of the oracle's encoding (after MetaNGP._world_to_unit when aabb is given) w.r.t. x; None if unused"""
    L, F, log2T, mn, mx, interp = cfg
    res, _ = NO.hash_resolutions(L, mn, mx)
    x = x.detach().clone().requires_grad_(True)
    x01 = x if aabb is None else ((x - aabb[0]) / (aabb[1] - aabb[0])).clamp(eps, 1.0 - eps)
    # the table takes part in the graph so that Nearest, whose output does not depend on x, still has one
    y = NO.hash_encode(table.detach().clone().requires_grad_(True), x01, res, log2T, F, interp)
    return torch.autograd.grad((y * gup).sum(), x, allow_unused=True)[0]


# ------------------------------------------------------------------------------------------ A. hash gradient

@pytest.mark.parametrize("tag", list(HCFG))
def test_hash_bwd_x_golden(z, N, tag):
    """HCFG a-d with the golden tables, hash_x and hash_*_gup; no sample excluded.
    Measured max |got - ref|: a 2.0e-3 of max|ref| 1.7e4 (bar 1.7), b 2.9e-3 of 1.5e4 (bar 1.5), d 2.4e-4 of 1.5e3
    (bar 0.15); c exact zeros."""
    cfg = HCFG[tag]
    table, x, gup = z[f"hash_{tag}_table"], z["hash_x"], z[f"hash_{tag}_gup"]
    ref = _oracle_hash_dx(table, x, gup, cfg)
    got = N.hash_encode_bwd_x(_grid(N, *cfg), table.to(DEV), x.to(DEV), gup.to(DEV), None, 0.0)
    if cfg[5] == "Nearest":
        assert ref is None
        assert torch.equal(got.cpu(), torch.zeros_like(x))
        return
    print(f"hash_bwd_x {tag}: max err {_err(got, ref):.3g}, max|ref| {ref.abs().max().item():.3g}")
    assert _err(got, ref) <= _bar(ref)
    again = N.hash_encode_bwd_x(_grid(N, *cfg), table.to(DEV), x.to(DEV), gup.to(DEV), None, 0.0)
    assert torch.equal(got, again)  # one summation order, no atomics


@pytest.mark.parametrize("interp", ["Linear", "Smoothstep"])
def test_hash_bwd_x_known_answer(N, interp):
    """Table linear in the vertex: d_x for a one-hot d_out is the closed-form Jacobian row.  Bound 1e-5; measured
    4.8e-7 / 1.2e-6 (Linear, f = 0 / 1), 1.4e-6 / 1.4e-6 (Smoothstep)."""
    table, _ = C.known_answer_table()
    x = C.known_answer_points()
    J = C.known_answer_jacobian(x, interp)
    g = _grid(N, C.KA["levels"], 2, C.KA["log2_hashmap_size"], C.KA["min_res"], C.KA["max_res"], interp)
    for f in range(2):
        d_out = torch.zeros(x.shape[0], 2)
        d_out[:, f] = 1.0
        got = N.hash_encode_bwd_x(g, table.to(DEV), x.to(DEV), d_out.to(DEV), None, 0.0)
        print(f"known answer {interp} f={f}: max err {_err(got, J[:, f]):.3g}")
        assert _err(got, J[:, f]) <= 1e-5


@pytest.fixture(scope="module")
def edge(z):
    """257 points around the unit cube on grid b (16 levels, Smoothstep) and their reference, computed once"""
    g = torch.Generator().manual_seed(17)
    x = torch.rand(257, 3, generator=g) * 1.4 - 0.2
    gup = torch.randn(257, 32, generator=g)
    return x, gup, _oracle_hash_dx(z["hash_b_table"], x, gup, HCFG["b"])


@pytest.mark.parametrize("xs", [3, 6])
@pytest.mark.parametrize("M", [0, 1, 15, 17, 31, 33, 257])
def test_hash_bwd_x_edges(z, N, edge, M, xs):
    """Ragged M, x rows of pitch 3 and 6, d_out of pitch 36 with NaN in the pad columns, d_x of pitch 4 whose column
    3 must survive.  Measured at M = 257: max err 1.7e-3 of max|ref| 1.25e4 (bar 1.25)."""
    x, gup, ref = (t[:M] for t in edge)
    xb = torch.full((M, xs), 7.0)
    xb[:, :3] = x
    db = torch.full((M, 36), float("nan"))
    db[:, :32] = gup
    out = torch.full((M, 4), -123.0, device=DEV)
    got = N.hash_encode_bwd_x(_grid(N, *HCFG["b"]), z["hash_b_table"].to(DEV), xb.to(DEV)[:, :3], db.to(DEV)[:, :32],
                              None, 0.0, d_x=out)
    assert got is out
    assert torch.equal(out[:, 3].cpu(), torch.full((M,), -123.0))
    assert torch.isfinite(out).all()
    print(f"edges M={M} xs={xs}: max err {_err(out[:, :3], ref):.3g}, bar {_bar(ref):.3g}")
    assert _err(out[:, :3], ref) <= _bar(ref)


def test_hash_bwd_x_aabb(z, N):
    """World points up to 7 % outside the box: a component outside on its axis is exactly 0 (torch.clamp's backward),
    the sample's other components still match.  Measured: max err 7.3e-4 of max|ref| 5.7e3 (bar 0.57)."""
    cfg = HCFG["a"]
    g = torch.Generator().manual_seed(23)
    aabb = torch.tensor([[-1.5, -1.0, -2.0], [1.5, 2.0, 1.0]])
    x = (torch.rand(300, 3, generator=g) * 1.14 - 0.07) * (aabb[1] - aabb[0]) + aabb[0]
    gup = torch.randn(300, 8, generator=g)
    ref = _oracle_hash_dx(z["hash_a_table"], x, gup, cfg, aabb, 1e-6)
    got = N.hash_encode_bwd_x(_grid(N, *cfg), z["hash_a_table"].to(DEV), x.to(DEV), gup.to(DEV),
                              aabb.reshape(-1).tolist(), 1e-6).cpu()
    outside = (x < aabb[0]) | (x > aabb[1])
    assert outside.any(0).all() and (outside.sum(-1) == 1).any()
    assert (got[outside] == 0).all() and (ref[outside] == 0).all()
    print(f"aabb: max err {_err(got, ref):.3g}, max|ref| {ref.abs().max().item():.3g}")
    assert _err(got, ref) <= _bar(ref)


def test_hash_encoder_module_backward_fills_x_grad(z, N):
    """HashGridEncoder(x).backward: x.grad is the oracle's, hash_table.grad still the golden one."""
    L, F, log2T, mn, mx, interp = HCFG["a"]
    enc = N.HashGridEncoder(levels=L, features_per_level=F, log2_hashmap_size=log2T, min_res=mn, max_res=mx,
                            interpolation=interp).to(DEV)
    with torch.no_grad():
        enc.hash_table.copy_(z["hash_a_table"].to(DEV))
    x = z["hash_x"].to(DEV).requires_grad_(True)
    y = enc(x)
    assert torch.equal(y.detach().cpu(), z["hash_a_out"])
    (y * z["hash_a_gup"].to(DEV)).sum().backward()
    ref = _oracle_hash_dx(z["hash_a_table"], z["hash_x"], z["hash_a_gup"], HCFG["a"])
    assert _err(x.grad, ref) <= _bar(ref)
    gt = z["hash_a_gtable"]
    assert _err(enc.hash_table.grad, gt) <= 1e-6 * max(1.0, gt.abs().max().item())


# ------------------------------------------------------------------------------------------ B. fused kernel

def _prod_net(N, state):
    net = N.InstantNGP(occ_conf={}, scene_box=C.AABB, **C.PROD)
    net.load_reference_state(state)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def prod(N):
    """The production-shape expert, the 4096 points and the fp32 oracle's sigma / gradient / kink margins (once)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    st = C.prod_state()
    x = C.prod_points()
    sig, g, zmin = C.oracle_density(st, x, C.PROD["hash_enc_conf"], C.AABB)
    return _prod_net(N, st), x, sig, g, zmin >= C.KINK


def _fused(N, net, x, grad=None):
    with torch.no_grad():
        return N.ngp_density_grad_enc(net.net_struct, net.xyz_encoder.grid, net.xyz_encoder.hash_table.detach(),
                                      net.packed().detach(), x, net._aabb_host, net._eps, grad=grad)


def _composed(net, x):
    with torch.no_grad():
        return net._density_grad_composed(x.contiguous(), net.packed().detach(), net.xyz_encoder.hash_table.detach())


def test_density_grad_fused_vs_composed_and_oracle(N, prod):
    """M = 4096: sigma bitwise nerf_ngp_density_enc's; grad within 1e-6 max|ref| of the composed path on EVERY sample
    (it came out bitwise equal on the MI355X: the same tile code and the same summation order); grad within the gradient
    bar of the fp32 oracle on every sample but the low-margin ones (<= 2 %, test_ngp_grad_reference.py).
    Measured: vs composed 0 (bitwise), vs oracle 3.8e-6 of max|ref| 14.9 (bar 1.5e-3), the same 3.8e-6 with the 1.15 %
    low-margin samples left in."""
    net, x, sig_ref, g_ref, keep = prod
    xg = x.to(DEV)
    out = _fused(N, net, xg)
    assert out is not None, "the production shape must take the fused launch"
    sig, grad = out
    with torch.no_grad():
        sig_enc = N.ngp_density_enc(net.net_struct, net.xyz_encoder.grid, net.xyz_encoder.hash_table.detach(),
                                    net.packed().detach(), xg, net._aabb_host, net._eps)
    assert torch.equal(sig, sig_enc)
    assert _err(sig, sig_ref) <= 1e-5 * max(1.0, sig_ref.abs().max().item())
    sig_c, grad_c = _composed(net, xg)
    assert torch.equal(sig_c, sig)
    print(f"fused vs composed: max err {_err(grad, grad_c):.3g} (bitwise: {torch.equal(grad, grad_c)}), "
          f"max|ref| {grad_c.abs().max().item():.3g}")
    assert _err(grad, grad_c) <= 1e-6 * grad_c.abs().max().item()
    assert keep.float().mean().item() >= 0.98
    print(f"fused vs oracle: max err {_err(grad.cpu()[keep], g_ref[keep]):.3g}, max|ref| {g_ref.abs().max().item():.3g}"
          f", all samples {_err(grad, g_ref):.3g}, kept {keep.float().mean().item():.4f}")
    assert _err(grad.cpu()[keep], g_ref[keep]) <= _bar(g_ref)
    outside = ((x < C.AABB[0]) | (x > C.AABB[1]))
    assert outside.any() and (grad.cpu()[outside] == 0).all()


@pytest.mark.parametrize("gs", [3, 4])
@pytest.mark.parametrize("xs", [3, 6])
@pytest.mark.parametrize("M", [0, 1, 31, 33, 1000])
def test_density_grad_fused_edges(N, prod, M, xs, gs):
    """Ragged M, x rows of pitch 3 and 6, grad rows of pitch 3 and 4 (column 3 must survive): bitwise the M = 4096
    launch's first M rows (rows are independent), hence the same distance from the oracle."""
    net, x, _, g_ref, keep = prod
    xb = torch.full((M, xs), 5.0)
    xb[:, :3] = x[:M]
    out = torch.full((M, gs), -7.0, device=DEV)
    sig, grad = _fused(N, net, xb.to(DEV)[:, :3], grad=out)
    assert grad is out and sig.shape == (M,)
    if gs == 4:
        assert torch.equal(out[:, 3].cpu(), torch.full((M,), -7.0))
    sig_c, grad_c = _composed(net, x[:M].to(DEV))
    assert torch.equal(sig, sig_c)
    assert _err(out[:, :3], grad_c) <= 1e-6 * (grad_c.abs().max().item() if M else 0.0)
    k = keep[:M]
    assert _err(out[:, :3].cpu()[k], g_ref[:M][k]) <= _bar(g_ref[:M])


def test_density_grad_saturated_head(N):
    """Huge sigma: sigma_head.bias = 88 and head weights scaled by 1e-3, so sigma ~ 1.6e38 and d sigma / d raw the
    same.  (A bias of 90 cannot have a finite reference in fp32: trunc_exp's clamp constant 88.722839111 rounds to
    88.72283936 > ln(FLT_MAX) = 88.72283905, so torch's exp gives inf there and the oracle's sigma is inf and its
    gradient inf / nan; 88 is the largest integer bias below the clamp.)  The reference must be finite; sigma and the
    gradient match it relatively: raw ~ 88 has an ulp of 2^-17 = 7.6e-6, and one ulp of raw is that relative error in
    sigma and in d sigma / d raw, so sigma's bar is 1e-5 and the gradient's the usual 1e-4 plus 1e-5, of max|ref|.
    Measured: sigma 0 (bitwise the oracle's), grad 2.4e-7 of max|ref| 6.5e36."""
    st = C.prod_state()
    st["sigma_head.bias"] = torch.full((1,), 88.0)
    st["sigma_head.weight"] = st["sigma_head.weight"] * 1e-3
    x = C.prod_points(1000)
    sig_ref, g_ref, zmin = C.oracle_density(st, x, C.PROD["hash_enc_conf"], C.AABB)
    assert torch.isfinite(sig_ref).all() and torch.isfinite(g_ref).all() and sig_ref.min().item() > 1e37
    net = _prod_net(N, st)
    sig, grad = net.density_grad(x.to(DEV))
    keep = zmin >= C.KINK
    assert keep.float().mean().item() >= 0.98
    assert torch.isfinite(sig).all() and torch.isfinite(grad).all()
    es = ((sig.cpu()[:, 0] - sig_ref).abs().max() / sig_ref.abs().max()).item()
    eg = ((grad.cpu()[keep] - g_ref[keep]).abs().max() / g_ref.abs().max()).item()
    print(f"saturated: sigma rel err {es:.3g}, grad rel err {eg:.3g}, max|ref| {g_ref.abs().max().item():.3g}")
    assert es <= 1e-5 and eg <= 1e-4 + 1e-5


@pytest.mark.parametrize("tag", ["m1", "m2"])
def test_density_grad_other_shapes_match_oracle(z, N, tag):
    """density_grad on the golden experts.  m2 (32-wide, one trunk layer) has no fused kernel and falls back to the
    composed general kernels; m1 (8 levels x 2 features, otherwise the production shape) is inside what
    nerf_ngp_density_enc supports, so it takes the fused launch and its composed path is checked beside it.
    Measured (both paths alike): m1 3.1e-6 of max|ref| 10.9, m2 6.7e-6 of 29.9."""
    net = _ngp_from_golden(z, N, tag).eval()
    c = MCFG[tag]
    x = z["ngp_x_d"][:, :3].contiguous()
    st = {k[len(tag) + 3:]: v for k, v in z.items() if k.startswith(f"{tag}_w/")}
    sig_ref, g_ref, zmin = C.oracle_density(st, x, c["hash_enc_conf"], z["ngp_aabb"], c["sigma_depth"])
    keep = zmin >= C.KINK
    assert keep.float().mean().item() >= 0.98
    fused = _fused(N, net, x.to(DEV))
    assert (fused is None) == (tag == "m2")
    sig, grad = net.density_grad(x.to(DEV).view(2, -1, 3))
    assert sig.shape == (2, x.shape[0] // 2, 1) and grad.shape == (2, x.shape[0] // 2, 3)
    sig_c, grad_c = _composed(net, x.to(DEV))
    for s_, g_ in ((sig.view(-1), grad.view(-1, 3)), (sig_c, grad_c)):
        assert _err(s_, sig_ref) <= 1e-5 * max(1.0, sig_ref.abs().max().item())
        print(f"{tag}: max err {_err(g_.cpu()[keep], g_ref[keep]):.3g}, max|ref| {g_ref.abs().max().item():.3g}")
        assert _err(g_.cpu()[keep], g_ref[keep]) <= _bar(g_ref)


# ------------------------------------------------------------------------------------------ C. surface

def test_density_with_x_requires_grad_and_normals(N, prod):
    """Frozen parameters: density(x) with x.requires_grad gives the oracle's x.grad (it used to return a tensor
    without a graph); without x.requires_grad it returns the same bits as nerf_ngp_density_enc, as before; normals are
    -normalize(grad), unit length or zero."""
    net, x, sig_ref, g_ref, keep = prod
    M = 1000
    for p in net.parameters():
        p.requires_grad_(False)
    try:
        xg = x[:M].to(DEV).requires_grad_(True)
        s = net.density(xg.view(10, 100, 3))
        assert s.shape == (10, 100, 1) and s.requires_grad
        gup = torch.randn(10, 100, 1, generator=torch.Generator().manual_seed(5))
        (s * gup.to(DEV)).sum().backward()
        ref = g_ref[:M] * gup.view(M, 1)
        k = keep[:M]
        assert _err(xg.grad.cpu()[k], ref[k]) <= _bar(ref)
        plain = net.density(x[:M].to(DEV))
        assert not plain.requires_grad
        with torch.no_grad():
            sig_enc = N.ngp_density_enc(net.net_struct, net.xyz_encoder.grid, net.xyz_encoder.hash_table.detach(),
                                        net.packed().detach(), x[:M].to(DEV), net._aabb_host, net._eps)
        assert torch.equal(plain.view(-1), sig_enc) and torch.equal(s.detach().view(-1), sig_enc)
        n = net.normals(x[:M].to(DEV))
        _, g = net.density_grad(x[:M].to(DEV))
        ln = n.norm(dim=-1)
        zero = g.abs().sum(-1) == 0
        assert ((ln - 1).abs() <= 1e-5)[~zero].all() and (ln[zero] == 0).all()
        assert _err(n, -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12)) <= 1e-6
    finally:
        for p in net.parameters():
            p.requires_grad_(True)
