"""CPU: the references of tests/ngp_mlp_reference.py checked on their own -- the Python restatement of make_plan
against the ngp_prod constants parsed out of csrc/ngp.hip, the path every named configuration of the GPU edge tests
must reach, mlp_reference against the reference's golden vectors, and its autograd against finite differences."""
import os
import re

import pytest
import torch

from golden_io import load
from oracle import ngp_oracle as NO
import ngp_mlp_reference as R

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nerf-sys_amd", "csrc", "ngp.hip")


def _prod_constants():
    src = open(HIP).read()
    body = src[src.index("namespace ngp_prod {"):]
    body = body[:body.index("}  // namespace ngp_prod")]
    scal = {}
    for m in re.finditer(r"constexpr int ([^;\[\]]+);", body):
        for item in m.group(1).split(","):
            k, v = item.split("=")
            if re.fullmatch(r"\s*-?\d+\s*", v):
                scal[k.strip()] = int(v)
    arr = {m.group(1): [int(x) for x in m.group(2).split(",")]
           for m in re.finditer(r"constexpr int (\w+)\[NL\] = \{([\d,\s]+)\};", body)}
    return scal, arr


def test_plan_reference_equals_production_constants():
    scal, arr = _prod_constants()
    for k in ("NL", "HEAD", "TOTAL", "BSUM", "SMEM", "GEO", "DIRD"):
        assert k in scal, f"ngp_prod::{k} not found in csrc/ngp.hip"
    for k in ("KP", "NP", "WOFF", "BOFF"):
        assert k in arr and len(arr[k]) == scal["NL"], f"ngp_prod::{k}[NL] not found in csrc/ngp.hip"
    p = R.config_plan(R.CONFIGS["prod"])
    assert (scal["GEO"], scal["DIRD"]) == (15, 16)
    assert len(p.layers) == scal["NL"] and p.head == scal["HEAD"]
    assert [L.Kpad for L in p.layers] == arr["KP"]
    assert [L.Npad for L in p.layers] == arr["NP"]
    assert [L.w_off for L in p.layers] == arr["WOFF"]
    assert [L.b_off for L in p.layers] == arr["BOFF"]
    assert (p.total, p.bsum, p.smem_floats) == (scal["TOTAL"], scal["BSUM"], scal["SMEM"])


@pytest.mark.parametrize("tag", list(R.CONFIGS))
def test_named_configurations_reach_their_path(tag):
    c = R.CONFIGS[tag]
    p = R.config_plan(c)
    assert p is not None
    assert (len(p.layers), p.nsb, p.bsum < 0) == R.EXPECTED_PATH[tag]
    assert len(p.layers) == c.sigma_depth + c.color_depth + 2
    # the packed layout has room for exactly the named tensors plus pads, without overlaps
    shapes = NO.ngp_param_shapes(c.in_dim, c.hidden, c.sigma_depth, c.geo, c.color_hidden, c.color_depth,
                                 R.config_dir_dim(c))
    assert sum(L.K * L.N + L.N for L in p.layers) == sum(int(torch.Size(s).numel()) for s in shapes.values())
    o = 0
    for L in p.layers:
        assert (L.w_off, L.b_off) == (o, o + L.Npad * L.Kpad) and L.K <= L.Kpad <= 64 and L.N <= L.Npad <= 64
        o = L.b_off + L.Npad
    assert o == p.total


def test_paths_named_by_the_issue():
    assert R.config_plan(R.CONFIGS["nsb8"]).wgrad_blocks == 28 and R.config_plan(R.CONFIGS["nsb8"]).slots_per_wave == 7
    assert R.config_plan(R.CONFIGS["nsb8_in64"]).wgrad_blocks == 26
    assert R.config_plan(R.CONFIGS["in40"]).nsb == 6
    assert len(R.config_plan(R.CONFIGS["twelve"]).layers) == R.MAX_LAYERS
    assert R.config_plan(R.CONFIGS["mix"]).bsum >= 0 and len(R.config_plan(R.CONFIGS["mix"]).layers) == 8
    w = R.config_plan(R.CONFIGS["wide_in"]).layers[0]
    assert (w.Kpad, w.Npad) == (64, 32)


@pytest.mark.parametrize("tag", list(R.REJECTED))
def test_rejected_shapes(tag):
    assert R.plan_reference(*R.REJECTED[tag]) is None
    # ... and each is one step beyond a shape that is accepted
    ok = {"hidden65": (16, 64, 2, 15, 64, 2, 16), "in65": (64, 64, 2, 15, 64, 2, 16), "geo32": (32, 64, 2, 31, 64, 2, 16),
          "layers13": (16, 32, 5, 15, 32, 5, 16), "twelve_wide": (16, 32, 5, 15, 32, 5, 16)}[tag]
    assert R.plan_reference(*ok) is not None


def test_mlp_reference_matches_golden_m1():
    z = load("ngp")
    w = {k[5:]: v for k, v in z.items() if k.startswith("m1_w/")}
    table = w.pop("xyz_encoder.hash_table")
    res, _ = NO.hash_resolutions(8, 16, 1024)
    x_d, aabb = z["ngp_x_d"], z["ngp_aabb"]
    x01 = ((x_d[:, :3] - aabb[0]) / (aabb[1] - aabb[0])).clamp(1e-6, 1.0 - 1e-6)
    enc = NO.hash_encode(table, x01, res, 12, 2, "Linear")
    out = R.mlp_reference(w, enc, x_d, sigma_depth=2, color_depth=2, dir_mode=0, sh_levels=4, sigmoid=True,
                          dtype=torch.float32)
    torch.testing.assert_close(out, z["m1_out"], rtol=1e-5, atol=1e-6)
    out64 = R.mlp_reference(w, enc, x_d, sigma_depth=2, color_depth=2, dir_mode=0, sh_levels=4, sigmoid=True)
    torch.testing.assert_close(out64.float(), z["m1_out"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("dir_mode,sigmoid", [(0, True), (1, False)])
def test_mlp_reference_autograd_vs_finite_differences(dir_mode, sigmoid):
    """2 rows, 4 layers of width 3, fp64: central differences (h = 1e-6) of sum(out * gup) in every weight, bias and
    enc entry.  The rows are kink free by 1e-3, far more than h moves any pre-activation."""
    cfg = R.Config(3, 3, 1, 2, 3, 1, dir_mode, 2)
    cs = R.draw_case(cfg, 2, 7, sigmoid=sigmoid, margin=1e-3)
    gup = cs.gup.double()
    named = {k: v.double() for k, v in cs.named.items()}
    enc = cs.enc.double()

    def f(nm, e):
        return float((R.mlp_reference(nm, e, cs.x_d, **cs.kw) * gup).sum())

    h = 1e-6
    for name, ref in list(cs.grads.items()) + [("enc", cs.d_enc)]:
        base = enc if name == "enc" else named[name]
        fd = torch.zeros_like(base)
        for i in range(base.numel()):
            vals = []
            for sgn in (1.0, -1.0):
                t = base.clone()
                t.view(-1)[i] += sgn * h
                vals.append(f(named, t) if name == "enc" else f({**named, name: t}, enc))
            fd.view(-1)[i] = (vals[0] - vals[1]) / (2 * h)
        assert ref.shape == base.shape
        assert float((fd - ref).abs().max()) <= 1e-8 * max(1.0, float(ref.abs().max())), name


def test_preactivations_and_kink_filter():
    cfg = R.CONFIGS["mix"]
    cs = R.draw_case(cfg, 16, 3)
    out, pre = R.mlp_reference(cs.named, cs.enc, cs.x_d, return_preacts=True, **cs.kw)
    assert [tuple(z.shape) for z in pre] == [(16, 64)] * 3 + [(16, 32)] * 3
    assert torch.equal(out, cs.out)
    assert R.kink_free_rows(pre, 1e-4).tolist() == list(range(16))
    z = pre[2].clone()
    z[5, 7] = 5e-5
    z[9, 0] = -9.9e-5
    assert R.kink_free_rows(pre[:2] + [z] + pre[3:], 1e-4).tolist() == [i for i in range(16) if i not in (5, 9)]
    assert R.kink_free_rows([], 1e-4, rows=4).tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("tag", list(R.CONFIGS))
def test_kink_filter_leaves_enough_rows(tag):
    """The survival condition of the GPU tests (at least M of 2 M candidate rows kink free) on the CPU, where it
    cannot depend on any kernel output; draw_case raises when it fails."""
    cs = R.draw_case(R.CONFIGS[tag], 97, 1)
    assert cs.survival >= 0.5 and cs.enc.shape == (97, R.CONFIGS[tag].in_dim)
