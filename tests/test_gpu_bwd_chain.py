"""The chained fp32 trunk input gradients (-m gpu; gemm_nt_x6w_dgrad_chain_kernel in nerf-sys_amd/csrc/gemm_x6.hpp):
one launch carries every 256-row tile through the seven input-gradient layers, both 128-column tiles of each.  It runs
the per-layer kernel's tile code once per body, so it must agree BITWISE with the fourteen per-layer launches
(MLP_BWD_LAYERED) — d_w and every dZ_i, padded rows included.  Sizes: one partial tile, the tile edge (255, 256, 257)
and 256 (CU count + 1) + 1 rows, which puts a second row tile on at least one CU, so a first body follows another tile's
last epilogue there.  Workspaces are zero-filled first (mlp_workspace is torch.empty) and both forms write each dZ_i to
its own buffer, so the whole workspaces can be compared as bytes."""
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def w(K):
    from nerf_amd.vanilla import VanillaNeRF
    net = VanillaNeRF().load_reference_state(O.init_vanilla_params(5)).to(DEV)
    return net.packed().detach().contiguous()


def _sizes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    return [1, 255, 256, 257, 256 * (cus + 1) + 1]


def _x(M):
    g = torch.Generator().manual_seed(M)
    return torch.cat([torch.rand(M, 3, generator=g) * 3 - 1.5,
                      torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=-1)], -1).to(DEV)


def _gup(M):
    return torch.randn(M, 4, generator=torch.Generator().manual_seed(M + 1)).to(DEV) * 1e-3


def _same_bits(a, b):
    """Bitwise: torch.equal on floats takes -0.0 for 0.0."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _fwd_ws(K, w, x, nbytes=None):
    """A zero-filled workspace after a training forward."""
    M = x.shape[0]
    ws = torch.zeros(nbytes if nbytes is not None else K.mlp_workspace_bytes(M, True), dtype=torch.uint8, device=DEV)
    K.mlp_fwd(w, x, ws, True)
    return ws


@pytest.fixture(scope="module")
def ref257(K, w):
    """M = 257: the layered backward's d_w and workspace, computed once and only read by the tests below."""
    M = 257
    ws = _fwd_ws(K, w, _x(M))
    dw = K.mlp_bwd(w, M, _gup(M), ws, fp32_flags=K.MLP_BWD_LAYERED)
    return dw, ws


@pytest.mark.parametrize("i", range(5), ids=["M1", "M255", "M256", "M257", "cu_count_plus_1_tiles"])
def test_chained_against_layered_bitwise(K, w, i):
    M = _sizes()[i]
    x, gup = _x(M), _gup(M)
    ws_c, ws_l = _fwd_ws(K, w, x), _fwd_ws(K, w, x)
    assert torch.equal(ws_c, ws_l)
    dw_c = K.mlp_bwd(w, M, gup, ws_c)
    dw_l = K.mlp_bwd(w, M, gup, ws_l, fp32_flags=K.MLP_BWD_LAYERED)
    assert torch.isfinite(dw_c).all() and dw_c.abs().max().item() > 0
    assert _same_bits(dw_c, dw_l), "d_w differs"
    assert torch.equal(ws_c, ws_l), "workspace (every dZ_i, padded rows included) differs"


def test_repeat_gives_the_same_bits(K, w, ref257):
    M = 257
    ws = _fwd_ws(K, w, _x(M))
    dw1 = K.mlp_bwd(w, M, _gup(M), ws).clone()
    ws1 = ws.clone()
    dw2 = K.mlp_bwd(w, M, _gup(M), ws)
    assert _same_bits(dw1, dw2) and torch.equal(ws1, ws)
    assert _same_bits(dw1, ref257[0]) and torch.equal(ws, ref257[1])


def test_accumulate_bitwise(K, w):
    M = 257
    x, gup = _x(M), _gup(M)
    base = torch.randn(w.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    dw_c = K.mlp_bwd(w, M, gup, _fwd_ws(K, w, x), d_w=base.clone(), accumulate=True)
    dw_l = K.mlp_bwd(w, M, gup, _fwd_ws(K, w, x), d_w=base.clone(), accumulate=True, fp32_flags=K.MLP_BWD_LAYERED)
    assert not _same_bits(dw_c, base)
    assert _same_bits(dw_c, dw_l)


def test_two_streams_bitwise(K, w, ref257):
    M = 257
    dw_c = K.mlp_bwd(w, M, _gup(M), _fwd_ws(K, w, _x(M)))
    ws2 = _fwd_ws(K, w, _x(M), K.mlp_workspace_bytes_2s(M))
    side = torch.cuda.Stream()
    sync = [torch.cuda.Event() for _ in range(10)]
    dw_2 = K.mlp_bwd(w, M, _gup(M), ws2, wgrad_stream=side, sync=sync)
    torch.cuda.synchronize()
    assert _same_bits(dw_c, dw_2)
    assert _same_bits(dw_c, ref257[0])


def test_events_run_the_layered_launches(K, w, ref257):
    M = 257
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(32)]
    for e in ev:
        e.record()  # materialise the handles
    ws_c, ws_e = _fwd_ws(K, w, _x(M)), _fwd_ws(K, w, _x(M))
    dw_c = K.mlp_bwd(w, M, _gup(M), ws_c)
    dw_e = K.mlp_bwd(w, M, _gup(M), ws_e, events=ev)
    torch.cuda.synchronize()
    assert _same_bits(dw_c, dw_e) and torch.equal(ws_c, ws_e)
    assert _same_bits(dw_e, ref257[0])
    for i in range(8):
        assert ev[4 * i].elapsed_time(ev[4 * i + 1]) >= 0.0      # weight gradient of trunk.i
        if i >= 1:
            assert ev[4 * i + 2].elapsed_time(ev[4 * i + 3]) >= 0.0  # input gradient of trunk.i
    assert ev[2].elapsed_time(ev[3]) >= 0.0                       # the backward tail


def test_unknown_flag_bit(K, w):
    M = 257
    ws = _fwd_ws(K, w, _x(M))
    for flags in (16, K.MLP_BWD_LAYERED | 16, 1 << 20):
        with pytest.raises(ValueError, match="nerf_mlp_bwd_ex: unknown enum value"):  # NERF_E_ENUM, not NERF_E_ARG
            K.mlp_bwd(w, M, _gup(M), ws, fp32_flags=flags)
