"""The chained fp32 trunk forward (-m gpu; gemm_nt_x6w_chain_kernel in nerf-sys_amd/csrc/gemm_x6.hpp): one launch
carries every 256-row tile through the eight trunk layers.  It runs the per-layer kernel's tile code once per layer, so
it must agree BITWISE with the eight per-layer launches (MLP_FWD_LAYERED) — outputs, every saved activation and ReLU
mask word, and the weight gradients a backward computes from them.  Sizes: one partial tile, the tile edge (255, 256,
257) and 256 (CU count + 1) + 1 rows, which puts a second tile on at least one CU.  The eval forward (ping-pong
buffers) is the case where a tile overwrites addresses its CU read two layers earlier.  Workspaces are zero-filled first
(mlp_workspace is torch.empty), so the whole buffers — padded rows included — can be compared as bytes."""
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


def _same_bits(a, b):
    """Bitwise: torch.equal on floats takes -0.0 for 0.0."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _fwd(K, w, x, training, flags, events=None):
    ws = K.mlp_workspace(x.shape[0], training, DEV).zero_()
    out = K.mlp_fwd(w, x, ws, training, fp32_flags=flags, events=events)
    return out, ws


@pytest.mark.parametrize("i", range(5), ids=["M1", "M255", "M256", "M257", "cu_count_plus_1_tiles"])
def test_training_forward_bitwise(K, w, i):
    x = _x(_sizes()[i])
    out_c, ws_c = _fwd(K, w, x, True, 0)
    out_l, ws_l = _fwd(K, w, x, True, K.MLP_FWD_LAYERED)
    assert torch.isfinite(out_c).all() and out_c.abs().max().item() > 0
    assert _same_bits(out_c, out_l), "rgb_sigma differs"
    assert torch.equal(ws_c, ws_l), "workspace (saved activations / masks / HO / CIN / C0) differs"


@pytest.mark.parametrize("i", range(5), ids=["M1", "M255", "M256", "M257", "cu_count_plus_1_tiles"])
def test_eval_forward_bitwise(K, w, i):
    x = _x(_sizes()[i])
    out_c, _ = _fwd(K, w, x, False, 0)
    out_l, _ = _fwd(K, w, x, False, K.MLP_FWD_LAYERED)
    assert torch.isfinite(out_c).all() and out_c.abs().max().item() > 0
    assert _same_bits(out_c, out_l), "rgb_sigma differs"


def test_backward_bitwise(K, w):
    M = 257
    x = _x(M)
    gup = torch.randn(M, 4, generator=torch.Generator().manual_seed(M + 1)).to(DEV) * 1e-3
    _, ws_c = _fwd(K, w, x, True, 0)
    _, ws_l = _fwd(K, w, x, True, K.MLP_FWD_LAYERED)
    dw_c = K.mlp_bwd(w, M, gup, ws_c)
    dw_l = K.mlp_bwd(w, M, gup, ws_l, fp32_flags=K.MLP_FWD_LAYERED)  # a forward-only flag: mlp_bwd drops it
    assert dw_c.abs().max().item() > 0
    assert _same_bits(dw_c, dw_l)


def test_events_run_the_layered_launches(K, w):
    M = 257
    x = _x(M)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(16)]
    for e in ev:
        e.record()  # materialise the handles
    out_c, ws_c = _fwd(K, w, x, True, 0)
    out_e, ws_e = _fwd(K, w, x, True, 0, events=ev)
    torch.cuda.synchronize()
    assert _same_bits(out_c, out_e) and torch.equal(ws_c, ws_e)
    for i in range(8):
        assert ev[2 * i].elapsed_time(ev[2 * i + 1]) >= 0.0


def test_unknown_flag_bit(K, w):
    x = _x(257)
    ws = K.mlp_workspace(257, True, DEV)
    for flags in (8, K.MLP_FWD_LAYERED | 8, 1 << 20):
        with pytest.raises(ValueError, match="nerf_mlp_fwd_ex: unknown enum value"):  # NERF_E_ENUM, not NERF_E_ARG
            K.mlp_fwd(w, x, ws, True, fp32_flags=flags)
