"""The yardsticks of the density-gradient tests, checked on the CPU: the oracle's autograd of the hash encoding
against a closed-form answer, and the share of the GPU test's samples that sit on a ReLU kink (where d sigma / d x
jumps, so fp32 implementations with different summation orders may legitimately land on different sides)."""
import pytest
import torch

import ngp_grad_cases as C
from oracle import ngp_oracle as NO


@pytest.mark.parametrize("interp", ["Linear", "Smoothstep"])
def test_oracle_hash_jacobian_known_answer(interp):
    """Table linear in the vertex -> autograd of the oracle's hash_encode gives r A[f] (Linear) and
    r A[f] 6 w (1 - w) (Smoothstep).  Measured deviations 1e-6 / 1.5e-6; bound 1e-5."""
    table, h = C.known_answer_table()
    assert h.unique().numel() == 125
    res, _ = NO.hash_resolutions(C.KA["levels"], C.KA["min_res"], C.KA["max_res"])
    assert res.tolist() == [4]
    x = C.known_answer_points().requires_grad_(True)
    y = NO.hash_encode(table, x, res, C.KA["log2_hashmap_size"], 2, interp)
    J = torch.stack([torch.autograd.grad(y[:, f].sum(), x, retain_graph=True)[0] for f in range(2)], 1)
    err = (J - C.known_answer_jacobian(x.detach(), interp)).abs().max().item()
    print(f"known answer {interp}: max deviation {err:.3g}")
    assert err <= 1e-5


def test_kink_share_of_gpu_inputs():
    """The GPU test's production-shape inputs: at most 2 % of the samples have a trunk pre-activation within 1e-5 of
    its kink in the fp32 oracle (those are the only samples its oracle comparison may leave out)."""
    st = C.prod_state()
    _, g, zmin = C.oracle_density(st, C.prod_points(), C.PROD["hash_enc_conf"], C.AABB)
    share = (zmin < C.KINK).float().mean().item()
    print(f"kink share {100 * share:.2f} %")
    assert torch.isfinite(g).all()
    assert share <= 0.02
