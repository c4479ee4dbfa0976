"""Shared inputs and the CPU reference of the density-gradient tests (test_ngp_grad_reference.py on the CPU,
test_gpu_ngp_grad.py on the GPU): the known-answer grid, the production-shape expert with fixed seeds, and the fp32
oracle's sigma, d sigma / d x and ReLU margins.  Everything here is plain torch on the CPU."""
import math
from collections import OrderedDict

import torch

from oracle import ngp_oracle as NO

# ---- known-answer grid: one level of resolution 4, table entry of vertex v = A v, so enc_f(p) = A[f] . (4 p) inside
# every cell (Linear) and the encoding's Jacobian is 4 A[f] (Linear) or 4 A[f] 6 w (1 - w) per axis (Smoothstep)
KA = dict(levels=1, min_res=4, max_res=4, log2_hashmap_size=12, features_per_level=2)
KA_A = torch.tensor([[0.5, -0.25, 0.125], [-1.0, 0.75, 0.375]])


def known_answer_table():
    """-> (table (4096, 2), the 125 vertex hashes)."""
    v = torch.stack(torch.meshgrid(*([torch.arange(5)] * 3), indexing="ij"), -1).reshape(-1, 3)
    h = NO.hash_index(v[:, 0], v[:, 1], v[:, 2], KA["log2_hashmap_size"])
    table = torch.zeros(2 ** KA["log2_hashmap_size"], 2)
    table[h] = v.float() @ KA_A.t()
    return table, h


def known_answer_points(M=64, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(M, 3, generator=g) * 0.98 + 0.01


def known_answer_jacobian(x01, interpolation):
    """(M, 2, 3): d enc[f] / d p[c] in closed form."""
    J = (4.0 * KA_A).expand(x01.shape[0], 2, 3).clone()
    if interpolation == "Smoothstep":
        w = x01 * 4.0 - torch.floor(x01 * 4.0)
        J = J * (6.0 * w * (1.0 - w))[:, None, :]
    return J


# ---- the production-shape expert (16 levels x 2 features, 2 x 64 sigma trunk, 1 + 15 head, SH colour input)
PROD = dict(hidden=64, sigma_depth=2, color_hidden=64, color_depth=2, dir_encoding="spherical",
            hash_enc_conf=dict(levels=16, features_per_level=2, log2_hashmap_size=14, min_res=16, max_res=2048,
                               interpolation="Linear"))
AABB = torch.tensor([[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]])
PROD_M = 4096
KINK = 1e-5  # a sample is low-margin when some trunk pre-activation is closer than this to its ReLU kink


def prod_state(seed=1234, table_scale=0.5):
    """Parameters by name (torch's default nn.Linear init: U(+-1/sqrt(fan_in)) for weights and biases; sigma_head.bias
    -1 as MetaNGP's constructor sets it) and the hash table U(+-table_scale)."""
    g = torch.Generator().manual_seed(seed)
    hc = PROD["hash_enc_conf"]
    st = OrderedDict()
    st["xyz_encoder.hash_table"] = (torch.rand(hc["levels"] * 2 ** hc["log2_hashmap_size"], hc["features_per_level"],
                                               generator=g) * 2 - 1) * table_scale
    shapes = NO.ngp_param_shapes(hc["levels"] * hc["features_per_level"], PROD["hidden"], PROD["sigma_depth"], 15,
                                 PROD["color_hidden"], PROD["color_depth"], 16)
    for name, shp in shapes.items():
        fan_in = shp[1] if len(shp) == 2 else shapes[name[:-4] + "weight"][1]
        st[name] = (torch.rand(*shp, generator=g) * 2 - 1) / math.sqrt(fan_in)
    st["sigma_head.bias"] = torch.full((1,), -1.0)
    return st


def prod_points(M=PROD_M, seed=99):
    """World points drawn 5 % beyond the box on every side."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(M, 3, generator=g) * 2 - 1) * (1.5 * 1.05)


def oracle_density(state, x, hash_conf, aabb, sigma_depth=2, enc_eps=1e-6):
    """MetaNGP.density in the oracle's fp32 torch ops -> (sigma (M,), d sigma / d x (M, 3) by autograd, the smallest
    |trunk pre-activation| per sample (M,))."""
    x = x.detach().clone().requires_grad_(True)
    res, _ = NO.hash_resolutions(hash_conf["levels"], hash_conf["min_res"], hash_conf["max_res"])
    x01 = ((x - aabb[0]) / (aabb[1] - aabb[0])).clamp(enc_eps, 1.0 - enc_eps)
    h = NO.hash_encode(state["xyz_encoder.hash_table"], x01, res, hash_conf["log2_hashmap_size"],
                       hash_conf["features_per_level"], hash_conf.get("interpolation", "Linear"))
    zs = []
    for i in range(sigma_depth):
        zs.append(NO._lin(h, state, f"sigma_trunk.{i}.linear"))
        h = torch.relu(zs[-1])
    sigma = NO._TruncExp.apply(NO._lin(h, state, "sigma_head"))[:, 0]
    (g,) = torch.autograd.grad(sigma.sum(), x)
    return sigma.detach(), g, torch.cat(zs, -1).detach().abs().min(-1).values
