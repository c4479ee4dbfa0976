#!/usr/bin/env python3
"""Timing of sigma + d sigma / d x at world points on the production Instant-NGP expert (16-level hash grid, F = 2,
2^20 entries per level, max_res 4096, 2 x 64 sigma trunk; tools/bench_ngp.py's expert), M = 2^20 points uniform in
the scene box.  Three ways, alternated inside every round so that drift of the machine hits all of them alike:

  density_enc   nerf_ngp_density_enc alone (sigma only, no gradient): the floor
  composed      hash_encode -> ngp_density -> ngp_bwd(d_rgb_sigma = [0,0,0,1]) -> hash_encode_bwd_x
  fused         nerf_ngp_density_grad_enc, one launch (plus the small weight transpose)

Each figure is the device time between two events around `--inner` back-to-back calls, after `--warmup` untimed
calls of each way; the median over `--rounds` rounds is reported with the fastest and slowest round.  Needs a GPU (no
CPU fallback).  Prints one JSON line and writes it to --out.

  python tools/bench_density_grad.py [--points N] [--rounds R] [--inner I] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-sys_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CONF = dict(hidden=64, sigma_depth=2, color_hidden=64, color_depth=2, dir_encoding="spherical",
            hash_enc_conf=dict(levels=16, features_per_level=2, log2_hashmap_size=20, min_res=16, max_res=4096,
                               interpolation="Linear"))
AABB = [[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_grad.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_density_grad: needs a GPU (timings on a CPU say nothing about the MI355X)")
    from nerf_amd import ngp as N
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = N.InstantNGP(occ_conf={}, scene_box=torch.tensor(AABB), **CONF)
    with torch.no_grad():
        net.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    net = net.to(dev).eval()
    x = ((torch.rand(a.points, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1) * 1.5).to(dev)
    with torch.no_grad():
        w = net.packed().detach()
        table = net.xyz_encoder.hash_table.detach()
    g, ns, ab, eps = net.xyz_encoder.grid, net.net_struct, net._aabb_host, net._eps

    ways = {
        "density_enc": lambda: N.ngp_density_enc(ns, g, table, w, x, ab, eps),
        "composed": lambda: net._density_grad_composed(x, w, table),
        "fused": lambda: N.ngp_density_grad_enc(ns, g, table, w, x, ab, eps),
    }
    with torch.no_grad():
        assert ways["fused"]() is not None and ways["density_enc"]() is not None, "not the production shape"
        sig_f, grad_f = ways["fused"]()
        sig_c, grad_c = ways["composed"]()
        sig_d = ways["density_enc"]()
        same = dict(sigma_bitwise_density_enc=bool(torch.equal(sig_f, sig_d)),
                    sigma_bitwise_composed=bool(torch.equal(sig_f, sig_c)),
                    grad_bitwise_composed=bool(torch.equal(grad_f, grad_c)),
                    grad_max_abs_diff=float((grad_f - grad_c).abs().max()), grad_max_abs=float(grad_c.abs().max()))
        for f in ways.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, f in ways.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.inner)
    res = {"bench": "density_grad", "points": a.points, "rounds": a.rounds, "inner": a.inner,
           "device": torch.cuda.get_device_name(0), "outputs": same}
    for k, v in ms.items():
        med = statistics.median(v)
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                  "mpoints_per_s": round(a.points / med / 1e3, 1)}
    res["fused_over_composed"] = round(res["fused"]["ms_median"] / res["composed"]["ms_median"], 3)
    res["fused_over_density_enc"] = round(res["fused"]["ms_median"] / res["density_enc"]["ms_median"], 3)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
