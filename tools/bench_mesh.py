#!/usr/bin/env python3
"""Timing of the mesh extractor (csrc/mesh.hip).  A record, not a gate: there is no earlier
implementation to compare with.

  lattice   an analytic sphere field 0.6 - |x| on [-1,1]^3 at 128^3, 256^3 and 512^3: nerf_mesh_classify, the two
            nerf_exclusive_scan_i32 launches, nerf_mesh_emit (without and with grid normals) and the whole
            kernels.mesh_extract call (which adds the finiteness check, the allocations and the host read of the two
            totals), with V and F.  For the two kernels: effective bytes over time, next to the practical HBM rate
            DESIGN uses (about 5 TB/s).  Effective bytes count the field once plus the masks, counts and offsets, plus
            the vertices and faces written: classify 4P + P + 8P, emit 4P + P + 8P + 12V + 12F.
  model     InstantNGP.extract_mesh(256) on the production expert with random weights (tools/bench_ngp.py's shape),
            split into the density evaluation (density_lattice), the extraction and the field normals at the vertices.
            The threshold is the median of the lattice, so the surface is the noisy worst case of a random field.

Each figure is the device time between two events around back-to-back calls after `--warmup` untimed ones: at least
`--inner` calls, and as many as fill a window of about 40 ms where a call is short.  The median over `--rounds` rounds
is reported with the fastest and slowest; the phases are alternated inside every round.  Needs a GPU (no CPU
fallback).  Prints one JSON line and writes it to --out.

  python tools/bench_mesh.py [--sizes 128 256 512] [--rounds R] [--inner I] [--warmup W] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-sys_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PRACTICAL_TBS = 5.0
CONF = dict(hidden=64, sigma_depth=2, color_hidden=64, color_depth=2, dir_encoding="spherical",
            hash_enc_conf=dict(levels=16, features_per_level=2, log2_hashmap_size=20, min_res=16, max_res=4096,
                               interpolation="Linear"))
AABB = [[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]]


def timed(ways, rounds, inner, warmup, window_ms=40.0):
    """ways: name -> callable.  -> name -> {ms_median, ms_min, ms_max, inner}, alternating the ways inside every
    round.  A way's window holds at least `inner` calls and as many as fill about window_ms (from one probe window):
    a window of a few tens of microseconds would time the event pair and the launch gaps."""
    def window(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for f in ways.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    reps = {k: max(inner, min(2000, int(window_ms / max(window(f, inner), 1e-4)))) for k, f in ways.items()}
    ms = {k: [] for k in ways}
    for _ in range(rounds):
        for k, f in ways.items():
            ms[k].append(window(f, reps[k]))
    return {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                "inner": reps[k]} for k, v in ms.items()}


def sphere_field(n, dev):
    ax = torch.linspace(-1.0, 1.0, n, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return (0.6 - torch.sqrt(x * x + y * y + z * z)).contiguous()


def bench_lattice(n, a, dev):
    from nerf_amd import kernels as K
    from nerf_amd._lib import check, lib, ptr, stream
    L = lib()
    field = sphere_field(n, dev)
    P = n ** 3
    lo, hi = (ctypes.c_float * 3)(-1.0, -1.0, -1.0), (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    mask = torch.empty(P, dtype=torch.uint8, device=dev)
    vcnt = torch.empty(P, dtype=torch.int32, device=dev)
    fcnt = torch.empty(P, dtype=torch.int32, device=dev)
    voff = torch.empty(P + 1, dtype=torch.int32, device=dev)
    foff = torch.empty(P + 1, dtype=torch.int32, device=dev)
    wsb = int(L.nerf_scan_workspace_bytes(P))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def classify():
        check(L.nerf_mesh_classify(ptr(field), n, n, n, 0.0, ptr(mask), ptr(vcnt), ptr(fcnt), stream()), "classify")

    def scan():
        check(L.nerf_exclusive_scan_i32(ptr(vcnt), P, ptr(voff), ptr(ws), wsb, stream()), "scan")
        check(L.nerf_exclusive_scan_i32(ptr(fcnt), P, ptr(foff), ptr(ws), wsb, stream()), "scan")

    classify()
    scan()
    V, F = int(voff[-1]), int(foff[-1])
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    nrm = torch.empty((V, 3), dtype=torch.float32, device=dev)

    def emit(normals):
        check(L.nerf_mesh_emit(ptr(field), n, n, n, 0.0, lo, hi, ptr(mask), ptr(voff), ptr(foff), V, F, ptr(verts),
                               ptr(faces), ptr(nrm) if normals else None, stream()), "emit")

    emit(True)
    ref = K.mesh_extract(field, 0.0, [-1.0] * 3, [1.0] * 3, normals=True)
    same = bool(torch.equal(ref[0], verts) and torch.equal(ref[1], faces) and torch.equal(ref[2], nrm))
    res = timed({"classify": classify, "scan_x2": scan, "emit": lambda: emit(False),
                 "emit_grid_normals": lambda: emit(True),
                 "mesh_extract": lambda: K.mesh_extract(field, 0.0, [-1.0] * 3, [1.0] * 3)}, a.rounds, a.inner, a.warmup)
    res["kernels_total_ms_median"] = round(sum(res[k]["ms_median"] for k in ("classify", "scan_x2", "emit")), 4)
    eff = {"classify": 13 * P, "emit": 13 * P + 12 * V + 12 * F}
    for k, b in eff.items():
        res[k]["effective_bytes"] = b
        res[k]["effective_tb_per_s"] = round(b / (res[k]["ms_median"] * 1e-3) / 1e12, 3)
        res[k]["of_practical_hbm"] = round(res[k]["effective_tb_per_s"] / HBM_PRACTICAL_TBS, 3)
    res.update({"n": n, "points": P, "vertices": V, "faces": F, "pieces_equal_mesh_extract": same})
    return res


def bench_model(a, dev):
    from nerf_amd import kernels as K
    from nerf_amd.mesh import density_lattice
    from nerf_amd.ngp import InstantNGP
    torch.manual_seed(0)
    net = InstantNGP(occ_conf={}, scene_box=torch.tensor(AABB), **CONF)
    with torch.no_grad():
        net.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    net = net.to(dev).eval()
    lo, hi, n = AABB[0], AABB[1], a.model_resolution
    field = density_lattice(net.density, lo, hi, n)
    thr = float(field.median())
    verts, faces = K.mesh_extract(field, thr, lo, hi)
    res = timed({"density_lattice": lambda: density_lattice(net.density, lo, hi, n),
                 "mesh_extract": lambda: K.mesh_extract(field, thr, lo, hi),
                 "field_normals": lambda: net.normals(verts),
                 "extract_mesh_total": lambda: net.extract_mesh(resolution=n, threshold=thr, normals="field")},
                a.rounds, max(1, a.inner // 2), max(1, a.warmup // 2))
    res.update({"resolution": n, "threshold_median_sigma": thr, "vertices": int(verts.shape[0]),
                "faces": int(faces.shape[0])})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--model-resolution", type=int, default=256)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_extract.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh: needs a GPU (timings on a CPU say nothing about the MI355X)")
    dev = torch.device("cuda:0")
    res = {"bench": "mesh_extract", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
           "hbm_practical_tb_per_s": HBM_PRACTICAL_TBS, "lattice": [bench_lattice(n, a, dev) for n in a.sizes]}
    if not a.no_model:
        res["model"] = bench_model(a, dev)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
