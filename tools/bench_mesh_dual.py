#!/usr/bin/env python3
"""Timing of dual contouring (csrc/mesh_dual.hip) next to marching tetrahedra on the same field in
the same run.  A record, not a gate: no speed ratio is required of either method.

  lattice   an analytic sphere field 0.6 - |x| on [-1,1]^3 at 256^3 and 512^3 (tools/bench_mesh.py's field):
            nerf_mesh_dual_classify, the three nerf_exclusive_scan_i32 launches, nerf_mesh_dual_edges (with grid
            normals and keys), nerf_mesh_dual_cells ("qef" and "mean"), the whole kernels.mesh_extract_dual call (which
            adds the finiteness checks, the allocations and the host read of the three totals) and, alternating with
            them in every round, kernels.mesh_extract.  E, V and F of dual contouring and V and F of marching
            tetrahedra.
  fallback  the share of active cells whose "qef" solve kept the mean, at tol = 1e-3, 1e-2 and 1e-1, on the sphere and
            on a smooth-noise field (a sum of sines, iso 0.2) at the same sizes.

Each figure is the device time between two events around back-to-back calls after `--warmup` untimed ones: at least
`--inner` calls, and as many as fill a window of about 40 ms where a call is short.  The median over `--rounds` rounds
is reported with the fastest and slowest; the ways are alternated inside every round.  Needs a GPU (no CPU fallback).
Prints one JSON line and writes it to --out.

  python tools/bench_mesh_dual.py [--sizes 256 512] [--rounds R] [--inner I] [--warmup W] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-sys_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_mesh import sphere_field, timed  # noqa: E402

TOLS = (1e-3, 1e-2, 1e-1)
BOX = ([-1.0] * 3, [1.0] * 3)


def sines_field(n, dev):
    ax = torch.linspace(-1.0, 1.0, n, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return (torch.sin(2.3 * x + 0.4) + torch.sin(3.1 * y - 0.7) * torch.cos(1.7 * z)
            + 0.5 * torch.sin(4.0 * x * z + 1.1)).contiguous()


def fallback_shares(K, field, iso):
    rec, pts, nrm, _ = K.mesh_dual_hermite(field, iso, *BOX)
    out = {"cells": rec.V}
    for tol in TOLS:
        fb = K.mesh_dual_vertices(rec, pts, nrm, tol=tol, return_fallback=True)[2]
        out[f"tol_{tol:g}"] = round(float(fb.sum()) / max(rec.V, 1), 5)
    return out


def bench_lattice(n, a, dev):
    from nerf_amd import kernels as K
    from nerf_amd._lib import check, lib, ptr, stream
    L = lib()
    field = sphere_field(n, dev)
    P = n ** 3
    lo, hi = (ctypes.c_float * 3)(-1.0, -1.0, -1.0), (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    mask = torch.empty(P, dtype=torch.uint8, device=dev)
    cnt = [torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3)]
    off = [torch.empty(P + 1, dtype=torch.int32, device=dev) for _ in range(3)]
    wsb = int(L.nerf_scan_workspace_bytes(P))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def classify():
        check(L.nerf_mesh_dual_classify(ptr(field), n, n, n, 0.0, ptr(mask), ptr(cnt[0]), ptr(cnt[1]), ptr(cnt[2]),
                                        stream()), "classify")

    def scan():
        for c, o in zip(cnt, off):
            check(L.nerf_exclusive_scan_i32(ptr(c), P, ptr(o), ptr(ws), wsb, stream()), "scan")

    classify()
    scan()
    E, V, F = (int(o[-1]) for o in off)
    pts = torch.empty((E, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((E, 3), dtype=torch.float32, device=dev)
    keys = torch.empty(E, dtype=torch.int32, device=dev)
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    fb = torch.empty(V, dtype=torch.uint8, device=dev)

    def edges():
        check(L.nerf_mesh_dual_edges(ptr(field), n, n, n, 0.0, lo, hi, ptr(mask), ptr(off[0]), E, ptr(pts), ptr(nrm),
                                     ptr(keys), stream()), "edges")

    def cells(placement):
        check(L.nerf_mesh_dual_cells(ptr(field), n, n, n, 0.0, lo, hi, ptr(mask), ptr(off[0]), ptr(off[1]), ptr(off[2]),
                                     ptr(pts), ptr(nrm), placement, 1e-3, V, F, ptr(verts), ptr(faces), None, ptr(fb),
                                     stream()), "cells")

    edges()
    cells(1)
    ref = K.mesh_extract_dual(field, 0.0, *BOX)
    same = bool(torch.equal(ref[0], verts) and torch.equal(ref[1], faces))
    tv, tf = K.mesh_extract(field, 0.0, *BOX)
    res = timed({"classify": classify, "scan_x3": scan, "edges": edges, "cells_qef": lambda: cells(1),
                 "cells_mean": lambda: cells(0), "mesh_extract_dual": lambda: K.mesh_extract_dual(field, 0.0, *BOX),
                 "mesh_extract_tets": lambda: K.mesh_extract(field, 0.0, *BOX)}, a.rounds, a.inner, a.warmup)
    res["kernels_total_ms_median"] = round(sum(res[k]["ms_median"] for k in ("classify", "scan_x3", "edges", "cells_qef")), 4)
    res.update({"n": n, "points": P, "dual": {"edges": E, "vertices": V, "faces": F},
                "tets": {"vertices": int(tv.shape[0]), "faces": int(tf.shape[0])},
                "pieces_equal_mesh_extract_dual": same,
                "fallback_share": {"sphere": fallback_shares(K, field, 0.0),
                                   "sines": fallback_shares(K, sines_field(n, dev), 0.2)}})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_dual.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_dual: needs a GPU (timings on a CPU say nothing about the MI355X)")
    dev = torch.device("cuda:0")
    res = {"bench": "mesh_dual", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
           "tols": list(TOLS), "lattice": [bench_lattice(n, a, dev) for n in a.sizes]}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
