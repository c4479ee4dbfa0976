#!/usr/bin/env python3
"""Timing of the exact point-to-surface distance (csrc/mesh_distance.hip) next to the point-set
distance of §3.11.4 on the same inputs in the same run.  A record, not a gate.

  mesh      the sphere mesh of tools/bench_mesh.py (0.6 - |x| on [-1,1]^3 at --size^3; 320 gives about 1 M faces); the
            other surface is the mesh after simplify(2 lattice spacings).
  phases    counts             nerf_mesh_face_cell_counts
            keys               nerf_mesh_face_cell_keys at the offsets of those counts
            sort               torch.sort of the keys
            face_grid          kernels.mesh_face_grid as a whole (box read, range check, counts, cumsum and its total,
                               keys, sort)
            nearest_sorted     kernels.mesh_nearest_faces of --samples samples of the other surface, queries in cell order
            nearest_unsorted   the same with sort_queries=False
            distance_exact     mesh_metrics.mesh_distance(exact=True) end to end at --samples per mesh
            distance_point_set mesh_metrics.mesh_distance(exact=False) on the same meshes: the yardstick
  counts    keys_per_face = n_keys / F of both meshes, and the mean number of faces measured per query
            (evaluations_per_query, from a host restatement of the shells over a sample of --probe queries: the share
            of the query time that goes to faces met more than once or to shells without a nearer face shows here).

Each figure is the time between two events around back-to-back calls after `--warmup` untimed ones; the median over
`--rounds` rounds is reported with the fastest and slowest; the phases are alternated inside every round.  Needs a GPU
(no CPU fallback).  Prints one JSON line and writes it to --out.

  python tools/bench_mesh_distance.py [--size 320] [--samples N] [--rounds R] [--out FILE]
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


def evaluations_per_query(grid, query, d2, probe):
    """The faces one query measures, counted on the host for ``probe`` queries: the keys of every cell within the
    Chebyshev radius the search reaches, which is the first r >= 2 at which the stopping rule holds for the final d2
    (the search cannot stop earlier; it may stop one shell later while its best is not yet the final one)."""
    import numpy as np
    nx, ny, nz = grid["dims"]
    per_cell = torch.bincount(grid["keys"] >> 32, minlength=nx * ny * nz).reshape(nx, ny, nz).cpu().numpy()
    lo, inv, cell = np.float32(grid["lo"]), np.float32(grid["inv"]), float(grid["cell"])
    q = query[:probe].cpu().numpy()
    best = d2[:probe].cpu().numpy()
    total, shells = 0, 0
    for i in range(len(q)):
        c = [int(min(max(np.floor((q[i, k] - lo[k]) * inv), 0), n - 1)) for k, n in enumerate((nx, ny, nz))]
        r = 2
        while r < max(nx, ny, nz) and not best[i] <= (((r - 1) - 0.00390625) * cell) ** 2 * (1 - 0.0009765625):
            r += 1
        r -= 1  # the last shell searched
        box = [slice(max(c[k] - r, 0), min(c[k] + r, n - 1) + 1) for k, n in enumerate((nx, ny, nz))]
        total += int(per_cell[box[0], box[1], box[2]].sum())
        shells += r + 1
    return total / max(len(q), 1), shells / max(len(q), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=320)
    ap.add_argument("--samples", type=int, default=2 ** 18)
    ap.add_argument("--probe", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_distance.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_distance: needs a GPU (timings on a CPU say nothing about the MI355X)")
    dev = torch.device("cuda:0")
    from nerf_amd import Mesh, mesh_distance
    from nerf_amd import kernels as K
    from nerf_amd._lib import check, lib, ptr, stream
    L = lib()
    mesh = Mesh(*K.mesh_extract(sphere_field(a.size, dev), 0.0, [-1.0] * 3, [1.0] * 3))
    other = mesh.simplify(2 * 2.0 / (a.size - 1))
    v, f = mesh.vertices, mesh.faces
    F, n = int(f.shape[0]), a.samples
    query = other.sample_surface(n)[0]
    grid = K.mesh_face_grid(v, f)
    other_grid = K.mesh_face_grid(other.vertices, other.faces)
    lo_c, dims_c = (ctypes.c_float * 3)(*grid["lo"]), (ctypes.c_int32 * 3)(*grid["dims"])
    counts = torch.empty(F, dtype=torch.int64, device=dev)
    keys = torch.empty(grid["n_keys"], dtype=torch.int64, device=dev)

    def counts_kernel():
        check(L.nerf_mesh_face_cell_counts(ptr(v), ptr(f), F, lo_c, grid["inv"], dims_c, ptr(counts), stream()), "counts")

    counts_kernel()
    offsets = torch.cumsum(counts, 0) - counts

    def keys_kernel():
        check(L.nerf_mesh_face_cell_keys(ptr(v), ptr(f), F, lo_c, grid["inv"], dims_c, ptr(offsets), ptr(keys),
                                         stream()), "keys")

    keys_kernel()
    ways = {"counts": counts_kernel, "keys": keys_kernel, "sort": lambda: torch.sort(keys),
            "face_grid": lambda: K.mesh_face_grid(v, f),
            "nearest_sorted": lambda: K.mesh_nearest_faces(query, v, f, grid, finite_checked=True),
            "nearest_unsorted": lambda: K.mesh_nearest_faces(query, v, f, grid, sort_queries=False, finite_checked=True),
            "distance_exact": lambda: mesh_distance(mesh, other, n, exact=True),
            "distance_point_set": lambda: mesh_distance(mesh, other, n)}
    res = timed(ways, a.rounds, a.inner, a.warmup)
    s = K.mesh_nearest_faces(query, v, f, grid)
    u = K.mesh_nearest_faces(query, v, f, grid, sort_queries=False)
    exact, point_set = mesh_distance(mesh, other, n, exact=True), mesh_distance(mesh, other, n)
    evals, shells = evaluations_per_query(grid, query, s[0], a.probe)
    res.update({"bench": "mesh_distance", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
                "size": a.size, "vertices": int(v.shape[0]), "faces": F, "other_faces": int(other.faces.shape[0]),
                "samples": n, "cell": grid["cell"], "dims": grid["dims"], "n_keys": grid["n_keys"],
                "keys_per_face": grid["n_keys"] / F, "other_keys_per_face": other_grid["n_keys"] / other_grid["F"],
                "evaluations_per_query": evals, "shells_per_query": shells,
                "sorted_equals_unsorted": all(bool(torch.equal(x, y)) for x, y in zip(s, u)),
                "exact_over_point_set": res["distance_exact"]["ms_median"] / res["distance_point_set"]["ms_median"],
                "chamfer_exact": exact["chamfer"], "chamfer_point_set": point_set["chamfer"],
                "hausdorff_exact": exact["hausdorff"], "hausdorff_point_set": point_set["hausdorff"]})
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
