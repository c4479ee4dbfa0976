#!/usr/bin/env python3
"""Timing of the mesh smoothing (csrc/mesh_smooth.hip).  A record, not a gate: there is no earlier
implementation to compare with.

  meshes    the sphere meshes of tools/bench_mesh.py (0.6 - |x| on [-1,1]^3 at 128^3, 256^3 and 512^3) and the
            many-component noise mesh of tools/bench_mesh_clean.py (128^3, threshold 0.8), each with grid normals.
  phases    keys               nerf_mesh_pair_keys, mode 0 (the 6 F directed pairs)
            sort               torch.sort of those keys
            flags_scan_build   nerf_mesh_csr_flags with the boundary flags, nerf_exclusive_scan_i32, nerf_mesh_csr_build
            adjacency          kernels.mesh_adjacency(boundary=True) as a whole (with its host read of E)
            smooth_pass        one nerf_mesh_smooth_pass with the boundary mask
            compute_normals    Mesh.compute_normals: the vertex-to-face adjacency and nerf_mesh_vertex_normals
            vertex_normals     nerf_mesh_vertex_normals alone
            smooth10           Mesh.smooth(10) end to end: the checks, the adjacency, 20 passes, the normals
  bytes     for one pass the traffic the method implies at the least: per vertex its row bounds (8, counting both
            ends), its own position read and written (24), per entry the column index and the 12-byte neighbour
            position (16 E): 32 V + 16 E, E about 6 V on a closed surface; next to the practical HBM rate DESIGN uses
            (about 5 TB/s).  The neighbour reads are gathers that mostly hit the cache, so this is a floor for the
            bytes, not a model of the time.

Each figure is the time between two events around back-to-back calls after `--warmup` untimed ones: at least
`--inner` calls, and as many as fill a window of about 40 ms where a call is short.  The median over `--rounds` rounds
is reported with the fastest and slowest; the phases are alternated inside every round.  Needs a GPU (no CPU fallback).
Prints one JSON line and writes it to --out.

  python tools/bench_mesh_smooth.py [--sizes 128 256 512] [--noise-size 128] [--rounds R] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-sys_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_mesh import HBM_PRACTICAL_TBS, sphere_field, timed  # noqa: E402


def bench_one(name, field, iso, a, dev):
    from nerf_amd import Mesh
    from nerf_amd import kernels as K
    from nerf_amd._lib import check, lib, ptr, stream
    L = lib()
    mesh = Mesh(*K.mesh_extract(field, iso, [-1.0] * 3, [1.0] * 3, normals=True))
    del field
    v, f = mesh.vertices, mesh.faces
    V, F = int(v.shape[0]), int(f.shape[0])
    n = 6 * F
    row_off, col, boundary = K.mesh_adjacency(f, V, boundary=True)
    E = int(col.shape[0])
    frow, fcol = K.mesh_vertex_faces(f, V)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    check(L.nerf_mesh_pair_keys(ptr(f), F, 0, ptr(keys), stream()), "keys")
    sorted_keys = torch.sort(keys).values
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    pos = torch.empty(n + 1, dtype=torch.int32, device=dev)
    wsb = int(L.nerf_scan_workspace_bytes(n))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    bnd = torch.zeros(V, dtype=torch.uint8, device=dev)
    row2, col2 = torch.empty_like(row_off), torch.empty_like(col)
    out, nrm = torch.empty_like(v), torch.empty_like(v)

    def keys_kernel():
        check(L.nerf_mesh_pair_keys(ptr(f), F, 0, ptr(keys), stream()), "keys")

    def flags_scan_build():
        bnd.zero_()
        check(L.nerf_mesh_csr_flags(ptr(sorted_keys), n, ptr(flags), ptr(bnd), stream()), "flags")
        check(L.nerf_exclusive_scan_i32(ptr(flags), n, ptr(pos), ptr(ws), wsb, stream()), "scan")
        check(L.nerf_mesh_csr_build(ptr(sorted_keys), n, ptr(flags), ptr(pos), V, E, ptr(row2), ptr(col2), stream()),
              "build")

    def smooth_pass():
        check(L.nerf_mesh_smooth_pass(ptr(v), ptr(row_off), ptr(col), ptr(boundary), V, 0.5, ptr(out), stream()), "pass")

    def vertex_normals():
        check(L.nerf_mesh_vertex_normals(ptr(v), ptr(f), ptr(frow), ptr(fcol), V, ptr(nrm), stream()), "normals")

    flags_scan_build()
    same = bool(torch.equal(row2, row_off) and torch.equal(col2, col) and torch.equal(bnd, boundary))
    res = timed({"keys": keys_kernel, "sort": lambda: torch.sort(keys), "flags_scan_build": flags_scan_build,
                 "adjacency": lambda: K.mesh_adjacency(f, V, boundary=True, ranges_checked=True),
                 "smooth_pass": smooth_pass, "compute_normals": mesh.compute_normals,
                 "vertex_normals": vertex_normals, "smooth10": lambda: mesh.smooth(10)},
                a.rounds, a.inner, a.warmup)
    b = 32 * V + 16 * E
    res["smooth_pass"]["effective_bytes"] = b
    res["smooth_pass"]["effective_tb_per_s"] = round(b / (res["smooth_pass"]["ms_median"] * 1e-3) / 1e12, 4)
    res["smooth_pass"]["of_practical_hbm"] = round(res["smooth_pass"]["effective_tb_per_s"] / HBM_PRACTICAL_TBS, 4)
    deg = row_off[1:] - row_off[:-1]
    res.update({"mesh": name, "vertices": V, "faces": F, "entries": E, "entries_per_vertex": round(E / max(V, 1), 3),
                "longest_row": int(deg.max()), "boundary_vertices": int(boundary.sum()),
                "face_entries": int(fcol.shape[0]), "pieces_equal_adjacency": same})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--noise-size", type=int, default=128)
    ap.add_argument("--noise-threshold", type=float, default=0.8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_smooth: needs a GPU (timings on a CPU say nothing about the MI355X)")
    dev = torch.device("cuda:0")
    runs = [bench_one(f"sphere{n}", sphere_field(n, dev), 0.0, a, dev) for n in a.sizes]
    if a.noise_size:
        n = a.noise_size
        g = torch.Generator(device="cpu").manual_seed(18)
        noise = (torch.rand((n, n, n), generator=g) * 2.0 - 1.0).to(dev).contiguous()
        runs.append(bench_one(f"noise{n}", noise, a.noise_threshold, a, dev))
    res = {"bench": "mesh_smooth", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
           "hbm_practical_tb_per_s": HBM_PRACTICAL_TBS, "meshes": runs}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
