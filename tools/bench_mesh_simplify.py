#!/usr/bin/env python3
"""Timing of the mesh simplification by vertex clustering (csrc/mesh_simplify.hip).  A record, not a
gate: there is no earlier implementation to compare with.

  meshes    the sphere meshes of tools/bench_mesh.py (0.6 - |x| on [-1,1]^3 at 128^3, 256^3 and 512^3) and the
            many-component noise mesh of tools/bench_mesh_clean.py (128^3, threshold 0.8), each with grid normals,
            clustered with cells of `--factor` lattice spacings (default 2), with V and F before and after.
  phases    labels_kernels     nerf_mesh_cluster_labels alone (keys, insert, lookup: 3 launches + 2 memsets)
            reduce_kernels     nerf_mesh_cluster_reduce alone, positions + normals (init, accumulate, finalize)
            faces_kernels      nerf_mesh_cluster_faces alone (remap, insert, lookup: 3 launches + 2 memsets)
            compact            kernels.mesh_compact of the clustered vertices, remapped faces and keep flags
            simplify           Mesh.simplify as a whole (the min / max read, two status reads, the compaction's read)
            filter_components  Mesh.filter_components(min_faces=...) on the same mesh, for context
            with --placement quadric ("Quadric placement"), on the same meshes by the same method:
            csr_build          kernels.mesh_vertex_faces of the remapped faces (keys, torch.sort, flags, scan, one
                               host read, row build): the lists of faces per cluster
            quadric_kernel     nerf_mesh_cluster_quadric alone (one launch)
            simplify_quadric   Mesh.simplify(placement="quadric") as a whole, next to ``simplify`` (the mean placement,
                               which is what Mesh.simplify did before the option existed)
  bytes     for the three kernel groups the traffic the method implies at the least, next to the practical HBM rate
            DESIGN uses (about 5 TB/s).  labels: 12 V read, keys written and read twice (24 V), the table cleared and
            one slot per vertex touched twice (4 T + 8 V), labels written (4 V): 48 V + 4 T.  reduce with normals:
            the accumulators cleared and read (2 x 52 V), the inputs read (28 V + 16 V), 24 V written: 172 V.  faces: 12 F
            read, 12 F labels, 12 F written and read twice (36 F), table 4 T + 8 F, keep F: 69 F + 4 T.  The inserts
            and lookups are dependent 4-byte and 8-byte loads, so these are floors for the bytes, not models of the time.

Each figure is the time between two events around back-to-back calls after `--warmup` untimed ones: at least
`--inner` calls, and as many as fill a window of about 40 ms where a call is short.  The median over `--rounds` rounds
is reported with the fastest and slowest; the phases are alternated inside every round.  Needs a GPU (no CPU fallback).
Prints one JSON line and writes it to --out.

  python tools/bench_mesh_simplify.py [--sizes 128 256 512] [--noise-size 128] [--factor 2] [--rounds R] [--out FILE]
  python tools/bench_mesh_simplify.py --placement quadric     (writes profiles/mesh_simplify_quadric.json)
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

from bench_mesh import HBM_PRACTICAL_TBS, sphere_field, timed  # noqa: E402


def bench_one(name, field, iso, n, a, dev):
    import numpy as np
    from nerf_amd import Mesh
    from nerf_amd import kernels as K
    from nerf_amd._lib import check, lib, ptr, stream
    L = lib()
    mesh = Mesh(*K.mesh_extract(field, iso, [-1.0] * 3, [1.0] * 3, normals=True))
    del field
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    cell = np.float32(a.factor * 2.0 / (n - 1))
    out = mesh.simplify(cell)
    # the grid of Mesh.simplify, for the kernel-only calls
    box = np.asarray(torch.cat([mesh.vertices.min(0).values, mesh.vertices.max(0).values]).tolist(), np.float32)
    inv = np.float32(1.0) / cell
    dims = [int(c) + 1 for c in np.floor((box[3:] - box[:3]) * inv)]
    lo_c, dims_c = (ctypes.c_float * 3)(*box[:3].tolist()), (ctypes.c_int32 * 3)(*dims)
    kv, kf = K._table_log2(V, None), K._table_log2(F, None)
    ws_l = torch.empty(int(L.nerf_mesh_cluster_labels_workspace_bytes(V, kv)), dtype=torch.uint8, device=dev)
    ws_r = torch.empty(int(L.nerf_mesh_cluster_reduce_workspace_bytes(V, 1, 0)), dtype=torch.uint8, device=dev)
    ws_f = torch.empty(int(L.nerf_mesh_cluster_faces_workspace_bytes(F, kf)), dtype=torch.uint8, device=dev)
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    cv, cn = torch.empty_like(mesh.vertices), torch.empty_like(mesh.normals)
    faces2 = torch.empty_like(mesh.faces)
    keep = torch.empty(F, dtype=torch.uint8, device=dev)

    def labels_kernels():
        check(L.nerf_mesh_cluster_labels(ptr(mesh.vertices), V, lo_c, float(cell), float(inv), dims_c, kv, ptr(ws_l),
                                         ws_l.numel(), ptr(labels), ptr(status), stream()), "labels")

    def reduce_kernels():
        check(L.nerf_mesh_cluster_reduce(ptr(mesh.vertices), ptr(labels), ptr(mesh.normals), None, V, lo_c, float(cell),
                                         float(inv), dims_c, ptr(ws_r), ws_r.numel(), ptr(cv), ptr(cn), None, stream()),
              "reduce")

    def faces_kernels():
        check(L.nerf_mesh_cluster_faces(ptr(mesh.faces), ptr(labels), F, V, kf, ptr(ws_f), ws_f.numel(), ptr(faces2),
                                        ptr(keep), ptr(status), stream()), "faces")

    labels_kernels()
    probes_v = int(status[1])
    reduce_kernels()
    faces_kernels()
    probes_f = int(status[1])
    again = K.mesh_compact(cv, faces2, keep, [cn], ranges_checked=True)
    same = bool(torch.equal(again[0], out.vertices) and torch.equal(again[1], out.faces) and
                torch.equal(again[2][0], out.normals))
    quadric = {}
    if a.placement == "quadric":
        out_q = mesh.simplify(cell, placement="quadric")
        row_off, col = K.mesh_vertex_faces(faces2, V, ranges_checked=True)
        pos = torch.empty_like(mesh.vertices)
        placed = torch.empty(V, dtype=torch.uint8, device=dev)

        def quadric_kernel():
            check(L.nerf_mesh_cluster_quadric(ptr(mesh.vertices), ptr(mesh.faces), ptr(labels), ptr(row_off), ptr(col),
                                              ptr(cv), V, F, lo_c, float(cell), float(inv), dims_c, 1e-3, ptr(pos),
                                              ptr(placed), stream()), "quadric")

        quadric_kernel()
        again_q = K.mesh_compact(pos, faces2, keep, [cn], ranges_checked=True)
        same = same and bool(torch.equal(again_q[0], out_q.vertices) and torch.equal(again_q[1], out_q.faces))
        quadric = {"csr_build": lambda: K.mesh_vertex_faces(faces2, V, ranges_checked=True),
                   "quadric_kernel": quadric_kernel,
                   "simplify_quadric": lambda: mesh.simplify(cell, placement="quadric")}
    res = timed({"labels_kernels": labels_kernels, "reduce_kernels": reduce_kernels, "faces_kernels": faces_kernels,
                 "compact": lambda: K.mesh_compact(cv, faces2, keep, [cn], ranges_checked=True),
                 "simplify": lambda: mesh.simplify(cell),
                 "filter_components": lambda: mesh.filter_components(min_faces=a.min_faces), **quadric},
                a.rounds, a.inner, a.warmup)
    eff = {"labels_kernels": 48 * V + 4 * (1 << kv), "reduce_kernels": 172 * V,
           "faces_kernels": 69 * F + 4 * (1 << kf)}
    for k, b in eff.items():
        res[k]["effective_bytes"] = b
        res[k]["effective_tb_per_s"] = round(b / (res[k]["ms_median"] * 1e-3) / 1e12, 4)
        res[k]["of_practical_hbm"] = round(res[k]["effective_tb_per_s"] / HBM_PRACTICAL_TBS, 4)
    res.update({"mesh": name, "vertices": V, "faces": F, "cell": float(cell), "dims": dims,
                "vertices_out": int(out.vertices.shape[0]), "faces_out": int(out.faces.shape[0]),
                "table_log2_vertices": kv, "table_log2_faces": kf, "longest_probe_chain_vertices": probes_v,
                "longest_probe_chain_faces": probes_f, "clusters": int((labels == torch.arange(
                    V, dtype=torch.int32, device=dev)).sum()), "pieces_equal_simplify": same})
    if quadric:
        rows = (row_off[1:] - row_off[:-1])
        rep = labels == torch.arange(V, dtype=torch.int32, device=dev)
        res.update({"csr_entries": int(col.shape[0]), "longest_row": int(rows.max()),
                    "clusters_placed": int(placed.sum()), "clusters_kept_mean": int(rep.sum()) - int(placed.sum()),
                    "volume_in": mesh.volume(), "volume_mean": out.volume(), "volume_quadric": out_q.volume()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--noise-size", type=int, default=128)
    ap.add_argument("--noise-threshold", type=float, default=0.8)
    ap.add_argument("--factor", type=float, default=2.0, help="cell size in lattice spacings")
    ap.add_argument("--min-faces", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--placement", choices=["mean", "quadric"], default="mean",
                    help="quadric: also time the CSR build, the quadric kernel and Mesh.simplify(placement='quadric')")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "mesh_simplify_quadric.json" if a.placement == "quadric"
                             else "mesh_simplify.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_simplify: needs a GPU (timings on a CPU say nothing about the MI355X)")
    dev = torch.device("cuda:0")
    runs = [bench_one(f"sphere{n}", sphere_field(n, dev), 0.0, n, a, dev) for n in a.sizes]
    if a.noise_size:
        n = a.noise_size
        g = torch.Generator(device="cpu").manual_seed(18)
        noise = (torch.rand((n, n, n), generator=g) * 2.0 - 1.0).to(dev).contiguous()
        runs.append(bench_one(f"noise{n}", noise, a.noise_threshold, n, a, dev))
    res = {"bench": "mesh_simplify" if a.placement == "mean" else "mesh_simplify_quadric",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
           "factor": a.factor, "hbm_practical_tb_per_s": HBM_PRACTICAL_TBS, "meshes": runs}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
