#!/usr/bin/env python3
"""Timing of the mesh clean-up (csrc/mesh_clean.hip).  A record, not a gate: there is no earlier
implementation to compare with.

  meshes    the sphere meshes of tools/bench_mesh.py (0.6 - |x| on [-1,1]^3 at 128^3, 256^3 and 512^3: one component,
            the deepest trees) and a many-component mesh (a seeded uniform noise lattice at 128^3, threshold 0.8), each
            with V, F and the number of components.
  phases    components_kernels   nerf_mesh_components alone (init, unite, flatten, count: 4 launches, no host read)
            mesh_components      the wrapper: plus the index-range check and the status read (two host reads)
            selection            the torch ops that turn face counts into a keep flag per label (min_faces)
            compact              kernels.mesh_compact with that flag and the labels, vertices + normals carried
            filter_components    Mesh.filter_components(min_faces=...) as a whole
  bytes     for components_kernels the traffic the method implies at the least, 16 V + 40 F bytes: labels and counts
            initialised (8 V), the face list and one parent word per index in the unite pass (24 F), parent read and
            written in the flatten pass (8 V), the face list and one label per face in the count pass (16 F); over the
            time, next to the practical HBM rate DESIGN uses (about 5 TB/s).  The unite pass walks parent chains with
            dependent 4-byte loads, so this is a floor for the bytes, not a model of the time.
  scipy     for context only: scipy.sparse.csgraph.connected_components on the host for the 256^3 sphere mesh, the
            copy of the faces to the host included (one run, wall clock).

Each device figure is the time between two events around back-to-back calls after `--warmup` untimed ones: at least
`--inner` calls, and as many as fill a window of about 40 ms where a call is short.  The median over `--rounds` rounds
is reported with the fastest and slowest; the phases are alternated inside every round.  Needs a GPU (no CPU fallback).
Prints one JSON line and writes it to --out.

  python tools/bench_mesh_clean.py [--sizes 128 256 512] [--noise-size 128] [--rounds R] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-sys_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_mesh import HBM_PRACTICAL_TBS, sphere_field, timed  # noqa: E402


def bench_one(name, field, iso, min_faces, a, dev, with_scipy=False):
    from nerf_amd import Mesh
    from nerf_amd import kernels as K
    from nerf_amd._lib import check, lib, ptr, stream
    L = lib()
    mesh = Mesh(*K.mesh_extract(field, iso, [-1.0] * 3, [1.0] * 3, normals=True))
    del field
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    counts = torch.empty(V, dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)

    def kernels_only():
        check(L.nerf_mesh_components(ptr(mesh.faces), F, V, ptr(labels), ptr(counts), ptr(status), stream()),
              "nerf_mesh_components")

    kernels_only()
    ref_l, ref_c, steps = K.mesh_components(mesh.faces, V, return_steps=True)
    same = bool(torch.equal(ref_l, labels) and torch.equal(ref_c, counts))
    n_comp = int((ref_c > 0).sum())
    arange = torch.arange(V, dtype=torch.int32, device=dev)

    def selection():
        return (ref_l == arange) & (ref_c >= min_faces)

    keep = selection()
    out = mesh.filter_components(min_faces=min_faces)
    res = timed({"components_kernels": kernels_only,
                 "mesh_components": lambda: K.mesh_components(mesh.faces, V),
                 "selection": selection,
                 "compact": lambda: K.mesh_compact(mesh.vertices, mesh.faces, keep, [mesh.normals], labels=ref_l,
                                                   ranges_checked=True),
                 "filter_components": lambda: mesh.filter_components(min_faces=min_faces)},
                a.rounds, a.inner, a.warmup)
    b = 16 * V + 40 * F
    k = res["components_kernels"]
    k["effective_bytes"] = b
    k["effective_tb_per_s"] = round(b / (k["ms_median"] * 1e-3) / 1e12, 4)
    k["of_practical_hbm"] = round(k["effective_tb_per_s"] / HBM_PRACTICAL_TBS, 4)
    res.update({"mesh": name, "vertices": V, "faces": F, "components": n_comp, "most_find_steps_of_a_face": steps,
                "min_faces": min_faces, "faces_kept": int(out.faces.shape[0]), "vertices_kept": int(out.vertices.shape[0]),
                "kernels_equal_wrapper": same})
    if with_scipy:
        import numpy as np
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = mesh.faces.cpu().numpy().astype(np.int64)
        i = np.concatenate([f[:, 0], f[:, 1]])
        j = np.concatenate([f[:, 1], f[:, 2]])
        n, comp = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(V, V)), directed=False)
        res["scipy_host_ms_with_copy"] = round((time.perf_counter() - t0) * 1e3, 2)
        res["scipy_components"] = int(n)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--noise-size", type=int, default=128)
    ap.add_argument("--noise-threshold", type=float, default=0.8)
    ap.add_argument("--min-faces", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_clean: needs a GPU (timings on a CPU say nothing about the MI355X)")
    dev = torch.device("cuda:0")
    runs = [bench_one(f"sphere{n}", sphere_field(n, dev), 0.0, a.min_faces, a, dev, with_scipy=(n == 256))
            for n in a.sizes]
    if a.noise_size:
        n = a.noise_size
        g = torch.Generator(device="cpu").manual_seed(18)
        noise = (torch.rand((n, n, n), generator=g) * 2.0 - 1.0).to(dev).contiguous()
        runs.append(bench_one(f"noise{n}", noise, a.noise_threshold, a.min_faces, a, dev))
    res = {"bench": "mesh_clean", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
           "hbm_practical_tb_per_s": HBM_PRACTICAL_TBS, "meshes": runs}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
