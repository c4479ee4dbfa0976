#!/usr/bin/env python3
"""Timing of the mesh metrics (csrc/mesh_metrics.hip).  A record, not a gate: there is no earlier
implementation to compare with.

  meshes    the sphere meshes of tools/bench_mesh.py (0.6 - |x| on [-1,1]^3 at 128^3, 256^3 and 512^3) and the
            many-component noise mesh of tools/bench_mesh_clean.py (128^3, threshold 0.8).  The other surface of every
            query and distance is the mesh after simplify(2 lattice spacings).
  phases    areas_cdf          nerf_mesh_face_areas and the integer CDF in torch (with its two host reads)
            sample             nerf_mesh_sample_surface alone, --samples points with face normals
            keys               nerf_points_cell_keys of those points
            sort               torch.sort of those keys
            grid               kernels.points_grid as a whole (box read, keys, sort, gather)
            nearest_sorted     kernels.points_nearest of the other surface's samples, queries in cell order
            nearest_unsorted   the same with sort_queries=False
            distance_2^18, distance_2^20   mesh_metrics.mesh_distance end to end at that many samples per mesh
  brute     at n = m = 2^16 samples of the first mesh and its simplified form: a chunked torch.cdist + min next to
            nearest_points on the same points, as the yardstick; `index_agreement` is the share of equal indices
            (cdist takes another route to the distance, so its bits and, on near-ties, its choice differ).
  quality   chamfer / hausdorff of simplify(cell) and smooth(N) against the extracted surface on the first mesh, at
            2^--quality-log2 samples, next to the sampling floor: the surface against itself with two seeds.

Each figure is the time between two events around back-to-back calls after `--warmup` untimed ones; the median over
`--rounds` rounds is reported with the fastest and slowest; the phases are alternated inside every round.  Needs a GPU
(no CPU fallback).  Prints one JSON line and writes it to --out.

  python tools/bench_mesh_metrics.py [--sizes 128 256 512] [--noise-size 128] [--samples N] [--rounds R] [--out FILE]
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


def bench_one(name, field, iso, a, dev):
    from nerf_amd import Mesh, mesh_distance
    from nerf_amd import kernels as K
    from nerf_amd._lib import check, lib, ptr, stream
    L = lib()
    size = int(field.shape[0])
    mesh = Mesh(*K.mesh_extract(field, iso, [-1.0] * 3, [1.0] * 3))
    del field
    other = mesh.simplify(2 * 2.0 / (size - 1))
    v, f = mesh.vertices, mesh.faces
    F, n = int(f.shape[0]), a.samples
    cdf, total = K.mesh_area_cdf(K.mesh_face_areas(v, f))
    pts, face_idx, nrm = mesh.sample_surface(n, normals="face")
    query = other.sample_surface(n)[0]
    grid = K.points_grid(pts)
    lo_c, dims_c = (ctypes.c_float * 3)(*grid["lo"]), (ctypes.c_int32 * 3)(*grid["dims"])
    keys = torch.empty(n, dtype=torch.int64, device=dev)

    def sample():
        check(L.nerf_mesh_sample_surface(ptr(v), ptr(f), F, ptr(cdf), total, None, n, 0, ptr(pts), ptr(face_idx),
                                         ptr(nrm), stream()), "sample")

    def keys_kernel():
        check(L.nerf_points_cell_keys(ptr(pts), n, lo_c, grid["inv"], dims_c, ptr(keys), stream()), "keys")

    keys_kernel()
    ways = {"areas_cdf": lambda: K.mesh_area_cdf(K.mesh_face_areas(v, f, ranges_checked=True)), "sample": sample,
            "keys": keys_kernel, "sort": lambda: torch.sort(keys), "grid": lambda: K.points_grid(pts),
            "nearest_sorted": lambda: K.points_nearest(query, grid, finite_checked=True),
            "nearest_unsorted": lambda: K.points_nearest(query, grid, sort_queries=False, finite_checked=True)}
    for k in a.distance_log2:
        ways[f"distance_2^{k}"] = (lambda k=k: mesh_distance(mesh, other, 2 ** k))
    res = timed(ways, a.rounds, a.inner, a.warmup)
    s, u = K.points_nearest(query, grid), K.points_nearest(query, grid, sort_queries=False)
    d = mesh_distance(mesh, other, n)
    res.update({"mesh": name, "vertices": int(v.shape[0]), "faces": F, "other_vertices": int(other.vertices.shape[0]),
                "other_faces": int(other.faces.shape[0]), "samples": n, "cell": grid["cell"], "dims": grid["dims"],
                "sorted_equals_unsorted": bool(torch.equal(s[0], u[0]) and torch.equal(s[1], u[1])),
                "chamfer": d["chamfer"], "hausdorff": d["hausdorff"]})
    return res, mesh


def brute(mesh, a, dev, chunk=2048):
    from nerf_amd import nearest_points
    n = 2 ** a.brute_log2
    q = mesh.simplify(2 * 2.0 / (a.sizes[0] - 1)).sample_surface(n)[0]
    p = mesh.sample_surface(n)[0]

    def cdist_min():
        d, i = [], []
        for s in range(0, n, chunk):
            m = torch.cdist(q[s:s + chunk], p).min(1)
            d.append(m.values)
            i.append(m.indices)
        return torch.cat(d), torch.cat(i)

    res = timed({"cdist_min": cdist_min, "nearest_points": lambda: nearest_points(q, p)}, a.rounds, 1, a.warmup)
    (d2, idx), (bd, bi) = nearest_points(q, p), cdist_min()
    err = (torch.sqrt(d2.double()) - bd.double()).abs().max()
    res.update({"n": n, "m": n, "chunk": chunk, "index_agreement": float((idx.long() == bi).double().mean()),
                "max_abs_distance_difference": float(err)})
    return res


def quality(mesh, a):
    h = 2.0 / (a.sizes[0] - 1)
    n = 2 ** a.quality_log2
    rows = []
    for cells in (1, 2, 4, 8):
        m = mesh.simplify(cells * h)
        d = m.distance_to(mesh, n_samples=n)
        rows.append({"op": f"simplify({cells} h)", "cell": cells * h, "vertices": int(m.vertices.shape[0]),
                     "faces": int(m.faces.shape[0]), "chamfer": d["chamfer"], "hausdorff": d["hausdorff"],
                     "a_to_b_rms": d["a_to_b_rms"]})
    for it in (1, 10, 50):
        m = mesh.smooth(it)
        d = m.distance_to(mesh, n_samples=n)
        rows.append({"op": f"smooth({it})", "vertices": int(m.vertices.shape[0]), "faces": int(m.faces.shape[0]),
                     "chamfer": d["chamfer"], "hausdorff": d["hausdorff"], "a_to_b_rms": d["a_to_b_rms"]})
    floor = mesh.distance_to(mesh, n_samples=n, seed=1)  # same surface: exactly 0 with one seed on both sides
    other = mesh_other_seed(mesh, n)
    return {"lattice_spacing": h, "samples": n, "spacing": (mesh.area() / n) ** 0.5, "same_seed_chamfer": floor["chamfer"],
            "other_seed_chamfer": other["chamfer"], "other_seed_hausdorff": other["hausdorff"], "rows": rows}


def mesh_other_seed(mesh, n):
    """the sampling floor: the surface against itself with two different seeds"""
    from nerf_amd import point_set_metrics
    return point_set_metrics(mesh.sample_surface(n, seed=0)[0], mesh.sample_surface(n, seed=1)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--noise-size", type=int, default=128)
    ap.add_argument("--noise-threshold", type=float, default=0.8)
    ap.add_argument("--samples", type=int, default=2 ** 18)
    ap.add_argument("--distance-log2", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--brute-log2", type=int, default=16)
    ap.add_argument("--quality-log2", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_metrics.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_metrics: needs a GPU (timings on a CPU say nothing about the MI355X)")
    dev = torch.device("cuda:0")
    runs, first = [], None
    for n in a.sizes:
        r, mesh = bench_one(f"sphere{n}", sphere_field(n, dev), 0.0, a, dev)
        runs.append(r)
        first = mesh if first is None else first
    if a.noise_size:
        n = a.noise_size
        g = torch.Generator(device="cpu").manual_seed(18)
        noise = (torch.rand((n, n, n), generator=g) * 2.0 - 1.0).to(dev).contiguous()
        runs.append(bench_one(f"noise{n}", noise, a.noise_threshold, a, dev)[0])
    res = {"bench": "mesh_metrics", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
           "meshes": runs, "brute_force": brute(first, a, dev), "quality": quality(first, a)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
