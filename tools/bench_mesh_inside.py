#!/usr/bin/env python3
"""Timing of the crossing counts (csrc/mesh_inside.hip) next to the nearest-face search of §3.11.5 on
the same queries through the same face grid in the same run.  A record, not a gate: nothing before it counts
crossings.

  mesh      the sphere mesh of tools/bench_mesh.py (0.6 - |x| on [-1,1]^3 at --size^3; 320 gives about 1 M faces), its
            default face grid.
  queries   --queries kernels.box_points of the box of the vertices, and as many surface samples of the mesh's
            simplify(2 h): points within a few cells of the surface, which is what the nearest-face search is
            built for (a query r cells from the surface walks r shells of the grid, about 4/3 r^3 columns: the box
            points, up to 250 cells away, are no workload for it).
  phases    box_points           kernels.box_points alone
            crossings_sorted     kernels.mesh_point_crossings of the box points, queries in cell order
            crossings_unsorted   the same with sort_queries=False
            crossings_surface    the surface samples, sorted
            nearest_sorted       kernels.mesh_nearest_faces of the surface samples, sorted, for scale
            signed_distance      mesh_metrics.signed_distance_to_mesh of the surface samples end to end (the grid
                                 given)
            volume_iou           mesh_metrics.volume_iou of the sphere against its simplify(2 h) at --iou-samples,
                                 both face grids included
  counts    keys_per_query: the keys of the column from the query's cell upwards, for every box point, by two
            torch.searchsorted over the grid's keys.  faces_per_query and exact_path_share: the faces tested after
            the once-only rule and the share of orientation tests that fall through the floating filter, from the
            host restatement of the walk (tests/mesh_inside_reference.column_walk with orient_float) over --probe
            queries spread evenly over each set, not from the kernel; the same queries' counts are compared with the
            device's.
  at scale  inside share x box volume against Mesh.volume(), with its binomial standard error.

Each figure is the time between two events around back-to-back calls after `--warmup` untimed ones; the median over
`--rounds` rounds is reported with the fastest and slowest; the phases are alternated inside every round.  Needs a GPU
(no CPU fallback).  Prints one JSON line and writes it to --out.

  python tools/bench_mesh_inside.py [--size 320] [--queries 640000] [--rounds R] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-sys_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from bench_mesh import sphere_field, timed  # noqa: E402


def keys_per_query(q, grid):
    """(n,) int64: the keys from cell (cx, cy, cz) of every query to the end of its column, in torch on the device"""
    lo = torch.tensor(grid["lo"], dtype=torch.float32, device=q.device)
    dims = torch.tensor(grid["dims"], dtype=torch.float32, device=q.device)
    t = (q - lo) * torch.tensor(grid["inv"], dtype=torch.float32, device=q.device)
    c = torch.minimum(torch.clamp(torch.floor(t), min=0.0), dims - 1).to(torch.int64)
    base = (c[:, 0] * grid["dims"][1] + c[:, 1]) * grid["dims"][2]
    first = torch.searchsorted(grid["keys"], (base + c[:, 2]) << 32)
    return torch.searchsorted(grid["keys"], (base + grid["dims"][2]) << 32) - first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=320)
    ap.add_argument("--queries", type=int, default=640000)
    ap.add_argument("--iou-samples", type=int, default=2 ** 20)
    ap.add_argument("--probe", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_inside.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_inside: needs a GPU (timings on a CPU say nothing about the MI355X)")
    dev = torch.device("cuda:0")
    import numpy as np

    import mesh_inside_reference as R
    from nerf_amd import Mesh
    from nerf_amd import kernels as K
    from nerf_amd import mesh_metrics as MM
    mesh = Mesh(*K.mesh_extract(sphere_field(a.size, dev), 0.0, [-1.0] * 3, [1.0] * 3))
    v, f = mesh.vertices, mesh.faces
    F, n = int(f.shape[0]), a.queries
    h = 2.0 / (a.size - 1)
    simple = mesh.simplify(2 * h)
    grid = K.mesh_face_grid(v, f)
    lo, hi = v.amin(0).tolist(), v.amax(0).tolist()
    box = K.box_points(n, lo, hi, seed=0, device=dev)
    surface = simple.sample_surface(n)[0]
    ways = {"box_points": lambda: K.box_points(n, lo, hi, seed=0, device=dev),
            "crossings_sorted": lambda: K.mesh_point_crossings(box, v, f, grid, finite_checked=True),
            "crossings_unsorted": lambda: K.mesh_point_crossings(box, v, f, grid, sort_queries=False, finite_checked=True),
            "crossings_surface": lambda: K.mesh_point_crossings(surface, v, f, grid, finite_checked=True),
            "nearest_sorted": lambda: K.mesh_nearest_faces(surface, v, f, grid, finite_checked=True),
            "signed_distance": lambda: MM.signed_distance_to_mesh(surface, mesh, grid=grid),
            "volume_iou": lambda: MM.volume_iou(mesh, simple, n_samples=a.iou_samples)}
    res = timed(ways, a.rounds, a.inner, a.warmup)
    got = K.mesh_point_crossings(box, v, f, grid)
    again = K.mesh_point_crossings(box, v, f, grid, sort_queries=False)
    on = K.mesh_point_crossings(surface, v, f, grid)
    # the host restatement on a subsample: what one query tests, how often the filter decides, and the same counts
    pick = torch.linspace(0, n - 1, a.probe).round().to(torch.int64).to(dev)
    ref_grid = {"lo": np.asarray(grid["lo"], np.float32), "inv": np.float32(grid["inv"]), "cell": np.float32(grid["cell"]),
                "dims": grid["dims"]}
    vh, fh, kh = v.cpu().numpy(), f.cpu().numpy(), grid["keys"].cpu().numpy()
    probe = {}
    for name, q, dev_counts in (("box", box, got), ("surface", surface, on)):
        took = [0, 0]

        def orient(P, Q, R_):
            s, exact = R.orient_float(P, Q, R_)
            took[0] += 1
            took[1] += exact
            return s

        c, w, count = R.column_walk(vh, fh, q[pick].cpu().numpy(), ref_grid, counts=True, keys=kh, orient=orient)
        probe[name] = {"equals_device": bool(np.array_equal(dev_counts[0][pick].cpu().numpy(), c)
                                             and np.array_equal(dev_counts[1][pick].cpu().numpy(), w)),
                       "keys_per_query": float(count[:, 0].mean()), "faces_per_query": float(count[:, 1].mean()),
                       "orient_tests_per_query": took[0] / a.probe,
                       "exact_path_share": took[1] / took[0] if took[0] else None}
    inside = (got[0] & 1).to(torch.bool)
    p = float(inside.double().mean())
    vol_box = ((hi[0] - lo[0]) * (hi[1] - lo[1])) * (hi[2] - lo[2])
    iou = MM.volume_iou(mesh, simple, n_samples=a.iou_samples)
    kq = keys_per_query(box, grid)
    res.update({"bench": "mesh_inside", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
                "size": a.size, "vertices": int(v.shape[0]), "faces": F, "queries": n, "cell": grid["cell"],
                "dims": grid["dims"], "n_keys": grid["n_keys"], "keys_per_face": grid["n_keys"] / F,
                "inside_share": p, "inside_share_surface": float((on[0] & 1).double().mean()),
                "parity_equals_winding": bool(torch.equal(inside, got[1] != 0)),
                "unsorted_equals_sorted": all(bool(torch.equal(x, y)) for x, y in zip(got, again)),
                "keys_per_query": float(kq.double().mean()), "keys_per_query_max": int(kq.max()),
                "probe": a.probe, "probe_box": probe["box"], "probe_surface": probe["surface"],
                "volume_mesh": mesh.volume(), "volume_simplified": simple.volume(),
                "volume_monte_carlo": p * vol_box, "volume_standard_error": vol_box * math.sqrt(p * (1 - p) / n),
                "volume_sphere": 4.0 / 3.0 * math.pi * 0.6 ** 3, "iou_samples": a.iou_samples,
                "faces_simplified": int(simple.faces.shape[0]), "iou": iou,
                "ns_per_query_sorted": 1e6 * res["crossings_sorted"]["ms_median"] / n,
                "ns_per_query_unsorted": 1e6 * res["crossings_unsorted"]["ms_median"] / n,
                "ns_per_query_surface": 1e6 * res["crossings_surface"]["ms_median"] / n,
                "ns_per_query_nearest_sorted": 1e6 * res["nearest_sorted"]["ms_median"] / n,
                "unsorted_over_sorted": res["crossings_unsorted"]["ms_median"] / res["crossings_sorted"]["ms_median"],
                "crossings_over_nearest_surface": res["crossings_surface"]["ms_median"] / res["nearest_sorted"]["ms_median"]})
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh_out:
        fh_out.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
