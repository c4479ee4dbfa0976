#!/usr/bin/env python3
"""Timing of the generalised winding number (csrc/mesh_winding.hip): the far-field form against the
exact form on the same box in the same process, and against the crossing counts of §3.11.7 for scale.  A record, not a
gate: nothing before it computes a winding number.

  meshes    the sphere level set of tools/bench_mesh.py (0.6 - |x| on [-1,1]^3) at every --sizes^3 (64, 128, 256 give
            about 41 k, 165 k and 660 k faces): closed, so the answer is known (1 inside, 0 outside).
  queries   kernels.box_points of the box of the vertices, --queries of them (2^16 and 2^20).
  phases    bricks               kernels.mesh_winding_bricks alone (keys, sort, soup, the host read of B, moments)
            crossings            kernels.mesh_point_crossings through the default face grid, for scale
            exact                kernels.mesh_winding_number(exact=True): n x F solid angles; skipped, and named as
                                 skipped, where n x F exceeds --exact-pairs
            beta2, beta3, beta4  the far-field form on the default bricks
            sweep                beta = 3 on 2^16 queries with k = ceil(c F^(1/4)) bricks along the longest axis for
                                 every c of --sweep; the default is c = 1.25
  errors    max and mean |w_beta - w_exact| and the number of queries whose side of 0.5 differs from the parity of
            the crossing counts, wherever the exact form ran.
  work      far bricks and exactly summed faces per query, counted in torch on a subsample of --probe queries from
            the bricks' records (the kernel's own near / far rule restated), not from the kernel.

Each figure is the time between two events around back-to-back calls after `--warmup` untimed ones; the median over
`--rounds` rounds (3 for the exact form) is reported with the fastest and slowest; the phases are alternated inside
every round.  Needs a GPU (no CPU fallback).  Prints one JSON line and writes it to --out.

  python tools/bench_mesh_winding.py [--sizes 64 128 256] [--queries 65536 1048576] [--rounds R] [--out FILE]
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

import torch  # noqa: E402

from bench_mesh import sphere_field, timed  # noqa: E402


def work_per_query(q, bricks, beta):
    """(far bricks, exactly summed faces) per query, means over q (m,3): the near / far rule in float64 torch ops"""
    p, r2 = bricks["moments"][:, :3], bricks["moments"][:, 6]
    size = (bricks["runs"][:, 1] - bricks["runs"][:, 0]).to(torch.float64)
    d = p[None] - q.to(torch.float64)[:, None]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    far = d2 > (beta * beta) * r2[None]
    return float(far.sum(1).double().mean()), float(((~far) * size[None]).sum(1).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--queries", type=int, nargs="+", default=[2 ** 16, 2 ** 20])
    ap.add_argument("--sweep", type=float, nargs="+", default=[0.625, 0.9, 1.25, 1.8, 2.5, 3.5, 5.0])
    ap.add_argument("--exact-pairs", type=float, default=1e11, help="skip the exact form above this many n x F")
    ap.add_argument("--probe", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_winding.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_winding: needs a GPU (timings on a CPU say nothing about the MI355X)")
    dev = torch.device("cuda:0")
    from nerf_amd import Mesh
    from nerf_amd import kernels as K
    out = {"bench": "mesh_winding", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "meshes": []}
    for size in a.sizes:
        mesh = Mesh(*K.mesh_extract(sphere_field(size, dev), 0.0, [-1.0] * 3, [1.0] * 3))
        v, f = mesh.vertices, mesh.faces
        F = int(f.shape[0])
        lo, hi = v.amin(0).tolist(), v.amax(0).tolist()
        bricks = K.mesh_winding_bricks(v, f)
        grid = K.mesh_face_grid(v, f)
        rec = {"size": size, "faces": F, "vertices": int(v.shape[0]), "bricks_per_axis": max(bricks["dims"]),
               "dims": bricks["dims"], "B": bricks["B"], "faces_per_brick": F / bricks["B"],
               "bytes_per_face": (bricks["keys"].element_size() * bricks["keys"].numel()
                                  + bricks["soup"].element_size() * bricks["soup"].numel()) / F,
               "bytes_per_brick": 8 + 56, "runs": []}
        rec.update(timed({"bricks": lambda: K.mesh_winding_bricks(v, f), "face_grid": lambda: K.mesh_face_grid(v, f)},
                         a.rounds, 1, a.warmup))
        for n in a.queries:
            q = K.box_points(n, lo, hi, seed=0, device=dev)

            def far(beta, br=bricks, qq=q):
                return lambda: K.mesh_winding_number(qq, v, f, br, beta=beta, finite_checked=True)

            ways = {"crossings": lambda: K.mesh_point_crossings(q, v, f, grid, finite_checked=True),
                    "beta2": far(2.0), "beta3": far(3.0), "beta4": far(4.0),
                    "beta3_unsorted": lambda: K.mesh_winding_number(q, v, f, bricks, sort_queries=False,
                                                                    finite_checked=True)}
            run = {"queries": n, "pairs": n * F}
            run.update(timed(ways, a.rounds, 1, a.warmup))
            pick = q[torch.linspace(0, n - 1, a.probe).round().to(torch.int64).to(dev)]
            run["work"] = {f"beta{b}": dict(zip(("far_bricks", "exact_faces"), work_per_query(pick, bricks, float(b))))
                           for b in (2, 3, 4)}
            parity = (K.mesh_point_crossings(q, v, f, grid)[0] & 1).to(torch.bool)
            run["inside_share"] = float(parity.double().mean())
            ws = {b: K.mesh_winding_number(q, v, f, bricks, beta=float(b)) for b in (2, 3, 4)}
            run["side_differs_from_parity"] = {f"beta{b}": int(((w > 0.5) != parity).sum()) for b, w in ws.items()}
            if n * F <= a.exact_pairs:
                run.update(timed({"exact": lambda: K.mesh_winding_number(q, v, f, bricks, exact=True,
                                                                         finite_checked=True)}, 3, 1, a.warmup))
                exact = K.mesh_winding_number(q, v, f, bricks, exact=True)
                run["side_differs_from_parity"]["exact"] = int(((exact > 0.5) != parity).sum())
                run["exact_from_integer_max"] = float((exact - exact.round()).abs().max())
                run["errors"] = {f"beta{b}": {"max": float((w - exact).abs().max()), "mean": float((w - exact).abs().mean())}
                                 for b, w in ws.items()}
                run["ns_per_pair_exact"] = 1e6 * run["exact"]["ms_median"] / (n * F)
                run["exact_over_beta3"] = run["exact"]["ms_median"] / run["beta3"]["ms_median"]
            else:
                run["exact"] = None
                run["exact_skipped"] = f"n x F = {n * F:.3g} exceeds --exact-pairs {a.exact_pairs:.3g}: not measured"
            run["beta3_over_crossings"] = run["beta3"]["ms_median"] / run["crossings"]["ms_median"]
            run["ns_per_query_beta3"] = 1e6 * run["beta3"]["ms_median"] / n
            rec["runs"].append(run)
        # the bricks-per-axis sweep: beta = 3, every query count
        rec["sweeps"] = []
        for n in a.queries:
            q = K.box_points(n, lo, hi, seed=0, device=dev)
            pick = q[torch.linspace(0, n - 1, a.probe).round().to(torch.int64).to(dev)]
            exact = K.mesh_winding_number(q, v, f, bricks, exact=True) if n * F <= a.exact_pairs else None
            sweep, ways = [], {}
            for c in a.sweep:
                k = min(max(math.ceil(c * F ** 0.25), 1), 1024)
                br = K.mesh_winding_bricks(v, f, k)
                far_bricks, exact_faces = work_per_query(pick, br, 3.0)
                sweep.append({"c": c, "bricks_per_axis": k, "B": br["B"], "far_bricks": far_bricks,
                              "exact_faces": exact_faces})
                if exact is not None:
                    sweep[-1]["max_error"] = float((K.mesh_winding_number(q, v, f, br) - exact).abs().max())
                ways[f"c{c}"] = (lambda b=br, qq=q: K.mesh_winding_number(qq, v, f, b, finite_checked=True))
            times = timed(ways, a.rounds, 1, a.warmup)
            for row in sweep:
                row.update(times[f"c{row['c']}"])
            rec["sweeps"].append({"queries": n, "beta": 3.0, "rows": sweep})
        out["meshes"].append(rec)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
