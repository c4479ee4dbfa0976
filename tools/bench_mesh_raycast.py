#!/usr/bin/env python3
"""Timing of nearest-hit ray casting against a mesh (csrc/mesh_raycast.hip) next to the nearest-face
search of §3.11.5 on as many queries through the same face grid in the same run.  A record, not a gate: nothing before
it casts rays.

  mesh      the sphere mesh of tools/bench_mesh.py (0.6 - |x| on [-1,1]^3 at --size^3; 320 gives about 1 M faces).
  rays      a --image x --image pinhole camera outside the sphere, looking at its centre; the sphere covers about
            half of the picture.
  phases    cast_pixel_order   kernels.mesh_ray_cast of the camera's rays as rays_for_camera orders them (row by row)
            cast_permuted      the same rays in a random permutation: the price of incoherent lanes
            cast_culled        pixel order, cull_backfaces=True
            render             Mesh.render of the view end to end (rays, the cast, normals; the grid given)
            nearest_sorted     kernels.mesh_nearest_faces of as many surface samples of the simplified mesh, queries
                               in cell order; nearest_unsorted the same with sort_queries=False
            face_grid          kernels.mesh_face_grid as a whole, which both queries share
  counts    layers_per_ray and faces_per_ray: the layers walked and the faces tested by one ray, from the numpy
            restatement of the walk (tests/mesh_raycast_reference.grid_ray_cast) over --probe rays spread evenly over
            the picture, not from the kernel; the same rays' results are compared with the device's, bit for bit.

Each figure is the time between two events around back-to-back calls after `--warmup` untimed ones; the median over
`--rounds` rounds is reported with the fastest and slowest; the phases are alternated inside every round.  Needs a GPU
(no CPU fallback).  Prints one JSON line and writes it to --out.

  python tools/bench_mesh_raycast.py [--size 320] [--image 800] [--rounds R] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-sys_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from bench_mesh import sphere_field, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=320)
    ap.add_argument("--image", type=int, default=800)
    ap.add_argument("--focal", type=float, default=None, help="default: 1.375 x --image (the sphere fills half the view)")
    ap.add_argument("--probe", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_raycast.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_raycast: needs a GPU (timings on a CPU say nothing about the MI355X)")
    dev = torch.device("cuda:0")
    import numpy as np

    import mesh_raycast_reference as R
    from nerf_amd import Mesh
    from nerf_amd import kernels as K
    from nerf_amd.ray_sampling import rays_for_camera
    from nerf_amd.scene import look_at
    mesh = Mesh(*K.mesh_extract(sphere_field(a.size, dev), 0.0, [-1.0] * 3, [1.0] * 3))
    v, f = mesh.vertices, mesh.faces
    F = int(f.shape[0])
    H = W = a.image
    focal = a.focal or 1.375 * a.image
    c2w = look_at(torch.tensor([1.5, -1.2, 1.0], dtype=torch.float64))[:3, :4].to(torch.float32).to(dev)
    cam = (H, W, focal, focal, W / 2.0, H / 2.0)
    rays = rays_for_camera(*cam, c2w, near=0.0, far=float("inf"))
    n = int(rays.shape[0])
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(dev)
    shuffled = rays[perm].contiguous()
    grid = K.mesh_face_grid(v, f)
    query = mesh.simplify(2 * 2.0 / (a.size - 1)).sample_surface(n)[0]
    ways = {"cast_pixel_order": lambda: K.mesh_ray_cast(rays, v, f, grid, finite_checked=True),
            "cast_permuted": lambda: K.mesh_ray_cast(shuffled, v, f, grid, finite_checked=True),
            "cast_culled": lambda: K.mesh_ray_cast(rays, v, f, grid, cull_backfaces=True, finite_checked=True),
            "render": lambda: mesh.render(*cam, c2w, grid=grid),
            "nearest_sorted": lambda: K.mesh_nearest_faces(query, v, f, grid, finite_checked=True),
            "nearest_unsorted": lambda: K.mesh_nearest_faces(query, v, f, grid, sort_queries=False, finite_checked=True),
            "face_grid": lambda: K.mesh_face_grid(v, f)}
    res = timed(ways, a.rounds, a.inner, a.warmup)
    got = K.mesh_ray_cast(rays, v, f, grid)
    again = K.mesh_ray_cast(shuffled, v, f, grid)
    culled = K.mesh_ray_cast(rays, v, f, grid, cull_backfaces=True)
    # the host restatement on a subsample: what one ray walks and tests, and the same bits
    pick = torch.linspace(0, n - 1, a.probe).round().to(torch.int64).to(dev)
    ref_grid = {"lo": np.asarray(grid["lo"], np.float32), "cell": np.float32(grid["cell"]), "dims": grid["dims"]}
    ref = R.grid_ray_cast(v.cpu().numpy(), f.cpu().numpy(), rays[pick].cpu().numpy(), ref_grid, counts=True,
                          keys=grid["keys"].cpu().numpy())
    same = all(g[pick].cpu().numpy().tobytes() == r.tobytes() for g, r in zip(got, ref[:3]))
    hit = ref[1] >= 0
    res.update({"bench": "mesh_raycast", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
                "size": a.size, "vertices": int(v.shape[0]), "faces": F, "image": a.image, "focal": focal, "rays": n,
                "cell": grid["cell"], "dims": grid["dims"], "n_keys": grid["n_keys"], "keys_per_face": grid["n_keys"] / F,
                "hit_share": float((got[1] >= 0).float().mean()),
                "culled_equals_plain": all(bool(torch.equal(x, y)) for x, y in zip(got, culled)),
                "permuted_equals_pixel_order": all(bool(torch.equal(x[perm], y)) for x, y in zip(got, again)),
                "probe": a.probe, "probe_equals_device": same,
                "layers_per_ray": float(ref[3][:, 0].mean()), "faces_per_ray": float(ref[3][:, 1].mean()),
                "layers_per_hit_ray": float(ref[3][hit, 0].mean()) if hit.any() else None,
                "faces_per_hit_ray": float(ref[3][hit, 1].mean()) if hit.any() else None,
                "layers_per_miss_ray": float(ref[3][~hit, 0].mean()) if (~hit).any() else None,
                "ns_per_ray_pixel_order": 1e6 * res["cast_pixel_order"]["ms_median"] / n,
                "ns_per_ray_permuted": 1e6 * res["cast_permuted"]["ms_median"] / n,
                "ns_per_query_nearest_sorted": 1e6 * res["nearest_sorted"]["ms_median"] / n,
                "permuted_over_pixel_order": res["cast_permuted"]["ms_median"] / res["cast_pixel_order"]["ms_median"],
                "cast_over_nearest_sorted": res["cast_pixel_order"]["ms_median"] / res["nearest_sorted"]["ms_median"]})
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
