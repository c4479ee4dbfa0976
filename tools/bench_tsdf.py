#!/usr/bin/env python3
"""Timing of the TSDF fusion kernel (csrc/tsdf.hip).  A record, not a gate: there is no earlier
implementation to compare with.

  volume    [-1,1]^3 at 128^3, 256^3 and 512^3; views: scene.hemisphere_poses(64) at 800x800 with the Blender focal,
            depth the analytic range to a sphere of radius 0.6 (+inf on a miss).
  ways      nerf_tsdf_integrate with 1, 8 and 64 views in one call (the entry point runs one launch per 8 views, so 64
            views are 8 launches); the same 64 views as 64 calls of one view (the A/B for the in-kernel view loop); and
            the same rule for one view written with torch ops on the device (the lattice positions precomputed outside
            the timed region, which favours the torch form).
  figures   per way the time, voxel-views per second, and effective bytes over time next to the practical HBM rate
            DESIGN uses (about 5 TB/s).  Effective bytes are 8 B read + 8 B written per voxel per launch (tsdf and
            weight); the depth gathers are not counted.  Ratios per size: 64 calls of one view over one call of
            64, and the torch form over one call, per voxel-view.
  profiles/tsdf_integrate_one_launch.json is this tool's record of the entry point before it capped the views per
  launch: there kernel_64_views is a single launch.

--color (off by default; the ways and every JSON key above are unchanged without it) adds the fusion with colour
(nerf_tsdf_integrate_color) to the same rounds, on a volume with a colour lattice and the views'
analytic colours 0.5 + 0.4 p / R (0 on a miss):
  color_1_views, color_8_views, color_64_views   one call, as the kernel_* ways (the entry point splits 64 views by its
            own views-per-launch cap);
  color_64_views_by_K for K = 1, 2, 4, 8   the same 64 views as 64 / K calls of K views: the candidates for that cap.
            A call of K views is one launch as long as K does not exceed the compiled cap.
  Effective bytes of the colour path are 24 B read + 24 B written per voxel per launch (tsdf, weight and the 16-byte
  colour slot).  Per size the line gains color_views_per_launch_fastest and ratio_color_over_plain_64_views (the colour
  call of 64 views over the plain one).  The default --out is then profiles/tsdf_color.json; the committed record is
  such a line with two keys added by hand: a second process's color_64_views_by_K medians, and plain_parent_vs_this,
  the plain ways of four alternated processes on one box (the parent commit's library through NERF_AMD_LIB, and this
  one's).

The method is tools/bench_mesh.py's: device events around back-to-back calls after `--warmup` untimed ones, at least
`--inner` calls and as many as fill a window of about 40 ms, the median over `--rounds` rounds with the fastest and
slowest, the ways alternated inside every round.  Needs a GPU (no CPU fallback).  Prints one JSON line and writes it
to --out.

  python tools/bench_tsdf.py [--sizes 128 256 512] [--rounds R] [--inner I] [--warmup W] [--color] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-sys_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_mesh import HBM_PRACTICAL_TBS, timed  # noqa: E402

LO, HI = [-1.0] * 3, [1.0] * 3
RADIUS = 0.6
VIEWS = (1, 8, 64)
COLOR_SPLITS = (1, 2, 4, 8)  # views per call of the color_64_views_by_K ways


def sphere_depth(c2w, size, focal, dev):
    """(size,size) fp32: the range along unit pixel-centre rays to the sphere at the origin, +inf on a miss"""
    M = c2w.to(dev, torch.float64)
    j, i = torch.meshgrid(torch.arange(size, device=dev, dtype=torch.float64) + 0.5,
                          torch.arange(size, device=dev, dtype=torch.float64) + 0.5, indexing="ij")
    d = torch.stack([(i - size / 2.0) / focal, -(j - size / 2.0) / focal, -torch.ones_like(i)], -1)
    d = (d / d.norm(dim=-1, keepdim=True)) @ M[:, :3].T
    o = M[:, 3]
    b = d @ o
    disc = b * b - (o @ o - RADIUS * RADIUS)
    t = -b - disc.clamp_min(0).sqrt()
    return torch.where((disc > 0) & (t > 0), t, torch.full_like(t, float("inf"))).float()


def sphere_rgb(c2w, depth, focal):
    """(size,size,3) fp32: 0.5 + 0.4 p / RADIUS at the hit point p of every pixel of sphere_depth's image, 0 on a
    miss"""
    size, dev = depth.shape[0], depth.device
    M = c2w.to(dev, torch.float64)
    j, i = torch.meshgrid(torch.arange(size, device=dev, dtype=torch.float64) + 0.5,
                          torch.arange(size, device=dev, dtype=torch.float64) + 0.5, indexing="ij")
    d = torch.stack([(i - size / 2.0) / focal, -(j - size / 2.0) / focal, -torch.ones_like(i)], -1)
    d = (d / d.norm(dim=-1, keepdim=True)) @ M[:, :3].T
    hit = torch.isfinite(depth)
    p = M[:, 3] + d * torch.where(hit, depth, torch.zeros_like(depth)).double()[..., None]
    return torch.where(hit[..., None], 0.5 + 0.4 * p / RADIUS, torch.zeros_like(p)).float()


def torch_view(tsdf, weight, x, M, depth, fx, fy, cx, cy, trunc):
    """the rule of nerf_tsdf_integrate for one view with torch ops, in place; x (P,3) the lattice positions"""
    H, W = depth.shape
    q0, q1, q2 = x[:, 0] - M[0, 3], x[:, 1] - M[1, 3], x[:, 2] - M[2, 3]
    c0 = q0 * M[0, 0] + q1 * M[1, 0] + q2 * M[2, 0]
    c1 = q0 * M[0, 1] + q1 * M[1, 1] + q2 * M[2, 1]
    zc = -(q0 * M[0, 2] + q1 * M[1, 2] + q2 * M[2, 2])
    u = fx * (c0 / zc) + cx
    v = fy * ((-c1) / zc) + cy
    ok = (zc > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    col = torch.where(ok, u.floor(), torch.zeros_like(u)).long()
    row = torch.where(ok, v.floor(), torch.zeros_like(v)).long()
    d = depth.reshape(-1)[row * W + col]
    s = d - torch.sqrt(q0 * q0 + q1 * q1 + q2 * q2)
    ok &= torch.isfinite(d) & (d > 0) & ~(s < -trunc)
    t = (s / trunc).clamp_max(1.0)
    T, Wt = tsdf.view(-1), weight.view(-1)
    T.copy_(torch.where(ok, (T * Wt + t) / (Wt + 1.0), T))
    Wt.copy_(torch.where(ok, Wt + 1.0, Wt))


def bench_volume(n, a, depth, poses, cam, dev, rgb=None):
    from nerf_amd import TSDFVolume
    from nerf_amd import kernels as K
    from nerf_amd._lib import check, lib, ptr, stream
    L = lib()
    vol = TSDFVolume(LO, HI, n, device=dev)
    P = n ** 3
    fx, fy, cx, cy = cam
    trunc = vol.trunc
    ax = [torch.tensor(LO[k], device=dev) + torch.arange(n, device=dev, dtype=torch.float32) * vol.spacing[k]
          for k in range(3)]
    x = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).contiguous()

    # the entry point itself: kernels.tsdf_integrate adds a host read (the finiteness of c2w) to every call
    lo_c, hi_c = (ctypes.c_float * 3)(*LO), (ctypes.c_float * 3)(*HI)
    size = depth.shape[1]

    def launch(first, k):
        check(L.nerf_tsdf_integrate(ptr(vol.tsdf), ptr(vol.weight), n, n, n, lo_c, hi_c, ptr(depth[first:]),
                                    ptr(poses[first:]), k, size, size, fx, fy, cx, cy, trunc, stream()), "integrate")

    def kernel(k):
        return lambda: launch(0, k)

    def per_view():
        for v in range(64):
            launch(v, 1)

    def torch_form():
        torch_view(vol.tsdf, vol.weight, x, poses[0], depth[0], fx, fy, cx, cy, trunc)

    # one view by the kernel and by the torch form on fresh volumes: reported, not required
    K.tsdf_integrate(vol.tsdf, vol.weight, LO, HI, depth[:1], poses[:1], fx, fy, cx, cy, trunc)
    got = (vol.tsdf.clone(), vol.weight.clone())
    vol.reset()
    torch_form()
    same = bool(torch.equal(got[0], vol.tsdf) and torch.equal(got[1], vol.weight))
    diff = float((got[0] - vol.tsdf).abs().max())
    touched = float((got[1] > 0).float().mean())
    vol.reset()
    ways = {f"kernel_{k}_views": kernel(k) for k in VIEWS}
    ways["kernel_64_launches_of_1"] = per_view
    ways["torch_1_view"] = torch_form
    if rgb is not None:
        cvol = TSDFVolume(LO, HI, n, device=dev, color=True)

        def color_launch(first, k):
            check(L.nerf_tsdf_integrate_color(ptr(cvol.tsdf), ptr(cvol.weight), ptr(cvol.color), n, n, n, lo_c, hi_c,
                                              ptr(depth[first:]), ptr(rgb[first:]), ptr(poses[first:]), k, size, size,
                                              fx, fy, cx, cy, trunc, stream()), "integrate_color")

        def color_by(k):
            def run():
                for first in range(0, 64, k):
                    color_launch(first, k)
            return run

        for k in VIEWS:
            ways[f"color_{k}_views"] = (lambda k: lambda: color_launch(0, k))(k)
        for k in COLOR_SPLITS:
            ways[f"color_64_views_by_{k}"] = color_by(k)
    res = timed(ways, a.rounds, a.inner, a.warmup)
    views = {"kernel_1_views": (1, 1), "kernel_8_views": (8, 1), "kernel_64_views": (64, 1),
             "kernel_64_launches_of_1": (64, 64), "torch_1_view": (1, 1)}
    for k, (nv, launches) in views.items():
        sec = res[k]["ms_median"] * 1e-3
        res[k]["voxel_views_per_s"] = round(P * nv / sec)
        res[k]["effective_bytes"] = 16 * P * launches
        res[k]["effective_tb_per_s"] = round(16 * P * launches / sec / 1e12, 3)
        res[k]["of_practical_hbm"] = round(res[k]["effective_tb_per_s"] / HBM_PRACTICAL_TBS, 3)
    res["ratio_64_launches_over_one_launch"] = round(
        res["kernel_64_launches_of_1"]["ms_median"] / res["kernel_64_views"]["ms_median"], 3)
    res["ratio_torch_over_kernel_1_view"] = round(res["torch_1_view"]["ms_median"] / res["kernel_1_views"]["ms_median"], 3)
    res["ratio_torch_per_view_over_kernel_64_per_view"] = round(
        res["torch_1_view"]["ms_median"] / (res["kernel_64_views"]["ms_median"] / 64.0), 3)
    if rgb is not None:
        cviews = {f"color_{k}_views": (k, 1) for k in VIEWS}
        cviews.update({f"color_64_views_by_{k}": (64, 64 // k) for k in COLOR_SPLITS})
        for k, (nv, launches) in cviews.items():
            sec = res[k]["ms_median"] * 1e-3
            res[k]["voxel_views_per_s"] = round(P * nv / sec)
            res[k]["effective_bytes"] = 48 * P * launches
            res[k]["effective_tb_per_s"] = round(48 * P * launches / sec / 1e12, 3)
            res[k]["of_practical_hbm"] = round(res[k]["effective_tb_per_s"] / HBM_PRACTICAL_TBS, 3)
        res["color_views_per_launch_fastest"] = min(COLOR_SPLITS,
                                                    key=lambda k: res[f"color_64_views_by_{k}"]["ms_median"])
        res["ratio_color_over_plain_64_views"] = round(
            res["color_64_views"]["ms_median"] / res["kernel_64_views"]["ms_median"], 3)
        res["color_share_after_64_views"] = round(float((cvol.color[..., 3] > 0).float().mean()), 4)
    res.update({"n": n, "voxels": P, "trunc": trunc, "touched_share_one_view": round(touched, 4),
                "torch_form_bitwise_equal_one_view": same, "torch_form_max_abs_diff_one_view": diff})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--image-size", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--color", action="store_true", help="add the ways of the fusion with colour")
    ap.add_argument("--out", default=None,
                    help="default: profiles/tsdf_integrate.json, with --color profiles/tsdf_color.json")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "tsdf_color.json" if a.color else "tsdf_integrate.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf: needs a GPU (timings on a CPU say nothing about the MI355X)")
    import math

    from nerf_amd.scene import hemisphere_poses
    dev = torch.device("cuda:0")
    size = a.image_size
    focal = 0.5 * size / math.tan(0.5 * 0.6911112)
    poses = hemisphere_poses(64, seed=0).to(dev).contiguous()
    depth = torch.stack([sphere_depth(M, size, focal, dev) for M in poses]).contiguous()
    cam = (focal, focal, size / 2.0, size / 2.0)
    rgb = torch.stack([sphere_rgb(M, d, focal) for M, d in zip(poses, depth)]).contiguous() if a.color else None
    res = {"bench": "tsdf_integrate", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
           "image_size": size, "views": 64, "hit_share": round(float(torch.isfinite(depth).float().mean()), 4),
           "hbm_practical_tb_per_s": HBM_PRACTICAL_TBS,
           "volumes": [bench_volume(n, a, depth, poses, cam, dev, rgb) for n in a.sizes]}
    if a.color:
        res["color"] = True
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
