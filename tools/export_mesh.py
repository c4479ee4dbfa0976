#!/usr/bin/env python3
"""Export the surface of an Instant-NGP expert as a PLY (and optionally an OBJ): InstantNGP.extract_mesh, i.e. the
density on a lattice over the scene box, then marching tetrahedra on the device.

The expert is the production shape of tools/bench_ngp.py.  Its weights come from one of
  --checkpoint FILE   a torch.save()d state_dict of the InstantNGP module (after NGPTrainer.sync_to_modules()), or
  --train-steps N     N steps of NGPTrainer on the synthetic Blender-style scene (as tools/train_psnr.py builds it).
With --save-checkpoint the trained state_dict is written for a later run.  Needs a GPU (no CPU fallback).

  python tools/export_mesh.py --train-steps 2000 --resolution 256 --threshold 10 --out mesh.ply

--colors linear|srgb adds vertex colours (uchar red green blue in the PLY, `v x y z r g b` in the OBJ); --min-faces N
or --keep-largest K removes the small detached components (floaters) on the device before normals and colours are
evaluated.  The JSON line reports the number of components (those with a face) of the unfiltered
surface and the faces before and after the filter.

  python tools/export_mesh.py --train-steps 2000 --colors srgb --min-faces 200 --out mesh.ply

--simplify CELL decimates the surface by vertex clustering on the device (Mesh.simplify): one vertex
per occupied cell of edge CELL (world units), after the component filter and before normals and colours are evaluated.
The JSON line then also reports the faces before the clustering.

  python tools/export_mesh.py --train-steps 2000 --min-faces 200 --simplify 0.02 --out mesh.ply

--simplify-placement quadric puts every cluster's vertex at the minimum of the summed plane quadrics of the faces that
touch the cluster instead of at the members' mean (Mesh.simplify(placement="quadric")): edges, corners and the enclosed
volume are kept, the faces are the same.  The default, mean, changes nothing; with quadric the JSON line also carries
"simplify_placement".

  python tools/export_mesh.py --train-steps 2000 --simplify 0.02 --simplify-placement quadric --out mesh.ply

--smooth N runs N Taubin iterations on the device (Mesh.smooth) after the filter and the clustering and
before normals and colours are evaluated; "grid" normals become the face-derived normals of the smoothed surface.

  python tools/export_mesh.py --train-steps 2000 --min-faces 200 --smooth 10 --out mesh.ply

--report-error (off by default; the files and the first JSON line are unchanged) prints a second JSON line with
Mesh.distance_to between the surface before --simplify / --smooth (after the component filter) and the
exported one: Chamfer, Hausdorff and F-score at one and two lattice spacings, from --error-samples points per surface.
With --exact every sample is measured against the other surface's triangles instead of its samples (DESIGN §3.11.5:
no floor at the sampling spacing) and the line carries "exact": true; without it the line is unchanged.

  python tools/export_mesh.py --train-steps 2000 --simplify 0.02 --smooth 10 --report-error --out mesh.ply

--report-iou (off by default; the files and the other JSON lines are unchanged) prints one more JSON line for the same
pair as --report-error, the exported mesh (a) and the surface before --simplify / --smooth (b): Mesh.iou (DESIGN
§3.11.7), the Monte Carlo volumetric intersection over union from --iou-samples points of their common box, and both
Mesh.volume() values.  All of it means something where the surfaces are closed; a surface that meets the box of the
extraction is open there.  --iou-rule generalized (default parity; the line then carries "rule") calls a point inside
where the generalised winding number is above 0.5, which also answers for open surfaces: use it
with --tsdf, whose meshes are open at every silhouette and unseen region.

  python tools/export_mesh.py --train-steps 2000 --keep-largest 1 --simplify 0.02 --report-iou --out mesh.ply

--report-depth VIEWS (off by default; the files and the other JSON lines are unchanged) prints one more JSON line that
puts the exported mesh next to the field it came from, seen from VIEWS cameras of the synthetic scene at --image-size:
Mesh.render's depth against render_image's.  The field sees a surface where acc > 0.5.  The line gives
the share of pixels where both, only the mesh, only the field or neither see a surface, and the median and the 90th
percentile of |depth_mesh - depth_field| over the pixels where both do.

  python tools/export_mesh.py --train-steps 2000 --min-faces 200 --report-depth 4 --out mesh.ply

--tsdf VIEWS (off by default; the files and every JSON line are unchanged without it) exports the surface that VIEWS
cameras of the synthetic scene see instead of the density level set: InstantNGP.extract_mesh_tsdf
renders depth from scene.hemisphere_poses(VIEWS) at --image-size, fuses it into a TSDF volume of --resolution points and
meshes the zero level; --threshold is then unused.  --tsdf-min-weight is the number of views every corner of a cell
needs for its faces to be kept.  Every option and report above works on it; the first JSON line gains "tsdf" and
"tsdf_min_weight".

  python tools/export_mesh.py --train-steps 2000 --tsdf 32 --report-depth 4 --out mesh.ply

--colors fused (with --tsdf only, an error otherwise) fuses the colour of the rendered views alongside their depth and
colours every vertex from the volume instead of querying the colour network: the route that also
works for models without such a query.  The first JSON line then says "colors": "fused".

  python tools/export_mesh.py --train-steps 2000 --tsdf 32 --colors fused --out mesh.ply

--method dual (default tets; the files and every JSON line are unchanged without it) extracts by dual contouring
 instead of marching tetrahedra: one vertex per sign-changing cell, one quad per sign-changing lattice
edge, about a third of the triangles.  --dual-placement qef|mean chooses the vertex (the minimum of the cell's plane
quadric, or the mean of its crossing points), --dual-hermite field|grid the normals of the crossing points (the field's
own gradient, or the lattice's central differences) and --dual-refine N bisects every crossing point N times along its
lattice edge with the density itself.  Every option and report above works on the result; the first JSON line gains
"method", "dual_placement", "dual_hermite" and "dual_refine".  Not with --tsdf, whose observed-face filter needs one
cell per face.

  python tools/export_mesh.py --train-steps 2000 --method dual --dual-refine 4 --report-depth 4 --out mesh.ply

--texture TEXELS (off by default; the files and every JSON line are unchanged without it) bakes a texture over a
per-face atlas with cells of TEXELS x TEXELS texels as the last step of the extraction and writes a
textured OBJ to --out, with FILE.mtl and FILE.png beside it: the colour detail then no longer falls with the triangle
count, so it pairs with --simplify and --method dual.  The texture takes the colour space of --colors (srgb where that
is none; fused bakes from the TSDF volume).  --out must not be a .ply, which carries no texture coordinates.  The first
JSON line gains "texture" and "texture_side".

  python tools/export_mesh.py --train-steps 2000 --simplify 0.02 --texture 8 --out mesh.obj
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-sys_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CONF = dict(hidden=64, sigma_depth=2, color_hidden=64, color_depth=2, dir_encoding="spherical",
            hash_enc_conf=dict(levels=16, features_per_level=2, log2_hashmap_size=20, min_res=16, max_res=4096,
                               interpolation="Linear"))
AABB = [[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]]


def main():
    ap = argparse.ArgumentParser()
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--checkpoint", help="state_dict of the InstantNGP module")
    src.add_argument("--train-steps", type=int, help="train this many steps on the synthetic scene first")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=96)
    ap.add_argument("--train-views", type=int, default=100)
    ap.add_argument("--image-size", type=int, default=800)
    ap.add_argument("--save-checkpoint", default=None)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=10.0)
    ap.add_argument("--normals", default="field", choices=["field", "grid", "none"])
    ap.add_argument("--colors", default="none", choices=["none", "linear", "srgb", "fused"],
                    help="vertex colours from the colour network, seen head-on along the field normal; fused (with "
                         "--tsdf): the colours of the rendered views, fused in the volume")
    flt = ap.add_mutually_exclusive_group()
    flt.add_argument("--min-faces", type=int, default=None, help="drop connected components with fewer faces")
    flt.add_argument("--keep-largest", type=int, default=None, help="keep the K components with the most faces")
    ap.add_argument("--simplify", type=float, default=None, metavar="CELL",
                    help="vertex clustering with cells of this edge (world units)")
    ap.add_argument("--simplify-placement", choices=["mean", "quadric"], default="mean",
                    help="where --simplify puts a cluster's vertex: the members' mean or the quadric-error minimum")
    ap.add_argument("--smooth", type=int, default=None, metavar="N", help="Taubin smoothing iterations")
    ap.add_argument("--report-error", action="store_true",
                    help="also print the distance between the surface before --simplify / --smooth and the exported one")
    ap.add_argument("--error-samples", type=int, default=2 ** 18, help="points per surface for --report-error")
    ap.add_argument("--exact", action="store_true",
                    help="--report-error measures the samples against the other surface's triangles, not its samples")
    ap.add_argument("--report-iou", action="store_true",
                    help="also print the volumetric IoU of the exported mesh and the surface before --simplify / --smooth")
    ap.add_argument("--iou-samples", type=int, default=2 ** 20, help="points of the common box for --report-iou")
    ap.add_argument("--iou-rule", default="parity", choices=["parity", "winding", "generalized"],
                    help="what --report-iou calls inside: crossing parity, crossing winding, or the generalised "
                         "winding number above 0.5; use generalized with --tsdf, whose surfaces are open")
    ap.add_argument("--report-depth", type=int, default=0, metavar="VIEWS",
                    help="also compare the exported mesh's depth with the field's from this many cameras")
    ap.add_argument("--tsdf", type=int, default=0, metavar="VIEWS",
                    help="export the TSDF fusion of the depth of this many cameras instead of the density level set")
    ap.add_argument("--tsdf-min-weight", type=float, default=1.0,
                    help="--tsdf keeps the faces of cells whose corners were all updated by this many views")
    ap.add_argument("--method", default="tets", choices=["tets", "dual"],
                    help="marching tetrahedra, or dual contouring (one vertex per cell, one quad per crossing edge)")
    ap.add_argument("--dual-placement", default="qef", choices=["qef", "mean"],
                    help="--method dual: the quadric-error minimum of the cell's Hermite data, or the mean of its points")
    ap.add_argument("--dual-hermite", default="field", choices=["field", "grid"],
                    help="--method dual: normals of the crossing points from the field's gradient or the lattice's")
    ap.add_argument("--dual-refine", type=int, default=0, metavar="N",
                    help="--method dual: bisection steps of every crossing point along its lattice edge")
    ap.add_argument("--texture", type=int, default=None, metavar="TEXELS",
                    help="bake a texture with TEXELS x TEXELS texels per pair of faces and write OBJ, MTL and PNG to --out")
    ap.add_argument("--out", default="mesh.ply")
    ap.add_argument("--obj", default=None, help="also write a Wavefront OBJ here")
    a = ap.parse_args()
    if a.colors == "fused" and not a.tsdf:
        ap.error("--colors fused needs --tsdf VIEWS: the colours are fused from the rendered views")
    if a.method == "dual" and a.tsdf:
        ap.error("--method dual does not combine with --tsdf: its observed-face filter needs one cell per face")
    if a.texture is not None:
        if a.out.lower().endswith(".ply"):
            ap.error(f"--texture writes a textured OBJ with its MTL and PNG: give --out FILE.obj, not {a.out!r} "
                     "(a PLY carries no texture coordinates)")
        if a.texture < 5:
            ap.error("--texture needs at least 5 texels: a cell holds two triangles and their gutter")
    dual = dict(method="dual", placement=a.dual_placement, hermite=a.dual_hermite, refine=a.dual_refine) \
        if a.method == "dual" else {}
    if not torch.cuda.is_available():
        raise SystemExit("export_mesh: needs a GPU (no CPU fallback)")
    from nerf_amd.ngp import InstantNGP
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = InstantNGP(occ_conf={}, scene_box=torch.tensor(AABB), **CONF)
    if a.checkpoint:
        model.load_state_dict(torch.load(a.checkpoint, map_location="cpu"))
        model = model.to(dev).eval()
    else:
        from nerf_amd.ngp_trainer import NGPTrainer
        from nerf_amd.scene import make_blender_scene
        from nerf_amd.trainer import RayBatcher
        scene = make_blender_scene(n_train=a.train_views, n_test=1, H=a.image_size, W=a.image_size, seed=0, device=dev)
        model = model.to(dev)
        tr = NGPTrainer(model, n_samples=a.samples, device=dev)
        rb = RayBatcher(scene, dev)
        for step in range(a.train_steps):
            rays, gt = rb.batch(a.batch, seed=step)
            loss = tr.step(rays, gt, seed=step)
        tr.sync_to_modules()
        model.eval()
        print(f"trained {a.train_steps} steps, loss {float(loss):.5f}" if a.train_steps else "untrained", file=sys.stderr)
        if a.save_checkpoint:
            torch.save(model.state_dict(), a.save_checkpoint)
    if a.tsdf:
        import math

        from nerf_amd.scene import hemisphere_poses
        size = a.image_size
        focal = 0.5 * size / math.tan(0.5 * 0.6911112)  # make_blender_scene's
        poses = hemisphere_poses(a.tsdf, seed=0)

        def extract(**kw):
            return model.extract_mesh_tsdf(poses, size, size, focal, focal, size / 2.0, size / 2.0, 2.0, 6.0,
                                           resolution=a.resolution, min_weight=a.tsdf_min_weight,
                                           ray_samples=a.samples, **kw)
    else:
        def extract(**kw):
            return model.extract_mesh(resolution=a.resolution, threshold=a.threshold, **dual, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mesh = extract(normals=None if a.normals == "none" else a.normals, colors=None if a.colors == "none" else a.colors,
                   min_faces=a.min_faces, keep_largest=a.keep_largest, simplify=a.simplify, smooth=a.smooth,
                   simplify_placement=a.simplify_placement, **({} if a.texture is None else {"texture": a.texture}))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if a.texture is None:
        mesh.save_ply(a.out)
    else:
        mesh.save_obj(a.out)
    if a.obj:
        mesh.save_obj(a.obj)
    # for the report only (outside the timed call): the unfiltered surface and its components
    filtered = a.min_faces is not None or a.keep_largest is not None
    full = mesh if not filtered and a.simplify is None else extract(normals=None)
    n_components = int((full.components()[1] > 0).sum())
    after_filter = mesh if a.simplify is None else (
        full.filter_components(min_faces=a.min_faces, keep_largest=a.keep_largest) if filtered else full)
    print(json.dumps({"vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0]),
                      "resolution": a.resolution, "threshold": a.threshold, "normals": a.normals,
                      "colors": a.colors, "min_faces": a.min_faces, "keep_largest": a.keep_largest,
                      "components": n_components, "faces_before_filter": int(full.faces.shape[0]),
                      "faces_after_filter": int(after_filter.faces.shape[0]), "simplify": a.simplify,
                      "smooth": a.smooth,
                      "faces_after_simplify": int(mesh.faces.shape[0]) if a.simplify is not None else None,
                      "extract_seconds": round(dt, 4), "out": a.out,
                      **({"simplify_placement": a.simplify_placement} if a.simplify_placement != "mean" else {}),
                      **({"tsdf": a.tsdf, "tsdf_min_weight": a.tsdf_min_weight} if a.tsdf else {}),
                      **({"texture": a.texture, "texture_side": int(mesh.texture.shape[0])} if a.texture else {}),
                      **({"method": "dual", "dual_placement": a.dual_placement, "dual_hermite": a.dual_hermite,
                          "dual_refine": a.dual_refine} if dual else {})}))
    if a.report_error:
        # the surface the clustering and the smoothing started from: extracted again, filtered, nothing else
        before = extract(normals=None, min_faces=a.min_faces, keep_largest=a.keep_largest)
        h = (AABB[1][0] - AABB[0][0]) / (a.resolution - 1)
        if mesh.faces.shape[0] == 0 or before.faces.shape[0] == 0:
            print(json.dumps({"report_error": None, "reason": "a surface without faces has no samples"}))
        else:
            err = mesh.distance_to(before, n_samples=a.error_samples, thresholds=(h, 2 * h), exact=a.exact)
            print(json.dumps({"report_error": {"a": "exported", "b": "before simplify / smooth",
                                               "samples": a.error_samples, "lattice_spacing": h,
                                               **({"exact": True} if a.exact else {}), **err}}))
    if a.report_iou:
        before = extract(normals=None, min_faces=a.min_faces, keep_largest=a.keep_largest)
        if mesh.faces.shape[0] == 0 or before.faces.shape[0] == 0:
            print(json.dumps({"report_iou": None, "reason": "a surface without faces encloses nothing"}))
        else:
            print(json.dumps({"report_iou": {"a": "exported", "b": "before simplify / smooth",
                                             "mesh_volume_a": mesh.volume(), "mesh_volume_b": before.volume(),
                                             **({"rule": a.iou_rule} if a.iou_rule != "parity" else {}),
                                             **mesh.iou(before, n_samples=a.iou_samples, rule=a.iou_rule)}}))
    if a.report_depth:
        print(json.dumps({"report_depth": depth_report(model, mesh, a.report_depth, a.image_size, a.samples)}))


def depth_report(model, mesh, views, size, samples):
    """The exported mesh against the field it came from, seen from ``views`` cameras of the synthetic scene
    (scene.hemisphere_poses, near 2 / far 6, ``size`` x ``size`` pixels): Mesh.render's depth next to render_image's.
    The field sees a surface where acc > 0.5, the mesh where a face is hit; both depths are in the ray parameter of
    unit directions."""
    import math

    from nerf_amd.ray_rendering import render_image
    from nerf_amd.scene import hemisphere_poses
    focal = 0.5 * size / math.tan(0.5 * 0.6911112)  # make_blender_scene's
    dev = mesh.vertices.device
    cam = dict(H=size, W=size, fx=focal, fy=focal, cx=size / 2.0, cy=size / 2.0)
    grid = None
    both, only_mesh, only_field, neither, diffs = 0, 0, 0, 0, []
    for c2w in hemisphere_poses(views, seed=0):
        _, depth_field, acc = render_image(model, c2w=c2w, near=2.0, far=6.0, ray_samples=samples, **cam)
        if mesh.faces.shape[0] and grid is None:
            from nerf_amd import kernels as K
            grid = K.mesh_face_grid(mesh.vertices, mesh.faces)
        image = mesh.render(c2w=c2w.to(dev), near=2.0, far=6.0, grid=grid, **cam)
        seen_mesh, seen_field = image["mask"].reshape(-1), acc > 0.5
        both += int((seen_mesh & seen_field).sum())
        only_mesh += int((seen_mesh & ~seen_field).sum())
        only_field += int((~seen_mesh & seen_field).sum())
        neither += int((~seen_mesh & ~seen_field).sum())
        diffs.append((image["depth"].reshape(-1) - depth_field)[seen_mesh & seen_field].abs())
    diffs = torch.cat(diffs).to(torch.float64)
    n = float(views * size * size)
    q = torch.quantile(diffs, torch.tensor([0.5, 0.9], dtype=torch.float64, device=diffs.device)).tolist() \
        if diffs.numel() else [None, None]
    return {"views": views, "image_size": size, "faces": int(mesh.faces.shape[0]), "both": both / n,
            "only_mesh": only_mesh / n, "only_field": only_field / n, "neither": neither / n,
            "depth_diff_median": q[0], "depth_diff_p90": q[1]}


if __name__ == "__main__":
    main()
