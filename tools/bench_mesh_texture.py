#!/usr/bin/env python3
"""Timing of texture baking (csrc/mesh_texture.hip).  A record, not a gate: the feature has no parent
to compare with, so nothing is required of the figures.

  texels   nerf_mesh_atlas_texels on the marching-tetrahedra mesh of an analytic sphere field 0.6 - |x| on [-1,1]^3
           (tools/bench_mesh.py's field) at --size^3 lattice points, with cells of --texels texels: with the face's own
           normal, with the mix of vertex normals, and without normals.  Bytes: what the kernel must store (4 + 8 + 12
           bytes per texel, 12 more with normals) plus one read of the faces and of the vertices; the corners that the
           texels of a face re-read come from the caches and are not counted.
  lookup   nerf_mesh_texture_lookup of --lookups random (face, barycentric pair) on the C = 3 texture of that atlas,
           with the faces in random order and sorted (what a rendered image's coherent hits look like).  Bytes: 12 read
           and 12 written per lookup plus the four texels of 12 bytes it gathers; the gathers arrive in cache lines,
           of which a random lookup uses a fraction, so this counts what the lookup needs, not what the memory moves.
           Back-to-back calls repeat the same lookups, and a texture below 256 MB then stays in the Infinity Cache:
           these figures are cache rates where they pass what HBM delivers.

Each figure is the device time between two events around back-to-back calls after `--warmup` untimed ones: at least
`--inner` calls, and as many as fill a window of about 40 ms.  The median over `--rounds` rounds is reported with the
fastest and slowest, and next to it the counted bytes per second and their share of the 6.3 TB/s that HBM delivers to
a streaming kernel on the MI355X (8 TB/s is the specification).  Needs a GPU (no CPU fallback).  Prints one JSON line
and writes it to --out.

  python tools/bench_mesh_texture.py [--size N] [--texels S] [--lookups N] [--rounds R] [--inner I] [--warmup W]
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

from bench_mesh import sphere_field, timed  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.3


def rate(res, nbytes):
    for k, b in nbytes.items():
        tbs = b / (res[k]["ms_median"] * 1e-3) / 1e12
        res[k].update(bytes=int(b), tb_per_s=round(tbs, 4), hbm_share=round(tbs / HBM_ACHIEVABLE_TBS, 4))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--texels", type=int, default=8)
    ap.add_argument("--lookups", type=int, default=2 ** 20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_texture.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_texture: needs a GPU (timings on a CPU say nothing about the MI355X)")
    from nerf_amd import kernels as K
    from nerf_amd._lib import check, lib, ptr, stream
    dev = torch.device("cuda:0")
    L = lib()
    verts, faces, vn = K.mesh_extract(sphere_field(a.size, dev), 0.0, [-1.0] * 3, [1.0] * 3, normals=True)
    V, F, S = int(verts.shape[0]), int(faces.shape[0]), a.texels
    cols, T = K.atlas_layout(F, S)
    face = torch.empty((T, T), dtype=torch.int32, device=dev)
    bary = torch.empty((T, T, 2), dtype=torch.float32, device=dev)
    pos = torch.empty((T, T, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((T, T, 3), dtype=torch.float32, device=dev)

    def texels(vertex_normals, normal):
        check(L.nerf_mesh_atlas_texels(ptr(verts), ptr(faces), F, S, T, ptr(vertex_normals), ptr(face), ptr(bary),
                                       ptr(pos), ptr(normal), stream()), "texels")

    texels(vn, nrm)
    ref = K.mesh_atlas_texels(verts, faces, S, vertex_normals=vn)
    same = all(torch.equal(x.view(torch.int32), ref[k].view(torch.int32))
               for k, x in (("face", face), ("bary", bary), ("position", pos), ("normal", nrm)))
    owned = int((face >= 0).sum())
    mesh_bytes = 12 * F + 12 * V
    res = rate(timed({"texels_face_normals": lambda: texels(None, nrm), "texels_vertex_normals": lambda: texels(vn, nrm),
                      "texels_no_normals": lambda: texels(None, None)}, a.rounds, a.inner, a.warmup),
               {"texels_face_normals": 36 * T * T + mesh_bytes, "texels_vertex_normals": 36 * T * T + mesh_bytes + 12 * V,
                "texels_no_normals": 24 * T * T + mesh_bytes})

    N = a.lookups
    g = torch.Generator(device=dev).manual_seed(0)
    texture = torch.rand((T, T, 3), generator=g, device=dev)
    qf = torch.randint(0, F, (N,), generator=g, device=dev, dtype=torch.int32)
    uv = torch.rand((N, 2), generator=g, device=dev)
    uv = torch.where((uv.sum(1) > 1)[:, None], 1.0 - uv, uv).contiguous()
    qs = torch.sort(qf).values.contiguous()
    out = torch.empty((N, 3), dtype=torch.float32, device=dev)

    def lookup(f):
        check(L.nerf_mesh_texture_lookup(ptr(texture), T, 3, F, S, ptr(f), ptr(uv), N, ptr(out), stream()), "lookup")

    lookup(qf)
    same_lookup = bool(torch.equal(out, K.mesh_texture_lookup(texture, S, F, qf, uv)))
    lk = (24 + 4 * 12) * N
    res.update(rate(timed({"lookup_random_faces": lambda: lookup(qf), "lookup_sorted_faces": lambda: lookup(qs)},
                          a.rounds, a.inner, a.warmup), {"lookup_random_faces": lk, "lookup_sorted_faces": lk}))
    res = {"bench": "mesh_texture", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
           "hbm_achievable_tb_per_s": HBM_ACHIEVABLE_TBS, "size": a.size, "vertices": V, "faces": F, "texels": S,
           "cols": cols, "T": T, "texels_total": T * T, "texels_owned": owned, "lookups": N,
           "pieces_equal_wrappers": bool(same and same_lookup), **res}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
