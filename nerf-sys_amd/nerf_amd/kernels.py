"""Typed wrappers over the C-ABI: allocate outputs with torch (caller-owned buffers), launch on the
current stream, raise on a non-zero status.  No autograd here (see ray_rendering / vanilla)."""
from __future__ import annotations

import ctypes
from typing import Sequence

import torch

from ._lib import check, lib, need, ptr, stream

F32 = torch.float32
_CS = {"linear": 0, "srgb": 1, "identity": 2}


def _empty(shape, like):
    return torch.empty(shape, dtype=F32, device=like.device)


def rays_gen(c2w, H, W, fx, fy, cx, cy, *, pix=None, near=None, far=None, aabb=None, center_pixels=True,
             images_u8=None, aabb_max_bound=1e10, aabb_invalid=1e10):
    """get_rays(get_ray_directions(...)) for a dense image (pix=None) or a batch of (img,row,col)."""
    need(c2w, "c2w")
    if c2w.dim() == 2:
        c2w = c2w[:3, :4].reshape(1, 3, 4).contiguous()
    c2w = c2w[..., :3, :4].contiguous()
    n_poses = c2w.shape[0]
    if pix is not None:
        need(pix, "pix", torch.int32)
        n = pix.shape[0]
    else:
        n = H * W
    if aabb is None and (near is None or far is None):
        raise ValueError("Provide near/far when scene_box is None")
    if aabb is not None:
        aabb = need(aabb.reshape(6).contiguous(), "aabb")
    rays = torch.empty((n, 8), dtype=F32, device=c2w.device)
    rgb = torch.empty((n, 3), dtype=F32, device=c2w.device) if images_u8 is not None else None
    if images_u8 is not None:
        need(images_u8, "images_u8", torch.uint8)
    st = lib().nerf_rays_gen(ptr(c2w), n_poses, ptr(pix), n, H, W, fx, fy, cx, cy, int(center_pixels),
                             float(near or 0.0), float(far or 0.0), ptr(aabb), aabb_max_bound, aabb_invalid,
                             ptr(images_u8), ptr(rays), ptr(rgb), stream())
    check(st, "nerf_rays_gen")
    return (rays, rgb) if images_u8 is not None else rays


def pick_pixels(n, n_images, H, W, seed, device, step_dev=None, seed_mul=0):
    """n random (image, row, col) triples of the counter RNG stream ``seed``; with ``step_dev`` (int64 device
    counter) the stream is seed + step_dev * seed_mul, read by the kernel (captured train-step graphs)."""
    pix = torch.empty((n, 3), dtype=torch.int32, device=device)
    if step_dev is not None:
        need(step_dev, "step_dev", torch.int64)
        check(lib().nerf_pick_pixels_dseed(n, n_images, H, W, ctypes.c_uint64(seed & (2**64 - 1)),
                                           ctypes.c_uint64(seed_mul & (2**64 - 1)), ptr(step_dev), ptr(pix),
                                           stream()), "nerf_pick_pixels_dseed")
        return pix
    check(lib().nerf_pick_pixels(n, n_images, H, W, ctypes.c_uint64(seed & (2**64 - 1)), ptr(pix), stream()),
          "nerf_pick_pixels")
    return pix


def clamp_near_far(rays, near=None, far=None, eps=1e-6, invalid_value=float("inf")):
    need(rays, "rays")
    rays = rays.clone()
    valid = torch.empty(rays.shape[0], dtype=torch.uint8, device=rays.device)
    check(lib().nerf_clamp_near_far(ptr(rays), rays.shape[0], int(near is not None), float(near or 0.0),
                                    int(far is not None), float(far or 0.0), eps, invalid_value, ptr(valid),
                                    stream()), "nerf_clamp_near_far")
    return rays, valid.bool()


def rays_ndc(rays, H, W, focal, near_plane=1.0):
    need(rays, "rays")
    out = torch.empty_like(rays)
    check(lib().nerf_rays_ndc(ptr(rays), rays.shape[0], H, W, focal, near_plane, ptr(out), stream()), "nerf_rays_ndc")
    return out


def sample_stratified(rays, S, randomized, u=None, seed=0):
    need(rays, "rays")
    if u is not None:
        need(u, "u")
    t = _empty((rays.shape[0], S), rays)
    check(lib().nerf_sample_stratified(ptr(rays), rays.shape[0], S, int(bool(randomized)), ptr(u),
                                       ctypes.c_uint64(seed & (2**64 - 1)), ptr(t), stream()),
          "nerf_sample_stratified")
    return t


def build_xd(rays, t):
    need(rays, "rays"), need(t, "t")
    n, S = t.shape
    xd = _empty((n * S, 6), rays)
    check(lib().nerf_build_xd(ptr(rays), ptr(t), n, S, ptr(xd), stream()), "nerf_build_xd")
    return xd


def sample_pdf(t, w, n_imp, u=None, det=False, seed=0):
    need(t, "t"), need(w, "weights")
    if u is not None:
        need(u, "u")
    n, S = t.shape
    out = _empty((n, S + n_imp), t)
    check(lib().nerf_sample_pdf(ptr(t), ptr(w), n, S, n_imp, ptr(u), int(bool(det)),
                                ctypes.c_uint64(seed & (2**64 - 1)), ptr(out), stream()), "nerf_sample_pdf")
    return out


def freq_encode(x, L, include_input=True):
    need(x, "x")
    D = x.shape[-1]
    flat = x.reshape(-1, D)
    od = D * (2 * L + (1 if include_input else 0))
    out = _empty((flat.shape[0], od), x)
    check(lib().nerf_freq_encode(ptr(flat), flat.shape[0], D, L, int(include_input), ptr(out), od, stream()),
          "nerf_freq_encode")
    return out.view(*x.shape[:-1], od)


# ------------------------------------------------------------------ MLP


PRECISIONS = ("fp32", "bf16", "fp16")
# the 16-bit builds of the fused MLP kernels (include/nerf_amd.h): bf16 (configs[2], autocast(bfloat16)) and fp16 (the
# reference's autocast(float16) operands and rounding points, runtime_adapt.py:291-310)
_H16 = {"bf16": "bf16", "fp16": "f16"}
# bf16 path selection (include/nerf_amd.h): 0 = the fused production kernels; the layered launches are their
# bitwise references.  A workspace's backward must use the NERF_BF16_LAYERED_BWD bit of its training forward.
BF16_LAYERED_FWD = 1
BF16_LAYERED_BWD = 2


def _check_precision(precision):
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")


def mlp_workspace_bytes(M, training, precision="fp32"):
    _check_precision(precision)
    if precision in _H16:
        return getattr(lib(), f"nerf_mlp_workspace_bytes_{_H16[precision]}")(M, int(training))
    return lib().nerf_mlp_workspace_bytes(M, int(training))


def mlp_workspace_bytes_2s(M):
    """Workspace of the two-stream fp32 backward (nerf_mlp_bwd_2s): one input-gradient buffer per trunk layer."""
    return lib().nerf_mlp_workspace_bytes_2s(M)


def mlp_workspace(M, training, device, precision="fp32"):
    return torch.empty(mlp_workspace_bytes(M, training, precision), dtype=torch.uint8, device=device)


def _events_arg(events):
    if events is None:
        return None
    arr = (ctypes.c_void_p * len(events))(*[ctypes.c_void_p(e.cuda_event) for e in events])
    return arr


# fp32 GEMM engine flags (include/nerf_amd.h): 0 = bf16 split products (default), NATIVE_FP32 = fp32 MFMA kernels
MLP_NATIVE_FP32 = 1
MLP_NATIVE_DGRAD = 2  # backward only: input-gradient GEMMs on the fp32 MFMA (default: split, small-term accumulators)
MLP_FWD_LAYERED = 4  # forward only: one GEMM launch per trunk layer (default: one chained launch; bitwise the same)
MLP_BWD_LAYERED = 8  # backward only: one input-gradient launch per trunk layer (default: one chained launch; bitwise the same)


def mlp_fwd(w_packed, x_d, ws, training, out=None, events=None, precision="fp32", bf16_flags=0, fp32_flags=0):
    need(w_packed, "packed weights"), need(x_d, "x_d")
    _check_precision(precision)
    M = x_d.shape[0]
    if out is None:
        out = _empty((M, 4), x_d)
    if precision in _H16:
        fn = f"nerf_mlp_fwd_{_H16[precision]}"
        check(getattr(lib(), fn)(ptr(w_packed), ptr(x_d), M, ptr(out), ptr(ws), ws.numel(), int(training),
                                 int(bf16_flags), _events_arg(events), stream()), fn)
        return out
    check(lib().nerf_mlp_fwd_ex(ptr(w_packed), ptr(x_d), M, ptr(out), ptr(ws), ws.numel(), int(training),
                                int(fp32_flags) & ~MLP_NATIVE_DGRAD,  # MLP_NATIVE_DGRAD is a backward-only flag
                                _events_arg(events), stream()), "nerf_mlp_fwd_ex")
    return out


def mlp_bwd(w_packed, M, d_rgb_sigma, ws, d_w=None, accumulate=False, events=None, precision="fp32", bf16_flags=0,
            wgrad_stream=None, sync=None, fp32_flags=0):
    """wgrad_stream (fp32 only): run the weight-gradient GEMMs there (nerf_mlp_bwd_2s; sync = 10 torch.cuda.Events,
    ws from mlp_workspace_bytes_2s); d_w is complete in the current stream's order either way."""
    need(w_packed, "packed weights"), need(d_rgb_sigma, "d_rgb_sigma")
    _check_precision(precision)
    if d_w is None:
        d_w = torch.empty_like(w_packed)
        accumulate = False
    if precision in _H16:
        fn = f"nerf_mlp_bwd_{_H16[precision]}"
        check(getattr(lib(), fn)(ptr(w_packed), M, ptr(d_rgb_sigma), ptr(d_w), int(accumulate), ptr(ws),
                                 ws.numel(), int(bf16_flags), _events_arg(events), stream()), fn)
        return d_w
    if wgrad_stream is not None:
        if sync is None or len(sync) < 10:
            raise ValueError("nerf_mlp_bwd_2s needs 10 sync events")
        for e in sync:  # torch creates an event's HIP handle at its first record
            if not e.cuda_event:
                e.record()
        check(lib().nerf_mlp_bwd_2s_ex(ptr(w_packed), M, ptr(d_rgb_sigma), ptr(d_w), int(accumulate), ptr(ws),
                                       ws.numel(), int(fp32_flags) & ~MLP_FWD_LAYERED, _events_arg(events), stream(),
                                       ctypes.c_void_p(wgrad_stream.cuda_stream), _events_arg(sync)),
              "nerf_mlp_bwd_2s_ex")
        return d_w
    check(lib().nerf_mlp_bwd_ex(ptr(w_packed), M, ptr(d_rgb_sigma), ptr(d_w), int(accumulate), ptr(ws), ws.numel(),
                                int(fp32_flags) & ~MLP_FWD_LAYERED,  # MLP_FWD_LAYERED is a forward-only flag
                                _events_arg(events), stream()), "nerf_mlp_bwd_ex")
    return d_w


# ------------------------------------------------------------------ compositing


def composite_fwd(rgb_sigma, t, bg=None, sigma_scale=1.0, gt=None, color_space="linear", inv_count=None,
                  loss_sum=None, outs=None):
    need(rgb_sigma, "rgb_sigma"), need(t, "t")
    n, S = t.shape
    if bg is not None:
        need(bg, "bg")
    if outs is None:
        rgb, depth, w, acc = _empty((n, 3), t), _empty((n,), t), _empty((n, S), t), _empty((n,), t)
    else:
        rgb, depth, w, acc = outs
    d_rgb = None
    if gt is not None:
        need(gt, "gt")
        d_rgb = _empty((n, 3), t)
        if loss_sum is None:
            loss_sum = torch.zeros(1, dtype=F32, device=t.device)
        if inv_count is None:
            inv_count = 1.0 / (3 * n)
    cs = _CS.get(color_space)
    if cs is None:
        raise ValueError(f"Invalid color_space={color_space!r}; use 'linear'|'srgb'|'identity'")
    check(lib().nerf_composite_fwd(ptr(rgb_sigma), ptr(t), ptr(bg), n, S, float(sigma_scale), ptr(rgb), ptr(depth),
                                   ptr(w), ptr(acc), ptr(gt), cs, float(inv_count or 0.0), ptr(loss_sum),
                                   ptr(d_rgb), stream()), "nerf_composite_fwd")
    if gt is not None:
        return rgb, depth, w, acc, loss_sum, d_rgb
    return rgb, depth, w, acc


def composite_bwd(rgb_sigma, t, bg, g_rgb, g_depth=None, g_acc=None, g_w=None, sigma_scale=1.0, out=None):
    need(rgb_sigma, "rgb_sigma"), need(t, "t"), need(g_rgb, "g_rgb")
    n, S = t.shape
    if rgb_sigma.numel() != n * S * 4 or rgb_sigma.shape[-1] != 4:   # (N,S,4) or the MLP's (N*S,4)
        raise ValueError(f"rgb_sigma must hold ({n},{S},4), got {tuple(rgb_sigma.shape)}")
    if tuple(g_rgb.shape) != (n, 3):
        raise ValueError(f"g_rgb must be ({n},3), got {tuple(g_rgb.shape)}")
    for x, name, shape in ((bg, "bg", (n, 3)), (g_depth, "g_depth", (n,)), (g_acc, "g_acc", (n,)),
                           (g_w, "g_w", (n, S))):
        if x is not None:
            need(x, name)
            if tuple(x.shape) != shape:
                raise ValueError(f"{name} must be {shape}, got {tuple(x.shape)}")
    if out is None:
        out = torch.empty_like(rgb_sigma)
    else:
        need(out, "out")
    check(lib().nerf_composite_bwd(ptr(rgb_sigma), ptr(t), ptr(bg), n, S, float(sigma_scale), ptr(g_rgb),
                                   ptr(g_depth), ptr(g_acc), ptr(g_w), ptr(out), stream()), "nerf_composite_bwd")
    return out


# ------------------------------------------------------------------ image metrics


def image_metrics_tile():
    """(tile_h, tile_w): the SSIM-map pixels one workgroup of nerf_image_metrics covers."""
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().nerf_image_metrics_tile(ctypes.byref(th), ctypes.byref(tw)), "nerf_image_metrics_tile")
    return th.value, tw.value


def image_metrics_workspace_bytes(n_img, H, W):
    return lib().nerf_image_metrics_workspace_bytes(n_img, H, W)


def image_metrics(pred, gt, color_space="linear", out=None, ws=None):
    """nerf_image_metrics: pred (H,W,3) or (N,H,W,3) linear float32 against gt of the same shape, float32 or uint8
    (8-bit sRGB, v / 255) -> (N,4) float32 = mse, ssim_r, ssim_g, ssim_b in ``color_space``.  ``ws`` is a uint8 device
    buffer of image_metrics_workspace_bytes(N, H, W) bytes."""
    need(pred, "pred")
    need(gt, "gt", torch.uint8 if isinstance(gt, torch.Tensor) and gt.dtype == torch.uint8 else F32)
    cs = _CS.get(color_space)
    if cs is None:
        raise ValueError(f"Invalid color_space={color_space!r}; use 'linear'|'srgb'|'identity'")
    if pred.dim() not in (3, 4) or pred.shape[-1] != 3:
        raise ValueError(f"pred must be (H,W,3) or (N,H,W,3), got {tuple(pred.shape)}")
    if tuple(gt.shape) != tuple(pred.shape):
        raise ValueError(f"gt must have pred's shape {tuple(pred.shape)}, got {tuple(gt.shape)}")
    n = pred.shape[0] if pred.dim() == 4 else 1
    H, W = int(pred.shape[-3]), int(pred.shape[-2])
    if out is None:
        out = _empty((n, 4), pred)
    else:
        need(out, "out")
        if tuple(out.shape) != (n, 4):
            raise ValueError(f"out must be ({n},4), got {tuple(out.shape)}")
    if ws is None:
        ws = torch.empty(max(int(image_metrics_workspace_bytes(n, H, W)), 0), dtype=torch.uint8, device=pred.device)
    else:
        need(ws, "ws", torch.uint8)
    u8 = gt.dtype == torch.uint8
    check(lib().nerf_image_metrics(ptr(pred), None if u8 else ptr(gt), ptr(gt) if u8 else None, n, H, W, cs,
                                   ptr(ws), ws.numel(), ptr(out), stream()), "nerf_image_metrics")
    return out


# ------------------------------------------------------------------ mesh extraction


def _box3(v, name):
    v = [float(x) for x in (v.reshape(-1).tolist() if isinstance(v, torch.Tensor) else v)]
    if len(v) != 3:
        raise ValueError(f"{name} must hold 3 floats, got {len(v)}")
    return v


def mesh_extract(field, iso, lo, hi, normals=False, face_offsets=False):
    """Marching tetrahedra (nerf_mesh_classify -> two scans -> nerf_mesh_emit): field (nx,ny,nz) float32, finite, every
    dimension >= 2, sampled at lo + (ix,iy,iz) (hi - lo) / (n - 1); inside iff field > iso.  Returns verts (V,3)
    float32 and faces (F,3) int32 (welded: one vertex per crossing lattice edge; face normals towards lower values),
    and with ``normals`` the unit normals (V,3) of the lattice's central-difference gradient.  With ``face_offsets``
    the tuple gains, as its last element, face_off (nx ny nz + 1,) int32: the faces of the cell with low corner p are
    [face_off[p], face_off[p+1]).  Two host reads: the finiteness check and the two totals that size the outputs.
    Bitwise reproducible (no atomics)."""
    from .occupancy import exclusive_scan
    need(field, "field")
    if field.dim() != 3:
        raise ValueError(f"field must be (nx,ny,nz), got {tuple(field.shape)}")
    nx, ny, nz = (int(n) for n in field.shape)
    if min(nx, ny, nz) < 2:
        raise ValueError(f"every lattice dimension must be >= 2, got {(nx, ny, nz)}")
    lo, hi = _box3(lo, "lo"), _box3(hi, "hi")
    if not all(a < b for a, b in zip(lo, hi)):
        raise ValueError(f"lo must be below hi on every axis, got {lo} vs {hi}")
    dev, P = field.device, nx * ny * nz
    if 12 * P >= 2 ** 31:  # int32 scans of up to 12 triangles per cell (512^3 still fits)
        raise ValueError(f"lattice too large: 12 * {P} points reaches 2^31")
    if not bool(torch.isfinite(field).all()):
        raise ValueError("field must be finite")
    mask = torch.empty(P, dtype=torch.uint8, device=dev)
    vcnt = torch.empty(P, dtype=torch.int32, device=dev)  # two allocations: the scan wants 16-byte aligned inputs
    fcnt = torch.empty(P, dtype=torch.int32, device=dev)
    check(lib().nerf_mesh_classify(ptr(field), nx, ny, nz, float(iso), ptr(mask), ptr(vcnt), ptr(fcnt), stream()),
          "nerf_mesh_classify")
    voff, foff = exclusive_scan(vcnt), exclusive_scan(fcnt)
    V, F = (int(v) for v in torch.stack([voff[-1], foff[-1]]).tolist())
    verts = torch.empty((V, 3), dtype=F32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    nrm = torch.empty((V, 3), dtype=F32, device=dev) if normals else None
    lo_c, hi_c = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi)
    check(lib().nerf_mesh_emit(ptr(field), nx, ny, nz, float(iso), lo_c, hi_c, ptr(mask), ptr(voff), ptr(foff), V, F,
                               ptr(verts) if V else None, ptr(faces) if F else None,
                               ptr(nrm) if normals and V else None, stream()), "nerf_mesh_emit")
    out = (verts, faces, nrm) if normals else (verts, faces)
    return out + (foff,) if face_offsets else out


# ------------------------------------------------------------------ dual contouring

_DUAL_PLACEMENT = {"mean": 0, "qef": 1}


class DualLattice:
    """What mesh_dual_hermite found on a lattice and mesh_dual_vertices needs again: the field, iso and the box, the
    crossing bits of every point's three axis edges (mask), the exclusive scans of the edge, cell and face counts
    (nx ny nz + 1 entries each, int32) and their totals E, V, F."""
    __slots__ = ("field", "iso", "lo", "hi", "mask", "edge_off", "cell_off", "face_off", "E", "V", "F")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def _hermite_arg(t, name, E, dev):
    need(t, name)
    if tuple(t.shape) != (E, 3):
        raise ValueError(f"{name} must be ({E},3), got {tuple(t.shape)}")
    if t.device != dev:
        raise ValueError(f"{name} must be on {dev}, got {t.device}")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} must be finite")
    return t


def mesh_dual_hermite(field, iso, lo, hi, normals=True):
    """The Hermite data of dual contouring (nerf_mesh_dual_classify -> three scans -> nerf_mesh_dual_edges): field, iso
    and the box as mesh_extract takes them.  Returns (record, points, normals, keys): a DualLattice, and for the E
    crossing axis edges of the lattice, ordered by (point, axis), the crossing point (E,3) float32 (the bits of
    mesh_extract's vertex on that edge), with ``normals`` the unit grid normal (E,3) float32 (else None), and
    keys (E,) int32 = 3 p + a.  Two host reads: the finiteness check and the three totals."""
    from .occupancy import exclusive_scan
    need(field, "field")
    if field.dim() != 3:
        raise ValueError(f"field must be (nx,ny,nz), got {tuple(field.shape)}")
    nx, ny, nz = (int(n) for n in field.shape)
    if min(nx, ny, nz) < 2:
        raise ValueError(f"every lattice dimension must be >= 2, got {(nx, ny, nz)}")
    lo, hi = _box3(lo, "lo"), _box3(hi, "hi")
    if not all(a < b for a, b in zip(lo, hi)):
        raise ValueError(f"lo must be below hi on every axis, got {lo} vs {hi}")
    dev, P = field.device, nx * ny * nz
    if 12 * P >= 2 ** 31:  # the bound of mesh_extract, so that both methods take the same lattices
        raise ValueError(f"lattice too large: 12 * {P} points reaches 2^31")
    if not bool(torch.isfinite(field).all()):
        raise ValueError("field must be finite")
    mask = torch.empty(P, dtype=torch.uint8, device=dev)
    ecnt, ccnt, fcnt = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))  # 16-byte aligned each
    check(lib().nerf_mesh_dual_classify(ptr(field), nx, ny, nz, float(iso), ptr(mask), ptr(ecnt), ptr(ccnt), ptr(fcnt),
                                        stream()), "nerf_mesh_dual_classify")
    eoff, coff, foff = exclusive_scan(ecnt), exclusive_scan(ccnt), exclusive_scan(fcnt)
    E, V, F = (int(v) for v in torch.stack([eoff[-1], coff[-1], foff[-1]]).tolist())
    points = torch.empty((E, 3), dtype=F32, device=dev)
    nrm = torch.empty((E, 3), dtype=F32, device=dev) if normals else None
    keys = torch.empty(E, dtype=torch.int32, device=dev)
    lo_c, hi_c = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi)
    check(lib().nerf_mesh_dual_edges(ptr(field), nx, ny, nz, float(iso), lo_c, hi_c, ptr(mask), ptr(eoff), E,
                                     ptr(points) if E else None, ptr(nrm) if normals and E else None,
                                     ptr(keys) if E else None, stream()), "nerf_mesh_dual_edges")
    rec = DualLattice(field=field, iso=float(iso), lo=lo, hi=hi, mask=mask, edge_off=eoff, cell_off=coff, face_off=foff,
                      E=E, V=V, F=F)
    return rec, points, nrm, keys


def mesh_dual_vertices(record, points, normals=None, placement="qef", tol=1e-3, vertex_normals=False,
                       return_fallback=False):
    """The dual mesh of a lattice from Hermite data (nerf_mesh_dual_cells): ``record`` from mesh_dual_hermite, points
    (E,3) and normals (E,3) float32, finite, in that call's order; they may be what it returned or a replacement
    (refined crossings, normals of the field itself).  One vertex per sign-changing cell: placement "mean" is the mean
    of the cell's crossing points (surface nets); "qef" minimises the plane quadric of the cell's points and normals,
    starting at that mean, with eigenvalues below ``tol`` x the largest truncated (0 < tol < 1), and keeps the mean
    where the minimiser leaves the cell.  One quad (two triangles) per crossing edge whose four cells exist, normals
    towards lower values; the surface is open at the box.  Returns verts (V,3) float32, faces (F,3) int32, then with
    ``vertex_normals`` the normalised sums of each cell's edge normals (V,3) float32, then with ``return_fallback``
    fallback (V,) uint8, 1 where "qef" kept the mean.  "qef" and ``vertex_normals`` need ``normals``.  A cell that two
    sheets cross still gets one vertex, so noisy fields can give edges shared by more than two triangles.  Bitwise
    reproducible (no atomics)."""
    if not isinstance(record, DualLattice):
        raise ValueError("record must be the DualLattice that mesh_dual_hermite returned")
    if placement not in _DUAL_PLACEMENT:
        raise ValueError(f'placement must be "qef" or "mean", got {placement!r}')
    tol = float(tol)
    if not 0.0 < tol < 1.0:  # a NaN fails both
        raise ValueError(f"tol must be in (0, 1), got {tol}")
    if normals is None and (placement == "qef" or vertex_normals):
        raise ValueError('placement="qef" and vertex_normals need the (E,3) normals')
    field = record.field
    dev = field.device
    nx, ny, nz = (int(n) for n in field.shape)
    E, V, F = record.E, record.V, record.F
    _hermite_arg(points, "points", E, dev)
    if normals is not None:
        _hermite_arg(normals, "normals", E, dev)
    verts = torch.empty((V, 3), dtype=F32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    vnrm = torch.empty((V, 3), dtype=F32, device=dev) if vertex_normals else None
    fb = torch.empty(V, dtype=torch.uint8, device=dev) if return_fallback else None
    if V:
        lo_c, hi_c = (ctypes.c_float * 3)(*record.lo), (ctypes.c_float * 3)(*record.hi)
        check(lib().nerf_mesh_dual_cells(ptr(field), nx, ny, nz, record.iso, lo_c, hi_c, ptr(record.mask),
                                         ptr(record.edge_off), ptr(record.cell_off), ptr(record.face_off), ptr(points),
                                         ptr(normals), _DUAL_PLACEMENT[placement], tol, V, F, ptr(verts),
                                         ptr(faces) if F else None, ptr(vnrm), ptr(fb), stream()),
              "nerf_mesh_dual_cells")
    out = (verts, faces)
    if vertex_normals:
        out += (vnrm,)
    if return_fallback:
        out += (fb,)
    return out


def mesh_extract_dual(field, iso, lo, hi, placement="qef", tol=1e-3, normals=False):
    """Dual contouring with the lattice's own Hermite data: mesh_dual_hermite then mesh_dual_vertices with the grid
    normals.  Returns verts (V,3) float32 and faces (F,3) int32, and with ``normals`` the cell normals (V,3)."""
    if placement not in _DUAL_PLACEMENT:
        raise ValueError(f'placement must be "qef" or "mean", got {placement!r}')
    rec, points, nrm, _ = mesh_dual_hermite(field, iso, lo, hi, normals=True)
    return mesh_dual_vertices(rec, points, nrm, placement=placement, tol=tol, vertex_normals=normals)


# ------------------------------------------------------------------ TSDF fusion of depth views


def _volume_arg(t, name, shape=None):
    need(t, name)
    if t.dim() != 3 or min(t.shape) < 2:
        raise ValueError(f"{name} must be (nx,ny,nz) with every dimension >= 2, got {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
    if t.numel() >= 2 ** 31:
        raise ValueError(f"lattice too large: {t.numel()} points reaches 2^31")
    return tuple(int(n) for n in t.shape)


def _f32_arg(v, name, positive):
    """v as a finite (and positive) fp32, else ValueError"""
    try:
        f = float(torch.tensor(float(v), dtype=F32))
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{name} must be a number, got {v!r}") from None
    if f != f or f in (float("inf"), float("-inf")) or (positive and not f > 0.0):
        raise ValueError(f"{name} must be a finite{' positive' if positive else ''} float32, got {v!r}")
    return f


def _tsdf_views_args(tsdf, weight, lo, hi, depth, c2w, fx, fy, cx, cy, trunc):
    """the checks of tsdf_integrate -> shape, lo, hi, depth (n,H,W), c2w (n,3|4,4), (n, H, W), (fx, fy, cx, cy, trunc)"""
    shape = _volume_arg(tsdf, "tsdf")
    _volume_arg(weight, "weight", shape)
    if tsdf.device != weight.device:
        raise ValueError("tsdf and weight must be on one device")
    lo, hi = _box3(lo, "lo"), _box3(hi, "hi")
    if not all(a < b for a, b in zip(lo, hi)):
        raise ValueError(f"lo must be below hi on every axis, got {lo} vs {hi}")
    need(depth, "depth")
    need(c2w, "c2w")
    if depth.device != tsdf.device or c2w.device != tsdf.device:
        raise ValueError("depth and c2w must be on the volume's device")
    if depth.dim() == 2:
        depth = depth[None]
    if depth.dim() != 3 or (depth.shape[0] and min(depth.shape[1:]) < 1):
        raise ValueError(f"depth must be (n,H,W) or (H,W) with H, W >= 1, got {tuple(depth.shape)}")
    if c2w.dim() == 2:
        c2w = c2w[None]
    if c2w.dim() != 3 or tuple(c2w.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"c2w must be (n,3,4), (n,4,4), (3,4) or (4,4), got {tuple(c2w.shape)}")
    n, H, W = (int(v) for v in depth.shape)
    if max(H, W) > 2 ** 24:
        raise ValueError(f"H and W must be at most 2^24, got {H}, {W}")
    if c2w.shape[0] != n:
        raise ValueError(f"depth holds {n} views, c2w {c2w.shape[0]}")
    fx, fy = _f32_arg(fx, "fx", True), _f32_arg(fy, "fy", True)
    cx, cy = _f32_arg(cx, "cx", False), _f32_arg(cy, "cy", False)
    trunc = _f32_arg(trunc, "trunc", True)
    return shape, lo, hi, depth, c2w, (n, H, W), (fx, fy, cx, cy, trunc)


def _tsdf_rows(c2w):
    """(n,12) contiguous rows of the 3x4 matrices; one host read: their finiteness"""
    rows = c2w[:, :3, :].contiguous()
    if not bool(torch.isfinite(rows).all()):
        raise ValueError("c2w must be finite")
    return rows


def tsdf_integrate(tsdf, weight, lo, hi, depth, c2w, fx, fy, cx, cy, trunc):
    """Fuse depth views into a truncated signed distance volume, in place (nerf_tsdf_integrate, one launch per 8 views):
    tsdf and
    weight (nx,ny,nz) float32 over the lattice of mesh_extract; depth (n,H,W) or (H,W) float32, ranges along unit ray
    directions (render_image's depth over acc, Mesh.render's depth: +inf, NaN, 0 and negative values are "no surface");
    c2w (n,3,4), (n,4,4), (3,4) or (4,4) float32, finite, the cameras of rays_gen.  Per voxel and view, in the order of
    the views: project to the pixel that holds the voxel, s = depth - range of the voxel, skip if s < -trunc, else
    tsdf = (tsdf w + min(1, s / trunc)) / (w + 1), w += 1 (DESIGN §3.11.8 states every step).  n views in one call
    are bit for bit n calls of one view.  Returns nothing.  One host read: the finiteness of c2w."""
    shape, lo, hi, depth, c2w, (n, H, W), cam = _tsdf_views_args(tsdf, weight, lo, hi, depth, c2w, fx, fy, cx, cy,
                                                                 trunc)
    if n == 0:
        return
    rows = _tsdf_rows(c2w)
    lo_c, hi_c = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi)
    check(lib().nerf_tsdf_integrate(ptr(tsdf), ptr(weight), *shape, lo_c, hi_c, ptr(depth), ptr(rows), n, H, W, *cam,
                                    stream()), "nerf_tsdf_integrate")


def _color_volume_arg(color, shape, device):
    need(color, "color")
    if tuple(color.shape) != tuple(shape) + (4,):
        raise ValueError(f"color must be {tuple(shape) + (4,)}, got {tuple(color.shape)}")
    if color.device != device:
        raise ValueError("color must be on the volume's device")
    if color.data_ptr() % 16:
        raise ValueError("color must be 16-byte aligned")


def tsdf_integrate_color(tsdf, weight, color, lo, hi, depth, rgb, c2w, fx, fy, cx, cy, trunc):
    """tsdf_integrate with colour, in place (nerf_tsdf_integrate_color): color (nx,ny,nz,4) float32
    holds r, g, b and a colour weight cw per voxel (a fresh volume: zeros), rgb (n,H,W,3) or (H,W,3) float32 the colour of
    the pixel each depth came from (render_image's rgb, Mesh.render's "color").  tsdf and weight come out bit for bit
    as from tsdf_integrate.  Where a view updated a voxel without clamping (s / trunc < 1: within trunc of the surface
    the pixel saw) and the pixel's three channels are finite: c = (c cw + pixel) / (cw + 1) per channel, cw += 1.
    The other arguments, the checks and the host read are tsdf_integrate's.  Returns nothing."""
    shape, lo, hi, depth, c2w, (n, H, W), cam = _tsdf_views_args(tsdf, weight, lo, hi, depth, c2w, fx, fy, cx, cy,
                                                                 trunc)
    _color_volume_arg(color, shape, tsdf.device)
    need(rgb, "rgb")
    if rgb.device != tsdf.device:
        raise ValueError("rgb must be on the volume's device")
    if rgb.dim() == 3:
        rgb = rgb[None]
    if tuple(rgb.shape) != (n, H, W, 3):
        raise ValueError(f"rgb must be {(n, H, W, 3)} to match depth, got {tuple(rgb.shape)}")
    if n == 0:
        return
    rows = _tsdf_rows(c2w)
    lo_c, hi_c = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi)
    check(lib().nerf_tsdf_integrate_color(ptr(tsdf), ptr(weight), ptr(color), *shape, lo_c, hi_c, ptr(depth), ptr(rgb),
                                          ptr(rows), n, H, W, *cam, stream()), "nerf_tsdf_integrate_color")


def tsdf_sample_color(color, lo, hi, points):
    """The fused colour at points (N,3) float32 (nerf_tsdf_sample_color) -> rgb (N,3), cover (N,):
    over the 8 corners of the cell that holds the point (points outside the box are clamped onto it), each weighted by
    its trilinear weight times its colour weight cw; cover is the sum of those weights, rgb the weighted mean where
    cover > 0 and 0 elsewhere (no corner was ever coloured, or a coordinate is NaN)."""
    need(color, "color")
    if color.dim() != 4 or color.shape[3] != 4:
        raise ValueError(f"color must be (nx,ny,nz,4), got {tuple(color.shape)}")
    shape = tuple(int(n) for n in color.shape[:3])
    if min(shape) < 2:
        raise ValueError(f"every lattice dimension must be >= 2, got {shape}")
    if shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError(f"lattice too large: {shape} reaches 2^31 points")
    lo, hi = _box3(lo, "lo"), _box3(hi, "hi")
    if not all(a < b for a, b in zip(lo, hi)):
        raise ValueError(f"lo must be below hi on every axis, got {lo} vs {hi}")
    need(points, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (N,3), got {tuple(points.shape)}")
    if points.device != color.device:
        raise ValueError("points must be on the volume's device")
    N = int(points.shape[0])
    rgb, cover = _empty((N, 3), color), _empty((N,), color)
    lo_c, hi_c = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi)
    check(lib().nerf_tsdf_sample_color(ptr(color), *shape, lo_c, hi_c, ptr(points) if N else None, N,
                                       ptr(rgb) if N else None, ptr(cover) if N else None, stream()),
          "nerf_tsdf_sample_color")
    return rgb, cover


def tsdf_face_observed(face_off, weight, min_weight):
    """keep (F,) uint8 for the faces of mesh_extract(..., face_offsets=True) over the lattice of ``weight``
    (nx,ny,nz) float32: 1 iff every one of the 8 corners of the face's cell has weight >= min_weight
    (nerf_tsdf_face_observed).  face_off (nx ny nz + 1,) int32.  One host read: F = face_off[-1]."""
    shape = _volume_arg(weight, "weight")
    need(face_off, "face_off", torch.int32)
    P = shape[0] * shape[1] * shape[2]
    if tuple(face_off.shape) != (P + 1,):
        raise ValueError(f"face_off must be ({P + 1},), got {tuple(face_off.shape)}")
    if face_off.device != weight.device:
        raise ValueError("face_off and weight must be on one device")
    min_weight = float(min_weight)
    if min_weight != min_weight:
        raise ValueError("min_weight must not be NaN")
    F = int(face_off[-1])
    if F < 0 or F > 12 * P:
        raise ValueError(f"face_off is no scan of face counts: its total is {F}")
    keep = torch.zeros(F, dtype=torch.uint8, device=weight.device)
    check(lib().nerf_tsdf_face_observed(ptr(face_off), ptr(weight), *shape, min_weight, F, ptr(keep) if F else None,
                                        stream()), "nerf_tsdf_face_observed")
    return keep


# ------------------------------------------------------------------ mesh clean-up


def _faces_arg(faces, n_vertices, labels=None, ranges_checked=False):
    """faces (F,3) int32, contiguous, on the device, 0 <= index < V, V and 3 F below 2^31 (and labels (V,) int32 in the
    same range): ValueError before any launch (the kernels do not check).  The range check is one host read."""
    need(faces, "faces", torch.int32)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be (F,3), got {tuple(faces.shape)}")
    V, F = int(n_vertices), int(faces.shape[0])
    if V < 0 or V >= 2 ** 31 or 3 * F >= 2 ** 31:
        raise ValueError(f"n_vertices and 3 * F must be in [0, 2^31), got V = {V}, F = {F}")
    if labels is not None:
        need(labels, "labels", torch.int32)
        if tuple(labels.shape) != (V,):
            raise ValueError(f"labels must be ({V},), got {tuple(labels.shape)}")
    if F and not ranges_checked:
        ranged =[faces] if labels is None else [faces, labels]
        lim = torch.stack([t.min() for t in ranged] + [t.max() for t in ranged]).tolist()
        if min(lim) < 0 or max(lim) >= V:
            raise ValueError(f"face indices (and labels) must be in [0, {V}), got {min(lim)} .. {max(lim)}")
    return V, F


def mesh_components(faces, n_vertices, return_steps=False):
    """Connected components of an indexed triangle list (nerf_mesh_components): faces (F,3) int32 with
    0 <= index < n_vertices, any list (arbitrary order, duplicated faces, repeated indices, unused vertices).  Returns
    labels (V,) int32, labels[v] = the smallest vertex index of v's component (an unused vertex is its own), and
    face_count (V,) int32, face_count[l] = faces of the component labelled l (0 where l is no label).  Bitwise
    reproducible: both are functions of the input alone.  Two host reads: the index range before the launches, the
    status word after them (RuntimeError if a thread exhausted a loop bound; never silently wrong labels).  With
    ``return_steps`` also the most find steps one face's unions took."""
    V, F = _faces_arg(faces, n_vertices)
    dev = faces.device
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    counts = torch.empty(V, dtype=torch.int32, device=dev)
    if V == 0:  # nothing to launch, nothing to read
        return (labels, counts, 0) if return_steps else (labels, counts)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    check(lib().nerf_mesh_components(ptr(faces) if F else None, F, V, ptr(labels), ptr(counts), ptr(status), stream()),
          "nerf_mesh_components")
    err, steps = status.tolist()
    if err:
        raise RuntimeError(f"nerf_mesh_components: a loop bound was exhausted (status {err}); the labels are invalid")
    return (labels, counts, steps) if return_steps else (labels, counts)


def mesh_compact(vertices, faces, keep_face, attrs=(), labels=None, ranges_checked=False):
    """The mesh of the faces with keep_face != 0 (nerf_mesh_mark_used -> two scans -> nerf_mesh_remap_faces,
    nerf_flag_compact, nerf_gather_rows): vertices (V,3) float32, faces (F,3) int32, keep_face (F,) uint8 or bool,
    attrs a sequence of (V,C) float32.  Kept faces stay in their order; the vertices a kept face uses stay in their
    order and are renumbered densely; every attribute is gathered like the vertices.  Returns (vertices, faces,
    [attrs...]).  With ``labels`` (the (V,) int32 of mesh_components) keep_face is (V,), a flag per component label,
    and face f is kept iff keep_face[labels[faces[f, 0]]].  Host reads: the index range (skipped with
    ``ranges_checked``: these very faces and labels have just passed mesh_components), and the two totals that size
    the outputs in one read."""
    from .occupancy import exclusive_scan
    need(vertices, "vertices")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be (V,3), got {tuple(vertices.shape)}")
    V, F = _faces_arg(faces, vertices.shape[0], labels, ranges_checked)
    if not isinstance(keep_face, torch.Tensor) or keep_face.dtype not in (torch.uint8, torch.bool):
        raise ValueError("keep_face must be a uint8 or bool tensor")
    keep_face = need(keep_face.view(torch.uint8) if keep_face.dtype == torch.bool else keep_face, "keep_face",
                     torch.uint8)
    n_keep = F if labels is None else V
    if tuple(keep_face.shape) != (n_keep,):
        raise ValueError(f"keep_face must be ({n_keep},), got {tuple(keep_face.shape)}")
    attrs = list(attrs)
    for i, a in enumerate(attrs):
        need(a, f"attrs[{i}]")
        if a.dim() != 2 or a.shape[0] != V or a.shape[1] < 1:
            raise ValueError(f"attrs[{i}] must be ({V},C), got {tuple(a.shape)}")
    dev = faces.device
    if F == 0:
        return (vertices.new_empty((0, 3)), faces.new_empty((0, 3)), [a.new_empty((0, a.shape[1])) for a in attrs])
    keep32 = torch.empty(F, dtype=torch.int32, device=dev)
    used = torch.zeros(V, dtype=torch.int32, device=dev)
    check(lib().nerf_mesh_mark_used(ptr(faces), ptr(keep_face), ptr(labels), F, V, ptr(keep32), ptr(used), stream()),
          "nerf_mesh_mark_used")
    vpos, fpos = exclusive_scan(used), exclusive_scan(keep32)
    Vo, Fo = (int(v) for v in torch.stack([vpos[-1], fpos[-1]]).tolist())
    out_f = torch.empty((Fo, 3), dtype=torch.int32, device=dev)
    check(lib().nerf_mesh_remap_faces(ptr(faces), ptr(keep32), ptr(fpos), ptr(vpos), F, Fo,
                                      ptr(out_f) if Fo else None, stream()), "nerf_mesh_remap_faces")
    vidx = torch.empty(Vo, dtype=torch.int32, device=dev)
    if Vo:
        check(lib().nerf_flag_compact(ptr(used), ptr(vpos), V, ptr(vidx), stream()), "nerf_flag_compact")

    def rows(src):
        dst = torch.empty((Vo, src.shape[1]), dtype=F32, device=dev)
        check(lib().nerf_gather_rows(ptr(src), src.stride(0), ptr(vidx) if Vo else None, Vo, src.shape[1],
                                     ptr(dst) if Vo else None, src.shape[1], stream()), "nerf_gather_rows")
        return dst

    return rows(vertices), out_f, [rows(a) for a in attrs]


# ------------------------------------------------------------------ mesh simplification


def _table_log2(items, table_log2):
    """The hash set's size: by default the smallest 2^k >= 2 * items, at least 2^6; a given k needs 2^k > items (one
    slot always stays empty, which ends every probe chain)."""
    if table_log2 is None:
        return max(6, (2 * items - 1).bit_length())
    k = int(table_log2)
    if not 0 <= k <= 31 or (1 << k) <= items:
        raise ValueError(f"table_log2 must be in [0, 31] with 2^table_log2 > {items}, got {table_log2}")
    return k


def _grid_arg(lo, cell, dims):
    """(lo, cell, inv, dims) as the C-ABI takes them: cell > 0 rounded to fp32, inv = fp32(1) / fp32(cell)."""
    import numpy as np
    lo = _box3(lo, "lo")
    with np.errstate(all="ignore"):
        cell32 = np.float32(cell)
        inv = np.float32(1.0) / cell32
    if not (np.isfinite(cell32) and cell32 > 0 and np.isfinite(inv) and inv > 0):
        raise ValueError(f"cell must be a finite positive float32 with a finite reciprocal, got {cell!r}")
    dims = [int(d) for d in dims]
    if len(dims) != 3 or min(dims) < 1 or max(dims) > 2 ** 20:
        raise ValueError(f"dims must be 3 integers in [1, 2^20], got {dims}")
    return (ctypes.c_float * 3)(*lo), float(cell32), float(inv), (ctypes.c_int32 * 3)(*dims)


def _vertices_arg(vertices):
    need(vertices, "vertices")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be (V,3), got {tuple(vertices.shape)}")
    V = int(vertices.shape[0])
    if V >= 2 ** 31:
        raise ValueError(f"V must be below 2^31, got {V}")
    return V


def _status(status, what):
    err, probes = status.tolist()
    if err:
        raise RuntimeError(f"{what}: a probe bound was exhausted (status {err}); the result is invalid")
    return probes


def mesh_cluster_labels(vertices, lo, cell, dims, table_log2=None, return_probes=False):
    """Vertex clustering, step 1 (nerf_mesh_cluster_labels): vertices (V,3) float32, finite; the grid of cells
    lo + (ix,iy,iz) cell with dims = (nx,ny,nz) cells, each in [1, 2^20]; a vertex outside lands in a border cell.
    Returns labels (V,) int32, labels[v] = the smallest vertex index in v's cell: a function of the input alone, so
    bitwise reproducible.  table_log2: the hash set has 2^table_log2 slots (default: the smallest with
    2^k >= 2 V, at least 6; a given value needs 2^k > V, else ValueError).  One host read, the status word
    (RuntimeError if a thread exhausted its probe bound; never silently wrong labels).  With ``return_probes`` also
    the longest probe chain."""
    V = _vertices_arg(vertices)
    lo_c, cell32, inv, dims_c = _grid_arg(lo, cell, dims)
    k = _table_log2(V, table_log2)
    dev = vertices.device
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    if V == 0:
        return (labels, 0) if return_probes else labels
    L = lib()
    nb = int(L.nerf_mesh_cluster_labels_workspace_bytes(V, k))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    check(L.nerf_mesh_cluster_labels(ptr(vertices), V, lo_c, cell32, inv, dims_c, k, ptr(ws), nb, ptr(labels),
                                     ptr(status), stream()), "nerf_mesh_cluster_labels")
    probes = _status(status, "nerf_mesh_cluster_labels")
    return (labels, probes) if return_probes else labels


def mesh_cluster_reduce(vertices, labels, lo, cell, dims, normals=None, colors=None, ranges_checked=False):
    """Vertex clustering, step 2 (nerf_mesh_cluster_reduce): one vertex per cluster, at the row of its representative
    (labels[v] == v), every other row zeros.  Position: the cell's corner plus the mean of the members' cell-relative
    positions in 24-bit fixed point; normals: the normalised sum of the members' (clamped to [-1,1], rounded to
    2^-20; zeros when they cancel); colours: the mean of the members' (clamped to [0,1], rounded to 2^-24).  Integer
    sums, so the result does not depend on the order of the atomics.  Returns (vertices, normals or None, colors or
    None), each (V,3) float32.  One host read, the range of ``labels`` (skipped with ``ranges_checked``: these labels
    have just come from mesh_cluster_labels)."""
    V = _vertices_arg(vertices)
    lo_c, cell32, inv, dims_c = _grid_arg(lo, cell, dims)
    need(labels, "labels", torch.int32)
    if tuple(labels.shape) != (V,):
        raise ValueError(f"labels must be ({V},), got {tuple(labels.shape)}")
    for a, name in ((normals, "normals"), (colors, "colors")):
        if a is not None:
            need(a, name)
            if tuple(a.shape) != (V, 3):
                raise ValueError(f"{name} must be ({V},3), got {tuple(a.shape)}")
    if V and not ranges_checked:
        a, b = torch.stack([labels.min(), labels.max()]).tolist()
        if a < 0 or b >= V:
            raise ValueError(f"labels must be in [0, {V}), got {a} .. {b}")
    out = [torch.empty_like(vertices)] + [None if a is None else torch.empty_like(a) for a in (normals, colors)]
    if V == 0:
        return tuple(out)
    L = lib()
    nb = int(L.nerf_mesh_cluster_reduce_workspace_bytes(V, normals is not None, colors is not None))
    ws = torch.empty(nb, dtype=torch.uint8, device=vertices.device)
    check(L.nerf_mesh_cluster_reduce(ptr(vertices), ptr(labels), ptr(normals), ptr(colors), V, lo_c, cell32, inv,
                                     dims_c, ptr(ws), nb, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream()),
          "nerf_mesh_cluster_reduce")
    return tuple(out)


def mesh_cluster_faces(faces, labels, table_log2=None, return_probes=False, ranges_checked=False):
    """Vertex clustering, step 3 (nerf_mesh_cluster_faces): faces (F,3) int32 and labels (V,) int32, both in [0, V).
    Returns faces' (F,3) int32 = labels[faces] (still indices of the V input rows) and keep (F,) uint8: 1 iff the three
    new indices differ and the face is the first (smallest face index) of its canonical form, the rotation with the
    smallest index first; a face and its mirror image are different forms and are both kept.  mesh_compact(vertices of
    mesh_cluster_reduce, faces', keep, attrs) then gives the simplified mesh.  table_log2 as in mesh_cluster_labels,
    with F for V.  Two host reads: the index ranges (skipped with ``ranges_checked``) and the status word
    (RuntimeError on an exhausted probe bound)."""
    V, F = _faces_arg(faces, labels.shape[0] if isinstance(labels, torch.Tensor) and labels.dim() == 1 else -1, labels,
                      ranges_checked)
    k = _table_log2(F, table_log2)
    dev = faces.device
    out = torch.empty_like(faces)
    keep = torch.empty(F, dtype=torch.uint8, device=dev)
    if F == 0:
        return (out, keep, 0) if return_probes else (out, keep)
    L = lib()
    nb = int(L.nerf_mesh_cluster_faces_workspace_bytes(F, k))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    check(L.nerf_mesh_cluster_faces(ptr(faces), ptr(labels), F, V, k, ptr(ws), nb, ptr(out), ptr(keep), ptr(status),
                                    stream()), "nerf_mesh_cluster_faces")
    probes = _status(status, "nerf_mesh_cluster_faces")
    return (out, keep, probes) if return_probes else (out, keep)


def _tol_arg(tol):
    try:
        t = float(tol)
    except (TypeError, ValueError):
        raise ValueError(f"tol must be a float, got {tol!r}") from None
    if not 0.0 < t < 1.0:  # false for a NaN
        raise ValueError(f"tol must be a finite float in (0, 1), got {tol!r}")
    return t


def mesh_cluster_quadric(vertices, faces, labels, row_off, col, mean, lo, cell, dims, tol=1e-3, ranges_checked=False):
    """Vertex clustering, quadric-error placement (nerf_mesh_cluster_quadric): the cluster's vertex at the point that
    minimises the summed plane quadrics of the faces that touch the cluster, in place of the members' mean.  vertices
    (V,3) float32, finite, and faces (F,3) int32 of the ORIGINAL mesh; labels (V,) int32 of mesh_cluster_labels;
    (row_off, col) = mesh_vertex_faces(faces', V) on the faces' of mesh_cluster_faces, so that the row of a
    representative lists the original faces with a corner in its cluster; mean (V,3) float32, the positions of
    mesh_cluster_reduce; the grid as there.  In the frame of the representative's cell (the box [-0.5, 0.5]^3) the
    row's faces are summed in the row's order, weighted by twice their area; 8 cyclic Jacobi sweeps give the
    eigenpairs, and from the mean the solve moves only along eigenvectors whose eigenvalue exceeds ``tol`` times the
    largest (Lindstrom's 1e-3): a flat cluster's vertex is the mean projected onto its plane, an edge cluster's onto
    the edge, a corner cluster's is the corner.  A cluster without a face of positive area, and one whose solution is
    not finite or leaves the cell, keeps the mean bit for bit.  Returns position (V,3) float32 and placed (V,) uint8
    (1 where the solution was accepted), both zeros at the rows that are no representative.  All in double, every
    operation rounded on its own, so bitwise reproducible.  ValueError before any launch on a wrong dtype, shape or
    device and on a ``tol`` outside (0, 1).  Host reads: the index ranges of faces, labels and of the adjacency
    (skipped with ``ranges_checked``)."""
    V = _vertices_arg(vertices)
    need(labels, "labels", torch.int32)
    _, F = _smooth_faces_arg(faces, V, ranges_checked, labels=labels)
    lo_c, cell32, inv, dims_c = _grid_arg(lo, cell, dims)
    _csr_arg(row_off, col, V, F, ranges_checked)
    need(mean, "mean")
    if tuple(mean.shape) != (V, 3):
        raise ValueError(f"mean must be ({V},3), got {tuple(mean.shape)}")
    t = _tol_arg(tol)
    position = torch.empty_like(vertices)
    placed = torch.empty(V, dtype=torch.uint8, device=vertices.device)
    if V:
        check(lib().nerf_mesh_cluster_quadric(ptr(vertices), ptr(faces) if F else None, ptr(labels), ptr(row_off),
                                              ptr(col) if col.numel() else None, ptr(mean), V, F, lo_c, cell32, inv,
                                              dims_c, t, ptr(position), ptr(placed), stream()),
              "nerf_mesh_cluster_quadric")
    return position, placed


# ------------------------------------------------------------------ mesh smoothing


def _smooth_faces_arg(faces, n_vertices, ranges_checked=False, labels=None):
    """_faces_arg with the tighter size limit of the adjacency build: 6 F below 2^31 (the int32 scan of the flags)."""
    if isinstance(faces, torch.Tensor) and faces.dim() == 2 and 6 * int(faces.shape[0]) >= 2 ** 31:
        raise ValueError(f"6 * F must be below 2^31, got F = {int(faces.shape[0])}")
    return _faces_arg(faces, n_vertices, labels, ranges_checked)


def _csr(faces, V, F, mode, boundary=False):
    """(row_off (V+1), col (E)[, boundary (V) uint8]) of the keys of ``mode``: nerf_mesh_pair_keys -> torch.sort ->
    nerf_mesh_csr_flags -> the scan -> one host read of E -> nerf_mesh_csr_build."""
    from .occupancy import exclusive_scan
    dev = faces.device
    n = (6 if mode == 0 else 3) * F
    bnd = torch.zeros(V, dtype=torch.uint8, device=dev) if boundary else None
    if n == 0:
        out = (torch.zeros(V + 1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
        return out + (bnd,) if boundary else out
    L = lib()
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    check(L.nerf_mesh_pair_keys(ptr(faces), F, mode, ptr(keys), stream()), "nerf_mesh_pair_keys")
    keys = torch.sort(keys).values
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    check(L.nerf_mesh_csr_flags(ptr(keys), n, ptr(flags), ptr(bnd) if boundary and V else None, stream()),
          "nerf_mesh_csr_flags")
    pos = exclusive_scan(flags)
    E = int(pos[-1])
    row_off = torch.empty(V + 1, dtype=torch.int32, device=dev)
    col = torch.empty(E, dtype=torch.int32, device=dev)
    check(L.nerf_mesh_csr_build(ptr(keys), n, ptr(flags), ptr(pos), V, E, ptr(row_off), ptr(col) if E else None,
                                stream()), "nerf_mesh_csr_build")
    return (row_off, col, bnd) if boundary else (row_off, col)


def mesh_adjacency(faces, n_vertices, boundary=False, ranges_checked=False):
    """The vertex adjacency of an indexed triangle list as a CSR pair: faces (F,3) int32 with 0 <= index < n_vertices,
    any list (duplicated faces, repeated indices, unused vertices), n_vertices and 6 F below 2^31.  Returns row_off
    (V+1,) int32 and col (E,) int32: row v = col[row_off[v]:row_off[v+1]] lists, ascending and once each, the vertices
    u != v that share a face with v (symmetric; an unused vertex has an empty row).  With ``boundary`` also (V,) uint8,
    1 at the vertices of an edge that exactly one face uses (each face emits (a,b) and (b,a) for its three edges; a
    vertex is marked iff one of its pairs occurs exactly once).  Sorted int64 keys (torch.sort), run flags, the
    exclusive scan and a row build; no atomics, bitwise reproducible.  Two host reads: the index range (skipped with
    ``ranges_checked``) and E."""
    V, F = _smooth_faces_arg(faces, n_vertices, ranges_checked)
    return _csr(faces, V, F, 0, boundary)


def mesh_vertex_faces(faces, n_vertices, ranges_checked=False):
    """The vertex-to-face adjacency in the same CSR form: row v lists, ascending and once each, the faces that contain
    v (a face such as (a,a,b) is listed once for a).  Arguments and host reads as mesh_adjacency."""
    V, F = _smooth_faces_arg(faces, n_vertices, ranges_checked)
    return _csr(faces, V, F, 1)


def _csr_arg(row_off, col, V, n_items, ranges_checked):
    """row_off (V+1,) and col (E,) int32 on the device, and unless ``ranges_checked`` one host read: row_off starts at
    0, never decreases and ends at E, col in [0, n_items)."""
    need(row_off, "row_off", torch.int32)
    need(col, "col", torch.int32)
    if tuple(row_off.shape) != (V + 1,) or col.dim() != 1:
        raise ValueError(f"row_off must be ({V + 1},) and col (E,), got {tuple(row_off.shape)}, {tuple(col.shape)}")
    E = int(col.shape[0])
    if not ranges_checked:
        steps = (row_off[1:] - row_off[:-1]).min() if V else row_off[0] * 0
        lim = [row_off[0], row_off[-1], steps] + ([col.min(), col.max()] if E else [])
        lim = torch.stack([t.to(torch.int64) for t in lim]).tolist()
        if lim[0] != 0 or lim[1] != E or lim[2] < 0:
            raise ValueError(f"row_off must rise from 0 to len(col) = {E}")
        if E and (lim[3] < 0 or lim[4] >= n_items):
            raise ValueError(f"col must be in [0, {n_items}), got {lim[3]} .. {lim[4]}")
    return E


def mesh_smooth_pass(vertices, row_off, col, s, fixed=None, out=None, ranges_checked=False):
    """One Jacobi smoothing step (nerf_mesh_smooth_pass): vertices (V,3) float32, finite; (row_off, col) of
    mesh_adjacency; s a float32 factor; fixed None or (V,) uint8 / bool.  out[v] = float(q + double(s) (m - q)) per
    axis with q = double(vertices[v]) and m the mean, in double and in the row's order, of the row's vertices; a vertex
    with an empty row, a fixed one and s == 0 keep their bits.  ``out``: a (V,3) float32 buffer that does not share
    memory with ``vertices`` (default: a new one).  One host read, the ranges of the adjacency (skipped with
    ``ranges_checked``: it has just come from mesh_adjacency for this vertex count)."""
    import numpy as np
    V = _vertices_arg(vertices)
    _csr_arg(row_off, col, V, V, ranges_checked)
    with np.errstate(all="ignore"):
        s32 = np.float32(s)
    if not np.isfinite(s32):
        raise ValueError(f"s must be a finite float32, got {s!r}")
    if fixed is not None:
        if not isinstance(fixed, torch.Tensor) or fixed.dtype not in (torch.uint8, torch.bool):
            raise ValueError("fixed must be a uint8 or bool tensor")
        fixed = need(fixed.view(torch.uint8) if fixed.dtype == torch.bool else fixed, "fixed", torch.uint8)
        if tuple(fixed.shape) != (V,):
            raise ValueError(f"fixed must be ({V},), got {tuple(fixed.shape)}")
    if out is None:
        out = torch.empty_like(vertices)
    else:
        need(out, "out")
        if tuple(out.shape) != (V, 3):
            raise ValueError(f"out must be ({V},3), got {tuple(out.shape)}")
        if V and abs(out.data_ptr() - vertices.data_ptr()) < 12 * V:
            raise ValueError("out must not share memory with vertices (a Jacobi step reads every old position)")
    if V:
        check(lib().nerf_mesh_smooth_pass(ptr(vertices), ptr(row_off), ptr(col) if col.numel() else None, ptr(fixed),
                                          V, float(s32), ptr(out), stream()), "nerf_mesh_smooth_pass")
    return out


def mesh_vertex_normals(vertices, faces, row_off, col, ranges_checked=False):
    """Unit vertex normals from the faces (nerf_mesh_vertex_normals): vertices (V,3) float32, finite; faces (F,3)
    int32; (row_off, col) of mesh_vertex_faces.  normal[v] = g / max(|g|, 1e-12), g = the sum in double, in the row's
    order, of (p[i1] - p[i0]) x (p[i2] - p[i0]) over the faces of v: area-weighted, by the faces' winding (the
    extractor's winding points to lower density); zeros at an unused vertex and where the faces cancel.  Host reads:
    the index ranges of the faces and of the adjacency (skipped with ``ranges_checked``)."""
    V = _vertices_arg(vertices)
    _, F = _smooth_faces_arg(faces, V, ranges_checked)
    _csr_arg(row_off, col, V, F, ranges_checked)
    out = torch.empty_like(vertices)
    if V:
        check(lib().nerf_mesh_vertex_normals(ptr(vertices), ptr(faces) if F else None, ptr(row_off),
                                             ptr(col) if col.numel() else None, V, ptr(out), stream()),
              "nerf_mesh_vertex_normals")
    return out


# ------------------------------------------------------------------ mesh metrics


def _finite_vertices(vertices):
    V = _vertices_arg(vertices)
    if V and not bool(torch.isfinite(vertices).all()):
        raise ValueError("vertices must be finite")
    return V


def mesh_face_areas(vertices, faces, ranges_checked=False):
    """The area of every face (nerf_mesh_face_areas): vertices (V,3) float32, finite; faces (F,3) int32.  Returns (F,)
    float64: 0.5 |(p1 - p0) x (p2 - p0)| with every operation in double and rounded on its own; a face with a repeated
    index has area exactly 0.  Bitwise reproducible.  Host reads: the finiteness of the vertices and the index range
    (both skipped with ``ranges_checked``)."""
    V = _vertices_arg(vertices) if ranges_checked else _finite_vertices(vertices)
    _, F = _faces_arg(faces, V, ranges_checked=ranges_checked)
    area = torch.empty(F, dtype=torch.float64, device=faces.device)
    if F:
        check(lib().nerf_mesh_face_areas(ptr(vertices), ptr(faces), F, ptr(area), stream()), "nerf_mesh_face_areas")
    return area


def mesh_area_cdf(area):
    """The integer CDF of the sampler, exact in any order of evaluation: area (F,) float64 >= 0 ->
    (cdf (F,) int64, total int).  e = 32 - frexp(max area).exponent, weight = rint(area 2^e) (the largest weight lies in
    [2^31, 2^32], a face more than 2^32 times smaller than the largest gets weight 0), cdf = the inclusive sum,
    total = cdf[-1] < 2^63 for F < 2^31.  Two host reads: the largest area (the power of two is then an exact host
    float, whatever the device's pow does) and total.  F == 0 and an all-zero area give total 0."""
    import math
    if area.numel() == 0:
        return torch.empty(0, dtype=torch.int64, device=area.device), 0
    amax = float(area.max())
    if not amax > 0.0:
        return torch.zeros(area.shape[0], dtype=torch.int64, device=area.device), 0
    scale = math.ldexp(1.0, 32 - math.frexp(amax)[1])
    cdf = torch.cumsum(torch.round(area * scale).to(torch.int64), 0)
    return cdf, int(cdf[-1])


def _count_arg(n, name="n"):
    if isinstance(n, bool) or not isinstance(n, int) or n < 0 or n >= 2 ** 31:
        raise ValueError(f"{name} must be an int in [0, 2^31), got {n!r}")
    return n


def _seed_arg(seed):
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be an int in [0, 2^64), got {seed!r}")
    return seed


def mesh_sample_surface(vertices, faces, n, seed=0, normals=None, vertex_normals=None):
    """n points distributed uniformly by area over the faces (nerf_mesh_face_areas -> mesh_area_cdf ->
    nerf_mesh_sample_surface): vertices (V,3) float32, finite; faces (F,3) int32; n an int in [0, 2^31); seed an int in
    [0, 2^64).  Returns (points (n,3) float32, face_idx (n,) int32) and, with ``normals`` = "face" or "vertex", unit
    normals (n,3) float32: the face's own by its winding, or the barycentric mix of ``vertex_normals`` (V,3),
    normalised.  Sample i is a function of (seed, i) and the mesh alone: bitwise reproducible, and a prefix of a longer
    run.  A face with a repeated index, of zero area, or more than 2^32 times smaller than the largest face is never
    chosen.  ValueError before the sampling launch on a bad argument and when no face has area (n > 0).  Host reads:
    finiteness, the index range, the CDF's total."""
    V = _finite_vertices(vertices)
    _, F = _faces_arg(faces, V)
    n, seed = _count_arg(n), _seed_arg(seed)
    if normals not in (None, "face", "vertex"):
        raise ValueError(f"normals must be None, 'face' or 'vertex', got {normals!r}")
    if (normals == "vertex") != (vertex_normals is not None):
        raise ValueError("vertex_normals goes with normals='vertex', and only with it")
    if vertex_normals is not None:
        need(vertex_normals, "vertex_normals")
        if tuple(vertex_normals.shape) != (V, 3):
            raise ValueError(f"vertex_normals must be ({V},3), got {tuple(vertex_normals.shape)}")
        if V and not bool(torch.isfinite(vertex_normals).all()):
            raise ValueError("vertex_normals must be finite")
    dev = vertices.device
    points = torch.empty((n, 3), dtype=F32, device=dev)
    face_idx = torch.empty(n, dtype=torch.int32, device=dev)
    nrm = torch.empty((n, 3), dtype=F32, device=dev) if normals else None
    if n:
        cdf, total = mesh_area_cdf(mesh_face_areas(vertices, faces, ranges_checked=True))
        if total <= 0:
            raise ValueError("no face of the mesh has area: nothing to sample")
        check(lib().nerf_mesh_sample_surface(ptr(vertices), ptr(faces), F, ptr(cdf), total, ptr(vertex_normals), n,
                                             seed, ptr(points), ptr(face_idx), ptr(nrm), stream()),
              "nerf_mesh_sample_surface")
    return (points, face_idx, nrm) if normals else (points, face_idx)


MAX_GRID_DIM = 1024


def _points_arg(points, name):
    need(points, name)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{name} must be (N,3), got {tuple(points.shape)}")
    if points.shape[0] >= 2 ** 31:
        raise ValueError(f"{name} must have fewer than 2^31 rows")
    return int(points.shape[0])


def _gather3(src, idx):
    n = int(idx.shape[0])
    dst = torch.empty((n, 3), dtype=F32, device=src.device)
    if n:
        check(lib().nerf_gather_rows(ptr(src), 3, ptr(idx), n, 3, ptr(dst), 3, stream()), "nerf_gather_rows")
    return dst


def _sorted_cell_keys(points, m, lo_c, inv, dims_c):
    """(sorted keys (m,) int64, the original index of every sorted position (m,) int32)"""
    keys = torch.empty(m, dtype=torch.int64, device=points.device)
    check(lib().nerf_points_cell_keys(ptr(points), m, lo_c, inv, dims_c, ptr(keys), stream()), "nerf_points_cell_keys")
    keys = torch.sort(keys).values
    return keys, (keys & 0xffffffff).to(torch.int32)


def _run_sorted(query, n, grid_c, outs, run):
    """run(q, *outs) with the queries in the order of their own cell keys (one key launch, a sort, a gather), every
    output scattered back to the caller's order; ``outs`` may hold None for an output that is not wanted."""
    lo_c, _, inv, dims_c = grid_c
    _, order = _sorted_cell_keys(query, n, lo_c, inv, dims_c)
    sorted_outs = [None if o is None else torch.empty_like(o) for o in outs]
    run(_gather3(query, order), *sorted_outs)
    order = order.to(torch.int64)
    for o, so in zip(outs, sorted_outs):
        if o is not None:
            o[order] = so


def _cell_size_arg(cell_size):
    """(cell, inv) as fp32 numpy values: ValueError unless cell_size is a finite positive float32 with a finite
    reciprocal."""
    import numpy as np
    with np.errstate(all="ignore"):
        try:
            cell = np.float32(cell_size)
        except (TypeError, ValueError):
            raise ValueError(f"cell_size must be a float, got {cell_size!r}") from None
        inv = np.float32(1.0) / cell
    if not (np.isfinite(cell) and cell > 0 and np.isfinite(inv) and inv > 0):
        raise ValueError(f"cell_size must be a finite positive float32 with a finite reciprocal, got {cell_size!r}")
    return cell, inv


def _finite_box(points, what):
    """The per-axis minimum and maximum of points (n,3), n > 0, as 6 fp32 numpy values (one host read); ValueError
    unless they are finite."""
    import numpy as np
    mm = [torch.aminmax(points[:, c]) for c in range(3)]
    box = np.asarray(torch.stack([x.min for x in mm] + [x.max for x in mm]).tolist(), np.float32)
    if not np.isfinite(box).all():
        raise ValueError(f"{what} must be finite")
    return box


def _grid_from_box(box, count, cell_size, what, per_axis=None):
    """The grid (lo, cell, inv, dims) of ``count`` items in ``box`` (of _finite_box; None for no items: one cell at the
    origin): lo 3 floats, cell and inv fp32 values as floats, dims 3 ints.  ``cell_size`` None: the default cell,
    longest extent / clamp(ceil(sqrt(count) / 2), 1, 1024), 1 for an all-zero extent; otherwise the caller has passed
    it through _cell_size_arg already.  ``per_axis`` (with cell_size None): that many cells along the longest extent
    instead of the square-root rule, an int in [1, 1024]."""
    import math

    import numpy as np
    cell, inv = (np.float32(1.0), np.float32(1.0)) if cell_size is None else _cell_size_arg(cell_size)
    if box is None:
        return [0.0, 0.0, 0.0], float(cell), float(inv), [1, 1, 1]
    lo = box[:3]
    with np.errstate(all="ignore"):
        ext = box[3:] - lo
        if not np.isfinite(ext).all():
            raise ValueError(f"the extent of the {what} overflows float32")
        if cell_size is None:
            k = min(max(math.ceil(math.sqrt(count) / 2.0), 1), MAX_GRID_DIM) if per_axis is None else per_axis
            cell = ext.max() / np.float32(k) if ext.max() > 0 else np.float32(1.0)
            inv = np.float32(1.0) / cell
            if not (np.isfinite(cell) and cell > 0 and np.isfinite(inv) and inv > 0):
                cell, inv = np.float32(1.0), np.float32(1.0)  # an extent too small to divide: one cell holds it all
        cells = np.floor(ext * inv)  # fp32, like the kernel's cell index of the largest coordinate
    if cell_size is None:
        # only rounding can exceed it; the kernel clamps into the last cell (with per_axis: the maximum itself too)
        cells = np.minimum(cells, (MAX_GRID_DIM if per_axis is None else per_axis) - 1)
    elif not np.isfinite(cells).all() or cells.max() + 1 > MAX_GRID_DIM:
        raise ValueError(f"cell_size {cell_size!r} needs more than {MAX_GRID_DIM} cells along an axis")
    return lo.tolist(), float(cell), float(inv), [int(c) + 1 for c in cells]


def _grid_c(grid):
    """The ctypes arguments (lo, cell, inv, dims) of a grid dict."""
    return ((ctypes.c_float * 3)(*grid["lo"]), float(grid["cell"]), float(grid["inv"]),
            (ctypes.c_int32 * 3)(*grid["dims"]))


def points_grid(points, cell_size=None):
    """The search grid of a reference point set (nerf_points_cell_keys -> torch.sort -> nerf_gather_rows): points
    (m,3) float32, finite.  Returns the dict {keys (m,) int64 sorted, points (m,3) float32 in key order, lo (3 floats),
    cell, inv (fp32 values as floats), dims (3 ints), m}.  lo is the minimum of the points.  The default cell is
    longest extent / clamp(ceil(sqrt(m) / 2), 1, 1024), a handful of surface samples per occupied cell; an all-zero
    extent gets cell = 1.  dims = floor((max - lo) * inv) + 1 per axis in fp32 (1 for an axis of zero extent).
    ``cell_size``: a finite positive float; ValueError if it needs more than 1024 cells on an axis (the cap keeps the
    fp32 cell index within 2^-12 of a cell, which the search's stopping rule rests on).  Memory: 8 + 12 bytes per
    point beyond the input, no cell table.  One host read: the box (it carries the finiteness check)."""
    m = _points_arg(points, "points")
    if cell_size is not None:
        _cell_size_arg(cell_size)
    lo, cell, inv, dims = _grid_from_box(_finite_box(points, "points") if m else None, m, cell_size, "points")
    grid = {"lo": lo, "cell": cell, "inv": inv, "dims": dims, "m": m}
    if m:
        lo_c, _, _, dims_c = _grid_c(grid)
        grid["keys"], order = _sorted_cell_keys(points, m, lo_c, inv, dims_c)
        grid["points"] = _gather3(points, order)
    else:
        grid["keys"], grid["points"] = torch.empty(0, dtype=torch.int64, device=points.device), points.new_empty((0, 3))
    return grid


def _finite_points(points, name):
    n = _points_arg(points, name)
    if n and not bool(torch.isfinite(points).all()):
        raise ValueError(f"{name} must be finite")
    return n


def points_nearest(query, grid, sort_queries=True, finite_checked=False):
    """The nearest reference point of every query (nerf_points_nearest): query (n,3) float32, finite; ``grid`` of
    points_grid.  Returns (d2 (n,) float32, idx (n,) int32): d2 = (dx dx + dy dy) + dz dz in fp32 to the nearest point,
    idx its row in the reference set, the smallest row on equal d2; exactly what a brute-force search gives, bit for
    bit.  An empty reference set gives d2 = +inf, idx = -1.  ``sort_queries``: present the queries in the order of
    their own cell keys (one more key launch, sort and gather, the results scattered back) so that the lanes of a
    wave walk the same columns; the result is the same either way.  One host read: the finiteness of the queries
    (skipped with ``finite_checked``)."""
    n = _points_arg(query, "query") if finite_checked else _finite_points(query, "query")
    if not isinstance(grid, dict) or not {"keys", "points", "lo", "cell", "inv", "dims", "m"} <= set(grid):
        raise ValueError("grid must be the dict that points_grid returns")
    m = int(grid["m"])
    dev = query.device
    d2 = torch.empty(n, dtype=F32, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return d2, idx
    grid_c = _grid_c(grid)
    L = lib()

    def run(q, out_d2, out_idx):
        check(L.nerf_points_nearest(ptr(q), n, ptr(grid["keys"]) if m else None, ptr(grid["points"]) if m else None,
                                    m, *grid_c, ptr(out_d2), ptr(out_idx), stream()), "nerf_points_nearest")

    if not sort_queries or m == 0:
        run(query, d2, idx)
    else:
        _run_sorted(query, n, grid_c, (d2, idx), run)
    return d2, idx


# ------------------------------------------------------------------ exact point-to-surface distance


_FACE_GRID_KEYS = {"keys", "lo", "cell", "inv", "dims", "n_keys", "F"}


def mesh_face_grid(vertices, faces, cell_size=None):
    """The search grid of a mesh's faces (nerf_mesh_face_cell_counts -> torch.cumsum -> nerf_mesh_face_cell_keys ->
    torch.sort): vertices (V,3) float32, finite; faces (F,3) int32.  Returns the dict {keys (n_keys,) int64 sorted, lo
    (3 floats), cell, inv (fp32 values as floats), dims (3 ints), n_keys, F}.  A face is registered in every cell of
    the index box of its bounding box, key = (cell_id << 32) | face; binning is by bounding box, not by exact
    triangle / box overlap.  lo and the box are those of ALL vertices, used by a face or not (a vertex no face uses
    only enlarges the grid).  The default cell is longest extent / clamp(ceil(sqrt(F) / 2), 1, 1024), about two faces
    of an even triangulation per cell edge; an all-zero extent gets cell = 1.  dims = floor((max - lo) * inv) + 1 per
    axis in fp32.  ``cell_size``: a finite positive float; ValueError if it needs more than 1024 cells on an axis, and
    ValueError before the key launch when the faces have 2^31 keys or more between them (a finer cell_size, or faces
    that span the grid, multiply the keys: 8 bytes each).  F == 0 gives an empty grid.  Host reads: the box (it carries
    the finiteness check), the index range, the total number of keys."""
    V = _vertices_arg(vertices)
    _, F = _faces_arg(faces, V)
    if cell_size is not None:
        _cell_size_arg(cell_size)
    dev = vertices.device
    box = _finite_box(vertices, "vertices") if V else None
    lo, cell, inv, dims = _grid_from_box(box if F else None, F, cell_size, "vertices")
    grid = {"lo": lo, "cell": cell, "inv": inv, "dims": dims, "n_keys": 0, "F": F}
    if F == 0:
        grid["keys"] = torch.empty(0, dtype=torch.int64, device=dev)
        return grid
    lo_c, _, _, dims_c = _grid_c(grid)
    L = lib()
    counts = torch.empty(F, dtype=torch.int64, device=dev)
    check(L.nerf_mesh_face_cell_counts(ptr(vertices), ptr(faces), F, lo_c, inv, dims_c, ptr(counts), stream()),
          "nerf_mesh_face_cell_counts")
    ends = torch.cumsum(counts, 0)
    n_keys = int(ends[-1])
    if n_keys >= 2 ** 31:
        raise ValueError(f"the faces are registered in {n_keys} cells, 2^31 or more: use a larger cell_size")
    keys = torch.empty(n_keys, dtype=torch.int64, device=dev)
    check(L.nerf_mesh_face_cell_keys(ptr(vertices), ptr(faces), F, lo_c, inv, dims_c, ptr(ends - counts), ptr(keys),
                                     stream()), "nerf_mesh_face_cell_keys")
    grid["keys"], grid["n_keys"] = torch.sort(keys).values, n_keys
    return grid


def _face_grid_arg(grid, F):
    """(keys, n_keys) of a grid of mesh_face_grid; ValueError unless it is one and belongs to F faces."""
    if not isinstance(grid, dict) or not _FACE_GRID_KEYS <= set(grid):
        raise ValueError("grid must be the dict that mesh_face_grid returns")
    n_keys = int(grid["n_keys"])
    keys = grid["keys"]
    if int(grid["F"]) != F or not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64 or \
            tuple(keys.shape) != (n_keys,) or (F == 0) != (n_keys == 0):
        raise ValueError(f"grid does not belong to these faces: grid F = {grid['F']}, n_keys = {n_keys}, F = {F}")
    if n_keys:
        need(keys, "grid['keys']", torch.int64)
    return keys, n_keys


def mesh_nearest_faces(query, vertices, faces, grid, sort_queries=True, closest=True, finite_checked=False):
    """The nearest face of every query (nerf_mesh_nearest_faces): query (n,3) float32, finite; vertices and faces the
    mesh that ``grid`` = mesh_face_grid(vertices, faces) was built from.  Returns (d2 (n,) float64, face (n,) int32)
    and, with ``closest``, the closest point (n,3) float32: d2 is the squared distance, in double, from the query to
    the closest point of the face (Ericson's region walk over the fp32 corners), face the nearest
    face, the smallest index on equal d2, and the point that closest point rounded to fp32; exactly what a brute-force
    search over all faces gives, bit for bit.  A face without area counts as its three edges.  A mesh without faces
    gives d2 = +inf, face = -1 and the query itself as the point.  ``sort_queries``: present the queries in the order
    of their own cell keys (as points_nearest does); the result is the same either way.  Host reads: the finiteness of
    the queries and of the vertices and the index range, all three skipped with ``finite_checked`` (the caller has
    made them, as mesh_face_grid does for the mesh)."""
    n = _points_arg(query, "query") if finite_checked else _finite_points(query, "query")
    V = _vertices_arg(vertices) if finite_checked else _finite_vertices(vertices)
    _, F = _faces_arg(faces, V, ranges_checked=finite_checked)
    keys, n_keys = _face_grid_arg(grid, F)
    dev = query.device
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    point = torch.empty((n, 3), dtype=F32, device=dev) if closest else None
    if n == 0:
        return (d2, face, point) if closest else (d2, face)
    grid_c = _grid_c(grid)
    L = lib()

    def run(q, out_d2, out_face, out_point):
        check(L.nerf_mesh_nearest_faces(ptr(q), n, ptr(keys) if n_keys else None, n_keys,
                                        ptr(vertices) if n_keys else None, ptr(faces) if n_keys else None, F, *grid_c,
                                        ptr(out_d2), ptr(out_face), ptr(out_point), stream()),
              "nerf_mesh_nearest_faces")

    if not sort_queries or n_keys == 0:
        run(query, d2, face, point)
    else:
        _run_sorted(query, n, grid_c, (d2, face, point), run)
    return (d2, face, point) if closest else (d2, face)


# ------------------------------------------------------------------ nearest-hit ray casting


def _rays_arg(rays, finite_checked=False):
    """rays (n,8) float32 rows [o, d, near, far]: o and d finite, d not all zero, near and far no NaN (one host read,
    skipped with ``finite_checked``)."""
    need(rays, "rays")
    if rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError(f"rays must be (n,8), got {tuple(rays.shape)}")
    n = int(rays.shape[0])
    if n >= 2 ** 31:
        raise ValueError("rays must have fewer than 2^31 rows")
    if n and not finite_checked:
        bad = torch.stack([(~torch.isfinite(rays[:, :6])).any(), (rays[:, 3:6] == 0).all(1).any(),
                           torch.isnan(rays[:, 6:]).any()]).tolist()
        if bad[0]:
            raise ValueError("the origins and directions of the rays must be finite")
        if bad[1]:
            raise ValueError("a ray's direction must not be all zeros")
        if bad[2]:
            raise ValueError("near and far must not be NaN")
    return n


def mesh_ray_cast(rays, vertices, faces, grid, cull_backfaces=False, finite_checked=False):
    """The nearest face every ray hits (nerf_mesh_ray_cast): rays (n,8) float32 rows [o, d, near, far] as
    rays_for_camera packs them, the ray's points o + t d with d not normalised; vertices and faces the mesh that
    ``grid`` = mesh_face_grid(vertices, faces) was built from.  Returns (t (n,) float64, face (n,) int32, bary (n,2)
    float32): t the ray's own parameter of the nearest hit with near <= t <= far, +inf on a miss; face the face hit,
    the smallest index on equal t, -1 on a miss; bary = (u, v), the hit point being (1 - u - v) a + u b + v c of the
    face's corners, (0, 0) on a miss; exactly what testing every face gives, bit for bit (the test: DESIGN §3.11.6).  A
    face without area is never hit.  ``cull_backfaces``: only faces whose winding normal points against the ray.
    ``far < near`` is a miss, +-inf are allowed.  A mesh without faces gives all misses without a launch.
    ValueError before any launch on CPU tensors, wrong dtypes or shapes, non-finite origins or directions, a direction
    of all zeros, NaN in near / far, non-finite vertices, out-of-range indices, a grid that is not the face grid of
    these faces, and a grid whose cell is below 2^-20 of the largest |coordinate| (sixteen fp32 ulps: the walk's
    argument needs the hit test's box margin within 2^-10 of a cell).  Host reads: the largest |coordinate| (it
    carries the finiteness of the vertices), and the rays' check and the index range, both skipped with
    ``finite_checked``."""
    n = _rays_arg(rays, finite_checked)
    V = _vertices_arg(vertices)
    _, F = _faces_arg(faces, V, ranges_checked=finite_checked)
    keys, n_keys = _face_grid_arg(grid, F)
    lo_c, cell, inv, dims_c = _grid_c(grid)
    c_max = float(vertices.abs().max()) if V else 0.0
    if not c_max < float("inf"):
        raise ValueError("vertices must be finite")
    if F and cell < 2.0 ** -20 * c_max:
        raise ValueError(f"the grid's cell {cell!r} is below 2^-20 of the largest |coordinate| {c_max!r}")
    dev = rays.device
    if F == 0 or n == 0:
        return (torch.full((n,), float("inf"), dtype=torch.float64, device=dev),
                torch.full((n,), -1, dtype=torch.int32, device=dev), torch.zeros((n, 2), dtype=F32, device=dev))
    t = torch.empty(n, dtype=torch.float64, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    bary = torch.empty((n, 2), dtype=F32, device=dev)
    check(lib().nerf_mesh_ray_cast(ptr(rays), n, ptr(keys), n_keys, ptr(vertices), ptr(faces), F, lo_c, cell, inv,
                                   dims_c, 2.0 ** -30 * c_max, int(bool(cull_backfaces)), ptr(t), ptr(face), ptr(bary),
                                   stream()), "nerf_mesh_ray_cast")
    return t, face, bary


# ------------------------------------------------------------------ crossing counts


def mesh_point_crossings(query, vertices, faces, grid, sort_queries=True, finite_checked=False):
    """The faces crossed by the vertical ray from every query (nerf_mesh_point_crossings): query (n,3) float32, finite;
    vertices and faces the mesh that ``grid`` = mesh_face_grid(vertices, faces) was built from.  Returns (crossings
    (n,) int32, winding (n,) int32): the number of faces the open ray q + t e_z, t > 0, crosses and the sum of the signs
    of their projected orientations (+1 inside a closed mesh whose normals point outwards); exactly what testing every
    face gives, bit for bit.  Whether q's vertical line passes through a face's projection is decided exactly, with q
    perturbed symbolically by (+eps, +eps^2), so a ray through a shared edge or a vertex of a closed mesh is counted
    once per sheet; the side of the face's plane is decided in rounded double, so only a query within
    rounding of the surface itself is unspecified, and even it is deterministic.  A vertical or degenerate face is never
    crossed.  ``sort_queries``: present the queries in the order of their own cell keys (as points_nearest does); the
    result is the same either way.  F == 0 or n == 0 gives zeros without a launch.  ValueError before any launch on
    CPU tensors, wrong dtypes or shapes, non-finite queries or vertices, out-of-range indices and a grid that is not
    the face grid of these faces.  Host reads: the finiteness of the queries and of the vertices and the index range,
    all three skipped with ``finite_checked``."""
    n = _points_arg(query, "query") if finite_checked else _finite_points(query, "query")
    V = _vertices_arg(vertices) if finite_checked else _finite_vertices(vertices)
    _, F = _faces_arg(faces, V, ranges_checked=finite_checked)
    keys, n_keys = _face_grid_arg(grid, F)
    dev = query.device
    if F == 0 or n == 0:
        return torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    crossings = torch.empty(n, dtype=torch.int32, device=dev)
    winding = torch.empty(n, dtype=torch.int32, device=dev)
    grid_c = _grid_c(grid)
    L = lib()

    def run(q, out_c, out_w):
        check(L.nerf_mesh_point_crossings(ptr(q), n, ptr(keys), n_keys, ptr(vertices), ptr(faces), F, *grid_c,
                                          ptr(out_c), ptr(out_w), stream()), "nerf_mesh_point_crossings")

    if not sort_queries:
        run(query, crossings, winding)
    else:
        _run_sorted(query, n, grid_c, (crossings, winding), run)
    return crossings, winding


def box_points(n, lo, hi, seed=0, device=None):
    """n points distributed uniformly over the box [lo, hi] (nerf_box_points): n an int in [0, 2^31); lo and hi 3 finite
    floats each, taken as fp32, with lo <= hi and a finite difference; seed an int in [0, 2^64); ``device`` a HIP
    device (default: the current one).  Returns (n,3) float32: coordinate c of point i is lo_c + u (hi_c - lo_c) in
    fp32 with u a 24-bit counter random number of (seed, c, i) in [0, 1): point i depends on (seed, i) and the box
    alone, bitwise reproducible, and a prefix of a longer run.  ValueError before the launch on a bad argument."""
    import numpy as np
    n, seed = _count_arg(n), _seed_arg(seed)
    try:
        with np.errstate(all="ignore"):
            box = [np.asarray([float(x) for x in (b.reshape(-1).tolist() if isinstance(b, torch.Tensor) else b)],
                              np.float32) for b in (lo, hi)]
    except (TypeError, ValueError):
        raise ValueError(f"lo and hi must be 3 floats each, got {lo!r} and {hi!r}") from None
    with np.errstate(all="ignore"):
        if box[0].shape != (3,) or box[1].shape != (3,) or not (np.isfinite(box[0]).all() and np.isfinite(box[1]).all()
                                                               and (box[0] <= box[1]).all()
                                                               and np.isfinite(box[1] - box[0]).all()):
            raise ValueError(f"lo and hi must be 3 finite floats each with lo <= hi, got {lo!r} and {hi!r}")
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError("nerf_amd ops take HIP device tensors only (no CPU fallback)")
    points = torch.empty((n, 3), dtype=F32, device=dev)
    if n:
        with torch.cuda.device(dev):
            check(lib().nerf_box_points(n, seed, (ctypes.c_float * 3)(*box[0].tolist()),
                                        (ctypes.c_float * 3)(*box[1].tolist()), ptr(points), stream()),
                  "nerf_box_points")
    return points


# ------------------------------------------------------------------ generalised winding number


_WINDING_KEYS = {"keys", "runs", "moments", "soup", "lo", "cell", "inv", "dims", "B", "F"}


def _bricks_per_axis(F):
    """the default: clamp(ceil(1.25 F^(1/4)), 1, 1024)"""
    import math
    return min(max(math.ceil(1.25 * F ** 0.25), 1), MAX_GRID_DIM)


def mesh_winding_bricks(vertices, faces, bricks_per_axis=None):
    """The bricks of the generalised winding number (nerf_mesh_winding_keys -> torch.sort -> nerf_mesh_winding_soup ->
    nerf_mesh_winding_moments): vertices (V,3) float32, finite; faces (F,3) int32.  Every face belongs to ONE brick,
    the cell of its fp32 centroid ((a + b) + c) * fp32(1/3) in a coarse grid over the box of ALL vertices (unlike
    mesh_face_grid, which registers a face in every cell of its bounding box).  ``bricks_per_axis``: the cells along
    the longest extent, an int in [1, 1024]; default clamp(ceil(1.25 F^(1/4)), 1, 1024).  cell = longest extent /
    bricks_per_axis (1 for an all-zero extent), dims = min(floor((max - lo) * inv) + 1, bricks_per_axis) per axis in
    fp32.  Returns the dict {keys (F,) int64 sorted, (brick << 32) | face; runs (B,2) int32, the sorted positions
    [start, end) of every occupied brick; moments (B,7) float64, per brick the area-weighted centroid p (the plain
    mean of the face centroids when the brick has no area), the dipole n = sum of 0.5 (b - a) x (c - a) and r2, the
    largest squared distance from p to a corner of the brick; soup (F,9) float32, the corners in sorted order; lo (3
    floats), cell, inv (fp32 values as floats), dims (3 ints), B, F}: 8 + 36 bytes per face and 64 per occupied brick.
    The sums run in sorted order with one owner per brick: bitwise reproducible (and serial within a brick: a
    bricks_per_axis far below the default makes the build slow on a large mesh).  F == 0 gives an empty grid (B = 0).
    ValueError before any launch on CPU tensors, wrong dtypes or shapes, non-finite vertices, out-of-range indices and
    a bad bricks_per_axis.  Host reads: the box (it carries the finiteness check), the index range, and the number of
    occupied bricks."""
    V = _vertices_arg(vertices)
    _, F = _faces_arg(faces, V)
    if bricks_per_axis is not None and (isinstance(bricks_per_axis, bool) or not isinstance(bricks_per_axis, int)
                                        or not 1 <= bricks_per_axis <= MAX_GRID_DIM):
        raise ValueError(f"bricks_per_axis must be an int in [1, {MAX_GRID_DIM}], got {bricks_per_axis!r}")
    dev = vertices.device
    box = _finite_box(vertices, "vertices") if V else None
    k = _bricks_per_axis(F) if bricks_per_axis is None else bricks_per_axis
    lo, cell, inv, dims = _grid_from_box(box if F else None, F, None, "vertices", per_axis=k)
    bricks = {"lo": lo, "cell": cell, "inv": inv, "dims": dims, "B": 0, "F": F}
    if F == 0:
        bricks.update(keys=torch.empty(0, dtype=torch.int64, device=dev),
                      runs=torch.empty((0, 2), dtype=torch.int32, device=dev),
                      moments=torch.empty((0, 7), dtype=torch.float64, device=dev),
                      soup=torch.empty((0, 9), dtype=F32, device=dev))
        return bricks
    lo_c, _, _, dims_c = _grid_c(bricks)
    L = lib()
    keys = torch.empty(F, dtype=torch.int64, device=dev)
    check(L.nerf_mesh_winding_keys(ptr(vertices), ptr(faces), F, lo_c, inv, dims_c, ptr(keys), stream()),
          "nerf_mesh_winding_keys")
    keys = torch.sort(keys).values
    soup = torch.empty((F, 9), dtype=F32, device=dev)
    check(L.nerf_mesh_winding_soup(ptr(vertices), ptr(faces), F, ptr(keys), ptr(soup), stream()),
          "nerf_mesh_winding_soup")
    cells = keys >> 32
    first = torch.ones(F, dtype=torch.bool, device=dev)
    first[1:] = cells[1:] != cells[:-1]
    starts = torch.nonzero(first).reshape(-1)  # (B,) int64 ascending, starts[0] = 0; the host read of B
    B = int(starts.shape[0])
    runs = torch.empty((B, 2), dtype=torch.int32, device=dev)
    moments = torch.empty((B, 7), dtype=torch.float64, device=dev)
    check(L.nerf_mesh_winding_moments(ptr(soup), F, ptr(starts), B, ptr(runs), ptr(moments), stream()),
          "nerf_mesh_winding_moments")
    bricks.update(keys=keys, runs=runs, moments=moments, soup=soup, B=B)
    return bricks


def _winding_bricks_arg(bricks, F):
    """ValueError unless ``bricks`` is a dict of mesh_winding_bricks and belongs to F faces; returns B."""
    if not isinstance(bricks, dict) or not _WINDING_KEYS <= set(bricks):
        raise ValueError("bricks must be the dict that mesh_winding_bricks returns")
    B = int(bricks["B"])
    shapes = (("keys", torch.int64, (F,)), ("runs", torch.int32, (B, 2)), ("moments", torch.float64, (B, 7)),
              ("soup", F32, (F, 9)))
    if int(bricks["F"]) != F or not 0 <= B <= F or (F == 0) != (B == 0) or any(
            not isinstance(bricks[name], torch.Tensor) or bricks[name].dtype != dtype
            or tuple(bricks[name].shape) != shape for name, dtype, shape in shapes):
        raise ValueError(f"bricks do not belong to these faces: bricks F = {bricks['F']}, B = {B}, F = {F}")
    if F:
        for name, dtype, _ in shapes:
            need(bricks[name], f"bricks['{name}']", dtype)
    return B


def _beta_arg(beta):
    import math
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not math.isfinite(beta) or beta < 1:
        raise ValueError(f"beta must be a finite float >= 1, got {beta!r}")
    return float(beta)


def mesh_winding_number(query, vertices, faces, bricks, beta=3.0, exact=False, sort_queries=True,
                        finite_checked=False):
    """The generalised winding number of every query (nerf_mesh_winding): query (n,3) float32, finite; vertices and
    faces the mesh that ``bricks`` = mesh_winding_bricks(vertices, faces) was built from.  Returns w (n,) float64:
    (1 / 4 pi) times the sum over the faces of the signed solid angle 2 atan2(N, D) (Van Oosterom and Strackee) of the
    face seen from the query.  On a closed mesh whose normals point outwards (positive Mesh.volume()) w is 1 inside
    and 0 outside, the winding of mesh_point_crossings with the same sign; on an open or broken mesh it falls smoothly
    from about 1 to about 0 across the holes, and "inside" is w > 0.5.  ``exact``: every face by its solid angle, in
    sorted-face order, n x F of them.  Otherwise a brick with |p - q|^2 > beta^2 r2 (strictly) contributes its dipole
    (p - q) . n / |p - q|^3 and only the nearer bricks are summed face by face; the error falls as beta grows (DESIGN
    §3.11.10 has the table), beta a finite float >= 1.  One double accumulator per query, bricks in ascending key
    order, faces in sorted order: bitwise reproducible, independent of the other queries.  ON the surface w is
    whatever atan2(+-0, .) gives: deterministic, not meaningful.  ``sort_queries``: present the queries in the order
    of their own cell keys in the brick grid (as points_nearest does); the result is the same either way.  A mesh
    without faces gives zeros without a launch.  ValueError before any launch on CPU tensors, wrong dtypes or shapes,
    non-finite queries or vertices, out-of-range indices, a bad beta, and bricks that are not the dict of these faces.
    Host reads: the finiteness of the queries and of the vertices and the index range, all three skipped with
    ``finite_checked``."""
    beta = _beta_arg(beta)
    n = _points_arg(query, "query") if finite_checked else _finite_points(query, "query")
    V = _vertices_arg(vertices) if finite_checked else _finite_vertices(vertices)
    _, F = _faces_arg(faces, V, ranges_checked=finite_checked)
    B = _winding_bricks_arg(bricks, F)
    dev = query.device
    if F == 0 or n == 0:
        return torch.zeros(n, dtype=torch.float64, device=dev)
    w = torch.empty(n, dtype=torch.float64, device=dev)
    L = lib()

    def run(q, out_w):
        check(L.nerf_mesh_winding(ptr(q), n, ptr(bricks["runs"]), ptr(bricks["moments"]), B, ptr(bricks["soup"]), F,
                                  beta, int(bool(exact)), ptr(out_w), stream()), "nerf_mesh_winding")

    if not sort_queries:
        run(query, w)
    else:
        _run_sorted(query, n, _grid_c(bricks), (w,), run)
    return w


# ------------------------------------------------------------------ texture baking

ATLAS_MIN_TEXELS = 5
ATLAS_MAX_SIDE = 16384


def atlas_layout(n_faces, texels):
    """(cols, T) of the texture atlas of ``n_faces`` faces with cells of ``texels`` x ``texels`` texels: faces 2c and
    2c + 1 share cell c, cells = max(1, (F + 1) // 2), cols = the smallest integer with cols^2 >= cells (integer
    arithmetic), T = cols * texels; cell c starts at texel (texels * (c % cols), texels * (c // cols)).  ValueError on
    ``texels`` that is no int >= 5, a negative face count and T > 16384."""
    import math
    if isinstance(texels, bool) or not isinstance(texels, int) or texels < ATLAS_MIN_TEXELS:
        raise ValueError(f"texels must be an int >= {ATLAS_MIN_TEXELS}, got {texels!r}")
    F = int(n_faces)
    if F < 0:
        raise ValueError(f"the face count must be >= 0, got {F}")
    cells = max(1, (F + 1) // 2)
    cols = math.isqrt(cells - 1) + 1
    T = cols * texels
    if T > ATLAS_MAX_SIDE:
        raise ValueError(f"{F} faces at {texels} texels need a {T} x {T} texture: the limit is {ATLAS_MAX_SIDE}")
    return cols, T


def mesh_atlas_texels(vertices, faces, texels, vertex_normals=None, normals=True, ranges_checked=False):
    """What every texel of the atlas of (F, texels) stands for (nerf_mesh_atlas_texels): vertices
    (V,3) float32, faces (F,3) int32.  Returns a dict of (T,T,...) device tensors indexed [y, x]: "face" int32, the
    owning face or -1; "bary" (T,T,2) float32, the pair (b1, b2) of the surface point; "position" (T,T,3) float32 =
    b0 v0 + b1 v1 + b2 v2; with ``normals`` also "normal" (T,T,3) float32: the normalised mix of ``vertex_normals``
    (V,3) with the same weights, or without them the face's unit normal by its winding, zeros where the length is
    zero; and "texels", "cols", "T" as ints.  An unowned texel holds zeros.  A texel in the gutter of its face takes
    a nearby boundary point of that face.  NaN vertices propagate; F = 0 gives a T = texels atlas that nobody owns.
    Bitwise reproducible.  ValueError before the launch on CPU tensors, wrong dtypes or shapes, out-of-range indices
    (one host read, skipped with ``ranges_checked``), texels < 5 and T > 16384."""
    V = _vertices_arg(vertices)
    _, F = _faces_arg(faces, V, ranges_checked=ranges_checked)
    cols, T = atlas_layout(F, texels)
    if faces.device != vertices.device:
        raise ValueError("vertices and faces must be on one device")
    if vertex_normals is not None:
        if not normals:
            raise ValueError("vertex_normals are given but normals are not asked for")
        need(vertex_normals, "vertex_normals")
        if tuple(vertex_normals.shape) != (V, 3) or vertex_normals.device != vertices.device:
            raise ValueError(f"vertex_normals must be ({V},3) on the vertices' device, got {tuple(vertex_normals.shape)}")
    dev = vertices.device
    out = {"face": torch.empty((T, T), dtype=torch.int32, device=dev), "bary": torch.empty((T, T, 2), dtype=F32, device=dev),
           "position": torch.empty((T, T, 3), dtype=F32, device=dev)}
    if normals:
        out["normal"] = torch.empty((T, T, 3), dtype=F32, device=dev)
    check(lib().nerf_mesh_atlas_texels(ptr(vertices) if F else None, ptr(faces) if F else None, F, texels, T,
                                       ptr(vertex_normals) if F else None, ptr(out["face"]), ptr(out["bary"]),
                                       ptr(out["position"]), ptr(out.get("normal")), stream()),
          "nerf_mesh_atlas_texels")
    out.update(texels=texels, cols=cols, T=T)
    return out


def _texture_arg(texture, n_faces, texels):
    """texture (T,T,C) float32 on the device, 1 <= C <= 4, T the side of the atlas of (n_faces, texels)."""
    need(texture, "texture")
    if texture.dim() != 3 or texture.shape[0] != texture.shape[1] or not 1 <= texture.shape[2] <= 4:
        raise ValueError(f"texture must be (T,T,C) with 1 <= C <= 4, got {tuple(texture.shape)}")
    if isinstance(texels, bool) or not isinstance(texels, int) or texels < ATLAS_MIN_TEXELS:
        raise ValueError(f"texels must be an int >= {ATLAS_MIN_TEXELS}, got {texels!r}")
    side = int(texture.shape[0])
    if side % texels:
        raise ValueError(f"texels = {texels} does not divide the texture's side {side}")
    cols, T = atlas_layout(n_faces, texels)
    if side != T:
        raise ValueError(f"the atlas of {int(n_faces)} faces at {texels} texels is {T} x {T}, the texture is "
                         f"{side} x {side}")
    return T, int(texture.shape[2])


def mesh_texture_lookup(texture, texels, n_faces, face, bary, ranges_checked=False):
    """The texture at points of the surface (nerf_mesh_texture_lookup): texture (T,T,C) float32 over
    the atlas of (n_faces, texels), C in 1..4; face (N,) int32 and bary (N,2) float32 = (u, v) as mesh_ray_cast
    returns them, the point being (1 - u - v) a + u b + v c of the face's corners.  Returns (N,C) float32: the bilinear
    fetch at the face's own UV, written as lerps so that equal texels give their value exactly; zeros where face < 0.
    A point of a face blends texels of that face's half cell only, gutter included (no bleeding between faces).
    Bitwise reproducible.  ValueError before the launch on CPU tensors, wrong dtypes or shapes, a texture that is not
    the atlas of (n_faces, texels), and a face >= n_faces (one host read, skipped with ``ranges_checked``)."""
    F = int(n_faces)
    T, C = _texture_arg(texture, F, texels)
    if 3 * F >= 2 ** 31:
        raise ValueError(f"3 * F must be below 2^31, got F = {F}")
    need(face, "face", torch.int32)
    need(bary, "bary")
    if face.dim() != 1 or tuple(bary.shape) != (face.shape[0], 2):
        raise ValueError(f"face must be (N,) and bary (N,2), got {tuple(face.shape)}, {tuple(bary.shape)}")
    if face.device != texture.device or bary.device != texture.device:
        raise ValueError("face and bary must be on the texture's device")
    N = int(face.shape[0])
    if N >= 2 ** 31:
        raise ValueError("face must have fewer than 2^31 rows")
    if N and not ranges_checked and int(face.max()) >= F:
        raise ValueError(f"face must be below {F} (negative: no face), got {int(face.max())}")
    out = torch.empty((N, C), dtype=F32, device=texture.device)
    if N:
        check(lib().nerf_mesh_texture_lookup(ptr(texture), T, C, F, texels, ptr(face), ptr(bary), N, ptr(out),
                                             stream()), "nerf_mesh_texture_lookup")
    return out


# ------------------------------------------------------------------ optimiser


def grad_sqnorm(g, partials=None):
    if partials is None:
        partials = torch.empty(256, dtype=F32, device=g.device)
    check(lib().nerf_grad_sqnorm(ptr(g), g.numel(), ptr(partials), stream()), "nerf_grad_sqnorm")
    return partials


def adam(p, g, m, v, seg_off: Sequence[int], seg_lr: Sequence[float], step, betas=(0.9, 0.999), eps=1e-8,
         weight_decay=0.0, partials=None, max_norm=0.0):
    """nerf_adam; ``step`` an int, or an int64 device tensor holding the step count (nerf_adam_dstep)."""
    off = (ctypes.c_int64 * len(seg_off))(*seg_off)
    lr = (ctypes.c_double * len(seg_lr))(*seg_lr)
    if isinstance(step, torch.Tensor):
        need(step, "step", torch.int64)
        check(lib().nerf_adam_dstep(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), off, lr, len(seg_lr), betas[0],
                                    betas[1], eps, weight_decay, ptr(step), ptr(partials), max_norm, stream()),
              "nerf_adam_dstep")
        return
    check(lib().nerf_adam(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), off, lr, len(seg_lr), betas[0], betas[1], eps,
                          weight_decay, step, ptr(partials), max_norm, stream()), "nerf_adam")


def packed_points(rays, ray_idx, t0, t1):
    """nerf_packed_points: x_d (M,6) = [o + d (t0+t1)/2, d] of packed intervals."""
    M = ray_idx.numel()
    xd = torch.empty((M, 6), dtype=F32, device=rays.device)
    check(lib().nerf_packed_points(ptr(rays), ptr(ray_idx.to(torch.int32).contiguous()), ptr(t0), ptr(t1), M, ptr(xd),
                                   stream()), "nerf_packed_points")
    return xd
