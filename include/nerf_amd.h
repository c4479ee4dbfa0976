/*
 * nerf_amd.h — C-ABI of the MI355X (gfx950) NeRF hot-path library  libnerf_amd.so
 *
 * Every entry point is `extern "C"`, takes plain device pointers + sizes + a hipStream_t,
 * never allocates device memory, never synchronises the device, and returns an int status:
 *     0  ok
 *    <0  invalid argument (shape / alignment / enum)  — see NERF_E_* below
 *    >0  hipError_t of the failed launch (passthrough)
 * All buffers are caller-owned (PyTorch allocates them).  All floating point is fp32.
 * Thread-safe and re-entrant: no mutable global state.
 *
 * Each function names the reference interface it replaces (paths relative to
 * psklavos1/NeRF-Sys adaptive_nerf/).  INTEGRATION.md shows the ctypes binding.
 */
#ifndef NERF_AMD_H
#define NERF_AMD_H

#include <stdint.h>
#include <stddef.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NERF_OK 0
#define NERF_E_ARG (-1)      /* bad size / pointer */
#define NERF_E_ALIGN (-2)    /* pointer not 16-byte aligned */
#define NERF_E_ENUM (-3)     /* unknown enum value */
#define NERF_E_WORKSPACE (-4)/* workspace too small */
#define NERF_E_UNSUPPORTED (-5) /* valid arguments, but no kernel for this configuration (use the general path) */

/* ------------------------------------------------------------------ rays */

/* get_ray_directions (nerfs/ray_sampling.py:111-136) + get_rays (:50-108, _rays_cam_to_world :10-24)
 * + SceneBox.ray_aabb_intersect (nerfs/scene_box.py:45-107).
 * Pixel p of the batch is (img, row, col) = pix[3p..3p+2] (pix may be NULL: dense H*W image of
 * pose 0, row-major).  c2w: n_poses x 3 x 4 row-major.  aabb (6 floats min,max) or NULL for the
 * constant [near,far].  Writes rays (n,8) = [o, d, near, far].  If images_u8 != NULL (n_poses x H x
 * W x 3 bytes) the gathered pixel colour /255 is written to rgb_out (n,3).  A NaN in the pose reaches near and far
 * of the AABB test as NaN, as in the reference (torch's amax / clamp), so nerf_clamp_near_far calls the ray invalid. */
int nerf_rays_gen(const float* c2w, int n_poses, const int32_t* pix, int64_t n, int H, int W,
                  float fx, float fy, float cx, float cy, int center_pixels, float near_v, float far_v,
                  const float* aabb, float aabb_max_bound, float aabb_invalid,
                  const uint8_t* images_u8, float* rays_out, float* rgb_out, hipStream_t stream);

/* Random training batch: draws n (img,row,col) triplets with a counter-based RNG (seed) into
 * pix_out (n,3) — the data path of RamRaysDataset/DataLoader (pipelines/online_stage/runtime_adapt.py:76-86).
 * n == 0 is an empty call (here and in nerf_pick_pixels_dseed): pix_out may be NULL. */
int nerf_pick_pixels(int64_t n, int n_images, int H, int W, uint64_t seed, int32_t* pix_out,
                     hipStream_t stream);

/* nerf_pick_pixels with the seed seed_base + (*step_dev) * seed_mul read on the device (*step_dev: int64 step
 * counter in HBM), so a captured hipGraph draws a new batch per replay (tools/bench_container.py --graph; the
 * reference draws each batch from its host RNG, runtime_adapt.py:286-296). */
int nerf_pick_pixels_dseed(int64_t n, int n_images, int H, int W, uint64_t seed_base, uint64_t seed_mul,
                           const int64_t* step_dev, int32_t* pix_out, hipStream_t stream);

/* clamp_rays_near_far (nerfs/ray_sampling.py:139-176), in place; valid_out (n) bytes or NULL.
 * has_near/has_far select the overrides; a NaN near or far stays NaN through them (torch.maximum / minimum), so the
 * ray is invalid.  Here and in nerf_rays_ndc, nerf_sample_stratified, nerf_build_xd,
 * nerf_sample_pdf and nerf_freq_encode n == 0 is an empty call: the scalar arguments are still checked, the buffers
 * may be NULL. */
int nerf_clamp_near_far(float* rays, int64_t n, int has_near, float near_v, int has_far, float far_v,
                        float eps, float invalid_value, uint8_t* valid_out, hipStream_t stream);

/* Forward-facing NDC rays (canonical NeRF; absent in the reference).  rays_in/out (n,8); output
 * near=0, far=1. */
int nerf_rays_ndc(const float* rays_in, int64_t n, int H, int W, float focal, float near_plane,
                  float* rays_out, hipStream_t stream);

/* ------------------------------------------------------------------ sampling */

/* stratified_t_vals (nerfs/ray_rendering.py:262-287).  randomized!=0 jitters each interval with u
 * (n,S) if given, else with the counter RNG (seed).  t_out (n,S). */
int nerf_sample_stratified(const float* rays, int64_t n, int S, int randomized, const float* u,
                           uint64_t seed, float* t_out, hipStream_t stream);

/* Point construction of render_rays_stratified (nerfs/ray_rendering.py:317-319):
 * x_d[r*S+s] = [o + d t, d]  (n*S, 6). */
int nerf_build_xd(const float* rays, const float* t, int64_t n, int S, float* xd_out, hipStream_t stream);

/* Hierarchical inverse-CDF resampling (canonical NeRF sample_pdf; ABSENT in the reference).
 * t (n,S) sorted coarse depths, w (n,S) coarse weights.  Draws n_imp samples from the pdf of the
 * interior weights over the S-1 t-midpoints (u (n,n_imp) in [0,1) if given, else linspace when
 * det!=0, else counter RNG(seed)), and writes the sorted union t_out (n, S+n_imp).
 * Requires S+n_imp <= 512 and S >= 3. */
int nerf_sample_pdf(const float* t, const float* w, int64_t n, int S, int n_imp, const float* u, int det,
                    uint64_t seed, float* t_out, hipStream_t stream);

/* ------------------------------------------------------------------ encoding */

/* FrequencyEncoder.torch_forward (models/encodings.py:437-444): out (n, D*(2L+inc)) with row
 * stride ld_out floats; per dim [cos 2^0..2^{L-1}, sin ...] after the optional raw input.  L = 0 without the input
 * has no output element: an empty call as well. */
int nerf_freq_encode(const float* x, int64_t n, int D, int L, int include_input, float* out, int ld_out,
                     hipStream_t stream);

/* ------------------------------------------------------------------ MLP (vanilla expert) */

/* Packed weight layout of the 8x256 NeRF MLP (models/inr/meta_vanilla.py:13-154, frequency dirs):
 * tensors (PyTorch (out,in) row-major, zero-padded):  trunk.i W (256 x Kpad_i) b(256), i=0..7 with
 * Kpad = 64 / 256 / 320 (skip, [h|enc] hidden first) ; head W (32 x 256) rows [sigma, geo0..14, 0..]
 * b(32) ; color0 W (128 x 64) cols [geo 15 | dir-enc 27 | 0] b(128) ; color1 W (32 x 128) b(32).
 * nerf_mlp_layout fills table[t*4 + {offset, rows, cols_padded, cols_real}] for t < 22 tensors
 * (order: W0,b0,...,W7,b7, Wh,bh, Wc0,bc0, Wc1,bc1) and returns the total packed floats. */
int64_t nerf_mlp_layout(int64_t* table);

/* Workspace (bytes) needed by nerf_mlp_fwd/bwd for M samples.  training!=0 keeps every
 * activation for nerf_mlp_bwd, and one [Mp][256] fp32 input-gradient buffer per trunk layer (Mp = M rounded up to
 * 256): the weight gradient of a layer reads its dZ after the chained input-gradient launch has run.  That is six
 * buffers more than a two-buffer ping-pong, 4.8 GB at M = 4096 x 192. */
int64_t nerf_mlp_workspace_bytes(int64_t M, int training);

/* expert(x_d (M,6), params) -> (M,4) [sigmoid rgb, trunc_exp sigma]  (meta_vanilla.py:123-154,
 * metamodule.py:140-156, trunc_exp.py:43-61).  w: packed weights.  ws: workspace (16B aligned).
 * M = 0 is an empty call: x_d / rgb_sigma (and the backward's d_rgb_sigma) may be null; the backward then zero-fills
 * d_w (accumulate = 0) or leaves it untouched.  The same holds for the _bf16 / _f16 entry points. */
int nerf_mlp_fwd(const float* w, const float* x_d, int64_t M, float* rgb_sigma, void* ws, int64_t ws_bytes,
                 int training, hipEvent_t* events, hipStream_t stream);

/* events: NULL, or 16 caller-created hipEvent_t recorded on `stream` around each trunk layer's GEMM
 * (events[2i], events[2i+1] bracket trunk.i) — for live per-kernel timing (bench.py roofline). */

/* Backward of nerf_mlp_fwd (autograd of the same modules).  Needs the workspace of a training
 * forward on the same x_d/w.  d_w (packed layout) is overwritten, or accumulated into if
 * accumulate!=0. */
int nerf_mlp_bwd(const float* w, int64_t M, const float* d_rgb_sigma, float* d_w, int accumulate, void* ws,
                 int64_t ws_bytes, hipEvent_t* events, hipStream_t stream);
/* events: NULL, or 32 hipEvent_t: events[4i+0/1] bracket the weight-gradient GEMM of trunk.i,
 * events[4i+2/3] its input-gradient GEMM (i >= 1); events[2/3] bracket the backward tail (colour branch + head -> dZ7). */

/* nerf_mlp_bwd with the weight-gradient GEMMs on a second stream: the input-gradient chain (colour branch, head and
 * trunk dgrads) stays on `stream`; each weight-gradient GEMM runs on `wgrad_stream` behind an event recorded on
 * `stream` after the launch that produced its input; `stream` waits for `wgrad_stream` before the final split reduce,
 * so d_w is complete in `stream` order.  sync: 10 caller-created hipEvent_t (hipEventDisableTiming is fine).  The
 * workspace keeps one input-gradient buffer per trunk layer: nerf_mlp_workspace_bytes_2s(M) bytes, filled by a
 * training nerf_mlp_fwd (the same layout and size as nerf_mlp_workspace_bytes(M, 1)).  Same kernels, grids and split
 * slabs as nerf_mlp_bwd: d_w is bitwise equal.  The events[4i+0/1] of a weight-gradient GEMM are recorded on
 * wgrad_stream. */
int64_t nerf_mlp_workspace_bytes_2s(int64_t M);
int nerf_mlp_bwd_2s(const float* w, int64_t M, const float* d_rgb_sigma, float* d_w, int accumulate, void* ws,
                    int64_t ws_bytes, hipEvent_t* events, hipStream_t stream, hipStream_t wgrad_stream, hipEvent_t* sync);

/* fp32 GEMM engine of the three calls above.  Default (flags 0, and the un-suffixed entry points): the 256-wide
 * trunk GEMMs (forward, input gradient, weight gradient) run on the bf16 matrix cores as split products — every fp32
 * operand is cut into three bf16 pieces hi + mid + lo that sum to it exactly, and the six piece products down to
 * 2^-16 of the leading one are accumulated in fp32 (v_mfma_f32_32x32x16_bf16); measured error against fp64 equals the
 * fp32 MFMA's and a sequential fp32 fmaf chain's (tools/split_probe.hip); the input-gradient GEMMs keep the small
 * products in separate accumulators (see NERF_MLP_NATIVE_DGRAD).  NERF_MLP_NATIVE_FP32 selects the
 * v_mfma_f32_16x16x4_f32 kernels instead.  Unknown flag bits: NERF_E_ENUM.  Replaces the same reference interfaces as
 * nerf_mlp_fwd / nerf_mlp_bwd (MetaNeRF forward / autograd, models/inr/meta_vanilla.py:123-154). */
#define NERF_MLP_NATIVE_FP32 1
/* NERF_MLP_NATIVE_DGRAD (backward, with the split engine): the input-gradient GEMMs on the fp32 MFMA kernels.  By
 * default they are split products too, with the five small products in accumulators of their own: the bf16 MFMA adds
 * each 16-product sum to its fp32 accumulator with one guard bit (tools/mfma_round_probe.hip), and with ONE accumulator
 * that biased the long signed input-gradient chain (weight gradients 1.3-20x the fp32 engine's error); with separate
 * small-term accumulators they are as accurate as the fp32 engine's (tests/test_gpu_split_gemm.py). */
#define NERF_MLP_NATIVE_DGRAD 2
/* NERF_MLP_FWD_LAYERED (forward, with the split engine): one GEMM launch per trunk layer.  By default the split
 * forward is four launches — xyz encoding, weight piece planes, ONE chained launch that carries every 256-row tile
 * through the eight trunk layers, and the head / colour tail — in training and in eval.  The chained launch runs the
 * per-layer kernel's tile code once per layer, so every stored value (activations, ReLU mask words) is bitwise the
 * layered form's (tests/test_gpu_fwd_chain.py).  A call with events != NULL also runs the eight launches, because an
 * event pair brackets one layer's launch: per-layer timings are always those of a layer launched alone.  No effect
 * with NERF_MLP_NATIVE_FP32.  nerf_mlp_bwd_ex does not know this bit (NERF_E_ENUM). */
#define NERF_MLP_FWD_LAYERED 4
/* NERF_MLP_BWD_LAYERED (backward, with the split engine): one input-gradient launch per trunk layer, each followed by
 * the layer's weight gradient.  By default nerf_mlp_bwd runs the seven trunk input gradients in ONE chained launch
 * (a 256-row tile per workgroup, both 128-column tiles of every layer) right after the head backward, and the weight
 * gradients after it.  The chained launch runs the per-layer kernel's tile code, so every dZ_i and d_w are bitwise the
 * layered form's (tests/test_gpu_bwd_chain.py).  The layered form also runs when events != NULL (an event pair brackets
 * one launch), with a weight-gradient stream (nerf_mlp_bwd_2s), with NERF_MLP_NATIVE_DGRAD and with
 * NERF_MLP_NATIVE_FP32.  nerf_mlp_fwd_ex does not know this bit (NERF_E_ENUM). */
#define NERF_MLP_BWD_LAYERED 8
int nerf_mlp_fwd_ex(const float* w, const float* x_d, int64_t M, float* rgb_sigma, void* ws, int64_t ws_bytes,
                    int training, int flags, hipEvent_t* events, hipStream_t stream);
int nerf_mlp_bwd_ex(const float* w, int64_t M, const float* d_rgb_sigma, float* d_w, int accumulate, void* ws,
                    int64_t ws_bytes, int flags, hipEvent_t* events, hipStream_t stream);
int nerf_mlp_bwd_2s_ex(const float* w, int64_t M, const float* d_rgb_sigma, float* d_w, int accumulate, void* ws,
                       int64_t ws_bytes, int flags, hipEvent_t* events, hipStream_t stream, hipStream_t wgrad_stream,
                       hipEvent_t* sync);

/* bf16 variants (BASELINE configs[2]: "bf16 MLP with fp32 compositing"): the same network, packed fp32
 * parameters, inputs and outputs as nerf_mlp_fwd/bwd; the layer GEMMs run on bf16 MFMA with fp32
 * accumulation and the activations / activation gradients live in the workspace as bf16.  The weight
 * gradient d_w is fp32.  Not bit-compatible with the fp32 path (tolerance: bf16 rounding).
 * flags (0 = the production kernels; a bitwise OR of):
 *   NERF_BF16_LAYERED_FWD  one GEMM launch per layer instead of the fused single-launch forward;
 *   NERF_BF16_LAYERED_BWD  one dgrad + one wgrad GEMM launch per layer instead of the fused per-layer backward.
 *                          The backward of a workspace must be called with the same NERF_BF16_LAYERED_BWD bit as
 *                          the training forward that filled it (the layered backward reads ReLU bitmasks that only
 *                          such a forward writes).
 * The layered launches are the bitwise references of the fused kernels (tests/test_gpu_bf16.py); unknown bits ->
 * NERF_E_ENUM.  The split counts are compile-time constants (NERF_BF16_MAX_SPLITS, NERF_BF16_NARROW_MUL). */
#define NERF_BF16_LAYERED_FWD 1
#define NERF_BF16_LAYERED_BWD 2
int64_t nerf_mlp_workspace_bytes_bf16(int64_t M, int training);
int nerf_mlp_fwd_bf16(const float* w, const float* x_d, int64_t M, float* rgb_sigma, void* ws, int64_t ws_bytes,
                      int training, int flags, hipEvent_t* events, hipStream_t stream);
int nerf_mlp_bwd_bf16(const float* w, int64_t M, const float* d_rgb_sigma, float* d_w, int accumulate, void* ws,
                      int64_t ws_bytes, int flags, hipEvent_t* events, hipStream_t stream);
/* events: as for nerf_mlp_fwd / nerf_mlp_bwd. */

/* fp16 variants: the reference's AMP training loop (pipelines/online_stage/runtime_adapt.py:291-310,
 * configs/train.json "use_amp": torch.autocast(float16) + GradScaler) on the same fused kernels as the bf16 entry
 * points, with fp16 operands on v_mfma_f32_32x32x16_f16 (fp32 accumulation) and the reference's rounding points under
 * autocast (models/metamodule/metamodule.py:150-156: `inputs.matmul(weight.t()) + bias`):
 *   forward   every layer output = fp32(fp16(x16 W16^T)) + bias (fp32), ReLU, then fp16 as the next matmul's operand;
 *             the heads / colour-out pre-activations (sigma's trunc_exp input, clamp 88.72) stay fp32;
 *   backward  activation gradients fp16 (the matmul backward's fp16 outputs), weight gradients summed in fp32 and
 *             rounded to fp16 once per call (the fp16 grad of the autocast weight cast, then fp32), bias gradients
 *             fp32 sums; d_w is fp32 and accumulates in fp32 after the rounding.
 * Workspace as nerf_mlp_workspace_bytes_bf16.  flags: 0 only (no layered form; other bits NERF_E_ENUM). */
int64_t nerf_mlp_workspace_bytes_f16(int64_t M, int training);
int nerf_mlp_fwd_f16(const float* w, const float* x_d, int64_t M, float* rgb_sigma, void* ws, int64_t ws_bytes,
                     int training, int flags, hipEvent_t* events, hipStream_t stream);
int nerf_mlp_bwd_f16(const float* w, int64_t M, const float* d_rgb_sigma, float* d_w, int accumulate, void* ws,
                     int64_t ws_bytes, int flags, hipEvent_t* events, hipStream_t stream);

/* ------------------------------------------------------------------ compositing + loss */

/* volume_render (nerfs/ray_rendering.py:114-165, raw_rgb=raw_sigma=False).  rgb_sigma (n,S,4),
 * t (n,S), bg (n,3) or NULL.  Outputs rgb (n,3), depth (n), weights (n,S), acc (n).
 * Optional fused loss head (nerfs/losses.py:10-32 + color_space.py:22-66): if gt != NULL,
 * loss_sum[0] += inv_count * sum((cs(pred)-cs(gt))^2) and d_rgb (n,3) = dloss/drgb.
 * color_space: 0 linear, 1 srgb, 2 identity.  S <= 1024. */
int nerf_composite_fwd(const float* rgb_sigma, const float* t, const float* bg, int64_t n, int S,
                       float sigma_scale, float* rgb, float* depth, float* weights, float* acc,
                       const float* gt, int color_space, float inv_count, float* loss_sum, float* d_rgb,
                       hipStream_t stream);

/* Backward of volume_render: upstream grads g_rgb (n,3) [required], g_depth (n), g_acc (n),
 * g_weights (n,S) [each nullable] -> d_rgb_sigma (n,S,4). */
int nerf_composite_bwd(const float* rgb_sigma, const float* t, const float* bg, int64_t n, int S,
                       float sigma_scale, const float* g_rgb, const float* g_depth, const float* g_acc,
                       const float* g_weights, float* d_rgb_sigma, hipStream_t stream);

/* ------------------------------------------------------------------ image metrics */

/* runtime_evaluate's full-image metrics (pipelines/online_stage/runtime_adapt.py:150-158): color_space_transformer
 * (nerfs/color_space.py:22-66) on both images, then the MSE of PSNR and pytorch_msssim.ssim(data_range=1) per channel
 * (11-tap Gaussian window, sigma 1.5, valid convolution, C1 = 1e-4, C2 = 9e-4, mean of the unclamped map).
 * pred (n_img,H,W,3) is the linear render; the ground truth is 8-bit sRGB (gt_u8, converted as v / 255) or the same
 * as floats (gt_f32): exactly one of the two is non-NULL.  color_space as nerf_composite_fwd.  H, W >= 11.
 * out (n_img,4) = mse, ssim_r, ssim_g, ssim_b.  ws: nerf_image_metrics_workspace_bytes bytes, 16-byte aligned
 * (per-tile partial sums; a second launch adds them in a fixed order in double, so equal inputs give equal bits).
 * n_img == 0 is an empty call.  nerf_image_metrics_tile reports the SSIM-map pixels one workgroup covers. */
int nerf_image_metrics_tile(int* tile_h, int* tile_w);
int64_t nerf_image_metrics_workspace_bytes(int64_t n_img, int H, int W);
int nerf_image_metrics(const float* pred, const float* gt_f32, const uint8_t* gt_u8, int64_t n_img, int H, int W,
                       int color_space, void* ws, int64_t ws_bytes, float* out, hipStream_t stream);

/* ------------------------------------------------------------------ optimiser */

/* Per-block partial sums of squares of g (n) into partials[256] (first pass of
 * clip_grad_norm_, pipelines/online_stage/runtime_adapt.py:305-307).  n == 0 (g may be NULL) writes 256 zeros. */
int nerf_grad_sqnorm(const float* g, int64_t n, float* partials, hipStream_t stream);

/* torch.optim.Adam step (common/utils.py:16-76 param groups) over a flat buffer split into
 * n_seg segments [seg_off[i], seg_off[i+1]) with learning rate seg_lr[i] (n_seg <= 8).
 * If partials != NULL and max_norm > 0 the gradient is first scaled by
 * min(1, max_norm / (sqrt(sum(partials)) + 1e-6))  (clip_grad_norm_). step is 1-based. */
int nerf_adam(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_off_host,
              const double* seg_lr_host, int n_seg, double beta1, double beta2, float eps, float weight_decay,
              int step, const float* partials, float max_norm, hipStream_t stream);

/* nerf_adam with the step count read from device memory (*step_dev >= 1; the bias corrections are formed in the
 * kernel in double, as nerf_adam forms them on the host): the optimiser node of a captured train-step hipGraph. */
int nerf_adam_dstep(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_off_host,
                    const double* seg_lr_host, int n_seg, double beta1, double beta2, float eps, float weight_decay,
                    const int64_t* step_dev, const float* partials, float max_norm, hipStream_t stream);

/* ------------------------------------------------------------------ Instant-NGP expert */

#define NERF_HASH_MAX_LEVELS 32

/* HashGridEncoder configuration (models/encodings.py:175-270).  resolutions[l] are the integers the
 * reference computes, floor(min_res * growth**l) in fp32 (:205-209).  interpolation: 0 Nearest,
 * 1 Linear, 2 Smoothstep (:331-361).  levels*features_per_level <= 64, features_per_level in {1,2,4,8}. */
typedef struct {
  int32_t levels;
  int32_t features_per_level;
  int32_t log2_hashmap_size;
  int32_t interpolation;
  int32_t resolutions[NERF_HASH_MAX_LEVELS];
} NerfHashGrid;

/* HashGridEncoder._torch_forward (models/encodings.py:313-381) with _hash/_gather (:288-311): table
 * (levels * 2^log2 , F) fp32.  Positions x (M rows, pitch x_stride floats, first 3 used).  If aabb (HOST
 * pointer, 6 floats: min xyz, max xyz — part of the expert's configuration) is non-NULL the positions are world coordinates mapped as
 * MetaNGP._world_to_unit (models/inr/meta_ngp.py:166-169): clamp((x-min)/extent, eps, 1-eps); else x is
 * used as given.  out (M rows, pitch out_stride >= levels*F): cols [0, L*F) = [level0 f0..fF-1, level1 ...],
 * cols [L*F, out_stride) zero. */
int nerf_hash_encode(const NerfHashGrid* grid, const float* table, const float* x, int64_t x_stride, int64_t M,
                     const float* aabb, float enc_eps, float* out, int out_stride, hipStream_t stream);

/* Backward of nerf_hash_encode w.r.t. the table (autograd of the reference's gather + trilinear blend):
 * d_table += scatter of d_out (M rows, pitch d_stride).  Accumulates with fp32 atomics (the caller zeroes
 * d_table first); the order of the additions is not deterministic. */
int nerf_hash_encode_bwd(const NerfHashGrid* grid, const float* x, int64_t x_stride, int64_t M, const float* aabb,
                         float enc_eps, const float* d_out, int d_stride, float* d_table, hipStream_t stream);

/* Backward of nerf_hash_encode w.r.t. the POSITION: what autograd gives for HashGridEncoder._torch_forward
 * (models/encodings.py:313-381) and, with aabb, MetaNGP._world_to_unit (models/inr/meta_ngp.py:166-169).
 * d_x[m][0..2] = sum over levels (ascending) and features (ascending) of d_out[m][l*F+f] * d enc[l*F+f] / d x; it is
 * overwritten, columns >= 3 of a wider pitch dx_stride are left untouched.  Cells and weights are the forward's
 * (same fp32 operations).  Linear (:362-381): resolution times the corner difference along the axis, blended by the
 * other two axes' weights; Smoothstep (:355-361): that times 6w(1-w) of the raw w on the axis, the other axes with
 * their smoothed weights; Nearest (:331-353): zeros.  With aabb, component c is divided by the extent where
 * eps <= (x-min)/extent <= 1-eps (inclusive, torch.clamp's backward) and is exactly 0 elsewhere.  No atomics: equal
 * inputs give equal bits.  M == 0 is an empty call. */
int nerf_hash_encode_bwd_x(const NerfHashGrid* grid, const float* table, const float* x, int64_t x_stride, int64_t M,
                           const float* aabb, float enc_eps, const float* d_out, int d_stride, float* d_x,
                           int64_t dx_stride, hipStream_t stream);

/* SHEncoder.forward (models/encodings.py:133-151, components :27-81): normalise (clamp 1e-9), real SH of
 * degree levels-1 (levels 1..5) -> out (M rows, pitch out_stride >= levels^2). */
int nerf_sh_encode(const float* d, int64_t d_stride, int64_t M, int levels, float* out, int out_stride,
                   hipStream_t stream);

/* MetaNGP networks (models/inr/meta_ngp.py:75-105): sigma trunk of sigma_depth ReLU layers (hidden),
 * sigma_head (1) + geo_head (geo_feat_dim), colour MLP of color_depth ReLU layers (color_hidden) on
 * cat([geo, dir-enc]) and a 3-wide output (sigmoid if use_sigmoid_rgb).  dir_encoding: 0 spherical
 * harmonics (sh_levels), 1 FrequencyEncoder(3, 4, include_input).  Every width <= 64, 1+geo <= 32. */
typedef struct {
  int32_t in_dim;
  int32_t hidden;
  int32_t sigma_depth;
  int32_t geo_feat_dim;
  int32_t color_hidden;
  int32_t color_depth;
  int32_t dir_encoding;
  int32_t sh_levels;
  int32_t use_sigmoid_rgb;
  int32_t generic_kernels; /* 0: the compile-time production-shape kernels when the shape is MetaNGP's default (the
                              fused *_enc / bwd_hash entry points need them); 1: always the plan-driven generic
                              kernels (their reference in the tests; the fused entry points return NERF_E_UNSUPPORTED) */
} NerfNgpNet;

/* Packed parameter layout: per layer (trunk 0..sd-1, head, colour 0..cd-1, out) W (Npad x Kpad) then
 * b (Npad), PyTorch (out,in) row-major, zero padded to multiples of 32; the head's rows are [sigma, geo...].
 * table (may be NULL) receives 4 int64 per tensor {offset, rows_pad, cols_pad, cols_real}; *n_tensors the
 * tensor count.  Returns the packed float count, or <0 for an unsupported configuration. */
int64_t nerf_ngp_layout(const NerfNgpNet* net, int64_t* table, int32_t* n_tensors);

/* Workspace (bytes) of nerf_ngp_bwd for M samples (per-workgroup weight-gradient slabs). */
int64_t nerf_ngp_workspace_bytes(const NerfNgpNet* net, int64_t M);

/* MetaNGP.forward after the xyz encoding (meta_ngp.py:182-255): enc (M rows, pitch enc_stride) from
 * nerf_hash_encode, directions x_d[:,3:6] (x_d (M,6)) -> rgb_sigma (M,4).  One fused kernel: all layers
 * run on fp32 MFMA with the activations in LDS. */
int nerf_ngp_fwd(const NerfNgpNet* net, const float* w, const float* enc, int enc_stride, const float* x_d,
                 int64_t M, float* rgb_sigma, hipStream_t stream);
/* MetaNGP.density (models/inr/meta_ngp.py:192-224): sigma (M) = trunc_exp of the sigma head after the trunk;
 * the colour branch is not evaluated. */
int nerf_ngp_density(const NerfNgpNet* net, const float* w, const float* enc, int enc_stride, int64_t M,
                     float* sigma, hipStream_t stream);
/* sigma from world points in ONE launch (hash-grid encoding into LDS + sigma trunk + head; bitwise the
 * nerf_hash_encode + nerf_ngp_density pair) for the production expert shape (16 x 2 hash features, 2 x 64 sigma
 * trunk, 1 + 15 head, SH degree 4 colour input — MetaNGP's defaults); NERF_E_UNSUPPORTED for other shapes. */
/* the expert's forward in ONE launch for the production shape: hash encoding of x_d's positions into LDS (also
 * written to enc [M][enc_stride] for nerf_ngp_bwd, bitwise nerf_hash_encode's) + the fused MLP -> rgb_sigma (bitwise
 * nerf_ngp_fwd's); NERF_E_UNSUPPORTED for other shapes. */
int nerf_ngp_fwd_enc(const NerfNgpNet* net, const NerfHashGrid* grid, const float* table, const float* w,
                     const float* x_d, int64_t M, const float* aabb, float enc_eps, float* enc, int enc_stride,
                     float* rgb_sigma, hipStream_t stream);
int nerf_ngp_density_enc(const NerfNgpNet* net, const NerfHashGrid* grid, const float* table, const float* w,
                         const float* x, int64_t x_stride, int64_t M, const float* aabb, float enc_eps, float* sigma,
                         hipStream_t stream);

/* sigma AND its spatial gradient at world points in ONE launch for the shapes nerf_ngp_density_enc supports
 * (NERF_E_UNSUPPORTED otherwise, answered before any buffer is looked at): autograd of MetaNGP.density
 * (models/inr/meta_ngp.py:203-239) w.r.t. x, through trunc_exp's backward exp(clamp(raw)) (models/trunc_exp.py:54-57),
 * the sigma head and trunk (ReLU masks of the forward) and the encoding's Jacobian (nerf_hash_encode_bwd_x).
 * sigma (M) is bitwise nerf_ngp_density_enc's; grad (M rows, pitch grad_stride >= 3): columns 0..2 = d sigma / d x,
 * further columns untouched.  ws (16-byte aligned, nerf_ngp_density_grad_workspace_bytes(net) bytes) receives the
 * transposed trunk weights in a small launch of its own ahead of the kernel. */
int64_t nerf_ngp_density_grad_workspace_bytes(const NerfNgpNet* net);
int nerf_ngp_density_grad_enc(const NerfNgpNet* net, const NerfHashGrid* grid, const float* table, const float* w,
                              const float* x, int64_t x_stride, int64_t M, const float* aabb, float enc_eps,
                              float* sigma, float* grad, int64_t grad_stride, void* ws, int64_t ws_bytes,
                              hipStream_t stream);

/* Backward of nerf_ngp_fwd (recomputes the forward on chip): d_enc (M rows, pitch enc_stride; cols
 * >= in_dim untouched) and d_w (packed layout; overwritten, or accumulated into if accumulate != 0). */
int nerf_ngp_bwd(const NerfNgpNet* net, const float* w, const float* enc, int enc_stride, const float* x_d,
                 int64_t M, const float* d_rgb_sigma, float* d_enc, float* d_w, int accumulate, void* ws,
                 int64_t ws_bytes, hipStream_t stream);
/* nerf_ngp_bwd + nerf_hash_encode_bwd(d_table += ...) in ONE launch for the production expert shape with a
 * Linear / Smoothstep F = 2 grid (d_enc never leaves the chip; the table scatter runs beside the MLP backward);
 * NERF_E_UNSUPPORTED otherwise.  d_table accumulates (atomics), d_w as nerf_ngp_bwd. */
int nerf_ngp_bwd_hash(const NerfNgpNet* net, const NerfHashGrid* grid, const float* w, const float* enc,
                      int enc_stride, const float* x_d, int64_t M, const float* d_rgb_sigma, const float* aabb,
                      float enc_eps, float* d_table, float* d_w, int accumulate, void* ws, int64_t ws_bytes,
                      hipStream_t stream);

/* Device-sized forms (the container's sync-free train step, meta_container.py:275-343 with the sizes never read on
 * the host): every buffer is sized for `cap` rows and the row count is read on the device from rng (int32 pair,
 * device): rows = min(rng[1] - rng[0], cap).  The grids cover the capacity; workgroups past the count exit.
 *   _fwd_enc_n / _bwd_hash_n: rows 0 .. rows - 1 of x_d / enc / rgb_sigma / d_rgb_sigma (an expert's gathered samples,
 *                             rng = that expert's dispatch offsets); ws sized by nerf_ngp_workspace_bytes(net, cap)
 *   _density_enc_rng:         rows rng[0] .. rng[1] - 1 of x and sigma (one expert's slice of a packed march) */
int nerf_ngp_fwd_enc_n(const NerfNgpNet* net, const NerfHashGrid* grid, const float* table, const float* w,
                       const float* x_d, int64_t cap, const int32_t* rng, const float* aabb, float enc_eps, float* enc,
                       int enc_stride, float* rgb_sigma, hipStream_t stream);
int nerf_ngp_density_enc_rng(const NerfNgpNet* net, const NerfHashGrid* grid, const float* table, const float* w,
                             const float* x, int64_t x_stride, int64_t cap, const int32_t* rng, const float* aabb,
                             float enc_eps, float* sigma, hipStream_t stream);
int nerf_ngp_bwd_hash_n(const NerfNgpNet* net, const NerfHashGrid* grid, const float* w, const float* enc,
                        int enc_stride, const float* x_d, int64_t cap, const int32_t* rng, const float* d_rgb_sigma,
                        const float* aabb, float enc_eps, float* d_table, float* d_w, int accumulate, void* ws,
                        int64_t ws_bytes, hipStream_t stream);

/* ------------------------------------------------------------------ MoE container */

/* MetaContainer._routing (models/inr/meta_container.py:97-134): distances of x[:, :3] (rows of pitch
 * x_stride) to K <= 32 centroids (HOST array K x 3) on (y,z) if cluster_2d else (x,y,z).  boundary_margin
 * > 1: soft inverse-distance weights of the experts within margin x the nearest distance; else one-hot
 * argmin.  weights (M, K) fp32. */
int nerf_moe_route(const float* x, int64_t x_stride, int64_t M, const float* centroids, int K, int cluster_2d,
                   float boundary_margin, float* weights, hipStream_t stream);
/* nerf_moe_route over `capacity` rows of which the first *m_dev (device int32) are real: rows past it get all-zero
 * weights (no expert), so a following nerf_moe_dispatch over the capacity needs no host read of the count. */
int nerf_moe_route_n(const float* x, int64_t x_stride, int64_t capacity, const int32_t* m_dev, const float* centroids,
                     int K, int cluster_2d, float boundary_margin, float* weights, hipStream_t stream);

/* Order-preserving per-expert dispatch (the `(w[:,k] > 0).nonzero()` of meta_container.py:288-296):
 * idx (up to M*K int32) receives the rows with weights[m][k] > eps, expert-major and ascending within an
 * expert; offsets (K+1 int32, device) the exclusive expert offsets.  ws: nerf_moe_dispatch_workspace_bytes. */
int64_t nerf_moe_dispatch_workspace_bytes(int64_t M, int K);
int nerf_moe_dispatch(const float* weights, int64_t M, int K, float eps, int32_t* offsets, int32_t* idx, void* ws,
                      int64_t ws_bytes, hipStream_t stream);

/* dst[i][c] = src[idx[i]][c], c < cols (the expert's x.index_select rows). */
int nerf_gather_rows(const float* src, int64_t src_stride, const int32_t* idx, int64_t n, int cols, float* dst,
                     int64_t dst_stride, hipStream_t stream);
/* Device-sized forms (see nerf_ngp_fwd_enc_n): dispatch over `cap` rows of which the first *m_dev are real; gather
 * of idx entries rng[0] .. rng[1] - 1 (rng = an expert's device offsets) into dst rows 0 .. */
int nerf_moe_dispatch_n(const float* weights, int64_t cap, const int32_t* m_dev, int K, float eps, int32_t* offsets,
                        int32_t* idx, void* ws, int64_t ws_bytes, hipStream_t stream);
int nerf_gather_rows_rng(const float* src, int64_t src_stride, const int32_t* idx, const int32_t* rng, int64_t cap,
                         int cols, float* dst, int64_t dst_stride, hipStream_t stream);

/* The mix of expert k (meta_container.py:304-318): out[idx[i]][c] += y[i][c] * weights[idx[i]][k] for the
 * n rows of the expert (rows unique within a call; call k = 0..K-1 in order for the reference's sum order;
 * one-hot weights reproduce index_copy_).  Backward: d_y[i][c] = d_out[idx[i]][c] * weights[idx[i]][k]. */
int nerf_moe_combine(const float* y, int64_t n, int C, const int32_t* idx, const float* weights, int K, int k,
                     float* out, hipStream_t stream);
int nerf_moe_combine_bwd(const float* d_out, int64_t n, int C, const int32_t* idx, const float* weights, int K,
                         int k, float* d_y, hipStream_t stream);

/* MetaContainer.background_color (meta_container.py:334-363, bg_encoding "spherical"): F.normalize(d),
 * SHEncoder(levels=4), Linear(16,H)-ReLU-Linear(H,3)-Sigmoid, H <= 64.  w packed [W1 (H,16) | b1 (H) |
 * W2 (3,H) | b2 (3)] (PyTorch layouts).  Backward: d_w (20H+3 floats, overwritten) from d_out (N,3);
 * per-workgroup slabs + deterministic reduce. */
int nerf_bg_mlp_fwd(const float* d, int64_t d_stride, int64_t N, const float* w, int H, float* out,
                    hipStream_t stream);
int64_t nerf_bg_mlp_workspace_bytes(int64_t N, int H);
int nerf_bg_mlp_bwd(const float* d, int64_t d_stride, int64_t N, const float* w, int H, const float* d_out,
                    float* d_w, void* ws, int64_t ws_bytes, hipStream_t stream);

/* ------------------------------------------------------------------ occupancy rendering */
/* nerfacc 0.5.3 pieces the reference calls (nerfs/ray_rendering.py:349-558, models/inr/meta_ngp.py:108-145,
 * 318-443), rebuilt from the published algorithms (oracle/occ_oracle.py; nerfacc's source is not in the
 * image: PARITY UNPINNED).  Grid: levels x R^3 cells, id = l*R^3 + (ix*R + iy)*R + iz; level l covers the
 * ROI box scaled by 2^l about its centre.  Packed samples are ray-major with offsets[N+1]. */
typedef struct {
  int32_t levels;
  int32_t resolution;
  float roi[6];
} NerfOccGrid;

/* OccGridEstimator.sampling marching: per ray, t from max(near_plane, rays[:,6]) (+ u*step when stratified;
 * u (N) or the counter RNG) to min(far_plane, rays[:,7]) clipped to the outermost level; dt =
 * clamp(t*cone_angle, step, 1e10); [t, t+dt) is emitted when the cell of its midpoint is occupied, empty
 * cells are skipped on the dt lattice.  Count pass (offsets == NULL): counts[N].  Write pass: offsets (N+1)
 * from nerf_exclusive_scan_i32(counts) -> ray_idx / t0 / t1. */
int nerf_occ_march(const NerfOccGrid* grid, const uint8_t* binaries, const float* rays, int64_t N, float near_plane,
                   float far_plane, float step, float cone_angle, int stratified, const float* u, uint64_t seed,
                   int max_steps, int32_t* counts, const int32_t* offsets, int32_t* ray_idx, float* t0, float* t1,
                   hipStream_t stream);

/* nerf_occ_march for every expert of a container in one launch (render_rays_occ, nerfs/ray_rendering.py:397-422):
 * ray r is marched through expert k's grid only when it hits boxes[6k..6k+5] (_intersect_rays_aabb, :171-190).
 * grids (K), binaries (K device pointers), boxes (K x 6), steps (K): HOST arrays; K <= 8.  Count pass:
 * counts[k*N + r]; write pass: offsets (K*N+1, exclusive scan of counts) -> ray_idx (= r) / t0 / t1, so expert
 * k's samples are the contiguous range [offsets[k*N], offsets[(k+1)*N]).  Jitter: counter RNG (seed, k, r). */
int nerf_occ_march_multi(const NerfOccGrid* grids, const uint8_t* const* binaries, const float* boxes,
                         const float* steps, int K, const float* rays, int64_t N, float near_plane, float far_plane,
                         float cone_angle, int stratified, uint64_t seed, int max_steps, int32_t* counts,
                         const int32_t* offsets, int32_t* ray_idx, float* t0, float* t1, hipStream_t stream);

/* nerf_occ_march_multi with the write pass replaced by a copy.  Count pass (offsets == NULL): counts as above, and
 * the first `cap` segments [t0, t1] of pair j = k*N + r are kept in stage (K*N*cap float pairs, 8-byte aligned).
 * Emit pass (offsets given, same arguments and seed): pairs with counts[j] <= cap are copied from stage, longer
 * pairs are marched again; the output equals nerf_occ_march_multi's write pass exactly. */
int nerf_occ_march_multi_staged(const NerfOccGrid* grids, const uint8_t* const* binaries, const float* boxes,
                                const float* steps, int K, const float* rays, int64_t N, float near_plane,
                                float far_plane, float cone_angle, int stratified, uint64_t seed, int max_steps,
                                int32_t* counts, float* stage, int cap, const int32_t* offsets, int32_t* ray_idx,
                                float* t0, float* t1, hipStream_t stream);

/* nerf_occ_march_multi_staged with the jitter seed seed + (*step_dev) * seed_mul read on the device (captured
 * train-step graphs: one marching jitter stream per replay). */
int nerf_occ_march_multi_staged_dseed(const NerfOccGrid* grids, const uint8_t* const* binaries, const float* boxes,
                                      const float* steps, int K, const float* rays, int64_t N, float near_plane,
                                      float far_plane, float cone_angle, int stratified, uint64_t seed, int max_steps,
                                      int32_t* counts, float* stage, int cap, const int32_t* offsets,
                                      int32_t* ray_idx, float* t0, float* t1, const int64_t* step_dev,
                                      uint64_t seed_mul, hipStream_t stream);

/* Exclusive scan of n int32 into out[n+1] (out[n] = total); in / out 16-byte aligned. Reduce-then-scan over
 * 2048-element tiles: 3 launches, 12 B of HBM traffic per element. */
int64_t nerf_scan_workspace_bytes(int64_t n);
int nerf_exclusive_scan_i32(const int32_t* in, int64_t n, int32_t* out, void* ws, int64_t ws_bytes,
                            hipStream_t stream);

/* render_weight_from_density + accumulate_along_rays (+ background): w_i = exp(-sum_{j<i} s_j) (1-exp(-s_i)),
 * s = sigma (t1 - t0); rgb = sum w c + (1-acc) bg, depth = sum w (t0+t1)/2, acc = sum w.  rgb_sigma (M,4). */
int nerf_packed_composite_fwd(const float* rgb_sigma, const float* t0, const float* t1, const int32_t* offsets,
                              int64_t N, const float* bg, float* rgb, float* depth, float* acc, float* weights,
                              hipStream_t stream);
/* Backward: g_rgb (N,3) required; g_depth, g_acc (N), g_weights (M) nullable -> d_rgb_sigma (M,4). */
int nerf_packed_composite_bwd(const float* rgb_sigma, const float* t0, const float* t1, const int32_t* offsets,
                              int64_t N, const float* bg, const float* g_rgb, const float* g_depth, const float* g_acc,
                              const float* g_weights, float* d_rgb_sigma, hipStream_t stream);

/* render_visibility_from_density: keep[j] = T_j >= early_stop_eps && (alpha_thre <= 0 || alpha_j >= alpha_thre). */
/* nerf_packed_visibility over n_seg segments in groups of `group` consecutive segments (one group per expert of
 * a multi-expert march): segment s uses min(alpha_thre, alpha_groups[s / group]) (alpha_groups: device). */
int nerf_packed_visibility_groups(const float* t0, const float* t1, const float* sigmas, const int32_t* offsets,
                                  int64_t n_seg, int64_t group, float early_stop_eps, float alpha_thre,
                                  const float* alpha_groups, int32_t* keep, hipStream_t stream);
int nerf_packed_visibility(const float* t0, const float* t1, const float* sigmas, const int32_t* offsets, int64_t N,
                           float early_stop_eps, float alpha_thre, int32_t* keep, hipStream_t stream);
/* Compaction of the kept samples (pos = exclusive scan of keep); counts_out (N, zeroed by the caller, or NULL)
 * receives the per-ray kept counts. */
int nerf_packed_compact(const int32_t* keep, const int32_t* pos, int64_t M, const int32_t* ray_idx, const float* t0,
                        const float* t1, int32_t* ray_idx_out, float* t0_out, float* t1_out, int32_t* counts_out,
                        hipStream_t stream);

/* OccGridEstimator update: jittered points of the given cells (n,3); EMA update occs[c] = max(occs[c]*decay,
 * value) for visible cells; threshold thre[0] = min(mean(occs >= 0), occ_thre), thre[1] = mean(occs)
 * (device, no host sync); binaries = occs > thre[0]. */
int nerf_occ_cell_points(const NerfOccGrid* grid, const int32_t* cells, int64_t n, uint64_t seed, float* x,
                         hipStream_t stream);
int nerf_occ_update(float* occs, const int32_t* cells, const float* values, int64_t n, float ema_decay,
                    hipStream_t stream);
/* The cell draw of OccGridEstimator._update after warm-up (nerfacc _sample_uniform_and_occupied_cells) with no
 * host read: occ_list / pos = nerf_flag_compact / exclusive scan of the binaries (levels x cells_per_level) as
 * int32 flags.  Per level: n uniform cells, then every occupied cell if there are <= n of them (other slots
 * -1), else n draws with replacement.  cells: levels x 2n global ids; cell_points / update skip ids < 0. */
int nerf_occ_sample_cells(const int32_t* occ_list, const int32_t* pos, int levels, int64_t cells_per_level,
                          int64_t n, uint64_t seed, int32_t* cells, hipStream_t stream);
int nerf_occ_threshold(const float* occs, int64_t n, float occ_thre, float* thre_out, hipStream_t stream);
/* thre_out must hold nerf_occ_threshold_floats() floats (2 results + 16-B pad + fp64 block partials). */
int64_t nerf_occ_threshold_floats(void);
int nerf_occ_binarize(const float* occs, int64_t n, const float* thre, uint8_t* binaries, hipStream_t stream);

/* OccGridEstimator.mark_invisible_cells: cells whose centre no camera sees (K (n_cam,3,3), c2w (n_cam,3,4) RDF,
 * depth > near_plane, inside W x H) get occs = -1. */
int nerf_occ_mark_invisible(const NerfOccGrid* grid, const float* K, const float* c2w, int n_cam, int W, int H,
                            float near_plane, float* occs, hipStream_t stream);

/* nerfacc.pack_info: per-ray sample counts of a packed ray_idx (M) -> counts (N, zeroed here). */
int nerf_ray_counts(const int32_t* ray_idx, int64_t M, int64_t N, int32_t* counts, hipStream_t stream);
/* Sample points of packed intervals (render_expert_occ, ray_rendering.py:523-525): x_d[j] = [o + d t_mid, d]. */
int nerf_packed_points(const float* rays, const int32_t* ray_idx, const float* t0, const float* t1, int64_t M,
                       float* x_d, hipStream_t stream);
/* nerf_packed_points for the first *m_dev (device int32) of `capacity` rows; the rest are left untouched. */
int nerf_packed_points_n(const float* rays, const int32_t* ray_idx, const float* t0, const float* t1,
                         int64_t capacity, const int32_t* m_dev, float* x_d, hipStream_t stream);

/* Full-container occupancy rendering (render_rays_occ, nerfs/ray_rendering.py:384-481).
 * nerf_rays_aabb_hit: _intersect_rays_aabb (:171-190) of rays (N,8) with box (HOST, 6 floats) -> hit (N) int32.
 * nerf_flag_compact: idx[pos[i]] = i for flags[i] != 0 (pos = exclusive scan of flags).
 * nerf_scatter_counts: counts[hit_idx[i]] = counts_k[i] (an expert's per-ray counts on the global rays).
 * nerf_segments_union: _merge_segments_union (:193-258): per ray, the sorted distinct union of every expert's
 *   t0 and t1 boundaries (t0s / t1s / offs: HOST arrays of K <= 8 device pointers; offs[k] (N+1) per-expert
 *   offsets over the global rays) -> the segments between consecutive boundaries.  Count pass (out_off NULL)
 *   -> counts (N); write pass -> ray_idx / t0 / t1 at out_off.
 * nerf_moe_blend / _finish / _bwd: sigma and rgb blended BEFORE integration (:441-471): s += w_k sigma_k,
 *   c += (w_k sigma_k) rgb_k over the rows expert k evaluated (call in expert order), then
 *   rgb_sigma = [c / max(s, 1e-12), max(s, 1e-12)]; backward per expert -> d_y (n,4). */
int nerf_rays_aabb_hit(const float* rays, int64_t N, const float* box, int32_t* hit, hipStream_t stream);
int nerf_flag_compact(const int32_t* flags, const int32_t* pos, int64_t n, int32_t* idx, hipStream_t stream);
int nerf_scatter_counts(const int32_t* hit_idx, const int32_t* counts_k, int64_t n, int32_t* counts, hipStream_t stream);
int nerf_segments_union(const float* const* t0s, const float* const* t1s, const int32_t* const* offs, int K, int64_t N,
                        int32_t* counts, const int32_t* out_off, int32_t* ray_idx, float* t0, float* t1,
                        hipStream_t stream);
int nerf_moe_blend(const float* y, int64_t n, const int32_t* idx, const float* weights, int K, int k, float* s_acc,
                   float* c_acc, hipStream_t stream);
int nerf_moe_blend_finish(const float* s_acc, const float* c_acc, int64_t M, float* rgb_sigma, hipStream_t stream);
int nerf_moe_blend_bwd(const float* y, int64_t n, const int32_t* idx, const float* weights, int K, int k,
                       const float* s_acc, const float* rgb_sigma, const float* d_rgb_sigma, float* d_y,
                       hipStream_t stream);
/* Device-sized blend (see nerf_ngp_fwd_enc_n): y / d_y rows 0 .. rng[1] - rng[0] - 1 pair with idx entries rng[0] ..;
 * _finish_n over `cap` rows of which the first *m_dev are real. */
int nerf_moe_blend_rng(const float* y, int64_t cap, const int32_t* idx, const int32_t* rng, const float* weights, int K,
                       int k, float* s_acc, float* c_acc, hipStream_t stream);
int nerf_moe_blend_finish_n(const float* s_acc, const float* c_acc, int64_t cap, const int32_t* m_dev, float* rgb_sigma,
                            hipStream_t stream);
int nerf_moe_blend_bwd_rng(const float* y, int64_t cap, const int32_t* idx, const int32_t* rng, const float* weights,
                           int K, int k, const float* s_acc, const float* rgb_sigma, const float* d_rgb_sigma,
                           float* d_y, hipStream_t stream);

/* ------------------------------------------------------------------ meta-learning updates (§8f row 4) */

/* task_adapt's inner update (adaptive_nerf/pipelines/offline_stage/meta_core.py:61-64):
 * out_i = w_i - lr * g_i (two rounded fp32 ops, like torch) for up to 64 fast tensors in one launch.
 * w / g / out / numel are HOST arrays; g[i] NULL -> out_i = w_i (a parameter autograd left unused). */
int nerf_sgd_multi(int n_tensors, const float* const* w, const float* const* g, float* const* out,
                   const int64_t* numel, float lr, hipStream_t stream);

/* reptile_meta_update (meta_core.py:145-176): per tensor t, delta = (sum_f (fast[t*n_fast+f] - theta_t)) / n_fast
 * (summed in fast-list order) and theta_t += lr * delta, skipped when delta has a non-finite element or is all
 * zero (the reference's per-tensor guard). theta / fast / numel are HOST arrays of device pointers / sizes;
 * flags: device int32 workspace of nerf_reptile_workspace_bytes(n_tensors) bytes. */
int64_t nerf_reptile_workspace_bytes(int n_tensors);
int nerf_reptile_update(int n_tensors, float* const* theta, const float* const* fast, int n_fast,
                        const int64_t* numel, float lr, int32_t* flags, int64_t ws_bytes, hipStream_t stream);

/* ------------------------------------------------------------------ ray dataset build (§8f row 4) */

/* _process_single_image (adaptive_nerf/data/ram_rays_dataset.py:46-121) for n_images same-size (H x W) images in
 * two passes around nerf_exclusive_scan_i32 (n = n_images*H*W pixels, image-major, row-major):
 *   count pass (pos == NULL): flags[n] = keep-mask (:97-104; masks NULL = keep all) && valid after
 *     get_rays with the AABB near/far (:88-92, max_bound = invalid = 1e10) and clamp_rays_near_far (:104-106,
 *     has_near / has_far = the override; eps 1e-6, invalid -> inf);
 *   write pass (pos = exclusive scan of flags, n+1 entries): kept pixel g -> row pos[g] of out_rays (8 floats,
 *     16-byte aligned), out_rgb (3 floats, pixel / 255, :112) and out_idx (image_index[image of g], :117).
 * c2w (n_images x 12), intrinsics (n_images x 4: fx fy cx cy), image_index (n_images), aabb (6): device.
 * n_images * H * W < 2^31 (int32 row positions; RamRaysDataset builds runs of <= 2^26 pixels). */
int nerf_dataset_rays(const float* c2w, const float* intrinsics, const int32_t* image_index, int n_images, int H,
                      int W, int center_pixels, const float* aabb, int has_near, float near_v, int has_far,
                      float far_v, const uint8_t* images, const uint8_t* masks, int32_t* flags, const int32_t* pos,
                      float* out_rays, float* out_rgb, int32_t* out_idx, hipStream_t stream);

/* ------------------------------------------------------------------ mesh extraction */

/* Marching tetrahedra over the Kuhn split of a lattice of densities: field (nx,ny,nz) contiguous fp32, linear index
 * p = (ix ny + iy) nz + iz, every dimension >= 2 and 12 nx ny nz < 2^31 (else NERF_E_ARG); a point is inside iff
 * field > iso (the field must be finite; the kernels do not check).  Point p owns the edges to p + d, d = 1..7
 * (bit 0 = +x, bit 1 = +y, bit 2 = +z) that stay inside the lattice.
 * nerf_mesh_classify: edge_mask[p] = crossing bits of the owned edges (bit d-1), vert_count[p] = their number,
 *   face_count[p] = triangles (0..12) of the cell whose low corner is p (0 on a high border).
 * nerf_mesh_emit: vert_off / face_off = nerf_exclusive_scan_i32 of the two counts, V / F their totals.  Writes the
 *   vertices lo + (i + t d) h, h = (hi - lo) / (n - 1), t = (f[p] - iso) / (f[p] - f[q]), ordered by (p, d); the
 *   triangles (int32 vertex indices, normals towards lower density) ordered by (cell, tetrahedron, triangle); and,
 *   when normals != NULL, -g / max(|g|, 1e-12) of the lattice's central-difference gradient (one-sided on the
 *   border) interpolated along the edge.  lo / hi: HOST arrays of 3 floats, lo < hi.  V = F = 0 launches nothing.
 *   No atomics: equal inputs give equal bits.  Zero-area triangles (a lattice value equal to iso) are kept. */
int nerf_mesh_classify(const float* field, int nx, int ny, int nz, float iso, uint8_t* edge_mask,
                       int32_t* vert_count, int32_t* face_count, hipStream_t stream);
int nerf_mesh_emit(const float* field, int nx, int ny, int nz, float iso, const float* lo, const float* hi,
                   const uint8_t* edge_mask, const int32_t* vert_off, const int32_t* face_off, int64_t V, int64_t F,
                   float* verts, int32_t* faces, float* normals, hipStream_t stream);

/* Dual contouring over the same lattice: field, the index p, inside iff field > iso, lo / hi (HOST
 * arrays of 3 floats, lo < hi) and the bound 12 nx ny nz < 2^31 are those of nerf_mesh_classify / nerf_mesh_emit (else
 * NERF_E_ARG; the field must be finite, the kernels do not check).  Point p owns the axis edges p -> p + e_a,
 * a = 0,1,2, that stay inside the lattice; cell p is the cell whose low corner is p (none on a high border).
 * nerf_mesh_dual_classify: edge_mask[p] = crossing bits of the owned edges (bit a), edge_count[p] = their number,
 *   cell_flag[p] = 1 iff cell p exists and its 8 inside bits are mixed (an active cell: one vertex), face_count[p] =
 *   2 x the interior crossing edges of p, an edge along a being interior iff 1 <= j_b <= n_b - 2 and
 *   1 <= j_c <= n_c - 2 for the two other axes, so that its four cells exist (they are then active).
 * edge_off / cell_off / face_off = nerf_exclusive_scan_i32 of the three counts (nx ny nz + 1 entries each), E / V / F
 *   their totals.  Edge (p, a) has the index edge_off[p] + popcount(edge_mask[p] & ((1 << a) - 1)).
 * nerf_mesh_dual_edges: the Hermite data of every crossing edge, ordered by (p, a).  points (E,3) = the vertex
 *   nerf_mesh_emit puts on that edge, bit for bit; normals (E,3) or NULL = its grid normal -g / max(|g|, 1e-12);
 *   keys (E) or NULL = 3 p + a.  E = 0 launches nothing.
 * nerf_mesh_dual_cells: one vertex per active cell and two triangles per interior crossing edge.  points / normals are
 *   plain inputs, (E,3) in the order above: the caller may replace what nerf_mesh_dual_edges wrote.
 *   Vertex cell_off[p]: the cell's 12 edges in the order a = 0,1,2, (b,c) = ((a+1)%3, (a+2)%3), corner offsets
 *   (ob,oc) = (0,0),(1,0),(0,1),(1,1) (owner p + ob e_b + oc e_c).  Every crossing edge's point goes to the cell's
 *   centred coordinates in double, y_k = (x_k - pa_k) / h_k - 0.5 with pa_k = lo_k + (float)i_k h_k in fp32; xbar is
 *   their sum in that order over their number.  placement 0 (mean, surface nets): x = xbar.  placement 1 (QEF): every
 *   crossing edge adds the plane through y with the direction m_k = n_k h_k (covariant, so anisotropic spacing is
 *   right; |m| == 0 adds nothing), unit weight; x = the minimiser closest to xbar along the eigen-directions above
 *   tol x the largest eigenvalue (8 cyclic Jacobi sweeps, the solve of nerf_mesh_cluster_quadric); where it is not
 *   finite or leaves [-0.5, 0.5]^3, x = xbar and fallback[v] = 1 (else 0; always 0 for placement 0).
 *   verts[v] = pa_k + (float)(x_k + 0.5) h_k: a vertex stays in its cell.  vertex_normals (V,3) or NULL: the double
 *   sum s of the cell's edge normals in order, (float)(s / max(|s|, 1e-12)).  fallback (V) uint8 or NULL.
 *   Faces [face_off[p], face_off[p+1]): for a = 0,1,2, an interior crossing edge (p, a) gives the quad over the cells
 *   k0 = p - e_b - e_c, k1 = p - e_c, k2 = p, k3 = p - e_b (counter-clockwise seen from +a), kept when p is inside (so
 *   normals point towards lower values, as nerf_mesh_emit's do) and reversed to k0 k3 k2 k1 otherwise, split on the
 *   fixed diagonal: (v0,v1,v2), (v0,v2,v3).  A crossing edge on the border of the box gives Hermite data but no quad:
 *   the surface is open at the box.  A cell that two sheets cross still gets one vertex, so a noisy field can give
 *   edges shared by more than two triangles.
 *   normals must not be NULL for placement 1 or with vertex_normals; 0 < tol < 1 (else NERF_E_ARG); an unknown
 *   placement, V > nx ny nz, F > 6 nx ny nz or F > 0 with V = 0: NERF_E_ARG.  V = 0 launches nothing.
 * One thread per lattice point, no LDS, no atomics, one writer per output slot: equal inputs give equal bits. */
int nerf_mesh_dual_classify(const float* field, int nx, int ny, int nz, float iso, uint8_t* edge_mask,
                            int32_t* edge_count, int32_t* cell_flag, int32_t* face_count, hipStream_t stream);
int nerf_mesh_dual_edges(const float* field, int nx, int ny, int nz, float iso, const float* lo, const float* hi,
                         const uint8_t* edge_mask, const int32_t* edge_off, int64_t E, float* points, float* normals,
                         int32_t* keys, hipStream_t stream);
int nerf_mesh_dual_cells(const float* field, int nx, int ny, int nz, float iso, const float* lo, const float* hi,
                         const uint8_t* edge_mask, const int32_t* edge_off, const int32_t* cell_off,
                         const int32_t* face_off, const float* points, const float* normals, int placement, double tol,
                         int64_t V, int64_t F, float* verts, int32_t* faces, float* vertex_normals, uint8_t* fallback,
                         hipStream_t stream);

/* Mesh clean-up.  faces (F,3) int32 with 0 <= index < V: ANY indexed triangle list (any vertex
 * order, duplicated faces, repeated indices, unused vertices).  The kernels do not check the indices; the caller does.
 * V < 2^31 and 3 F < 2^31 (else NERF_E_ARG).
 * nerf_mesh_components: labels[v] = the smallest vertex index of v's connected component (two vertices are connected
 *   iff a chain of faces joins them; an unused vertex is its own component) and face_count[l] = the faces of the
 *   component labelled l (0 where l is no label); both (V) int32.  A lock-free union-find over labels itself
 *   (parent[v] <= v at every instant), a flatten and a count: 4 launches, integer atomics only.  The outputs are a
 *   function of the input alone, so equal inputs give equal bits.  status: 2 device int32; after the call status[0] != 0
 *   iff a thread exhausted a loop bound (the outputs are then invalid) and status[1] = the most find steps one face
 *   took.  F = 0 launches only the initialisation, V = 0 nothing.
 * nerf_mesh_mark_used: keep32[f] = keep[f] != 0 (labels == NULL, keep (F) bytes) or keep[labels[faces[f][0]]] != 0
 *   (keep (V) bytes, a flag per component label), and used[v] = 1 for every vertex of a kept face (used (V) int32,
 *   zeroed by the caller).
 * nerf_mesh_remap_faces: face_pos / vert_pos = nerf_exclusive_scan_i32 of keep32 / used, F_out the first total; kept
 *   face f -> out row face_pos[f] = vert_pos of its three indices.  Kept faces and used vertices keep their order;
 *   the vertex rows follow by nerf_flag_compact(used, vert_pos) and nerf_gather_rows. */
int nerf_mesh_components(const int32_t* faces, int64_t F, int64_t V, int32_t* labels, int32_t* face_count,
                         int32_t* status, hipStream_t stream);
int nerf_mesh_mark_used(const int32_t* faces, const uint8_t* keep, const int32_t* labels, int64_t F, int64_t V,
                        int32_t* keep32, int32_t* used, hipStream_t stream);
int nerf_mesh_remap_faces(const int32_t* faces, const int32_t* keep32, const int32_t* face_pos, const int32_t* vert_pos,
                          int64_t F, int64_t F_out, int32_t* out, hipStream_t stream);

/* Mesh simplification by vertex clustering.  The vertices are snapped to a uniform grid of cells
 * lo + (ix,iy,iz) cell, dims = (nx,ny,nz) cells with every entry in [1, 2^20]; every occupied cell becomes one vertex.
 * lo (3 floats) and dims (3 int32) are HOST arrays; cell > 0 and inv = 1 / cell, both fp32, the division done by the
 * caller.  Per axis t = (v - lo) * inv (one fp32 subtract, one fp32 multiply), i = clamp(floorf(t), 0, dim - 1)
 * clamped as a float, key = (ix ny + iy) nz + iz in int64: vertices outside the grid land in the border cells.  The
 * vertices must be finite (the kernels do not check).  V < 2^31 and 3 F < 2^31, table_log2 in [0, 31] and
 * 2^table_log2 > the number of items (V or F), else NERF_E_ARG; the workspace 16-byte aligned (else NERF_E_ALIGN) and
 * of at least the bytes of the matching *_workspace_bytes function (else NERF_E_WORKSPACE), all before any launch.
 * Integer atomics only, and every output is a function of the input alone, so equal inputs give equal bits.
 * status: 2 device int32; after the call status[0] != 0 iff a thread exhausted its probe bound (2^table_log2 probes;
 * the outputs are then invalid), status[1] = the longest probe chain a thread walked.
 * nerf_mesh_cluster_labels: labels[v] (V) int32 = the smallest vertex index whose key equals v's.  A key pre-pass,
 *   an insert into an open-addressing hash set of vertex indices (compare-and-swap on empty slots, atomicMin on the
 *   slot of an equal key) and a lookup: 3 launches.  Workspace: the int64 keys and the 2^table_log2 int32 slots.
 * nerf_mesh_cluster_reduce: the row of every representative (labels[v] == v) of out_vertices = the cell's corner plus
 *   the mean cell-relative position of its members in 24-bit fixed point (uint64 sums), of out_normals (normals !=
 *   NULL) = the normalised sum of the members' normals, clamped to [-1,1] and rounded to 2^-20 (int64 sums; a zero
 *   sum gives zeros), of out_colors (colors != NULL) = the mean of the members' colours, clamped to [0,1] and rounded
 *   to 2^-24; every other row zeros.  A NaN attribute counts as the lower bound of its clamp.  Init, accumulate
 *   (64-bit integer atomicAdd at the row labels[v]) and finalize (double precision, every operation rounded on its
 *   own): 3 launches.  Workspace: 3 (1 + normals + colours) uint64 and one int32 per vertex.
 * nerf_mesh_cluster_faces: faces_out (F,3) = labels[faces] (still indices into the V input rows), keep[f] (F) uint8 =
 *   1 iff the three new indices differ and f is the smallest face index among the faces with f's canonical form (the
 *   rotation with the smallest index first; the cyclic order, hence the orientation, is kept: a face and its mirror
 *   image are different forms).  A remap pass, an insert of the non-degenerate faces into a hash set of face indices
 *   keyed by the canonical triple read through the index, and a lookup: 3 launches.  faces_out must not alias faces.
 *   The result goes to nerf_mesh_mark_used / nerf_mesh_remap_faces with keep as the per-face flag.
 * nerf_mesh_cluster_quadric: the quadric-error position of every cluster in place of the mean.  faces (F,3) are the
 *   ORIGINAL faces; (row_off (V+1), col) is the vertex-to-face adjacency (nerf_mesh_pair_keys mode 1 ...
 *   nerf_mesh_csr_build) of faces_out of nerf_mesh_cluster_faces, so row r of a representative lists, ascending and
 *   once each, the original faces with a corner in cluster r; mean (V,3) is out_vertices of nerf_mesh_cluster_reduce;
 *   tol in (0, 1), else NERF_E_ARG.  In the frame of the representative's cell (centre c = lo + (i + 0.5) cell,
 *   y = (p - c) / cell, all in double, every operation rounded on its own) the row's faces are summed in the row's
 *   order into A += L m m^T, b += (L d) m with n = (b - a) x (c - a), L = |n|, m = n / L, d = -(m . a); faces with
 *   L == 0 are skipped.  8 cyclic Jacobi sweeps give the eigenpairs of A; from x = the mean's local coordinates,
 *   x += ((e_i . g) / l_i) e_i for i = 0, 1, 2 with l_i > tol max|l| and g = -b - A x.  out_position[r] =
 *   float(c + x cell) and out_placed[r] = 1 when max|l| > 0 and x is finite and inside [-0.5, 0.5]^3, else
 *   out_position[r] = mean[r] bit for bit and out_placed[r] = 0; both are zeros at the rows that are no
 *   representative.  out_position must alias neither mean nor vertices.  One thread per vertex row, one launch, no
 *   workspace, no atomics; it allocates nothing and does not synchronise. */
int64_t nerf_mesh_cluster_labels_workspace_bytes(int64_t V, int table_log2);
int nerf_mesh_cluster_labels(const float* vertices, int64_t V, const float* lo, float cell, float inv,
                             const int32_t* dims, int table_log2, void* workspace, int64_t workspace_bytes,
                             int32_t* labels, int32_t* status, hipStream_t stream);
int64_t nerf_mesh_cluster_reduce_workspace_bytes(int64_t V, int has_normals, int has_colors);
int nerf_mesh_cluster_reduce(const float* vertices, const int32_t* labels, const float* normals, const float* colors,
                             int64_t V, const float* lo, float cell, float inv, const int32_t* dims, void* workspace,
                             int64_t workspace_bytes, float* out_vertices, float* out_normals, float* out_colors,
                             hipStream_t stream);
int64_t nerf_mesh_cluster_faces_workspace_bytes(int64_t F, int table_log2);
int nerf_mesh_cluster_faces(const int32_t* faces, const int32_t* labels, int64_t F, int64_t V, int table_log2,
                            void* workspace, int64_t workspace_bytes, int32_t* faces_out, uint8_t* keep,
                            int32_t* status, hipStream_t stream);
int nerf_mesh_cluster_quadric(const float* vertices, const int32_t* faces, const int32_t* labels,
                              const int32_t* row_off, const int32_t* col, const float* mean, int64_t V, int64_t F,
                              const float* lo, float cell, float inv, const int32_t* dims, double tol,
                              float* out_position, uint8_t* out_placed, hipStream_t stream);

/* Mesh smoothing: two CSR adjacencies built from sorted int64 keys, a Jacobi smoothing pass over the
 * first and face-derived vertex normals over the second.  faces (F,3) int32 with 0 <= index < V: ANY indexed triangle
 * list, as for the clean-up; the kernels do not check the indices or the finiteness of the vertices, the caller does.
 * V < 2^31 and 6 F < 2^31 (the int32 scan of the flags), else NERF_E_ARG; the key arrays 8-byte aligned, else
 * NERF_E_ALIGN; both before any launch.  No atomics: every output is a function of the input alone, so equal inputs
 * give equal bits.  F = 0, n = 0 and V = 0 are empty calls (n = 0 with V > 0 zeroes row_off).
 * A key is ((int64)row << 32) | (uint32)entry; INT64_MAX is the sentinel of a dropped pair.
 * nerf_mesh_pair_keys: mode 0 writes the 6 F keys (a << 32) | b of the directed pairs (a,b) and (b,a) of every face's
 *   three edges, in any order that is a function of the face index; a pair with a == b becomes the sentinel.  Mode 1
 *   writes the 3 F keys (v << 32) | f of the corners.  The CALLER sorts the keys ascending (any int64 sort).
 * nerf_mesh_csr_flags: flags[i] (n) int32 = sorted_keys[i] != sentinel && (i == 0 || sorted_keys[i] !=
 *   sorted_keys[i-1]).  boundary (V) uint8, zeroed by the caller, or NULL: a plain store of 1 at the row of every
 *   run of exactly one key (mode 0: a directed pair that occurs once, i.e. an edge used by exactly one face).
 * nerf_mesh_csr_build: pos (n+1) = nerf_exclusive_scan_i32(flags), E = pos[n] read by the caller, who sizes col (E).
 *   col[pos[i]] = the low 32 bits of sorted_keys[i] where flags[i] (positions >= E are not written), and
 *   row_off[v] = pos[lower bound of v << 32 in sorted_keys] for v = 0..V (row_off (V+1), row_off[V] = E): a binary
 *   search of at most 32 steps per vertex.  Row v of the result lists, ascending and once each, the vertices u != v
 *   that share a face with v (mode 0) or the faces that contain v (mode 1); an unused vertex has an empty row.
 * nerf_mesh_smooth_pass: v_out[v] = float(q + double(s) (m - q)) per axis, q = double(v_in[v]), m = the sum of
 *   double(v_in[u]) over row v in the row's order divided by the row's length; every operation rounded on its own.
 *   An empty row, fixed[v] != 0 (fixed (V) uint8 or NULL) and s == 0 copy v_in[v] bit for bit.  A Jacobi step: v_out
 *   must not be v_in (NERF_E_ARG).  One thread per vertex.
 * nerf_mesh_vertex_normals: normals_out[v] = g / max(|g|, 1e-12) in double, rounded to fp32, g = the sum over the
 *   faces f of row v (the vertex-to-face adjacency), in the row's order, of (p[i1] - p[i0]) x (p[i2] - p[i0]) with
 *   (i0,i1,i2) = faces[f]: area-weighted, by the face's winding; a zero sum (an unused vertex, faces that cancel)
 *   gives zeros.  One thread per vertex. */
int nerf_mesh_pair_keys(const int32_t* faces, int64_t F, int mode, int64_t* keys, hipStream_t stream);
int nerf_mesh_csr_flags(const int64_t* sorted_keys, int64_t n, int32_t* flags, uint8_t* boundary, hipStream_t stream);
int nerf_mesh_csr_build(const int64_t* sorted_keys, int64_t n, const int32_t* flags, const int32_t* pos, int64_t V,
                        int64_t E, int32_t* row_off, int32_t* col, hipStream_t stream);
int nerf_mesh_smooth_pass(const float* v_in, const int32_t* row_off, const int32_t* col, const uint8_t* fixed,
                          int64_t V, float s, float* v_out, hipStream_t stream);
int nerf_mesh_vertex_normals(const float* vertices, const int32_t* faces, const int32_t* row_off, const int32_t* col,
                             int64_t V, float* normals_out, hipStream_t stream);

/* Mesh metrics: area-weighted surface samples and the exact nearest neighbour of every point of one
 * set in another, the two device stages of Chamfer / Hausdorff / F-score.  vertices (V,3) float32 finite, faces (F,3)
 * int32 with 0 <= index < V, points (.,3) float32 finite: the kernels check neither the indices nor the finiteness,
 * the caller does.  3 F, n and m below 2^31, total in (0, 2^63), every dim in [1, 1024], cell and inv finite and
 * positive, else NERF_E_ARG; the double, int64 key and cdf arrays 8-byte aligned, else NERF_E_ALIGN; both before any
 * launch.  No LDS, no atomics: every output is a function of the input alone, so equal inputs give equal bits.
 * F = 0 (areas), n = 0 and m = 0 (keys) are empty calls.  Every fp32 and fp64 operation named below rounds on its own.
 * nerf_mesh_face_areas: area[f] (F) double = 0.5 sqrt((x x + y y) + z z) of (p1 - p0) x (p2 - p0), the corners
 *   converted to double first; exactly 0 for a face with a repeated index.  One thread per face.
 * nerf_mesh_sample_surface: cdf (F) int64 = the CALLER's inclusive sum of non-negative integer face weights and
 *   total = cdf[F-1] (kernels.mesh_sample_surface: weights rint(area 2^e) with the largest in [2^31, 2^32]).  Sample
 *   i draws z_k = mix64(seed 0x9e3779b97f4a7c15 + mix64((0x6d657368 + k) 0xd1b54a32d192ed03 + i)), k = 0, 1, 2 (the
 *   64-bit value behind the project's counter RNG).  Face f = the first with cdf[f] > umulhi64(z_0, total), a binary
 *   search of at most 32 steps: a face of weight 0 is never chosen.  k1 = z_1 >> 40, k2 = z_2 >> 40, both replaced by
 *   2^24 - k when k1 + k2 > 2^24, u = k 2^-24; points[i] = float((p0 + u1 (p1 - p0)) + u2 (p2 - p0)) per axis in
 *   double, face_idx[i] = f.  normals_out (n,3) or NULL: with vertex_normals == NULL the face's cross product divided
 *   by its length, in double, rounded once; with vertex_normals (V,3) g / max(|g|, 1e-12) of
 *   g = ((1 - u1 - u2) n0 + u1 n1) + u2 n2.  vertex_normals without normals_out is NERF_E_ARG.  One thread per sample.
 * nerf_points_cell_keys: keys[j] (m) int64 = (cell_id << 32) | j, cell_id = (ix ny + iy) nz + iz < 2^30 with the fp32
 *   cell index of nerf_mesh_cluster_labels: t = (p - lo) * inv, i = clamp(floorf(t), 0, dim - 1).  lo (3 floats) and
 *   dims (3 int32) are HOST arrays, inv = 1 / cell in fp32, the division done by the caller.  The CALLER sorts the keys
 *   ascending (any int64 sort) and gathers the points in key order (nerf_gather_rows over the low words).
 * nerf_points_nearest: for every query (n,3) the nearest of the m reference points behind sorted_keys (m) and
 *   sorted_points (m,3): d2[i] = (dx dx + dy dy) + dz dz in fp32, the smallest over the points, idx[i] = the original
 *   index (the key's low word) of that point, the smallest such index on equal d2: brute force's result bit for bit.
 *   Every reference point must lie in the box [lo, lo + dims cell] (up to rounding); a query may lie anywhere.  The
 *   search walks the Chebyshev shells r = 0, 1, .. < max(dims) around the query's clamped cell, per (ix, iy) column
 *   one lower bound over the keys and a walk over the column's run, and stops before shell r >= 2 once
 *   best_d2 <= ((r - 1 - 2^-8) cell)^2 (1 - 2^-10) (the slack: mesh_metrics_core.hpp).  m = 0: d2 = +inf, idx = -1.
 *   One thread per query; queries presented in the order of their own cell keys keep a wave on the same columns. */
int nerf_mesh_face_areas(const float* vertices, const int32_t* faces, int64_t F, double* area, hipStream_t stream);
int nerf_mesh_sample_surface(const float* vertices, const int32_t* faces, int64_t F, const int64_t* cdf,
                             uint64_t total, const float* vertex_normals, int64_t n, uint64_t seed, float* points,
                             int32_t* face_idx, float* normals_out, hipStream_t stream);
int nerf_points_cell_keys(const float* points, int64_t m, const float* lo, float inv, const int32_t* dims,
                          int64_t* keys, hipStream_t stream);
int nerf_points_nearest(const float* query, int64_t n, const int64_t* sorted_keys, const float* sorted_points,
                        int64_t m, const float* lo, float cell, float inv, const int32_t* dims, float* d2,
                        int32_t* idx, hipStream_t stream);

/* Exact point-to-surface distance: the nearest FACE of every query, its squared distance and the
 * closest point on it, through the uniform grid of the mesh metrics with faces binned by bounding box.  vertices
 * (V,3) float32 finite, faces (F,3) int32 with 0 <= index < V, query (n,3) float32 finite: the kernels check neither,
 * the caller does.  3 F, n and n_keys below 2^31, every dim in [1, 1024], cell and inv finite and positive, else
 * NERF_E_ARG; the int64 and double arrays 8-byte aligned, else NERF_E_ALIGN; both before any launch.  lo (3 floats)
 * and dims (3 int32) are HOST arrays and the grid's box [lo, lo + dims cell] must hold every vertex (up to rounding).
 * No LDS, no atomics, one writer per output: equal inputs give equal bits.  Every fp64 operation rounds on its own.
 * nerf_mesh_face_cell_counts: counts[f] (F) int64 = the number of cells of the index box
 *   [cell_index(min corner), cell_index(max corner)] of face f on the three axes (fminf / fmaxf over its corners, the
 *   fp32 cell index of nerf_points_cell_keys), at most 2^30.  One thread per face.
 * nerf_mesh_face_cell_keys: offsets (F) int64 = the CALLER's exclusive sum of the counts; face f writes its
 *   counts[f] keys (cell_id << 32) | f at keys[offsets[f] ..] in ascending cell_id order.  The CALLER sorts all keys
 *   ascending (any int64 sort) and keeps their number below 2^31.  One thread per face.
 * nerf_mesh_nearest_faces: for every query the nearest of the faces behind sorted_keys (n_keys): d2[i] (double) = the
 *   squared distance to the closest point of that face, face[i] = its index, the smallest on equal d2, closest (n,3)
 *   float32 or NULL = that point rounded to fp32: a brute-force search's result bit for bit.  The closest point is
 *   computed in double from the fp32 corners by the region walk of Ericson, Real-Time Collision Detection §5.1.5 (vertex
 *   a, vertex b, edge ab, vertex c, edge ac, edge bc, interior), dot products (x x' + y y') + z z', every edge
 *   parameter and interior weight clamped to [0, 1]; a face with a repeated index, with a cross product of exactly
 *   (0, 0, 0) or with va + vb + vc <= 0 in the interior is measured as its three edges ab, ac, bc (the earlier edge
 *   on a tie): no NaN, no division by zero.  d2 = (dx dx + dy dy) + dz dz of d = query - point in double.  The search
 *   walks the shells, columns and runs of nerf_points_nearest, measures every face key of a run (a face registered in
 *   several cells more than once) and stops before shell r >= 2 once best_d2, rounded up to fp32, satisfies the rule
 *   of nerf_points_nearest (the argument: mesh_distance_core.hpp).  n_keys = 0: d2 = +inf, face = -1, closest = the
 *   query.  One thread per query. */
int nerf_mesh_face_cell_counts(const float* vertices, const int32_t* faces, int64_t F, const float* lo, float inv,
                               const int32_t* dims, int64_t* counts, hipStream_t stream);
int nerf_mesh_face_cell_keys(const float* vertices, const int32_t* faces, int64_t F, const float* lo, float inv,
                             const int32_t* dims, const int64_t* offsets, int64_t* keys, hipStream_t stream);
int nerf_mesh_nearest_faces(const float* query, int64_t n, const int64_t* sorted_keys, int64_t n_keys,
                            const float* vertices, const int32_t* faces, int64_t F, const float* lo, float cell,
                            float inv, const int32_t* dims, double* d2, int32_t* face, float* closest,
                            hipStream_t stream);

/* Nearest-hit ray casting against a mesh through the face grid above.  rays (n,8) float32 rows
 * [o, d, near, far] with o and d finite, d not all zero and near / far no NaN, vertices and faces as above: the kernel
 * checks none of it, the caller does.  The argument checks of nerf_mesh_nearest_faces, and 0 <= margin <= 2^-10 cell
 * and cull in {0, 1}, else NERF_E_ARG; sorted_keys and t 8-byte aligned, else NERF_E_ALIGN; both before any launch.
 * nerf_mesh_ray_cast: for every ray the nearest face it hits: t[i] (double) = the ray's own parameter of the hit
 *   (points are o + t d, d is not normalised), +inf on a miss; face[i] = the face, the smallest index on equal t, -1
 *   on a miss; bary (n,2) float32 = (u, v) rounded, the hit point being (1 - u - v) a + u b + v c, (0, 0) on a miss: a
 *   brute-force search's result bit for bit.  Per face, in double from the fp32 values, dot products
 *   (x x' + y y') + z z', cross products six products and three differences: e1 = b - a, e2 = c - a, p = d x e2,
 *   det = e1 . p, s = o - a, u = (s . p) / det, q = s x e1, v = (d . q) / det, t = (e2 . q) / det.  Never hit: a face
 *   with a repeated index, with a cross product of exactly (0, 0, 0), with det == 0 or, with cull, det <= 0 (det > 0:
 *   the ray runs against the winding normal).  Hit: u >= 0, u <= 1, v >= 0, u + v <= 1, near <= t <= far, and
 *   o_k + t d_k within [min_k - margin, max_k + margin] of the face's corners on every axis (margin = 2^-30 of the
 *   largest |coordinate| of the mesh, the caller's); a NaN fails every comparison.  The ray is clipped to the grid's
 *   box and walks the layers of cells along its major axis, at most 3 x 3 cells per layer, stopping before a layer
 *   entered after the best t (the argument: mesh_raycast_core.hpp); a ray whose origin lies more than 2^32 cells from
 *   the grid tests every face.  n_keys = 0: all misses.  One thread per ray. */
int nerf_mesh_ray_cast(const float* rays, int64_t n, const int64_t* sorted_keys, int64_t n_keys,
                       const float* vertices, const int32_t* faces, int64_t F, const float* lo, float cell, float inv,
                       const int32_t* dims, double margin, int cull, double* t, int32_t* face, float* bary,
                       hipStream_t stream);

/* Point-in-mesh by exact crossing counts through the face grid above, and uniform points of a box.
 * query (n,3) float32 finite, vertices and faces as above: the kernels check none of it, the caller does.  The
 * argument checks of nerf_mesh_ray_cast (without margin and cull): NERF_E_ARG, and NERF_E_ALIGN for sorted_keys, both
 * before any launch.  No LDS, no atomics, one writer per output: equal inputs give equal bits.
 * nerf_mesh_point_crossings: for every query q the faces crossed by the open vertical ray q + t e_z, t > 0:
 *   crossings[i] = their number, winding[i] = the sum of their s (+1 inside a closed mesh whose normals point
 *   outwards): the result of testing every face, bit for bit.  orient(P, Q, R) is the EXACT sign of
 *   (Qx - Px)(Ry - Py) - (Qy - Py)(Rx - Px) (six exact double products of fp32 values, a floating filter
 *   |sum| > 2^-48 sum |terms|, else a Shewchuk expansion).  Face (a, b, c) is crossed iff (1) in fp32, max z > qz and
 *   qx, qy lie in [min, max] of the corners' x and y; (2) s = orient(a, b, c) != 0; (3) for each directed edge U -> V
 *   of the projection taken counter-clockwise (b and c swapped when s < 0), e = orient(U, V, q) > 0, or e == 0 and
 *   (Vy < Uy, or Vy == Uy and Vx > Ux): the query perturbed by (+eps, +eps^2), the same for every face; (4) in
 *   rounded double, n = (b - a) x (c - a), g = (nx wx + ny wy) + nz wz of w = q - a: g < 0 and s > 0, or g > 0 and
 *   s < 0.  The column of the query's cell is read from the query's own cell upwards; a face registered in several
 *   of its cells is tested once (the argument: mesh_inside_core.hpp).  n_keys = 0: zeros.  One thread per query.
 * nerf_box_points: points (n,3) float32, coordinate c of point i = lo_c + u (hi_c - lo_c) in fp32 (difference, product
 *   and sum each rounded), u = (rand64(seed, 0x626f78 + c, i) >> 40) 2^-24 with the counter random numbers of
 *   nerf_mesh_sample_surface: point i depends on (seed, i) and the box alone.  lo and hi are HOST arrays of 3 finite
 *   floats with lo <= hi and a finite difference, else NERF_E_ARG.  One thread per point. */
int nerf_mesh_point_crossings(const float* query, int64_t n, const int64_t* sorted_keys, int64_t n_keys,
                              const float* vertices, const int32_t* faces, int64_t F, const float* lo, float cell,
                              float inv, const int32_t* dims, int32_t* crossings, int32_t* winding,
                              hipStream_t stream);
int nerf_box_points(int64_t n, uint64_t seed, const float* lo, const float* hi, float* points, hipStream_t stream);

/* The generalised winding number: inside tests that also answer for open and broken meshes.
 * vertices (V,3) float32 finite, faces (F,3) int32 in [0, V), query (n,3) float32 finite: the kernels check none of
 * it, the caller does.  0 <= F, 3 F < 2^31, 0 <= n < 2^31, 0 <= B <= F, lo / inv / dims as for the face grid above,
 * else NERF_E_ARG; 64-bit arrays (keys, starts, moments, w) 8-byte aligned, else NERF_E_ALIGN; both before any
 * launch.  Everything but the centroid cell is double, every operation rounded once ((x x' + y y') + z z' for a dot
 * product, six products and three differences for a cross product).  No LDS, no atomics, one writer per output.
 * nerf_mesh_winding_keys: keys[f] = (brick << 32) | f, brick the cell_id of the cell of the fp32 centroid
 *   g_k = ((a_k + b_k) + c_k) * 0x1.555556p-2f of face f (the fp32 cell index of the face grid).  One thread per face.
 * nerf_mesh_winding_soup: soup (F,9) float32, row j = the corners a, b, c of face sorted_keys[j] & 0xffffffff.
 * nerf_mesh_winding_moments: starts (B,) int64 ascending with starts[0] = 0, the first sorted position of every
 *   occupied brick; brick b owns [starts[b], starts[b+1]) ([.., F) for the last).  runs (B,2) int32 = that run;
 *   moments (B,7) double = p (3), n (3), r2, summed over the run in sorted order by one thread: x = (b - a) x (c - a),
 *   n += 0.5 x, m = sqrt(x . x), s = (a + b) + c, P += m s, M += m, S += s; p = P / (3 M) if M > 0 else
 *   S / (3 count); r2 = the largest (corner - p) . (corner - p) of the run.
 * nerf_mesh_winding: w[i] (double) = acc / 12.566370614359172, acc summed over the bricks b = 0 .. B-1 in order: with
 *   d = p_b - q and d2 = d . d, brick b is far iff exact == 0 and d2 > (beta beta) r2_b (strict), and adds
 *   (d . n_b) / (d2 sqrt(d2)); otherwise it adds 2 atan2(N, D) for the faces of its run in order, with a, b, c =
 *   corner - q, N = a . (b x c), D = (((|a| |b|) |c| + (a . b) |c|) + (b . c) |a|) + (c . a) |b|, |a| = sqrt(a . a).
 *   +1 inside a closed mesh whose normals point outwards.  beta finite and >= 1, exact in {0, 1}, (B > 0) == (F > 0),
 *   else NERF_E_ARG.  B = 0: zeros.  One thread per query. */
int nerf_mesh_winding_keys(const float* vertices, const int32_t* faces, int64_t F, const float* lo, float inv,
                           const int32_t* dims, int64_t* keys, hipStream_t stream);
int nerf_mesh_winding_soup(const float* vertices, const int32_t* faces, int64_t F, const int64_t* sorted_keys,
                           float* soup, hipStream_t stream);
int nerf_mesh_winding_moments(const float* soup, int64_t F, const int64_t* starts, int64_t B, int32_t* runs,
                              double* moments, hipStream_t stream);
int nerf_mesh_winding(const float* query, int64_t n, const int32_t* runs, const double* moments, int64_t B,
                      const float* soup, int64_t F, double beta, int exact, double* w, hipStream_t stream);

/* TSDF fusion of depth views.  The volume is the lattice of nerf_mesh_emit: tsdf and weight
 * (nx,ny,nz) contiguous fp32, p = (ix ny + iy) nz + iz, the point x = lo + (ix,iy,iz) h, h = (hi - lo) / (n - 1);
 * every dimension >= 2 and nx ny nz < 2^31, lo / hi HOST arrays of 3 floats with lo < hi (else NERF_E_ARG).  A fresh
 * volume holds tsdf = 1, weight = 0.  Everything is fp32 and every operation is rounded once.
 * nerf_tsdf_integrate: c2w (n_views,12) rows of the 3x4 camera-to-world matrices of nerf_rays_gen, depth
 *   (n_views,H,W) ranges along unit ray directions (the depth of Mesh.render / render_image), indexed in int64; one
 *   fx, fy, cx, cy and trunc for the launch: trunc, fx, fy finite and > 0, cx, cy finite, 1 <= H, W <= 2^24 (else
 *   NERF_E_ARG).  Per voxel, the views in ascending order (n views in one launch are bit for bit n launches of one):
 *   q = x - o, o = (M[3], M[7], M[11]); c_j = q0 M[j] + q1 M[4+j] + q2 M[8+j]; zc = -c_2, skip unless zc > 0;
 *   u = fx (c_0 / zc) + cx, v = fy ((-c_1) / zc) + cy, skip unless 0 <= u < W and 0 <= v < H (in float; NaN skips);
 *   d = depth[view, floor(v), floor(u)], skip unless d is finite and > 0; r = sqrt(q0 q0 + q1 q1 + q2 q2),
 *   s = d - r, skip if s < -trunc; t = min(1, s / trunc); tsdf = (tsdf w + t) / (w + 1), w = w + 1.  A voxel that
 *   no view updated is not written.  n_views = 0 launches nothing.  One thread per voxel, no atomics; at most 8
 *   views per launch, the launches of a call one after the other on the stream (the same bits as one launch).  c2w must be
 *   finite; the kernel does not check.
 * nerf_tsdf_face_observed: face_off (nx ny nz + 1) = the exclusive scan nerf_mesh_emit took, F its total
 *   (0 <= F <= 12 nx ny nz); keep[f] = 1 iff all 8 corners of the cell that owns face f have weight >= min_weight,
 *   else 0, for f in [face_off[p], face_off[p+1]) of every point p (a slot outside [0, F) is not written).  F = 0
 *   launches nothing.  One thread per lattice point. */
int nerf_tsdf_integrate(float* tsdf, float* weight, int nx, int ny, int nz, const float* lo, const float* hi,
                        const float* depth, const float* c2w, int n_views, int H, int W, float fx, float fy, float cx,
                        float cy, float trunc, hipStream_t stream);
int nerf_tsdf_face_observed(const int32_t* face_off, const float* weight, int nx, int ny, int nz, float min_weight,
                            int64_t F, uint8_t* keep, hipStream_t stream);

/* TSDF fusion with colour.  color (nx,ny,nz,4) contiguous fp32, 16-byte aligned (else
 * NERF_E_ALIGN): r, g, b and a colour weight cw per voxel; a fresh volume holds zeros.
 * nerf_tsdf_integrate_color: nerf_tsdf_integrate's arguments, checks and rule, and rgb (n_views,H,W,3) fp32, the
 *   colour of the pixel each depth came from.  tsdf and weight are bit for bit nerf_tsdf_integrate's.  Per voxel and
 *   view, in the order of the views, after that view's update of (tsdf, w):
 *   skip the colour unless the view updated the voxel and tq = s / trunc < 1 (the update was not clamped: the voxel
 *   lies within trunc of the surface the pixel saw, so a voxel far in front of it does not take the pixel's colour);
 *   skip unless the pixel's three channels are all finite;
 *   c_j = (c_j cw + pixel_j) / (cw + 1) for j = r, g, b, then cw = cw + 1.
 *   color is written only where a view coloured the voxel.  n_views = 0 launches nothing.  One thread per voxel, no
 *   atomics; at most 8 views per launch (profiles/tsdf_color.json), the launches one after the other on the stream.
 * nerf_tsdf_sample_color: points (N,3) -> rgb_out (N,3), cover_out (N), one thread per point.  Per axis a:
 *   g = (x_a - lo_a) / h_a clamped to [0, n_a - 1]; i = min((int)floor(g), n_a - 2); f = g - (float)i.
 *   Over the 8 corners c = 0..7 of the cell (i_x + (c & 1), i_y + (c >> 1 & 1), i_z + (c >> 2 & 1)):
 *   w_a = f_a where the corner's bit of axis a is set, else 1 - f_a; tw = (w_x w_y) w_z; k = tw cw_corner;
 *   cover = cover + k, then acc_j = acc_j + k c_j for j = r, g, b.
 *   rgb_j = acc_j / cover where cover > 0, else 0.  A point with a NaN coordinate gets cover = 0 and rgb = 0; a point
 *   outside the box takes the colour of the nearest point of the box.  N = 0 launches nothing. */
int nerf_tsdf_integrate_color(float* tsdf, float* weight, float* color, int nx, int ny, int nz, const float* lo,
                              const float* hi, const float* depth, const float* rgb, const float* c2w, int n_views,
                              int H, int W, float fx, float fy, float cx, float cy, float trunc, hipStream_t stream);
int nerf_tsdf_sample_color(const float* color, int nx, int ny, int nz, const float* lo, const float* hi,
                           const float* points, int64_t N, float* rgb_out, float* cover_out, hipStream_t stream);

/* Texture baking for meshes.  The atlas is a function of (F, S = texels) alone: faces 2c and 2c + 1
 * share the square cell c of S x S texels, cells = max(1, (F + 1) / 2), cols = the smallest integer with
 * cols^2 >= cells, T = cols S, cell c starts at texel (S (c % cols), S (c / cols)); texel units, x right, y down.  In
 * its cell the even face has the UV corners (1,1), (S-3,1), (1,S-3) for its vertices 0, 1, 2, the odd face
 * (S-1,S-1), (3,S-1), (S-1,3); texel (i,j) of a cell belongs to the even face where i + j < S, else to the odd one,
 * and to nobody where that face is >= F.  S >= 5, T <= 16384, 3 F < 2^31, and T as passed equal to cols S (else
 * NERF_E_ARG).  Everything rounds once per operation.
 * nerf_mesh_atlas_texels: one thread per texel p = j T + i.  face (T,T) int32, -1 for an unowned texel; bary (T,T,2) =
 *   (b1, b2): with (x, y) the texel's centre inside its cell, turned back to (S - x, S - y) for an odd face, and
 *   L = S - 4: b1 = max((x - 1) / L, 0), b2 = max((y - 1) / L, 0), both divided by their sum where it exceeds 1,
 *   b0 = max((1 - b1) - b2, 0); position (T,T,3) = (b0 v0 + b1 v1) + b2 v2 in fp32; normal (T,T,3) or NULL: in double,
 *   rounded to fp32 at the end, g / |g| with g = (b0 n0 + b1 n1) + b2 n2 of vertex_normals (V,3), or with
 *   vertex_normals NULL g = (v1 - v0) x (v2 - v0); zeros where |g| = 0.  An unowned texel gets zeros.  F = 0 is legal
 *   (T = S, nobody owns a texel).  vertex_normals without normal is NERF_E_ARG.  The vertex indices are not checked.
 * nerf_mesh_texture_lookup: texture (T,T,C) fp32, 1 <= C <= 4; face (N) int32 and bary (N,2) = (u, v) as
 *   nerf_mesh_ray_cast returns them; out (N,C).  In the face's cell (x, y) = (w0 P0 + u P1) + v P2 of its corners with
 *   w0 = (1 - u) - v; i0 = floor(x - .5), fx = (x - .5) - i0, likewise j0, fy; the cell's origin is added to i0, i0 + 1,
 *   j0, j0 + 1 and each is clamped to [0, T - 1]; top = c00 + fx (c10 - c00), bot = c01 + fx (c11 - c01),
 *   out = top + fy (bot - top) per channel.  face < 0 gives zeros.  A face >= F or a pair outside the triangle reads
 *   other texels, never outside the texture.  N = 0 launches nothing.  One thread per lookup. */
int nerf_mesh_atlas_texels(const float* vertices, const int32_t* faces, int64_t F, int texels, int T,
                           const float* vertex_normals, int32_t* face, float* bary, float* position, float* normal,
                           hipStream_t stream);
int nerf_mesh_texture_lookup(const float* texture, int T, int C, int64_t F, int texels, const int32_t* face,
                             const float* bary, int64_t N, float* out, hipStream_t stream);

/* Library build identification (string, static). */
const char* nerf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NERF_AMD_H */
