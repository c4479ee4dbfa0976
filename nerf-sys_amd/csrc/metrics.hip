// Full-image quality metrics of rendered views: the MSE behind PSNR and the per-channel SSIM.
//
// Restates runtime_evaluate's metrics (psklavos1/NeRF-Sys pipelines/online_stage/runtime_adapt.py:150-158):
// color_space_transformer (nerfs/color_space.py:22-66) on both images, then
//   mse  = mean((X - Y)^2) over all H*W*3 values,
//   ssim = pytorch_msssim.ssim(X, Y, data_range=1) per channel: with filt = the separable VALID 11-tap Gaussian
//          (sigma 1.5, fp32-normalised), mu1 = filt(X), mu2 = filt(Y), s1 = filt(X X) - mu1^2, s2 = filt(Y Y) - mu2^2,
//          s12 = filt(X Y) - mu1 mu2, C1 = 1e-4, C2 = 9e-4,
//          map = (2 mu1 mu2 + C1)/(mu1^2 + mu2^2 + C1) * (2 s12 + C2)/(s1 + s2 + C2), mean over (H-10)(W-10), unclamped.
//
// One workgroup of 256 threads per (image, 32x32 tile of the SSIM map).  It stages the 42x42-pixel halo of both
// transformed images into LDS channel-last, exactly as the rows lie in memory: a staged row is 126 contiguous floats
// and the horizontal filter of float i is sum_k g_k row[i + 3k], so the three channels need no de-interleaving.  The
// 96 filtered floats of a row are processed in three parts of 32 so that the five horizontal intermediates take
// 26 KB instead of 79 KB (69 KB of LDS in all: two workgroups per CU).  An 8-bit ground truth in the linear colour
// space goes through a 256-entry table of its transfer function, built once per workgroup.  In the vertical pass thread (vg, vi) owns
// column vi of the part and four output rows, forms the SSIM map in registers and adds it to the sum of its
// column's channel.  The squared error is summed while staging, each image pixel by the one tile that owns it.
// Every workgroup stores its four partial sums; a second launch adds an image's partials in a fixed order in double.
// No atomics anywhere: two calls on the same input give the same bits.
#include "common.hpp"

#include <mutex>

namespace {

constexpr int WIN = 11, HALO = WIN - 1;
constexpr int TH = 32, TW = 32;              // SSIM-map pixels per workgroup
constexpr int SH = TH + HALO, SW = TW + HALO;  // staged pixels
constexpr int ROW = SW * 3;                  // floats of a staged row (channel-last)
constexpr int OUTW = TW * 3;                 // horizontally filtered floats of a row
constexpr int PART = 32, NPART = OUTW / PART;
constexpr int RG = 4;                        // output rows per thread in the vertical pass
constexpr int NTHREADS = 256, NWAVES = NTHREADS / 64;
constexpr int NQ = 5;                        // filtered quantities: X, Y, XX, YY, XY
constexpr int LDS_FLOATS = 2 * SH * ROW + NQ * SH * PART + 4 * NWAVES + 256;  // halo, filtered, sums, u8 table
constexpr size_t LDS_BYTES = sizeof(float) * LDS_FLOATS;
static_assert(OUTW % PART == 0 && PART * (TH / RG) == NTHREADS && TH % RG == 0, "vertical pass: one item per thread");
static_assert(LDS_BYTES * 2 <= 160 * 1024, "two workgroups per CU");
static_assert(NTHREADS == 256, "one table entry of the 8-bit ground truth per thread");

// torch's fp32 window: exp(-(i-5)^2 / (2 1.5^2)) / sum, taps 0..5 (mirrored about the centre).  Kept as constants: a
// window recomputed with expf may differ in the last bit, which moves the result at the 1e-5 level.
constexpr float G[WIN] = {0.00102838036f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005528f, 0.266011715f,
                          0.213005528f,   0.109360687f,   0.0360007733f, 0.00759875821f, 0.00102838036f};
static_assert(__builtin_bit_cast(uint32_t, G[0]) == 0x3a86cab8u && __builtin_bit_cast(uint32_t, G[1]) == 0x3bf8ff01u &&
                  __builtin_bit_cast(uint32_t, G[2]) == 0x3d13758cu && __builtin_bit_cast(uint32_t, G[3]) == 0x3ddff87fu &&
                  __builtin_bit_cast(uint32_t, G[4]) == 0x3e5a1e1fu && __builtin_bit_cast(uint32_t, G[5]) == 0x3e8832b0u,
              "window taps are torch's fp32 values");

constexpr float C1 = 1e-4f, C2 = 9e-4f;  // (0.01 data_range)^2, (0.03 data_range)^2

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

template <bool U8>
__global__ __launch_bounds__(NTHREADS) void image_metrics_kernel(const float* __restrict__ pred,
                                                                 const void* __restrict__ gt, int H, int W, int nty,
                                                                 int ntx, int cs, float4* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sX = smem;
  float* sY = sX + SH * ROW;
  float* sF = sY + SH * ROW;          // [NQ][SH][PART]
  float* sRed = sF + NQ * SH * PART;  // [NWAVES][4]
  float* sLut = sRed + 4 * NWAVES;    // [256]
  const int tid = threadIdx.x;
  const int ntile = nty * ntx;
  const int64_t img = (int64_t)blockIdx.x / ntile;
  const int tile = (int)((int64_t)blockIdx.x - img * ntile);
  const int ty = tile / ntx, tx = tile - ty * ntx;
  const int r0 = ty * TH, c0 = tx * TW;
  const bool last_y = ty == nty - 1, last_x = tx == ntx - 1;

  // stage the halo (zeros outside the image) and sum the squared error of the pixels this tile owns: pixel (r,c)
  // belongs to tile (min(r/TH, last), min(c/TW, last)), whose halo always holds it.
  // An 8-bit ground truth takes 256 values: in the linear colour space each workgroup transforms them once (one powf
  // per thread) instead of once per staged value.  The table entry is computed exactly as the float path computes it.
  if (U8 && cs == 0) {
    sLut[tid] = clamp01(nerf_srgb_to_linear(clamp01((float)tid / 255.0f)));
    __syncthreads();
  }
  float se = 0.f;
  for (int it = tid; it < SH * ROW; it += NTHREADS) {
    const int r = it / ROW, j = it - r * ROW, pc = j / 3;
    const int gr = r0 + r;
    float x = 0.f, y = 0.f;
    if (gr < H && c0 + pc < W) {
      const int64_t o = ((img * H + gr) * (int64_t)W + c0) * 3 + j;
      x = pred[o];
      if (U8 && cs == 0) {  // linear, 8-bit: clamp(pred) against the table's clamp(srgb_to_linear(gt))
        x = clamp01(x);
        y = sLut[static_cast<const uint8_t*>(gt)[o]];
      } else {
        if (U8) y = (float)static_cast<const uint8_t*>(gt)[o] / 255.0f;
        else y = static_cast<const float*>(gt)[o];
        y = clamp01(y);  // color_space_transformer clamps the ground truth in every mode
        if (cs == 0) {   // linear: clamp(pred) against clamp(srgb_to_linear(gt))
          x = clamp01(x);
          y = clamp01(nerf_srgb_to_linear(y));
        } else if (cs == 1) {  // srgb: clamp(linear_to_srgb(clamp(pred))) against gt
          x = clamp01(nerf_linear_to_srgb(clamp01(x)));
        }
      }
      if ((r < TH || last_y) && (pc < TW || last_x)) {
        const float d = x - y;
        se += d * d;
      }
    }
    sX[it] = x;
    sY[it] = y;
  }

  const int vi = tid & (PART - 1), vg = tid / PART;
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
#pragma unroll 1
  for (int p = 0; p < NPART; ++p) {
    __syncthreads();  // the staged halo is complete / the previous part's vertical pass has read sF
    // horizontal pass: SH rows x PART floats, five quantities each
    for (int it = tid; it < SH * PART; it += NTHREADS) {
      const int r = it / PART, ii = it - r * PART;
      const float* xr = sX + r * ROW + p * PART + ii;
      const float* yr = sY + r * ROW + p * PART + ii;
      float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
      for (int k = 0; k < WIN; ++k) {
        const float x = xr[3 * k], y = yr[3 * k], g = G[k];
        m1 += g * x;
        m2 += g * y;
        xx += g * __fmul_rn(x, x);
        yy += g * __fmul_rn(y, y);
        xy += g * __fmul_rn(x, y);
      }
      sF[0 * SH * PART + it] = m1;
      sF[1 * SH * PART + it] = m2;
      sF[2 * SH * PART + it] = xx;
      sF[3 * SH * PART + it] = yy;
      sF[4 * SH * PART + it] = xy;
    }
    __syncthreads();
    // vertical pass: column vi, output rows vg*RG .. vg*RG+RG-1
    float f[NQ][RG];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float col[RG + HALO];
#pragma unroll
      for (int j = 0; j < RG + HALO; ++j) col[j] = sF[q * SH * PART + (vg * RG + j) * PART + vi];
#pragma unroll
      for (int o = 0; o < RG; ++o) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) s += G[k] * col[o + k];
        f[q][o] = s;
      }
    }
    const int i = p * PART + vi, oc = i / 3, ch = i - oc * 3;
    const bool col_ok = c0 + oc < W - HALO;
    float part = 0.f;
#pragma unroll
    for (int o = 0; o < RG; ++o) {
      const float mu1 = f[0][o], mu2 = f[1][o];
      // the products are rounded before they are subtracted, as the reference's tensor ops round them; identical
      // images then give s1 == s2 == s12 and a map of exactly (2m + C1)/(m + m + C1) * (2s + C2)/(s + s + C2)
      const float mu11 = __fmul_rn(mu1, mu1), mu22 = __fmul_rn(mu2, mu2), mu12 = __fmul_rn(mu1, mu2);
      const float s1 = __fsub_rn(f[2][o], mu11), s2 = __fsub_rn(f[3][o], mu22), s12 = __fsub_rn(f[4][o], mu12);
      const float lum = __fadd_rn(__fmul_rn(2.f, mu12), C1) / __fadd_rn(__fadd_rn(mu11, mu22), C1);
      const float con = __fadd_rn(__fmul_rn(2.f, s12), C2) / __fadd_rn(__fadd_rn(s1, s2), C2);
      const float v = lum * con;
      if (col_ok && r0 + vg * RG + o < H - HALO) part += v;
    }
    acc0 += ch == 0 ? part : 0.f;
    acc1 += ch == 1 ? part : 0.f;
    acc2 += ch == 2 ? part : 0.f;
  }

  // workgroup sums in a fixed order: wave butterflies, then the waves in index order
  se = wave_sum(se);
  acc0 = wave_sum(acc0);
  acc1 = wave_sum(acc1);
  acc2 = wave_sum(acc2);
  if (nerf_lane() == 0) {
    float* d = sRed + 4 * (tid >> 6);
    d[0] = se; d[1] = acc0; d[2] = acc1; d[3] = acc2;
  }
  __syncthreads();
  if (tid == 0) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
      o.x += sRed[4 * w]; o.y += sRed[4 * w + 1]; o.z += sRed[4 * w + 2]; o.w += sRed[4 * w + 3];
    }
    partials[blockIdx.x] = o;
  }
}

// One wave per image: lane l adds tiles l, l+64, ... in double, then a butterfly over the lanes.
__global__ __launch_bounds__(64) void image_metrics_finish_kernel(const float4* __restrict__ partials, int ntile,
                                                                  double n_values, double n_window,
                                                                  float* __restrict__ out) {
  const int64_t img = blockIdx.x;
  const int lane = nerf_lane();
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int t = lane; t < ntile; t += 64) {
    const float4 p = partials[img * ntile + t];
    s0 += (double)p.x; s1 += (double)p.y; s2 += (double)p.z; s3 += (double)p.w;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    s0 += __shfl_xor(s0, d, 64); s1 += __shfl_xor(s1, d, 64);
    s2 += __shfl_xor(s2, d, 64); s3 += __shfl_xor(s3, d, 64);
  }
  if (lane == 0) {
    float* o = out + img * 4;
    o[0] = (float)(s0 / n_values);
    o[1] = (float)(s1 / n_window);
    o[2] = (float)(s2 / n_window);
    o[3] = (float)(s3 / n_window);
  }
}

// dynamic LDS above 64 KB must be allowed per kernel, once per process
template <typename K>
void allow_lds(K kernel) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)LDS_BYTES);
}
std::once_flag g_lds_once;

int64_t tiles_of(int H, int W) { return nerf_cdiv(H - HALO, TH) * nerf_cdiv(W - HALO, TW); }

}  // namespace

extern "C" int nerf_image_metrics_tile(int* tile_h, int* tile_w) {
  NERF_CHECK_ARG(tile_h && tile_w);
  *tile_h = TH;
  *tile_w = TW;
  return NERF_OK;
}

extern "C" int64_t nerf_image_metrics_workspace_bytes(int64_t n_img, int H, int W) {
  if (n_img < 0 || H < WIN || W < WIN) return -1;
  return n_img * tiles_of(H, W) * (int64_t)sizeof(float4);
}

extern "C" int nerf_image_metrics(const float* pred, const float* gt_f32, const uint8_t* gt_u8, int64_t n_img, int H,
                                  int W, int color_space, void* ws, int64_t ws_bytes, float* out,
                                  hipStream_t stream) {
  if (color_space < 0 || color_space > 2) return NERF_E_ENUM;
  NERF_CHECK_ARG(n_img >= 0 && H >= WIN && W >= WIN);
  if (n_img == 0) return NERF_OK;
  NERF_CHECK_ARG(pred && out && ws && ((gt_f32 != nullptr) != (gt_u8 != nullptr)));
  if (!nerf_aligned16(ws)) return NERF_E_ALIGN;
  const int64_t ntile = tiles_of(H, W);
  NERF_CHECK_ARG(ntile <= INT32_MAX && n_img <= INT32_MAX / ntile);  // one workgroup per (image, tile): grid.x
  if (ws_bytes < nerf_image_metrics_workspace_bytes(n_img, H, W)) return NERF_E_WORKSPACE;
  std::call_once(g_lds_once, [] {
    allow_lds(image_metrics_kernel<false>);
    allow_lds(image_metrics_kernel<true>);
  });
  const int nty = (int)nerf_cdiv(H - HALO, TH), ntx = (int)nerf_cdiv(W - HALO, TW);
  const unsigned grid = (unsigned)(n_img * ntile);
  float4* partials = static_cast<float4*>(ws);
  if (gt_u8)
    image_metrics_kernel<true><<<grid, NTHREADS, LDS_BYTES, stream>>>(pred, gt_u8, H, W, nty, ntx, color_space, partials);
  else
    image_metrics_kernel<false><<<grid, NTHREADS, LDS_BYTES, stream>>>(pred, gt_f32, H, W, nty, ntx, color_space, partials);
  image_metrics_finish_kernel<<<(unsigned)n_img, 64, 0, stream>>>(partials, (int)ntile, (double)H * W * 3.0,
                                                                 (double)(H - HALO) * (W - HALO), out);
  return nerf_launch_status();
}
