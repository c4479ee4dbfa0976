// The vanilla NeRF expert — 8x256 ReLU trunk with the [h|enc] skip at layer 4, sigma/geo heads,
// 2-layer colour MLP — forward and backward on fp32 MFMA (gfx950).
//
// Restates (psklavos1/NeRF-Sys adaptive_nerf/):
//   MetaNeRF.density / color / forward   models/inr/meta_vanilla.py:109-154 (ctor :36-97)
//   MetaLinear.forward (x W^T + b)       models/metamodule/metamodule.py:140-156
//   FrequencyEncoder (xyz L=10, dir L=4) models/encodings.py:437-444
//   trunc_exp fwd/bwd                    models/trunc_exp.py:30-61
// as the expert contract x_d (M,6) -> (M,4) of models/inr/meta_ngp.py:226-241.
//
// Activation layout in the caller's workspace (Mp = M rounded up to 256, row-major, fp32):
//   X3E [Mp][320] : cols 0..255 = trunk.3 output, cols 256..318 = xyz encoding, col 319 = 0
//                   (so trunk.4 reads cat([h, enc]) with K = 320 and no copy; trunk.0 reads cols 256..319)
//   Y0..Y2, Y4..Y7 [Mp][256], HO [Mp][4] (colour pre-activations 0..2, sigma_raw), CIN [Mp][64] (geo | dir-enc |
//   0), C0 [Mp][128].  Backward adds dZ0..dZ7 [Mp][256] (the input gradient of every trunk layer in a buffer of its
//   own), dO16 [Mp][16] (from the fused colour-branch backward), transposed trunk weights, and S split-M partial slabs
//   of the packed gradient.
//
// Forward launches (nerf_mlp_fwd_ex), split engine: pe_xyz, x6_planes (this call's weights as bf16 piece planes),
// gemm_nt_x6w_chain (trunk.0 .. trunk.7 in one launch, a 256-row tile per workgroup), fwd_tail.  With
// NERF_MLP_FWD_LAYERED or with events the trunk is eight gemm_nt_x6w launches (the chain's bitwise reference, and
// what the per-layer event pairs time); with NERF_MLP_NATIVE_FP32: pe_xyz, eight gemm_nt16, fwd_tail.
//
// Backward launches (nerf_mlp_bwd_ex), split engine, one stream: x6_planes (the transposed weights as piece planes),
// color_bwd, head_bwd (writes dZ7), gemm_nt_x6w_dgrad_chain (dZ6 .. dZ0 in one launch, a 256-row tile per workgroup),
// the weight gradients of trunk.7 .. trunk.0 (eight gemm_wgrad_x6w and the two narrow gemm_wgrad_x6 of trunk.4 and
// trunk.0), reduce_splits2.  With NERF_MLP_BWD_LAYERED, with events, with a weight-gradient stream or with
// NERF_MLP_NATIVE_DGRAD the input gradients are seven launches of two column tiles each (gemm_nt_x6w, or gemm_nt16),
// each behind its layer's weight gradient: the chain's bitwise reference, and what the per-layer event pairs time.
#include "gemm.hpp"
#include "gemm_x6.hpp"
#include "mlp_common.hpp"
#include "mlp_tail.hpp"
#include "mlp_fwd_tail.hpp"

namespace {
using namespace nerf_mlp;

struct WS {
  int64_t Mp;
  float *X3E, *Y[8], *HO, *CIN, *C0;
  uint32_t* MB[8];  // ReLU bitmasks of the trunk outputs [Mp][8] (colour layer 0 re-derives its mask from C0 > 0)
  // backward
  float *dO16, *WT, *partial, *partial2;
  float* dZ[8];  // one input-gradient buffer per trunk layer (dZ_i of trunk.i): the weight gradient of layer i reads
                 // dZ_i after the whole input-gradient chain has run (one stream) or while it runs ahead (two streams)
  nerf_bf16* WPf;  // bf16 piece planes of the trunk weights (split GEMMs): layer i at x6_fwd_off(i), [3][256][KPAD_i]
  nerf_bf16* WPb;  // ... of the transposed trunk weights (input gradients): layer i >= 1 at 3 * 65536 * (i - 1)
  int S;
  int64_t rps;
  int64_t bytes;
};

constexpr int64_t WT_FLOATS = 7 * 65536;
// bf16 piece planes (gemm_x6.hpp): forward 3 x 256 x sum(KPAD) bf16, input gradient 7 x 3 x 256 x 256 bf16
inline int64_t x6_fwd_off(int i) {
  int64_t o = 0;
  for (int j = 0; j < i; ++j) o += 3 * 256 * (int64_t)KPAD[j];
  return o;
}
constexpr int64_t X6_BWD_BF16 = 7 * 3 * 65536;
// the head backward (dZ7, head weight / bias sums) is one pass (head_bwd_kernel); the second-half sums of the split
// walks (head + colour tensors) start at P2BASE
#define P2BASE (layout().off[16])

WS carve(void* base, int64_t M, int training) {
  WS w{};
  w.Mp = round_up(M < 1 ? 1 : M, 256);
  const int64_t Mp = w.Mp;
  float* p = reinterpret_cast<float*>(base);
  auto take = [&](int64_t n) {
    float* q = p;
    p += round_up(n, 64);
    return q;
  };
  w.X3E = take(Mp * 320);
  w.WPf = reinterpret_cast<nerf_bf16*>(take(x6_fwd_off(8) / 2));
  if (training) {
    for (int i = 0; i < 8; ++i) w.Y[i] = (i == 3) ? w.X3E : take(Mp * 256);
  } else {
    float* q = take(Mp * 256);
    for (int i = 0; i < 8; ++i) w.Y[i] = (i % 2 == 0) ? q : w.X3E;  // ping-pong
  }
  w.HO = take(Mp * 4);
  w.CIN = take(Mp * 64);
  w.C0 = take(Mp * 128);
  if (training) {
    for (int i = 0; i < 8; ++i) w.MB[i] = reinterpret_cast<uint32_t*>(take(Mp * 8));
    // one training layout for the one-stream (1) and the two-stream (2) backward
    for (int i = 0; i < 8; ++i) w.dZ[i] = take(Mp * 256);
    w.dO16 = take(Mp * 16);  // [Mp][16]: the head-output gradient, written by color_bwd, read by head_bwd
    w.WT = take(WT_FLOATS);
    w.WPb = reinterpret_cast<nerf_bf16*>(take(X6_BWD_BF16 / 2));
    w.S = n_splits(Mp);
    w.rps = round_up(nerf_cdiv(Mp, w.S), 64);  // whole slabs for every wgrad MR
    w.partial = take((int64_t)w.S * layout().total);
    w.partial2 = take((int64_t)(TAIL_NQ - 1) * w.S * (layout().total - P2BASE));  // head + colour sums, parts 1..
  }
  w.bytes = (int64_t)((char*)p - (char*)base);
  return w;
}

inline int ld_of(const WS& w, int i) { return (i == 3) ? 320 : 256; }

// ------------------------------------------------------------------ elementwise kernels

// xyz positional encoding of x_d[:, :3] into X3E cols 256..319 (pad col 319 = 0; rows >= M zero).
// One thread per sample row computes its 64 values; a wave's 64 rows then leave through a per-wave LDS tile, 32 columns
// at a time, so that each store instruction writes 8 rows x 128 B (whole lines) instead of one 16-B piece of each of
// 64 rows 1280 B apart.  Same values, same bits.  Against the row-per-lane stores it measured within the noise (C2
// 225.3k vs 225.2k, profiles/r05/x6_variants_ab.txt): the kernel is bound by its 30 libm sincosf per row.  Tile pitch
// 33 floats: the row-per-lane writes of a column hit 64 distinct banks.
constexpr int PE_TP = 33;
__global__ __launch_bounds__(256) void pe_xyz_kernel(const float* __restrict__ xd, int64_t M, int64_t Mp,
                                                     float* __restrict__ X3E) {
  __shared__ float tile[4][64 * PE_TP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t m0 = ((int64_t)blockIdx.x * 4 + wv) * 64;  // this wave's first row (Mp is a multiple of 256)
  if (m0 >= Mp) return;  // wave-uniform
  const int64_t m = m0 + lane;
  float v[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) v[c] = 0.f;
  if (m < M) {
    const float x[3] = {xd[m * 6], xd[m * 6 + 1], xd[m * 6 + 2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = x[k];
      float band = 1.0f;
#pragma unroll
      for (int l = 0; l < 10; ++l) {
        float s, c;
        sincosf(x[k] * band, &s, &c);
        v[3 + k * 20 + l] = c;
        v[3 + k * 20 + 10 + l] = s;
        band *= 2.0f;
      }
    }
  }
  float* t = tile[wv];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
    for (int c = 0; c < 32; ++c) t[lane * PE_TP + c] = v[32 * hf + c];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // store i: rows 8 i + (lane >> 3), float4 (lane & 7) of the half
      const int r = 8 * i + (lane >> 3), q = lane & 7;
      const float* src = t + r * PE_TP + 4 * q;
      *reinterpret_cast<float4*>(X3E + (m0 + r) * 320 + 256 + 32 * hf + 4 * q) =
          make_float4(src[0], src[1], src[2], src[3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// batched transpose: dst_i[c][r] = src_i[r][c] for r < rows_i, c < cols_i  (src pitch lds_i)
struct TJob {
  const float* src;
  float* dst;
  int rows, cols, lds;
};
struct TJobs {
  TJob j[10];
};
__global__ void transpose_kernel(TJobs jobs) {
  const TJob J = jobs.j[blockIdx.z];
  __shared__ float tile[32][33];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  if (r0 >= J.rows || c0 >= J.cols) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int y = ty; y < 32; y += 8) {
    const int r = r0 + y, c = c0 + tx;
    tile[y][tx] = (r < J.rows && c < J.cols) ? J.src[(int64_t)r * J.lds + c] : 0.f;
  }
  __syncthreads();
  for (int y = ty; y < 32; y += 8) {
    const int c = c0 + y, r = r0 + tx;
    if (c < J.cols && r < J.rows) J.dst[(int64_t)c * J.rows + r] = tile[tx][y];
  }
}

// ------------------------------------------------------------------ launch helpers

// 16x16x4 trunk forward / input-gradient GEMMs (gemm.hpp): waves per SIMD the register budget is sized for.
// tools/gemm_bench16.hip (MI355X, C2 fine-net shape, 9 interleaved rounds): fwd 0.839 / dgrad 0.817 ms per 256x256
// launch at 3 against 0.901 / 0.874 for the 32x32x2 kernel (2: 0.861 / 0.821, 4: 0.858; BK = 32: 0.957 / 0.940).
#ifndef NERF_NT16_MINW
#define NERF_NT16_MINW 3
#endif

// The native-fp32 trunk GEMMs (N = 256): 128 x 128 tiles of the 16x16x4 form.  mbits: ReLU bitmask [M][N/32] read by
// EPI_MASK; mbits_out: bitmask written by EPI_BIAS_RELU (nullable).
template <int EPI>
int nt(const float* A, int lda, const float* B, int ldb, const float* bias, float* C, int ldc, const uint32_t* mbits,
       uint32_t* mbits_out, int64_t M, int N, int K, hipStream_t st) {
  if (M % 128 || N != 256 || K % 16) return NERF_E_ARG;
  const int ntn = N / 128;
  gemm_nt16_kernel<128, 128, 2, EPI, NERF_NT16_MINW><<<(unsigned)((M / 128) * ntn), 256, 0, st>>>(
      A, lda, B, ldb, bias, C, ldc, mbits, N / 32, mbits_out, K, ntn);
  return NERF_OK;
}

// native-fp32 trunk weight gradient, N = 256: 128 x 128 tiles over the first 256 input columns, and for K = 64
// (trunk.0) and the K = 320 remainder of trunk.4 (its encoding columns) one 256 x 64 block
int wgrad(const float* G, int ldg, const float* X, int ldx, int tensor_w, const WS& w, int N, int K, hipStream_t st) {
  const Layout& L = layout();
  float* P = w.partial + L.off[tensor_w];
  float* Pb = w.partial + L.off[tensor_w + 1];
  const int ldp = L.cols[tensor_w];
  const int64_t slab = L.total;
  if (N != 256) return NERF_E_ARG;
  auto t128 = [&](const float* Xk, float* Pk, float* Pbk) {
    gemm_wgrad_kernel<128, 128, 2><<<4 * w.S, 256, 0, st>>>(G, ldg, Xk, ldx, Pk, ldp, Pbk, slab, w.rps, w.Mp, 2, 4);
  };
  // the 256 x 64 block: four 64 x 64 tiles per split (1024 workgroups) staging 32 rows per slab.  Measured on MI355X
  // at the fine net's M (per launch): 256x64 tiles at 16 / 32 rows 398 / 358 us, 128x64 323 us, 128x32 309 us, 64x64
  // at 16 rows 272 us, this 252 us.
  auto t64 = [&](const float* Xk, float* Pk, float* Pbk) {
    gemm_wgrad_kernel<64, 64, 2, 32><<<4 * w.S, 256, 0, st>>>(G, ldg, Xk, ldx, Pk, ldp, Pbk, slab, w.rps, w.Mp, 1, 4);
  };
  if (K == 64) {
    t64(X, P, Pb);
  } else if (K == 256) {
    t128(X, P, Pb);
  } else if (K == 320) {
    t128(X, P, Pb);
    t64(X + 256, P + 256, nullptr);
  } else {
    return NERF_E_ARG;
  }
  return NERF_OK;
}

// split-product (bf16 x 6) forms of the trunk GEMMs (gemm_x6.hpp), N = 256, M a multiple of 256 (the workspace pads
// it): the forward (K = 64, 256 or 320) on 256 x 256 tiles, the input gradient (K = 256) on 256 x 128 tiles
template <int EPI>
int nt_x6(const float* A, int lda, const nerf_bf16* Bp, int ldb, int64_t bplane, const float* bias, float* C, int ldc,
          const uint32_t* mbits, uint32_t* mbits_out, int64_t M, int N, int K, hipStream_t st) {
  static_assert(EPI == EPI_BIAS_RELU || EPI == EPI_MASK, "trunk forward or input gradient");
  if (M % 256 || N != 256 || lda % 4 || ldb % 8) return NERF_E_ARG;
  if constexpr (EPI == EPI_MASK) {
    if (K != 256) return NERF_E_ARG;
    gemm_nt_x6w_kernel<EPI, true, 8, 4><<<(unsigned)((M / 256) * 2), 512, 0, st>>>(A, lda, Bp, ldb, bplane, bias, C, ldc,
                                                                                   mbits, N / 32, mbits_out, K, 2);
  } else {
    if (K % 64) return NERF_E_ARG;
    gemm_nt_x6w_kernel<EPI, false, 0, 8><<<(unsigned)(M / 256), 512, 0, st>>>(A, lda, Bp, ldb, bplane, bias, C, ldc,
                                                                              mbits, N / 32, mbits_out, K, 1);
  }
  return NERF_OK;
}

// split trunk weight gradient, N = 256: one 512-thread workgroup per split over the first 256 input columns
// (gemm_wgrad_x6w), 128 x 64 tiles over K = 64 (trunk.0) and the K = 320 remainder of trunk.4 (its encoding columns)
int wgrad_x6(const float* G, int ldg, const float* X, int ldx, int tensor_w, const WS& w, int N, int K, hipStream_t st) {
  const Layout& L = layout();
  float* P = w.partial + L.off[tensor_w];
  float* Pb = w.partial + L.off[tensor_w + 1];
  const int ldp = L.cols[tensor_w];
  const int64_t slab = L.total;
  if (N != 256 || ldg % 4 || ldx % 4) return NERF_E_ARG;
  auto t128 = [&](const float* Xk, float* Pk, float* Pbk) {
    gemm_wgrad_x6w_kernel<<<w.S, 512, 0, st>>>(G, ldg, Xk, ldx, Pk, ldp, Pbk, slab, w.rps, w.Mp);
  };
  auto t64 = [&](const float* Xk, float* Pk, float* Pbk) {
    // (a one-workgroup-per-split form reading G and X once, as gemm_wgrad_x6w, measured 185 -> 191 us per launch:
    // profiles/r04/x6_narrow_wgrad_ab.txt)
    gemm_wgrad_x6_kernel<128, 64, 4><<<2 * w.S, 256, 0, st>>>(G, ldg, Xk, ldx, Pk, ldp, Pbk, slab, w.rps, w.Mp, 1, 2);
  };
  if (K == 64) {
    t64(X, P, Pb);
  } else if (K == 256) {
    t128(X, P, Pb);
  } else if (K == 320) {
    t128(X, P, Pb);
    t64(X + 256, P + 256, nullptr);
  } else {
    return NERF_E_ARG;
  }
  return NERF_OK;
}

}  // namespace

extern "C" int64_t nerf_mlp_layout(int64_t* table) {
  const Layout& L = layout();
  if (table) {
    for (int t = 0; t < NT; ++t) {
      table[4 * t + 0] = L.off[t];
      table[4 * t + 1] = L.rows[t];
      table[4 * t + 2] = L.cols[t];
      table[4 * t + 3] = L.creal[t];
    }
  }
  return L.total;
}

extern "C" int64_t nerf_mlp_workspace_bytes(int64_t M, int training) {
  if (M < 0) return -1;
  return carve(nullptr, M, training).bytes + 256;
}

extern "C" int nerf_mlp_fwd_ex(const float* w, const float* x_d, int64_t M, float* rgb_sigma, void* ws,
                               int64_t ws_bytes, int training, int flags, hipEvent_t* ev, hipStream_t st) {
  NERF_CHECK_ARG(w && ws && M >= 0 && (M == 0 || (x_d && rgb_sigma)));  // an empty batch may pass null rows
  if (flags & ~(NERF_MLP_NATIVE_FP32 | NERF_MLP_FWD_LAYERED)) return NERF_E_ENUM;
  const bool native = flags & NERF_MLP_NATIVE_FP32;
  // the split trunk in ONE launch (gemm_nt_x6w_chain_kernel) unless the caller asks for the per-layer launches or for
  // their events: an event pair brackets one layer's launch
  const bool chained = !native && !ev && !(flags & NERF_MLP_FWD_LAYERED);
  if (!nerf_aligned16(w) || !nerf_aligned16(ws) || !nerf_aligned16(rgb_sigma)) return NERF_E_ALIGN;
  const WS W = carve(ws, M, training);
  if (ws_bytes < W.bytes) return NERF_E_WORKSPACE;
  if (M == 0) return NERF_OK;
  const Layout& L = layout();
  const int64_t Mp = W.Mp;
  auto Wt = [&](int t) { return w + L.off[t]; };

  pe_xyz_kernel<<<(unsigned)nerf_cdiv(Mp, 256), 256, 0, st>>>(x_d, M, Mp, W.X3E);  // 4 waves x 64 rows
  if (!native) {  // this call's weights as bf16 piece planes
    X6Jobs jobs{};
    for (int i = 0; i < 8; ++i)
      jobs.j[i] = X6Job{Wt(2 * i), W.WPf + x6_fwd_off(i), 256, KPAD[i], KPAD[i], 0, 256 * (int64_t)KPAD[i]};
    x6_planes_kernel<<<dim3(10, 8, 8), 256, 0, st>>>(jobs);
  }
  // trunk
  const float* in = W.X3E + 256;
  int ld_in = 320;
  X6Chain chain{};
  for (int i = 0; i < 8; ++i) {
    float* out = W.Y[i];
    const int ld_out = training ? ld_of(W, i) : ((i % 2 == 0) ? 256 : 320);
    if (i == 4) { in = W.X3E; ld_in = 320; }  // cat([h3, enc]) lives in X3E
    if (chained) {  // the same operands as nt_x6 below, one table entry per layer
      chain.l[i] = X6ChainLayer{in, W.WPf + x6_fwd_off(i), Wt(2 * i + 1), out, training ? W.MB[i] : nullptr,
                                256 * (int64_t)KPAD[i], ld_in, KPAD[i], ld_out, KPAD[i]};
      in = out;
      ld_in = ld_out;
      continue;
    }
    if (ev) (void)hipEventRecord(ev[2 * i], st);
    if (native)
      TRY(nt<EPI_BIAS_RELU>(in, ld_in, Wt(2 * i), KPAD[i], Wt(2 * i + 1), out, ld_out, nullptr,
                            training ? W.MB[i] : nullptr, Mp, 256, KPAD[i], st));
    else
      TRY(nt_x6<EPI_BIAS_RELU>(in, ld_in, W.WPf + x6_fwd_off(i), KPAD[i], 256 * (int64_t)KPAD[i], Wt(2 * i + 1), out,
                               ld_out, nullptr, training ? W.MB[i] : nullptr, Mp, 256, KPAD[i], st));
    if (ev) (void)hipEventRecord(ev[2 * i + 1], st);
    in = out;
    ld_in = ld_out;
  }
  if (chained) {
    chain.n = 8;
    for (int i = 0; i < 8; ++i) {
      if (chain.l[i].K % 64 || chain.l[i].lda % 4 || chain.l[i].ldb % 8) return NERF_E_ARG;
      // a layer's first 64 input columns are handed over in registers: they must be its predecessor's output
      if (i > 0 && (chain.l[i].A != chain.l[i - 1].C || chain.l[i].lda != chain.l[i - 1].ldc)) return NERF_E_ARG;
    }
    gemm_nt_x6w_chain_kernel<<<(unsigned)(Mp / 256), 512, 0, st>>>(chain);
  }
  // heads + colour MLP + output activations in ONE launch (mlp_fwd_tail.hpp)
  {
    FwdTailArgs T{};
    T.Y7 = in; T.ldy = ld_in; T.xd = x_d; T.w = w;
    T.off_wh = L.off[16]; T.off_bh = L.off[17]; T.off_wc0 = L.off[18]; T.off_bc0 = L.off[19];
    T.off_wc1 = L.off[20]; T.off_bc1 = L.off[21];
    T.HO = W.HO; T.CIN = W.CIN; T.C0 = W.C0; T.out = rgb_sigma;
    T.M = M; T.Mp = Mp; T.ntiles = (int)(Mp / FT_ROWS);
    const int n_cu = nerf_cu_count();
    const int grid = T.ntiles < 2 * n_cu ? T.ntiles : 2 * n_cu;
    if (training)
      fwd_tail_kernel<true><<<grid, 256, 0, st>>>(T);
    else
      fwd_tail_kernel<false><<<grid, 256, 0, st>>>(T);
  }
  return nerf_launch_status();
}


extern "C" int nerf_mlp_fwd(const float* w, const float* x_d, int64_t M, float* rgb_sigma, void* ws, int64_t ws_bytes,
                            int training, hipEvent_t* ev, hipStream_t st) {
  return nerf_mlp_fwd_ex(w, x_d, M, rgb_sigma, ws, ws_bytes, training, 0, ev, st);
}

extern "C" int64_t nerf_mlp_workspace_bytes_2s(int64_t M) {
  if (M < 0) return -1;
  return carve(nullptr, M, 2).bytes + 256;
}

namespace {
// The backward of nerf_mlp_fwd.  stw == nullptr: every launch on st (nerf_mlp_bwd).  Otherwise the weight-gradient
// GEMMs go to stw, each behind an event recorded on st after the launch that produced its input (sync[1]: colour
// branch + head dgrad -> head and trunk.7 wgrads; sync[8 - i], i < 7: trunk.(i+1) dgrad -> trunk.i wgrad), and st
// waits for stw (sync[9]) before the split reduce; sync[0] is unused.  The same kernels, grids and slabs: bitwise the
// one-stream result.
int mlp_bwd_impl(const float* w, int64_t M, const float* d_rgb_sigma, float* d_w, int accumulate, void* ws,
                 int64_t ws_bytes, int flags, hipEvent_t* ev, hipStream_t st, hipStream_t stw, hipEvent_t* sync) {
  NERF_CHECK_ARG(w && d_w && ws && M >= 0 && (M == 0 || d_rgb_sigma));
  NERF_CHECK_ARG(!stw || sync);
  if (flags & ~(NERF_MLP_NATIVE_FP32 | NERF_MLP_NATIVE_DGRAD | NERF_MLP_BWD_LAYERED)) return NERF_E_ENUM;
  const bool native = flags & NERF_MLP_NATIVE_FP32;
  // input gradients: split products with the small terms in their own accumulators (gemm_nt_x6w BIGSMALL) unless
  // NERF_MLP_NATIVE_DGRAD keeps them on the fp32 MFMA
  const bool split_dgrad = !native && !(flags & NERF_MLP_NATIVE_DGRAD);
  if (!nerf_aligned16(w) || !nerf_aligned16(ws) || !nerf_aligned16(d_w) || !nerf_aligned16(d_rgb_sigma))
    return NERF_E_ALIGN;
  const bool two = stw != nullptr;
  // the seven split input gradients in ONE launch (gemm_nt_x6w_dgrad_chain_kernel), followed by the weight gradients,
  // unless the caller asks for the per-layer launches, for their events (an event pair brackets one launch) or for a
  // weight-gradient stream (whose launches trail the per-layer input gradients)
  const bool chained = split_dgrad && !ev && !two && !(flags & NERF_MLP_BWD_LAYERED);
  const WS W = carve(ws, M, two ? 2 : 1);
  if (ws_bytes < W.bytes) return NERF_E_WORKSPACE;
  hipStream_t sw = two ? stw : st;  // the weight-gradient stream
  auto handoff = [&](int k) -> int {  // sw waits for everything issued on st so far
    if (!two) return NERF_OK;
    hipError_t e = hipEventRecord(sync[k], st);
    if (e == hipSuccess) e = hipStreamWaitEvent(stw, sync[k], 0);
    return nerf_hip_status(e);
  };
  const Layout& L = layout();
  if (M == 0) {
    if (!accumulate) (void)hipMemsetAsync(d_w, 0, L.total * sizeof(float), st);
    return nerf_launch_status();
  }
  const int64_t Mp = W.Mp;
  auto Wt = [&](int t) { return w + L.off[t]; };

  // transposed weights for the dgrad GEMMs: bf16 piece planes (split) or fp32 (NERF_MLP_NATIVE_DGRAD / native)
  float* T = W.WT;
  float* WTi[8] = {nullptr};
  TJobs jobs{};
  int nj = 0;
  if (!split_dgrad) {
    for (int i = 1; i < 8; ++i) {
      WTi[i] = T;
      jobs.j[nj++] = TJob{Wt(2 * i), T, 256, 256, KPAD[i]};  // first 256 input cols (h part for trunk.4)
      T += 65536;
    }
  } else {
    X6Jobs xj{};
    for (int i = 1; i < 8; ++i)
      xj.j[i - 1] = X6Job{Wt(2 * i), W.WPb + 3 * 65536 * (int64_t)(i - 1), 256, 256, KPAD[i], 1, 65536};
    x6_planes_kernel<<<dim3(8, 8, 7), 256, 0, st>>>(xj);
  }
  if (nj) transpose_kernel<<<dim3(8, 8, nj), 256, 0, st>>>(jobs);

  // colour branch + head activations in one kernel: dO16 and the colour weight / bias slabs (TAIL_NQ workgroups per
  // split; the colour sums of parts 1.. go to W.partial2 and are added by the final reduce)
  // events 2/3 (layer 0 has no input gradient) bracket the backward tail (colour branch + heads -> dZ7)
  if (ev) (void)hipEventRecord(ev[2], st);
  // colour branch -> dO16 [Mp][16]; then ONE pass over Y7 for dZ7 and the head weight / bias sums (mlp_tail.hpp)
  color_bwd_kernel<float, float><<<TAIL_NQ * W.S, 256, 0, st>>>(d_rgb_sigma, W.HO, W.C0, W.CIN, Wt(18), Wt(20), W.dO16,
                                                          W.partial, L.total, L.off[18], L.off[19], L.off[20], L.off[21],
                                                          W.rps, M, Mp, W.partial2, L.total - P2BASE, P2BASE, 16);
  head_bwd_kernel<<<TAIL_NQ * W.S, 256, 0, st>>>(W.dO16, W.Y[7], Wt(16), W.dZ[7], W.partial, L.total, W.partial2,
                                           L.total - P2BASE, P2BASE, L.off[16], L.off[17], W.rps, Mp);
  if (ev) (void)hipEventRecord(ev[3], st);
  TRY(handoff(1));  // dZ7 and the head / colour slabs are complete
  if (chained) {  // the same operands as the nt_x6 launches below, one table entry per layer, trunk.7 first
    X6DgradChain chain{};
    chain.n = 7;
    for (int i = 7; i >= 1; --i)
      chain.l[7 - i] = X6DgradLayer{W.dZ[i], W.WPb + 3 * 65536 * (int64_t)(i - 1), W.dZ[i - 1], W.MB[i - 1], 65536,
                                    256, 256, 256, 8};
    for (int k = 0; k < chain.n; ++k) {
      const X6DgradLayer& E = chain.l[k];
      // what nt_x6<EPI_MASK> checks, the 16-B accesses of the tile, and one pitch for every entry (a body prefetches
      // its successor's operands with its own)
      if (E.lda % 4 || E.ldb % 8 || E.ldc % 4 || E.ldmb % 4 || E.lda < 256 || E.ldc < 256 || E.ldmb < 8) return NERF_E_ARG;
      if (E.lda != chain.l[0].lda || E.ldb != chain.l[0].ldb || E.bplane != chain.l[0].bplane) return NERF_E_ARG;
      if (!nerf_aligned16(E.A) || !nerf_aligned16(E.Bp) || !nerf_aligned16(E.C) || !nerf_aligned16(E.mbits))
        return NERF_E_ALIGN;
      // a layer reads the rows its predecessor stored in the same workgroup
      if (k > 0 && (E.A != chain.l[k - 1].C || E.lda != chain.l[k - 1].ldc)) return NERF_E_ARG;
    }
    gemm_nt_x6w_dgrad_chain_kernel<<<(unsigned)(Mp / 256), 512, 0, st>>>(chain);
  }
  // trunk
  for (int i = 7; i >= 0; --i) {
    float* dcur = W.dZ[i];
    const float* X = (i == 0) ? W.X3E + 256 : (i == 4 ? W.X3E : W.Y[i - 1]);
    const int ldx = (i == 0 || i == 4) ? 320 : ld_of(W, i - 1);
    if (two && i < 7) TRY(handoff(8 - i));  // dZ_i, written by the trunk.(i+1) dgrad: sync[8 - i]
    if (ev) (void)hipEventRecord(ev[4 * i], sw);
    if (native)
      TRY(wgrad(dcur, 256, X, ldx, 2 * i, W, 256, KPAD[i], sw));
    else
      TRY(wgrad_x6(dcur, 256, X, ldx, 2 * i, W, 256, KPAD[i], sw));
    if (ev) (void)hipEventRecord(ev[4 * i + 1], sw);
    if (i > 0 && !chained) {
      float* dnext = W.dZ[i - 1];  // never a buffer that a later (or trailing) weight gradient still reads
      if (ev) (void)hipEventRecord(ev[4 * i + 2], st);
      if (!split_dgrad)
        TRY(nt<EPI_MASK>(dcur, 256, WTi[i], 256, nullptr, dnext, 256, W.MB[i - 1], nullptr, Mp, 256, 256, st));
      else
        TRY(nt_x6<EPI_MASK>(dcur, 256, W.WPb + 3 * 65536 * (int64_t)(i - 1), 256, 65536, nullptr, dnext, 256,
                            W.MB[i - 1], nullptr, Mp, 256, 256, st));
      if (ev) (void)hipEventRecord(ev[4 * i + 3], st);
    }
  }
  if (two) {  // join: the split reduce reads every weight-gradient slab
    TRY(nerf_hip_status(hipEventRecord(sync[9], stw)));
    TRY(nerf_hip_status(hipStreamWaitEvent(st, sync[9], 0)));
  }
  const int64_t n4 = L.total / 4;
  reduce_splits2_kernel<<<(unsigned)nerf_cdiv(n4, 64), 256, 0, st>>>(W.partial, L.total, W.S, d_w, n4, accumulate,
                                                                      W.partial2, L.total - P2BASE, P2BASE / 4);
  return nerf_launch_status();
}
}  // namespace

extern "C" int nerf_mlp_bwd_ex(const float* w, int64_t M, const float* d_rgb_sigma, float* d_w, int accumulate,
                               void* ws, int64_t ws_bytes, int flags, hipEvent_t* ev, hipStream_t st) {
  return mlp_bwd_impl(w, M, d_rgb_sigma, d_w, accumulate, ws, ws_bytes, flags, ev, st, nullptr, nullptr);
}

extern "C" int nerf_mlp_bwd(const float* w, int64_t M, const float* d_rgb_sigma, float* d_w, int accumulate, void* ws,
                            int64_t ws_bytes, hipEvent_t* ev, hipStream_t st) {
  return mlp_bwd_impl(w, M, d_rgb_sigma, d_w, accumulate, ws, ws_bytes, 0, ev, st, nullptr, nullptr);
}

extern "C" int nerf_mlp_bwd_2s_ex(const float* w, int64_t M, const float* d_rgb_sigma, float* d_w, int accumulate,
                                  void* ws, int64_t ws_bytes, int flags, hipEvent_t* ev, hipStream_t st,
                                  hipStream_t wgrad_stream, hipEvent_t* sync) {
  NERF_CHECK_ARG(wgrad_stream && sync && wgrad_stream != st);
  return mlp_bwd_impl(w, M, d_rgb_sigma, d_w, accumulate, ws, ws_bytes, flags, ev, st, wgrad_stream, sync);
}

extern "C" int nerf_mlp_bwd_2s(const float* w, int64_t M, const float* d_rgb_sigma, float* d_w, int accumulate, void* ws,
                               int64_t ws_bytes, hipEvent_t* ev, hipStream_t st, hipStream_t wgrad_stream,
                               hipEvent_t* sync) {
  return nerf_mlp_bwd_2s_ex(w, M, d_rgb_sigma, d_w, accumulate, ws, ws_bytes, 0, ev, st, wgrad_stream, sync);
}
