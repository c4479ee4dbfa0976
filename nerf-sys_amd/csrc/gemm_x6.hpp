// fp32 trunk GEMMs on the bf16 matrix cores: every fp32 operand is split into three bf16 pieces x = hi + mid + lo
// (round-to-nearest at each step; 3 x 8 significant bits cover fp32's 24, so the split is exact for normal numbers)
// and A.B^T is accumulated in fp32 from the six piece products whose magnitude is >= 2^-16 of the leading one:
//   lo.hi + mid.mid + hi.lo + mid.hi + hi.mid + hi.hi     (smallest first, one fp32 accumulator per output)
// The three dropped products (mid.lo, lo.mid, lo.lo) are <= 2^-24 relative — fp32 rounding size.  Measured on
// MI355X (tools/split_probe.hip, K = 256, forward- and backward-like data, error / sum_k |a_k b_k| against fp64):
// max 5.71 / mean 0.347 x 2^-24 for this scheme against 5.78 / 0.307 for the 16x16x4 fp32 MFMA and for a sequential
// fp32 fmaf chain (the two are bitwise equal) — the same accuracy as the fp32 path, at six `v_mfma_f32_32x32x16_bf16`
// (16 cycles per 16K MACs each) instead of sixteen `v_mfma_f32_16x16x4_f32` (8 cycles per 1K MACs each): 2.7x the
// MAC rate of the fp32 matrix cores, which moves the 256x256 trunk layers from MFMA-bound to HBM-bound.
//
//   gemm_nt_x6w    C[m][n] = epi( sum_k A[m][k] B[n][k] ): A fp32 activations (split in registers), B the layer
//                  weights (forward) or their transpose (input gradient) as three pre-split bf16 planes
//   gemm_wgrad_x6  P[s][n][k] = sum_{m in split s} G[m][n] X[m][k] (+ bias column sums): both operands fp32
//                  activations, split while staged; fp32 slabs, deterministic reduce as in gemm.hpp
// Fragment / LDS conventions are gemm_bf16.hpp's (NT: [rows][BK] tiles, ds_read_b128 per fragment, C^T so a lane
// owns one output row; wgrad: row-major [m][cols] tiles read with ds_read_b64_tr_b16), one image per piece plane.
#pragma once
#include "gemm_bf16.hpp"

// two fp32 -> one packed bf16 pair in ONE v_cvt_pk_bf16_f32 (round to nearest even); the scalar-cast form
// (nerf_pack_bf16x2) compiles to two converts plus a repack
typedef float x6_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 x6_bf16x2 __attribute__((ext_vector_type(2)));
typedef float x6_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t x6_pack(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(x6_f32x2{a, b}, x6_bf16x2));
}

// four fp32 values -> their hi / mid / lo bf16 pieces, packed in pairs (v_cvt_pk_bf16_f32 rounds to nearest even).
// Each residual is the fp32 value minus the widened piece (shift / mask, packed subtract: 9 VALU per pair).  A
// v_dot2c_f32_bf16 form (7 VALU per pair, the same pieces) measured forward 0.574 -> 0.566 ms, input gradient
// unchanged, weight gradient 0.479 -> 0.515 ms, and on the forward alone within the noise
// (profiles/r05/x6_variants_ab.txt): not kept.
__device__ __forceinline__ void x6_split4(const float4 v, uint2& h, uint2& m, uint2& l) {
  const uint32_t h0 = x6_pack(v.x, v.y), h1 = x6_pack(v.z, v.w);
  const float r0 = v.x - nerf_bf16_lo(h0), r1 = v.y - nerf_bf16_hi(h0);
  const float r2 = v.z - nerf_bf16_lo(h1), r3 = v.w - nerf_bf16_hi(h1);
  const uint32_t m0 = x6_pack(r0, r1), m1 = x6_pack(r2, r3);
  const uint32_t l0 = x6_pack(r0 - nerf_bf16_lo(m0), r1 - nerf_bf16_hi(m0));
  const uint32_t l1 = x6_pack(r2 - nerf_bf16_lo(m1), r3 - nerf_bf16_hi(m1));
  h = make_uint2(h0, h1);
  m = make_uint2(m0, m1);
  l = make_uint2(l0, l1);
}

// the six piece products, smallest first: term t multiplies A piece X6_PA[t] by B piece X6_PB[t] (0 = hi, 1 = mid,
// 2 = lo).  One term is issued for every accumulator of the wave before the next term, so consecutive MFMAs never
// chain on one accumulator (a dependent 32x32x16 MFMA waits for its predecessor's result).
__device__ constexpr int X6_PA[6] = {2, 1, 0, 1, 0, 0};
__device__ constexpr int X6_PB[6] = {0, 1, 2, 0, 1, 0};
// The forward uses the same order.  A hi.lo-first forward order ran slower with the LDS epilogue (227.9k vs 229.3k
// rays/s) and its 3000-step PSNR sat inside the default's band (profiles/r04/psnr_band.txt): lo.hi first is kept.
// acc_[TM_][TN_] += over the six terms; MFMA(first_, second_) operands: NT passes (B fragment, A fragment) so the
// accumulator is C^T (gemm_bf16.hpp); the weight gradient passes (G^T fragment, X fragment)
#define X6_MFMA_BLOCK(acc_, TM_, TN_, FIRST_, SECOND_)                                                      \
  _Pragma("unroll") for (int t_ = 0; t_ < 6; ++t_)                                                        \
    _Pragma("unroll") for (int a_ = 0; a_ < TM_; ++a_)                                                    \
      _Pragma("unroll") for (int b_ = 0; b_ < TN_; ++b_)                                                  \
        acc_[a_][b_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FIRST_, SECOND_, acc_[a_][b_], 0, 0, 0);

// ------------------------------------------------------------------------------------------ weight planes
// dst plane p (p = hi, mid, lo) of job j: [rows_out][cols_out] bf16 at dst + p * plane, where for a plain job
// rows_out x cols_out = rows x cols of src (row pitch lds) and for a transposed job dst[c][r] = src[r][c]
struct X6Job {
  const float* src;
  nerf_bf16* dst;
  int rows, cols, lds, transpose;
  int64_t plane;
};
struct X6Jobs {
  X6Job j[16];
};
static __global__ void x6_planes_kernel(X6Jobs jobs) {
  const X6Job J = jobs.j[blockIdx.z];
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
    // plain: element (r0 + y, c0 + tx); transposed: element (r0 + tx, c0 + y) written to row c0 + y
    const float v = J.transpose ? tile[tx][y] : tile[y][tx];
    const int orow = J.transpose ? c0 + y : r0 + y, ocol = J.transpose ? r0 + tx : c0 + tx;
    const int orows = J.transpose ? J.cols : J.rows, ocols = J.transpose ? J.rows : J.cols;
    if (orow < orows && ocol < ocols) {
      const nerf_bf16 h = (nerf_bf16)v;
      const float r1 = v - (float)h;
      const nerf_bf16 m = (nerf_bf16)r1;
      const nerf_bf16 l = (nerf_bf16)(r1 - (float)m);
      const int64_t o = (int64_t)orow * ocols + ocol;
      J.dst[o] = h;
      J.dst[J.plane + o] = m;
      J.dst[2 * J.plane + o] = l;
    }
  }
}


// ------------------------------------------------------------------------------------------ LDS-staged epilogue
// The C^T accumulator leaves lane (li, lh) with row li, columns 8q + 4lh .. + 3 of each 32 x 32 block: the direct
// store (ntb_epilogue) writes 32 rows x 32 B per instruction, and with one workgroup per CU the 256 KiB of a tile's
// outputs leave at the store-issue rate while the matrix cores idle (cdna_hip_programming.md T21).  Here each block
// goes registers -> a private [32][36] fp32 LDS tile (144-B pitch) -> registers as 8 lanes per row, so every store
// instruction writes 8 whole 128-B lines.  Bias / ReLU / mask words are applied in registers first, exactly as
// ntb_epilogue does (same fp32 operations, bitwise the same outputs).  Against the direct stores
// (profiles/r04/x6_epilogue_ab.txt): fwd 0.625 -> 0.591 ms, dgrad 0.669 -> 0.610 ms per fine layer.
constexpr int X6E_PITCH = 36;
constexpr int X6E_WAVE_FLOATS = 32 * X6E_PITCH;
// a's upper 32 lanes <-> b's lower 32 lanes (v_permlane32_swap).  The pair's elements go through scalar temporaries:
// __builtin_bit_cast applied directly to an element expression (bit_cast(float, r[1])) read element 0 with this clang.
__device__ __forceinline__ void x6_swap32(float& a, float& b) {
  typedef unsigned x6_u32x2 __attribute__((ext_vector_type(2)));
  const x6_u32x2 r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b),
                                                      false, false);
  const unsigned r0 = r[0], r1 = r[1];
  a = __builtin_bit_cast(float, r0);
  b = __builtin_bit_cast(float, r1);
}

// HAND (the chained forward, TM = 1, n0 = 0): the stored values of columns 0 .. 63 also leave in ho[2][1][2][2] as the
// activation registers of the next layer's slabs 0 and 1 (x6w_tile's ra sets).  Lane (li, lh) holds columns
// 8 q + 4 lh + e of block b; the A fragment of k-step ks of slab b wants lane (r, h) to hold k = 16 ks + 8 h + 0 .. 7.
// For q0 = 2 ks, v_permlane32_swap of (q0, e) with (q0 + 1, e) swaps the first register's upper lanes with the second's
// lower lanes: the first then holds k = 16 ks + 8 h + e and the second k = 16 ks + 8 h + 4 + e on both lane halves.
// PREW (EPI_MASK, TM = 1): the mask words of the lane's row come in pw[TN] (x6w_tile loads them under the last slab), so
// the epilogue issues no global load: a load here sits behind the previous block's stores in the in-order counter.
template <int TM, int TN, int EPI, bool HAND = false, bool PREW = false>
__device__ __forceinline__ void x6_epilogue_lds(nerf_f32x16 (&acc)[TM][TN], int64_t mw, int n0, int lane,
                                                const float* __restrict__ bias, float* __restrict__ C, int ldc,
                                                const uint32_t* __restrict__ mbits, int ldmb,
                                                uint32_t* __restrict__ mbits_out, float* E,
                                                float4 (*ho)[1][2][2] = nullptr, const float* bias_lds = nullptr,
                                                const uint32_t* pw = nullptr) {
  static_assert(!HAND || (TM == 1 && TN >= 2 && EPI == EPI_BIAS_RELU), "hand-off: the forward tile");
  static_assert(!PREW || (TM == 1 && EPI == EPI_MASK), "preloaded mask words: the input-gradient tile");
  const int li = lane & 31, lh = lane >> 5;
  const int rr = lane >> 3, cc = 4 * (lane & 7);  // read-back: row rr + 8 i, columns cc .. cc + 3
#pragma unroll
  for (int b = 0; b < TN; ++b) {
    const int nb = n0 + b * 32;
    const int g = nb >> 5;
    float4 bv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      bv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (HAND) {
        // the wave's LDS copy of the bias row: a global load here sits behind the previous block's stores in the
        // in-order memory counter, so its wait also waits for those stores
        bv[q] = *reinterpret_cast<const float4*>(bias_lds + nb + 8 * q + 4 * lh);
      } else if (EPI == EPI_BIAS || EPI == EPI_BIAS_RELU) {
        bv[q] = *reinterpret_cast<const float4*>(bias + nb + 8 * q + 4 * lh);
      }
    }
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      const int64_t m = mw + a * 32 + li;
      uint32_t word = 0;
      if constexpr (PREW) {
        word = pw[b];
      } else if (EPI == EPI_MASK) {
        word = mbits[m * ldmb + g];
      }
      float hv[4][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = acc[a][b][4 * q + e];
          const float bb = e == 0 ? bv[q].x : (e == 1 ? bv[q].y : (e == 2 ? bv[q].z : bv[q].w));
          if (EPI == EPI_BIAS) v[e] += bb;
          if (EPI == EPI_BIAS_RELU) {
            v[e] = fmaxf(v[e] + bb, 0.f);
            word |= (v[e] > 0.f ? 1u : 0u) << (8 * q + 4 * lh + e);
          }
          if (EPI == EPI_MASK) v[e] = ((word >> (8 * q + 4 * lh + e)) & 1u) ? v[e] : 0.f;
          if constexpr (HAND) hv[q][e] = v[e];
        }
        *reinterpret_cast<float4*>(E + li * X6E_PITCH + 8 * q + 4 * lh) = make_float4(v[0], v[1], v[2], v[3]);
      }
      if constexpr (HAND) {
        if (b < 2) {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            float f0[4], f1[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              f0[e] = hv[2 * ks][e];
              f1[e] = hv[2 * ks + 1][e];
              x6_swap32(f0[e], f1[e]);
            }
            ho[b][0][ks][0] = make_float4(f0[0], f0[1], f0[2], f0[3]);
            ho[b][0][ks][1] = make_float4(f1[0], f1[1], f1[2], f1[3]);
          }
        }
      }
      if (EPI == EPI_BIAS_RELU && mbits_out) {
        word |= __shfl_xor(word, 32, 64);
        if (lh == 0) mbits_out[m * ldmb + g] = word;
      }
      // The read-back takes rows other lanes wrote.  What orders it: the wave's LDS operations execute in issue order,
      // and the write and read addresses (lane-dependent offsets into the same tile) may alias for the compiler, so it
      // can move neither the reads above these writes nor the next block's writes above these reads.  Explicit
      // barriers were built and measured (round 5, profiles/r05/x6_epi_fence_ab.txt): wavefront-scope release / acquire
      // fences cost 17 % of the launch (they wait for the block's global stores); "memory" asm clobbers and
      // sched_barriers here stop SROA from keeping o in registers (80 B of scratch per lane, or 32 KiB of LDS once
      // promoted).  Neither is kept.
      float4 o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = *reinterpret_cast<const float4*>(E + (rr + 8 * i) * X6E_PITCH + cc);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4*>(C + (mw + a * 32 + rr + 8 * i) * ldc + nb + cc) = o[i];
    }
  }
}

// ------------------------------------------------------------------------------------------ gemm_nt_x6w
// 256 x (32 TN) output tile per 512-thread workgroup (one per CU): each of the eight waves owns 32 rows x ALL columns
// of the tile, so every activation row is loaded and split by exactly one wave.  The activation operand goes HBM ->
// registers in fragment layout (lane (r, h): row r, k = 8 h .. 8 h + 7 of each 16-k step = two float4) and is split
// there, so only the pre-split weight planes pass through LDS (staging all six piece images through LDS left the LDS
// pipe as busy as the matrix cores).  Slabs of BK = 32 (two MFMA k-steps); weight images [3][BN][32] bf16,
// double-buffered; B fragments are read per pair of column blocks so that at most 24 VGPRs of them are live.
// B: three planes of [N][ldb] bf16, plane stride bplane.  Requirements (host): M % 256 == 0, N % (32 TN) == 0,
// K % 64 == 0 (the slabs are walked in pairs), lda % 4 == 0, ldb % 8 == 0.
//   forward        <EPI_BIAS_RELU, false, 0, 8>: 256 x 256 tiles, each activation row split by ONE workgroup instead of
//                  one per 128-column tile (profiles/r05/x6_variants_ab.txt: 0.572 -> 0.539 ms per fine layer)
//   input gradient <EPI_MASK, true, 8, 4>: 256 x 128 tiles at two waves per SIMD, split accumulators (BIGSMALL below;
//                  0.73-0.75 -> 0.665 ms per fine layer against 64-row waves at one per SIMD), K = 256 unrolled on
//                  three activation register sets (NKC below)
// bf16 elements of the two weight buffers (three piece images of [32 TN][32] each)
template <int TN>
constexpr int x6w_smem_elems() { return 2 * 3 * (32 * TN) * 32; }

// One output tile — rows m0 .. m0 + 255, columns n0 .. n0 + 32 TN - 1 — by the whole workgroup: the slab loop and the
// epilogue.  smem: the workgroup's x6w_smem_elems<TN>() bf16.  Called once per launch by gemm_nt_x6w_kernel (CH = 0)
// and once per layer by gemm_nt_x6w_chain_kernel (CH = 1).  There `first` marks the chain's first layer; every later
// one finds its slabs 0 and 1 in ra[0] / ra[1] (the previous layer's epilogue left them there) and its slab-0 weights
// already in buffer 0, and skips the prologue.  nBp / nldb / nbplane (CH = 1): the next layer's weight planes, nBp ==
// nullptr after the last layer.
// CH = 2: once per body by gemm_nt_x6w_dgrad_chain_kernel (the input-gradient tile, NKC = 8).  smem then has NW
// X6E_WAVE_FLOATS floats behind the weight buffers for the epilogue tiles.  After the last barrier of its slab loop
// the body issues the NEXT body's slab-0 / slab-1 activation loads (nA, the same pitch lda) into ra[0] / ra[1], and its
// last slab fetches the next body's slab-0 weights (nBp / nldb / nbplane, rows nn0 ..) into buffer 0; every body but
// the `first` skips the prologue.  After the last body the caller passes the body's own operands again (dead loads of
// valid addresses keep the instruction stream free of a branch).
// The row's four mask words are then loaded (one 16-B load) at the start of the last slab, whose closing vmcnt(0) covers
// them, and the epilogue issues no global load (x6_epilogue_lds PREW).  The per-layer launch keeps its own stream: the
// preload alone measured 0.060 ms per step there, 2.3 x the run-to-run spread (profiles/bwd_chain_ab.txt).
template <int EPI, bool BIGSMALL, int NKC, int TN, int CH = 0>
__device__ __forceinline__ void x6w_tile(const float* __restrict__ A, int lda, const nerf_bf16* __restrict__ Bp,
                                         int ldb, int64_t bplane, const float* __restrict__ bias,
                                         float* __restrict__ C, int ldc, const uint32_t* __restrict__ mbits, int ldmb,
                                         uint32_t* __restrict__ mbits_out, int K, int64_t m0, int n0,
                                         nerf_bf16* smem, float4 (&ra)[NKC > 0 ? 3 : 2][1][2][2],
                                         const nerf_bf16* nBp = nullptr, int nldb = 0, int64_t nbplane = 0,
                                         bool first = true, const float* nA = nullptr, int nn0 = 0) {
  static_assert(CH != 1 || (NKC == 0 && EPI == EPI_BIAS_RELU), "chained: the forward tile");
  static_assert(CH != 2 || (NKC > 0 && EPI == EPI_MASK), "chained: the input-gradient tile");
  constexpr bool PF = CH == 2;    // the body hands its successor slabs 0 / 1 and the slab-0 weights ...
  constexpr bool PREW = CH == 2;  // ... and preloads its mask words
  static_assert(!PREW || TN == 4, "preloaded mask words: one 16-B load per row");
  constexpr int BK = 32, NW = 8, TM = 1;          // slab depth, waves, 32-row blocks per wave
  constexpr int WTM = 32 * TM, BM = WTM * NW, BN = 32 * TN;
  constexpr int KS = BK / 16;                     // MFMA k-steps per slab
  // weight images [BN][BK] bf16 unpadded, 16-B chunk q of row r in slot q ^ ((r >> 2) & 3) (four chunks per 64-B row):
  // the staging writes (4 rows x 4 chunks per 16-lane group) and the fragment reads (16 consecutive rows, one chunk)
  // both hit 16 distinct 16-B bank slots.  The 80-B padded pitch it replaces was 2-way conflicted on the staging
  // writes (PMC SQ_LDS_BANK_CONFLICT 8.5e6 cycles per fine forward launch, profiles/r04/pmc_split.txt).
  constexpr int LS = BK;
  static_assert(BK == 32, "the swizzle assumes four 16-B chunks per row");
  auto sw = [](int r, int q) { return q ^ ((r >> 2) & 3); };
  constexpr int PL = BN * LS;
  // the epilogue tiles reuse the two weight buffers
  static_assert(2 * 3 * PL >= NW * X6E_WAVE_FLOATS * 2, "epilogue tiles");
  // chained: buffer 0 receives the next layer's slab 0 during the last slab, so the tiles take buffer 1 alone
  // ... followed by one copy of the layer's bias row (BN floats) per wave
  static_assert(CH != 1 || 3 * PL >= NW * (X6E_WAVE_FLOATS + BN) * 2, "epilogue tiles and bias rows in buffer 1");
  static_assert(CH != 1 || BN == 256, "bias row: one float4 per lane");
  // CH = 2: buffer 0 holds the next body's slab 0 during the epilogue and one 24-KiB buffer is smaller than the 36 KiB
  // of tiles, so they live behind the two buffers
  static_assert(2 * 3 * PL == x6w_smem_elems<TN>(), "weight buffers");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const nerf_bf16* Bb = Bp + (int64_t)n0 * ldb;
  const float* At = A + (m0 + wave * WTM) * lda;
  int aoff[TM];
#pragma unroll
  for (int a = 0; a < TM; ++a) aoff[a] = (a * 32 + li) * lda + 8 * lh;

  // NKC > 0 (K = NKC BK at compile time): three activation register sets, the slab loop fully unrolled — slab kt + 2's
  // loads are issued at the start of slab kt, after its weight DMA, so the end-of-slab weight wait leaves them in
  // flight (two slabs of latency instead of one; profiles/r04/x6_a3_ab.txt: 0.597 -> 0.584 ms per fine launch)
  constexpr bool A3 = NKC > 0;
  // the weight slab is DMA'd straight into the LDS image (global_load_lds_dwordx4, no VGPRs): one wave-instruction
  // fills 16 rows x 64 B of a piece image, lane l -> row l / 4, slot l % 4, so the swizzle goes on the source: lane l
  // reads chunk (l % 4) ^ ((row >> 2) & 3) = (l & 3) ^ ((l >> 4) & 3) of its row.  Issued as inline asm after the touch
  // of the slab's activation registers (hipcc neither counts these loads nor drains them at its own waits).  Against
  // register staging (profiles/r04/x6_glds_ab.txt): fwd 0.595 -> 0.572-0.583 ms, dgrad 0.614 -> 0.588-0.594 ms per fine
  // launch, the same loss bits
  constexpr int GPP = BN * BK * 2 / 1024, GPW = 3 * GPP / NW;  // 1-KiB groups per piece image / per wave
  // the NW waves' GPW groups each must cover the three piece images' 3 GPP 1-KiB groups exactly
  static_assert(GPW * NW == 3 * GPP && GPP * 1024 == BN * BK * 2, "weight staging");
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t gofs = (uint32_t)((((lane >> 2) * ldb) + 8 * ((lane & 3) ^ ((lane >> 4) & 3))) * 2);
  const uint32_t ngofs = (uint32_t)((((lane >> 2) * nldb) + 8 * ((lane & 3) ^ ((lane >> 4) & 3))) * 2);
  const nerf_bf16* nBb = nBp + (int64_t)(CH == 2 ? nn0 : n0) * nldb;
  const uint32_t smem_u32 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)smem;
#define X6W_ALOAD(set_, k0_) X6W_ALOAD_SRC(At, set_, k0_)
#define X6W_ALOAD_SRC(At_, set_, k0_)                                                                     \
  _Pragma("unroll") for (int a = 0; a < TM; ++a)                                                         \
    _Pragma("unroll") for (int ks = 0; ks < KS; ++ks)                                                    \
      _Pragma("unroll") for (int hf = 0; hf < 2; ++hf)                                                   \
        ra[set_][a][ks][hf] = *reinterpret_cast<const float4*>((At_) + aoff[a] + (k0_) + 16 * ks + 4 * hf);
  // B fragments are read per pair of column blocks (2 x 3 fragments live).  Measured and not kept
  // (profiles/r04/x6_bfrag_ab.txt): one block at a time (fwd 0.603 -> 0.612 ms), with the next block read under the
  // current block's MFMAs (0.613-0.619); the two 4-wave halves staggered by one barrier (ping-pong): fwd 0.58 -> 0.64,
  // dgrad 0.59 -> 0.67 ms (profiles/r04/x6_pingpong_ab.txt)
  constexpr int BPG = 2;
  // slab k0_'s weight DMA into buffer dbuf_, after the touch of activation set j
#define X6W_BLOAD(k0_, dbuf_) X6W_BLOAD_SRC(Bb, ldb, bplane, gofs, k0_, dbuf_)
#define X6W_BLOAD_SRC(Bb_, ldb_, bplane_, gofs_, k0_, dbuf_)                                              \
  {                                                                                                       \
    _Pragma("unroll") for (int a = 0; a < TM; ++a)                                                       \
      _Pragma("unroll") for (int ks = 0; ks < KS; ++ks)                                                  \
        asm volatile("" ::"v"(__builtin_bit_cast(x6_f32x4, ra[j][a][ks][0])),                            \
                     "v"(__builtin_bit_cast(x6_f32x4, ra[j][a][ks][1])) : "memory");                     \
    _Pragma("unroll") for (int i = 0; i < GPW; ++i) {                                                    \
      const int g_ = wave_u + NW * i, p_ = g_ / GPP, rb_ = (g_ % GPP) * 16;                              \
      const nerf_bf16* sb_ = (Bb_) + p_ * (bplane_) + (int64_t)rb_ * (ldb_) + (k0_);                     \
      const uint32_t dst_ = smem_u32 + (uint32_t)((((dbuf_) * 3 + p_) * PL + rb_ * LS) * 2);             \
      unsigned keep_;                                                                                     \
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t" \
                   "s_mov_b32 m0, %0" : "=&s"(keep_) : "v"(gofs_), "s"(sb_), "s"(dst_) : "memory");      \
    }                                                                                                     \
  }
  // the weight DMA done: the four activation loads (TM KS 2) issued after it stay in flight
  static_assert(TM * KS * 2 == 4, "vmcnt: the activation loads after the weight DMA");
#define X6W_BWAIT() asm volatile("s_waitcnt vmcnt(4)" ::: "memory")

  // BIGSMALL: the five small piece products accumulate in their own registers (2^-8 of the hi.hi sum, so the bf16
  // MFMA's one-guard-bit accumulator update loses 2^8 less there) and hi.hi gets 1 update per k-step instead of 6
  nerf_f32x16 acc[TM][TN], accs[BIGSMALL ? TM : 1][BIGSMALL ? TN : 1];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[a][b][r] = 0.f;
        if constexpr (BIGSMALL) accs[a][b][r] = 0.f;
      }

  const int nk = A3 ? NKC : K / BK;
  float4 bz = make_float4(0.f, 0.f, 0.f, 0.f);  // chained: this lane's four values of the bias row, for the epilogue
  if constexpr (CH == 1) bz = *reinterpret_cast<const float4*>(bias + n0 + 4 * lane);
  uint4 pw4 = make_uint4(0u, 0u, 0u, 0u);   // PREW: the four mask words of row m0 + 32 wave + li
  if (CH == 0 || first) {
    X6W_ALOAD(0, 0);
    X6W_ALOAD(1, (nk > 1 ? 1 : 0) * BK);
    {
      const int j = 0;
      X6W_BLOAD(0, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
  }
  // one slab's k-steps on activation register set rj and weight buffer S
  auto slab_mfma = [&](const float4 (&rj)[TM][KS][2], const nerf_bf16* S, auto&& after_split) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          nerf_bf16x8 af[TM][3];
#pragma unroll
          for (int a = 0; a < TM; ++a) {
            uint2 h0, m0_, l0, h1, m1, l1;
            x6_split4(rj[a][ks][0], h0, m0_, l0);
            x6_split4(rj[a][ks][1], h1, m1, l1);
            af[a][0] = __builtin_bit_cast(nerf_bf16x8, make_uint4(h0.x, h0.y, h1.x, h1.y));
            af[a][1] = __builtin_bit_cast(nerf_bf16x8, make_uint4(m0_.x, m0_.y, m1.x, m1.y));
            af[a][2] = __builtin_bit_cast(nerf_bf16x8, make_uint4(l0.x, l0.y, l1.x, l1.y));
          }
          // ... and their pieces computed: without this touch the scheduler may leave part of the last k-step's split
          // after after_split's loads, the old and new values of a set then interfere, and the allocator gives the loads
          // other registers and copies them at the end of the round — behind a vmcnt(0) that drains the loads in flight
          // (seen in the chained kernel: 8 v_mov_b64 and the drain per round)
          if constexpr (CH == 1) {
            if (ks == KS - 1) {
#pragma unroll
              for (int a = 0; a < TM; ++a) asm volatile("" ::"v"(af[a][0]), "v"(af[a][1]), "v"(af[a][2]) : "memory");
            }
          }
          if (ks == KS - 1) after_split();  // the slab's activation registers are all split
#pragma unroll
          for (int bp = 0; bp < TN / BPG; ++bp) {  // groups of BPG column blocks: BPG x 3 B fragments live
            nerf_bf16x8 bf[BPG][3];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
              for (int b = 0; b < BPG; ++b)
                bf[b][p] = *reinterpret_cast<const nerf_bf16x8*>(S + p * PL + ((BPG * bp + b) * 32 + li) * LS +
                                                                 8 * sw((BPG * bp + b) * 32 + li, 2 * ks + lh));
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
              for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < BPG; ++b) {
                  if constexpr (BIGSMALL) {
                    if (t < 5)
                      accs[a][BPG * bp + b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                          bf[b][X6_PB[t]], af[a][X6_PA[t]], accs[a][BPG * bp + b], 0, 0, 0);
                    else
                      acc[a][BPG * bp + b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                          bf[b][X6_PB[t]], af[a][X6_PA[t]], acc[a][BPG * bp + b], 0, 0, 0);
                  } else {
                    acc[a][BPG * bp + b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        bf[b][X6_PB[t]], af[a][X6_PA[t]], acc[a][BPG * bp + b], 0, 0, 0);
                  }
                }
          }
        }
  };
  if constexpr (A3) {
#pragma unroll
    for (int kt = 0; kt < NKC; ++kt) {
      const int j = kt % 3;
      if (PF && kt == NKC - 1) {
        // the last slab would fetch its own weights again: it fetches the next body's slab 0 instead, which lands in
        // buffer 0 behind this slab's vmcnt(0) and barrier like any other slab
        X6W_BLOAD_SRC(nBb, nldb, nbplane, ngofs, 0, (kt + 1) & 1);
      } else {
        X6W_BLOAD((kt + 1 < NKC ? kt + 1 : kt) * BK, (kt + 1) & 1);
      }
      if constexpr (PREW) {
        if (kt == NKC - 1)
          pw4 = *reinterpret_cast<const uint4*>(mbits + (m0 + wave * WTM + li) * ldmb + (n0 >> 5));
      }
      // set (kt + 2) % 3 was consumed by slab kt - 1; the last two slabs load nothing (a dead load would be deleted by the
      // compiler and leave the counted weight wait short), so their weight wait drains the queue
      if (kt + 2 < NKC) X6W_ALOAD((kt + 2) % 3, (kt + 2) * BK);
      asm volatile("" ::: "memory");  // pinned here: hipcc otherwise sinks the loads to the end of the slab
      slab_mfma(ra[j], smem + (kt & 1) * 3 * PL, [] {});
      if (kt + 2 < NKC) {
        X6W_BWAIT();
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __syncthreads();
    }
    if constexpr (PF) {
      // sets 0 and 1 are dead (slabs 6 and 7 are split) and nothing is in flight: the next body's slabs 0 and 1, issued
      // before the epilogue's first store so that they are older than every store in the in-order counter.  Columns
      // 0 .. 63 of the next A were stored either by another launch or by the nt = 0 epilogue of this layer, which the
      // vmcnt(0) of the slab loop above has drained.  Pinned: hipcc may not sink them below the epilogue.
      const float* nAt = nA + (m0 + wave * WTM) * lda;
      X6W_ALOAD_SRC(nAt, 0, 0);
      X6W_ALOAD_SRC(nAt, 1, BK);
      asm volatile("" ::: "memory");
    }
  } else {
    for (int kt0 = 0; kt0 < nk; kt0 += 2) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {  // slab kt = kt0 + j: LDS buffer j, activation register set j
        // nk is even (host: K % (2 BK) == 0), so no guard — every path into the loop header then has the same loads in
        // flight and the compiler's counted wait there stays vmcnt(8) instead of draining to vmcnt(0)
        const int kt = kt0 + j;
        if (CH != 0 && j == 1) {
          // chained: the last slab (always an odd one) fetches the NEXT layer's slab 0 instead of its own slab again;
          // it lands in buffer 0 behind this slab's wait and barrier like any other slab
          const bool nx = nBp != nullptr && kt + 1 >= nk;
          X6W_BLOAD_SRC((nx ? nBb : Bb), (nx ? nldb : ldb), (nx ? nbplane : bplane), (nx ? ngofs : gofs),
                        (nx ? 0 : (kt + 1 < nk ? kt + 1 : kt) * BK), j ^ 1);
        } else {
          X6W_BLOAD((kt + 1 < nk ? kt + 1 : kt) * BK, j ^ 1);
        }
        // set j's next loads issued right after its last split, pinned before the last k-step's MFMAs
        // (profiles/r04/x6_early_a_ab.txt: fwd 0.582 -> 0.578 ms, C2 +0.5 %)
        slab_mfma(ra[j], smem + j * 3 * PL, [&] {
          X6W_ALOAD(j, (kt + 2 < nk ? kt + 2 : nk - 1) * BK);
          asm volatile("" ::: "memory");
        });
        X6W_BWAIT();
        __syncthreads();
      }
    }
    // the last slab re-issued slab nk - 1's weight DMA into buffer 0, which the epilogue tiles below reuse; the loop's
    // counted vmcnt covered it only while the (dead) activation loads after it were still issued.  Drain every wave's
    // DMA and meet before any wave writes its epilogue tile, independent of what hipcc keeps.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
#undef X6W_ALOAD
#undef X6W_ALOAD_SRC
#undef X6W_BLOAD
#undef X6W_BLOAD_SRC
#undef X6W_BWAIT

  if constexpr (BIGSMALL) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b) acc[a][b] += accs[a][b];
  }
  // the loop's last barrier freed the weight images: every wave stages its 32 x 32 blocks through a private LDS
  // tile and stores whole 128-B row lines (8 lanes per row; x6_epilogue_lds)
  float* Eb = nullptr;  // chained: this wave's copy of the bias row, behind the eight tiles in buffer 1
  if constexpr (CH == 1) {
    Eb = reinterpret_cast<float*>(smem + 3 * PL) + NW * X6E_WAVE_FLOATS + wave * BN - n0;
    *reinterpret_cast<float4*>(Eb + n0 + 4 * lane) = bz;
  }
  const uint32_t pw[4] = {pw4.x, pw4.y, pw4.z, pw4.w};
  x6_epilogue_lds<TM, TN, EPI, CH == 1, PREW>(
      acc, m0 + wave * WTM, n0, lane, bias, C, ldc, mbits, ldmb, mbits_out,
      reinterpret_cast<float*>(smem + (CH == 1 ? 3 * PL : (CH == 2 ? 2 * 3 * PL : 0))) + wave * X6E_WAVE_FLOATS,
      CH == 1 ? &ra[0] : nullptr, Eb, pw);
}

template <int EPI, bool BIGSMALL, int NKC, int TN>
__global__ __launch_bounds__(512, 1) void gemm_nt_x6w_kernel(const float* __restrict__ A, int lda,
                                                             const nerf_bf16* __restrict__ Bp, int ldb, int64_t bplane,
                                                             const float* __restrict__ bias, float* __restrict__ C,
                                                             int ldc, const uint32_t* __restrict__ mbits, int ldmb,
                                                             uint32_t* __restrict__ mbits_out, int K, int n_ntiles) {
  __shared__ __attribute__((aligned(16))) nerf_bf16 smem[x6w_smem_elems<TN>()];
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = tile / n_ntiles, nt = tile - mt * n_ntiles;
  float4 ra[NKC > 0 ? 3 : 2][1][2][2];  // the activation register sets
  x6w_tile<EPI, BIGSMALL, NKC, TN>(A, lda, Bp, ldb, bplane, bias, C, ldc, mbits, ldmb, mbits_out, K, (int64_t)mt * 256,
                                   nt * 32 * TN, smem, ra);
}

// ------------------------------------------------------------------------------------------ chained forward
// The trunk forward is row-local: in the forward tile above a workgroup owns 256 rows x all 256 columns and each wave
// 32 whole rows, so the rows a wave loads for layer i + 1 are the rows it stored itself for layer i.  One launch
// therefore carries every 256-row tile through all the layers: the same x6w_tile per layer (the same MFMA sequence on
// every accumulator, bitwise the per-layer launches' outputs; tests/test_gpu_fwd_chain.py), the layers read from a
// by-value table that the kernel only reads (a write at a run-time index would move it to scratch).
// Chaining alone was SLOWER than the eight launches (17.29 -> 17.76 ms per step).  The supposed cause (only the A/B
// totals are measured): a layer's first activation loads read what the epilogue has just stored, and its first weight
// DMA sits behind those stores in the in-order memory counter, so every layer begins with the drain of 256 KiB of
// stores per CU that a launch boundary hides behind the next workgroup's start.  Built on that reading, and faster
// (profiles/fwd_chain_ab.txt):
//   - slabs 0 and 1 of the next layer stay in registers: the epilogue leaves columns 0 .. 63 in the two activation
//     register sets (x6_epilogue_lds HAND), which are dead during the epilogue and hold exactly two slabs;
//   - the last slab of a layer fetches the next layer's slab-0 weights (its weight DMA would otherwise repeat its own
//     slab), so the next layer starts computing at once and its first memory wait is one slab away.  Buffer 0 is
//     therefore busy during the epilogue, and the epilogue tiles take buffer 1 alone (36 of its 48 KiB);
//   - the epilogue reads the bias row from a per-wave LDS copy (8 x 1 KiB behind the tiles): in the ISA each block's
//     global bias loads were followed by a counted wait that also covers the previous block's stores.
// Between two layers:
//   - one release / acquire fence pair at wavefront scope: the epilogue's stores (8 lanes per row) before the next
//     layer's activation loads (one lane per row, slab 2 on) of the same wave.  No wave reads another wave's rows, so
//     nothing wider is needed;
//   - one workgroup barrier: the epilogue tiles and bias rows live in buffer 1, and the next layer's slab-1 weight DMA
//     may land there only after every wave has read its last tile back.
// A tile only touches its own rows of every buffer, so the eval ping-pong (a layer overwrites the buffer its
// predecessor's input came from) works unchanged.  Layer i >= 1 must read what layer i - 1 wrote (A_i == C_{i-1},
// lda_i == ldc_{i-1}; the host checks it).  Resources (-Rpass-analysis=kernel-resource-usage): 246 VGPRs, 89 SGPRs,
// no scratch, 96 KiB LDS, two waves per SIMD.
struct X6ChainLayer {
  const float* A;        // activations in (column 0 of row 0), row pitch lda
  const nerf_bf16* Bp;   // weight piece planes [3][256][ldb], plane stride bplane
  const float* bias;
  float* C;              // activations out, row pitch ldc
  uint32_t* mbits_out;   // ReLU bitmask [M][8], nullable
  int64_t bplane;
  int lda, ldb, ldc, K;  // K % 64 == 0
};
constexpr int X6_CHAIN_MAX = 8;
struct X6Chain {
  X6ChainLayer l[X6_CHAIN_MAX];
  int n;
};
__global__ __launch_bounds__(512, 1) void gemm_nt_x6w_chain_kernel(const X6Chain ch) {
  __shared__ __attribute__((aligned(16))) nerf_bf16 smem[x6w_smem_elems<8>()];
  const int64_t m0 = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * 256;
  float4 ra[2][1][2][2];
  // between two layers: the epilogue's stores before the next layer's loads of the same rows (slab 2 on), and every
  // wave's epilogue tile (buffer 1) read back before the next layer's slab-1 weights land there
#define X6_CHAIN_NEXT()                                        \
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       \
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");       \
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < ch.n; ++i) {
    const X6ChainLayer& L = ch.l[i];
    const X6ChainLayer& N = ch.l[i + 1 < ch.n ? i + 1 : i];
    x6w_tile<EPI_BIAS_RELU, false, 0, 8, 1>(L.A, L.lda, L.Bp, L.ldb, L.bplane, L.bias, L.C, L.ldc, nullptr, 8,
                                            L.mbits_out, L.K, m0, 0, smem, ra, i + 1 < ch.n ? N.Bp : nullptr, N.ldb,
                                            N.bplane, i == 0);
    X6_CHAIN_NEXT()
  }
#undef X6_CHAIN_NEXT
}

// ------------------------------------------------------------------------------------------ chained input gradient
// The trunk input gradients are row-local too once ONE workgroup does both 128-column tiles of a 256-row tile: in the
// input-gradient tile wave w loads rows m0 + 32 w .. + 31 of dZ_i and stores the same rows of dZ_{i-1}; after (layer i,
// columns 0 .. 127) and (layer i, columns 128 .. 255) it has written every column of its rows, which are exactly its A
// operand of layer i - 1.  One launch therefore runs the 2 n bodies of a row tile — x6w_tile<EPI_MASK, true, 8, 4> in
// chain mode CH = 2, the per-layer launch's slab loop and MFMA sequence on every accumulator, so every stored value is
// bitwise the per-layer launches' (tests/test_gpu_bwd_chain.py) — from a by-value table it only reads.
// Between two bodies, as in the forward chain: a wavefront-scope release / acquire fence pair (the wave's own stores
// before its own later loads) and one workgroup barrier (no LDS region is refilled before every wave has finished
// reading it, and every wave's part of the prefetched slab-0 weights has landed).  No flags, no polling, no atomics,
// nothing between workgroups: a tile touches only its own rows of every buffer.
// Each body hands its successor what a launch would fetch in its prologue (x6w_tile CH = 2): the next slab-0 weights
// arrive during the last slab, and the next slab-0 / slab-1 activation loads are issued before the epilogue's first
// store.  The epilogue tiles (36 KiB) have LDS of their own behind the two 24-KiB weight buffers: 84 KiB, one
// workgroup per CU as before (registers).  Against the fourteen launches: 16.578 -> 16.301 ms per step; chaining
// alone, with every body's own prologue, was not faster (profiles/bwd_chain_ab.txt).  Resources
// (-Rpass-analysis=kernel-resource-usage): 248 VGPRs, 72 SGPRs, no scratch, 84 KiB LDS, two waves per SIMD.
// l[k] is the k-th layer IN EXECUTION ORDER (trunk.7's input gradient first): C of l[k] must be A of l[k + 1], and
// lda / ldb / bplane are the same for every entry (the host checks both).
struct X6DgradLayer {
  const float* A;         // dZ_i, row pitch lda
  const nerf_bf16* Bp;    // transposed weight piece planes [3][256][ldb], plane stride bplane
  float* C;               // dZ_{i-1}, row pitch ldc
  const uint32_t* mbits;  // ReLU mask words of trunk.(i-1)'s output [M][ldmb]
  int64_t bplane;
  int lda, ldb, ldc, ldmb;
};
constexpr int X6_DGRAD_CHAIN_MAX = 7;
struct X6DgradChain {
  X6DgradLayer l[X6_DGRAD_CHAIN_MAX];
  int n;
};
constexpr int x6w_dgrad_chain_smem_elems() { return x6w_smem_elems<4>() + 8 * X6E_WAVE_FLOATS * 2; }
__global__ __launch_bounds__(512, 1) void gemm_nt_x6w_dgrad_chain_kernel(const X6DgradChain ch) {
  __shared__ __attribute__((aligned(16))) nerf_bf16 smem[x6w_dgrad_chain_smem_elems()];
  const int64_t m0 = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * 256;
  float4 ra[3][1][2][2];
  const int nb = 2 * ch.n;
#pragma unroll 1
  for (int b = 0; b < nb; ++b) {
    const int bn = b + 1 < nb ? b + 1 : b;  // after the last body: its own operands again
    const X6DgradLayer& L = ch.l[b >> 1];
    const X6DgradLayer& N = ch.l[bn >> 1];
    x6w_tile<EPI_MASK, true, 8, 4, 2>(L.A, L.lda, L.Bp, L.ldb, L.bplane, nullptr, L.C, L.ldc, L.mbits, L.ldmb, nullptr,
                                      256, m0, 128 * (b & 1), smem, ra, N.Bp, N.ldb, N.bplane, b == 0, N.A,
                                      128 * (bn & 1));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------ gemm_wgrad_x6
// gemm_wgrad_bf16_kernel's tiling with fp32 operands split while staged: 16-row slabs (one MFMA k-step), per stage
// three G piece images [16][PG] and three X images [16][PX] (pitch = 64 B mod 256 B for the transposing reads),
// double-buffered: 60 KiB for 128 x 128 tiles -> two workgroups per CU.  Bias column sums (tiles of k-block 0) add
// the three pieces of every G value, which sum to it exactly.  Requirements: rows_per_split % 16 == 0, M % 16 == 0,
// ldg / ldx % 4 == 0.
template <int BN, int BK, int WAVES_N>
__global__ __launch_bounds__(256, 2) void gemm_wgrad_x6_kernel(const float* __restrict__ G, int ldg,
                                                              const float* __restrict__ X, int ldx,
                                                              float* __restrict__ P, int ldp, float* __restrict__ Pb,
                                                              int64_t slab, int64_t rows_per_split, int64_t M,
                                                              int n_ktiles, int n_tiles) {
  constexpr int MR = 16;
  constexpr int WAVES_K = 4 / WAVES_N;
  constexpr int WTN = BN / WAVES_N, WTK = BK / WAVES_K;
  constexpr int TM = WTN / 32, TN = WTK / 32;
  static_assert(TM >= 1 && TN >= 1, "wave tile");
  constexpr int PG = ((BN + 127) / 128) * 128 + 32, PX = ((BK + 127) / 128) * 128 + 32;
  constexpr int IG = MR * PG, IX = MR * PX;       // one piece image
  constexpr int STAGE = 3 * (IG + IX);
  constexpr int G_F4 = MR * BN / 4, X_F4 = MR * BK / 4;
  constexpr int G_PER = (G_F4 + 255) / 256, X_PER = (X_F4 + 255) / 256;
  __shared__ __attribute__((aligned(16))) nerf_bf16 smem[2 * STAGE];

  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int s = lin / n_tiles;
  const int tile = lin - s * n_tiles;
  const int nt = tile / n_ktiles, kt = tile - nt * n_ktiles;
  const int n0 = nt * BN, k0 = kt * BK;
  const int64_t r0 = (int64_t)s * rows_per_split;
  int64_t r1 = r0 + rows_per_split;
  if (r1 > M) r1 = M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave / WAVES_K, wk = wave % WAVES_K;
  const int li = lane & 31, lh = lane >> 5;
  const bool do_bias = (Pb != nullptr) && kt == 0 && wk == 0;

  constexpr int PF = 4;  // register sets in flight
  float4 rg[PF][G_PER], rx[PF][X_PER];
#define WX6_GLOAD(set_, m_)                                                                                \
  {                                                                                                        \
    _Pragma("unroll") for (int i = 0; i < G_PER; ++i) {                                                    \
      const int f = tid + 256 * i;                                                                         \
      if (G_F4 % 256 == 0 || f < G_F4)                                                                     \
        rg[set_][i] = *reinterpret_cast<const float4*>(G + ((m_) + f / (BN / 4)) * ldg + n0 + (f % (BN / 4)) * 4); \
    }                                                                                                      \
    _Pragma("unroll") for (int i = 0; i < X_PER; ++i) {                                                    \
      const int f = tid + 256 * i;                                                                         \
      if (X_F4 % 256 == 0 || f < X_F4)                                                                     \
        rx[set_][i] = *reinterpret_cast<const float4*>(X + ((m_) + f / (BK / 4)) * ldx + k0 + (f % (BK / 4)) * 4); \
    }                                                                                                      \
  }
#define WX6_SSTORE(set_, buf_)                                                                             \
  {                                                                                                        \
    nerf_bf16* Gs_ = smem + (buf_) * STAGE;                                                                \
    nerf_bf16* Xs_ = Gs_ + 3 * IG;                                                                         \
    _Pragma("unroll") for (int i = 0; i < G_PER; ++i) {                                                    \
      const int f = tid + 256 * i;                                                                         \
      if (G_F4 % 256 == 0 || f < G_F4) {                                                                   \
        uint2 h, m, l;                                                                                     \
        x6_split4(rg[set_][i], h, m, l);                                                                   \
        const int o = (f / (BN / 4)) * PG + (f % (BN / 4)) * 4;                                            \
        *reinterpret_cast<uint2*>(Gs_ + o) = h;                                                            \
        *reinterpret_cast<uint2*>(Gs_ + IG + o) = m;                                                       \
        *reinterpret_cast<uint2*>(Gs_ + 2 * IG + o) = l;                                                   \
      }                                                                                                    \
    }                                                                                                      \
    _Pragma("unroll") for (int i = 0; i < X_PER; ++i) {                                                    \
      const int f = tid + 256 * i;                                                                         \
      if (X_F4 % 256 == 0 || f < X_F4) {                                                                   \
        uint2 h, m, l;                                                                                     \
        x6_split4(rx[set_][i], h, m, l);                                                                   \
        const int o = (f / (BK / 4)) * PX + (f % (BK / 4)) * 4;                                            \
        *reinterpret_cast<uint2*>(Xs_ + o) = h;                                                            \
        *reinterpret_cast<uint2*>(Xs_ + IX + o) = m;                                                       \
        *reinterpret_cast<uint2*>(Xs_ + 2 * IX + o) = l;                                                   \
      }                                                                                                    \
    }                                                                                                      \
  }

  nerf_f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  float bsum[TM];
#pragma unroll
  for (int a = 0; a < TM; ++a) bsum[a] = 0.f;

  // transposing-read addressing (gemm_bf16.hpp): lane 4q + p of 16-lane group g reads row 8 (g >> 1) + 4 t + q,
  // columns 16 (g & 1) + 4 p .. + 3; lane i of the group receives column 16 (g & 1) + i
  const int grp = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3;
  const int trow = 8 * (grp >> 1) + q, tcol = 16 * (grp & 1) + 4 * p4;
  auto tr_frag = [&](const nerf_bf16* base, int pitch) {
    const nerf_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) nerf_s16x4*)(base));
    const nerf_s16x4 hi =
        __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) nerf_s16x4*)(base + 4 * pitch));
    const short v8 __attribute__((ext_vector_type(8))) = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(nerf_bf16x8, v8);
  };

  const int64_t nit = (r1 - r0) / MR;
  if (nit > 0) {
#pragma unroll
    for (int j = 0; j < PF; ++j) WX6_GLOAD(j, r0 + (j < nit ? j : nit - 1) * MR);
    WX6_SSTORE(0, 0);
  }
  __syncthreads();
  for (int64_t it0 = 0; it0 < nit; it0 += PF) {
#pragma unroll
   for (int j = 0; j < PF; ++j) {  // slab it = it0 + j: LDS buffer j & 1, register set j
    const int64_t it = it0 + j;
    if (it >= nit) break;
    WX6_GLOAD(j, r0 + (it + PF < nit ? it + PF : nit - 1) * MR);
    const nerf_bf16* Gs = smem + (j & 1) * STAGE;
    const nerf_bf16* Xs = Gs + 3 * IG;
    nerf_bf16x8 af[TM][3], bf[TN][3];
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
#pragma unroll
      for (int a = 0; a < TM; ++a) af[a][pc] = tr_frag(Gs + pc * IG + trow * PG + wn * WTN + a * 32 + tcol, PG);
#pragma unroll
      for (int b = 0; b < TN; ++b) bf[b][pc] = tr_frag(Xs + pc * IX + trow * PX + wk * WTK + b * 32 + tcol, PX);
    }
    if (do_bias) {
#pragma unroll
      for (int a = 0; a < TM; ++a)
        {  // the slab's 8 rows summed first, then added to the running sum (64x fewer additions to the large sum)
          float t8 = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) t8 += ((float)af[a][0][j] + (float)af[a][1][j]) + (float)af[a][2][j];
          bsum[a] += t8;
        }
    }
    // A = G^T (rows n, piece X6_PA), B = X (columns k, piece X6_PB); P itself is accumulated (not transposed)
    // the next slab's split + LDS stores interleaved with this slab's MFMAs (as gemm_wgrad_x6w; unconditional: past the
    // last slab they fill the free buffer): C2 208.8k -> 209.6k rays/s on one box, bitwise the same
    // (profiles/r03/x6_wgrad_interleave_ab.txt)
    WX6_SSTORE((j + 1) % PF, (j + 1) & 1);
    X6_MFMA_BLOCK(acc, TM, TN, af[a_][X6_PA[t_]], bf[b_][X6_PB[t_]])
#pragma unroll
    for (int q = 0; q < 6 * TM * TN; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
    }
    __syncthreads();
   }
  }
#undef WX6_GLOAD
#undef WX6_SSTORE

  float* Ps = P + (int64_t)s * slab;
#pragma unroll
  for (int a = 0; a < TM; ++a) {
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const int k = k0 + wk * WTK + b * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wn * WTN + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        Ps[(int64_t)n * ldp + k] = acc[a][b][r];
      }
    }
  }
  if (do_bias) {
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      const float v = bsum[a] + __shfl_xor(bsum[a], 32, 64);
      if (lh == 0) Pb[(int64_t)s * slab + n0 + wn * WTN + a * 32 + li] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------ gemm_wgrad_x6w
// The 256 x 256 weight gradient of one split in ONE 512-thread workgroup: G and X are each read once per split (the
// 128 x 128-tile form reads them twice, PMC 2.30 GB against 1.68 GB algorithmic per fine launch) and every element is
// split once; eight waves of 64 (n) x 128 (k) (2 x 4 MFMA tiles) amortise each G fragment over four X fragments.
// 16-row slabs, six piece images [16][288] bf16 per stage, double-buffered (108 KiB: one workgroup per CU, two waves
// per SIMD); the loads of slab it + 2 are issued at iteration it (two register sets; three were slower,
// 0.477 -> 0.512 ms in a round-4 A/B build, not kept).  The bias columns are summed from the raw staging registers.  Requirements: rows_per_split % 16 == 0, M % 16 == 0, ldg / ldx % 4 == 0, K >= 256 (the first
// 256 columns of X).
__global__ __launch_bounds__(512, 1) void gemm_wgrad_x6w_kernel(const float* __restrict__ G, int ldg,
                                                               const float* __restrict__ X, int ldx,
                                                               float* __restrict__ P, int ldp, float* __restrict__ Pb,
                                                               int64_t slab, int64_t rows_per_split, int64_t M) {
  constexpr int MR = 16, TM = 2, TN = 4, WTN = 64, WTK = 128;
  constexpr int PT = 256 + 32;                   // pitch = 64 B mod 256 B (transposing reads, gemm_bf16.hpp)
  constexpr int IMG = MR * PT;                   // one piece image
  constexpr int STAGE = 6 * IMG;                 // G hi / mid / lo, X hi / mid / lo
  __shared__ __attribute__((aligned(16))) nerf_bf16 smem[2 * STAGE];

  const int s = blockIdx.x;
  const int64_t r0 = (int64_t)s * rows_per_split;
  int64_t r1 = r0 + rows_per_split;
  if (r1 > M) r1 = M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  // bias columns: summed from the raw fp32 G values in the staging registers, 8 FMAs per thread and slab (thread tid
  // holds columns 4 (tid & 63) .. + 3 of rows tid >> 6 (mod 8)), the eight waves' partials added in wave order at the
  // end.  Round 4 summed the three pieces of each MFMA fragment in the wk == 0 waves (48 VALU per tile and slab, the
  // wk == 1 waves idle at the barrier meanwhile): 0.477 ms per fine layer -> 0.445 with the tiles shared by both waves
  // -> 0.426 ms summed raw (profiles/r05/x6_variants_ab.txt; the bias gradients' summation order changed, ~1e-7 of
  // their scale)
  const bool braw = Pb != nullptr;
  float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);

  // staging: a 16 x 256 fp32 slab = 1024 float4, thread f = tid + 512 i: row f >> 6, float4 f & 63
  constexpr int PF = 2;  // register sets (three, loads issued three slabs ahead, were slower: call 29)
  float4 rg[PF][2], rx[PF][2];
#define WX6W_GLOAD(set_, m_)                                                                               \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                          \
    const int f = tid + 512 * i;                                                                           \
    rg[set_][i] = *reinterpret_cast<const float4*>(G + ((m_) + (f >> 6)) * ldg + 4 * (f & 63));            \
    rx[set_][i] = *reinterpret_cast<const float4*>(X + ((m_) + (f >> 6)) * ldx + 4 * (f & 63));            \
  }
#define WX6W_SSTORE(set_, buf_)                                                                            \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                          \
    const int f = tid + 512 * i;                                                                           \
    const int o = (f >> 6) * PT + 4 * (f & 63);                                                            \
    nerf_bf16* S_ = smem + (buf_) * STAGE;                                                                 \
    uint2 h, m, l;                                                                                         \
    x6_split4(rg[set_][i], h, m, l);                                                                       \
    *reinterpret_cast<uint2*>(S_ + o) = h;                                                                 \
    *reinterpret_cast<uint2*>(S_ + IMG + o) = m;                                                           \
    *reinterpret_cast<uint2*>(S_ + 2 * IMG + o) = l;                                                       \
    x6_split4(rx[set_][i], h, m, l);                                                                       \
    *reinterpret_cast<uint2*>(S_ + 3 * IMG + o) = h;                                                       \
    *reinterpret_cast<uint2*>(S_ + 4 * IMG + o) = m;                                                       \
    *reinterpret_cast<uint2*>(S_ + 5 * IMG + o) = l;                                                       \
  }
#define WX6W_BACC(set_, sc_)                                                                               \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                          \
    b4.x = fmaf(rg[set_][i].x, (sc_), b4.x);                                                               \
    b4.y = fmaf(rg[set_][i].y, (sc_), b4.y);                                                               \
    b4.z = fmaf(rg[set_][i].z, (sc_), b4.z);                                                               \
    b4.w = fmaf(rg[set_][i].w, (sc_), b4.w);                                                               \
  }

  nerf_f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  const int grp = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3;
  const int trow = 8 * (grp >> 1) + q, tcol = 16 * (grp & 1) + 4 * p4;
  auto tr_frag = [&](const nerf_bf16* base) {
    const nerf_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) nerf_s16x4*)(base));
    const nerf_s16x4 hi =
        __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) nerf_s16x4*)(base + 4 * PT));
    const short v8 __attribute__((ext_vector_type(8))) = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(nerf_bf16x8, v8);
  };

  const int64_t nit = (r1 - r0) / MR;
  if (nit > 0) {
#pragma unroll
    for (int j = 0; j < PF; ++j) WX6W_GLOAD(j, r0 + (j < nit ? j : nit - 1) * MR);
    WX6W_SSTORE(0, 0);
    if (braw) WX6W_BACC(0, 1.f);
  }
  __syncthreads();
  // slab it: LDS buffer j = it & 1, register set j.  Whole rounds of the two sets run in the loop and a last odd slab
  // is peeled after it: with a break inside the unrolled round, a path with set 0's loads still in flight reached the
  // loop header and the compiler's wait counting drained every load (vmcnt(0)) at the top of each round; 0.425 ->
  // 0.421 ms per fine layer, bitwise the same (profiles/r05/x6_variants_ab.txt, call 34)
  auto do_slab = [&](auto J, const int64_t it) __attribute__((always_inline)) {
      constexpr int j = decltype(J)::value;
      WX6W_GLOAD(j, r0 + (it + PF < nit ? it + PF : nit - 1) * MR);
      const int buf = j;
      const nerf_bf16* Gs = smem + buf * STAGE;
      const nerf_bf16* Xs = Gs + 3 * IMG;
      nerf_bf16x8 af[TM][3];
#pragma unroll
      for (int pc = 0; pc < 3; ++pc)
#pragma unroll
        for (int a = 0; a < TM; ++a) af[a][pc] = tr_frag(Gs + pc * IMG + trow * PT + wn * WTN + a * 32 + tcol);
#pragma unroll
      for (int bp = 0; bp < TN / 2; ++bp) {  // column-block pairs: 2 x 3 X fragments live
        // the next slab's split + LDS stores go between the two column-block pairs (unconditionally: past the last
        // slab they fill the free buffer), and the group barriers below interleave their VALU work one MFMA at a time
        // with the second pair's MFMAs instead of leaving it between the last MFMA and the barrier: 0.52 -> 0.47 ms
        // per fine layer on MI355X (profiles/r03/x6_wgrad_interleave_ab.txt), bitwise the same results
        if (bp == 1) WX6W_SSTORE((j + 1) % PF, buf ^ 1);
        // slab it + 1's G values (a clamped repeat past the last slab: weight 0); x * 1 + s is the exact sum
        if (bp == 1 && braw) WX6W_BACC((j + 1) % PF, it + 1 < nit ? 1.f : 0.f);
        nerf_bf16x8 bf[2][3];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
#pragma unroll
          for (int b = 0; b < 2; ++b)
            bf[b][pc] = tr_frag(Xs + pc * IMG + trow * PT + wk * WTK + (2 * bp + b) * 32 + tcol);
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
          for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
              acc[a][2 * bp + b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a][X6_PA[t]], bf[b][X6_PB[t]],
                                                                         acc[a][2 * bp + b], 0, 0, 0);
        if (bp == 1) {  // the pair's fragment reads first, then one MFMA per ~4 VALU of the split, LDS writes spread
          __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
          for (int q = 0; q < 24; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
            if (q & 1) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
          }
        }
      }
      __syncthreads();
  };
  int64_t it0 = 0;
  for (; it0 + PF <= nit; it0 += PF) {
    do_slab(std::integral_constant<int, 0>{}, it0);
    do_slab(std::integral_constant<int, 1>{}, it0 + 1);
  }
  if (it0 < nit) do_slab(std::integral_constant<int, 0>{}, it0);
#undef WX6W_GLOAD
#undef WX6W_SSTORE
#undef WX6W_BACC
  if (braw) {  // the eight waves' partials meet in LDS (free after the loop's last barrier), added in wave order
    float* part = reinterpret_cast<float*>(smem);
    *reinterpret_cast<float4*>(part + wave * 256 + 4 * lane) = b4;
    __syncthreads();
    if (tid < 256) {
      float v = part[tid];
#pragma unroll
      for (int w = 1; w < 8; ++w) v += part[w * 256 + tid];
      Pb[(int64_t)s * slab + tid] = v;
    }
  }

  float* Ps = P + (int64_t)s * slab;
#pragma unroll
  for (int a = 0; a < TM; ++a) {
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const int k = wk * WTK + b * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = wn * WTN + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        Ps[(int64_t)n * ldp + k] = acc[a][b][r];
      }
    }
  }
}

