// Texture baking for meshes: the per-face atlas, the surface point and normal of every texel and the
// bilinear lookup by (face, barycentric pair), written once for the device and for a host compiler so that both can
// be run and checked under a host sanitizer without a GPU.  tests/mesh_texture_reference.py restates them in numpy.
// Build with -ffp-contract=off: every fp32 and fp64 operation below rounds on its own.
//
// The atlas is a function of (F, S) alone.  Faces 2c and 2c + 1 share the square cell c of S x S texels, S >= 5;
// cells = max(1, (F + 1) / 2), cols = the smallest integer with cols^2 >= cells, the texture is T x T with
// T = cols S, and cell c starts at texel (S (c % cols), S (c / cols)).  Texel units, x to the right, y down, texel
// (i, j) covers [i, i + 1] x [j, j + 1].  Inside its cell the even face has the UV corners (1, 1), (S - 3, 1),
// (1, S - 3) for its vertices 0, 1, 2 and the odd face those turned by 180 degrees about the cell's centre:
// (S - 1, S - 1), (3, S - 1), (S - 1, 3).  Texel (i, j) of a cell belongs to the even face where i + j < S and to the
// odd face elsewhere; a texel whose face is >= F belongs to nobody.
//
// No bleeding.  A point of the even triangle has x, y >= 1 and x + y <= S - 2.  The bilinear fetch at a = x - .5,
// b = y - .5 reads the texels i0 = floor(a), i0 + 1 and j0 = floor(b), j0 + 1, and a + b <= S - 3.  Texel (i0, j0) has
// i0 + j0 <= S - 3.  Texel (i0 + 1, j0) carries the weight frac(a) (1 - frac(b)); where that is not zero,
// i0 + j0 <= a + b - frac(a) < S - 3, an integer, so i0 + j0 <= S - 4 and the texel's sum is at most S - 3; likewise
// (i0, j0 + 1), and (i0 + 1, j0 + 1) with its weight frac(a) frac(b) has a sum of at most S - 2.  So every texel with
// weight has i + j <= S - 2, and a, b >= .5 keep it at i, j >= 0.  The odd triangle is the same picture turned: every
// texel with weight has i + j >= S and i, j <= S - 1.  The diagonal i + j = S - 1 and the one-texel border of the cell
// are the gutter.  This holds for the real numbers; the fp32 mix of the corners can round a point of the odd
// hypotenuse that sits on a texel centre below that centre in both coordinates, and the diagonal texel then enters
// with the product of two rounding errors as its weight (below 2^-40).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NERF_MT_HD __host__ __device__ __forceinline__
#else
#define NERF_MT_HD inline
#endif

namespace nerf_mt {

constexpr int32_t MIN_TEXELS = 5;
constexpr int32_t MAX_SIDE = 16384;

struct Atlas {
  int64_t F;
  int32_t S, cols, T;
};

// The layout of (F, S) in integers: false where S < 5, F < 0 or T would exceed MAX_SIDE.  cols by bisection over
// [1, MAX_SIDE]: at most 15 halvings, no float root.
inline bool make_atlas(int64_t F, int64_t S, Atlas& A) {
  if (F < 0 || S < MIN_TEXELS || S > MAX_SIDE) return false;
  const int64_t cells = F > 1 ? F / 2 + (F & 1) : 1;  // max(1, (F + 1) / 2) without the overflow at the largest F
  int64_t lo = 1, hi = MAX_SIDE;  // the smallest cols in [lo, hi] with cols^2 >= cells, if any
  if (hi * hi < cells) return false;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (mid * mid >= cells) hi = mid;
    else lo = mid + 1;
  }
  if (lo * S > MAX_SIDE) return false;
  A.F = F, A.S = (int32_t)S, A.cols = (int32_t)lo, A.T = (int32_t)(lo * S);
  return true;
}

// UV corner k of a face of the given parity, inside its cell: small integers, exact in fp32
NERF_MT_HD void corner_uv(int32_t S, int odd, int k, float& x, float& y) {
  const float ex = k == 1 ? (float)(S - 3) : 1.0f, ey = k == 2 ? (float)(S - 3) : 1.0f;
  x = odd ? (float)S - ex : ex;
  y = odd ? (float)S - ey : ey;
}

NERF_MT_HD double norm3(const double g[3]) {
  const double xx = g[0] * g[0], yy = g[1] * g[1], zz = g[2] * g[2];
  return sqrt((xx + yy) + zz);
}

// Texel p = j T + i of the atlas: its face (-1: nobody's), the barycentric pair (b1, b2) of the surface point it
// stands for, that point b0 v0 + b1 v1 + b2 v2 in fp32 (three products, (t0 + t1) + t2) and, with normal_out, a unit
// normal in double rounded to fp32 at the end: the same mix of the vertex normals, or without them the cross product
// (v1 - v0) x (v2 - v0) of the face, divided by its length; zeros where the length is zero.  An unowned texel gets
// zeros.  A NaN vertex propagates to the position and to the face normal.
//
// The point: the texel's centre (i + .5, j + .5) inside its cell, for an odd face turned back to (S - i - .5,
// S - j - .5), is (x, y); with L = S - 4, b1 = max((x - 1) / L, 0), b2 = max((y - 1) / L, 0), both divided by their sum
// where that exceeds 1, b0 = max((1 - b1) - b2, 0).  Inside the UV triangle this inverts the corner mix; a gutter texel
// takes a nearby boundary point of its own face, which is the dilation.
NERF_MT_HD void texel(const Atlas& A, const float* __restrict__ verts, const int32_t* __restrict__ faces,
                      const float* __restrict__ vertex_normals, int64_t p, int32_t* __restrict__ face_out,
                      float* __restrict__ bary_out, float* __restrict__ position_out,
                      float* __restrict__ normal_out) {
  const int32_t ia = (int32_t)(p % A.T), ja = (int32_t)(p / A.T);
  const int32_t cx = ia / A.S, cy = ja / A.S;
  const int32_t i = ia - cx * A.S, j = ja - cy * A.S;
  const int odd = i + j >= A.S;
  const int64_t f = 2 * ((int64_t)cy * A.cols + cx) + odd;
  if (f >= A.F) {
    face_out[p] = -1;
    bary_out[2 * p] = bary_out[2 * p + 1] = 0.0f;
    position_out[3 * p] = position_out[3 * p + 1] = position_out[3 * p + 2] = 0.0f;
    if (normal_out) normal_out[3 * p] = normal_out[3 * p + 1] = normal_out[3 * p + 2] = 0.0f;
    return;
  }
  const float xc = (float)i + 0.5f, yc = (float)j + 0.5f;
  const float x = odd ? (float)A.S - xc : xc, y = odd ? (float)A.S - yc : yc;
  const float L = (float)(A.S - 4);
  float b1 = (x - 1.0f) / L, b2 = (y - 1.0f) / L;
  b1 = b1 > 0.0f ? b1 : 0.0f;
  b2 = b2 > 0.0f ? b2 : 0.0f;
  const float s = b1 + b2;
  if (s > 1.0f) b1 = b1 / s, b2 = b2 / s;
  float b0 = (1.0f - b1) - b2;
  b0 = b0 > 0.0f ? b0 : 0.0f;
  face_out[p] = (int32_t)f;
  bary_out[2 * p] = b1;
  bary_out[2 * p + 1] = b2;
  const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  for (int c = 0; c < 3; ++c) {
    const float t0 = b0 * verts[3 * i0 + c], t1 = b1 * verts[3 * i1 + c], t2 = b2 * verts[3 * i2 + c];
    position_out[3 * p + c] = (t0 + t1) + t2;
  }
  if (!normal_out) return;
  double g[3];
  if (vertex_normals) {
    for (int c = 0; c < 3; ++c) {
      const double t0 = (double)b0 * (double)vertex_normals[3 * i0 + c];
      const double t1 = (double)b1 * (double)vertex_normals[3 * i1 + c];
      const double t2 = (double)b2 * (double)vertex_normals[3 * i2 + c];
      g[c] = (t0 + t1) + t2;
    }
  } else {
    double a[3], b[3];
    for (int c = 0; c < 3; ++c) {
      const double o = (double)verts[3 * i0 + c];
      a[c] = (double)verts[3 * i1 + c] - o;
      b[c] = (double)verts[3 * i2 + c] - o;
    }
    const double x0 = a[1] * b[2], x1 = a[2] * b[1];
    const double y0 = a[2] * b[0], y1 = a[0] * b[2];
    const double z0 = a[0] * b[1], z1 = a[1] * b[0];
    g[0] = x0 - x1, g[1] = y0 - y1, g[2] = z0 - z1;
  }
  const double len = norm3(g);
  for (int c = 0; c < 3; ++c) normal_out[3 * p + c] = len == 0.0 ? 0.0f : (float)(g[c] / len);
}

// a float that holds an integer (or anything else) as an index in [0, hi]: compared in float before any conversion,
// a NaN gives 0
NERF_MT_HD int32_t clamp_index(float v, int32_t hi) { return v >= 0.0f ? (v <= (float)hi ? (int32_t)v : hi) : 0; }

// Lookup n: the texture at the point (u, v) of face f, C channels.  The UV inside the cell is the fp32 mix
// (w0 P0 + u P1) + v P2 of the face's corners with w0 = (1 - u) - v; the fetch is bilinear at (x - .5, y - .5): the
// floor and the fraction are taken inside the cell, the cell's origin is added to the integer part (exact), the four
// indices are clamped to [0, T - 1], and the blend is written as three lerps a + t (b - a), so that four equal texels
// return their value exactly.  face < 0 gives zeros.  The clamp keeps every read inside the texture whatever the
// face and the pair hold.
NERF_MT_HD void lookup(const Atlas& A, const float* __restrict__ texture, int C, const int32_t* __restrict__ face,
                       const float* __restrict__ bary, int64_t n, float* __restrict__ out) {
  const int64_t f = face[n];
  if (f < 0) {
    for (int c = 0; c < C; ++c) out[C * n + c] = 0.0f;
    return;
  }
  const float u = bary[2 * n], v = bary[2 * n + 1];
  const float w0 = (1.0f - u) - v;
  const int odd = (int)(f & 1);
  float px[3], py[3];
  for (int k = 0; k < 3; ++k) corner_uv(A.S, odd, k, px[k], py[k]);
  const float x0 = w0 * px[0], x1 = u * px[1], x2 = v * px[2];
  const float y0 = w0 * py[0], y1 = u * py[1], y2 = v * py[2];
  const float x = (x0 + x1) + x2, y = (y0 + y1) + y2;
  const float ax = x - 0.5f, ay = y - 0.5f;
  const float flx = floorf(ax), fly = floorf(ay);
  const float fx = ax - flx, fy = ay - fly;
  const int64_t cell = f >> 1;
  const float ox = (float)((cell % A.cols) * A.S), oy = (float)((cell / A.cols) * A.S);  // exact below 2^24
  const int64_t ix0 = clamp_index(flx + ox, A.T - 1), ix1 = clamp_index((flx + 1.0f) + ox, A.T - 1);
  const int64_t iy0 = clamp_index(fly + oy, A.T - 1), iy1 = clamp_index((fly + 1.0f) + oy, A.T - 1);
  const float* r0 = texture + iy0 * A.T * C;
  const float* r1 = texture + iy1 * A.T * C;
  for (int c = 0; c < C; ++c) {
    const float c00 = r0[ix0 * C + c], c10 = r0[ix1 * C + c], c01 = r1[ix0 * C + c], c11 = r1[ix1 * C + c];
    const float top = c00 + fx * (c10 - c00);
    const float bot = c01 + fx * (c11 - c01);
    out[C * n + c] = top + fy * (bot - top);
  }
}

}  // namespace nerf_mt
