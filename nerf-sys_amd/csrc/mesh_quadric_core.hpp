// Quadric-error placement of a cluster's vertex ("Quadric placement"): the plane quadric of the faces
// that touch a cluster, the cyclic Jacobi eigen-decomposition of its 3x3 matrix and the truncated solve that starts at
// the members' mean, written once for the device and for a host compiler so that every loop can be run and checked
// under a host sanitizer without a GPU.  Build with -ffp-contract=off: every double operation below rounds on its own,
// in the order written, and tests/mesh_quadric_reference.py restates them one by one.
//
// The frame.  All of it happens in the cell's own coordinates: the cell of the representative is the box
// [-0.5, 0.5]^3, c = lo + (i + 0.5) cell its centre, y = (p - c) / cell.  The eigenvalue threshold and the guard are
// therefore independent of the mesh's scale.
//
// The state is nine plus nine named doubles (the symmetric matrix, the right-hand side, the eigenvectors); the three
// Jacobi pairs are written out, so nothing is indexed by a run-time value and nothing goes to scratch.
#pragma once
#include "mesh_grid_core.hpp"

#define NERF_MQ_HD NERF_GRID_HD

namespace nerf_mq {

using nerf_grid::Grid;

constexpr int SWEEPS = 8;

// A (symmetric, 6 entries) and b of the quadric x^T A x + 2 b^T x + const
struct Quadric {
  double a00, a01, a02, a11, a12, a22;
  double b0, b1, b2;
};

// the eigenvalues l_i and the eigenvectors (column i: e0i, e1i, e2i)
struct Eigen {
  double l0, l1, l2;
  double e00, e01, e02, e10, e11, e12, e20, e21, e22;
};

NERF_MQ_HD Quadric zero_quadric() { return Quadric{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// the centre of cell i on axis c
NERF_MQ_HD double cell_centre(const Grid& g, int c, int32_t i) {
  const double cells = (double)i + 0.5;
  const double off = cells * (double)g.cell;
  return (double)g.lo[c] + off;
}

// the local coordinate of the world coordinate p
NERF_MQ_HD double to_local(const Grid& g, double centre, float p) {
  const double d = (double)p - centre;
  return d / (double)g.cell;
}

// One face with the local corners a, b, c: n = (b - a) x (c - a), L = |n| (twice the area), m = n / L,
// d = -(m . a); A += L m m^T, b += (L d) m.  A face with L == 0 (or a NaN) adds nothing.
NERF_MQ_HD void add_face(Quadric& q, const double a[3], const double b[3], const double c[3]) {
  const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];
  const double w0 = c[0] - a[0], w1 = c[1] - a[1], w2 = c[2] - a[2];
  const double x0 = u1 * w2, x1 = u2 * w1;
  const double y0 = u2 * w0, y1 = u0 * w2;
  const double z0 = u0 * w1, z1 = u1 * w0;
  const double nx = x0 - x1, ny = y0 - y1, nz = z0 - z1;
  const double xx = nx * nx, yy = ny * ny, zz = nz * nz;
  const double L = sqrt((xx + yy) + zz);
  if (!(L > 0.0)) return;
  const double mx = nx / L, my = ny / L, mz = nz / L;
  const double dx = mx * a[0], dy = my * a[1], dz = mz * a[2];
  const double d = -((dx + dy) + dz);
  const double mxx = mx * mx, mxy = mx * my, mxz = mx * mz, myy = my * my, myz = my * mz, mzz = mz * mz;
  q.a00 = q.a00 + L * mxx;
  q.a01 = q.a01 + L * mxy;
  q.a02 = q.a02 + L * mxz;
  q.a11 = q.a11 + L * myy;
  q.a12 = q.a12 + L * myz;
  q.a22 = q.a22 + L * mzz;
  const double Ld = L * d;
  q.b0 = q.b0 + Ld * mx;
  q.b1 = q.b1 + Ld * my;
  q.b2 = q.b2 + Ld * mz;
}

// One plane through the local point y with the direction m (any length): L = |m|, u = m / L, d = -(u . y);
// A += u u^T, b += d u (unit weight: dual contouring's Hermite planes, mesh_dual_core.hpp).  A direction with
// L == 0 (or a NaN) adds nothing.
NERF_MQ_HD void add_plane(Quadric& q, const double m[3], const double y[3]) {
  const double xx = m[0] * m[0], yy = m[1] * m[1], zz = m[2] * m[2];
  const double L = sqrt((xx + yy) + zz);
  if (!(L > 0.0)) return;
  const double ux = m[0] / L, uy = m[1] / L, uz = m[2] / L;
  const double dx = ux * y[0], dy = uy * y[1], dz = uz * y[2];
  const double d = -((dx + dy) + dz);
  q.a00 = q.a00 + ux * ux;
  q.a01 = q.a01 + ux * uy;
  q.a02 = q.a02 + ux * uz;
  q.a11 = q.a11 + uy * uy;
  q.a12 = q.a12 + uy * uz;
  q.a22 = q.a22 + uz * uz;
  q.b0 = q.b0 + d * ux;
  q.b1 = q.b1 + d * uy;
  q.b2 = q.b2 + d * uz;
}

// One Jacobi rotation of the pair (p, q); r is the third index.  apq == 0 leaves everything as it is.  theta * theta
// may overflow to +inf: then t = +-0, c = 1, s = +-0 and the rotation is the identity.
NERF_MQ_HD void rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                       double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double diff = aqq - app;
  const double twice = 2.0 * apq;
  const double theta = diff / twice;
  const double th2 = theta * theta;
  const double root = sqrt(th2 + 1.0);
  const double den = fabs(theta) + root;
  const double tp = 1.0 / den;
  const double t = theta < 0.0 ? -tp : tp;  // sgn(0) = +1
  const double t2 = t * t;
  const double c = 1.0 / sqrt(t2 + 1.0);
  const double s = t * c;
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  const double cp = c * arp, sq = s * arq, sp = s * arp, cq = c * arq;
  arp = cp - sq;
  arq = sp + cq;
  const double c0p = c * v0p, s0q = s * v0q, s0p = s * v0p, c0q = c * v0q;
  v0p = c0p - s0q;
  v0q = s0p + c0q;
  const double c1p = c * v1p, s1q = s * v1q, s1p = s * v1p, c1q = c * v1q;
  v1p = c1p - s1q;
  v1q = s1p + c1q;
  const double c2p = c * v2p, s2q = s * v2q, s2p = s * v2p, c2q = c * v2q;
  v2p = c2p - s2q;
  v2q = s2p + c2q;
}

// Cyclic Jacobi on the symmetric matrix of q: SWEEPS sweeps over the pairs (0,1), (0,2), (1,2), a fixed trip count.
NERF_MQ_HD Eigen jacobi(const Quadric& q) {
  double a00 = q.a00, a01 = q.a01, a02 = q.a02, a11 = q.a11, a12 = q.a12, a22 = q.a22;
  Eigen e;
  e.e00 = 1.0, e.e01 = 0.0, e.e02 = 0.0;
  e.e10 = 0.0, e.e11 = 1.0, e.e12 = 0.0;
  e.e20 = 0.0, e.e21 = 0.0, e.e22 = 1.0;
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
    rotate(a00, a11, a01, a02, a12, e.e00, e.e01, e.e10, e.e11, e.e20, e.e21);
    rotate(a00, a22, a02, a01, a12, e.e00, e.e02, e.e10, e.e12, e.e20, e.e22);
    rotate(a11, a22, a12, a01, a02, e.e01, e.e02, e.e11, e.e12, e.e21, e.e22);
  }
  e.l0 = a00, e.l1 = a11, e.l2 = a22;
  return e;
}

// x += ((e . g) / l) e for one eigenpair with l > cut
NERF_MQ_HD void step(double l, double cut, double e0, double e1, double e2, double g0, double g1, double g2,
                     double x[3]) {
  if (!(l > cut)) return;
  const double p0 = e0 * g0, p1 = e1 * g1, p2 = e2 * g2;
  const double k = ((p0 + p1) + p2) / l;
  x[0] = x[0] + k * e0;
  x[1] = x[1] + k * e1;
  x[2] = x[2] + k * e2;
}

// The minimiser of q closest to xbar along the directions the planes constrain (eigenvalues above tol * the largest),
// in local coordinates.  False (keep the mean) when the matrix is zero or not a number, or when the result is not
// finite or leaves the cell [-0.5, 0.5]^3.
NERF_MQ_HD bool solve(const Quadric& q, const double xbar[3], double tol, double x[3]) {
  const Eigen e = jacobi(q);
  const double m0 = fabs(e.l0), m1 = fabs(e.l1), m2 = fabs(e.l2);
  double lmax = m0;
  if (m1 > lmax) lmax = m1;
  if (m2 > lmax) lmax = m2;
  if (!(lmax > 0.0)) return false;
  const double r00 = q.a00 * xbar[0], r01 = q.a01 * xbar[1], r02 = q.a02 * xbar[2];
  const double r10 = q.a01 * xbar[0], r11 = q.a11 * xbar[1], r12 = q.a12 * xbar[2];
  const double r20 = q.a02 * xbar[0], r21 = q.a12 * xbar[1], r22 = q.a22 * xbar[2];
  const double g0 = -q.b0 - ((r00 + r01) + r02);
  const double g1 = -q.b1 - ((r10 + r11) + r12);
  const double g2 = -q.b2 - ((r20 + r21) + r22);
  const double cut = tol * lmax;
  x[0] = xbar[0], x[1] = xbar[1], x[2] = xbar[2];
  step(e.l0, cut, e.e00, e.e10, e.e20, g0, g1, g2, x);
  step(e.l1, cut, e.e01, e.e11, e.e21, g0, g1, g2, x);
  step(e.l2, cut, e.e02, e.e12, e.e22, g0, g1, g2, x);
  bool ok = true;
  for (int c = 0; c < 3; ++c) ok = ok && x[c] >= -0.5 && x[c] <= 0.5;  // a NaN or an infinity fails
  return ok;
}

// Row r of the outputs.  A representative (labels[r] == r) walks its row of the vertex-to-face adjacency of the
// remapped faces in the row's order, one face after the other; every other row is zeros.  The loop is bounded by the
// row's length.
NERF_MQ_HD void place_vertex(const float* verts, const int32_t* faces, const int32_t* labels, const int32_t* row_off,
                             const int32_t* col, const float* mean, const Grid& g, double tol, int64_t r,
                             float* out_pos, uint8_t* out_placed) {
  if (labels[r] != (int32_t)r) {
    out_pos[3 * r] = 0.0f, out_pos[3 * r + 1] = 0.0f, out_pos[3 * r + 2] = 0.0f;
    out_placed[r] = 0;
    return;
  }
  double centre[3], xbar[3];
  for (int c = 0; c < 3; ++c) {
    centre[c] = cell_centre(g, c, nerf_grid::cell_index(g, c, verts[3 * r + c]));
    xbar[c] = to_local(g, centre[c], mean[3 * r + c]);
  }
  Quadric q = zero_quadric();
  for (int32_t k = row_off[r], end = row_off[r + 1]; k < end; ++k) {
    const int64_t f = col[k];
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    double a[3], b[3], cc[3];
    for (int c = 0; c < 3; ++c) {
      a[c] = to_local(g, centre[c], verts[3 * i0 + c]);
      b[c] = to_local(g, centre[c], verts[3 * i1 + c]);
      cc[c] = to_local(g, centre[c], verts[3 * i2 + c]);
    }
    add_face(q, a, b, cc);
  }
  double x[3] = {0.0, 0.0, 0.0};
  const bool placed = solve(q, xbar, tol, x);
  for (int c = 0; c < 3; ++c) {
    const double off = x[c] * (double)g.cell;
    out_pos[3 * r + c] = placed ? (float)(centre[c] + off) : mean[3 * r + c];
  }
  out_placed[r] = placed ? 1 : 0;
}

}  // namespace nerf_mq
