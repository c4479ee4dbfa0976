// Host check of csrc/mesh_quadric_core.hpp (quadric placement): the cyclic Jacobi eigenpairs on
// random symmetric, rank-1, rank-2, diagonal and zero matrices, the truncated solve on one, two and three planes in
// the cell's frame against the projection it must equal, and place_vertex on small clusters (one plane, an edge, a
// corner, an empty row, a row of zero-area faces, a solution outside the cell, a row that is no representative), run
// serially exactly as the kernel runs them (one call per thread).  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/mesh_quadric_host_check.cpp -o mesh_quadric_host_check && ./mesh_quadric_host_check
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_quadric_core.hpp"

namespace {

using nerf_mq::Eigen;
using nerf_mq::Quadric;

struct M3 {
  double a[3][3];
};

Quadric quadric_of(const M3& m) {
  Quadric q = nerf_mq::zero_quadric();
  q.a00 = m.a[0][0], q.a01 = m.a[0][1], q.a02 = m.a[0][2], q.a11 = m.a[1][1], q.a12 = m.a[1][2], q.a22 = m.a[2][2];
  return q;
}

// A e = l e within 1e-12 |A| (largest entry) and E^T E = 1 within 1e-14
bool eigen_check(const char* name, const M3& m) {
  const Eigen e = nerf_mq::jacobi(quadric_of(m));
  const double l[3] = {e.l0, e.l1, e.l2};
  const double v[3][3] = {{e.e00, e.e01, e.e02}, {e.e10, e.e11, e.e12}, {e.e20, e.e21, e.e22}};  // v[j][i]: column i
  double norm = 0.0, res = 0.0, orth = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) norm = std::max(norm, std::fabs(m.a[i][j]));
  for (int i = 0; i < 3; ++i) {
    for (int r = 0; r < 3; ++r) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += m.a[r][k] * v[k][i];
      res = std::max(res, std::fabs(s - l[i] * v[r][i]));
    }
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += v[k][i] * v[k][j];
      orth = std::max(orth, std::fabs(s - (i == j ? 1.0 : 0.0)));
    }
  }
  const bool ok = res <= 1e-12 * norm && orth <= 1e-14;
  if (!ok) std::printf("%s: residual %.3g of |A| = %.3g, orthonormality %.3g\n", name, res, norm, orth);
  return ok;
}

M3 outer_sum(const double u[3], const double w[3], double ww) {
  M3 m;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m.a[i][j] = u[i] * u[j] + ww * w[i] * w[j];
  return m;
}

bool eigen_cases() {
  std::mt19937 rng(7);
  std::normal_distribution<double> nrm(0.0, 1.0);
  bool ok = true;
  for (int k = 0; k < 3000; ++k) {
    const double scale = std::pow(10.0, (double)((int)(rng() % 13) - 6));
    M3 m;
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j) m.a[i][j] = m.a[j][i] = nrm(rng) * scale;
    ok &= eigen_check("random symmetric", m);
    const double u[3] = {nrm(rng), nrm(rng), nrm(rng)}, w[3] = {nrm(rng), nrm(rng), nrm(rng)};
    ok &= eigen_check("rank 1", outer_sum(u, w, 0.0));
    ok &= eigen_check("rank 2", outer_sum(u, w, 1.0));
    M3 d = {};
    for (int i = 0; i < 3; ++i) d.a[i][i] = nrm(rng) * scale;
    ok &= eigen_check("diagonal", d);
  }
  const M3 zero = {};
  ok &= eigen_check("zero", zero);
  const Eigen e = nerf_mq::jacobi(quadric_of(zero));
  if (e.l0 != 0.0 || e.l1 != 0.0 || e.l2 != 0.0 || e.e00 != 1.0 || e.e11 != 1.0 || e.e22 != 1.0 || e.e01 != 0.0) {
    std::printf("zero matrix: the eigenvectors must stay the identity\n");
    ok = false;
  }
  M3 tiny = {};  // theta * theta overflows: the rotation is the identity
  tiny.a[0][0] = 1.0, tiny.a[1][1] = 2.0, tiny.a[2][2] = 3.0, tiny.a[0][1] = tiny.a[1][0] = 1e-200;
  ok &= eigen_check("tiny off-diagonal", tiny);
  return ok;
}

// ---------------------------------------------------------------- the solve against the projection it must equal

void cross(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
}

double dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// a random rotation: three orthonormal rows
void rotation(std::mt19937& rng, double r[3][3]) {
  std::normal_distribution<double> nrm(0.0, 1.0);
  double a[3] = {nrm(rng), nrm(rng), nrm(rng)}, b[3] = {nrm(rng), nrm(rng), nrm(rng)};
  const double la = std::sqrt(dot(a, a));
  for (double& x : a) x /= la;
  const double ab = dot(a, b);
  for (int i = 0; i < 3; ++i) b[i] -= ab * a[i];
  const double lb = std::sqrt(dot(b, b));
  for (double& x : b) x /= lb;
  double c[3];
  cross(a, b, c);
  for (int i = 0; i < 3; ++i) r[0][i] = a[i], r[1][i] = b[i], r[2][i] = c[i];
}

// `planes` planes through x0 with the normals r[0..planes), two triangles each; the expected point is xbar with its
// components along those normals replaced by x0's
bool solve_case(std::mt19937& rng, int planes) {
  std::uniform_real_distribution<double> in(-0.3, 0.3), size(0.2, 5.0);
  double r[3][3];
  rotation(rng, r);
  const double x0[3] = {in(rng), in(rng), in(rng)}, xbar[3] = {in(rng), in(rng), in(rng)};
  Quadric q = nerf_mq::zero_quadric();
  for (int p = 0; p < planes; ++p)
    for (int t = 0; t < 2; ++t) {
      const double* s1 = r[(p + 1) % 3];
      const double* s2 = r[(p + 2) % 3];
      double a[3], b[3], c[3];
      const double ea = size(rng), eb = size(rng), ec = size(rng), fa = size(rng);
      for (int i = 0; i < 3; ++i) {
        a[i] = x0[i] - ea * s1[i] + fa * s2[i];
        b[i] = x0[i] + eb * s1[i];
        c[i] = x0[i] + ec * s2[i] * (t ? -1.0 : 1.0);
      }
      nerf_mq::add_face(q, a, b, c);
    }
  double want[3] = {xbar[0], xbar[1], xbar[2]};
  for (int p = 0; p < planes; ++p) {
    const double diff[3] = {x0[0] - want[0], x0[1] - want[1], x0[2] - want[2]};
    const double k = dot(r[p], diff);
    for (int i = 0; i < 3; ++i) want[i] += k * r[p][i];
  }
  double x[3] = {0.0, 0.0, 0.0};
  const bool placed = nerf_mq::solve(q, xbar, 1e-3, x);
  bool inside = true;
  for (double w : want) inside = inside && std::fabs(w) < 0.499;
  double err = 0.0;
  for (int i = 0; i < 3; ++i) err = std::max(err, std::fabs(x[i] - want[i]));
  if ((inside && !placed) || (placed && err > 1e-9)) {
    std::printf("solve with %d planes: placed %d, error %.3g\n", planes, (int)placed, err);
    return false;
  }
  return true;
}

bool solve_cases() {
  std::mt19937 rng(11);
  bool ok = true;
  for (int k = 0; k < 2000; ++k)
    for (int planes = 1; planes <= 3; ++planes) ok &= solve_case(rng, planes);
  // no face at all, and three planes that meet outside the cell: the mean is kept
  const double xbar[3] = {0.1, -0.2, 0.3};
  double x[3] = {0.0, 0.0, 0.0};
  if (nerf_mq::solve(nerf_mq::zero_quadric(), xbar, 1e-3, x)) ok = false, std::printf("empty quadric placed\n");
  Quadric q = nerf_mq::zero_quadric();
  const double o[3] = {0.7, 0.0, 0.0}, ex[3] = {1.7, 0.0, 0.0}, ey[3] = {0.7, 1.0, 0.0}, ez[3] = {0.7, 0.0, 1.0};
  nerf_mq::add_face(q, o, ex, ey);
  nerf_mq::add_face(q, o, ey, ez);
  nerf_mq::add_face(q, o, ez, ex);
  if (nerf_mq::solve(q, xbar, 1e-3, x)) ok = false, std::printf("a corner outside the cell was accepted\n");
  // a NaN corner poisons the quadric: not placed, nothing trapped
  Quadric bad = nerf_mq::zero_quadric();
  const double nan3[3] = {NAN, 0.0, 0.0};
  nerf_mq::add_face(bad, o, ex, ey);
  bad.a00 = NAN;
  if (nerf_mq::solve(bad, xbar, 1e-3, x)) ok = false, std::printf("a NaN quadric was accepted\n");
  nerf_mq::add_face(bad, nan3, ex, ey);  // L is a NaN: skipped
  return ok;
}

// ---------------------------------------------------------------- place_vertex on small clusters

struct Mesh {
  std::vector<float> v;
  std::vector<int32_t> f, labels, row_off, col;
};

// labels by the cell keys (the smallest index of a cell), rows = the faces with a corner in the cluster, ascending
void finish(Mesh& m, const nerf_grid::Grid& g) {
  const int64_t V = (int64_t)m.v.size() / 3, F = (int64_t)m.f.size() / 3;
  m.labels.assign((size_t)V, -1);
  std::vector<int64_t> key((size_t)V);
  for (int64_t i = 0; i < V; ++i) {
    key[i] = nerf_grid::cell_id(g, nerf_grid::cell_index(g, 0, m.v[3 * i]), nerf_grid::cell_index(g, 1, m.v[3 * i + 1]),
                                nerf_grid::cell_index(g, 2, m.v[3 * i + 2]));
    for (int64_t j = 0; j <= i; ++j)
      if (key[j] == key[i]) {
        m.labels[i] = (int32_t)j;
        break;
      }
  }
  std::vector<std::set<int32_t>> rows((size_t)V);
  for (int64_t f = 0; f < F; ++f)
    for (int c = 0; c < 3; ++c) rows[m.labels[m.f[3 * f + c]]].insert((int32_t)f);
  m.row_off.assign(1, 0);
  m.col.clear();
  for (const auto& r : rows) {
    m.col.insert(m.col.end(), r.begin(), r.end());
    m.row_off.push_back((int32_t)m.col.size());
  }
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

bool place_cases() {
  nerf_grid::Grid g;
  g.lo[0] = g.lo[1] = g.lo[2] = 0.0f;
  g.cell = 1.0f, g.inv = 1.0f;
  g.dims[0] = g.dims[1] = g.dims[2] = 4;
  // the corner P = vertex 0 of a box that extends towards the origin, vertex 7 a second member of P's cell on the top
  // plane; faces 0-2 lie in z = 1.4, 3-4 in y = 1.6, 5-6 in x = 1.3, face 7 has zero area, face 8 a repeated corner
  const std::vector<float> verts = {1.3f, 1.6f, 1.4f, 0.3f, 1.6f, 1.4f, 1.3f, 0.6f, 1.4f, 1.3f, 1.6f, 0.4f,
                                    0.3f, 0.6f, 1.4f, 0.3f, 1.6f, 0.4f, 1.3f, 0.6f, 0.4f, 1.1f, 1.2f, 1.4f,
                                    3.5f, 3.5f, 3.5f};  // vertex 8: a cell of its own that no face of positive area touches
  const std::vector<int32_t> top = {0, 1, 4, 0, 4, 2, 7, 4, 2}, side_y = {0, 3, 5, 0, 5, 1}, side_x = {0, 2, 6, 0, 6, 3};
  const std::vector<int32_t> dead = {0, 7, 7, 8, 8, 8};
  const float mean0[3] = {1.2f, 1.4f, 1.45f};
  const double want[3][3] = {{1.2, 1.4, 1.4}, {1.2, 1.6, 1.4}, {1.3, 1.6, 1.4}};
  bool ok = true;
  for (int planes = 1; planes <= 3; ++planes) {
    Mesh m;
    m.v = verts;
    m.f = top;
    if (planes >= 2) m.f.insert(m.f.end(), side_y.begin(), side_y.end());
    if (planes >= 3) m.f.insert(m.f.end(), side_x.begin(), side_x.end());
    m.f.insert(m.f.end(), dead.begin(), dead.end());
    finish(m, g);
    const int64_t V = (int64_t)m.v.size() / 3;
    if (m.labels[7] != 0 || m.labels[8] != 8) ok = false, std::printf("labels of the test mesh\n");
    std::vector<float> mean(m.v), pos((size_t)(3 * V), -1.0f);
    std::vector<uint8_t> placed((size_t)V, 9);
    std::copy(mean0, mean0 + 3, mean.begin());
    mean[3 * 8] = -0.0f;  // a kept mean keeps its bits, the sign of a zero included
    for (int64_t r = 0; r < V; ++r)
      nerf_mq::place_vertex(m.v.data(), m.f.data(), m.labels.data(), m.row_off.data(), m.col.data(), mean.data(), g,
                            1e-3, r, pos.data(), placed.data());
    for (int c = 0; c < 3; ++c)
      if (placed[0] != 1 || std::fabs((double)pos[c] - want[planes - 1][c]) > 1e-6) {
        std::printf("%d planes: axis %d gives %.9g, expected %.9g (placed %d)\n", planes, c, pos[c],
                    want[planes - 1][c], (int)placed[0]);
        ok = false;
      }
    // vertex 7 is no representative: zeros; vertex 8 has only a face of zero area: the mean's bits
    if (placed[7] != 0 || pos[21] != 0.0f || pos[22] != 0.0f || pos[23] != 0.0f) ok = false, std::printf("row 7\n");
    for (int c = 0; c < 3; ++c)
      if (placed[8] != 0 || !same_bits(pos[24 + c], mean[24 + c])) ok = false, std::printf("all-degenerate row\n");
  }
  {
    // every vertex its own cell.  Vertices 0 and 6 are used by no face (empty rows), vertex 1 only by the face
    // (1,1,1); the other three faces lie in the planes x = 1.2, z = 0.1 and y = 0.1 and meet at vertex 2
    Mesh m;
    m.v = {0.5f, 0.5f, 0.5f, 2.5f, 0.5f, 0.5f, 1.2f, 0.1f, 0.1f, 1.2f, 2.1f, 0.1f, 1.2f, 0.1f, 2.1f,
           3.1f, 0.1f, 0.1f, 0.1f, 2.2f, 0.1f};
    m.f = {2, 3, 4, 2, 5, 3, 2, 4, 5, 1, 1, 1};
    finish(m, g);
    const int64_t V = (int64_t)m.v.size() / 3;
    std::vector<float> mean(m.v), pos((size_t)(3 * V), -1.0f);
    std::vector<uint8_t> placed((size_t)V, 9);
    for (int64_t r = 0; r < V; ++r)
      nerf_mq::place_vertex(m.v.data(), m.f.data(), m.labels.data(), m.row_off.data(), m.col.data(), mean.data(), g,
                            1e-3, r, pos.data(), placed.data());
    if (m.row_off[1] != m.row_off[0] || placed[0] != 0 || !same_bits(pos[0], 0.5f)) ok = false, std::printf("empty row\n");
    // vertex 2 at (1.2, 0.1, 0.1) is the corner itself: accepted, and exactly there
    if (placed[2] != 1 || std::fabs(pos[6] - 1.2f) > 1e-6f || std::fabs(pos[7] - 0.1f) > 1e-6f) {
      std::printf("corner at the vertex: %.9g %.9g %.9g placed %d\n", pos[6], pos[7], pos[8], (int)placed[2]);
      ok = false;
    }
    // vertex 5 at (3.1, 0.1, 0.1) sees the planes y = 0.1 and z = 0.1 only: it stays on that edge, at its own x
    if (placed[5] != 1 || std::fabs(pos[15] - 3.1f) > 1e-6f || std::fabs(pos[16] - 0.1f) > 1e-6f) {
      std::printf("edge vertex: %.9g %.9g %.9g placed %d\n", pos[15], pos[16], pos[17], (int)placed[5]);
      ok = false;
    }
    // vertex 1 has only a face of zero area: kept
    if (placed[1] != 0 || !same_bits(pos[3], 2.5f)) ok = false, std::printf("degenerate face row\n");
  }
  return ok;
}

}  // namespace

int main() {
  bool ok = eigen_cases();
  ok &= solve_cases();
  ok &= place_cases();
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
