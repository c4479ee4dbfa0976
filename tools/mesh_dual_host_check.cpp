// Host check of csrc/mesh_dual_core.hpp (dual contouring): classify_point, edges_point and
// cells_point run serially, one call per lattice point exactly as the kernels run them (one call per thread), on small
// lattices: one cell, axes too thin for interior edges, random fields and integer fields whose values meet iso.  Every
// output array has exactly its size, so a slot written out of range is caught by the sanitizer; every slot is
// checked to have been written once; the Hermite points are compared with emit_point's vertices bit for bit; every
// vertex must lie in its cell and every face index below V.  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/mesh_dual_host_check.cpp -o mesh_dual_host_check && ./mesh_dual_host_check
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
#include <cstdio>
#include <cstring>

#include "mesh_host_check_common.hpp"

#include "../nerf-sys_amd/csrc/mesh_dual_core.hpp"

namespace {

using nerf_mesh::Lattice;

std::vector<int32_t> scan(const std::vector<int32_t>& c) {
  std::vector<int32_t> o(c.size() + 1, 0);
  for (size_t i = 0; i < c.size(); ++i) o[i + 1] = o[i] + c[i];
  return o;
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

bool run_case(const char* name, int nx, int ny, int nz, const std::vector<float>& field, float iso) {
  Lattice L{nx, ny, nz, iso, {-1.0f, -0.8f, -0.6f}, {0.f, 0.f, 0.f}};
  const float hi[3] = {1.0f, 0.9f, 0.7f};
  const int n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) L.h[a] = (hi[a] - L.lo[a]) / (float)(n[a] - 1);
  const int64_t P = (int64_t)nx * ny * nz;
  bool ok = true;
  auto fail = [&](const char* what) {
    std::printf("%s (%d,%d,%d): %s\n", name, nx, ny, nz, what);
    ok = false;
  };

  std::vector<uint8_t> mask((size_t)P), tmask((size_t)P);
  std::vector<int32_t> ec((size_t)P), cc((size_t)P), fc((size_t)P), tvc((size_t)P), tfc((size_t)P);
  for (int64_t p = 0; p < P; ++p) {
    const int ix = (int)(p / ((int64_t)ny * nz)), iy = (int)(p / nz % ny), iz = (int)(p % nz);
    int e, c, f, tf;
    nerf_dual::classify_point(field.data(), L, ix, iy, iz, p, mask[p], e, c, f);
    ec[p] = e, cc[p] = c, fc[p] = f;
    nerf_mesh::classify_point(field.data(), L, ix, iy, iz, p, tmask[p], tf);
    tvc[p] = nerf_mesh::popc(tmask[p]), tfc[p] = tf;
    // the dual mask is marching tetrahedra's at the classes 1, 2 and 4
    const unsigned want = (tmask[p] & 1u) | ((tmask[p] >> 1) & 1u) << 1 | ((tmask[p] >> 3) & 1u) << 2;
    if (mask[p] != want) fail("edge mask differs from marching tetrahedra's axis classes");
    if ((c != 0) != (tf != 0)) fail("a cell is active iff marching tetrahedra cuts it");
  }
  const std::vector<int32_t> eoff = scan(ec), coff = scan(cc), foff = scan(fc), tvoff = scan(tvc), tfoff = scan(tfc);
  const int64_t E = eoff[P], V = coff[P], F = foff[P], TV = tvoff[P], TF = tfoff[P];

  // marching tetrahedra's vertices, for the bits of the Hermite points
  std::vector<float> tv((size_t)(3 * TV)), tn((size_t)(3 * TV));
  std::vector<int32_t> tf((size_t)(3 * TF));
  for (int64_t p = 0; p < P; ++p) {
    const int ix = (int)(p / ((int64_t)ny * nz)), iy = (int)(p / nz % ny), iz = (int)(p % nz);
    nerf_mesh::emit_point(field.data(), L, ix, iy, iz, p, tmask.data(), tvoff.data(), tfoff.data(), TV, TF, tv.data(),
                          tf.data(), tn.data());
  }

  const float unset = -12345.0f;
  std::vector<float> pts((size_t)(3 * E), unset), nrm((size_t)(3 * E), unset);
  std::vector<int32_t> keys((size_t)E, -1);
  for (int64_t p = 0; p < P; ++p) {
    const int ix = (int)(p / ((int64_t)ny * nz)), iy = (int)(p / nz % ny), iz = (int)(p % nz);
    nerf_dual::edges_point(field.data(), L, ix, iy, iz, p, mask.data(), eoff.data(), E, pts.data(), nrm.data(),
                           keys.data());
  }
  for (int64_t e = 0; e < E; ++e) {
    if (keys[e] < 0 || (e > 0 && keys[e] <= keys[e - 1])) fail("keys must ascend");
    const int64_t p = keys[e] / 3;
    const int a = keys[e] % 3, d = 1 << a;
    const int64_t t = tvoff[p] + nerf_mesh::popc(tmask[p] & ((1u << (d - 1)) - 1u));
    for (int k = 0; k < 3; ++k) {
      if (!same_bits(pts[3 * e + k], tv[3 * t + k])) fail("Hermite point differs from marching tetrahedra's vertex");
      if (!same_bits(nrm[3 * e + k], tn[3 * t + k])) fail("Hermite normal differs from marching tetrahedra's");
    }
  }

  for (int placement = 0; placement < 2; ++placement) {
    std::vector<float> verts((size_t)(3 * V), unset), vn((size_t)(3 * V), unset);
    std::vector<int32_t> faces((size_t)(3 * F), -1);
    std::vector<uint8_t> fb((size_t)V, 9);
    for (int64_t p = 0; p < P; ++p) {
      const int ix = (int)(p / ((int64_t)ny * nz)), iy = (int)(p / nz % ny), iz = (int)(p % nz);
      nerf_dual::cells_point(field.data(), L, ix, iy, iz, p, P, mask.data(), eoff.data(), coff.data(), foff.data(),
                             pts.data(), nrm.data(), placement, 1e-3, V, F, verts.data(), faces.data(), vn.data(),
                             fb.data());
    }
    for (int64_t p = 0; p < P; ++p) {
      if (!cc[p]) continue;
      const int i[3] = {(int)(p / ((int64_t)ny * nz)), (int)(p / nz % ny), (int)(p % nz)};
      const int64_t v = coff[p];
      if (fb[v] > 1 || (placement == 0 && fb[v] != 0)) fail("fallback byte");
      double len = 0.0;
      for (int k = 0; k < 3; ++k) {
        const float a = L.lo[k] + (float)i[k] * L.h[k], b = L.lo[k] + (float)(i[k] + 1) * L.h[k];
        const float slack = 4e-7f * (std::fabs(a) + std::fabs(b) + L.h[k]);  // the roundings of pa + t h and of the points
        if (!(verts[3 * v + k] >= a - slack && verts[3 * v + k] <= b + slack)) fail("a vertex left its cell");
        len += (double)vn[3 * v + k] * vn[3 * v + k];
      }
      if (!(len < 1.0 + 1e-5)) fail("vertex normal longer than one");
    }
    for (int64_t f = 0; f < 3 * F; ++f)
      if (faces[f] < 0 || faces[f] >= V) fail("face index out of range or unwritten");
    for (int64_t f = 0; f < F; ++f)
      if (faces[3 * f] == faces[3 * f + 1] || faces[3 * f + 1] == faces[3 * f + 2] || faces[3 * f] == faces[3 * f + 2])
        fail("a quad's four cells must differ");
  }
  return ok;
}

}  // namespace

int main() {
  std::mt19937 rng(5);
  const int shapes[][3] = {{2, 2, 2}, {3, 3, 3}, {5, 4, 3}, {3, 2, 9}, {2, 7, 2}, {7, 6, 5}, {9, 8, 10}};
  bool ok = true;
  for (const auto& s : shapes) {
    const int64_t P = (int64_t)s[0] * s[1] * s[2];
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::uniform_int_distribution<int> iv(-2, 2);
    std::vector<float> noise((size_t)P), ints((size_t)P), all_in((size_t)P, 1.0f), all_out((size_t)P, -1.0f);
    for (auto& x : noise) x = u(rng);
    for (auto& x : ints) x = (float)iv(rng);
    ok &= run_case("noise", s[0], s[1], s[2], noise, 0.0f);
    ok &= run_case("noise, iso 0.5", s[0], s[1], s[2], noise, 0.5f);
    ok &= run_case("integers", s[0], s[1], s[2], ints, 0.0f);
    ok &= run_case("all inside", s[0], s[1], s[2], all_in, 0.0f);
    ok &= run_case("all outside", s[0], s[1], s[2], all_out, 0.0f);
  }
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
