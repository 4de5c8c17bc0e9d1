// Global coarsening on the host under AddressSanitizer + UBSan (CPU build only): the coarsening sequence of the adaptive
// stand-in meshes down to the root cell (mfgpu_mesh_coarsen_leaves), every member built by mfgpu_mesh_create_from_leaves,
// the map between consecutive members (mfgpu_mesh_coarsening_map) checked in place, and the inputs the calls refuse.
// Built and run by tests/test_gc_sanitizers.py.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "mfgpu.h"

static int bad = 0;
static void expect(bool ok, const char *what) {
  if (!ok) {
    std::printf("FAILED: %s (%s)\n", what, mfgpu_last_error());
    ++bad;
  }
}

static void run_sequence(int dim, int degree, mfgpu_mesh *fine) {
  while (fine) {
    const uint32_t *lv = nullptr;
    const int64_t cnt = mfgpu_mesh_cell_levels(fine, &lv);
    const uint32_t n_fine = (uint32_t)(cnt / 4);
    if (n_fine <= 1) break;
    std::vector<uint32_t> out((size_t)n_fine * 4);
    const int64_t n_coarse = mfgpu_mesh_coarsen_leaves(dim, lv, n_fine, out.data());
    expect(n_coarse >= 1 && n_coarse < (int64_t)n_fine, "coarsen_leaves makes the set smaller");
    if (n_coarse < 1) break;
    mfgpu_mesh *coarse = nullptr;
    expect(mfgpu_mesh_create_from_leaves(dim, degree, out.data(), (uint32_t)n_coarse, 0, &coarse) == 0, "from_leaves accepts it");
    if (!coarse) break;
    std::vector<uint32_t> parent(n_fine), child(n_fine), seen((size_t)n_coarse, 0);
    expect(mfgpu_mesh_coarsening_map(coarse, fine, parent.data(), child.data()) == 0, "coarsening_map");
    const uint32_t *cl = nullptr;
    mfgpu_mesh_cell_levels(coarse, &cl);
    bool ok = true;
    for (uint32_t f = 0; f < n_fine && ok; ++f) {
      ok = parent[f] < (uint32_t)n_coarse && child[f] <= (1u << dim);
      if (!ok) break;
      const uint32_t *c = cl + 4 * (size_t)parent[f], *l = lv + 4 * (size_t)f;
      if (child[f] == 0) {
        ok = c[0] == l[0] && c[1] == l[1] && c[2] == l[2] && c[3] == l[3];
      } else {
        const uint32_t k = child[f] - 1;
        ok = c[0] + 1 == l[0];
        for (int d = 0; d < 3; ++d) ok = ok && c[1 + d] == (l[1 + d] >> 1) && ((k >> d) & 1u) == (l[1 + d] & 1u);
      }
      seen[parent[f]] += 1;
    }
    for (int64_t c = 0; c < n_coarse && ok; ++c) ok = seen[c] == 1 || seen[c] == (1u << dim);
    expect(ok, "the map matches the coordinates and every coarse cell is itself or all its children");
    std::printf("  dim %d: %u -> %ld cells\n", dim, n_fine, (long)n_coarse);
    mfgpu_mesh_destroy(fine);
    fine = coarse;
  }
  mfgpu_mesh_destroy(fine);
}

int main() {
  for (int dim = 2; dim <= 3; ++dim)
    for (int n_ref = 2; n_ref <= 4; ++n_ref) {
      mfgpu_mesh *m = nullptr;
      expect(mfgpu_mesh_create_adaptive(dim, dim == 2 ? 2 : 1, n_ref, 0, &m) == 0, "create_adaptive");
      std::printf("adaptive dim %d n_ref %d\n", dim, n_ref);
      run_sequence(dim, dim == 2 ? 2 : 1, m);
      expect(mfgpu_mesh_create_adaptive_mg(dim, 1, n_ref, 0, &m) == 0, "create_adaptive_mg");
      run_sequence(dim, 1, m);
    }
  // what the calls refuse
  std::vector<uint32_t> out(64);
  const uint32_t root[4] = {0, 0, 0, 0};
  expect(mfgpu_mesh_coarsen_leaves(2, root, 1, out.data()) == MFGPU_EINVAL, "the root cell is refused");
  const uint32_t four[16] = {1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 0};
  expect(mfgpu_mesh_coarsen_leaves(2, four, 4, out.data()) == 1 && out[0] == 0, "four children become the root");
  expect(mfgpu_mesh_coarsen_leaves(2, four, 3, out.data()) == MFGPU_EINVAL, "a hole is refused");
  const uint32_t twice[20] = {1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0};
  expect(mfgpu_mesh_coarsen_leaves(2, twice, 5, out.data()) == MFGPU_EINVAL, "a leaf listed twice is refused");
  const uint32_t deep[4] = {40, 0, 0, 0};
  expect(mfgpu_mesh_coarsen_leaves(3, deep, 1, out.data()) == MFGPU_EINVAL, "a level beyond the key's range is refused");
  const uint32_t outside[16] = {1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 5, 1, 0};
  expect(mfgpu_mesh_coarsen_leaves(2, outside, 4, out.data()) == MFGPU_EINVAL, "a leaf outside the root cell is refused");
  expect(mfgpu_mesh_coarsen_leaves(2, nullptr, 4, out.data()) == MFGPU_EINVAL, "null leaves are refused");
  mfgpu_mesh *a = nullptr, *b = nullptr;
  uint32_t n3[3] = {2, 2, 1};
  expect(mfgpu_mesh_create_adaptive(2, 1, 3, 0, &a) == 0 && mfgpu_mesh_create_uniform(2, 1, n3, -1, 1, 0, 0, 0, &b) == 0, "meshes");
  std::vector<uint32_t> parent(4096), child(4096);
  expect(mfgpu_mesh_coarsening_map(b, a, parent.data(), child.data()) == MFGPU_EINVAL, "a cube is no leaf mesh");
  expect(mfgpu_mesh_coarsening_map(a, nullptr, parent.data(), child.data()) == MFGPU_EINVAL, "null mesh");
  mfgpu_mesh_destroy(a);
  mfgpu_mesh_destroy(b);
  std::printf("done bad=%d\n", bad);
  return bad != 0;
}
