// Adaptive refinement on the host under AddressSanitizer + UBSan (CPU build only): refinement steps of the adaptive stand-in
// meshes (the vertex-balanced recipe where the call balances over vertices) and of the root cell with pseudo-random flags
// (mfgpu_mesh_refine_leaves, with and without vertex balance), every result built by mfgpu_mesh_create_from_leaves, mapped
// onto its predecessor (mfgpu_mesh_coarsening_map) and coarsened back (mfgpu_mesh_coarsen_leaves), the exact-capacity call,
// and the inputs the call refuses.
// Built and run by tests/test_amr_sanitizers.py.
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

static uint32_t rng_state = 12345u;
static uint32_t rng() {  // xorshift32
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

// n_steps refinement steps from `leaves`, each flagging about one leaf in `one_in`
static void run_steps(int dim, int degree, std::vector<uint32_t> leaves, int n_steps, uint32_t one_in, uint32_t balance) {
  for (int step = 0; step < n_steps; ++step) {
    const uint32_t n = (uint32_t)(leaves.size() / 4);
    std::vector<uint8_t> flags(n);
    uint32_t n_flagged = 0;
    for (uint32_t i = 0; i < n; ++i) n_flagged += flags[i] = (rng() % one_in) == 0;
    std::vector<uint32_t> out((size_t)n * 4 << dim);
    const int64_t n_new = mfgpu_mesh_refine_leaves(dim, leaves.data(), n, flags.data(), balance, out.data(), (uint64_t)n << dim);
    expect(n_new >= (int64_t)n + (int64_t)n_flagged * ((1 << dim) - 1), "refine_leaves splits at least the flagged leaves");
    if (n_new < 1) return;
    // exactly enough room works and gives the same leaves; one leaf less is refused
    std::vector<uint32_t> tight((size_t)n_new * 4);
    expect(mfgpu_mesh_refine_leaves(dim, leaves.data(), n, flags.data(), balance, tight.data(), (uint64_t)n_new) == n_new,
           "exact capacity");
    bool same = true;
    for (size_t i = 0; i < tight.size(); ++i) same = same && tight[i] == out[i];
    expect(same, "the same leaves with exact capacity");
    if (n_new > 1)
      expect(mfgpu_mesh_refine_leaves(dim, leaves.data(), n, flags.data(), balance, tight.data(), (uint64_t)n_new - 1) == MFGPU_EINVAL,
             "one leaf too little room is refused");
    mfgpu_mesh *coarse = nullptr, *fine = nullptr;
    expect(mfgpu_mesh_create_from_leaves(dim, degree, leaves.data(), n, 0, &coarse) == 0, "from_leaves accepts the input");
    expect(mfgpu_mesh_create_from_leaves(dim, degree, out.data(), (uint32_t)n_new, 0, &fine) == 0, "from_leaves accepts the result");
    if (coarse && fine) {
      std::vector<uint32_t> parent((size_t)n_new), child((size_t)n_new), seen(n, 0);
      expect(mfgpu_mesh_coarsening_map(coarse, fine, parent.data(), child.data()) == 0, "coarsening_map(old, new)");
      bool ok = true;
      for (int64_t f = 0; f < n_new && ok; ++f) {
        ok = parent[f] < n && child[f] <= (1u << dim);
        if (ok) seen[parent[f]] += 1;
      }
      for (uint32_t c = 0; c < n && ok; ++c) ok = seen[c] == 1 || seen[c] == (1u << dim);
      expect(ok, "every old cell is itself or all its children");
    }
    mfgpu_mesh_destroy(coarse);
    mfgpu_mesh_destroy(fine);
    if (n_new > 1) {
      std::vector<uint32_t> back((size_t)n_new * 4);
      const int64_t n_back = mfgpu_mesh_coarsen_leaves(dim, out.data(), (uint32_t)n_new, back.data());
      expect(n_back >= 1 && n_back <= (int64_t)n, "one coarsening step is no finer than the input");
    }
    std::printf("  dim %d step %d: %u leaves, %u flagged -> %ld\n", dim, step, n, n_flagged, (long)n_new);
    out.resize((size_t)n_new * 4);
    leaves.swap(out);
  }
}

int main() {
  for (int dim = 2; dim <= 3; ++dim)
    for (uint32_t balance = 0; balance <= 1; ++balance) {
      std::printf("root cell, dim %d, balance_vertices %u\n", dim, balance);
      run_steps(dim, 1, {0, 0, 0, 0}, dim == 2 ? 7 : 5, 3, balance);
      for (int n_ref = 3; n_ref <= 4; ++n_ref) {
        mfgpu_mesh *m = nullptr;
        // (vertex balance needs an input that is balanced over vertices: the _mg recipe)
        expect((balance ? mfgpu_mesh_create_adaptive_mg : mfgpu_mesh_create_adaptive)(dim, 1, n_ref, 0, &m) == 0, "create_adaptive");
        const uint32_t *lv = nullptr;
        const int64_t cnt = m ? mfgpu_mesh_cell_levels(m, &lv) : 0;
        std::printf("adaptive dim %d n_ref %d, balance_vertices %u\n", dim, n_ref, balance);
        if (cnt > 0) run_steps(dim, dim == 2 ? 2 : 1, std::vector<uint32_t>(lv, lv + cnt), 2, 5, balance);
        mfgpu_mesh_destroy(m);
      }
    }
  // what the call refuses
  std::vector<uint32_t> out(256);
  const uint8_t on[8] = {1, 1, 1, 1, 1, 1, 1, 1}, off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t root[4] = {0, 0, 0, 0};
  expect(mfgpu_mesh_refine_leaves(2, root, 1, on, 0, out.data(), 4) == 4 && out[0] == 1 && out[4] == 1 && out[5] == 1 && out[6] == 0,
         "the root cell becomes its four children in child order");
  expect(mfgpu_mesh_refine_leaves(3, root, 1, on, 1, out.data(), 8) == 8 && out[4 * 7 + 3] == 1, "and its eight children in 3D");
  expect(mfgpu_mesh_refine_leaves(2, root, 1, off, 0, out.data(), 1) == 1 && out[0] == 0, "nothing flagged: unchanged");
  expect(mfgpu_mesh_refine_leaves(2, root, 1, on, 0, out.data(), 3) == MFGPU_EINVAL, "too little room is refused");
  expect(mfgpu_mesh_refine_leaves(2, root, 1, on, 0, out.data(), 0) == MFGPU_EINVAL, "no room is refused");
  const uint32_t four[16] = {1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 0};
  expect(mfgpu_mesh_refine_leaves(2, four, 3, on, 0, out.data(), 64) == MFGPU_EINVAL, "a hole is refused");
  const uint32_t twice[20] = {1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0};
  expect(mfgpu_mesh_refine_leaves(2, twice, 5, on, 0, out.data(), 64) == MFGPU_EINVAL, "a leaf listed twice is refused");
  const uint32_t deep[4] = {40, 0, 0, 0};
  expect(mfgpu_mesh_refine_leaves(3, deep, 1, on, 0, out.data(), 64) == MFGPU_EINVAL, "a level beyond the key's range is refused");
  const uint32_t outside[16] = {1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 5, 1, 0};
  expect(mfgpu_mesh_refine_leaves(2, outside, 4, on, 0, out.data(), 64) == MFGPU_EINVAL, "a leaf outside the root cell is refused");
  expect(mfgpu_mesh_refine_leaves(2, nullptr, 4, on, 0, out.data(), 64) == MFGPU_EINVAL, "null leaves are refused");
  expect(mfgpu_mesh_refine_leaves(2, four, 4, nullptr, 0, out.data(), 64) == MFGPU_EINVAL, "null flags are refused");
  expect(mfgpu_mesh_refine_leaves(2, four, 4, on, 0, nullptr, 64) == MFGPU_EINVAL, "null out is refused");
  expect(mfgpu_mesh_refine_leaves(4, four, 4, on, 0, out.data(), 64) == MFGPU_EINVAL, "dim 4 is refused");
  // not one-irregular: level 1 next to level 3 over a face
  const uint32_t jump[40] = {1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 0, 2, 0, 0, 0, 2, 1, 0, 0, 2, 0, 1, 0,
                             3, 2, 2, 0, 3, 3, 2, 0, 3, 2, 3, 0, 3, 3, 3, 0};
  expect(mfgpu_mesh_refine_leaves(2, jump, 10, off, 0, out.data(), 64) == MFGPU_EINVAL, "a two-level jump is refused");
  // one-irregular over faces, level 1 meets level 3 at the centre vertex: fine without vertex balance, refused with it
  const uint32_t vertex[64] = {1, 1, 1, 0, 2, 2, 0, 0, 2, 3, 0, 0, 2, 2, 1, 0, 2, 3, 1, 0, 2, 0, 2, 0, 2, 1, 2, 0, 2, 0, 3, 0, 2, 1, 3, 0,
                               2, 0, 0, 0, 2, 1, 0, 0, 2, 0, 1, 0, 3, 2, 2, 0, 3, 3, 2, 0, 3, 2, 3, 0, 3, 3, 3, 0};
  const uint8_t none[16] = {0};
  expect(mfgpu_mesh_refine_leaves(2, vertex, 16, none, 0, out.data(), 64) == 16, "a vertex jump passes without vertex balance");
  expect(mfgpu_mesh_refine_leaves(2, vertex, 16, none, 1, out.data(), 64) == MFGPU_EINVAL, "and is refused with it");
  // a corner chain down to level 18: its finest leaf cannot be flagged, the others can
  std::vector<uint32_t> chain = {0, 0, 0, 0};
  for (int l = 0; l < 18; ++l) {
    const uint32_t n = (uint32_t)(chain.size() / 4);
    std::vector<uint8_t> f(n, 0);
    for (uint32_t i = 0; i < n; ++i) f[i] = chain[4 * i] == (uint32_t)l && chain[4 * i + 1] == 0 && chain[4 * i + 2] == 0;
    std::vector<uint32_t> next((size_t)n * 16);
    const int64_t k = mfgpu_mesh_refine_leaves(2, chain.data(), n, f.data(), 0, next.data(), (uint64_t)n * 4);
    expect(k == (int64_t)n + 3, "the corner chain grows by three leaves per level");
    if (k < 1) break;
    next.resize((size_t)k * 4);
    chain.swap(next);
  }
  {
    const uint32_t n = (uint32_t)(chain.size() / 4);
    std::vector<uint8_t> f(n, 0);
    for (uint32_t i = 0; i < n; ++i) f[i] = chain[4 * i] == 18;
    std::vector<uint32_t> next((size_t)n * 16);
    expect(mfgpu_mesh_refine_leaves(2, chain.data(), n, f.data(), 0, next.data(), (uint64_t)n * 4) == MFGPU_EINVAL,
           "a child deeper than level 18 is refused");
    for (uint32_t i = 0; i < n; ++i) f[i] = chain[4 * i] == 17;
    // the three level-17 leaves may split; with vertex balance they drag the three leaves of every coarser level along
    expect(mfgpu_mesh_refine_leaves(2, chain.data(), n, f.data(), 1, next.data(), (uint64_t)n * 4) == (int64_t)n + 9 * 17,
           "the level-17 leaves split to level 18 and the closure runs up the chain");
  }
  std::printf("done bad=%d\n", bad);
  return bad != 0;
}
