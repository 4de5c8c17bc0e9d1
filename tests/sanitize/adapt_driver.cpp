// Adaptation in both directions on the host under AddressSanitizer + UBSan (CPU build only): steps of
// mfgpu_mesh_adapt_leaves with pseudo-random refine and coarsen flags in 2D and 3D, with and without vertex balance; every
// `new` and `mid` built by mfgpu_mesh_create_from_leaves, both pairs (mid, old) and (mid, new) mapped
// (mfgpu_mesh_coarsening_map) and handed to build_transfer_image with the interpolation image, every image checked in plain
// loops against the index format (the fine cells of each coarse cell, the owner marking of the coarse list, J1); the
// exact-capacity call and the inputs the call and the image builder refuse.
// Built and run by tests/test_adapt_sanitizers.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mfgpu.h"
#include "mfgpu_transfer_build.h"

using mfgpu::TransferImage;
using mfgpu::TransferInput;

static int bad = 0;
static void expect(bool ok, const std::string &what) {
  if (!ok) {
    std::printf("FAILED: %s (%s)\n", what.c_str(), mfgpu_last_error());
    ++bad;
  }
}

static uint32_t rng_state = 2463534242u;
static uint32_t rng() {  // xorshift32
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

static const uint32_t BIT31 = 0x80000000u;
static int ipow(int a, int e) { return e == 0 ? 1 : a * ipow(a, e - 1); }

struct M {  // a mesh and its description
  mfgpu_mesh *m = nullptr;
  mfgpu_desc d;
  M() { std::memset(&d, 0, sizeof d); }
  M(const M &) = delete;
  ~M() { mfgpu_mesh_destroy(m); }
  void leaves(int dim, int p, const std::vector<uint32_t> &lv) {
    const int rc = mfgpu_mesh_create_from_leaves(dim, p, lv.data(), (uint32_t)(lv.size() / 4), MFGPU_F64, &m);
    expect(rc == 0 && m, "create_from_leaves");
    if (m) expect(mfgpu_mesh_desc(m, &d) == 0, "mesh_desc");
  }
};

// the interpolation image of the pair (c, f) and its checks
static void image_of_pair(const M &c, const M &f, const std::string &tag) {
  const int dim = c.d.dim, p = c.d.degree, n = p + 1;
  const size_t N = (size_t)ipow(n, dim), NK = (size_t)1 << dim;
  std::vector<uint32_t> parent(f.d.n_cells), child(f.d.n_cells);
  expect(mfgpu_mesh_coarsening_map(c.m, f.m, parent.data(), child.data()) == 0, tag + ": coarsening_map");
  TransferInput in;
  in.who = "mfgpu_transfer_create_h_hn_interp";
  in.kind = mfgpu::TRANSFER_KIND_H_HN;
  in.dim = dim;
  in.degree = p;
  in.number_type = MFGPU_F64;
  in.n_coarse_cells = c.d.n_cells;
  in.n_fine_cells = f.d.n_cells;
  in.n_coarse_dofs = c.d.n_dofs;
  in.n_fine_dofs = f.d.n_dofs;
  in.coarse_cell_dofs = c.d.loc2glob;
  in.fine_cell_dofs = f.d.loc2glob;
  in.coarse_dirichlet = c.d.constrained_dofs;
  in.n_coarse_dirichlet = c.d.n_constrained;
  in.parent = parent.data();
  in.child = child.data();
  in.coarse_mask = c.d.constraint_mask;
  in.fine_mask = f.d.constraint_mask;
  in.constraint_weights = c.d.constraint_weights;
  {
    TransferImage plain;
    expect(mfgpu::build_transfer_image(in, plain) == 0, tag + ": the image without interpolation");
    expect(plain.interp_coarse.empty() && plain.interp_kids.empty() && plain.interp_fine_mask.empty() && plain.J1.empty(),
           tag + ": an image without interpolation holds none of its arrays");
  }
  in.interpolation = true;
  TransferImage img;
  const int rc = mfgpu::build_transfer_image(in, img);
  expect(rc == 0, tag + ": build_transfer_image with interpolation");
  if (rc) return;
  expect(img.interp_kids.size() == NK * c.d.n_cells && img.interp_coarse.size() == N * c.d.n_cells &&
             img.interp_fine_mask.size() == f.d.n_cells && img.J1.size() == (size_t)n * n,
         tag + ": sizes");
  // the fine cells of each coarse cell: every fine cell appears exactly once, where its parent and child say
  std::vector<uint32_t> met(f.d.n_cells, 0);
  bool kids = true;
  for (uint32_t cc = 0; cc < c.d.n_cells && kids; ++cc) {
    const uint32_t *k = &img.interp_kids[cc * NK];
    if (k[0] & BIT31) {
      const uint32_t ff = k[0] & ~BIT31;
      kids = ff < f.d.n_cells && parent[ff] == cc && child[ff] == 0;
      if (kids) met[ff] += 1;
    } else {
      for (size_t j = 0; j < NK && kids; ++j) {
        kids = k[j] < f.d.n_cells && parent[k[j]] == cc && child[k[j]] == 1 + j;
        if (kids) met[k[j]] += 1;
      }
    }
  }
  for (uint32_t ff = 0; ff < f.d.n_cells; ++ff) kids = kids && met[ff] == 1;
  expect(kids, tag + ": every fine cell stands once in its coarse cell's list");
  // the coarse list: the caller's dofs, at most one entry without bit 31 per dof, none for a Dirichlet dof
  std::vector<uint8_t> dir(c.d.n_dofs, 0);
  for (uint32_t i = 0; i < c.d.n_constrained; ++i) dir[c.d.constrained_dofs[i]] = 1;
  std::vector<uint32_t> owners(c.d.n_dofs, 0), listed(c.d.n_dofs, 0);
  bool same = true;
  size_t stored = 0;
  for (size_t i = 0; i < img.interp_coarse.size(); ++i) {
    const uint32_t e = img.interp_coarse[i], g = e & ~BIT31;
    same = same && g == c.d.loc2glob[i];
    if (g >= c.d.n_dofs) continue;
    listed[g] = 1;
    if (!(e & BIT31)) owners[g] += 1, ++stored;
  }
  bool one = true;
  for (uint32_t g = 0; g < c.d.n_dofs; ++g) one = one && owners[g] == (listed[g] && !dir[g] ? 1u : 0u);
  expect(same && one && stored == img.interp_covered, tag + ": one owner per listed coarse dof that is not a Dirichlet dof");
  bool masks = true;
  for (uint32_t ff = 0; ff < f.d.n_cells; ++ff) masks = masks && img.interp_fine_mask[ff] == (f.d.constraint_mask ? f.d.constraint_mask[ff] : 0u);
  expect(masks, tag + ": the fine masks");
  // J1: rows sum to 1, the lower half's rows are those of P1's even rows (a coarse node 2 xi is a node of the child)
  bool rows = true;
  for (int i = 0; i < n; ++i) {
    double s = 0;
    for (int j = 0; j < n; ++j) s += img.J1[(size_t)i * n + j];
    rows = rows && s > 1.0 - 1e-12 && s < 1.0 + 1e-12;
  }
  expect(rows && img.J1[0] == 1.0 && img.J1[(size_t)n * n - 1] == 1.0, tag + ": J1 is a partition of unity with unit end rows");
  // an explicit J1 is taken as it stands
  std::vector<double> j1((size_t)n * n);
  for (size_t i = 0; i < j1.size(); ++i) j1[i] = 0.25 * (double)i;
  in.interpolation_1d = j1.data();
  TransferImage img2;
  expect(mfgpu::build_transfer_image(in, img2) == 0 && img2.J1 == j1, tag + ": an explicit J1");
  in.interpolation_1d = nullptr;
  // refusals: a child twice (its sibling missing), a cell both unchanged and refined, another kind
  std::vector<uint32_t> ch = child, pa = parent;
  for (uint32_t ff = 0; ff < f.d.n_cells; ++ff)
    if (child[ff] == 1) {
      ch[ff] = 2;
      TransferInput b = in;
      b.child = ch.data();
      TransferImage r;
      expect(mfgpu::build_transfer_image(b, r) == MFGPU_EINVAL, tag + ": a child listed twice is refused");
      ch[ff] = 0;
      expect(mfgpu::build_transfer_image(b, r) == MFGPU_EINVAL, tag + ": a cell both unchanged and refined is refused");
      break;
    }
  TransferInput b = in;
  b.kind = mfgpu::TRANSFER_KIND_P;
  b.degree_coarse = p;
  b.degree = p < 6 ? p + 1 : p;
  TransferImage r;
  expect(mfgpu::build_transfer_image(b, r) == MFGPU_EINVAL, tag + ": another kind has no interpolation image");
}

static void run_steps(int dim, int degree, std::vector<uint32_t> leaves, int n_steps, uint32_t refine_in, uint32_t coarsen_in,
                      uint32_t balance) {
  for (int step = 0; step < n_steps; ++step) {
    const uint32_t n = (uint32_t)(leaves.size() / 4);
    std::vector<uint8_t> rf(n), cf(n);
    for (uint32_t i = 0; i < n; ++i) {
      rf[i] = (rng() % refine_in) == 0;
      cf[i] = (rng() % coarsen_in) != 0;  // most leaves are willing; some carry both flags
    }
    std::vector<uint32_t> fresh((size_t)n * 4 << dim), mid((size_t)n * 4);
    uint32_t n_mid = 0;
    const int64_t n_new = mfgpu_mesh_adapt_leaves(dim, leaves.data(), n, rf.data(), cf.data(), balance, fresh.data(),
                                                  (uint64_t)n << dim, mid.data(), &n_mid);
    expect(n_new >= 1 && n_mid >= 1 && n_mid <= n && (int64_t)n_mid <= n_new, "adapt_leaves");
    if (n_new < 1) return;
    std::vector<uint32_t> tight((size_t)n_new * 4), mid2((size_t)n * 4);
    uint32_t n_mid2 = 0;
    expect(mfgpu_mesh_adapt_leaves(dim, leaves.data(), n, rf.data(), cf.data(), balance, tight.data(), (uint64_t)n_new, mid2.data(),
                                   &n_mid2) == n_new && n_mid2 == n_mid,
           "exact capacity");
    bool same = true;
    for (size_t i = 0; i < tight.size(); ++i) same = same && tight[i] == fresh[i];
    for (size_t i = 0; i < (size_t)n_mid * 4; ++i) same = same && mid2[i] == mid[i];
    expect(same, "the same leaves with exact capacity");
    if (n_new > 1)
      expect(mfgpu_mesh_adapt_leaves(dim, leaves.data(), n, rf.data(), cf.data(), balance, tight.data(), (uint64_t)n_new - 1,
                                     mid2.data(), &n_mid2) == MFGPU_EINVAL,
             "one leaf too little room is refused");
    fresh.resize((size_t)n_new * 4);
    mid.resize((size_t)n_mid * 4);
    M m_old, m_mid, m_new;
    m_old.leaves(dim, degree, leaves), m_mid.leaves(dim, degree, mid), m_new.leaves(dim, degree, fresh);
    const std::string tag = "dim " + std::to_string(dim) + " step " + std::to_string(step) + " balance " + std::to_string(balance);
    if (m_old.m && m_mid.m && m_new.m) {
      image_of_pair(m_mid, m_old, tag + " (mid, old)");
      image_of_pair(m_mid, m_new, tag + " (mid, new)");
    }
    std::printf("  %s: %u leaves -> mid %u -> new %ld\n", tag.c_str(), n, n_mid, (long)n_new);
    leaves.swap(fresh);
  }
}

int main() {
  for (int dim = 2; dim <= 3; ++dim)
    for (uint32_t balance = 0; balance <= 1; ++balance) {
      // grow from the root cell, then adapt with mixed flags
      run_steps(dim, dim == 2 ? 3 : 2, {0, 0, 0, 0}, dim == 2 ? 7 : 5, 3, 4, balance);
      mfgpu_mesh *m = nullptr;
      expect((balance ? mfgpu_mesh_create_adaptive_mg : mfgpu_mesh_create_adaptive)(dim, 1, 4, 0, &m) == 0, "create_adaptive");
      const uint32_t *lv = nullptr;
      const int64_t cnt = m ? mfgpu_mesh_cell_levels(m, &lv) : 0;
      if (cnt > 0) run_steps(dim, 1, std::vector<uint32_t>(lv, lv + cnt), 3, 20, 8, balance);
      mfgpu_mesh_destroy(m);
    }
  // what the call refuses
  std::vector<uint32_t> out(256), mid(256);
  uint32_t n_mid = 0;
  const uint8_t on[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, off[16] = {0};
  const uint32_t root[4] = {0, 0, 0, 0};
  expect(mfgpu_mesh_adapt_leaves(2, root, 1, off, on, 0, out.data(), 1, mid.data(), &n_mid) == 1 && n_mid == 1 && out[0] == 0,
         "the root cell cannot be coarsened: unchanged");
  expect(mfgpu_mesh_adapt_leaves(2, root, 1, on, on, 0, out.data(), 4, mid.data(), &n_mid) == 4 && n_mid == 1 && out[5] == 1,
         "refinement wins on the root cell");
  const uint32_t four[16] = {1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 0};
  expect(mfgpu_mesh_adapt_leaves(2, four, 4, off, on, 0, out.data(), 4, mid.data(), &n_mid) == 1 && n_mid == 1 && out[0] == 0 &&
             mid[0] == 0,
         "four siblings become the root cell");
  expect(mfgpu_mesh_adapt_leaves(2, four, 4, off, on, 0, out.data(), 0, mid.data(), &n_mid) == MFGPU_EINVAL, "no room is refused");
  expect(mfgpu_mesh_adapt_leaves(2, four, 3, off, on, 0, out.data(), 64, mid.data(), &n_mid) == MFGPU_EINVAL, "a hole is refused");
  expect(mfgpu_mesh_adapt_leaves(2, nullptr, 4, off, on, 0, out.data(), 64, mid.data(), &n_mid) == MFGPU_EINVAL, "null leaves");
  expect(mfgpu_mesh_adapt_leaves(2, four, 4, nullptr, on, 0, out.data(), 64, mid.data(), &n_mid) == MFGPU_EINVAL, "null refine flags");
  expect(mfgpu_mesh_adapt_leaves(2, four, 4, off, nullptr, 0, out.data(), 64, mid.data(), &n_mid) == MFGPU_EINVAL, "null coarsen flags");
  expect(mfgpu_mesh_adapt_leaves(2, four, 4, off, on, 0, nullptr, 64, mid.data(), &n_mid) == MFGPU_EINVAL, "null out_new");
  expect(mfgpu_mesh_adapt_leaves(2, four, 4, off, on, 0, out.data(), 64, nullptr, &n_mid) == MFGPU_EINVAL, "null out_mid");
  expect(mfgpu_mesh_adapt_leaves(2, four, 4, off, on, 0, out.data(), 64, mid.data(), nullptr) == MFGPU_EINVAL, "null n_mid");
  expect(mfgpu_mesh_adapt_leaves(4, four, 4, off, on, 0, out.data(), 64, mid.data(), &n_mid) == MFGPU_EINVAL, "dim 4");
  const uint32_t jump[40] = {1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 0, 2, 0, 0, 0, 2, 1, 0, 0, 2, 0, 1, 0,
                             3, 2, 2, 0, 3, 3, 2, 0, 3, 2, 3, 0, 3, 3, 3, 0};
  expect(mfgpu_mesh_adapt_leaves(2, jump, 10, off, on, 0, out.data(), 64, mid.data(), &n_mid) == MFGPU_EINVAL, "a two-level jump");
  const uint32_t vertex[64] = {1, 1, 1, 0, 2, 2, 0, 0, 2, 3, 0, 0, 2, 2, 1, 0, 2, 3, 1, 0, 2, 0, 2, 0, 2, 1, 2, 0, 2, 0, 3, 0, 2, 1, 3, 0,
                               2, 0, 0, 0, 2, 1, 0, 0, 2, 0, 1, 0, 3, 2, 2, 0, 3, 3, 2, 0, 3, 2, 3, 0, 3, 3, 3, 0};
  expect(mfgpu_mesh_adapt_leaves(2, vertex, 16, off, off, 0, out.data(), 64, mid.data(), &n_mid) == 16 && n_mid == 16,
         "a vertex jump passes without vertex balance");
  expect(mfgpu_mesh_adapt_leaves(2, vertex, 16, off, off, 1, out.data(), 64, mid.data(), &n_mid) == MFGPU_EINVAL, "and is refused with it");
  std::printf("done bad=%d\n", bad);
  return bad != 0;
}
