// The host-side builder of the multigrid transfers (csrc/mfgpu_transfer_build.cpp: plain C++, no HIP) under
// AddressSanitizer + UBSan (CPU build only): build_transfer_image for all three kinds on meshes made through the mesh
// C-ABI, every image checked in plain loops against the index format (owner rule, Dirichlet flags, h_hn words), every
// input the builder refuses at the first and at the last cell, and constrained_position against a literal restatement of
// the nine mask bits.
// Built and run by tests/test_transfer_sanitizers.py.
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

static const uint32_t BIT31 = 0x80000000u;

// TYPE x, y, z: bits 0..2 (set: the coarse neighbour's face or edge is at coordinate 0 of that direction, else at p);
// FACE x, y, z: bits 3..5; EDGE xy, yz, zx: bits 6..8
static bool literal_constrained(int dim, int n, uint32_t m, int t) {
  const int p = n - 1, x = t % n, y = (t / n) % n, z = dim == 3 ? t / (n * n) : 0;
  const bool ax = x == ((m & 1u) ? 0 : p), ay = y == ((m & 2u) ? 0 : p), az = z == ((m & 4u) ? 0 : p);
  if ((m & 8u) && ax) return true;
  if ((m & 16u) && ay) return true;
  if (dim == 3) {
    if ((m & 32u) && az) return true;
    if ((m & 64u) && ax && ay) return true;
    if ((m & 128u) && ay && az) return true;
    if ((m & 256u) && az && ax) return true;
  }
  return false;
}

static int ipow(int a, int e) { return e == 0 ? 1 : a * ipow(a, e - 1); }

struct M {  // a mesh and its description
  mfgpu_mesh *m = nullptr;
  mfgpu_desc d;
  M() { std::memset(&d, 0, sizeof d); }
  M(const M &) = delete;
  ~M() { mfgpu_mesh_destroy(m); }
  void describe(int rc, const char *what) {
    expect(rc == 0 && m, what);
    if (m) expect(mfgpu_mesh_desc(m, &d) == 0, "mesh_desc");
  }
  void uniform(int dim, int p, uint32_t n) {
    const uint32_t nper[3] = {n, n, n};
    describe(mfgpu_mesh_create_uniform(dim, p, nper, -1.0, 1.0, 0, 0, MFGPU_F64, &m), "create_uniform");
  }
  void adaptive(int dim, int p, int n_ref) { describe(mfgpu_mesh_create_adaptive(dim, p, n_ref, MFGPU_F64, &m), "create_adaptive"); }
  void leaves(int dim, int p, const std::vector<uint32_t> &lv) {
    describe(mfgpu_mesh_create_from_leaves(dim, p, lv.data(), (uint32_t)(lv.size() / 4), MFGPU_F64, &m), "create_from_leaves");
  }
};

// the checks of one image; `in` is what it was built from
static void check_image(const TransferInput &in, const TransferImage &img, const std::string &tag) {
  const int nf = in.kind == mfgpu::TRANSFER_KIND_H ? 2 * in.degree + 1 : in.degree + 1;
  const size_t NF = (size_t)ipow(nf, in.dim), NC = (size_t)ipow((in.kind == mfgpu::TRANSFER_KIND_P ? in.degree_coarse : in.degree) + 1, in.dim);
  expect(img.fine.size() == NF * in.n_fine_cells && img.coarse.size() == NC * in.n_coarse_cells, tag + ": list sizes");
  if (img.fine.size() != NF * in.n_fine_cells || img.coarse.size() != NC * in.n_coarse_cells) return;
  std::vector<uint32_t> owners(in.n_fine_dofs, 0), listed(in.n_fine_dofs, 0);
  bool same = true, free_owner = true;
  for (uint32_t c = 0; c < in.n_fine_cells; ++c)
    for (size_t i = 0; i < NF; ++i) {
      const uint32_t e = img.fine[c * NF + i], g = e & ~BIT31;
      same = same && g == in.fine_cell_dofs[c * NF + i];
      if (g >= in.n_fine_dofs) continue;
      listed[g] = 1;
      if (!(e & BIT31)) {
        owners[g] += 1;
        free_owner = free_owner && !(in.fine_mask && literal_constrained(in.dim, nf, in.fine_mask[c], (int)i));
      }
    }
  size_t n_listed = 0;
  bool one_owner = true;
  for (uint32_t g = 0; g < in.n_fine_dofs; ++g) {
    n_listed += listed[g];
    one_owner = one_owner && owners[g] == listed[g];
  }
  expect(same, tag + ": the fine list holds the caller's dofs");
  expect(one_owner, tag + ": every listed fine dof has exactly one entry without bit 31");
  expect(free_owner, tag + ": the owner's position is not constrained");
  expect(img.covered == n_listed, tag + ": covered = the number of distinct listed dofs");
  std::vector<uint8_t> dir(in.n_coarse_dofs, 0);
  for (uint32_t i = 0; i < in.n_coarse_dirichlet; ++i) dir[in.coarse_dirichlet[i]] = 1;
  bool flags = true;
  for (size_t i = 0; i < img.coarse.size(); ++i) {
    const uint32_t g = img.coarse[i] & ~BIT31;
    flags = flags && g == in.coarse_cell_dofs[i] && ((img.coarse[i] >> 31) != 0) == (dir[g] != 0);
  }
  expect(flags, tag + ": a coarse entry has bit 31 exactly when its dof is a Dirichlet dof");
  if (in.kind == mfgpu::TRANSFER_KIND_H_HN) {
    bool words = img.words.size() == in.n_fine_cells && img.parent.size() == in.n_fine_cells;
    for (uint32_t f = 0; words && f < in.n_fine_cells; ++f)
      words = img.parent[f] == in.parent[f] &&
              img.words[f] == ((in.coarse_mask ? in.coarse_mask[in.parent[f]] : 0u) | in.child[f] << 16);
    expect(words, tag + ": word = coarse_mask[parent] | child << 16");
  }
}

// MFGPU_EINVAL with a message that begins with `who` and names the reason
static void refused(const TransferInput &in, const std::string &what, const char *reason = "bad argument") {
  TransferImage img;
  const int rc = mfgpu::build_transfer_image(in, img);
  const std::string msg = mfgpu_last_error(), who = std::string(in.who) + ": ";
  expect(rc == MFGPU_EINVAL && msg.compare(0, who.size(), who) == 0 && msg.find(reason) != std::string::npos,
         std::string(in.who) + " refuses " + what);
}

// some valid mask that constrains position t of an n^dim cell (0: none does, the cell's interior)
static uint32_t mask_constraining(int dim, int n, int t) {
  for (uint32_t m = 1; m < 0x200u; ++m)
    if (!(m & ~(dim == 3 ? 0x1ffu : 0x1bu)) && literal_constrained(dim, n, m, t)) return m;
  return 0;
}

// every input of the list the builder refuses, derived from the good input `in` (non-empty, with Dirichlet dofs)
static void refusals(const TransferInput &in) {
  const bool p_kind = in.kind == mfgpu::TRANSFER_KIND_P, h_hn = in.kind == mfgpu::TRANSFER_KIND_H_HN;
  const int nf = in.kind == mfgpu::TRANSFER_KIND_H ? 2 * in.degree + 1 : in.degree + 1;
  const size_t NF = (size_t)ipow(nf, in.dim), NC = (size_t)ipow((p_kind ? in.degree_coarse : in.degree) + 1, in.dim);
  const std::vector<uint32_t> cd(in.coarse_cell_dofs, in.coarse_cell_dofs + NC * in.n_coarse_cells),
      fd(in.fine_cell_dofs, in.fine_cell_dofs + NF * in.n_fine_cells),
      di(in.coarse_dirichlet, in.coarse_dirichlet + in.n_coarse_dirichlet);
  expect(!di.empty() && !cd.empty() && !fd.empty(), "the refusals start from a non-empty input with Dirichlet dofs");
  if (di.empty() || cd.empty() || fd.empty()) return;
  TransferInput b = in;
  b.dim = 4, refused(b, "dim 4");
  b = in, b.dim = 1, refused(b, "dim 1");
  b = in, b.degree = 7, refused(b, "degree 7");
  b = in, b.degree = p_kind ? in.degree_coarse : 0, refused(b, p_kind ? "degree_fine = degree_coarse" : "degree 0");
  if (p_kind) b = in, b.degree_coarse = 0, refused(b, "degree_coarse 0");
  b = in, b.number_type = 99, refused(b, "an unknown number type");
  b = in, b.coarse_cell_dofs = nullptr, refused(b, "null coarse_cell_dofs");
  b = in, b.fine_cell_dofs = nullptr, refused(b, "null fine_cell_dofs");
  b = in, b.coarse_dirichlet = nullptr, refused(b, "null coarse_dirichlet");
  b = in, b.n_coarse_dofs = 1u << 31, refused(b, "2^31 coarse dofs");
  b = in, b.n_fine_dofs = 1u << 31, refused(b, "2^31 fine dofs");
  for (int last = 0; last < 2; ++last) {  // the first and the last cell (or list entry)
    const std::string where = last ? " in the last cell" : " in the first cell";
    std::vector<uint32_t> v = di;
    v[last ? v.size() - 1 : 0] = in.n_coarse_dofs;
    b = in, b.coarse_dirichlet = v.data(), refused(b, "a Dirichlet dof out of range" + where, "Dirichlet dof out of range");
    v = cd, v[last ? v.size() - 1 : 0] = in.n_coarse_dofs;
    b = in, b.coarse_cell_dofs = v.data(), refused(b, "a coarse dof out of range" + where, "coarse dof out of range");
    v = fd, v[last ? v.size() - 1 : 0] = in.n_fine_dofs;
    b = in, b.fine_cell_dofs = v.data(), refused(b, "a fine dof out of range" + where, "fine dof out of range");
    if (in.kind == mfgpu::TRANSFER_KIND_H) continue;
    const uint32_t fc = last ? in.n_fine_cells - 1 : 0, cc = last ? in.n_coarse_cells - 1 : 0;
    std::vector<uint32_t> fm(in.n_fine_cells, 0u), cm(in.n_coarse_cells, 0u);
    if (in.fine_mask) fm.assign(in.fine_mask, in.fine_mask + in.n_fine_cells);
    if (in.coarse_mask) cm.assign(in.coarse_mask, in.coarse_mask + in.n_coarse_cells);
    v = fm, v[fc] |= in.dim == 3 ? 0x200u : 0x4u;  // (2D: TYPE z is not defined)
    b = in, b.fine_mask = v.data();
    if (p_kind) b.coarse_mask = v.data();
    refused(b, "a fine mask with bits outside the defined ones" + where, "a constraint mask has bits outside");
    // a dof that only cell fc lists, at a position that a mask of fc's constrains: nobody owns it
    std::vector<uint32_t> count(in.n_fine_dofs, 0);
    for (uint32_t g : fd) count[g] += 1;
    uint32_t m = 0;
    for (size_t i = 0; i < NF && !m; ++i)
      if (count[fd[fc * NF + i]] == 1) m = mask_constraining(in.dim, nf, (int)i);
    expect(m != 0, std::string(in.who) + ": the test finds a dof that one cell alone lists on its boundary" + where);
    v = fm, v[fc] = m;
    b = in, b.fine_mask = v.data();
    if (p_kind) b.coarse_mask = v.data();
    refused(b, "a fine dof listed only at constrained positions" + where, "only at constrained positions");
    if (!h_hn) continue;
    v = cm, v[cc] |= in.dim == 3 ? 0x200u : 0x20u;  // (2D: FACE z is not defined)
    b = in, b.coarse_mask = v.data(), refused(b, "a coarse mask with bits outside the defined ones" + where, "a coarse constraint mask has bits outside");
    v.assign(in.parent, in.parent + in.n_fine_cells), v[fc] = in.n_coarse_cells;
    b = in, b.parent = v.data(), refused(b, "a parent out of range" + where, "parent out of range");
    v.assign(in.child, in.child + in.n_fine_cells), v[fc] = (1u << in.dim) + 1;
    b = in, b.child = v.data(), refused(b, "child > 2^dim" + where, "child > 2^dim");
  }
  if (h_hn) {
    b = in, b.parent = nullptr, refused(b, "null parent");
    b = in, b.child = nullptr, refused(b, "null child");
  }
}

static TransferInput input_of(const char *who, int kind, const M &c, const M &f) {
  TransferInput in;
  in.who = who;
  in.kind = kind;
  in.dim = f.d.dim;
  in.degree = f.d.degree;
  in.degree_coarse = kind == mfgpu::TRANSFER_KIND_P ? c.d.degree : 0;
  in.number_type = f.d.number_type;
  in.n_coarse_cells = c.d.n_cells;
  in.n_fine_cells = kind == mfgpu::TRANSFER_KIND_H_HN ? f.d.n_cells : c.d.n_cells;
  in.n_coarse_dofs = c.d.n_dofs;
  in.n_fine_dofs = f.d.n_dofs;
  in.coarse_cell_dofs = c.d.loc2glob;
  in.fine_cell_dofs = f.d.loc2glob;
  in.coarse_dirichlet = c.d.constrained_dofs;
  in.n_coarse_dirichlet = c.d.n_constrained;
  return in;
}

static void build_and_check(const TransferInput &in, const std::string &tag, bool with_refusals) {
  TransferImage img;
  const int rc = mfgpu::build_transfer_image(in, img);
  expect(rc == 0, tag + ": build_transfer_image");
  if (rc) return;
  check_image(in, img, tag);
  const int nc = (in.kind == mfgpu::TRANSFER_KIND_P ? in.degree_coarse : in.degree) + 1;
  const int rows = in.kind == mfgpu::TRANSFER_KIND_P ? in.degree + 1 : 2 * in.degree + 1;
  expect(img.P1.size() == (size_t)rows * nc && img.W.size() == (img.hanging_nodes ? (size_t)nc * nc : 0), tag + ": P1 and W sizes");
  if (with_refusals) refusals(in);
  std::printf("  %s: %u coarse, %u fine cells, covered %zu of %u\n", tag.c_str(), in.n_coarse_cells, in.n_fine_cells, img.covered,
              in.n_fine_dofs);
}

static std::string tag_of(const char *kind, int dim, int pc, int p) {
  return std::string(kind) + " dim " + std::to_string(dim) + " degree " + (pc ? std::to_string(pc) + " -> " : "") + std::to_string(p);
}

int main() {
  // level h: uniform 2 -> 4 cells per direction, patches from the mesh code
  const int level_cases[5][2] = {{2, 1}, {2, 3}, {2, 6}, {3, 2}, {3, 4}};
  for (const auto &dp : level_cases) {
    const int dim = dp[0], p = dp[1];
    M c, f;
    c.uniform(dim, p, 2), f.uniform(dim, p, 4);
    if (!c.m || !f.m) continue;
    std::vector<uint32_t> cd((size_t)c.d.n_cells * ipow(p + 1, dim)), fd((size_t)c.d.n_cells * ipow(2 * p + 1, dim));
    expect(mfgpu_mesh_transfer_patches(c.m, f.m, cd.data(), fd.data()) == (int64_t)c.d.n_cells, "mesh_transfer_patches");
    TransferInput in = input_of("mfgpu_transfer_create", mfgpu::TRANSFER_KIND_H, c, f);
    in.coarse_cell_dofs = cd.data();
    in.fine_cell_dofs = fd.data();
    build_and_check(in, tag_of("level h", dim, 0, p), true);
  }
  // p and p_hn: uniform 3D (no masks), adaptive 2D and 3D (the cells' masks).  The 3D recipe refines nothing below
  // n_ref = 4 (n_ref = 2 is one cell without a mask), so n_ref = 4 stands beside it for hanging nodes in 3D
  const int pairs[3][2] = {{1, 2}, {2, 4}, {3, 6}};
  const int adaptive_cases[3][2] = {{2, 2}, {3, 2}, {3, 4}};  // dim, n_ref
  for (const auto &pp : pairs) {
    {
      M c, f;
      c.uniform(3, pp[0], 2), f.uniform(3, pp[1], 2);
      if (c.m && f.m)
        build_and_check(input_of("mfgpu_transfer_create_p_hn", mfgpu::TRANSFER_KIND_P, c, f), tag_of("p uniform", 3, pp[0], pp[1]), true);
    }
    for (const auto &dr : adaptive_cases) {
      M c, f;
      c.adaptive(dr[0], pp[0], dr[1]), f.adaptive(dr[0], pp[1], dr[1]);
      if (!c.m || !f.m) continue;
      TransferInput in = input_of("mfgpu_transfer_create_p_hn", mfgpu::TRANSFER_KIND_P, c, f);
      in.coarse_mask = in.fine_mask = c.d.constraint_mask;
      in.constraint_weights = c.d.constraint_weights;
      expect((c.d.n_cells > 1) == (in.coarse_mask != nullptr), "an adaptive mesh of more than one cell has masks");
      build_and_check(in, tag_of("p_hn adaptive", dr[0], pp[0], pp[1]) + " n_ref " + std::to_string(dr[1]), true);
    }
  }
  // h_hn: an adaptive mesh and its coarsening sequence, every member against the next finer one
  for (const auto &dr : adaptive_cases)
    for (int p : {1, 2, 4}) {
      const int dim = dr[0];
      M top;
      top.adaptive(dim, p, dr[1]);
      const uint32_t *lv = nullptr;
      const int64_t cnt = top.m ? mfgpu_mesh_cell_levels(top.m, &lv) : 0;
      expect(cnt > 0, "the adaptive mesh has leaves");
      if (cnt <= 0) continue;
      std::vector<uint32_t> fine_leaves(lv, lv + cnt);
      for (int step = 0; fine_leaves.size() > 4; ++step) {
        std::vector<uint32_t> coarse_leaves(fine_leaves.size());
        const int64_t n = mfgpu_mesh_coarsen_leaves(dim, fine_leaves.data(), (uint32_t)(fine_leaves.size() / 4), coarse_leaves.data());
        expect(n >= 1, "coarsen_leaves");
        if (n < 1) break;
        coarse_leaves.resize((size_t)n * 4);
        M c, f;
        c.leaves(dim, p, coarse_leaves), f.leaves(dim, p, fine_leaves);
        if (!c.m || !f.m) break;
        std::vector<uint32_t> parent(f.d.n_cells), child(f.d.n_cells);
        expect(mfgpu_mesh_coarsening_map(c.m, f.m, parent.data(), child.data()) == 0, "coarsening_map");
        TransferInput in = input_of("mfgpu_transfer_create_h_hn", mfgpu::TRANSFER_KIND_H_HN, c, f);
        in.parent = parent.data();
        in.child = child.data();
        in.coarse_mask = c.d.constraint_mask;
        in.fine_mask = f.d.constraint_mask;
        in.constraint_weights = c.d.constraint_weights;
        // (at p = 1 a cell may list no dof alone, which the refusals need; p = 2 and 4 run them)
        build_and_check(in, tag_of("h_hn", dim, 0, p) + " n_ref " + std::to_string(dr[1]) + " step " + std::to_string(step), p > 1 && n > 1);
        fine_leaves.swap(coarse_leaves);
      }
    }
  // empty transfers build, without arrays
  for (int kind = 0; kind < 3; ++kind) {
    TransferInput in;
    in.who = "empty";
    in.kind = kind;
    in.dim = 2;
    in.degree = 2;
    in.degree_coarse = 1;
    in.number_type = MFGPU_F32;
    TransferImage img;
    expect(mfgpu::build_transfer_image(in, img) == 0 && img.coarse.empty() && img.fine.empty() && img.covered == 0, "an empty transfer");
  }
  // constrained_position against the literal restatement: every valid mask, n = 2..7, both dimensions, every position
  long cases = 0, differ = 0;
  for (int dim = 2; dim <= 3; ++dim)
    for (uint32_t m = 0; m < 0x200u; ++m) {
      if (!mfgpu::valid_mask(dim, m)) continue;
      for (int n = 2; n <= 7; ++n)
        for (int t = 0; t < ipow(n, dim); ++t, ++cases) differ += mfgpu::constrained_position(dim, n, m, t) != literal_constrained(dim, n, m, t);
    }
  std::printf("constrained_position: %ld cases, %ld differ\n", cases, differ);
  expect(differ == 0 && cases == 403120, "constrained_position agrees with the nine mask bits on all 403120 cases");
  std::printf("done bad=%d\n", bad);
  return bad != 0;
}
