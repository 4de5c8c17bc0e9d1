// Pass 2 of the two-pass scatter: dst = sum of the partial sums the batches left in the halo buffer, for every dof
// on the pass-2 route (shared between batches, or demoted to this route by the plan), in ascending batch order
// (deterministic; the reference adds with atomics in arbitrary order, fee_gpu.cuh:359-362); constrained rows are
// identity rows, dst = src (laplace_operator_gpu.h:300-302, constraint_handler_gpu.cu:276-289).
//
// The dofs are sorted by their number of partial sums k into CLASSES (k = 2: interior of a face between two batches,
// 4: an edge, 8: a vertex, 1: demoted; other values on irregular meshes).  A class is stored structure-of-arrays --
// dof ids, then k arrays of halo slots -- so a thread's k + 1 index loads are independent and coalesced and the whole
// reduction is TWO dependent memory round trips (indices, partial sums) instead of the four of a descriptor ->
// group starts -> partials chain; every thread carries two dofs.  A 512-entry tile per workgroup; a class is padded
// to whole tiles with 0xffffffff.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mfgpu_kernels.h"

namespace mfgpu {

namespace {

// Width NV (mfgpu_vmult_multi): NV = 1 is the single apply, its halo buffer a plain pointer argument; a fused group of
// NV = 2, 3 vectors passes its halo buffers and the vectors' stride in a GroupHalos<T>.  The dof ids and the K halo
// slots of a thread's two entries are loaded once; then, per vector, the sums in the same order (slot 0 first,
// ascending touchers) from that vector's halo buffer into dst + v * stride (identity rows: from src + v * stride).
template <typename T>
struct GroupHalos {
  size_t stride;
  const T *h[kMaxFusedWidth];
};
template <typename T, typename P>
__device__ __forceinline__ P *vec_at(const T *, P *p, int) { return p; }
template <typename T, typename P>
__device__ __forceinline__ P *vec_at(const GroupHalos<T> &g, P *p, int v) { return p + (size_t)v * g.stride; }
template <typename T>
__device__ __forceinline__ const T *vec_halo(const T *halo, int) { return halo; }
template <typename T>
__device__ __forceinline__ const T *vec_halo(const GroupHalos<T> &g, int v) { return g.h[v]; }

template <typename T, int NV>
using HalosArg = std::conditional_t<NV == 1, const T *__restrict__, GroupHalos<T>>;

template <typename T, int K, int NV>
__device__ __forceinline__ void reduce_two(T *__restrict__ dst0, const T *__restrict__ src0, const HalosArg<T, NV> halos,
                                           const uint32_t *__restrict__ p, uint32_t cnt, uint32_t i0, uint32_t k,
                                           int add) {
  // K > 0: compile-time number of partial sums; K == 0: run-time k (rare classes)
  const uint32_t i1 = i0 + 256u;
  const uint32_t d0 = p[i0], d1 = p[i1];
  constexpr int KU = K > 0 ? K : 1;
  uint32_t s0[KU], s1[KU];
#pragma unroll
  for (int t = 0; t < KU; ++t) {
    s0[t] = p[(size_t)(1 + t) * cnt + i0];
    s1[t] = p[(size_t)(1 + t) * cnt + i1];
  }
  const bool on0 = d0 != 0xffffffffu, on1 = d1 != 0xffffffffu;
  const uint32_t g0 = d0 & 0x7fffffffu, g1 = d1 & 0x7fffffffu;
#pragma unroll
  for (int iv = 0; iv < NV; ++iv) {
    const int v = NV == 1 ? 0 : iv;  // (with the break below: no loop at NV = 1, see apply_batches_g)
    const T *__restrict__ halo = vec_halo(halos, v);
    const T *__restrict__ src = vec_at(halos, src0, v);
    T *__restrict__ dst = vec_at(halos, dst0, v);
    T v0 = T(0), v1 = T(0), o0 = T(0), o1 = T(0);
    if (on0) {
      if (d0 >> 31) {
        v0 = src[g0];
      } else {
        T q[KU];
#pragma unroll
        for (int t = 0; t < KU; ++t) q[t] = halo[s0[t]];
        v0 = q[0];
#pragma unroll
        for (int t = 1; t < KU; ++t) v0 += q[t];
        if (K == 0)
          for (uint32_t t = 1; t < k; ++t) v0 += halo[p[(size_t)(1 + t) * cnt + i0]];
      }
      if (add) o0 = dst[g0];
    }
    if (on1) {
      if (d1 >> 31) {
        v1 = src[g1];
      } else {
        T q[KU];
#pragma unroll
        for (int t = 0; t < KU; ++t) q[t] = halo[s1[t]];
        v1 = q[0];
#pragma unroll
        for (int t = 1; t < KU; ++t) v1 += q[t];
        if (K == 0)
          for (uint32_t t = 1; t < k; ++t) v1 += halo[p[(size_t)(1 + t) * cnt + i1]];
      }
      if (add) o1 = dst[g1];
    }
    if (on0) dst[g0] = add ? o0 + v0 : v0;
    if (on1) dst[g1] = add ? o1 + v1 : v1;
    if (NV == 1) break;
  }
}

template <typename T, int NV>
__global__ void __launch_bounds__(256)
reduce_classes(T *__restrict__ dst, const T *__restrict__ src, const HalosArg<T, NV> halos,
               const uint32_t *__restrict__ arr, const uint4 *__restrict__ tiles, int add) {
  const uint4 td = tiles[blockIdx.x];  // {class base in arr, k, entries of the class (padded), first entry of the tile}
  const uint32_t *p = arr + td.x;
  const uint32_t i0 = td.w + threadIdx.x;
  switch (td.y) {  // wave-uniform
    case 1: reduce_two<T, 1, NV>(dst, src, halos, p, td.z, i0, 1, add); break;
    case 2: reduce_two<T, 2, NV>(dst, src, halos, p, td.z, i0, 2, add); break;
    case 3: reduce_two<T, 3, NV>(dst, src, halos, p, td.z, i0, 3, add); break;
    case 4: reduce_two<T, 4, NV>(dst, src, halos, p, td.z, i0, 4, add); break;
    case 8: reduce_two<T, 8, NV>(dst, src, halos, p, td.z, i0, 8, add); break;
    default: reduce_two<T, 0, NV>(dst, src, halos, p, td.z, i0, td.y, add); break;
  }
}

// ---- Shared form (Plan::sh_p2rec / sh_p2tab, mfgpu_plan.cpp share_pass2_records): one workgroup per OWNER batch (the
// batch of a dof's first partial sum).  Where the numbering repeats from batch to batch the per-dof index words of
// reduce_classes (42 MB read once per vmult on the 54^3 mesh at p = 4) are 27 distinct records: the record is read from
// L2, and only the partial sums, src at identity rows and dst move through the fabric.  A record lists the batch's dofs
// sorted by k descending, so a wave's largest k is its first lane's; the lanes sum their own k <= that many partial sums
// in ascending toucher order -- the order, and hence the bits, of reduce_classes.
template <typename T, int K>
__device__ __forceinline__ void reduce_owned(T *__restrict__ dst, const T *__restrict__ src,
                                             const T *__restrict__ halo, const uint32_t *__restrict__ r, uint32_t e,
                                             uint32_t d, uint32_t kk, uint32_t kw, uint32_t hslot0, uint32_t hstride,
                                             int add) {
  // K > 0: compile-time bound of the wave's largest k; K == 0: run-time bound kw
  const T *const hb = halo + hslot0;  // the owner batch's first halo slot
  auto partial = [&](uint32_t w) -> T {
    return hb[(w >> kP2SlotBits) * hstride + (w & ((1u << kP2SlotBits) - 1u))];
  };
  constexpr int KU = K > 0 ? K : 1;
  uint32_t w[KU];
#pragma unroll
  for (int t = 0; t < KU; ++t) w[t] = (uint32_t)t < kk ? r[r[3 + t] + e] : 0u;
  if (d == 0xffffffffu) return;  // padding of the record's last wave
  T v;
  if (d >> 31) {
    v = src[d & 0x7fffffffu];
  } else {
    T q[KU];
#pragma unroll
    for (int t = 0; t < KU; ++t) q[t] = (uint32_t)t < kk ? partial(w[t]) : T(0);
    v = q[0];
#pragma unroll
    for (int t = 1; t < KU; ++t)
      if ((uint32_t)t < kk) v += q[t];
    if (K == 0)
      for (uint32_t t = 1; t < kw; ++t)
        if (t < kk) v += partial(r[r[3 + t] + e]);
  }
  T *const out = dst + (d & 0x7fffffffu);
  *out = add ? *out + v : v;
}

template <typename T>
__global__ void __launch_bounds__(256)
reduce_owner_batches(T *__restrict__ dst, const T *__restrict__ src, const T *__restrict__ halo,
                     const uint32_t *__restrict__ rec, const uint2 *__restrict__ tab, uint32_t n_batches,
                     uint32_t hstride, int reverse, int add) {
  const uint32_t ob = reverse ? n_batches - 1u - blockIdx.x : blockIdx.x;
  const uint2 t = tab[ob];  // {dof base, word offset of the batch's record}
  const uint32_t *const r = rec + t.y;
  const uint32_t e0 = r[1];  // entries, padded to whole waves
  dst += t.x;  // the record's dof ids are relative to the batch's dof base
  src += t.x;
  for (uint32_t e = threadIdx.x; e < e0; e += 256u) {  // (wave-uniform trip count)
    const uint32_t d = r[kP2Header + e], kk = r[kP2Header + e0 + e];
    const uint32_t kw = (uint32_t)__builtin_amdgcn_readfirstlane((int)kk);  // the wave's largest k
    const uint32_t h0 = ob * hstride;
    switch (kw) {  // wave-uniform
      case 0: break;
      case 1: reduce_owned<T, 1>(dst, src, halo, r, e, d, kk, kw, h0, hstride, add); break;
      case 2: reduce_owned<T, 2>(dst, src, halo, r, e, d, kk, kw, h0, hstride, add); break;
      case 3: reduce_owned<T, 3>(dst, src, halo, r, e, d, kk, kw, h0, hstride, add); break;
      case 4: reduce_owned<T, 4>(dst, src, halo, r, e, d, kk, kw, h0, hstride, add); break;
      case 5: case 6: case 7:
      case 8: reduce_owned<T, 8>(dst, src, halo, r, e, d, kk, kw, h0, hstride, add); break;
      default: reduce_owned<T, 0>(dst, src, halo, r, e, d, kk, kw, h0, hstride, add); break;
    }
  }
}

}  // namespace

// Host side: (sdofs, s_off, s_idx) of the plan -> class arrays.  `arr` = for every class [dofs | slots_0 | ... |
// slots_{k-1}], each `entries` long; `tiles` = one uint4 per 512 entries.
void build_pass2_classes(const std::vector<uint32_t> &sdofs, const std::vector<uint32_t> &s_off,
                         const std::vector<uint32_t> &s_idx, std::vector<uint32_t> &arr, std::vector<uint32_t> &tiles) {
  arr.clear();
  tiles.clear();
  const size_t ns = sdofs.size();
  uint32_t kmax = 0;
  for (size_t i = 0; i < ns; ++i) kmax = std::max(kmax, s_off[i + 1] - s_off[i]);
  std::vector<std::vector<uint32_t>> members(kmax + 1);
  for (size_t i = 0; i < ns; ++i) {
    uint32_t k = s_off[i + 1] - s_off[i];
    if (k == 0) k = 1;  // constrained dof listed without a partial sum: its slot entries are never read
    members[k].push_back((uint32_t)i);
  }
  for (uint32_t k = 1; k <= kmax; ++k) {
    const std::vector<uint32_t> &m = members[k];
    if (m.empty()) continue;
    const uint32_t entries = (uint32_t)((m.size() + 511) / 512 * 512);
    const uint32_t base = (uint32_t)arr.size();
    arr.resize(arr.size() + (size_t)(1 + k) * entries, 0u);
    for (uint32_t e = 0; e < entries; ++e) arr[base + e] = e < m.size() ? sdofs[m[e]] : 0xffffffffu;
    for (size_t e = 0; e < m.size(); ++e) {
      const uint32_t i = m[e], cnt = s_off[i + 1] - s_off[i];
      for (uint32_t t = 0; t < k; ++t) arr[base + (size_t)(1 + t) * entries + e] = t < cnt ? s_idx[s_off[i] + t] : 0u;
    }
    for (uint32_t first = 0; first < entries; first += 512) {
      tiles.push_back(base);
      tiles.push_back(k);
      tiles.push_back(entries);
      tiles.push_back(first);
    }
  }
}

template <typename T>
hipError_t reduce_classes_launch(T *dst, const T *src, const T *halo, const uint32_t *arr, const uint32_t *tiles,
                                 uint32_t n_tiles, int add, hipStream_t st) {
  if (n_tiles == 0) return hipSuccess;
  hipLaunchKernelGGL((reduce_classes<T, 1>), dim3(n_tiles), dim3(256), 0, st, dst, src, halo, arr,
                     reinterpret_cast<const uint4 *>(tiles), add);
  return hipGetLastError();
}
template <typename T>
hipError_t reduce_classes_multi_launch(int nv, T *dst, const T *src, size_t stride, T *const *halos, const uint32_t *arr,
                                       const uint32_t *tiles, uint32_t n_tiles, int add, hipStream_t st) {
  if (n_tiles == 0) return hipSuccess;
  if (nv != 2 && nv != 3) return hipErrorInvalidValue;
  GroupHalos<T> gh;
  gh.stride = stride;
  for (int v = 0; v < kMaxFusedWidth; ++v) gh.h[v] = v < nv ? halos[v] : nullptr;
  const uint4 *t4 = reinterpret_cast<const uint4 *>(tiles);
  if (nv == 2)
    hipLaunchKernelGGL((reduce_classes<T, 2>), dim3(n_tiles), dim3(256), 0, st, dst, src, gh, arr, t4, add);
  else
    hipLaunchKernelGGL((reduce_classes<T, 3>), dim3(n_tiles), dim3(256), 0, st, dst, src, gh, arr, t4, add);
  return hipGetLastError();
}
template hipError_t reduce_classes_multi_launch<double>(int, double *, const double *, size_t, double *const *,
                                                        const uint32_t *, const uint32_t *, uint32_t, int, hipStream_t);
template hipError_t reduce_classes_multi_launch<float>(int, float *, const float *, size_t, float *const *,
                                                       const uint32_t *, const uint32_t *, uint32_t, int, hipStream_t);
template <typename T>
hipError_t reduce_owner_batches_launch(T *dst, const T *src, const T *halo, const uint32_t *rec, const uint32_t *tab,
                                       uint32_t n_batches, uint32_t hstride, int reverse, int add, hipStream_t st) {
  if (n_batches == 0) return hipSuccess;
  hipLaunchKernelGGL(reduce_owner_batches<T>, dim3(n_batches), dim3(256), 0, st, dst, src, halo, rec,
                     reinterpret_cast<const uint2 *>(tab), n_batches, hstride, reverse, add);
  return hipGetLastError();
}
template hipError_t reduce_owner_batches_launch<double>(double *, const double *, const double *, const uint32_t *,
                                                        const uint32_t *, uint32_t, uint32_t, int, int, hipStream_t);
template hipError_t reduce_owner_batches_launch<float>(float *, const float *, const float *, const uint32_t *,
                                                       const uint32_t *, uint32_t, uint32_t, int, int, hipStream_t);
template hipError_t reduce_classes_launch<double>(double *, const double *, const double *, const uint32_t *,
                                                  const uint32_t *, uint32_t, int, hipStream_t);
template hipError_t reduce_classes_launch<float>(float *, const float *, const float *, const uint32_t *,
                                                 const uint32_t *, uint32_t, int, hipStream_t);

}  // namespace mfgpu
