// What mfgpu_vcycle_refresh (mfgpu_vcycle.hip) shares with the enqueue-only set-up calls of mfgpu_refresh.hip.
#ifndef MFGPU_REFRESH_H
#define MFGPU_REFRESH_H

#include <cstddef>
#include <cstdint>

#include "mfgpu_internal.h"

namespace mfgpu {

// The state block of the device power iteration; which kernel writes which part is told in mfgpu_refresh.hip.
struct EigState {
  mfgpu_eig_result result;  // eig_normalise_kernel (estimate, steps and status also reset by eig_start_kernel)
  double prev;              // eig_scale_kernel: the estimate, the count and the end of the step before
  uint32_t steps_old, frozen;
  double pad[3];
};
constexpr size_t kEigStateBytes = 64;

// mfgpu_estimate_lambda_max_enqueue on pieces the caller places itself: the state block, 2 * kStreamBlocks doubles of
// partial sums and the two work vectors of the operator's number type
int eig_enqueue(mfgpu_handle *op, const void *dinv, uint32_t min_iterations, uint32_t n_steps, EigState *state,
                double *partials, void *v, void *w, void *stream);

}  // namespace mfgpu
#endif
