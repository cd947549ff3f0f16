// gmvae_linprobe_*: the host side of csrc/linprobe.hpp (include/gmvae_hip.h).  A translation unit of its own, for the reason at the
// top of csrc/tsne.hip: the model-independent evaluator's kernels, descriptors and symbols stay out of the training step's code
// object.  The pointer ladder and the LDS attribute are csrc/hostutil.hpp's, shared with csrc/mixfit.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gmvae_hip.h"
#include "hostutil.hpp"
#include "linprobe.hpp"

using namespace gmvae;

namespace {

int lp_check_sizes(int64_t N, int L, int C) {
  return (N < 1 || N > (1ll << 24) || L < 1 || L > kLpMaxL || C < 2 || C > kLpMaxC || (int64_t)C * L > kLpMaxCL) ? GMVAE_E_DIMS : 0;
}

uint64_t lp_workspace_bytes(const LpPlan& p, int L, int C) {
  return ((lp_layout(L, C).part + lp_part_doubles(p)) * sizeof(double) + 15) / 16 * 16;
}

void lp_allow_lds() {
  static bool seen[64];
  allow_lds(seen, {reinterpret_cast<const void*>(linprobe_gram), reinterpret_cast<const void*>(linprobe_setup),
                   reinterpret_cast<const void*>(linprobe_pass<true>), reinterpret_cast<const void*>(linprobe_pass<false>)}, kMfLdsBytes);
}

}  // namespace

extern "C" {

int gmvae_linprobe_workspace_bytes(int64_t N, int L, int C, uint64_t* bytes) {
  if (int e = lp_check_sizes(N, L, C)) return e;
  if (!bytes) return GMVAE_E_NULL;
  *bytes = lp_workspace_bytes(lp_plan(N, L, C), L, C);
  return 0;
}

int gmvae_linprobe_fit(const float* codes, const int32_t* labels, int64_t N, int L, int C, double l2, int n_iter, float* W_out,
                       float* b_out, float* loss_history, float* grad_max_out, int32_t* info_out, void* workspace, void* stream) {
  if (int e = lp_check_sizes(N, L, C)) return e;
  if (n_iter < 0 || !(l2 > 0.0) || !isfinite(l2)) return GMVAE_E_DIMS;
  if (int e = check_pointers({codes, labels, W_out, b_out}, {loss_history, grad_max_out, info_out}, workspace)) return e;
  const LpPlan p = lp_plan(N, L, C);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* const ws = static_cast<double*>(workspace);
  double* const part = ws + lp_layout(L, C).part;
  (void)hipGetLastError();
  lp_allow_lds();
  // the set-up, three launches: the labelled rows' moments per row slice, the centred Gram sums per row slice, then one workgroup
  hipLaunchKernelGGL(linprobe_moments, dim3((unsigned)p.setup_groups), dim3(kMfBlock), 0, st, codes, labels, (int)N, L, C, p.setup_per_group,
                     part, p.setup_stride);
  hipLaunchKernelGGL(linprobe_gram, dim3((unsigned)p.setup_groups), dim3(kMfBlock), p.lds_gram, st, codes, labels, (int)N, L, C, p.setup_tile,
                     p.setup_per_group, p.setup_groups, part, p.setup_stride);
  hipLaunchKernelGGL(linprobe_setup, dim3(1), dim3(kMfBlock), p.lds_setup, st, (const double*)part, p.setup_groups, p.setup_stride, L, C, l2,
                     n_iter, ws, W_out, b_out, loss_history, grad_max_out, info_out);
  double t = 1.0;
  for (int it = 0; it < n_iter; ++it) {
    const double t1 = (1.0 + sqrt(1.0 + 4.0 * t * t)) / 2.0, beta = (t - 1.0) / t1;
    t = t1;
    hipLaunchKernelGGL(linprobe_pass<true>, dim3((unsigned)p.groups), dim3(kMfBlock), p.lds, st, codes, labels, (int)N, L, C,
                       (const double*)ws, (const float*)nullptr, (const float*)nullptr, p.tile, p.per_group, (float*)nullptr,
                       (int32_t*)nullptr, part, p.stride);
    hipLaunchKernelGGL(linprobe_update, dim3((unsigned)C), dim3(kMfBlock), 0, st, (const double*)part, p.groups, p.stride, L, C, l2, beta,
                       it, it == n_iter - 1 ? 1 : 0, ws, W_out, b_out, loss_history, grad_max_out);
  }
  return (int)hipGetLastError();
}

int gmvae_linprobe_predict(const float* codes, const int32_t* labels, int64_t N, int L, int C, const float* W, const float* b,
                           float* log_prob_out, int32_t* pred_out, double* sums_out, void* workspace, void* stream) {
  if (int e = lp_check_sizes(N, L, C)) return e;
  if (int e = check_pointers({codes, W, b}, {labels, log_prob_out, pred_out}, workspace)) return e;
  if (!aligned_to(sums_out, 8)) return GMVAE_E_ALIGN;
  const LpPlan p = lp_plan(N, L, C);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* const part = static_cast<double*>(workspace) + lp_layout(L, C).part;
  (void)hipGetLastError();
  lp_allow_lds();
  hipLaunchKernelGGL(linprobe_pass<false>, dim3((unsigned)p.groups), dim3(kMfBlock), p.lds, st, codes, labels, (int)N, L, C,
                     (const double*)nullptr, W, b, p.tile, p.per_group, log_prob_out, pred_out, part, 3);
  if (sums_out) hipLaunchKernelGGL(linprobe_sums, dim3(1), dim3(64), 0, st, (const double*)part, p.groups, sums_out);
  return (int)hipGetLastError();
}

}  // extern "C"
