// gmvae_mixfit_* and gmvae_mixfit_full_*: the host side of csrc/mixfit.hpp and csrc/mixfit_full.hpp (include/gmvae_hip.h).  A translation unit of its own, for the reason at the top
// of csrc/tsne.hip: the model-independent evaluator's kernels, descriptors and symbols stay out of the training step's code object.
// What the two fits' entry points share stands once, at the top: the N and K gate, the n_iter / reg_covar check and the iteration
// loop's optional outputs; the pointer and alignment ladder and the once-per-device LDS attribute are csrc/hostutil.hpp's.  Each
// fit's own L and product gate, workspace layout and launches stay beside its plan.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gmvae_hip.h"
#include "hostutil.hpp"
#include "mixfit.hpp"
#include "mixfit_full.hpp"

using namespace gmvae;

namespace {

// the checks, in the header's order: sizes -- the gate on N and K here, each fit's L and product next to it --, then n_iter and
// reg_covar (run), then NULL, then alignment
bool nk_in_gate(int64_t N, int K) { return N >= 1 && N <= (1ll << 24) && K >= 1 && K <= 256; }

int check_iterations(int n_iter, float reg_covar) {
  return (n_iter < 0 || !(reg_covar > 0.f) || !isfinite(reg_covar)) ? GMVAE_E_DIMS : 0;
}

// n_iter times iteration(it, history slot `it` or NULL, counts_out on the last iteration or NULL)
template <class Iteration>
int run_iterations(int n_iter, float* loglik_history, float* counts_out, Iteration iteration) {
  for (int it = 0; it < n_iter; ++it)
    iteration(it, loglik_history ? loglik_history + it : nullptr, it == n_iter - 1 ? counts_out : nullptr);
  return (int)hipGetLastError();
}

// -------------------------------------------------------------------------------------------- diagonal covariances
int mf_check_sizes(int64_t N, int L, int K) {
  return (!nk_in_gate(N, K) || L < 1 || L > 4096 || (int64_t)K * L > kMfMaxKL) ? GMVAE_E_DIMS : 0;
}

// Workspace, a function of (N, L, K): the workgroups' partial sums [groups][stride] (fp64).  Nothing is kept per row.
uint64_t mf_workspace_bytes(const MfPlan& p) { return ((uint64_t)p.groups * (uint64_t)p.stride * sizeof(double) + 15) / 16 * 16; }

void mf_allow_lds() {
  static bool seen[64];
  allow_lds(seen, {reinterpret_cast<const void*>(mixfit_pass<true>), reinterpret_cast<const void*>(mixfit_pass<false>)}, kMfLdsBytes);
}

// ------------------------------------------------------------------------------------------------ full covariances
int mff_check_sizes(int64_t N, int L, int K) {
  return (!nk_in_gate(N, K) || L < 1 || L > kMffMaxL || (int64_t)K * L * L > kMffMaxKLL) ? GMVAE_E_DIMS : 0;
}

// Workspace, in doubles: W [K][L (L + 1) / 2], sum ln C_dd [K], then the workgroups' partial sums [groups][stride].  Nothing per row.
uint64_t mff_part_offset(int L, int K) { return (uint64_t)K * (uint64_t)mff_tri(L) + (uint64_t)K; }
uint64_t mff_workspace_bytes(const MffPlan& p, int L, int K) {
  return ((mff_part_offset(L, K) + (uint64_t)p.groups * (uint64_t)p.stride) * sizeof(double) + 15) / 16 * 16;
}

void mff_allow_lds() {
  static bool seen[64];
  allow_lds(seen, {reinterpret_cast<const void*>(mixfit_full_factor), reinterpret_cast<const void*>(mixfit_full_pass<true>),
                   reinterpret_cast<const void*>(mixfit_full_pass<false>)}, kMfLdsBytes);
}

}  // namespace

extern "C" {

int gmvae_mixfit_workspace_bytes(int64_t N, int L, int K, uint64_t* bytes) {
  if (int e = mf_check_sizes(N, L, K)) return e;
  if (!bytes) return GMVAE_E_NULL;
  *bytes = mf_workspace_bytes(mf_plan(N, L, K));
  return 0;
}

int gmvae_mixfit_assign(const float* codes, int64_t N, int L, int K, const float* logw, const float* mu, const float* sigma,
                        float* log_resp_out, float* lse_out, void* workspace, void* stream) {
  if (int e = mf_check_sizes(N, L, K)) return e;
  if (int e = check_pointers({codes, logw, mu, sigma}, {log_resp_out, lse_out}, workspace)) return e;
  const MfPlan p = mf_plan(N, L, K);
  (void)hipGetLastError();
  mf_allow_lds();
  hipLaunchKernelGGL(mixfit_pass<false>, dim3((unsigned)p.groups), dim3(kMfBlock), p.lds, static_cast<hipStream_t>(stream), codes, (int)N,
                     L, K, logw, mu, sigma, p.tile, p.per_group, log_resp_out, lse_out, (double*)nullptr, p.stride);
  return (int)hipGetLastError();
}

int gmvae_mixfit_run(const float* codes, int64_t N, int L, int K, float* logw, float* mu, float* sigma, float reg_covar, int n_iter,
                     float* loglik_history, float* counts_out, void* workspace, void* stream) {
  if (int e = mf_check_sizes(N, L, K)) return e;
  if (int e = check_iterations(n_iter, reg_covar)) return e;
  if (int e = check_pointers({codes, logw, mu, sigma}, {loglik_history, counts_out}, workspace)) return e;
  if (n_iter == 0) return 0;
  const MfPlan p = mf_plan(N, L, K);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* const part = static_cast<double*>(workspace);
  const unsigned update_blocks = (unsigned)((K * L + kMfFoldSlots - 1) / kMfFoldSlots) + 1;
  (void)hipGetLastError();
  mf_allow_lds();
  return run_iterations(n_iter, loglik_history, counts_out, [&](int, float* hist, float* counts) {
    hipLaunchKernelGGL(mixfit_pass<true>, dim3((unsigned)p.groups), dim3(kMfBlock), p.lds, st, codes, (int)N, L, K, logw, mu, sigma,
                       p.tile, p.per_group, (float*)nullptr, (float*)nullptr, part, p.stride);
    hipLaunchKernelGGL(mixfit_update, dim3(update_blocks), dim3(kMfBlock), 0, st, part, p.groups, p.stride, (int)N, L, K, reg_covar, logw,
                       mu, sigma, hist, counts);
  });
}

int gmvae_mixfit_full_workspace_bytes(int64_t N, int L, int K, uint64_t* bytes) {
  if (int e = mff_check_sizes(N, L, K)) return e;
  if (!bytes) return GMVAE_E_NULL;
  *bytes = mff_workspace_bytes(mff_plan(N, L, K), L, K);
  return 0;
}

int gmvae_mixfit_full_assign(const float* codes, int64_t N, int L, int K, const float* logw, const float* mu, const float* cov,
                             float* log_resp_out, float* lse_out, int32_t* info_out, void* workspace, void* stream) {
  if (int e = mff_check_sizes(N, L, K)) return e;
  if (int e = check_pointers({codes, logw, mu, cov}, {log_resp_out, lse_out, info_out}, workspace)) return e;
  const MffPlan p = mff_plan(N, L, K);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* const W = static_cast<double*>(workspace);
  double* const sumlog = W + (size_t)K * mff_tri(L);
  (void)hipGetLastError();
  mff_allow_lds();
  hipLaunchKernelGGL(mixfit_full_factor, dim3((unsigned)K), dim3(kMfBlock), p.lds_factor, st, cov, L, W, sumlog, info_out, 1);
  hipLaunchKernelGGL(mixfit_full_pass<false>, dim3((unsigned)p.groups), dim3(kMfBlock), p.lds, st, codes, (int)N, L, K, logw, mu,
                     (const double*)W, (const double*)sumlog, p.tile, p.per_group, log_resp_out, lse_out, (double*)nullptr, p.stride);
  return (int)hipGetLastError();
}

int gmvae_mixfit_full_run(const float* codes, int64_t N, int L, int K, float* logw, float* mu, float* cov, float reg_covar, int n_iter,
                          float* loglik_history, float* counts_out, int32_t* info_out, void* workspace, void* stream) {
  if (int e = mff_check_sizes(N, L, K)) return e;
  if (int e = check_iterations(n_iter, reg_covar)) return e;
  if (int e = check_pointers({codes, logw, mu, cov}, {loglik_history, counts_out, info_out}, workspace)) return e;
  if (n_iter == 0) return 0;
  const MffPlan p = mff_plan(N, L, K);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* const W = static_cast<double*>(workspace);
  double* const sumlog = W + (size_t)K * mff_tri(L);
  double* const part = W + mff_part_offset(L, K);
  const unsigned update_blocks = (unsigned)((K * mff_tri(L) + kMfFoldSlots - 1) / kMfFoldSlots) + 1;
  (void)hipGetLastError();
  mff_allow_lds();
  return run_iterations(n_iter, loglik_history, counts_out, [&](int it, float* hist, float* counts) {
    hipLaunchKernelGGL(mixfit_full_factor, dim3((unsigned)K), dim3(kMfBlock), p.lds_factor, st, (const float*)cov, L, W, sumlog, info_out,
                       it == 0 ? 1 : 0);
    hipLaunchKernelGGL(mixfit_full_pass<true>, dim3((unsigned)p.groups), dim3(kMfBlock), p.lds, st, codes, (int)N, L, K,
                       (const float*)logw, (const float*)mu, (const double*)W, (const double*)sumlog, p.tile, p.per_group,
                       (float*)nullptr, (float*)nullptr, part, p.stride);
    hipLaunchKernelGGL(mixfit_full_update, dim3(update_blocks), dim3(kMfBlock), 0, st, (const double*)part, p.groups, p.stride, (int)N, L,
                       K, reg_covar, logw, mu, cov, hist, counts);
  });
}

}  // extern "C"
