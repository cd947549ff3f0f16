// gmvae_pca_*, gmvae_sym_eigh: the host side of csrc/pca.hpp (include/gmvae_hip.h).  A translation unit of its own, for the reason at
// the top of csrc/tsne.hip: the model-independent evaluator's kernels, descriptors and symbols stay out of the training step's code
// object.  The pointer ladder and the LDS attribute are csrc/hostutil.hpp's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gmvae_hip.h"
#include "hostutil.hpp"
#include "pca.hpp"

using namespace gmvae;

namespace {

int pca_check_sizes(int64_t N, int D, int k, int m) {
  if (N < 2 || N > (1ll << 24) || D < 1 || D > kPcaMaxD) return GMVAE_E_DIMS;
  if (k < 1 || k > m || m > D || m > kPcaMaxM) return GMVAE_E_DIMS;
  return (D <= kPcaMaxM && m != D) ? GMVAE_E_DIMS : 0;
}

PcaLayout pca_layout_of(const PcaPlan& p, int D, int m) { return pca_layout(D, m, p.mgroups, p.slices, p.nblk); }

void pca_allow_lds() {
  static bool seen[64];
  allow_lds(seen, {reinterpret_cast<const void*>(pca_cov), reinterpret_cast<const void*>(pca_eigh), reinterpret_cast<const void*>(pca_dense),
                   reinterpret_cast<const void*>(pca_orth), reinterpret_cast<const void*>(pca_ritz),
                   reinterpret_cast<const void*>(pca_transform)}, kMfLdsBytes);
}

bool all_aligned(Pointers ps, uintptr_t a) {
  for (const void* p : ps)
    if (!aligned_to(p, a)) return false;
  return true;
}

}  // namespace

extern "C" {

int gmvae_pca_workspace_bytes(int64_t N, int D, int m, uint64_t* bytes) {
  if (int e = pca_check_sizes(N, D, 1, m)) return e;
  if (!bytes) return GMVAE_E_NULL;
  *bytes = (pca_layout_of(pca_plan(N, D, m, m), D, m).end * sizeof(double) + 15) / 16 * 16;
  return 0;
}

int gmvae_pca_fit(const float* x, int64_t N, int D, int k, int m, int n_iter, int n_sweeps, const double* V0, double* mean_out,
                  double* components_out, double* variance_out, double* residual_out, double* stats_out, int32_t* info_out,
                  void* workspace, void* stream) {
  if (int e = pca_check_sizes(N, D, k, m)) return e;
  if (n_iter < 0 || n_sweeps < 1) return GMVAE_E_DIMS;
  const bool iterative = D > kPcaMaxM;
  if (int e = check_pointers({x, mean_out, components_out, variance_out, residual_out, stats_out}, {info_out}, workspace)) return e;
  if (iterative && !V0) return GMVAE_E_NULL;
  if (!all_aligned({V0, mean_out, components_out, variance_out, residual_out, stats_out}, 8)) return GMVAE_E_ALIGN;
  const PcaPlan p = pca_plan(N, D, m, k);
  const PcaLayout lay = pca_layout_of(p, D, m);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* const ws = static_cast<double*>(workspace);
  double *const mean = ws + lay.mean, *const C = ws + lay.c, *const Vt = ws + lay.vt;
  const double scale = 1.0 / (double)(N - 1);
  (void)hipGetLastError();
  pca_allow_lds();
  hipLaunchKernelGGL(pca_moments, dim3((unsigned)p.mgroups, (unsigned)p.mchunks), dim3(kMfBlock), 0, st, x, (int)N, D, p.mper, p.mcw, ws + lay.mpart);
  hipLaunchKernelGGL(pca_mean, dim3((unsigned)((D + kMfBlock - 1) / kMfBlock)), dim3(kMfBlock), 0, st, (const double*)(ws + lay.mpart), p.mgroups,
                     (int)N, D, mean, mean_out);
  hipLaunchKernelGGL(pca_cov, dim3((unsigned)p.nblk, (unsigned)p.slices), dim3(kMfBlock), 2 * kPcaMb * kPcaMbPad * sizeof(double), st, x, (int)N, D,
                     (const double*)mean, p.cper, p.slices, scale, C, ws + lay.cpart);
  if (p.slices > 1)
    hipLaunchKernelGGL(pca_cov_fold, dim3((unsigned)p.nblk, kPcaMb * kPcaMb / kMfBlock), dim3(kMfBlock), 0, st, (const double*)(ws + lay.cpart),
                       p.slices, D, scale, C);
  hipLaunchKernelGGL(pca_stats, dim3(1), dim3(kMfBlock), 0, st, (const double*)C, (int)N, D, ws, stats_out, info_out);
  if (!iterative) {
    hipLaunchKernelGGL(pca_dense, dim3(1), dim3(kMfBlock), p.lds_solve, st, (const double*)C, D, k, n_sweeps, Vt, components_out, variance_out,
                       residual_out, stats_out);
    return (int)hipGetLastError();
  }
  double *const V = ws + lay.v, *const W = ws + lay.w, *const Y = ws + lay.y, *const Z = ws + lay.z, *const cinvt = ws + lay.cinvt;
  double *const qs = ws + lay.qs, *const theta = ws + lay.theta;
  const dim3 grid((unsigned)p.nmb, (unsigned)((m + kPcaMb - 1) / kPcaMb));
  hipMemcpyAsync(V, V0, (size_t)D * m * sizeof(double), hipMemcpyDeviceToDevice, st);
  for (int it = 0; it <= n_iter; ++it) {
    hipLaunchKernelGGL(pca_gemm, grid, dim3(kMfBlock), 0, st, (const double*)ws, (const double*)C, D, (const double*)V, m, W, m, D, D, m);
    if (it == n_iter) break;
    hipLaunchKernelGGL(pca_orth, dim3(1), dim3(kMfBlock), p.lds_orth, st, ws, (const double*)W, D, m, k, cinvt, components_out, variance_out,
                       residual_out, stats_out, info_out);
    hipLaunchKernelGGL(pca_gemm, grid, dim3(kMfBlock), 0, st, (const double*)ws, (const double*)W, m, (const double*)cinvt, m, V, m, D, m, m);
  }
  hipLaunchKernelGGL(pca_ritz, dim3(1), dim3(kMfBlock), p.lds_solve, st, (const double*)ws, (const double*)V, (const double*)W, D, m, n_sweeps, Vt,
                     qs, theta, stats_out);
  hipLaunchKernelGGL(pca_gemm, grid, dim3(kMfBlock), 0, st, (const double*)ws, (const double*)V, m, (const double*)qs, m, Y, m, D, m, k);
  hipLaunchKernelGGL(pca_gemm, grid, dim3(kMfBlock), 0, st, (const double*)ws, (const double*)W, m, (const double*)qs, m, Z, m, D, m, k);
  hipLaunchKernelGGL(pca_finish, dim3((unsigned)k), dim3(kMfBlock), 0, st, (const double*)ws, (const double*)Y, (const double*)Z,
                     (const double*)theta, D, m, components_out, variance_out, residual_out);
  return (int)hipGetLastError();
}

int gmvae_pca_transform(const float* x, int64_t N, int D, int k, const double* mean, const double* components, const double* scale,
                        float* z_out, void* stream) {
  if (N < 1 || N > (1ll << 24) || D < 1 || D > kPcaMaxD || k < 1 || k > D || k > kPcaMaxM) return GMVAE_E_DIMS;
  if (!x || !mean || !components || !z_out) return GMVAE_E_NULL;
  if (!all_aligned({x, z_out}, 4) || !all_aligned({mean, components, scale}, 8)) return GMVAE_E_ALIGN;
  const PcaPlan p = pca_plan(N, D, k, k);
  (void)hipGetLastError();
  pca_allow_lds();
  hipLaunchKernelGGL(pca_transform, dim3((unsigned)p.tgroups), dim3(kMfBlock), p.lds_tr, static_cast<hipStream_t>(stream), x, (int)N, D, k, mean,
                     components, scale, p.tper, z_out);
  return (int)hipGetLastError();
}

int gmvae_sym_eigh(const double* A, int n, int n_sweeps, double* w_out, double* V_out, double* offdiag_out, void* workspace, void* stream) {
  if (n < 1 || n > kPcaMaxM || n_sweeps < 1) return GMVAE_E_DIMS;
  if (!A || !w_out || !V_out || !workspace) return GMVAE_E_NULL;
  if (!all_aligned({A, w_out, V_out, offdiag_out}, 8) || !aligned_to(workspace, 16)) return GMVAE_E_ALIGN;
  (void)hipGetLastError();
  pca_allow_lds();
  hipLaunchKernelGGL(pca_eigh, dim3(1), dim3(kMfBlock), pca_plan(2, n, n, n).lds_solve, static_cast<hipStream_t>(stream), A, n, n_sweeps,
                     static_cast<double*>(workspace), w_out, V_out, offdiag_out);
  return (int)hipGetLastError();
}

}  // extern "C"
