// gmvae_knn_*: the host side of csrc/neigh.hpp (include/gmvae_hip.h).  A translation unit -- and so a device code object -- of its
// own, for the reason csrc/tsne.hip gives: the training step's code object, and with it the placement of the one-launch step's
// code, is what it was without these kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gmvae_hip.h"
#include "hostutil.hpp"
#include "neigh.hpp"

using namespace gmvae;

namespace {

// Workspace, a function of (Nq, Nr, C): search and ranks hold d [Nq][Nr] (fp32) in it, class_sums the slices' parts
// [nn_class_slices(Nr)][C][Nq] (fp64); both begin at its start -- every call leaves it free for the next.
uint64_t nn_dist_bytes(int64_t Nq, int64_t Nr) { return (uint64_t)Nq * (uint64_t)Nr * sizeof(float); }
uint64_t nn_class_bytes(int64_t Nq, int64_t Nr, int C) {
  return (uint64_t)nn_class_slices(Nr) * (uint64_t)C * (uint64_t)Nq * sizeof(double);
}

int nn_check_sizes(int64_t Nq, int64_t Nr, int L) {
  return (Nq < 1 || Nq > (1ll << 30) || Nr < 1 || Nr > (1ll << 24) || L < 1 || L > 4096) ? GMVAE_E_DIMS : 0;
}
int nn_check_self(int64_t Nq, int64_t Nr, int64_t self_offset) {
  return (self_offset < -1 || (self_offset >= 0 && self_offset > Nr - Nq)) ? GMVAE_E_DIMS : 0;
}

void nn_launch_dist(hipStream_t st, const float* q, int64_t Nq, const float* r, int64_t Nr, int L, float* d) {
  const TsSplit sp = ts_split(Nr, ts_slices(Nq));
  hipLaunchKernelGGL(knn_dist, dim3((unsigned)((Nq + kTsBlock - 1) / kTsBlock), (unsigned)sp.used), dim3(kTsBlock), 0, st, q, (int)Nq,
                     r, (int)Nr, L, sp.per_slice, d);
}

}  // namespace

extern "C" {

int gmvae_knn_workspace_bytes(int64_t Nq, int64_t Nr, int L, int k, int C, uint64_t* bytes) {
  if (int e = nn_check_sizes(Nq, Nr, L)) return e;
  if (k < 1 || k > kNnMaxK || k > Nr || C < 1 || C > kNnMaxK) return GMVAE_E_DIMS;
  if (!bytes) return GMVAE_E_NULL;
  const uint64_t a = nn_dist_bytes(Nq, Nr), b = nn_class_bytes(Nq, Nr, C);
  *bytes = ((a > b ? a : b) + 255) / 256 * 256;
  return 0;
}

int gmvae_knn_search(const float* q, int64_t Nq, const float* r, int64_t Nr, int L, int k, int64_t self_offset, int32_t* idx_out,
                     float* d2_out, void* workspace, void* stream) {
  if (int e = nn_check_sizes(Nq, Nr, L)) return e;
  if (int e = nn_check_self(Nq, Nr, self_offset)) return e;
  if (k < 1 || k > kNnMaxK || k > Nr - (self_offset >= 0 ? 1 : 0)) return GMVAE_E_DIMS;
  if (!q || !r || (!idx_out && !d2_out) || !workspace) return GMVAE_E_NULL;
  if (!aligned_to(q, 4) || !aligned_to(r, 4) || !aligned_to(idx_out, 4) || !aligned_to(d2_out, 4) || !aligned_to(workspace, 16))
    return GMVAE_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* const d = static_cast<float*>(workspace);
  (void)hipGetLastError();
  nn_launch_dist(st, q, Nq, r, Nr, L, d);
  hipLaunchKernelGGL(knn_select, dim3((unsigned)((Nq + kNnRows - 1) / kNnRows)), dim3(kTsBlock), 0, st, d, (int)Nq, (int)Nr, k,
                     (long long)self_offset, idx_out, d2_out);
  return (int)hipGetLastError();
}

int gmvae_knn_ranks(const float* q, int64_t Nq, const float* r, int64_t Nr, int L, int64_t self_offset, const int32_t* cand, int m,
                    int32_t* rank_out, void* workspace, void* stream) {
  if (int e = nn_check_sizes(Nq, Nr, L)) return e;
  if (int e = nn_check_self(Nq, Nr, self_offset)) return e;
  if (m < 1 || m > kNnMaxK) return GMVAE_E_DIMS;
  if (!q || !r || !cand || !rank_out || !workspace) return GMVAE_E_NULL;
  if (!aligned_to(q, 4) || !aligned_to(r, 4) || !aligned_to(cand, 4) || !aligned_to(rank_out, 4) || !aligned_to(workspace, 16))
    return GMVAE_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* const d = static_cast<float*>(workspace);
  (void)hipGetLastError();
  nn_launch_dist(st, q, Nq, r, Nr, L, d);
  hipLaunchKernelGGL(knn_rank, dim3((unsigned)((Nq + kNnRows - 1) / kNnRows)), dim3(kTsBlock), 0, st, d, (int)Nq, (int)Nr,
                     (long long)self_offset, cand, m, rank_out);
  return (int)hipGetLastError();
}

int gmvae_knn_class_sums(const float* q, int64_t Nq, const float* r, int64_t Nr, int L, const int32_t* labels, int C,
                         double* sums_out, void* workspace, void* stream) {
  if (int e = nn_check_sizes(Nq, Nr, L)) return e;
  if (C < 1 || C > kNnMaxK) return GMVAE_E_DIMS;
  if (!q || !r || !labels || !sums_out || !workspace) return GMVAE_E_NULL;
  if (!aligned_to(q, 4) || !aligned_to(r, 4) || !aligned_to(labels, 4) || !aligned_to(sums_out, 8) || !aligned_to(workspace, 16))
    return GMVAE_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* const part = static_cast<double*>(workspace);
  const int ns = nn_class_slices(Nr);
  const dim3 grid((unsigned)((Nq + kTsBlock - 1) / kTsBlock), (unsigned)ns);
  (void)hipGetLastError();
  if (C <= kNnLdsClasses)
    hipLaunchKernelGGL(knn_class<true>, grid, dim3(kTsBlock), 0, st, q, (int)Nq, r, (int)Nr, L, labels, C, part);
  else
    hipLaunchKernelGGL(knn_class<false>, grid, dim3(kTsBlock), 0, st, q, (int)Nq, r, (int)Nr, L, labels, C, part);
  const uint64_t E = (uint64_t)Nq * (uint64_t)C;
  hipLaunchKernelGGL(knn_fold, dim3((unsigned)((E + kTsBlock - 1) / kTsBlock)), dim3(kTsBlock), 0, st, sums_out, part, (int)Nq, C, ns);
  return (int)hipGetLastError();
}

}  // extern "C"
