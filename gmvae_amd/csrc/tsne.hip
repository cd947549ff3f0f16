// gmvae_tsne_*: the host side of csrc/tsne.hpp (include/gmvae_hip.h).  A translation unit of its own, so a code object of its
// own: the model-independent evaluator's kernels, descriptors and symbols stay out of the training step's code object, whose
// layout -- and with it the one-launch step's time, which follows the placement of its 101 KB of code (profiles/tsne_notes.md)
// -- is then what it was without them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gmvae_hip.h"
#include "hostutil.hpp"
#include "tsne.hpp"

using namespace gmvae;

namespace {

int aligned16(const void* p) { return aligned_to(p, 16); }

// gmvae_tsne_*: csrc/tsne.hpp.  Workspace, a function of (N, rows): the slices' partial sums [ts_slices(N)][N][kTsAcc] and the
// folded sums [N][kTsAcc] (fp64), the statistics (4 fp64), the gradient [N][2] (fp32), then the affinity stage's d2 [rows][N]
// (fp32) -- the iteration's part comes first, so gmvae_tsne_gradient and gmvae_tsne_run need not know `rows`.  Checks in the
// order dims, NULL, alignment, all before any launch.
struct TsLayout {
  uint64_t part, pt, stats, grad, d2, bytes;
};
static TsLayout ts_layout(int64_t N, int64_t rows) {
  const auto up16 = [](uint64_t b) { return (b + 15) / 16 * 16; };
  TsLayout l;
  l.part = 0;
  l.pt = l.part + up16((uint64_t)ts_slices(N) * (uint64_t)N * kTsAcc * sizeof(double));
  l.stats = l.pt + up16((uint64_t)N * kTsAcc * sizeof(double));
  l.grad = l.stats + 64;
  l.d2 = l.grad + up16((uint64_t)N * 2 * sizeof(float));
  l.bytes = (l.d2 + (uint64_t)rows * (uint64_t)N * sizeof(float) + 255) / 256 * 256;
  return l;
}
static int ts_check_sizes(int64_t N, int L) {
  return (N < 4 || N > (1ll << 20) || L < 1 || L > (1 << 16)) ? GMVAE_E_DIMS : 0;
}

// pairs -> fold -> reduce -> grad on `st`; first: this pass also computes the constant sum p ln p
static void ts_gradient_pass(hipStream_t st, const float* codes, int64_t N, int L, const float* beta, const float* logz,
                             const float* y, float alpha, bool first, float* grad, float* kl_out, float* stats_out,
                             void* workspace) {
  const TsLayout l = ts_layout(N, 1);
  char* const w = static_cast<char*>(workspace);
  double* const part = reinterpret_cast<double*>(w + l.part);
  double* const pt = reinterpret_cast<double*>(w + l.pt);
  double* const stats = reinterpret_cast<double*>(w + l.stats);
  const TsSplit sp = ts_split(N, ts_slices(N));
  const dim3 grid((unsigned)((N + kTsBlock - 1) / kTsBlock), (unsigned)sp.used);
  if (first)
    hipLaunchKernelGGL(tsne_pairs<true>, grid, dim3(kTsBlock), 0, st, codes, (int)N, L, beta, logz, y, sp.per_slice, part);
  else
    hipLaunchKernelGGL(tsne_pairs<false>, grid, dim3(kTsBlock), 0, st, codes, (int)N, L, beta, logz, y, sp.per_slice, part);
  const uint64_t E = (uint64_t)N * kTsAcc;
  hipLaunchKernelGGL(tsne_fold, dim3((unsigned)((E + kTsBlock - 1) / kTsBlock)), dim3(kTsBlock), 0, st, pt, part,
                     (unsigned long long)E, sp.used);
  hipLaunchKernelGGL(tsne_reduce, dim3(1), dim3(kTsBlock), 0, st, pt, (int)N, first ? 1 : 0, stats, kl_out, stats_out);
  hipLaunchKernelGGL(tsne_grad, dim3((unsigned)((2 * N + kTsBlock - 1) / kTsBlock)), dim3(kTsBlock), 0, st, pt, stats, (int)N, alpha,
                     grad);
}

}  // namespace

extern "C" {

int gmvae_tsne_workspace_bytes(int64_t N, int L, int64_t rows, uint64_t* bytes) {
  if (int e = ts_check_sizes(N, L)) return e;
  if (rows < 1 || rows > N) return GMVAE_E_DIMS;
  if (!bytes) return GMVAE_E_NULL;
  *bytes = ts_layout(N, rows).bytes;
  return 0;
}

int gmvae_tsne_affinities(const float* codes, int64_t N, int L, float perplexity, int64_t r0, int64_t rows, float* beta,
                          float* logz, float* entropy, void* workspace, void* stream) {
  if (int e = ts_check_sizes(N, L)) return e;
  if (!(perplexity > 1.f && perplexity < (float)(N - 1)) || rows < 1 || r0 < 0 || r0 > N - rows) return GMVAE_E_DIMS;
  if (!codes || !beta || !logz || !entropy || !workspace) return GMVAE_E_NULL;
  if (!aligned_to(codes, 4) || !aligned_to(beta, 4) || !aligned_to(logz, 4) || !aligned_to(entropy, 4) || !aligned16(workspace))
    return GMVAE_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* const d2 = reinterpret_cast<float*>(static_cast<char*>(workspace) + ts_layout(N, rows).d2);
  const TsSplit sp = ts_split(N, ts_slices(rows));
  (void)hipGetLastError();
  hipLaunchKernelGGL(tsne_dist, dim3((unsigned)((rows + kTsBlock - 1) / kTsBlock), (unsigned)sp.used), dim3(kTsBlock), 0, st, codes,
                     (int)N, L, (int)r0, (int)rows, sp.per_slice, d2);
  constexpr int per_block = kTsBlock / kTsWave;
  hipLaunchKernelGGL(tsne_search, dim3((unsigned)((rows + per_block - 1) / per_block)), dim3(kTsBlock), 0, st, d2, (int)N, (int)r0,
                     (int)rows, log((double)perplexity), beta, logz, entropy);
  return (int)hipGetLastError();
}

int gmvae_tsne_gradient(const float* codes, int64_t N, int L, const float* beta, const float* logz, const float* y,
                        float exaggeration, float* grad_out, float* stats_out, void* workspace, void* stream) {
  if (int e = ts_check_sizes(N, L)) return e;
  if (!codes || !beta || !logz || !y || !grad_out || !workspace) return GMVAE_E_NULL;
  if (!aligned_to(codes, 4) || !aligned_to(beta, 4) || !aligned_to(logz, 4) || !aligned_to(y, 4) || !aligned_to(grad_out, 4) ||
      !aligned_to(stats_out, 4) || !aligned16(workspace))
    return GMVAE_E_ALIGN;
  (void)hipGetLastError();
  ts_gradient_pass(static_cast<hipStream_t>(stream), codes, N, L, beta, logz, y, exaggeration, true, grad_out, nullptr, stats_out,
                   workspace);
  return (int)hipGetLastError();
}

int gmvae_tsne_run(const float* codes, int64_t N, int L, const float* beta, const float* logz, float* y, float* vel,
                   float* gains, int n_iter, int exaggeration_iters, float exaggeration, float lr, float* kl_history,
                   void* workspace, void* stream) {
  if (int e = ts_check_sizes(N, L)) return e;
  if (n_iter < 0) return GMVAE_E_DIMS;
  if (!codes || !beta || !logz || !y || !vel || !gains || !workspace) return GMVAE_E_NULL;
  if (!aligned_to(codes, 4) || !aligned_to(beta, 4) || !aligned_to(logz, 4) || !aligned_to(y, 4) || !aligned_to(vel, 4) ||
      !aligned_to(gains, 4) || !aligned_to(kl_history, 4) || !aligned16(workspace))
    return GMVAE_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* const grad = reinterpret_cast<float*>(static_cast<char*>(workspace) + ts_layout(N, 1).grad);
  (void)hipGetLastError();
  for (int it = 0; it < n_iter; ++it) {
    const bool early = it < exaggeration_iters;
    ts_gradient_pass(st, codes, N, L, beta, logz, y, early ? exaggeration : 1.f, it == 0, grad, kl_history ? kl_history + it : nullptr,
                     nullptr, workspace);
    hipLaunchKernelGGL(tsne_update, dim3((unsigned)((2 * N + kTsBlock - 1) / kTsBlock)), dim3(kTsBlock), 0, st, y, vel, gains, grad,
                       (int)(2 * N), early ? 0.5f : 0.8f, lr);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
