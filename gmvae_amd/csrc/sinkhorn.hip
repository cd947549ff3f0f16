// gmvae_sinkhorn: the host side of csrc/sinkhorn.hpp (include/gmvae_hip.h).  A translation unit of its own, for the reason at the top
// of csrc/tsne.hip: the model-independent evaluator's kernels, descriptors and symbols stay out of the training step's code object.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gmvae_hip.h"
#include "hostutil.hpp"
#include "sinkhorn.hpp"

using namespace gmvae;

namespace {

int sk_check_sizes(int64_t n, int64_t m, int D) {
  return (n < 1 || n > (1 << 20) || m < 1 || m > (1 << 20) || D < 1 || D > 4096) ? GMVAE_E_DIMS : 0;
}

// the softmin at the points `rows` summed over the points `cols` (each a range of the pooled rows: x is [0, n), y is [n, n + m))
SkProb sk_prob(int row_off, int row_cnt, int col_off, int col_cnt, int slabs, const double* h, const double* logw, double* dst, int avg,
               double* err) {
  SkProb p;
  p.row_off = row_off;
  p.row_cnt = row_cnt;
  p.col_off = col_off;
  p.col_cnt = col_cnt;
  p.col_tiles = (col_cnt + kSkCols - 1) / kSkCols;
  p.tiles_per_slab = (p.col_tiles + slabs - 1) / slabs;
  p.sym = row_off == col_off;
  p.avg = avg;
  p.h = h;
  p.logw = logw;
  p.dst = dst;
  p.err = err;
  return p;
}

}  // namespace

extern "C" {

int gmvae_sinkhorn_workspace_bytes(int64_t n, int64_t m, int D, uint64_t* bytes) {
  if (int e = sk_check_sizes(n, m, D)) return e;
  if (!bytes) return GMVAE_E_NULL;
  const SkPlan p = sk_plan((int)n, (int)m);
  *bytes = (sk_layout(p, (int)n, (int)m, D).end * sizeof(double) + 15) / 16 * 16;
  return 0;
}

int gmvae_sinkhorn(const float* x, int64_t n64, const float* y, int64_t m64, int D, const double* a, const double* b, const double* eps_dev,
                   int n_iter, double* f, double* g, double* p, double* q, double* out, void* workspace, void* stream) {
  if (int e = sk_check_sizes(n64, m64, D)) return e;
  if (n_iter < 1 || n_iter > 100000) return GMVAE_E_DIMS;
  if (!x || !y || !eps_dev || !f || !g || !p || !q || !out || !workspace) return GMVAE_E_NULL;
  if (!aligned_to(x, 4) || !aligned_to(y, 4) || !aligned_to(a, 8) || !aligned_to(b, 8) || !aligned_to(eps_dev, 8) || !aligned_to(f, 8) ||
      !aligned_to(g, 8) || !aligned_to(p, 8) || !aligned_to(q, 8) || !aligned_to(out, 8) || !aligned_to(workspace, 16))
    return GMVAE_E_ALIGN;
  const int n = (int)n64, m = (int)m64, N = n + m;
  const SkPlan pl = sk_plan(n, m);
  const SkLayout lay = sk_layout(pl, n, m, D);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* const ws = static_cast<double*>(workspace);
  double* const part_max = ws + lay.part_max;
  double* const part_sum = ws + lay.part_sum;
  const double* const loga = ws + lay.logw;
  const double* const logb = ws + lay.logw + n;
  (void)hipGetLastError();

  // set-up: the pooled mean, the centred squared norms, the normalised log-weights; the potentials start at 0
  hipLaunchKernelGGL(sk_mean_part, dim3((unsigned)((D + 63) / 64), (unsigned)pl.mean_slices), dim3(kSkSmallBlock), 0, st, x, n, y, m, D,
                     pl.rows_per_slice, ws + lay.mean_part);
  hipLaunchKernelGGL(sk_mean_fold, dim3((unsigned)((D + kSkSmallBlock - 1) / kSkSmallBlock)), dim3(kSkSmallBlock), 0, st,
                     (const double*)(ws + lay.mean_part), pl.mean_slices, N, D, ws + lay.mean);
  hipLaunchKernelGGL(sk_norms, dim3((unsigned)((N + 3) / 4)), dim3(kSkSmallBlock), 0, st, x, n, y, m, D, (const double*)(ws + lay.mean),
                     ws + lay.nrm);
  hipLaunchKernelGGL(sk_logw, dim3(2), dim3(kSkSmallBlock), 0, st, a, n, b, m, ws + lay.logw, ws + lay.wsum);
  if (hipError_t e = hipMemsetAsync(f, 0, sizeof(double) * n, st)) return (int)e;
  if (hipError_t e = hipMemsetAsync(g, 0, sizeof(double) * m, st)) return (int)e;
  if (hipError_t e = hipMemsetAsync(p, 0, sizeof(double) * n, st)) return (int)e;
  if (hipError_t e = hipMemsetAsync(q, 0, sizeof(double) * m, st)) return (int)e;

  // a half-step: its two or three softmins as the problems of one tile launch, then the fold
  auto half = [&](const SkProbs& pr, const double* eps) {
    hipLaunchKernelGGL(sk_tiles, dim3((unsigned)pl.row_tiles, (unsigned)pl.slabs, (unsigned)kSkProblems), dim3(kSkBlock), 0, st, x, n, y, D, pr,
                       pl.slabs, pl.R, eps, (const double*)(ws + lay.mean), (const double*)(ws + lay.nrm), part_max, part_sum);
    hipLaunchKernelGGL(sk_fold, dim3((unsigned)((pl.R + kSkSmallBlock - 1) / kSkSmallBlock), (unsigned)kSkProblems), dim3(kSkSmallBlock), 0, st,
                       pr, pl.slabs, pl.R, eps, (const double*)part_max, (const double*)part_sum);
  };
  SkProbs A, B, last;
  for (int avg = 1; avg >= 0; --avg) {
    SkProbs& h = avg ? A : last;
    h.p[0] = sk_prob(0, n, n, m, pl.slabs, g, logb, f, 0, avg ? nullptr : ws + lay.err);      // f <- softmin(y, g, b) at x
    h.p[1] = sk_prob(0, n, 0, n, pl.slabs, p, loga, p, avg, nullptr);                         // p: softmin(x, p, a) at x
    h.p[2] = sk_prob(n, m, n, m, pl.slabs, q, logb, q, avg, nullptr);                         // q: softmin(y, q, b) at y
  }
  B = A;
  B.p[0] = sk_prob(n, m, 0, n, pl.slabs, f, loga, g, 0, nullptr);                             // g <- softmin(x, f, a) at y
  for (int t = 0; t < n_iter; ++t) {
    half(A, eps_dev + t);
    half(B, eps_dev + t);
  }
  half(last, eps_dev + n_iter);
  hipLaunchKernelGGL(sk_finish, dim3(1), dim3(kSkSmallBlock), 0, st, a, n, b, m, (const double*)(ws + lay.wsum), (const double*)f,
                     (const double*)g, (const double*)p, (const double*)q, (const double*)(ws + lay.err), out);
  return (int)hipGetLastError();
}

}  // extern "C"
