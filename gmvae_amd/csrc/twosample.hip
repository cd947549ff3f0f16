// gmvae_mmd and gmvae_sinkhorn: the host sides of csrc/twosample.hpp and csrc/sinkhorn.hpp (include/gmvae_hip.h).  One translation
// unit for both, so that csrc/cgram.hpp's kernels, which both launch, are defined once (csrc/ais.hip's reason); a unit apart from
// the others for the reason at the top of csrc/tsne.hip: the model-independent evaluators' kernels, descriptors and symbols stay out
// of the training step's code object.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gmvae_hip.h"
#include "hostutil.hpp"
#include "sinkhorn.hpp"
#include "twosample.hpp"

using namespace gmvae;

namespace {

// the three launches in front of a centred Gram tile kernel (csrc/cgram.hpp): the pooled mean of src's N rows, then the centred
// rows' squared norms
template <class Src>
void cg_setup(const Src& src, int N, int D, const CgSlices& sl, double* mean_part, double* mean, double* nrm, hipStream_t st) {
  hipLaunchKernelGGL(cg_mean_part<Src>, dim3((unsigned)((D + 63) / 64), (unsigned)sl.slices), dim3(kCgSmallBlock), 0, st, src, N, D, sl.rows,
                     mean_part);
  hipLaunchKernelGGL(cg_mean_fold, dim3((unsigned)((D + kCgSmallBlock - 1) / kCgSmallBlock)), dim3(kCgSmallBlock), 0, st,
                     (const double*)mean_part, sl.slices, N, D, mean);
  hipLaunchKernelGGL(cg_norms<Src>, dim3((unsigned)((N + 3) / 4)), dim3(kCgSmallBlock), 0, st, src, N, D, (const double*)mean, nrm);
}

int mmd_check_sizes(int N, int D, int P) {
  return (N < 2 || N > (1 << 20) || D < 1 || D > 4096 || P < 1 || P > 4096) ? GMVAE_E_DIMS : 0;
}

template <int NT, bool kEnergy>
void mmd_launch_tiles(const MmdPlan& p, const MmdLayout& lay, const float* z, int N, int D, const uint8_t* assign, int P, const MmdGamma& gam,
                      int Q, double* ws, hipStream_t st) {
  static bool seen[64];
  allow_lds(seen, {reinterpret_cast<const void*>(mmd_tiles<NT, kEnergy>)}, (int)mmd_plan(N, 128 * NT).lds);
  const int words_ok = (N & 3) == 0 && aligned_to(assign, 4);
  hipLaunchKernelGGL((mmd_tiles<NT, kEnergy>), dim3((unsigned)p.row_tiles, (unsigned)p.slabs, (unsigned)p.p_chunks), dim3(kCgBlock), p.lds, st,
                     z, N, D, assign, P, gam, Q, p.tiles_per_slab, p.col_tiles, words_ok, (const double*)(ws + lay.mean),
                     (const double*)(ws + lay.nrm), ws + lay.a, ws + lay.b, ws + lay.c, ws + lay.row_all, ws + lay.row_first);
}

template <int NT>
void mmd_launch(const MmdPlan& p, const MmdLayout& lay, const float* z, int N, int D, const uint8_t* assign, int P, int kind,
                const MmdGamma& gam, int Q, double* ws, hipStream_t st) {
  if (kind == kMmdKindEnergy) {
    mmd_launch_tiles<NT, true>(p, lay, z, N, D, assign, P, gam, Q, ws, st);
    return;
  }
  cg_setup(CgRows{z}, N, D, p.mean, ws + lay.mean_part, ws + lay.mean, ws + lay.nrm, st);
  mmd_launch_tiles<NT, false>(p, lay, z, N, D, assign, P, gam, Q, ws, st);
}

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
  p.col_tiles = (col_cnt + kCgCols - 1) / kCgCols;
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

int gmvae_mmd_workspace_bytes(int N, int D, int P, uint64_t* bytes) {
  if (int e = mmd_check_sizes(N, D, P)) return e;
  if (!bytes) return GMVAE_E_NULL;
  const MmdPlan p = mmd_plan(N, P);
  *bytes = (mmd_layout(p, N, D, P).end * sizeof(double) + 15) / 16 * 16;
  return 0;
}

int gmvae_mmd(const float* z, int N, int D, const uint8_t* assign, int P, int kernel, const double* gamma, int Q, double* mmd2,
              double* row_all, double* row_first, void* workspace, void* stream) {
  if (int e = mmd_check_sizes(N, D, P)) return e;
  if (kernel != GMVAE_MMD_RBF && kernel != GMVAE_MMD_ENERGY) return GMVAE_E_MODEL;
  MmdGamma gam = {};
  if (kernel == GMVAE_MMD_RBF) {
    if (Q < 1 || Q > kMmdMaxQ) return GMVAE_E_DIMS;
    if (!gamma) return GMVAE_E_NULL;
    for (int q = 0; q < Q; ++q) {
      if (!(gamma[q] >= 0.0) || !isfinite(gamma[q])) return GMVAE_E_DIMS;
      gam.g[q] = gamma[q];
    }
  } else {
    Q = 0;
  }
  if (!z || !assign || !mmd2 || !workspace) return GMVAE_E_NULL;
  if (!aligned_to(z, 4) || !aligned_to(mmd2, 8) || !aligned_to(row_all, 8) || !aligned_to(row_first, 8) || !aligned_to(workspace, 16))
    return GMVAE_E_ALIGN;
  const MmdPlan p = mmd_plan(N, P);
  const MmdLayout lay = mmd_layout(p, N, D, P);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* const ws = static_cast<double*>(workspace);
  (void)hipGetLastError();
  switch (p.nt) {
    case 1: mmd_launch<1>(p, lay, z, N, D, assign, P, kernel, gam, Q, ws, st); break;
    case 2: mmd_launch<2>(p, lay, z, N, D, assign, P, kernel, gam, Q, ws, st); break;
    case 4: mmd_launch<4>(p, lay, z, N, D, assign, P, kernel, gam, Q, ws, st); break;
    default: mmd_launch<8>(p, lay, z, N, D, assign, P, kernel, gam, Q, ws, st); break;
  }
  hipLaunchKernelGGL(mmd_finish, dim3((unsigned)(P + (N + kMmdSmallBlock - 1) / kMmdSmallBlock)), dim3(kMmdSmallBlock), 0, st, assign, N, P, (int)p.groups,
                     p.slabs, (const double*)(ws + lay.a), (const double*)(ws + lay.b), (const double*)(ws + lay.c),
                     (const double*)(ws + lay.row_all), (const double*)(ws + lay.row_first), mmd2, row_all, row_first);
  return (int)hipGetLastError();
}

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
  cg_setup(CgPooled{x, n, y}, N, D, pl.mean, ws + lay.mean_part, ws + lay.mean, ws + lay.nrm, st);
  hipLaunchKernelGGL(sk_logw, dim3(2), dim3(kSkSmallBlock), 0, st, a, n, b, m, ws + lay.logw, ws + lay.wsum);
  if (hipError_t e = hipMemsetAsync(f, 0, sizeof(double) * n, st)) return (int)e;
  if (hipError_t e = hipMemsetAsync(g, 0, sizeof(double) * m, st)) return (int)e;
  if (hipError_t e = hipMemsetAsync(p, 0, sizeof(double) * n, st)) return (int)e;
  if (hipError_t e = hipMemsetAsync(q, 0, sizeof(double) * m, st)) return (int)e;

  // a half-step: its two or three softmins as the problems of one tile launch, then the fold
  auto half = [&](const SkProbs& pr, const double* eps) {
    hipLaunchKernelGGL(sk_tiles, dim3((unsigned)pl.row_tiles, (unsigned)pl.slabs, (unsigned)kSkProblems), dim3(kCgBlock), 0, st, x, n, y, D, pr,
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
