// gmvae_mmd: the host side of csrc/twosample.hpp (include/gmvae_hip.h).  A translation unit of its own, for the reason at the top
// of csrc/tsne.hip: the model-independent evaluator's kernels, descriptors and symbols stay out of the training step's code object.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gmvae_hip.h"
#include "hostutil.hpp"
#include "twosample.hpp"

using namespace gmvae;

namespace {

int ts_check_sizes(int N, int D, int P) {
  return (N < 2 || N > (1 << 20) || D < 1 || D > 4096 || P < 1 || P > 4096) ? GMVAE_E_DIMS : 0;
}

template <int NT, bool kEnergy>
void ts_launch_tiles(const TsPlan& p, const TsLayout& lay, const float* z, int N, int D, const uint8_t* assign, int P, const TsGamma& gam,
                     int Q, double* ws, hipStream_t st) {
  static bool seen[64];
  allow_lds(seen, {reinterpret_cast<const void*>(mmd_tiles<NT, kEnergy>)}, (int)ts_plan(N, 128 * NT).lds);
  const int words_ok = (N & 3) == 0 && aligned_to(assign, 4);
  hipLaunchKernelGGL((mmd_tiles<NT, kEnergy>), dim3((unsigned)p.row_tiles, (unsigned)p.slabs, (unsigned)p.p_chunks), dim3(kTsBlock), p.lds, st,
                     z, N, D, assign, P, gam, Q, p.tiles_per_slab, p.col_tiles, words_ok, (const double*)(ws + lay.mean),
                     (const double*)(ws + lay.nrm), ws + lay.a, ws + lay.b, ws + lay.c, ws + lay.row_all, ws + lay.row_first);
}

template <int NT>
void ts_launch(const TsPlan& p, const TsLayout& lay, const float* z, int N, int D, const uint8_t* assign, int P, int kind,
               const TsGamma& gam, int Q, double* ws, hipStream_t st) {
  if (kind == kTsKindEnergy) {
    ts_launch_tiles<NT, true>(p, lay, z, N, D, assign, P, gam, Q, ws, st);
    return;
  }
  // rbf: the pooled mean and the centred rows' squared norms in front
  hipLaunchKernelGGL(mmd_mean_part, dim3((unsigned)((D + 63) / 64), (unsigned)p.mean_slices), dim3(kTsSmallBlock), 0, st, z, N, D,
                     p.rows_per_slice, ws + lay.mean_part);
  hipLaunchKernelGGL(mmd_mean_fold, dim3((unsigned)((D + kTsSmallBlock - 1) / kTsSmallBlock)), dim3(kTsSmallBlock), 0, st,
                     (const double*)(ws + lay.mean_part), p.mean_slices, N, D, ws + lay.mean);
  hipLaunchKernelGGL(mmd_norms, dim3((unsigned)((N + 3) / 4)), dim3(kTsSmallBlock), 0, st, z, N, D, (const double*)(ws + lay.mean),
                     ws + lay.nrm);
  ts_launch_tiles<NT, false>(p, lay, z, N, D, assign, P, gam, Q, ws, st);
}

}  // namespace

extern "C" {

int gmvae_mmd_workspace_bytes(int N, int D, int P, uint64_t* bytes) {
  if (int e = ts_check_sizes(N, D, P)) return e;
  if (!bytes) return GMVAE_E_NULL;
  const TsPlan p = ts_plan(N, P);
  *bytes = (ts_layout(p, N, D, P).end * sizeof(double) + 15) / 16 * 16;
  return 0;
}

int gmvae_mmd(const float* z, int N, int D, const uint8_t* assign, int P, int kernel, const double* gamma, int Q, double* mmd2,
              double* row_all, double* row_first, void* workspace, void* stream) {
  if (int e = ts_check_sizes(N, D, P)) return e;
  if (kernel != GMVAE_MMD_RBF && kernel != GMVAE_MMD_ENERGY) return GMVAE_E_MODEL;
  TsGamma gam = {};
  if (kernel == GMVAE_MMD_RBF) {
    if (Q < 1 || Q > kTsMaxQ) return GMVAE_E_DIMS;
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
  const TsPlan p = ts_plan(N, P);
  const TsLayout lay = ts_layout(p, N, D, P);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* const ws = static_cast<double*>(workspace);
  (void)hipGetLastError();
  switch (p.nt) {
    case 1: ts_launch<1>(p, lay, z, N, D, assign, P, kernel, gam, Q, ws, st); break;
    case 2: ts_launch<2>(p, lay, z, N, D, assign, P, kernel, gam, Q, ws, st); break;
    case 4: ts_launch<4>(p, lay, z, N, D, assign, P, kernel, gam, Q, ws, st); break;
    default: ts_launch<8>(p, lay, z, N, D, assign, P, kernel, gam, Q, ws, st); break;
  }
  hipLaunchKernelGGL(mmd_finish, dim3((unsigned)(P + (N + kTsSmallBlock - 1) / kTsSmallBlock)), dim3(kTsSmallBlock), 0, st, assign, N, P, (int)p.groups,
                     p.slabs, (const double*)(ws + lay.a), (const double*)(ws + lay.b), (const double*)(ws + lay.c),
                     (const double*)(ws + lay.row_all), (const double*)(ws + lay.row_first), mmd2, row_all, row_first);
  return (int)hipGetLastError();
}

}  // extern "C"
