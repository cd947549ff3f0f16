// What the model-independent fits share across translation units (csrc/mixfit.hpp and csrc/mixfit_full.hpp in mixfit.hip,
// csrc/linprobe.hpp in linprobe.hip): constants, the plan's tail, MF_ADVANCE, the wave sum, the fixed-order fold and the
// factorisation in LDS.  Device functions and inline host functions only -- a kernel defined here would be defined once per
// translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace gmvae {

constexpr int kMfBlock = 256;             // threads of a workgroup
constexpr int kMfMaxTile = 128;           // rows per tile at most (one thread per row in the row step)
constexpr int kMfMaxGroups = 256;         // workgroups of a pass at most: one per CU
constexpr int kMfLdsBytes = 160 * 1024;   // the LDS of a CU
constexpr int kMfMaxKL = 16384;           // the K L gate: the parameter image is then 128 KiB
constexpr int kMfFoldSlots = 16;          // mixfit_update: slots per block
constexpr int kMfFoldParts = 16;          // ... and threads per slot
constexpr double kMfEps0 = 10.0 * 2.220446049250313e-16;      // scikit-learn's 10 * finfo(float64).eps

// the pass's shape for (N, L, K): rows per tile, rows per workgroup (whole tiles), workgroups, LDS bytes, doubles per workgroup's partials
struct MfPlan {
  int tile, per_group, groups, stride;
  size_t lds;
};
// the tail of a plan: N rows in tiles of T -> whole tiles per workgroup -> workgroups, gmax of them at most
static inline void mf_plan_groups(MfPlan& p, int64_t N, int64_t T, int64_t gmax) {
  const int64_t tiles = (N + T - 1) / T, g = tiles < gmax ? tiles : gmax;
  const int64_t per = (tiles + g - 1) / g * T;
  p.tile = (int)T;
  p.per_group = (int)per;
  p.groups = (int)((N + per - 1) / per);
}

__device__ __forceinline__ double mf_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);      // (a + b == b + a: every lane ends with the same bits)
  return v;
}

// (q, r) of item i by `den` -> those of item i + kMfBlock
#define MF_ADVANCE(q, r, step_q, step_r, den) \
  do {                                        \
    q += step_q;                              \
    r += step_r;                              \
    if (r >= den) {                           \
      r -= den;                               \
      q += 1;                                 \
    }                                         \
  } while (0)

// this thread's run of the G workgroups' values at offset `off`, added in order
__device__ __forceinline__ double mf_fold_run(const double* __restrict__ part, const int G, const int stride, const size_t off,
                                              const int p) {
  const int run = (G + kMfFoldParts - 1) / kMfFoldParts, g0 = p * run, g1 = g0 + run < G ? g0 + run : G;
  double a = 0.0;
  for (int g = g0; g < g1; ++g) a += part[(size_t)g * stride + off];
  return a;
}

typedef double mff_d4 __attribute__((ext_vector_type(4)));

__host__ __device__ static inline int mff_tri(int i) { return i * (i + 1) / 2; }

// The factorisation in LDS, by a workgroup of kMfBlock threads, called between two barriers: a [P] holds the lower triangle of a
// symmetric matrix packed by rows and x [P] the identity; a ends as its Cholesky factor C and x as C^-1.  Returns 0, or j + 1 for
// the first pivot j that is not > 0 (a and x are then left as that step found them); sum_ln = sum_d ln C_dd.  Shared with
// csrc/linprobe.hpp (linprobe_setup: the metric's inverse).
__device__ __forceinline__ int mff_factor_lds(double* const a, double* const x, const int L, const int tid, double& sum_ln) {
  const int ti = tid >> 4, tj = tid & 15;
  int info = 0;
  double sl = 0.0;
  for (int t = 0; t < L; ++t) {
    const double p = a[mff_tri(t) + t];      // (nobody writes a_tt in step t: every thread takes the same branch)
    if (!(p > 0.0)) {
      info = t + 1;
      break;
    }
    const double c = sqrt(p);
    sl += log(c);
    if (tid < L - t - 1) {
      a[mff_tri(t + 1 + tid) + t] /= c;
    } else if (tid < L) {
      x[mff_tri(t) + tid - (L - t - 1)] /= c;
    }
    __syncthreads();
    for (int i = t + 1 + ti; i < L; i += 16) {
      double* const ai = a + mff_tri(i);
      double* const xi = x + mff_tri(i);
      const double cit = ai[t];
      for (int j = t + 1 + tj; j <= i; j += 16) ai[j] = fma(-cit, a[mff_tri(j) + t], ai[j]);
      for (int j = tj; j <= t; j += 16) xi[j] = fma(-cit, x[mff_tri(t) + j], xi[j]);
    }
    __syncthreads();
  }
  sum_ln = sl;
  return info;
}

}  // namespace gmvae
