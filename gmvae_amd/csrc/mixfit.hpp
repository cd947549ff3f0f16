// gmvae_mixfit_* (include/gmvae_hip.h; host side: csrc/mixfit.hip): a K-component diagonal Gaussian mixture fitted to N codes
// z [N][L] by EM, and the responsibilities of a given mixture.  Model independent.  The statement is tests/mixfit_ref.py:
//   l_nk = logw_k - 1/2 sum_d ((z_nd - mu_kd) / sigma_kd)^2 - sum_d ln sigma_kd - (L/2) ln 2 pi      (the difference form)
//   lse_n = logsumexp_k l_nk (max-subtracted), log r_nk = l_nk - lse_n, r_nk = exp(log r_nk)
//   R_k = sum_n r_nk, S1_kd = sum_n r_nk (z_nd - mu_kd), S2_kd = sum_n r_nk (z_nd - mu_kd)^2          (centred at the CURRENT mean)
//   R'_k = R_k + 10 * 2^-52, m = S1 / R', mu' = mu + m, sigma' = sqrt(max(S2 / R' - m^2, 0) + reg_covar), logw'_k = ln(R'_k / sum_j R'_j)
// Two launches per iteration.
// Arithmetic: fp64 on the vector units wherever a difference of large numbers decides the result, as csrc/tsne.hpp does for d2.
// log r_nk = l_nk - lse_n is such a difference: with sigma = 1e-3 and codes of unit scale l_nk is about -1e7, and the fp32 statement
// (mixfit_ref with dtype=float32) then misses log r by 1 and R_k by 3 points at N = 259, K = 65, and misses the 1e-4 gate on log r
// at sigma in [0.05, 3] too (1.3e-4 at N = 1031, L = 64, K = 10; profiles/mixfit_notes.md).  So z - mu, 1 / sigma, the sum over d
// and l are fp64 (v_add_f64, v_mul_f64 and v_fma_f64 issue at the rate of their unpacked fp32 forms here); the exponentials are
// fp32 (their arguments are <= 0 and are rounded to fp32 after the subtraction).
// mixfit_pass: a workgroup of kMfBlock threads owns a contiguous slice of `per_group` rows and walks it in tiles of T rows (T <=
// kMfMaxTile, chosen on the host so that everything below fits the LDS, mf_plan).  LDS, all dynamic: the parameter image -- mu and
// sigma as fp32 [K][L | 1] (the odd row stride keeps 32 consecutive rows on 32 banks) and the constant c_k = logw_k - sum_d ln
// sigma_kd - (L/2) ln 2 pi [K] (fp64) -- resident for the workgroup's life (128 KiB of fp32 at the K L = 16,384 gate; 1 / sigma in
// fp64 would not fit, so it is rebuilt where it is used: v_rcp_f32 and two Newton steps in fp64, shared by four rows); per tile
// the staged codes [T][L | 1] (fp32), l_nk and then r_nk [T][K | 1] (fp64), and per row the max, ln of the sum, and lse.  Per tile:
//   stage:  the tile's T L floats are contiguous in memory: one coalesced sweep;
//   l_nk:   an item per thread is four rows of one component: t = (z - mu) (1 / sigma), q += t t in fp64; l = c_k - q / 2;
//   rows:   a thread per row: the max over k, the sum of exp(l - max) in fp64, lse = max + ln sum (written to lse_out);
//   sweep:  log r = (l - max) - ln sum, written coalesced to log_resp_out, r = exp(log r) left in LDS;
//   sums:   a thread owns the slots (k, d) = tid, tid + kMfBlock, ... and, behind them, the K slots of R_k: over the tile's rows
//           S1 += r (z - mu), S2 += (r (z - mu)) (z - mu), the difference and the products in fp64.  r (z - mu) is then exact and
//           the sums carry 1e-16, not 6e-8: a component held by ONE point off its mean has S2 / R' - m^2 = 0 against reg_covar =
//           1e-6, and fp32 products leave 6e-8 (z - mu)^2 there -- a 10 % error of sigma' at |z - mu| = 2.
//           The tile's sums are added to the workgroup's partials in the workspace by their owner: a plain load, add, store (the
//           first tile stores only, so the workspace needs no initialisation); nothing is shared between threads, no atomics.
// With kAccum = false the same pass stops behind the sweep: gmvae_mixfit_assign.
// mixfit_update: folds the G workgroups' partials in a fixed order in fp64 -- 16 slots a block, 16 threads a slot, each adding a
// contiguous run of workgroups in order, the 16 runs added in order by the slot's first thread -- applies the M-step to its slot
// and writes mu and sigma in place; one more block folds R_k for every k and sum lse, and writes logw, counts_out and the history
// entry.  One owner per sum, fixed-order folds, no float atomics: two runs give the same bits.
// Shared with the full-covariance fit (csrc/mixfit_full.hpp): the plan's tail (mf_plan_groups), MF_ADVANCE, mf_wave_sum, the fold
// (mf_fold_run) -- these in csrc/mixfit_common.hpp, where csrc/linprobe.hpp, another translation unit that may not see this file's
// kernels defined a second time, shares them too -- and the update's last block (mf_update_weights, which takes the offset of R_k in a workgroup's partials as an
// int), with kMfBlock, kMfMaxGroups, kMfLdsBytes and the fold's shape.  The E-step's tail -- stage, rows, the tile's sum of lse,
// sweep -- is NOT shared: as forceinline helpers it compiled to the same instructions in another schedule, and one pass or the
// other then ran 1 to 5 % slower on the MI355X (profiles/mixfit_notes.md), so mixfit_pass and mixfit_full_pass each keep their
// own text of those four steps, and a change to one of them is to be made in both.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mixfit_common.hpp"

namespace gmvae {

static inline size_t mf_lds_bytes(int L, int K, int T) {
  const size_t Lp = (size_t)(L | 1), Kp = (size_t)(K | 1);
  return 8 * (3 * (size_t)T + (size_t)T * Kp + (size_t)K) + 4 * (2 * (size_t)K * Lp + (size_t)T * Lp);
}
static inline MfPlan mf_plan(int64_t N, int L, int K) {
  MfPlan p;
  const size_t image = mf_lds_bytes(L, K, 0), row = mf_lds_bytes(L, K, 1) - image;
  int64_t T = (int64_t)(((size_t)kMfLdsBytes - image) / row);      // >= 1 inside the gate: image <= 135,168 and row <= 16,452 bytes
  T = T > kMfMaxTile ? kMfMaxTile : T;
  T = T > N ? N : T;
  mf_plan_groups(p, N, T, kMfMaxGroups);
  p.stride = (2 * L + 1) * K + 1;      // S1 [K][L], S2 [K][L], R [K], sum lse
  p.lds = mf_lds_bytes(L, K, (int)T);
  return p;
}

template <bool kAccum>
__global__ __launch_bounds__(kMfBlock) void mixfit_pass(const float* __restrict__ codes, const int N, const int L, const int K,
                                                        const float* __restrict__ logw, const float* __restrict__ mu,
                                                        const float* __restrict__ sigma, const int T, const int per_group,
                                                        float* __restrict__ log_resp_out, float* __restrict__ lse_out,
                                                        double* __restrict__ part, const int stride) {
  extern __shared__ __attribute__((aligned(16))) char mf_smem[];
  const int tid = threadIdx.x, Lp = L | 1, Kp = K | 1, KL = K * L;
  double* const s_lse = reinterpret_cast<double*>(mf_smem);      // [T]
  double* const s_m = s_lse + T;                                 // [T]
  double* const s_ls = s_m + T;                                  // [T]
  double* const s_l = s_ls + T;                                  // [T][Kp]: l, then r
  double* const s_c = s_l + T * Kp;                              // [K]
  float* const s_mu = reinterpret_cast<float*>(s_c + K);         // [K][Lp]
  float* const s_sg = s_mu + K * Lp;                             // [K][Lp]
  float* const s_z = s_sg + K * Lp;                              // [T][Lp]

  // item tid + j kMfBlock as (quotient, remainder) by L and by K, advanced without a division
  const int nL0 = tid / L, dL0 = tid - nL0 * L, stepL_n = kMfBlock / L, stepL_d = kMfBlock - stepL_n * L;
  const int nK0 = tid / K, kK0 = tid - nK0 * K, stepK_n = kMfBlock / K, stepK_d = kMfBlock - stepK_n * K;
  // the parameter image
  for (int s = tid, k = nL0, d = dL0; s < KL; s += kMfBlock) {
    s_mu[k * Lp + d] = mu[s];
    s_sg[k * Lp + d] = sigma[s];
    MF_ADVANCE(k, d, stepL_n, stepL_d, L);
  }
  for (int k = tid >> 6; k < K; k += kMfBlock >> 6) {      // a wave per component: sum_d ln sigma_kd, lanes over d, a fixed tree
    double a = 0.0;
    for (int d = tid & 63; d < L; d += 64) a += log((double)sigma[(size_t)k * L + d]);
    a = mf_wave_sum(a);
    if ((tid & 63) == 0) s_c[k] = (double)logw[k] - a - 0.91893853320467274178 * (double)L;
  }

  const int64_t g_lo = (int64_t)blockIdx.x * per_group, g_hi = g_lo + per_group < N ? g_lo + per_group : N;
  double* const gpart = kAccum ? part + (size_t)blockIdx.x * stride : nullptr;
  double lse_acc = 0.0;      // (thread 0's)
  for (int64_t r0 = g_lo; r0 < g_hi; r0 += T) {
    const int rows = (int)(g_hi - r0 < T ? g_hi - r0 : T);
    __syncthreads();      // the image is in place; the previous tile's sums have read s_z and s_l
    {
      const float* __restrict__ src = codes + (size_t)r0 * L;
      int n = nL0, d = dL0;
      for (int i = tid; i < rows * L; i += kMfBlock) {
        s_z[n * Lp + d] = src[i];
        MF_ADVANCE(n, d, stepL_n, stepL_d, L);
      }
    }
    __syncthreads();
    {
      const int quads = (rows + 3) >> 2;      // item g K + k: the rows 4 g .. 4 g + 3 (a row past the end repeats the last one) of component k
      for (int i = tid, g = nK0, k = kK0; i < quads * K; i += kMfBlock) {
        const int last = rows - 1, n0 = 4 * g;
        const float* __restrict__ z0 = s_z + (n0 < last ? n0 : last) * Lp;
        const float* __restrict__ z1 = s_z + (n0 + 1 < last ? n0 + 1 : last) * Lp;
        const float* __restrict__ z2 = s_z + (n0 + 2 < last ? n0 + 2 : last) * Lp;
        const float* __restrict__ z3 = s_z + (n0 + 3 < last ? n0 + 3 : last) * Lp;
        const float* __restrict__ mr = s_mu + k * Lp;
        const float* __restrict__ sr = s_sg + k * Lp;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
        for (int d = 0; d < L; ++d) {
          const float sf = sr[d];
          const double sg = (double)sf, m = (double)mr[d];
          double y = (double)__builtin_amdgcn_rcpf(sf);      // 1 / sigma: 1 ulp of fp32, then two Newton steps in fp64
          y = fma(y, fma(-sg, y, 1.0), y);
          y = fma(y, fma(-sg, y, 1.0), y);
          const double t0 = ((double)z0[d] - m) * y, t1 = ((double)z1[d] - m) * y;
          const double t2 = ((double)z2[d] - m) * y, t3 = ((double)z3[d] - m) * y;
          q0 = fma(t0, t0, q0);
          q1 = fma(t1, t1, q1);
          q2 = fma(t2, t2, q2);
          q3 = fma(t3, t3, q3);
        }
        const double c = s_c[k];
        double* __restrict__ o = s_l + n0 * Kp + k;
        o[0] = fma(-0.5, q0, c);
        if (n0 + 1 < rows) o[Kp] = fma(-0.5, q1, c);
        if (n0 + 2 < rows) o[2 * Kp] = fma(-0.5, q2, c);
        if (n0 + 3 < rows) o[3 * Kp] = fma(-0.5, q3, c);
        MF_ADVANCE(g, k, stepK_n, stepK_d, K);
      }
    }
    __syncthreads();
    if (tid < rows) {
      const double* __restrict__ lr = s_l + tid * Kp;
      double m = -INFINITY;
      for (int k = 0; k < K; ++k) m = fmax(m, lr[k]);
      if (m == -INFINITY) m = 0.0;      // (every component at -inf: lse = -inf, nothing to subtract)
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += (double)expf((float)(lr[k] - m));
      const double ls = log(s), lse = m + ls;
      s_m[tid] = m;
      s_ls[tid] = ls;
      s_lse[tid] = lse;
      if (lse_out) lse_out[r0 + tid] = (float)lse;
    }
    __syncthreads();
    if (kAccum && tid < 64) {      // the tile's sum of lse: lanes over the rows, a fixed tree
      double a = 0.0;
      for (int n = tid; n < rows; n += 64) a += s_lse[n];
      lse_acc += mf_wave_sum(a);
    }
    for (int i = tid, n = nK0, k = kK0; i < rows * K; i += kMfBlock) {
      const float lr = (float)((s_l[n * Kp + k] - s_m[n]) - s_ls[n]);
      if (log_resp_out) log_resp_out[(size_t)r0 * K + i] = lr;
      if (kAccum) s_l[n * Kp + k] = (double)expf(lr);
      MF_ADVANCE(n, k, stepK_n, stepK_d, K);
    }
    if (kAccum) {
      __syncthreads();
      const bool first = r0 == g_lo;
      for (int s = tid, k = nL0, d = dL0; s < KL + K; s += kMfBlock) {
        if (s < KL) {
          const double m = (double)s_mu[k * Lp + d];
          double a1 = 0.0, a2 = 0.0;
          for (int n = 0; n < rows; ++n) {
            const double dz = (double)s_z[n * Lp + d] - m, t = s_l[n * Kp + k] * dz;
            a1 += t;
            a2 = fma(t, dz, a2);
          }
          if (!first) {
            a1 += gpart[s];
            a2 += gpart[KL + s];
          }
          gpart[s] = a1;
          gpart[KL + s] = a2;
          MF_ADVANCE(k, d, stepL_n, stepL_d, L);
        } else {
          const int kr = s - KL;
          double a = 0.0;
          for (int n = 0; n < rows; ++n) a += s_l[n * Kp + kr];
          if (!first) a += gpart[2 * KL + kr];
          gpart[2 * KL + kr] = a;
        }
      }
    }
  }
  if (kAccum && tid == 0) gpart[2 * KL + K] = lse_acc;
}

// the update's last block: folds R_k for every k (offset offR + k of a workgroup's partials) and sum lse (offR + K), and writes
// logw, counts_out and the history entry.  s_p: the kernel's fold planes, of which [0] and [1][0] serve here
__device__ __forceinline__ void mf_update_weights(const double* __restrict__ part, const int G, const int stride, const int offR,
                                                  const int N, const int K, float* __restrict__ logw, float* __restrict__ hist_out,
                                                  float* __restrict__ counts_out, double (*s_p)[kMfFoldSlots][kMfFoldParts + 1]) {
  __shared__ double s_R[256];
  __shared__ double s_tot;
  const int tid = threadIdx.x, q = tid / kMfFoldParts, p = tid % kMfFoldParts;
  for (int k0 = 0; k0 < K; k0 += kMfFoldSlots) {
    const int k = k0 + q;
    if (k < K) s_p[0][q][p] = mf_fold_run(part, G, stride, (size_t)(offR + k), p);
    __syncthreads();
    if (k < K && p == 0) {
      double R = 0.0;
      for (int j = 0; j < kMfFoldParts; ++j) R += s_p[0][q][j];
      s_R[k] = R;
    }
    __syncthreads();
  }
  if (q == 0) s_p[1][0][p] = mf_fold_run(part, G, stride, (size_t)(offR + K), p);
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0, lse = 0.0;
    for (int k = 0; k < K; ++k) tot += s_R[k] + kMfEps0;
    for (int j = 0; j < kMfFoldParts; ++j) lse += s_p[1][0][j];
    s_tot = tot;
    if (hist_out) *hist_out = (float)(lse / (double)N);
  }
  __syncthreads();
  if (tid < K) {
    logw[tid] = (float)log((s_R[tid] + kMfEps0) / s_tot);
    if (counts_out) counts_out[tid] = (float)s_R[tid];
  }
}

// blocks [0, slot_blocks): the M-step of kMfFoldSlots slots (k, d) each; the last block: logw, counts_out, the history entry
__global__ __launch_bounds__(kMfBlock) void mixfit_update(const double* __restrict__ part, const int G, const int stride, const int N,
                                                          const int L, const int K, const float reg_covar, float* __restrict__ logw,
                                                          float* __restrict__ mu, float* __restrict__ sigma,
                                                          float* __restrict__ hist_out, float* __restrict__ counts_out) {
  __shared__ double s_p[3][kMfFoldSlots][kMfFoldParts + 1];
  const int tid = threadIdx.x, q = tid / kMfFoldParts, p = tid % kMfFoldParts, KL = K * L;
  const int slot_blocks = (KL + kMfFoldSlots - 1) / kMfFoldSlots;
  if ((int)blockIdx.x < slot_blocks) {
    const int s = (int)blockIdx.x * kMfFoldSlots + q;
    const bool live = s < KL;
    const int k = live ? s / L : 0;
    if (live) {
      s_p[0][q][p] = mf_fold_run(part, G, stride, (size_t)s, p);
      s_p[1][q][p] = mf_fold_run(part, G, stride, (size_t)KL + s, p);
      s_p[2][q][p] = mf_fold_run(part, G, stride, (size_t)2 * KL + k, p);
    }
    __syncthreads();
    if (live && p == 0) {
      double S1 = 0.0, S2 = 0.0, R = 0.0;
      for (int j = 0; j < kMfFoldParts; ++j) {
        S1 += s_p[0][q][j];
        S2 += s_p[1][q][j];
        R += s_p[2][q][j];
      }
      // (the statement's operations in the statement's order, each rounded: where one far point holds a component, S2 / R' and
      // m^2 agree to 15 digits and a contracted fma would answer differently from the statement in the digits that are left)
      const double Rp = R + kMfEps0, m = S1 / Rp, var = __dsub_rn(S2 / Rp, __dmul_rn(m, m));
      mu[s] = (float)((double)mu[s] + m);
      sigma[s] = (float)sqrt((var > 0.0 ? var : 0.0) + (double)reg_covar);
    }
    return;
  }
  mf_update_weights(part, G, stride, 2 * KL, N, K, logw, hist_out, counts_out, s_p);
}

}  // namespace gmvae
