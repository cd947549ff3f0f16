// gmvae_mixfit_full_* (include/gmvae_hip.h; host side: csrc/mixfit.hip): a K-component FULL-covariance Gaussian mixture fitted
// to N codes z [N][L] by EM, and the responsibilities of a given mixture.  Model independent.  The statement is
// tests/mixfit_full_ref.py:
//   factor: C_k = the lower Cholesky factor of the lower triangle of cov_k; a pivot that is not > 0 gives info_k = j + 1, and the
//           component is absent from that E-step (l_nk = -inf)
//   l_nk = logw_k - 1/2 |C_k^-1 (z_n - mu_k)|^2 - sum_d ln C_k,dd - (L/2) ln 2 pi
//   lse_n = logsumexp_k l_nk (max-subtracted), log r_nk = l_nk - lse_n, r_nk = exp(log r_nk)
//   R_k = sum_n r_nk, S1_kd = sum_n r_nk (z_nd - mu_kd), S2_kde = sum_n r_nk (z_nd - mu_kd) (z_ne - mu_ke)    (centred at the CURRENT mean)
//   R'_k = R_k + 10 * 2^-52, m = S1 / R', mu' = mu + m, cov'_kde = S2_kde / R' - m_d m_e, its diagonal max(., 0) + reg_covar,
//   logw'_k = ln(R'_k / sum_j R'_j)
// Three launches per iteration.  Arithmetic: fp64 wherever a difference of large numbers decides the result, for the reason at the
// top of csrc/mixfit.hpp (log r = l - lse; evaluated in fp32 this statement misses the 1e-4 gate on log r by 6.6 x at N = 1031,
// L = 64, K = 10); the exponentials are fp32, as there.
// mixfit_full_factor: a workgroup per component.  LDS, dynamic: the lower triangle of cov_k and of the identity, both packed by
// rows in fp64 ((i, j) at i (i + 1) / 2 + j; 2 x 66,048 bytes at L = 128).  Step t of L: the pivot p = a_tt (every thread reads
// it: a uniform decision); column t of a and row t of x divided by c = sqrt(p); then the two rank-1 updates a_ij -= C_it C_jt
// (t < j <= i) and x_ij -= C_it X_tj (j <= t < i) over a 16 x 16 thread grid.  Two barriers a step; a ends as C_k and x as
// W_k = C_k^-1.  W_k (packed) and sum_d ln C_dd go to the workspace; a failed component stores W_k = 0 and +inf.
// mixfit_full_pass: a workgroup of kMfBlock threads owns a contiguous slice of `per_group` rows and walks it in tiles of T rows
// (T a multiple of 4, <= kMffMaxTile, chosen on the host so that everything below fits the LDS, mff_plan).  K L^2 fp64 does not fit
// the LDS (320 KiB at K = 10, L = 64), so the tile of rows is resident and the components pass by it, one W_k staged at a time.
// LDS, all dynamic: W_k packed [L (L + 1) / 2] and mu_k [L] (fp64); z - mu_k [T][L | 1] (fp64; the odd row stride of 8-byte words keeps
// consecutive rows on different bank pairs; rows past the end of the tile are 0); l_nk and then r_nk [T][K | 1] (fp64); per row
// the max, ln of the sum and lse; the staged codes [T][L | 1] (fp32).  Per tile:
//   stage:  the tile's T L floats: one coalesced sweep;
//   E, for each k:  W_k and z - mu_k staged; a wave owns 16 rows and walks the 16-column blocks of y = (z - mu_k) W_k^T by
//           v_mfma_f64_16x16x4_f64: A = (z_n - mu_k)_j [16 rows x 4], B = W_k,ij [4 x 16 columns i] with 0 above the diagonal, j
//           only up to the block's last column; every result is squared into the lane's four row sums, and the 16 column lanes
//           of a row are added by xor shuffles in a fixed order; l = c_k - q / 2.  (The same product on the vector units, 16
//           threads sharing four rows, took 1.1 ms of a 1.38 ms iteration at N = 60,000, L = 64, K = 10:
//           profiles/mixfit_full_notes.md);
//   rows, sweep:  as mixfit_pass (the same text, kept in step by hand: csrc/mixfit.hpp says why): max, fp32 exponentials summed in
//           fp64, lse, log r written coalesced, r left in LDS; here l = -inf -- an absent component -- gives log r = -inf even in a
//           row whose every l is -inf;
//   M, for each k (kAccum):  z - mu_k staged again; R_k and S1_kd by four threads each, added by shuffles; S2_k by v_mfma_f64_16x16x4_f64: a wave
//           owns 16 x 16 blocks (bi >= bj only) of the L x L sum, A = (r_n (z_n - mu_k)_i) [16 x 4 rows], B = (z_n - mu_k)_j
//           [4 rows x 16], four rows of the tile an instruction; lane l holds A[i = l & 15][n = l >> 4] and B[n = l >> 4][j = l & 15],
//           and result register g holds D[i = (l >> 4) + 4 g][j = l & 15] -- the f64 form's own C/D map.  Columns past L and rows
//           past the tile enter as 0.  The entries on or below the diagonal are added to the workgroup's partials in the
//           workspace by their owner lane: a plain load, add, store (the first tile stores only, so the workspace needs no
//           initialisation); no atomics.
// With kAccum = false the same pass stops behind the sweep: gmvae_mixfit_full_assign.
// mixfit_full_update: folds the G workgroups' partials as mixfit_update does (16 slots a block, 16 threads a slot, fixed order):
// a slot is one (k, i, j <= i); it folds S2_kij, S1_ki, S1_kj and R_k (the same folds in the same order wherever they are
// repeated, so the same bits), applies the M-step and writes cov'_kij and cov'_kji -- bit-symmetric -- and, where i = j, mu'_ki.
// One more block folds R_k for every k and sum lse, and writes logw, counts_out and the history entry: mixfit_update's last block
// (csrc/mixfit.hpp mf_update_weights) at this layout's offset of R.  The plan ends in mf_plan_groups; the block size and the
// workgroup limit are kMfBlock and kMfMaxGroups.
// One owner per sum, fixed-order fp64 folds, no float atomics: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mixfit.hpp"

namespace gmvae {

constexpr int kMffMaxTile = 64;                    // rows per tile at most: 16 rows for each of the four waves
constexpr int kMffMaxL = 128;                      // the factor kernel holds 2 L (L + 1) / 2 fp64 in LDS: 129 KiB
constexpr int kMffMaxKLL = 1 << 20;                // the K L^2 gate
constexpr int64_t kMffMaxPart = 1ll << 23;         // doubles of partial sums at most (64 MiB): bounds the number of row slices

// the pass's shape for (N, L, K): rows per tile, rows per workgroup (whole tiles), workgroups, doubles per workgroup's partials,
// LDS bytes of the pass and of the factor kernel
struct MffPlan : MfPlan {
  size_t lds_factor;
};
static inline size_t mff_lds_bytes(int L, int K, int T) {
  const size_t Lp = (size_t)(L | 1), Kp = (size_t)(K | 1), P = (size_t)mff_tri(L);
  return 8 * (P + (size_t)L + (size_t)T * (Lp + Kp + 3)) + 4 * (size_t)T * Lp;
}
static inline MffPlan mff_plan(int64_t N, int L, int K) {
  MffPlan p;
  const size_t image = mff_lds_bytes(L, K, 0), row = mff_lds_bytes(L, K, 1) - image;
  int64_t T = (int64_t)(((size_t)kMfLdsBytes - image) / row);      // >= 44 inside the gate: image <= 67,072 and row <= 2,860 bytes
  T = T > kMffMaxTile ? kMffMaxTile : T;
  T &= ~(int64_t)3;
  p.stride = K * (mff_tri(L) + L + 1) + 1;      // S2 [K][L (L + 1) / 2], S1 [K][L], R [K], sum lse
  int64_t gmax = kMffMaxPart / p.stride;        // >= 7 inside the gate
  gmax = gmax > kMfMaxGroups ? kMfMaxGroups : gmax;
  mf_plan_groups(p, N, T, gmax);
  p.lds = mff_lds_bytes(L, K, (int)T);
  p.lds_factor = 16 * (size_t)mff_tri(L);
  return p;
}

__global__ __launch_bounds__(kMfBlock) void mixfit_full_factor(const float* __restrict__ cov, const int L, double* __restrict__ Wg,
                                                                double* __restrict__ sumlog, int32_t* __restrict__ info_out,
                                                                const int first) {
  extern __shared__ __attribute__((aligned(16))) char mff_smem[];
  const int tid = threadIdx.x, k = blockIdx.x, P = mff_tri(L);
  double* const a = reinterpret_cast<double*>(mff_smem);      // [P]: the lower triangle of cov_k, then C_k
  double* const x = a + P;                                    // [P]: the identity, then W_k
  const float* __restrict__ src = cov + (size_t)k * L * L;
  {
    const int i0 = tid / L, step_i = kMfBlock / L;
    for (int s = tid, i = i0, j = tid - i0 * L; s < L * L; s += kMfBlock) {
      if (j <= i) {
        a[mff_tri(i) + j] = (double)src[s];
        x[mff_tri(i) + j] = i == j ? 1.0 : 0.0;
      }
      MF_ADVANCE(i, j, step_i, kMfBlock - step_i * L, L);
    }
  }
  __syncthreads();
  double sl;
  const int info = mff_factor_lds(a, x, L, tid, sl);
  double* __restrict__ dst = Wg + (size_t)k * P;
  for (int s = tid; s < P; s += kMfBlock) dst[s] = info ? 0.0 : x[s];
  if (tid == 0) {
    sumlog[k] = info ? (double)INFINITY : sl;
    if (info_out && (first || info_out[k] == 0)) info_out[k] = info;
  }
}

template <bool kAccum>
__global__ __launch_bounds__(kMfBlock) void mixfit_full_pass(const float* __restrict__ codes, const int N, const int L, const int K,
                                                              const float* __restrict__ logw, const float* __restrict__ mu,
                                                              const double* __restrict__ Wg, const double* __restrict__ sumlog,
                                                              const int T, const int per_group, float* __restrict__ log_resp_out,
                                                              float* __restrict__ lse_out, double* __restrict__ part, const int stride) {
  extern __shared__ __attribute__((aligned(16))) char mff_smem[];
  const int tid = threadIdx.x, Lp = L | 1, Kp = K | 1, P = mff_tri(L), KP = K * P;
  double* const s_W = reinterpret_cast<double*>(mff_smem);      // [P]
  double* const s_mu = s_W + P;                                 // [L]
  double* const s_dz = s_mu + L;                                // [T][Lp]
  double* const s_l = s_dz + T * Lp;                            // [T][Kp]: l, then r
  double* const s_lse = s_l + T * Kp;                           // [T]
  double* const s_m = s_lse + T;                                // [T]
  double* const s_ls = s_m + T;                                 // [T]
  float* const s_z = reinterpret_cast<float*>(s_ls + T);        // [T][Lp]

  const int nL0 = tid / L, dL0 = tid - nL0 * L, stepL_n = kMfBlock / L, stepL_d = kMfBlock - stepL_n * L;
  const int nK0 = tid / K, kK0 = tid - nK0 * K, stepK_n = kMfBlock / K, stepK_d = kMfBlock - stepK_n * K;
  const int wave = tid >> 6, lane = tid & 63, nb = (L + 15) >> 4;

  const int64_t g_lo = (int64_t)blockIdx.x * per_group, g_hi = g_lo + per_group < N ? g_lo + per_group : N;
  double* const gpart = kAccum ? part + (size_t)blockIdx.x * stride : nullptr;
  double lse_acc = 0.0;      // (thread 0's)
  for (int64_t r0 = g_lo; r0 < g_hi; r0 += T) {
    const int rows = (int)(g_hi - r0 < T ? g_hi - r0 : T);
    __syncthreads();      // the previous tile's sums have read s_z
    {
      const float* __restrict__ src = codes + (size_t)r0 * L;
      int n = nL0, d = dL0;
      for (int i = tid; i < rows * L; i += kMfBlock) {
        s_z[n * Lp + d] = src[i];
        MF_ADVANCE(n, d, stepL_n, stepL_d, L);
      }
    }
    // z - mu_k for all T rows (0 past the end of the tile), mu_k in s_mu: called between two barriers
    auto stage_dz = [&]() {
      int n = nL0, d = dL0;
      for (int i = tid; i < T * L; i += kMfBlock) {
        s_dz[n * Lp + d] = n < rows ? (double)s_z[n * Lp + d] - s_mu[d] : 0.0;
        MF_ADVANCE(n, d, stepL_n, stepL_d, L);
      }
    };
    for (int k = 0; k < K; ++k) {
      __syncthreads();      // s_z is staged; the previous component's products have read s_W and s_dz
      {
        const double* __restrict__ wk = Wg + (size_t)k * P;
        for (int s = tid; s < P; s += kMfBlock) s_W[s] = wk[s];
        if (tid < L) s_mu[tid] = (double)mu[(size_t)k * L + tid];
      }
      __syncthreads();
      stage_dz();
      __syncthreads();
      const double sk = sumlog[k];
      const double c = sk == (double)INFINITY ? -(double)INFINITY : ((double)logw[k] - sk) - 0.91893853320467274178 * (double)L;
      for (int rb = wave; 16 * rb < rows; rb += kMfBlock >> 6) {      // (uniform in the wave: the MFMA runs with every lane on)
        const int n = 16 * rb + (lane & 15), jj = lane >> 4;
        const bool n_in = n < rows;
        const double* __restrict__ zr = s_dz + (n_in ? n : 0) * Lp;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
        for (int bi = 0; bi < nb; ++bi) {
          const int i = 16 * bi + (lane & 15);
          const bool i_in = i < L;
          const double* __restrict__ w = s_W + mff_tri(i_in ? i : 0);
          mff_d4 acc = {0.0, 0.0, 0.0, 0.0};
          for (int j0 = 0; j0 < 16 * bi + 16; j0 += 16) {      // four instructions' operands read ahead of the four products
            double av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int j = j0 + 4 * u + jj;
              av[u] = n_in && j < L ? zr[j] : 0.0;
              bv[u] = i_in && j <= i ? w[j] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
          }
          q0 = fma(acc[0], acc[0], q0);
          q1 = fma(acc[1], acc[1], q1);
          q2 = fma(acc[2], acc[2], q2);
          q3 = fma(acc[3], acc[3], q3);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {      // the 16 columns of a row: a fixed tree, every lane ends with the same bits
          q0 += __shfl_xor(q0, o);
          q1 += __shfl_xor(q1, o);
          q2 += __shfl_xor(q2, o);
          q3 += __shfl_xor(q3, o);
        }
        if ((lane & 15) == 0) {      // register g is row 16 rb + (lane >> 4) + 4 g
          const int n0 = 16 * rb + jj;
          double* __restrict__ o = s_l + n0 * Kp + k;
          if (n0 < rows) o[0] = fma(-0.5, q0, c);
          if (n0 + 4 < rows) o[4 * Kp] = fma(-0.5, q1, c);
          if (n0 + 8 < rows) o[8 * Kp] = fma(-0.5, q2, c);
          if (n0 + 12 < rows) o[12 * Kp] = fma(-0.5, q3, c);
        }
      }
    }
    __syncthreads();
    if (tid < rows) {
      const double* __restrict__ lr = s_l + tid * Kp;
      double m = -INFINITY;
      for (int k = 0; k < K; ++k) m = fmax(m, lr[k]);
      if (!(m > -INFINITY)) m = 0.0;      // (every component at -inf: lse = -inf, nothing to subtract)
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
      const double l = s_l[n * Kp + k];
      const float lr = l == -(double)INFINITY ? -INFINITY : (float)((l - s_m[n]) - s_ls[n]);
      if (log_resp_out) log_resp_out[(size_t)r0 * K + i] = lr;
      if (kAccum) s_l[n * Kp + k] = (double)expf(lr);
      MF_ADVANCE(n, k, stepK_n, stepK_d, K);
    }
    if (kAccum) {
      const bool first = r0 == g_lo;
      const int nblk = nb * (nb + 1) / 2;
      for (int k = 0; k < K; ++k) {
        __syncthreads();      // r is in place; the previous component's sums have read s_dz
        if (tid < L) s_mu[tid] = (double)mu[(size_t)k * L + tid];
        __syncthreads();
        stage_dz();
        __syncthreads();
        for (int s = tid; s < 4 * (L + 1); s += kMfBlock) {      // item (d, part): the rows part, part + 4, ...; d = L is R_k
          const int d = s >> 2, part = s & 3;
          double a = 0.0;
          if (d < L) {
            for (int n = part; n < rows; n += 4) a = fma(s_l[n * Kp + k], s_dz[n * Lp + d], a);
          } else {
            for (int n = part; n < rows; n += 4) a += s_l[n * Kp + k];
          }
          a += __shfl_xor(a, 1);      // (the four parts are neighbouring lanes, in or out of the loop together)
          a += __shfl_xor(a, 2);
          if (part == 0) {
            const int off = d < L ? KP + k * L + d : KP + K * L + k;
            if (!first) a += gpart[off];
            gpart[off] = a;
          }
        }
        for (int b = wave; b < nblk; b += kMfBlock >> 6) {      // (uniform in the wave: the MFMA runs with every lane on)
          int bi = 0, bj = b;
          while (bj > bi) {
            bj -= bi + 1;
            ++bi;
          }
          const int ia = 16 * bi + (lane & 15), ib = 16 * bj + (lane & 15), nn = lane >> 4;
          double prev[4] = {0.0, 0.0, 0.0, 0.0};      // the partials so far, asked for ahead of the products
          if (!first) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int i = 16 * bi + nn + 4 * g;
              if (i < L && ib <= i) prev[g] = gpart[k * P + mff_tri(i) + ib];
            }
          }
          mff_d4 acc = {0.0, 0.0, 0.0, 0.0};
          for (int n0 = 0; n0 < rows; n0 += 16) {      // four instructions' operands read ahead of the four products
            double av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int n = n0 + 4 * u + nn;
              const bool n_in = n < rows;      // (a row past `rows` enters as 0 and is not read)
              const double r = n_in ? s_l[n * Kp + k] : 0.0;
              av[u] = r * (n_in && ia < L ? s_dz[n * Lp + ia] : 0.0);
              bv[u] = n_in && ib < L ? s_dz[n * Lp + ib] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int i = 16 * bi + nn + 4 * g;
            if (i < L && ib <= i) gpart[k * P + mff_tri(i) + ib] = acc[g] + prev[g];
          }
        }
      }
    }
  }
  if (kAccum && tid == 0) gpart[KP + K * L + K] = lse_acc;
}

// blocks [0, slot_blocks): the M-step of kMfFoldSlots slots (k, i, j <= i) each; the last block: logw, counts_out, the history entry
__global__ __launch_bounds__(kMfBlock) void mixfit_full_update(const double* __restrict__ part, const int G, const int stride, const int N,
                                                               const int L, const int K, const float reg_covar, float* __restrict__ logw,
                                                               float* __restrict__ mu, float* __restrict__ cov,
                                                               float* __restrict__ hist_out, float* __restrict__ counts_out) {
  __shared__ double s_p[4][kMfFoldSlots][kMfFoldParts + 1];
  const int tid = threadIdx.x, q = tid / kMfFoldParts, p = tid % kMfFoldParts, P = mff_tri(L), KP = K * P;
  const int slot_blocks = (KP + kMfFoldSlots - 1) / kMfFoldSlots;
  if ((int)blockIdx.x < slot_blocks) {
    const int s = (int)blockIdx.x * kMfFoldSlots + q;
    const bool live = s < KP;
    const int k = live ? s / P : 0, t = live ? s - k * P : 0;
    int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (mff_tri(i + 1) <= t) ++i;
    while (mff_tri(i) > t) --i;
    const int j = t - mff_tri(i);
    if (live) {
      s_p[0][q][p] = mf_fold_run(part, G, stride, (size_t)s, p);
      s_p[1][q][p] = mf_fold_run(part, G, stride, (size_t)KP + k * L + i, p);
      s_p[2][q][p] = mf_fold_run(part, G, stride, (size_t)KP + k * L + j, p);
      s_p[3][q][p] = mf_fold_run(part, G, stride, (size_t)KP + K * L + k, p);
    }
    __syncthreads();
    if (live && p == 0) {
      double S2 = 0.0, S1i = 0.0, S1j = 0.0, R = 0.0;
      for (int u = 0; u < kMfFoldParts; ++u) {
        S2 += s_p[0][q][u];
        S1i += s_p[1][q][u];
        S1j += s_p[2][q][u];
        R += s_p[3][q][u];
      }
      // (the statement's operations in the statement's order, each rounded, as in mixfit_update: where one far point holds a
      // component, S2 / R' and m_i m_j agree to 15 digits, and a product contracted into an fma answers 8e-4 of reg_covar away)
      const double Rp = R + kMfEps0, mi = S1i / Rp, mj = S1j / Rp;
      double c;
      {
#pragma clang fp contract(off)
        const double mm = mi * mj;
        c = S2 / Rp - mm;
      }
      const size_t base = (size_t)k * L * L;
      if (i == j) {
        c = (c > 0.0 ? c : 0.0) + (double)reg_covar;
        mu[k * L + i] = (float)((double)mu[k * L + i] + mi);
      }
      cov[base + (size_t)i * L + j] = (float)c;
      cov[base + (size_t)j * L + i] = (float)c;
    }
    return;
  }
  mf_update_weights(part, G, stride, KP + K * L, N, K, logw, hist_out, counts_out, s_p);
}

}  // namespace gmvae
