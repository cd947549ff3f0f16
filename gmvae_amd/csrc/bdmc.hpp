// gmvae_simulate and gmvae_ais_reverse (include/gmvae_hip.h; host side: csrc/ais.hip): the two halves bidirectional Monte Carlo
// (Grosse, Ghahramani & Adams 2015; Wu, Burda, Salakhutdinov & Grosse 2017) adds to gmvae_ais.  The statement is tests/bdmc_ref.py.
//   sim_rows: ancestral sampling (z*, x) ~ p(z) p(x|z) from the generative model, so z* is an EXACT posterior sample for x.
//   bdmc_rev_run: gmvae_ais's annealing chain run backwards from z*, beta = 1 down to 0.  The reversal of a Metropolis-corrected
//     HMC kernel is the kernel itself, and the ratio of the reverse to the forward path density is w Z_0 / Z_T, so the reverse
//     weights have E[w_rev] = 1 / p(x): -(logsumexp_c log w_rev - ln C) is an upper bound on log p(x) in expectation, as
//     gmvae_ais's bound is a lower one.
// Nothing of ais.hpp is restated: the panel geometry, the LDS layout (ais_lds), the noise keying (ais_noise), the prior table
// (ais_prep), the layer product (ais_mm) and -- for the chain -- the evaluation (ais_eval) are its own; ais_run is untouched.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// ais.hpp defines its kernels as plain functions, so one library can include it from one translation unit only: csrc/ais.hip
// includes this header after it.
#include "ais.hpp"

namespace gmvae {

// ---- sim_rows.  One workgroup of 256 threads owns a PANEL of kAisRows = 16 examples (ais_run's geometry: thread (row = tid / 16,
// j = tid % 16) owns elements l = j, j + 16, ... of its row; rows past the end repeat the last example and write nothing).
//   k by inverse CDF of the prior's weights with one uniform (ais_run's t = 0 loop, fp64 cumulation); z* = mu_k + sigma_k eps;
//   lambda = decoder(z*) + bias, forward only, on ais_mm with the panel as the tile's 16 rows; the top layer in passes of
//   kAisChunk = 128 output columns, two tiles per wave, so any D fits; x_d = [u_d < sigmoid(lambda_d)] as bytes, straight from the
//   accumulators to global memory.
// Noise: a.T = 1 makes ais_noise's key step 2 + t: t = 0 is (eps, the component's uniform); the pixel uniforms are the u stream of
// row row_base + b at step 2 + 1, element d -- what gmvae_noise_fill(NULL, u, B, 1, D, row_base, seed, 2 step + 1) returns.
struct SimArgs {
  AisArgs a;                     // the sizes, the decoder, the bias and the prior table; n = B, C = 1, T = 1, eps [B][L], u [B] or null
  const float* ux;               // [B][D] or null: Philox
  float* z_out;                  // [B][L]
  int* k_out;                    // [B]
  unsigned char* x_out;          // [B][D]
  float* prob_out;               // [B][D] or null
};

__global__ __launch_bounds__(kAisThreads) void sim_rows(const SimArgs sa) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const AisArgs& a = sa.a;
  const AisLds s = ais_lds(a.L, a.n_hidden, a.hidden);
  const int tid = threadIdx.x, row = tid >> 4, j = tid & 15, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int L = a.L, D = a.D;
  const long long b_first = (long long)blockIdx.x * kAisRows;
  const bool live = b_first + row < a.n;
  const long long b = live ? b_first + row : a.n - 1;
  float* const sz = reinterpret_cast<float*>(smem + s.z);
  float* const zr = sz + row * s.ldz;
  float* const pr = reinterpret_cast<float*>(smem + s.p) + row * s.ldz;

  const float uk = ais_noise(a, b, 0, pr, j);
  __syncthreads();
  {
    int k = a.Kp - 1;
    double cum = 0.0;
    for (int kk = 0; kk < a.Kp; ++kk) {
      cum += exp((double)a.prior_lw[kk]);
      if ((double)uk < cum) { k = kk; break; }
    }
    for (int l = j; l < L; l += 16) {
      const float zv = a.prior_mu[k * L + l] + a.prior_sg[k * L + l] * pr[l];
      zr[l] = zv;
      if (live) sa.z_out[b * L + l] = zv;
    }
    if (live && j == 0) sa.k_out[b] = k;
  }
  __syncthreads();

  // ---- decoder: hidden layers
  const float* in = sz;
  int ld_in = s.ldz, n_in = L;
  for (int i = 0; i < a.n_hidden; ++i) {
    float* const h = reinterpret_cast<float*>(smem + s.h[i]);
    const int N = a.hidden[i];
    for (int n0 = w * 16; n0 < N; n0 += 64) {
      const ais_f4 acc = ais_mm<false>(in, ld_in, n_in, a.w[i], N, n0, N, lane);
      if (n0 + r < N) {
        const float bias = a.b[i][n0 + r];
#pragma unroll
        for (int v = 0; v < 4; ++v) h[(4 * q + v) * s.ldh[i] + n0 + r] = ais_act(acc[v] + bias, a.act);
      }
    }
    __syncthreads();
    in = h; ld_in = s.ldh[i]; n_in = N;
  }

  // ---- top layer in passes of kAisChunk columns: lane (r, q) holds rows 4 q .. 4 q + 3 of column n0 + r
  const float* const Wt = a.w[a.n_hidden];
  const float* const bt = a.b[a.n_hidden];
  const unsigned long long key = a.step * 2ull + 1ull;
  for (int c0 = 0; c0 < D; c0 += kAisChunk) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n0 = c0 + (2 * w + i) * 16;
      if (n0 >= D) continue;
      const ais_f4 acc = ais_mm<false>(in, ld_in, n_in, Wt, D, n0, D, lane);
      const int col = n0 + r;
      if (col >= D) continue;
      const float bias = bt[col] + (a.gen_bias_vec ? a.gen_bias_vec[col] : a.gen_bias);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const long long bb = b_first + 4 * q + v;
        if (bb >= a.n) continue;
        const float lam = acc[v] + bias;
        const float e = expf(-fabsf(lam));
        const float pv = lam >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        float uv;
        if (sa.ux) {
          uv = sa.ux[bb * D + col];
        } else {
          float o[4];
          noise_vals(a.row_base + (unsigned long long)bb, (uint32_t)(col >> 2), true, a.seed, key, o);
          const int e4 = col & 3;
          uv = e4 == 0 ? o[0] : e4 == 1 ? o[1] : e4 == 2 ? o[2] : o[3];
        }
        sa.x_out[bb * D + col] = uv < pv ? 1 : 0;
        if (sa.prob_out) sa.prob_out[bb * D + col] = pv;
      }
    }
  }
}

// ---- bdmc_rev_run.  ais_run's geometry, LDS layout and state carry; ais_eval as it is.  Chain (b, c) starts at z_T = z_start[b]
// (all chains of an example from the one exact sample), one evaluation there; then for t = T .. 1: one HMC transition on f_t --
// ais_run's, draw t of ais_noise --, then log w_rev -= (beta_t - beta_{t-1}) (B - A | B) at the NEW point z_{t-1}.  A launch runs
// t_hi down to t_lo; t_hi = T + 1 is the start, which shares the one evaluation call site.
struct RevArgs {
  AisArgs a;
  const float* z_start;          // [B][L]
};

// Two waves per SIMD, as ais_run (profiles/bdmc_notes.md).
__global__ __launch_bounds__(kAisThreads, 2) void bdmc_rev_run(const RevArgs ra) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const AisArgs& a = ra.a;
  const AisLds s = ais_lds(a.L, a.n_hidden, a.hidden);
  const int tid = threadIdx.x, row = tid >> 4, j = tid & 15, q = (tid & 63) >> 4;
  const int L = a.L;
  const long long c_first = (long long)blockIdx.x * kAisRows;
  const bool live = c_first + row < a.n;
  const long long chain = live ? c_first + row : a.n - 1;      // (a row past the end repeats the last chain and writes nothing)
  const int b_row = (int)(chain / a.C);
  int xb[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) xb[v] = (int)(min(c_first + 4 * q + v, a.n - 1) / a.C);
  float* const zr = reinterpret_cast<float*>(smem + s.z) + row * s.ldz;
  float* const pr = reinterpret_cast<float*>(smem + s.p) + row * s.ldz;
  float* const gAr = reinterpret_cast<float*>(smem + s.gA) + row * s.ldz;
  float* const gBr = reinterpret_cast<float*>(smem + s.gB) + row * s.ldz;
  float* const wz = a.st_z + chain * L;
  float* const wA = a.st_gA + chain * L;
  float* const wB = a.st_gB + chain * L;

  double vA = 0.0, vB = 0.0, logw = 0.0;
  float step = a.step0;
  int nacc = 0;
  unsigned long long bits = 0ull;
  if (a.t_hi <= a.T) {
    for (int l = j; l < L; l += 16) { zr[l] = wz[l]; gAr[l] = wA[l]; gBr[l] = wB[l]; }
    vA = a.st_d[chain * 4]; vB = a.st_d[chain * 4 + 1]; logw = a.st_d[chain * 4 + 2];
    step = a.st_eps[chain];
    nacc = a.st_acc[chain];
    bits = a.st_bits[chain];
  }
  for (int t = a.t_hi; t >= a.t_lo; --t) {
    const bool hmc = t <= a.T;
    const float uacc = hmc ? ais_noise(a, chain, t, pr, j) : 1.f;
    __syncthreads();
    const double beta = hmc ? (double)a.betas[t] : 1.0;
    const float cA = a.enc ? (float)(1.0 - beta) : 1.f, cB = (float)beta;
    const double vA0 = vA, vB0 = vB;
    double h_old = 0.0;
    if (!hmc) {
      const float* zs = ra.z_start + (long long)b_row * L;
      for (int l = j; l < L; l += 16) zr[l] = zs[l];
    } else {
      double ke = 0.0;
      for (int l = j; l < L; l += 16) ke += (double)(pr[l] * pr[l]);
      h_old = -((double)cA * vA + (double)cB * vB) + 0.5 * ais_row_sum(ke);
      for (int l = j; l < L; l += 16) {
        pr[l] += 0.5f * step * (cA * gAr[l] + cB * gBr[l]);
        zr[l] += step * pr[l];
      }
    }
    const int n_eval = hmc ? a.n_leap : 1;
    for (int i = 1; i <= n_eval; ++i) {
      __syncthreads();
      ais_eval(a, s, smem, tid, b_row, xb, vA, vB);
      if (hmc) {
        const float kick = i < n_eval ? step : 0.5f * step;
        for (int l = j; l < L; l += 16) {
          pr[l] += kick * (cA * gAr[l] + cB * gBr[l]);
          if (i < n_eval) zr[l] += step * pr[l];
        }
      }
    }
    bool keep = true;
    if (hmc) {
      double ke = 0.0;
      for (int l = j; l < L; l += 16) ke += (double)(pr[l] * pr[l]);
      const double h_new = -((double)cA * vA + (double)cB * vB) + 0.5 * ais_row_sum(ke);
      keep = (fabs(h_new) < INFINITY) && log((double)uacc) < h_old - h_new;      // (a NaN compares false: rejected)
      nacc += keep ? 1 : 0;
      if (keep && t <= 64) bits |= 1ull << (t - 1);
      step = fminf(fmaxf(step * (keep ? a.step_up : a.step_down), kAisStepMin), kAisStepMax);
    }
    if (keep) {
      if (live)
        for (int l = j; l < L; l += 16) { wz[l] = zr[l]; wA[l] = gAr[l]; wB[l] = gBr[l]; }
    } else {
      for (int l = j; l < L; l += 16) { zr[l] = wz[l]; gAr[l] = wA[l]; gBr[l] = wB[l]; }
      vA = vA0; vB = vB0;
    }
    if (hmc) logw -= (beta - (double)a.betas[t - 1]) * (a.enc ? vB - vA : vB);      // at z_{t-1}, the point the transition left
  }
  if (live) {
    if (j == 0) {
      a.st_d[chain * 4] = vA; a.st_d[chain * 4 + 1] = vB; a.st_d[chain * 4 + 2] = logw; a.st_d[chain * 4 + 3] = 0.0;
      a.st_eps[chain] = step;
      a.st_acc[chain] = nacc;
      a.st_bits[chain] = bits;
    }
    if (a.t_lo == 1 && a.z_out)
      for (int l = j; l < L; l += 16) a.z_out[chain * L + l] = zr[l];
  }
}

}  // namespace gmvae
