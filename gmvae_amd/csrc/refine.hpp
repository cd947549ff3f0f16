// gmvae_refine (include/gmvae_hip.h; host side: csrc/ais.hip): per-example refinement of q(z|x) -- stochastic-gradient ascent on
// one example's own ELBO over the parameters phi = (m, s) of a local Gaussian q_phi(z) = N(m, diag e^{2 s}) (Cremer, Li & Duvenaud
// 2018), then the ELBO and the importance-weighted bound of the start phi_0 and of the refined phi* on common noise.  The statement
// is tests/refine_ref.py.
//   Target: log p(x, z) = log p(z) + log p(x|z) -- csrc/ais.hpp's ais_eval with enc = 0: A = log p(z), B = log p(x|z), the gradient
//   gA + gB.  Nothing of ais.hpp is restated: the panel geometry, the LDS layout (ais_lds) and the evaluation are its own.
//   Step t < n_steps, S samples eps_s:  z_s = m + e^s eps_s;  L-hat = 1/S sum_s log p(x, z_s) + sum_l s_l + L/2 (1 + ln 2 pi);
//     dm = 1/S sum_s g_s;  ds = 1/S sum_s g_s e^s eps_s + 1;  one ASCENT step of TF-Adam (adam.hpp adam_update on -d) on the 2 L
//     parameters with the example's own count t_b; a gradient that is not finite skips the update (moments and t_b untouched, as
//     gclip.hpp does for the training step), and so does one with an element of kRefineGMax = 2^63.5 = 1.3e19 or more in
//     magnitude: adam_update squares the element in fp32, 2^64 squared is past fp32's largest number, and a second moment of inf
//     would freeze that element for every later step while the rest of the example moved on (a prior sigma of 2e-9 gives
//     2.5e17 per unit distance: such gradients are finite and reachable); s clamped to [-20, 5] after the update.
//   Round t >= n_steps: S fresh eps, log w = log p(x, z) - log q_phi(z) at phi* and at phi_0 on the SAME eps: two evaluations.
// One workgroup of 256 threads owns a panel of kAisRows = 16 rows for every step of the launch; a row is one Monte-Carlo sample, an
// example's S samples (S in {1, 2, 4, 8, 16}) lie in one panel, which holds 16 / S examples; rows past the end repeat the last
// example and write nothing.  The example's FIRST row owns its optimizer state with the (row, j = tid % 16) element split of
// ais.hpp: its thread j forms z_l = m_l + e^{s_l} eps_l of the S rows for l = j, j + 16, ..., and after the evaluation reads the S
// rows of gA + gB from LDS in the order s = 0 .. S - 1, reduces dm, ds (fp64 sums over S) and L-hat (fp64 over S and L), and
// applies the update.  eps lives in the LDS `p` buffer, which the evaluation does not touch.
// State between launches AND between steps is the workspace's phi [B][6 L] (m, s, Adam's two moments of m, then of s), re-read per
// step by the thread that wrote it; the count t_b [B]; and per row the running (max, sum e, sum e^2, sum) of log w for phi* and
// phi_0 in fp64, folded in place by the owner's lane j = s.  No workgroup waits for another, no atomics, every sum has one owner and a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// ais.hpp defines its kernels as plain functions, so one library can include it from one translation unit only: csrc/ais.hip
// includes this header and hosts both entry points.
#include "adam.hpp"
#include "ais.hpp"

namespace gmvae {

constexpr float kRefineSMin = -20.f, kRefineSMax = 5.f;
constexpr float kRefineGMax = 0x1.6a09e6p+63f;      // 2^63.5 rounded to fp32: its square, 2^127, is the last binade fp32 has

struct RefineArgs {
  AisArgs a;                     // the evaluation's: enc = 0, C = S, n = B S, T = n_steps + n_rounds (ais_noise's key)
  int B, S, n_steps, t_lo, t_hi;      // this launch runs t_lo .. t_hi of the timeline: steps 0 .. n_steps - 1, then the rounds
  float lr, b1, b2, aeps;
  const float* start;            // [B][2 L]: mu_0, sigma_0
  float* phi;                    // [B][6 L]: m, s, Adam's (m, v) of m, Adam's (m, v) of s
  int* cnt;                      // [B]: updates applied
  double* acc;                   // [B S][8]: (max, sum e, sum e^2, sum) of log w at phi*, then at phi_0
  float* trace;                  // [n_steps][B] or null
};

// one more log w into a running (max, sum e^(lw - max), sum e^(2 (lw - max)), sum lw)
__device__ __forceinline__ void refine_fold(double* r, const double lw) {
  if (lw > r[0]) {
    const double e = exp(r[0] - lw);
    r[1] = r[1] * e + 1.0;
    r[2] = r[2] * e * e + 1.0;
    r[0] = lw;
  } else {
    const double e = exp(lw - r[0]);
    r[1] += e;
    r[2] += e * e;
  }
  r[3] += lw;
}

// Two waves per SIMD, as ais_run (profiles/refine_notes.md).
__global__ __launch_bounds__(kAisThreads, 2) void refine_run(const RefineArgs ra) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const AisArgs& a = ra.a;
  const AisLds s = ais_lds(a.L, a.n_hidden, a.hidden);
  const double half_log_2pi = 0.91893853320467274178;
  const int tid = threadIdx.x, row = tid >> 4, j = tid & 15, q = (tid & 63) >> 4;
  const int L = a.L, S = ra.S;
  const long long c_first = (long long)blockIdx.x * kAisRows;
  const bool live = c_first + row < a.n;
  const long long chain = live ? c_first + row : a.n - 1;      // (a row past the end repeats the last sample and writes nothing)
  const int b_row = (int)(chain / S);
  int xb[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) xb[v] = (int)(min(c_first + 4 * q + v, a.n - 1) / S);
  const int r0 = row - row % S;                                 // the example's first row of the panel (S divides 16)
  const bool own = row == r0;
  float* const zb = reinterpret_cast<float*>(smem + s.z) + r0 * s.ldz;
  float* const pb = reinterpret_cast<float*>(smem + s.p) + r0 * s.ldz;
  float* const gAb = reinterpret_cast<float*>(smem + s.gA) + r0 * s.ldz;
  float* const gBb = reinterpret_cast<float*>(smem + s.gB) + r0 * s.ldz;
  float* const pr = reinterpret_cast<float*>(smem + s.p) + row * s.ldz;
  double* const resp = reinterpret_cast<double*>(smem + s.resp);
  float* const ph = ra.phi + (long long)b_row * 6 * L;
  const float* const st = ra.start + (long long)b_row * 2 * L;
  const float omb1 = 1.f - ra.b1, omb2 = 1.f - ra.b2;

  int cnt = 0;
  if (ra.t_lo == 0) {
    if (own && live) {
      for (int l = j; l < L; l += 16) {
        ph[l] = st[l]; ph[L + l] = logf(st[L + l]);
        ph[2 * L + l] = 0.f; ph[3 * L + l] = 0.f; ph[4 * L + l] = 0.f; ph[5 * L + l] = 0.f;
      }
      if (j < S)
        for (int i = 0; i < 8; ++i) ra.acc[(chain + j) * 8 + i] = (i & 3) ? 0.0 : -INFINITY;
    }
  } else {
    cnt = ra.cnt[b_row];
  }
  for (int t = ra.t_lo; t <= ra.t_hi; ++t) {
    (void)ais_noise(a, chain, t, pr, j);
    __syncthreads();
    const bool opt = t < ra.n_steps;
    for (int pass = 0; pass < (opt ? 1 : 2); ++pass) {      // pass 0: the current phi; pass 1 (a round): phi_0
      double sum_s = 0.0;
      if (own) {
        for (int l = j; l < L; l += 16) {
          float m_l, s_l, sg;
          if (pass == 0) { m_l = ph[l]; s_l = ph[L + l]; }
          else { m_l = st[l]; s_l = logf(st[L + l]); }      // (phi_0 as the ascent holds it: s_0 = ln sigma_0 in fp32)
          sg = expf(s_l);
          sum_s += (double)s_l;
          for (int i = 0; i < S; ++i) zb[i * s.ldz + l] = m_l + sg * pb[i * s.ldz + l];
        }
      }
      sum_s = ais_row_sum(sum_s);
      __syncthreads();
      double vA, vB;
      ais_eval(a, s, smem, tid, b_row, xb, vA, vB);
      double val = vA + vB;
      if (!opt) {
        double ke = 0.0;
        for (int l = j; l < L; l += 16) ke += (double)(pr[l] * pr[l]);
        val += 0.5 * ais_row_sum(ke);                          // - log q_phi(z) = sum s + L/2 ln 2 pi + |eps|^2 / 2
      }
      if (j == 0) resp[row * kAisMaxK] = val;
      __syncthreads();
      if (!opt) {
        if (own && live && j < S)
          refine_fold(ra.acc + (chain + j) * 8 + 4 * pass, resp[(r0 + j) * kAisMaxK] + sum_s + (double)L * half_log_2pi);
        continue;      // (the next pass, or the next step's noise, meets a barrier before anything written here is read)
      }
      // ---- the step: d m, d s into the first row's gA, gB (each thread its own elements), then the update
      double lh = 0.0, bad = 0.0;
      if (own) {
        for (int i = 0; i < S; ++i) lh += resp[(r0 + i) * kAisMaxK];
        lh = lh / (double)S + sum_s + 0.5 * (double)L * (1.0 + 2.0 * half_log_2pi);
        for (int l = j; l < L; l += 16) {
          const double sg = (double)expf(ph[L + l]);
          double dm = 0.0, ds = 0.0;
          for (int i = 0; i < S; ++i) {
            const double g = (double)(gAb[i * s.ldz + l] + gBb[i * s.ldz + l]);
            dm += g;
            ds += g * sg * (double)pb[i * s.ldz + l];
          }
          const float fm = (float)(dm / (double)S), fs = (float)(ds / (double)S + 1.0);
          if (!(fabsf(fm) < kRefineGMax) || !(fabsf(fs) < kRefineGMax)) bad = 1.0;      // (a NaN compares false: skipped)
          gAb[l] = fm;
          gBb[l] = fs;
        }
      }
      bad = ais_row_sum(bad);
      if (own) {
        if (bad == 0.0) {
          ++cnt;
          const float lr_t =
              (float)((double)ra.lr * sqrt(1.0 - pow((double)ra.b2, (double)cnt)) / (1.0 - pow((double)ra.b1, (double)cnt)));
          if (live)
            for (int l = j; l < L; l += 16) {
              float m_l = ph[l], s_l = ph[L + l], m1 = ph[2 * L + l], v1 = ph[3 * L + l];
              adam_update(m_l, m1, v1, -gAb[l], 1.f, lr_t, omb1, omb2, ra.aeps);      // (g * 1 is g; a non-finite g never gets here)
              ph[l] = m_l; ph[2 * L + l] = m1; ph[3 * L + l] = v1;
              float m2 = ph[4 * L + l], v2 = ph[5 * L + l];
              adam_update(s_l, m2, v2, -gBb[l], 1.f, lr_t, omb1, omb2, ra.aeps);
              ph[L + l] = fminf(fmaxf(s_l, kRefineSMin), kRefineSMax); ph[4 * L + l] = m2; ph[5 * L + l] = v2;
            }
        }
        if (live && j == 0 && ra.trace) ra.trace[(long long)t * ra.B + b_row] = (float)lh;
      }
      __syncthreads();      // (the next step's noise overwrites the eps the owner has just read)
    }
  }
  if (own && live && j == 0) ra.cnt[b_row] = cnt;
}

// ---- per example: phi*, the four bounds, the effective sample size, the moves; fin [B][4] keeps the bounds in fp64 for the tail
// (ais_tail).  N = n_rounds S weights per example: the S rows' running sums merged in the order s = 0 .. S - 1.
__global__ __launch_bounds__(kAisThreads) void refine_finish(const float* __restrict__ phi, const float* __restrict__ start,
                                                             const int* __restrict__ cnt, const double* __restrict__ acc, const int B,
                                                             const int L, const int S, const int n_rounds,
                                                             float* __restrict__ phi_out, float* __restrict__ stats_out,
                                                             double* __restrict__ fin) {
  const int b = blockIdx.x * kAisThreads + threadIdx.x;
  if (b >= B) return;
  const double N = (double)S * (double)n_rounds;
  double elbo[2], iw[2], ess = 0.0;
  for (int p = 0; p < 2; ++p) {      // 0: phi*, 1: phi_0
    const double* r = acc + (long long)b * S * 8 + 4 * p;
    double m = -INFINITY;
    for (int i = 0; i < S; ++i) m = fmax(m, r[i * 8]);
    double s1 = 0.0, s2 = 0.0, sum = 0.0;
    for (int i = 0; i < S; ++i) {
      const double e = exp(r[i * 8] - m);
      s1 += r[i * 8 + 1] * e; s2 += r[i * 8 + 2] * e * e; sum += r[i * 8 + 3];
    }
    elbo[p] = sum / N;
    iw[p] = m + log(s1) - log(N);
    if (p == 0) ess = s1 * s1 / s2;
  }
  const float* ph = phi + (long long)b * 6 * L;
  const float* st = start + (long long)b * 2 * L;
  double dm = 0.0, ds = 0.0;
  for (int l = 0; l < L; ++l) {
    dm += (double)(fabsf(ph[l] - st[l]) / st[L + l]);
    ds += (double)ph[L + l] - (double)logf(st[L + l]);
    if (phi_out) { phi_out[(long long)b * 2 * L + l] = ph[l]; phi_out[(long long)b * 2 * L + L + l] = expf(ph[L + l]); }
  }
  if (stats_out) {
    float* o = stats_out + (long long)b * 8;
    o[0] = (float)elbo[1]; o[1] = (float)elbo[0]; o[2] = (float)iw[1]; o[3] = (float)iw[0]; o[4] = (float)ess; o[5] = (float)cnt[b];
    o[6] = (float)(dm / (double)L); o[7] = (float)(ds / (double)L);
  }
  fin[b * 4] = elbo[1]; fin[b * 4 + 1] = elbo[0]; fin[b * 4 + 2] = iw[1]; fin[b * 4 + 3] = iw[0];
}

}  // namespace gmvae
