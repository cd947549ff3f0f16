// The weighted objective (GmvaeDims::sched_flags & GMVAE_OBJ_WEIGHTS, S == 1): the KL terms of the bound carry weights a step
// reads from device memory -- wts = (beta_z, beta_y, lambda, 0), one row of the workspace's "obj_weights" -- so that a captured
// graph can warm them up step by step.  With nll, kl = log q(z|.) - log p(z|.) and nent_b = sum_k q ln q the existing terms,
//   VAE, VAE_GMP:      L_b = nll_b + beta_z kl_b                                (beta_y, lambda ignored)
//   GMVAE, Gumbel y:   L_b = nll_b + beta_z kl_b + beta_y ne'_b
//   GMVAE, y summed:   L_b = sum_k q_bk (nll_bk + beta_z kl_bk) + beta_y ne'_b
//   ne'_b = max(nent_b, lambda - ln K): free bits on KL(q(y|x_b) || uniform) = nent_b + ln K (the ln K stays out of the loss);
//   a_b = [nent_b > lambda - ln K] (1: the floor is inactive); lambda == 0 means no floor: a_b = 1, ne'_b = nent_b.
// The decoder path keeps the row weight rw (1, or q_bk); whatever differentiates the KL part (z_head_bwd's w, gmp_param_bwd's rw)
// takes rwk_r = beta_z rw_r in rw's place; the entropy term of dlogits takes beta_y a_b.  The kernels here stand where row_terms,
// ymarg_rows and y_head_bwd stand in the general schedule, and wobj_tail behind loss_tail; every other launch is the step's own.
// Fixed summation orders, no atomics: eager and graph steps give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace gmvae {

// the floor on the y term: a_b and ne'_b from nent_b and the step's lambda (lnK = ln K)
__device__ __forceinline__ bool wobj_floor(const float ne, const float lam, const float lnK, float& nef) {
  const float thr = lam - lnK;
  const bool on = lam == 0.f || ne > thr;        // (lambda == 0: off whatever the rounding of nent_b against -ln K)
  nef = on ? ne : thr;
  return on;
}

// Per-row terms in row_terms' place at S == 1 (row r = batch row b), one thread per row; nent null: the VAE family (no y term).
//   logpx_b = the fp64 sum of the decoder's Bernoulli partials (row_terms' sum), log w_b = logpx + logp - logq - nent (row_terms'
//   value: the row's importance weight does not depend on the objective's weights), terms4 (may be null) as row_terms
//   rwk_b = beta_z (may be null: forward only), act_b = a_b, pb[b] = (-L_b, nll_b, kl_b, 0) for loss_tail (L_b formed in fp64)
__global__ __launch_bounds__(256) void wobj_rows(const float* __restrict__ part, int nparts, const float* __restrict__ logq,
                                                 const float* __restrict__ logp, const float* __restrict__ nent,
                                                 const float* __restrict__ wts, float lnK, float* __restrict__ logpx,
                                                 float* __restrict__ logw, float* __restrict__ terms4, float* __restrict__ rwk,
                                                 float* __restrict__ pb, float* __restrict__ act, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float bz = wts[0], by = nent ? wts[1] : 0.f, lam = wts[2];
  double a64 = 0.0;
  for (int i = 0; i < nparts; ++i) a64 += (double)part[(long long)b * nparts + i];
  const float a = (float)a64, lq = logq[b], lp = logp[b];
  const float ne = nent ? nent[b] : 0.f;
  float nef = 0.f;
  const bool on = nent ? wobj_floor(ne, lam, lnK, nef) : true;
  const float lw = (float)(a64 + (double)lp - (double)lq - (double)ne);
  const double kl64 = (double)lq - (double)lp;
  const double L64 = -a64 + (double)bz * kl64 + (double)by * (double)nef;
  logpx[b] = a;
  logw[b] = lw;
  if (terms4) {
    terms4[4 * b + 0] = a;
    terms4[4 * b + 1] = lq;
    terms4[4 * b + 2] = lp;
    terms4[4 * b + 3] = lw;
  }
  if (rwk) rwk[b] = bz;
  act[b] = on ? 1.f : 0.f;
  pb[4 * b] = (float)(-L64);
  pb[4 * b + 1] = -a;
  pb[4 * b + 2] = lq - lp;
  pb[4 * b + 3] = 0.f;
}

// Per-example terms with y summed out, in ymarg_rows' place: one wave per batch row b, lanes stride over k (any K), row r = b K + k.
//   logpx_r, log w'_r = logpx + logp - logq, terms4 (may be null): ymarg_rows' values
//   l_bk = nll_bk + beta_z kl_bk (formed in fp64 from the fp64 sum of the partials), q = softmax(logits_b) (row_lse_parts)
//   rw_r = q_bk, rwk_r = beta_z q_bk (both may be null: forward only)
//   dlogits_bj = q_bj (l_bj - sum_k q_bk l_bk) + beta_y a_b q_bj (ln q_bj - nent_b)
//   nent[b] (unweighted), act_b = a_b, pb[b] = (-L_b, sum_k q nll, sum_k q kl, 0) for loss_tail
// dlogits holds l_bk between the two passes over k (the lane that writes it reads it back).  Fixed-order lane reductions.
__global__ __launch_bounds__(256) void ymarg_wobj_rows(const float* __restrict__ part, int nparts, const float* __restrict__ logq,
                                                       const float* __restrict__ logp, const float* __restrict__ logits,
                                                       const float* __restrict__ wts, float lnK, float* __restrict__ logpx,
                                                       float* __restrict__ logw, float* __restrict__ terms4, float* __restrict__ rw,
                                                       float* __restrict__ rwk, float* __restrict__ dlogits, float* __restrict__ nent,
                                                       float* __restrict__ pb, float* __restrict__ act, int B, int K) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* lg = logits + (long long)b * K;
  float m, l;
  row_lse_parts(lg, K, lane, m, l);
  const float bz = wts[0], by = wts[1], lam = wts[2];
  float ne = 0.f, sql = 0.f, nl = 0.f, kl = 0.f;
  for (int k = lane; k < K; k += 64) {
    const long long r = (long long)b * K + k;
    double a64 = 0.0;
    for (int i = 0; i < nparts; ++i) a64 += (double)part[r * nparts + i];
    const float a = (float)a64, lq = logq[r], lp = logp[r];
    const float lw = (float)(a64 + (double)lp - (double)lq);
    const float lk = (float)(-a64 + (double)bz * ((double)lq - (double)lp));
    logpx[r] = a;
    logw[r] = lw;
    if (terms4) {
      terms4[4 * r + 0] = a;
      terms4[4 * r + 1] = lq;
      terms4[4 * r + 2] = lp;
      terms4[4 * r + 3] = lw;
    }
    const float lpi = (lg[k] - m) - l, q = expf(lpi);
    dlogits[r] = lk;                                       // (r = b K + k: dlogits is [B][K])
    ne += q * lpi;
    sql += q * lk;
    nl -= q * a;
    kl += q * (lq - lp);
  }
  ne = wave_sum(ne); sql = wave_sum(sql); nl = wave_sum(nl); kl = wave_sum(kl);
  float nef;
  const bool on = wobj_floor(ne, lam, lnK, nef);          // (uniform over the wave: ne is the wave's sum)
  const float cy = on ? by : 0.f;
  for (int k = lane; k < K; k += 64) {
    const long long r = (long long)b * K + k;
    const float lpi = (lg[k] - m) - l, q = expf(lpi);
    if (rw) rw[r] = q;
    if (rwk) rwk[r] = bz * q;
    dlogits[r] = q * ((dlogits[r] - sql) + cy * (lpi - ne));
  }
  if (lane == 0) {
    nent[b] = ne;
    act[b] = on ? 1.f : 0.f;
    pb[4 * b] = -(sql + by * nef);
    pb[4 * b + 1] = nl;
    pb[4 * b + 2] = kl;
    pb[4 * b + 3] = 0.f;
  }
}

// y_head_bwd with the entropy term under the per-example coefficient beta_y a_b (act from wobj_rows):
//   dlogits_b = sum_s y (dy - y . dy) / T + beta_y a_b pi (log pi - nent_b)
// dy carries the weighted KL part already (z_head_bwd under rwk).  Both of y_head_bwd's paths -- one pass at K <= 64 and S <= 64,
// else the loop -- with its operations in its order.
__global__ __launch_bounds__(512) void y_head_bwd_w(const float* __restrict__ logits, const float* __restrict__ y,
                                                    const float* __restrict__ dy, const float* __restrict__ nent,
                                                    const float* __restrict__ wts, const float* __restrict__ act,
                                                    float* __restrict__ dlogits, int B, int S, int K, float invT) {
  __shared__ float red[8][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float by = wts[1];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* lg = logits + (long long)b * K;
    float m2, l2;
    row_lse_parts(lg, K, lane, m2, l2);
    const float ne = nent[b];
    const float cy = by * act[b];
    if (K <= 64 && S <= 64) {
      const bool kv = lane < K;
      float ys[8], ds[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int sidx = wave + 8 * j;
        const long long r = (long long)b * S + (sidx < S ? sidx : 0);
        ys[j] = (kv && sidx < S) ? y[r * K + lane] : 0.f;
        ds[j] = (kv && sidx < S) ? dy[r * K + lane] : 0.f;
      }
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (wave + 8 * j < S) {                    // (uniform per wave)
          const float ym = wave_max(kv ? fmaxf(0.f, ys[j]) : 0.f);
          const float c = wave_max((kv && ys[j] == ym) ? ds[j] : -INFINITY);
          const float dot = wave_sum(kv ? ys[j] * (ds[j] - c) : 0.f);
          if (kv) acc += ys[j] * ((ds[j] - c) - dot);
        }
      }
      red[wave][lane] = acc;
      __syncthreads();
      if (wave == 0 && kv) {
        float t = red[0][lane];
#pragma unroll
        for (int w = 1; w < 8; ++w) t += red[w][lane];
        const float lp = (lg[lane] - m2) - l2;
        dlogits[(long long)b * K + lane] = t * invT + cy * (expf(lp) * (lp - ne));
      }
      __syncthreads();
      continue;
    }
    for (int k0 = 0; k0 < K; k0 += 64) {
      const int k = k0 + lane;
      float acc = 0.f;
      for (int s = wave; s < S; s += 8) {
        const long long r = (long long)b * S + s;
        float ym = 0.f;
        for (int kk = lane; kk < K; kk += 64) ym = fmaxf(ym, y[r * K + kk]);
        ym = wave_max(ym);
        float c = -INFINITY;
        for (int kk = lane; kk < K; kk += 64) c = fmaxf(c, y[r * K + kk] == ym ? dy[r * K + kk] : -INFINITY);
        c = wave_max(c);
        float dot = 0.f;
        for (int kk = lane; kk < K; kk += 64) dot += y[r * K + kk] * (dy[r * K + kk] - c);
        dot = wave_sum(dot);
        if (k < K) acc += y[r * K + k] * ((dy[r * K + k] - c) - dot);
      }
      red[wave][lane] = acc;
      __syncthreads();
      if (wave == 0 && k < K) {
        float t = red[0][lane];                    // fixed order: the same bits whatever the timing
#pragma unroll
        for (int w = 1; w < 8; ++w) t += red[w][lane];
        const float lp = (lg[k] - m2) - l2;
        dlogits[(long long)b * K + k] = t * invT + cy * (expf(lp) * (lp - ne));
      }
      __syncthreads();
    }
  }
}

// One workgroup, right behind loss_tail on the same stream (which has just written zeros there): tail[5] = B beta_z,
// tail[6] = B beta_y (so that the data-parallel sum over tail[4] = B gives the weights back) and tail[7] = sum_b (1 - a_b), the
// examples whose y term sits on its floor.  Fixed-order tree: deterministic.  (The count is exact in fp32 up to 2^24 examples.)
__global__ __launch_bounds__(256) void wobj_tail(const float* __restrict__ act, const float* __restrict__ wts,
                                                 float* __restrict__ tail, int B) {
  __shared__ float red[256];
  float a0 = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) a0 += 1.f - act[b];
  red[threadIdx.x] = a0;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    tail[5] = (float)B * wts[0];
    tail[6] = (float)B * wts[1];
    tail[7] = red[0];
  }
}

}  // namespace gmvae
