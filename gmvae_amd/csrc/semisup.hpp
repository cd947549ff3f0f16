// The semi-supervised GMVAE objective (GmvaeDims::sched_flags & GMVAE_OBJ_LABELS, together with GMVAE_OBJ_MARGINAL_Y or
// GMVAE_OBJ_MARGINAL_Y_IW): the component of some examples is observed and clamps y for them -- Kingma et al.'s M2 objective,
// whose unlabelled half the marginal objectives already are.  With l_bk the marginal objectives' per-component term, c = c_b
// the observed component (outside [0, K): unlabelled) and alpha the classification weight,
//   unlabelled:  L_b = sum_k q_bk l_bk + nent_b                                 (ymarg_rows / ymarg_iw_rows, the same bits)
//   labelled:    L_b = l_bc + alpha (-ln q_bc),  rw_r = [k == c] softmax_s(log w'_bsc)_s,  dlogits_bj = alpha (q_bj - [j == c])
// Every launch between the y layers and these per-example terms, and every backward launch, is the marginal step's: the
// backward takes its row weights, DReG's second weight and the closed-form dlogits from here.  A labelled example still runs
// all K components through the networks with K - 1 zero row weights.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace gmvae {

// Per-example terms under GMVAE_OBJ_LABELS, in ymarg_rows' / ymarg_iw_rows' place: one wave per batch row b, lanes over k (any K),
// a loop over s (S >= 1); row r = (b S + s) K + k.  The forward outputs -- logpx, logw, lw64, terms4 (may be null), and vs (may be
// null: GMVAE_GRAD_DREG's softmax_s(log w'_bsk)_s) -- are written for every row of every example, labelled or not.
//   unlabelled (labels[b] outside [0, K)): ymarg_iw_rows' operations in ymarg_iw_rows' order (at S == 1 they give ymarg_rows'
//     values: max = log w', sum of exp = 1, ln 1 = 0, softmax_s = 1), so a batch without labels is the marginal step's bits
//   labelled, c = labels[b]:
//     rw_r = [k == c] softmax_s(log w'_bsc)_s   (may be null: forward only)
//     ce_b = -ln q_bc = -((lg_c - m) - l) from row_lse_parts' log-softmax parts (never logf(q): q may be denormal)
//     dlogits_bj = alpha (q_bj - [j == c]),  nent_b = 0
//     pb[b] = (-(l_bc + alpha ce_b), mean_s nll_bsc, mean_s kl_bsc, 0) for loss_tail
//   trip[b] = (ce_b, 1, [argmax_k lg_bk == c]) (the argmax's lowest index on ties), (0, 0, 0) for an unlabelled example: sup_tail
// dlogits holds l_bk between the two passes over k (the lane that writes it reads it back).  Fixed-order lane reductions, no
// atomics: deterministic.
__global__ __launch_bounds__(256) void ymarg_sup_rows(const float* __restrict__ part, int nparts, const float* __restrict__ logq,
                                                      const float* __restrict__ logp, const float* __restrict__ logits,
                                                      const int32_t* __restrict__ labels, const float* __restrict__ alpha_p,
                                                      float* __restrict__ logpx, float* __restrict__ logw, double* __restrict__ lw64,
                                                      float* __restrict__ terms4, float* __restrict__ rw, float* __restrict__ vs,
                                                      float* __restrict__ dlogits, float* __restrict__ nent, float* __restrict__ pb,
                                                      float* __restrict__ trip, int B, int S, int K) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* lg = logits + (long long)b * K;
  float m, l;
  row_lse_parts(lg, K, lane, m, l);
  const int c = labels[b];
  const bool lab = c >= 0 && c < K;              // (uniform over the wave)
  const float alpha = *alpha_p;
  const float invS = 1.f / (float)S, lnS = logf((float)S);
  const long long SK = (long long)S * K;
  float ne = 0.f, sql = 0.f, nl = 0.f, kl = 0.f;
  int amax = 0x7fffffff;                         // lowest k whose logit is the row maximum
  for (int k = lane; k < K; k += 64) {
    const long long r0 = (long long)b * SK + k;
    double mx = -INFINITY;
    float na = 0.f, nk = 0.f;
    for (int s = 0; s < S; ++s) {
      const long long r = r0 + (long long)s * K;
      double a64 = 0.0;
      for (int i = 0; i < nparts; ++i) a64 += (double)part[r * nparts + i];
      const float a = (float)a64, lq = logq[r], lp = logp[r];
      const double w64 = a64 + (double)lp - (double)lq;
      const float lw = (float)w64;
      logpx[r] = a;
      logw[r] = lw;
      lw64[r] = w64;
      if (terms4) {
        terms4[4 * r + 0] = a;
        terms4[4 * r + 1] = lq;
        terms4[4 * r + 2] = lp;
        terms4[4 * r + 3] = lw;
      }
      mx = fmax(mx, w64);
      na -= a;
      nk += lq - lp;
    }
    float se = 0.f;
    for (int s = 0; s < S; ++s) se += expf((float)(lw64[r0 + (long long)s * K] - mx));
    const float lrel = logf(se);
    const float lk = -(float)(mx + (double)lrel - (double)lnS);
    const float lpi = (lg[k] - m) - l, q = expf(lpi);
    if (rw || vs)
      for (int s = 0; s < S; ++s) {
        const long long r = r0 + (long long)s * K;
        const float sm = expf((float)(lw64[r] - mx) - lrel);
        if (rw) rw[r] = lab ? (k == c ? sm : 0.f) : q * sm;
        if (vs) vs[r] = sm;
      }
    if (lab) {
      if (k == c) {                                // (one lane: the sums below are that lane's terms, exactly)
        sql = lk;
        nl = na * invS;
        kl = nk * invS;
        ne = -lpi;                                 // ce_b, in ne's place: a labelled example has no entropy term
      }
      if (lg[k] == m && k < amax) amax = k;
    } else {
      dlogits[(long long)b * K + k] = lk;
      ne += q * lpi;
      sql += q * lk;
      nl += q * (na * invS);
      kl += q * (nk * invS);
    }
  }
  ne = wave_sum(ne); sql = wave_sum(sql); nl = wave_sum(nl); kl = wave_sum(kl);
  if (lab) {
    for (int o = 32; o > 0; o >>= 1) amax = min(amax, __shfl_xor(amax, o, 64));
    for (int k = lane; k < K; k += 64) {
      const float q = expf((lg[k] - m) - l);
      dlogits[(long long)b * K + k] = alpha * (q - (k == c ? 1.f : 0.f));
    }
    if (lane == 0) {
      nent[b] = 0.f;
      pb[4 * b] = -(sql + alpha * ne);
      pb[4 * b + 1] = nl;
      pb[4 * b + 2] = kl;
      pb[4 * b + 3] = 0.f;
      trip[3 * b] = ne;
      trip[3 * b + 1] = 1.f;
      trip[3 * b + 2] = amax == c ? 1.f : 0.f;
    }
    return;
  }
  for (int k = lane; k < K; k += 64) {
    float* const dl = dlogits + (long long)b * K + k;
    const float lpi = (lg[k] - m) - l, q = expf(lpi);
    *dl = q * ((*dl - sql) + (lpi - ne));
  }
  if (lane == 0) {
    nent[b] = ne;
    pb[4 * b] = -(ne + sql);
    pb[4 * b + 1] = nl;
    pb[4 * b + 2] = kl;
    pb[4 * b + 3] = 0.f;
    trip[3 * b] = 0.f;
    trip[3 * b + 1] = 0.f;
    trip[3 * b + 2] = 0.f;
  }
}

// One workgroup, right behind loss_tail on the same stream (which has just written zeros there): the sums over the batch of
// ymarg_sup_rows' per-example triples into tail[5] = sum of -ln q_bc, tail[6] = labelled examples, tail[7] = hits.  Fixed-order
// tree: deterministic.  (Counts are exact in fp32 up to 2^24 examples per device.)
__global__ __launch_bounds__(256) void sup_tail(const float* __restrict__ trip, float* __restrict__ tail, int B) {
  __shared__ float red[3][256];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    a0 += trip[3 * b];
    a1 += trip[3 * b + 1];
    a2 += trip[3 * b + 2];
  }
  red[0][threadIdx.x] = a0; red[1][threadIdx.x] = a1; red[2][threadIdx.x] = a2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int j = 0; j < 3; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    tail[5] = red[0][0];
    tail[6] = red[1][0];
    tail[7] = red[2][0];
  }
}

}  // namespace gmvae
