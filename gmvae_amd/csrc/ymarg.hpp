// The GMVAE objective with the cluster variable y summed out exactly over its K values (GmvaeDims::sched_flags &
// GMVAE_OBJ_MARGINAL_Y; the objective of Rui Shu's GMVAE post, which the reference README names as its model) instead of one
// Gumbel-softmax draw of y (scripts/gmvae.py:238-240):
//   L_b = sum_k q(k|x_b) [ nll_bk + kl_bk ] + nent_b,   nent_b = sum_k q_bk ln q_bk
// R = B*K rows, row r = b*K + k, y_r = e_k; everything between the y layers and the per-example terms is the general schedule's
// S = K path.  The three kernels here are what changes: the one-hot y layers (a gather-add of one weight row, no GEMM over a
// one-hot operand), the per-example terms (softmax of the logits, the row weights q_bk, the closed-form logits gradient) and
// the one-hot weight gradients (segmented column sums over the batch into the split-K slabs).  Fixed summation orders
// throughout: eager and graph steps give the same bits.
// GMVAE_OBJ_MARGINAL_Y_IW adds S importance samples of z per component (R = B*S*K rows, row (b S + s) K + k): the same launches
// at S K rows per batch row, with ymarg_iw_rows in ymarg_rows' place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm.hpp"
#include "kernels.hpp"

namespace gmvae {

// Forward of the layers that read y = e_k, rpx rows per batch row (K for the step; S K for gmvae_iw_bound_enum_y's chunk of S
// samples, row (b S + s) K + k), b = r / rpx, k = r mod K:
//   encoder_gmm layer 0:  hg[r][j] = act(gx[b][j] + Wy[k][j] + b0[j])   (act = 0: the layer is the network's output, no activation)
//   prior_gmm:            pp[r][c] = Wp[k][c] + bp[c]                    (K distinct rows, gmvae.py:243 at y = e_k)
//   y (may be null):      y[r][c] = [c == k]
// gx = x Wx without bias (the first-layer launch's x-part, once per batch row).  One thread per output element, grid-stride.
__global__ __launch_bounds__(256) void ymarg_y_fwd(const float* __restrict__ gx, const float* __restrict__ Wy,
                                                   const float* __restrict__ b0, float* __restrict__ hg, int H, int act,
                                                   const float* __restrict__ Wp, const float* __restrict__ bp,
                                                   float* __restrict__ pp, int N2, float* __restrict__ y, int B, int K,
                                                   int rpx) {
  const long long R = (long long)B * rpx;
  const long long nh = R * H, np = R * N2, ny = y ? R * K : 0;
  const long long n = nh + np + ny;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (i < nh) {
      const long long r = i / H;
      const int j = (int)(i - r * H);
      const long long b = r / rpx;
      const int k = (int)(r % K);
      const float v = gx[b * H + j] + Wy[(long long)k * H + j] + b0[j];
      hg[i] = act ? act_apply(v, act) : v;
    } else if (i < nh + np) {
      const long long e = i - nh;
      const long long r = e / N2;
      const int c = (int)(e - r * N2);
      const int k = (int)(r % K);
      pp[e] = Wp[(long long)k * N2 + c] + bp[c];
    } else {
      const long long e = i - nh - np;
      const long long r = e / K;
      const int c = (int)(e - r * K);
      y[e] = (c == (int)(r % K)) ? 1.f : 0.f;
    }
  }
}

// Per-example terms, one wave per batch row b (lanes stride over k; any K):
//   logpx_r = sum of the decoder's Bernoulli partials (fp64 accumulation, as row_terms), log w'_r = logpx + logp - logq (no nent)
//   q = softmax(logits_b) (row_lse_parts: accurate for a saturated q), nent_b = sum_k q ln q
//   rw_r = q_bk (may be null: forward only) -- the weight every per-row backward epilogue takes
//   dlogits_bj = q_bj (l_bj - sum_k q_bk l_bk) + q_bj (ln q_bj - nent_b),  l = -log w'
//   pb[b] = (-L_b, sum_k q nll, sum_k q kl, 0) for loss_tail (S = 1 form), nent[b]
// terms4 (may be null): [R][4] = logpx, logq, logp, log w'.  Fixed-order lane reductions: deterministic.
__global__ __launch_bounds__(256) void ymarg_rows(const float* __restrict__ part, int nparts, const float* __restrict__ logq,
                                                  const float* __restrict__ logp, const float* __restrict__ logits,
                                                  float* __restrict__ logpx, float* __restrict__ logw, float* __restrict__ terms4,
                                                  float* __restrict__ rw, float* __restrict__ dlogits, float* __restrict__ nent,
                                                  float* __restrict__ pb, int B, int K) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* lg = logits + (long long)b * K;
  float m, l;
  row_lse_parts(lg, K, lane, m, l);
  float ne = 0.f, sql = 0.f, nl = 0.f, kl = 0.f;
  for (int k = lane; k < K; k += 64) {
    const long long r = (long long)b * K + k;
    double a64 = 0.0;
    for (int i = 0; i < nparts; ++i) a64 += (double)part[r * nparts + i];
    const float a = (float)a64, lq = logq[r], lp = logp[r];
    const float lw = (float)(a64 + (double)lp - (double)lq);
    logpx[r] = a;
    logw[r] = lw;
    if (terms4) {
      terms4[4 * r + 0] = a;
      terms4[4 * r + 1] = lq;
      terms4[4 * r + 2] = lp;
      terms4[4 * r + 3] = lw;
    }
    const float lpi = (lg[k] - m) - l, q = expf(lpi);
    ne += q * lpi;
    sql -= q * lw;
    nl -= q * a;
    kl += q * (lq - lp);
  }
  ne = wave_sum(ne); sql = wave_sum(sql); nl = wave_sum(nl); kl = wave_sum(kl);
  for (int k = lane; k < K; k += 64) {
    const long long r = (long long)b * K + k;
    const float lpi = (lg[k] - m) - l, q = expf(lpi);
    if (rw) rw[r] = q;
    dlogits[r] = q * ((-logw[r] - sql) + (lpi - ne));      // (r = b K + k: dlogits is [B][K])
  }
  if (lane == 0) {
    nent[b] = ne;
    pb[4 * b] = -(ne + sql);
    pb[4 * b + 1] = nl;
    pb[4 * b + 2] = kl;
    pb[4 * b + 3] = 0.f;
  }
}

// Per-example terms of GMVAE_OBJ_MARGINAL_Y_IW (y summed out, z importance-weighted over S samples per component), one wave per
// batch row b, lanes over k (any K), a loop over s; row r = (b S + s) K + k, so neighbouring lanes read neighbouring rows:
//   log w'_r = logpx_r + logp_r - logq_r (the Bernoulli partials summed in fp64 as ymarg_rows; lw64 keeps it in fp64)
//   l_bk = -(logsumexp_s log w'_bsk - ln S)   (the differences to the maximum over s formed in fp64, as iwae_rows)
//   q = softmax(logits_b) (row_lse_parts), nent_b = sum_k q ln q,  L_b = sum_k q_bk l_bk + nent_b
//   rw_r = q_bk softmax_s(log w'_bsk)_s (may be null: forward only) -- the weight every per-row backward epilogue takes
//   vs_r = softmax_s(log w'_bsk)_s alone (may be null; GMVAE_GRAD_DREG: z_head_bwd_dreg's second weight -- not rw / q, q can be denormal)
//   dlogits_bj = q_bj (l_bj - sum_k q_bk l_bk) + q_bj (ln q_bj - nent_b)
//   pb[b] = (-L_b, sum_k q mean_s nll, sum_k q mean_s kl, 0) for loss_tail (S = 1 form), nent[b]
// terms4 (may be null): [R][4] = logpx, logq, logp, log w'.  dlogits holds l_bk between the two passes over k (the lane that
// writes it reads it back).  Fixed-order lane reductions, no atomics: deterministic.  (S == 1 is ymarg_rows: the host routes it.)
__global__ __launch_bounds__(256) void ymarg_iw_rows(const float* __restrict__ part, int nparts, const float* __restrict__ logq,
                                                     const float* __restrict__ logp, const float* __restrict__ logits,
                                                     float* __restrict__ logpx, float* __restrict__ logw, double* __restrict__ lw64,
                                                     float* __restrict__ terms4, float* __restrict__ rw, float* __restrict__ vs,
                                                     float* __restrict__ dlogits, float* __restrict__ nent, float* __restrict__ pb,
                                                     int B, int S, int K) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* lg = logits + (long long)b * K;
  float m, l;
  row_lse_parts(lg, K, lane, m, l);
  const float invS = 1.f / (float)S, lnS = logf((float)S);
  const long long SK = (long long)S * K;
  float ne = 0.f, sql = 0.f, nl = 0.f, kl = 0.f;
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
    if (rw)
      for (int s = 0; s < S; ++s) {
        const long long r = r0 + (long long)s * K;
        const float sm = expf((float)(lw64[r] - mx) - lrel);
        rw[r] = q * sm;
        if (vs) vs[r] = sm;
      }
    dlogits[(long long)b * K + k] = lk;
    ne += q * lpi;
    sql += q * lk;
    nl += q * (na * invS);
    kl += q * (nk * invS);
  }
  ne = wave_sum(ne); sql = wave_sum(sql); nl = wave_sum(nl); kl = wave_sum(kl);
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
  }
}

// Weight gradients of the one-hot layers: dW[k][c] = sum_b d[b K + k][c] (B = the batch rows times S under GMVAE_OBJ_MARGINAL_Y_IW:
// row (b S + s) K + k is "batch row" b S + s) (and, with db, db[c] = sum_k dW[k][c]) for up to two
// row-gradient tensors d [R][N] -- the y rows of encoder_gmm's first layer (d = its pre-activation gradient) and prior_gmm
// (d = dpp).  The batch is split into ns contiguous chunks; chunk s writes slab s of the split-K slab buffer (finalize_grads
// sums the slabs in a fixed order).  A workgroup owns (problem, chunk, 64 columns); its four waves take every fourth k.
struct YmDwProb {
  const float* d;
  float *dw, *db;          // slab-0 addresses of the gradient [K][N] and (may be null) of the bias gradient [N]
  int N, ns, blocks;       // columns, chunks (slabs), workgroups of the problem = ns * ceil(N / 64)
};
struct YmDwArgs {
  YmDwProb p[2];
  int np, B, K;
  long long slab_stride;   // floats between slabs
};
__global__ __launch_bounds__(256) void ymarg_dw(const YmDwArgs a) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int blk = blockIdx.x, pi = 0;
  if (a.np > 1 && blk >= a.p[0].blocks) { blk -= a.p[0].blocks; pi = 1; }
  const YmDwProb& p = a.p[pi];
  const int ncg = (p.N + 63) / 64;
  const int s = blk / ncg, c = (blk - s * ncg) * 64 + lane;
  const bool cv = c < p.N;
  const int b0 = (int)((long long)a.B * s / p.ns), b1 = (int)((long long)a.B * (s + 1) / p.ns);
  const long long so = (long long)s * a.slab_stride;
  float bsum = 0.f;
  for (int k = wave; k < a.K; k += 4) {
    float acc = 0.f;
    if (cv) {
      const float* src = p.d + (long long)k * p.N + c;
      const long long rs = (long long)a.K * p.N;
#pragma unroll 8
      for (int b = b0; b < b1; ++b) acc += src[(long long)b * rs];
      p.dw[so + (long long)k * p.N + c] = acc;
    }
    bsum += acc;
  }
  if (p.db) {                                     // (uniform per workgroup)
    red[wave][lane] = bsum;
    __syncthreads();
    if (wave == 0 && cv) p.db[so + c] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
  }
}

}  // namespace gmvae
