// gmvae_tsne_* (include/gmvae_hip.h; host side: csrc/tsne.hip): exact t-SNE of N codes c [N][L] into y [N][2], O(N^2) per
// iteration, no tree and no FFT; memory follows N (and rows N for the affinity stage's chunk of distance rows), never N^2.  Model independent.
//   d2_ij = sum_d (c_id - c_jd)^2, always in the difference form on the vector units (never the expanded square, which cancels
//   -- aggpost.hpp's header gives the reason -- and so never the Gram form on the matrix cores).  The differences and their sum
//   are fp64: a point 1e3 away from the rest has beta d2 around 2e3, and an fp32 sum's 1e-7 d2 moved that row's beta by 6e-5
//   and its p_{j|i} by 2.3e-4 of the row's maximum (measured; profiles/tsne_notes.md).  v_add_f64 and v_fma_f64 issue at the
//   rate of their unpacked fp32 forms here; the price is LDS traffic and registers (below).
// Affinities (tsne_dist, tsne_search), rows [r0, r0 + rows): tsne_dist writes d2 [rows][N] (rounded once, to fp32) into the
// workspace -- a lane owns a row, a 256-thread block 256 rows, tiles of kTsTile points c_j are staged in LDS kTsDims dimensions
// at a time and read back as broadcasts (every lane of a wave reads the same address), the tile's kTsTile sums live in
// registers; grid.y splits the j range so a small chunk still fills the chip.  tsne_search then gives a wave (kTsWave lanes) to
// each stored row: the lanes stride over j (coalesced), and every trial beta costs one pass over the row,
//   x_j = fma(-beta, d2_ij, m), m = beta min_j d2_ij;  S = sum_{j != i} e^x_j;  U = sum_{j != i} x_j e^x_j;  H = ln S - U / S
// which is the entropy of softmax(-beta d2) for ANY shift m: the fma rounds once, after the cancellation, so H carries no
// rounding of beta d2 however far the point is from the others, and S and U are fp64 (fp32 terms, fp64 sums per lane, a fixed
// xor tree over the wave), so H is good to about 1e-7 at N = 60,000 too.  Search: beta = 1, doubled or halved until the root is
// bracketed (at most kTsMaxDoublings times), then bisected until fp32 cannot split the bracket (24 halvings; at most
// kTsMaxHalvings).  It does NOT stop at |H - ln perplexity| <= 1e-5: on a row whose nearest neighbours nearly tie, dH / dln beta
// is small and that stop leaves logz 2.6e-4 off (N = 5, L = 1, perplexity 2, four clusters) and p_{j|i} 1.3e-4 of the row's
// maximum off (N = 33, L = 4, perplexity 8); bisected out, every row ends within 1e-5 of the target by a wide margin.
// logz = ln S - m.  A ROW WITH NO ROOT -- a point with at least `perplexity` exact duplicates has H >= ln(duplicates) at every
// beta, and so has a point whose `perplexity` nearest neighbours tie exactly -- keeps the last beta tried and reports the entropy
// reached there; nothing "fixes" it.  A row's result does not depend on the chunk it was computed in: chunking changes no bit.
// One iteration (tsne_pairs, tsne_fold, tsne_reduce, tsne_grad): a lane owns point i; tiles of j are staged as (c_j, y_j, beta_j,
// logz_j); d2_ij is rebuilt by the same code as in tsne_dist and p_ij = (e^fma(-beta_i, d2, -logz_i) + e^fma(-beta_j, d2,
// -logz_j)) / 2N from it (fp64 fmas: one rounding each, after the cancellation; both exponents <= 0 up to rounding; the
// exponentials are fp32), w_ij = 1 / (1 + |y_i - y_j|^2); per point the sums  attr = sum_j p w (y_i - y_j),  rep = sum_j w^2
// (y_i - y_j),  sum_j w,  sum_j p ln w  (and, on the first pass of a run only, sum_j p ln p: it is constant) -- fp32 within a
// tile, fp64 across tiles.  grid.y slices the j range for small N (ts_slices); the slices' partial sums go to the workspace and
// fold in slice order, Z = sum_i sum_j w and the KL pieces fold over i in a fixed order in one block, in fp64; Z being global, a
// second small launch forms
//   grad_i = 4 (alpha attr_i - rep_i / Z);   KL = sum p ln p - sum p ln w + ln Z   (the un-exaggerated P; p = 0 contributes 0).
// tsne_update is scikit-learn's _gradient_descent step, element-wise, without recentring.  No float atomics, one owner per
// sum, fixed-order folds: two runs give the same bits.  Cost: about 3 L + 30 flops per ordered pair and iteration.
// Constants: a block of kTsBlock = 256 lanes (points); kTsTile = 32 points per tile (their 32 fp64 sums, the 8 staged dimensions
// and the 7 + 7 tile and running sums stay in registers: 172 registers in tsne_pairs, no spill, 2 blocks a CU); kTsDims = 64
// dimensions per staging round (rows of 66 doubles: 16-byte rows, 17 KiB of LDS per block); slices begin at multiples of kTsTile.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "d2tile.hpp"

namespace gmvae {

constexpr int kTsWave = 64;          // tsne_search: lanes per row
constexpr int kTsAcc = 7;            // per-point sums: attr x, attr y, rep x, rep y, sum w, sum p ln w, sum p ln p
constexpr int kTsMaxHalvings = 100;
constexpr int kTsMaxDoublings = 80;

// d2 [rows][N] of the rows [r0, r0 + rows): one slice of the j range per blockIdx.y
__global__ __launch_bounds__(kTsBlock) void tsne_dist(const float* __restrict__ codes, const int N, const int L, const int r0,
                                                      const int rows, const int per_slice, float* __restrict__ d2) {
  __shared__ __attribute__((aligned(16))) double s_c[kTsTile][kTsLd];
  const int tid = threadIdx.x;
  const long long r = (long long)blockIdx.x * kTsBlock + tid;
  const bool live = r < rows;
  const float* __restrict__ ci = codes + (size_t)(r0 + (live ? r : 0)) * L;      // (a lane past the end computes on row r0 and writes nothing)
  const int c_lo = (int)blockIdx.y * per_slice, c_hi = min(N, c_lo + per_slice);
  for (int c0 = c_lo; c0 < c_hi; c0 += kTsTile) {
    double acc[kTsTile];
    ts_tile_d2(acc, s_c, codes, ci, L, c0, c_hi, tid);
    if (live) {
      float* __restrict__ o = d2 + (size_t)r * N + c0;
#pragma unroll
      for (int ct = 0; ct < kTsTile; ++ct)
        if (c0 + ct < c_hi) o[ct] = (float)acc[ct];
    }
  }
}

__device__ __forceinline__ double ts_wave_sum(double v) {
#pragma unroll
  for (int o = kTsWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);      // (a + b == b + a: every lane ends with the same bits)
  return v;
}

// the root beta_i of H_i(beta) = ln perplexity over the stored row, one wave per row; outputs at index r0 + r
__global__ __launch_bounds__(kTsBlock) void tsne_search(const float* __restrict__ d2, const int N, const int r0, const int rows,
                                                        const double target, float* __restrict__ beta, float* __restrict__ logz,
                                                        float* __restrict__ entropy) {
  const int lane = threadIdx.x & (kTsWave - 1);
  const long long r = (long long)blockIdx.x * (kTsBlock / kTsWave) + (threadIdx.x / kTsWave);
  if (r >= rows) return;      // (the whole wave leaves; no block-wide synchronisation below)
  const int i = r0 + (int)r;
  const float* __restrict__ row = d2 + (size_t)r * N;
  float dmin = INFINITY;
  for (int j = lane; j < N; j += kTsWave)
    if (j != i) dmin = fminf(dmin, row[j]);
#pragma unroll
  for (int o = kTsWave / 2; o > 0; o >>= 1) dmin = fminf(dmin, __shfl_xor(dmin, o));
  float b = 1.f, lo = 0.f, hi = INFINITY, m = 0.f;
  int halvings = 0, doublings = 0;
  double S = 1.0, H = 0.0;
  for (;;) {
    m = b * dmin;
    double s = 0.0, u = 0.0;
    for (int j = lane; j < N; j += kTsWave) {
      if (j == i) continue;
      const float x = fmaf(-b, row[j], m), e = __expf(x);
      s += (double)e;
      u += (double)(e > 0.f ? x * e : 0.f);
    }
    S = ts_wave_sum(s);
    const double U = ts_wave_sum(u);
    H = log(S) - U / S;
    const double diff = H - target;
    if (diff == 0.0) break;
    float nb;
    if (diff > 0.0) {      // too flat: a larger beta
      lo = b;
      if (hi == INFINITY) {
        if (++doublings > kTsMaxDoublings) break;
        nb = b * 2.f;
      } else {
        if (++halvings > kTsMaxHalvings) break;
        nb = 0.5f * (b + hi);
      }
    } else {
      hi = b;
      if (lo == 0.f) {
        if (++doublings > kTsMaxDoublings) break;
        nb = b * 0.5f;
      } else {
        if (++halvings > kTsMaxHalvings) break;
        nb = 0.5f * (lo + b);
      }
    }
    if (nb == lo || nb == hi) break;      // fp32 cannot split the bracket any further
    b = nb;
  }
  if (lane == 0) {
    beta[i] = b;
    logz[i] = (float)(log(S) - (double)m);
    entropy[i] = (float)H;
  }
}

// the per-point sums of one slice of the j range: part [slice][N][kTsAcc]
template <bool kPlogp>
__global__ __launch_bounds__(kTsBlock) void tsne_pairs(const float* __restrict__ codes, const int N, const int L,
                                                       const float* __restrict__ beta, const float* __restrict__ logz,
                                                       const float* __restrict__ y, const int per_slice, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double s_c[kTsTile][kTsLd];
  __shared__ float4 s_meta[kTsTile];      // (y_j0, y_j1, beta_j, logz_j)
  const int tid = threadIdx.x;
  const long long gi = (long long)blockIdx.x * kTsBlock + tid;
  const bool live = gi < N;
  const int i = live ? (int)gi : 0;      // (a lane past the end computes on point 0 and writes nothing)
  const float* __restrict__ ci = codes + (size_t)i * L;
  const double bi = (double)beta[i], lzi = (double)logz[i];
  const float yi0 = y[2 * (size_t)i], yi1 = y[2 * (size_t)i + 1];
  const float inv2n = 0.5f / (float)N;
  const int c_lo = (int)blockIdx.y * per_slice, c_hi = min(N, c_lo + per_slice);
  double A[kTsAcc];
#pragma unroll
  for (int k = 0; k < kTsAcc; ++k) A[k] = 0.0;
  for (int c0 = c_lo; c0 < c_hi; c0 += kTsTile) {
    __syncthreads();
    if (tid < kTsTile) {
      const int j = c0 + tid;
      s_meta[tid] = j < c_hi ? make_float4(y[2 * (size_t)j], y[2 * (size_t)j + 1], beta[j], logz[j]) : make_float4(0.f, 0.f, 0.f, INFINITY);
    }
    double acc[kTsTile];
    ts_tile_d2(acc, s_c, codes, ci, L, c0, c_hi, tid);      // (its barriers publish s_meta)
    float t[kTsAcc];
#pragma unroll
    for (int k = 0; k < kTsAcc; ++k) t[k] = 0.f;
#pragma unroll
    for (int ct = 0; ct < kTsTile; ++ct) {
      const float4 mj = s_meta[ct];
      const bool ok = (c0 + ct < c_hi) && (c0 + ct != i);
      const double d2 = acc[ct];
      const float p = ok ? (__expf((float)fma(-bi, d2, -lzi)) + __expf((float)fma(-(double)mj.z, d2, -(double)mj.w))) * inv2n : 0.f;
      const float dx = yi0 - mj.x, dy = yi1 - mj.y, tt = fmaf(dx, dx, dy * dy);
      const float w = ok ? __builtin_amdgcn_rcpf(1.f + tt) : 0.f;
      const float pw = p * w, w2 = w * w;
      t[0] = fmaf(pw, dx, t[0]);
      t[1] = fmaf(pw, dy, t[1]);
      t[2] = fmaf(w2, dx, t[2]);
      t[3] = fmaf(w2, dy, t[3]);
      t[4] += w;
      t[5] = fmaf(-p, log1pf(tt), t[5]);
      if (kPlogp) t[6] += p > 0.f ? p * logf(p) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kTsAcc; ++k) A[k] += (double)t[k];
  }
  if (live) {
    double* __restrict__ o = part + ((size_t)blockIdx.y * N + (size_t)i) * kTsAcc;
#pragma unroll
    for (int k = 0; k < kTsAcc; ++k) o[k] = A[k];
  }
}

// the slices' partial sums added in slice order: pt [E], part [ns][E]
__global__ __launch_bounds__(kTsBlock) void tsne_fold(double* __restrict__ pt, const double* __restrict__ part,
                                                      const unsigned long long E, const int ns) {
  const unsigned long long e = (unsigned long long)blockIdx.x * kTsBlock + threadIdx.x;
  if (e >= E) return;
  double r = 0.0;
  for (int s = 0; s < ns; ++s) r += part[(size_t)s * E + e];
  pt[e] = r;
}

// one block: Z, sum p ln w (and sum p ln p when this pass computed it) over the points in a fixed order, then the KL.
// stats: {Z, sum p ln w, KL, sum p ln p}
__global__ __launch_bounds__(kTsBlock) void tsne_reduce(const double* __restrict__ pt, const int N, const int with_plogp,
                                                        double* __restrict__ stats, float* __restrict__ kl_out,
                                                        float* __restrict__ stats_out) {
  __shared__ double s[3][kTsBlock];
  const int tid = threadIdx.x;
  double z = 0.0, a = 0.0, b = 0.0;
  for (int i = tid; i < N; i += kTsBlock) {
    const double* __restrict__ q = pt + (size_t)i * kTsAcc;
    z += q[4];
    a += q[5];
    b += q[6];
  }
  s[0][tid] = z;
  s[1][tid] = a;
  s[2][tid] = b;
  __syncthreads();
  for (int o = kTsBlock / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s[0][tid] += s[0][tid + o];
      s[1][tid] += s[1][tid + o];
      s[2][tid] += s[2][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double Z = s[0][0], spl = s[1][0], plogp = with_plogp ? s[2][0] : stats[3];
    const double kl = plogp - spl + log(Z);
    stats[0] = Z;
    stats[1] = spl;
    stats[2] = kl;
    stats[3] = plogp;
    if (kl_out) *kl_out = (float)kl;
    if (stats_out) {
      stats_out[0] = (float)Z;
      stats_out[1] = (float)spl;
      stats_out[2] = (float)kl;
      stats_out[3] = (float)plogp;
    }
  }
}

// grad [N][2] = 4 (alpha attr - rep / Z)
__global__ __launch_bounds__(kTsBlock) void tsne_grad(const double* __restrict__ pt, const double* __restrict__ stats, const int N,
                                                      const float alpha, float* __restrict__ grad) {
  const int e = (int)(blockIdx.x * kTsBlock + threadIdx.x);
  if (e >= 2 * N) return;
  const double* __restrict__ q = pt + (size_t)(e >> 1) * kTsAcc + (e & 1);
  grad[e] = (float)(4.0 * ((double)alpha * q[0] - q[2] / stats[0]));
}

// scikit-learn's _gradient_descent step over the 2 N elements, no recentring
__global__ __launch_bounds__(kTsBlock) void tsne_update(float* __restrict__ y, float* __restrict__ vel, float* __restrict__ gains,
                                                        const float* __restrict__ grad, const int n, const float momentum,
                                                        const float lr) {
  const int e = (int)(blockIdx.x * kTsBlock + threadIdx.x);
  if (e >= n) return;
  const float g = grad[e], v = vel[e];
  float gn = gains[e];
  gn = (v * g < 0.f) ? gn + 0.2f : gn * 0.8f;
  gn = fmaxf(gn, 0.01f);
  const float nv = momentum * v - lr * gn * g;
  gains[e] = gn;
  vel[e] = nv;
  y[e] += nv;
}

}  // namespace gmvae
