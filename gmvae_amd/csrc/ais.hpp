// gmvae_ais (include/gmvae_hip.h; host side: csrc/ais.hip): log p(x) by annealed importance sampling with Hamiltonian Monte Carlo
// transitions (Neal 2001; Wu, Burda, Salakhutdinov & Grosse 2017), the generative model alone.  The statement is tests/ais_ref.py.
//   Densities: p(z) = sum_k pi_k N(z; mu_k, diag sigma_k^2), the model's prior as a table (ais_prep builds it from `params`);
//   r_b(z) the base -- the prior, or the example's inference mixture as a caller's table of the same form --; log p(x|z) the
//   Bernoulli term of the decoder MLP.  f_t = r^(1 - beta_t) (p p(x|.))^beta_t.  With the prior as the base the path collapses to
//   p(z) p(x|z)^beta_t and the prior is evaluated once.  Both cases are ONE form here, two parts A and B with coefficients:
//     base = prior:    A = log p(z),   cA = 1;           B = log p(x|z),            cB = beta;   log w += dbeta * B
//     base = encoder:  A = log r_b(z), cA = 1 - beta;    B = log p(z) + log p(x|z), cB = beta;   log w += dbeta * (B - A)
//   and the chain keeps (z, grad A, grad B, A, B): grad log f_t at any t is cA gA + cB gB, so a transition costs n_leapfrog
//   evaluations and none at its start.
// One workgroup of 256 threads owns a PANEL of kAisRows = 16 chains for every temperature of the launch.  z, the momentum, the two
// gradients and the kept activations live in LDS; the chain's scalars (A, B, log w, eps, accept count) in registers, once per
// thread of the row.  No workgroup waits for another: no spins, no atomics; every sum has one owner and a fixed order, so two
// calls give the same bits, and a chain's result does not depend on which panel or launch it ran in.
//   Element-wise work: thread (row = tid / 16, j = tid % 16) owns elements l = j, j + 16, ... of its row; sums over L are an xor
//   tree over the 16 lanes of the row in fp64 (the same bits in every lane).
//   Layer products: v_mfma_f32_16x16x4_f32, the panel's 16 rows are the tile's rows, a wave takes output-column tiles w, w + 4, ...;
//   the A operand comes from LDS, the B operand (the weights) from global memory -- they stay in the L2, the decoder of the
//   default sizes is 217 KB --; two independent accumulators per tile (alternate groups of 4 contraction steps), added at the end.
//   The top layer runs in passes of kAisChunk = 128 output columns, so any D fits: lambda of the chunk, the row's Bernoulli sum
//   (fp32 terms, fp64 sums) and d lambda = x - sigmoid(lambda) into LDS, then the chunk's share of d h = d lambda W^T into
//   accumulators the waves keep across the passes.  The backward pass overwrites each kept activation a with d pre = (.) f'(a),
//   f' taken from the activation (ReLU' = 0 at a pre-activation <= 0).
//   The mixture parts: for each component the 16 lanes split L, the tree adds; a running logsumexp in fp64; the responsibilities
//   in LDS as doubles; the gradient sum_k r_k (mu_k - z) / sigma_k^2 per owned element.
// State between launches, and the "old" point of a transition, is the workspace's (z, gA, gB [n][L]; A, B, log w; eps; accepts):
// written at t = 0 and at every accept by the element's owner, re-read by the same thread on a reject; the workspace opens with
// the chains' accept records (one 64-bit word each: the tests hold the accept sequence to the statement with it).  A launch runs
// transitions t_lo .. t_hi; t = 0 is the start (component by inverse CDF, z_0 = mu_k + sigma_k eps) and shares the one evaluation
// call site.
// LDS at the largest admitted sizes (3 x 512 hidden, L = 128, K = 64): 150,016 bytes of the 160 KiB (ais_lds).
// The chain's state is fp32: a base whose sigma_kl lies below an ulp of mu_kl (6e-8 |mu|) is not resolved -- z_0 = fl(mu + sigma eps)
// is then mu itself and log r(z_0) is off by eps^2 / 2 per such dimension.  Trained encoders stay four orders above that; a
// diverged one (sigma = 2e-9) does not, and tests/test_inference_saturated.py holds such a case to the statement of an fp32 start.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "aux.hpp"

namespace gmvae {

constexpr int kAisRows = 16;
constexpr int kAisThreads = 256;
constexpr int kAisMaxHidden = 3, kAisMaxWidth = 512, kAisMaxL = 128, kAisMaxK = 64;
constexpr int kAisChunk = 128;            // top-layer output columns per pass: 8 tiles, 2 per wave
constexpr int kAisPad = 4;                // floats of padding per LDS row (row stride 4 mod 32 banks apart)
constexpr int kAisDhTiles = kAisMaxWidth / 16 / 4;      // d h tiles a wave keeps across the passes
constexpr float kAisStepMin = 1e-4f, kAisStepMax = 1.f;
constexpr unsigned kAisLdsLimit = 160u * 1024u;

typedef float ais_f4 __attribute__((ext_vector_type(4)));

struct AisArgs {
  int D, L, n_hidden, hidden[kAisMaxHidden], act;
  int C;                              // chains per example
  long long n;                        // chains: B C
  int enc;                            // base: 0 the prior, 1 the caller's table
  int Kp, Kb;
  const float* w[kAisMaxHidden + 1];  // decoder layers [in][out]
  const float* b[kAisMaxHidden + 1];
  float gen_bias;
  const float* gen_bias_vec;
  const unsigned char* x;
  const float* prior_lw; const double* prior_c; const float* prior_mu; const float* prior_sg;      // [Kp], [Kp], [Kp][L], [Kp][L]
  const float* base; const double* base_c;                                                        // records [B]; [B][Kb]
  const float* betas;                 // [T + 1]
  int T, t_lo, t_hi, n_leap;
  float step0, step_up, step_down;
  const float* eps; const float* u;   // [T + 1][n][L], [T + 1][n] or null: Philox
  unsigned long long row_base, seed, step;
  float* st_z; float* st_gA; float* st_gB;      // [n][L]
  double* st_d;                                  // [n][4]: A, B, log w, 0
  float* st_eps; int* st_acc;                    // [n]
  unsigned long long* st_bits;                   // [n]: bit t - 1 = transition t <= 64 was accepted (the workspace's first words)
  float* z_out;                                  // [n][L] or null
};

// floats of one caller's base record: ln w [Kb], mu [Kb][L], sigma [Kb][L]
__host__ __device__ inline long long ais_base_rec(int Kb, int L) { return (long long)Kb * (1 + 2 * L); }

struct AisLds {
  unsigned resp, red, z, p, gA, gB, h[kAisMaxHidden], dl, total;      // byte offsets
  int ldz, ldh[kAisMaxHidden], ldd;
};
__host__ __device__ inline AisLds ais_lds(int L, int n_hidden, const int* hidden) {
  AisLds s;
  unsigned o = 0;
  s.resp = o; o += kAisRows * kAisMaxK * sizeof(double);
  s.red = o; o += 4 * kAisRows * sizeof(double);
  s.ldz = L + kAisPad;
  const unsigned zb = kAisRows * s.ldz * sizeof(float);
  s.z = o; o += zb;
  s.p = o; o += zb;
  s.gA = o; o += zb;
  s.gB = o; o += zb;
  for (int i = 0; i < kAisMaxHidden; ++i) {
    s.ldh[i] = i < n_hidden ? hidden[i] + kAisPad : 0;
    s.h[i] = o;
    o += kAisRows * s.ldh[i] * sizeof(float);
  }
  s.ldd = kAisChunk + kAisPad;
  s.dl = o; o += kAisRows * s.ldd * sizeof(float);
  s.total = o;
  return s;
}

__device__ __forceinline__ float ais_act(const float h, const int act) {
  switch (act) {
    case 0: return fmaxf(h, 0.f);
    case 1: return tanhf(h);
    case 2: { const float e = expf(-fabsf(h)); return h >= 0.f ? 1.f / (1.f + e) : e / (1.f + e); }
    default: return h > 0.f ? h : expm1f(h);
  }
}
// f'(pre) from the activation a = f(pre)
__device__ __forceinline__ float ais_dact(const float a, const int act) {
  switch (act) {
    case 0: return a > 0.f ? 1.f : 0.f;
    case 1: return 1.f - a * a;
    case 2: return a * (1.f - a);
    default: return a > 0.f ? 1.f : a + 1.f;
  }
}

__device__ __forceinline__ double ais_row_sum(double v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// One [16 x 16] tile of A [16][Kd] (LDS, row stride lda) times the weights: columns n0 .. n0 + 15 of W [Kd][N] (TRANS = false:
// element (k, n) at W[k ldw + n]) or of W^T (TRANS = true: at W[n ldw + k]).  Lane (r = lane & 15, q = lane >> 4) gets rows
// 4 q .. 4 q + 3 of column n0 + r.  Whole groups of 16 contraction steps go four to a lane -- k = k0 + 4 q + s is step s's share of
// lane group q: one 16-byte LDS read of A and, for W^T, one 16-byte load of a row of W per four MFMAs -- where the rows are 16-byte
// aligned; the rest, and every ragged shape, goes one step at a time (k = k0 + q), steps and columns past the end contributing
// zero (their addresses are clamped).  Which path a step takes is a function of the sizes alone.
template <bool TRANS>
__device__ __forceinline__ ais_f4 ais_mm(const float* __restrict__ A, const int lda, const int Kd, const float* __restrict__ W,
                                         const int ldw, const int n0, const int N, const int lane) {
  const int r = lane & 15, q = lane >> 4;
  const bool n_ok = n0 + r < N;
  const int nc = n_ok ? n0 + r : N - 1;
  const float* __restrict__ a_row = A + r * lda;
  ais_f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int k0 = 0;
  if ((lda & 3) == 0 && (!TRANS || ((ldw & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0))) {
    for (; k0 + 16 <= Kd; k0 += 16) {
      const int k = k0 + 4 * q;
      const float4 a = *reinterpret_cast<const float4*>(a_row + k);
      float4 b;
      if (TRANS) {
        b = *reinterpret_cast<const float4*>(W + (long long)nc * ldw + k);
      } else {
        const float* __restrict__ wk = W + (long long)k * ldw + nc;
        b = make_float4(wk[0], wk[ldw], wk[2 * (long long)ldw], wk[3 * (long long)ldw]);
      }
      if (!n_ok) b = make_float4(0.f, 0.f, 0.f, 0.f);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc1, 0, 0, 0);
    }
  }
  for (; k0 < Kd; k0 += 8) {
    const int ka = k0 + q, kb = k0 + 4 + q;
    const bool oa = ka < Kd, ob = kb < Kd;
    const int kac = oa ? ka : Kd - 1, kbc = ob ? kb : Kd - 1;
    float a0 = a_row[kac], a1 = a_row[kbc];
    float b0 = TRANS ? W[(long long)nc * ldw + kac] : W[(long long)kac * ldw + nc];
    float b1 = TRANS ? W[(long long)nc * ldw + kbc] : W[(long long)kbc * ldw + nc];
    a0 = oa ? a0 : 0.f;
    a1 = ob ? a1 : 0.f;
    b0 = (oa && n_ok) ? b0 : 0.f;
    b1 = (ob && n_ok) ? b1 : 0.f;
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc1, 0, 0, 0);
  }
  return acc0 + acc1;
}

// ln sum_k exp(c_k - 1/2 |(z - mu_k) / sigma_k|^2) of the thread's row and its gradient into g (the owned elements).  Every
// thread of the block calls it (one barrier inside).
__device__ __forceinline__ double ais_mix(const double* __restrict__ cst, const float* __restrict__ mu, const float* __restrict__ sg,
                                          const int Kc, const int L, const float* zrow, double* resp_row, float* grow, const int j) {
  double m = -INFINITY, sum = 0.0;
  for (int k = 0; k < Kc; ++k) {
    double s = 0.0;
    for (int l = j; l < L; l += 16) {
      const float e = (zrow[l] - mu[k * L + l]) / sg[k * L + l];
      s += (double)(e * e);
    }
    const double c = cst[k] - 0.5 * ais_row_sum(s);
    if ((k & 15) == j) resp_row[k] = c;
    if (c > m) {
      sum = sum * exp(m - c) + 1.0;
      m = c;
    } else {
      sum += exp(c - m);
    }
  }
  const double lse = m + log(sum);
  for (int k = j; k < Kc; k += 16) resp_row[k] = exp(resp_row[k] - lse);
  __syncthreads();
  for (int l = j; l < L; l += 16) {
    const float zl = zrow[l];
    float g = 0.f;
    for (int k = 0; k < Kc; ++k) {
      const float s = sg[k * L + l];
      g += (float)resp_row[k] * ((mu[k * L + l] - zl) / s / s);
    }
    grow[l] = g;
  }
  return lse;
}

// A, B and their gradients at the panel's z (s.z) into s.gA, s.gB.  Every thread of the block calls it; it ends on a barrier.
__device__ __forceinline__ void ais_eval(const AisArgs& a, const AisLds& s, unsigned char* smem, const int tid, const int b_row,
                                         const int (&xb)[4], double& vA, double& vB) {
  const int lane = tid & 63, w = tid >> 6, row = tid >> 4, j = tid & 15, r = lane & 15, q = lane >> 4;
  float* const sz = reinterpret_cast<float*>(smem + s.z);
  float* const sgA = reinterpret_cast<float*>(smem + s.gA);
  float* const sgB = reinterpret_cast<float*>(smem + s.gB);
  float* const sdl = reinterpret_cast<float*>(smem + s.dl);
  double* const resp = reinterpret_cast<double*>(smem + s.resp) + row * kAisMaxK;
  double* const red = reinterpret_cast<double*>(smem + s.red);
  const int L = a.L;

  // ---- the mixture parts
  double vP = 0.0;
  if (a.enc) {
    const float* rec = a.base + (long long)b_row * ais_base_rec(a.Kb, L);
    vA = ais_mix(a.base_c + (long long)b_row * a.Kb, rec + a.Kb, rec + a.Kb + (long long)a.Kb * L, a.Kb, L, sz + row * s.ldz, resp,
                 sgA + row * s.ldz, j);
    __syncthreads();      // (resp is reused)
    vP = ais_mix(a.prior_c, a.prior_mu, a.prior_sg, a.Kp, L, sz + row * s.ldz, resp, sgB + row * s.ldz, j);
  } else {
    vA = ais_mix(a.prior_c, a.prior_mu, a.prior_sg, a.Kp, L, sz + row * s.ldz, resp, sgA + row * s.ldz, j);
    for (int l = j; l < L; l += 16) sgB[row * s.ldz + l] = 0.f;
  }

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

  // ---- top layer in passes of kAisChunk columns: the Bernoulli sums, d lambda, and d (top input) = d lambda W^T
  const float* const Wt = a.w[a.n_hidden];
  const float* const bt = a.b[a.n_hidden];
  const int D = a.D;
  double px[4] = {0.0, 0.0, 0.0, 0.0};
  ais_f4 dacc[kAisDhTiles];
#pragma unroll
  for (int i = 0; i < kAisDhTiles; ++i) dacc[i] = ais_f4{0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < D; c0 += kAisChunk) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n0 = c0 + (2 * w + i) * 16;
      if (n0 < D) {
        const ais_f4 acc = ais_mm<false>(in, ld_in, n_in, Wt, D, n0, D, lane);
        const int col = n0 + r;
        const bool ok = col < D;
        const float bias = ok ? bt[col] + (a.gen_bias_vec ? a.gen_bias_vec[col] : a.gen_bias) : 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float dlam = 0.f;
          if (ok) {
            const float lam = acc[v] + bias;
            const float xv = a.x[(long long)xb[v] * D + col] ? 1.f : 0.f;
            const float e = expf(-fabsf(lam));
            px[v] += (double)(xv * lam - (fmaxf(lam, 0.f) + log1pf(e)));
            dlam = xv - (lam >= 0.f ? 1.f / (1.f + e) : e / (1.f + e));
          }
          sdl[(4 * q + v) * s.ldd + (n0 - c0) + r] = dlam;
        }
      }
    }
    __syncthreads();
    const int kd = min(kAisChunk, D - c0);
#pragma unroll
    for (int i = 0; i < kAisDhTiles; ++i) {
      const int h0 = (w + 4 * i) * 16;
      if (h0 < n_in) dacc[i] += ais_mm<true>(sdl, s.ldd, kd, Wt + c0, D, h0, n_in, lane);
    }
    __syncthreads();
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    double t = px[v];
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) t += __shfl_xor(t, m);
    if (r == 0) red[w * kAisRows + 4 * q + v] = t;
  }
  // d (top input): times f' into the kept activation, or, with no hidden layer, added to B's gradient
  {
    float* const dst = a.n_hidden ? reinterpret_cast<float*>(smem + s.h[a.n_hidden - 1]) : sgB;
#pragma unroll
    for (int i = 0; i < kAisDhTiles; ++i) {
      const int h0 = (w + 4 * i) * 16;
      if (h0 < n_in && h0 + r < n_in) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float* const e = dst + (4 * q + v) * ld_in + h0 + r;
          *e = a.n_hidden ? dacc[i][v] * ais_dact(*e, a.act) : *e + dacc[i][v];
        }
      }
    }
  }
  __syncthreads();
  // ---- backward through the hidden layers
  for (int i = a.n_hidden - 1; i >= 0; --i) {
    const float* const dpre = reinterpret_cast<const float*>(smem + s.h[i]);
    const int N = i ? a.hidden[i - 1] : L;
    float* const dst = i ? reinterpret_cast<float*>(smem + s.h[i - 1]) : sgB;
    const int ldo = i ? s.ldh[i - 1] : s.ldz;
    for (int n0 = w * 16; n0 < N; n0 += 64) {
      const ais_f4 acc = ais_mm<true>(dpre, s.ldh[i], a.hidden[i], a.w[i], a.hidden[i], n0, N, lane);
      if (n0 + r < N) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float* const e = dst + (4 * q + v) * ldo + n0 + r;
          *e = i ? acc[v] * ais_dact(*e, a.act) : *e + acc[v];
        }
      }
    }
    __syncthreads();
  }
  vB = vP + (((red[row] + red[kAisRows + row]) + red[2 * kAisRows + row]) + red[3 * kAisRows + row]);
}

// eps (into dst, the row's LDS vector) and u of chain `chain` at transition t
__device__ __forceinline__ float ais_noise(const AisArgs& a, const long long chain, const int t, float* dst, const int j) {
  const int L = a.L;
  if (a.eps) {
    const float* src = a.eps + ((long long)t * a.n + chain) * L;
    for (int l = j; l < L; l += 16) dst[l] = src[l];
  } else {
    for (int qd = j; qd * 4 < L; qd += 16) {
      float o[4];
      noise_vals(a.row_base + (unsigned long long)chain, (uint32_t)qd, false, a.seed, a.step * (unsigned long long)(a.T + 1) + t, o);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (qd * 4 + i < L) dst[qd * 4 + i] = o[i];
    }
  }
  if (a.u) return a.u[(long long)t * a.n + chain];
  float o[4];
  noise_vals(a.row_base + (unsigned long long)chain, 0u, true, a.seed, a.step * (unsigned long long)(a.T + 1) + t, o);
  return o[0];
}

// Two waves per SIMD (256 registers): measured at the default sizes against one (306 registers, no spills: 1.60 x the time) and three
// (168 registers: 1.08 x) -- profiles/ais_notes.md.
__global__ __launch_bounds__(kAisThreads, 2) void ais_run(const AisArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
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
  if (a.t_lo > 0) {
    for (int l = j; l < L; l += 16) { zr[l] = wz[l]; gAr[l] = wA[l]; gBr[l] = wB[l]; }
    vA = a.st_d[chain * 4]; vB = a.st_d[chain * 4 + 1]; logw = a.st_d[chain * 4 + 2];
    step = a.st_eps[chain];
    nacc = a.st_acc[chain];
    bits = a.st_bits[chain];
  }
  for (int t = a.t_lo; t <= a.t_hi; ++t) {
    const float uacc = ais_noise(a, chain, t, pr, j);
    __syncthreads();
    const double beta = t ? (double)a.betas[t] : 0.0;
    const float cA = a.enc ? (float)(1.0 - beta) : 1.f, cB = (float)beta;
    const double vA0 = vA, vB0 = vB;
    double h_old = 0.0;
    if (t == 0) {
      // the start: a component of the base by inverse CDF, z_0 = mu_k + sigma_k eps
      const float* rec = a.enc ? a.base + (long long)b_row * ais_base_rec(a.Kb, L) : nullptr;
      const int Kc = a.enc ? a.Kb : a.Kp;
      const float* lw = a.enc ? rec : a.prior_lw;
      const float* mu = a.enc ? rec + a.Kb : a.prior_mu;
      const float* sg = a.enc ? rec + a.Kb + (long long)a.Kb * L : a.prior_sg;
      int k = Kc - 1;
      double cum = 0.0;
      for (int kk = 0; kk < Kc; ++kk) {
        cum += exp((double)lw[kk]);
        if ((double)uacc < cum) { k = kk; break; }
      }
      for (int l = j; l < L; l += 16) zr[l] = mu[k * L + l] + sg[k * L + l] * pr[l];
    } else {
      logw += (beta - (double)a.betas[t - 1]) * (a.enc ? vB - vA : vB);
      double ke = 0.0;
      for (int l = j; l < L; l += 16) ke += (double)(pr[l] * pr[l]);
      h_old = -((double)cA * vA + (double)cB * vB) + 0.5 * ais_row_sum(ke);
      for (int l = j; l < L; l += 16) {
        pr[l] += 0.5f * step * (cA * gAr[l] + cB * gBr[l]);
        zr[l] += step * pr[l];
      }
    }
    const int n_eval = t ? a.n_leap : 1;
    for (int i = 1; i <= n_eval; ++i) {
      __syncthreads();
      ais_eval(a, s, smem, tid, b_row, xb, vA, vB);
      if (t) {
        const float kick = i < n_eval ? step : 0.5f * step;
        for (int l = j; l < L; l += 16) {
          pr[l] += kick * (cA * gAr[l] + cB * gBr[l]);
          if (i < n_eval) zr[l] += step * pr[l];
        }
      }
    }
    bool keep = true;
    if (t) {
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
  }
  if (live) {
    if (j == 0) {
      a.st_d[chain * 4] = vA; a.st_d[chain * 4 + 1] = vB; a.st_d[chain * 4 + 2] = logw; a.st_d[chain * 4 + 3] = 0.0;
      a.st_eps[chain] = step;
      a.st_acc[chain] = nacc;
      a.st_bits[chain] = bits;
    }
    if (a.t_hi == a.T && a.z_out)
      for (int l = j; l < L; l += 16) a.z_out[chain * L + l] = zr[l];
  }
}

// ---- the prior table from `params`, and the constants c_k = ln w_k - sum_l ln sigma_kl - L/2 ln 2 pi of both tables.
// Block 0: the prior; block 1 + b: the constants of example b's base record.
struct AisPrep {
  int model, L, Kp, Kb;
  float raw_sigma_bias, sigma_min;
  const float* p0; const float* p1; const float* p2;      // VAE_GMP: loc, raw_scale_diag, mixture_logits; GMVAE: prior_gmm w, b
  float* lw; double* cst; float* mu; float* sg;
  const float* base; double* base_c;
};
__device__ __forceinline__ float ais_softplus(const float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

__global__ __launch_bounds__(kAisThreads) void ais_prep(const AisPrep a) {
  const double half_log_2pi = 0.91893853320467274178;
  const int L = a.L;
  if (blockIdx.x == 0) {
    for (int k = threadIdx.x; k < a.Kp; k += kAisThreads) {
      double lw = 0.0;
      if (a.model == 1) {
        double m = -INFINITY, sum = 0.0;
        for (int i = 0; i < a.Kp; ++i) m = fmax(m, (double)a.p2[i]);
        for (int i = 0; i < a.Kp; ++i) sum += exp((double)a.p2[i] - m);
        lw = (double)a.p2[k] - m - log(sum);
      } else if (a.model == 2) {
        lw = -log((double)a.Kp);
      }
      double ls = 0.0;
      for (int l = 0; l < L; ++l) {
        float mu = 0.f, sg = 1.f;
        if (a.model == 1) {
          mu = a.p0[k * L + l];
          sg = ais_softplus(a.p1[k * L + l]);
        } else if (a.model == 2) {
          mu = a.p0[k * 2 * L + l] + a.p1[l];
          sg = fmaxf(ais_softplus(a.p0[k * 2 * L + L + l] + a.p1[L + l] + a.raw_sigma_bias), a.sigma_min);
        }
        a.mu[k * L + l] = mu;
        a.sg[k * L + l] = sg;
        ls += log((double)sg);
      }
      a.lw[k] = (float)lw;
      a.cst[k] = (double)(float)lw - ls - (double)L * half_log_2pi;
    }
  } else {
    const long long b = blockIdx.x - 1;
    const float* rec = a.base + b * ais_base_rec(a.Kb, L);
    for (int k = threadIdx.x; k < a.Kb; k += kAisThreads) {
      const float* sg = rec + a.Kb + (long long)a.Kb * L + (long long)k * L;
      double ls = 0.0;
      for (int l = 0; l < L; ++l) ls += log((double)sg[l]);
      a.base_c[b * a.Kb + k] = (double)rec[k] - ls - (double)L * half_log_2pi;
    }
  }
}

// ---- per example: log w as floats, the bound, the chains' statistics; fin [B][4] keeps them in fp64 for the tail.  sign = 1: the
// lower bound of the forward chains (a product with 1.0 is exact: their bits are what they were); sign = -1: the upper bound
// -(logsumexp_c log w_rev - ln C) of the reverse chains (csrc/bdmc.hpp).
__global__ __launch_bounds__(kAisThreads) void ais_finish(const double* __restrict__ st_d, const float* __restrict__ st_eps,
                                                          const int* __restrict__ st_acc, const int B, const int C, const int T,
                                                          const double sign, float* __restrict__ logw_out, float* __restrict__ bound_out,
                                                          float* __restrict__ stats_out, double* __restrict__ fin) {
  const int b = blockIdx.x * kAisThreads + threadIdx.x;
  if (b >= B) return;
  const long long c0 = (long long)b * C;
  double m = -INFINITY;
  for (int c = 0; c < C; ++c) m = fmax(m, st_d[(c0 + c) * 4 + 2]);
  double s1 = 0.0, s2 = 0.0, se = 0.0;
  long long na = 0;
  for (int c = 0; c < C; ++c) {
    const double lw = st_d[(c0 + c) * 4 + 2];
    const double e = exp(lw - m);
    s1 += e; s2 += e * e;
    se += (double)st_eps[c0 + c];
    na += st_acc[c0 + c];
    if (logw_out) logw_out[c0 + c] = (float)lw;
  }
  const double bound = sign * (m + log(s1) - log((double)C)), ess = s1 * s1 / s2, acc = (double)na / ((double)C * (double)T), me = se / (double)C;
  if (bound_out) bound_out[b] = (float)bound;
  if (stats_out) {
    stats_out[b * 4] = (float)bound; stats_out[b * 4 + 1] = (float)ess; stats_out[b * 4 + 2] = (float)acc; stats_out[b * 4 + 3] = (float)me;
  }
  fin[b * 4] = -bound; fin[b * 4 + 1] = ess; fin[b * 4 + 2] = acc; fin[b * 4 + 3] = me;
}

// tail [8]: the sums over b of fin's four columns, B, zeros: one block, a strided pass per thread, then a fixed tree in LDS
__global__ __launch_bounds__(kAisThreads) void ais_tail(const double* __restrict__ fin, const int B, float* __restrict__ tail) {
  __shared__ double sh[4][kAisThreads];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < B; b += kAisThreads)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] += fin[b * 4 + i];
#pragma unroll
  for (int i = 0; i < 4; ++i) sh[i][threadIdx.x] = acc[i];
  __syncthreads();
  for (int n = kAisThreads / 2; n > 0; n >>= 1) {
    if ((int)threadIdx.x < n)
#pragma unroll
      for (int i = 0; i < 4; ++i) sh[i][threadIdx.x] += sh[i][threadIdx.x + n];
    __syncthreads();
  }
  if (threadIdx.x < 8) tail[threadIdx.x] = threadIdx.x < 4 ? (float)sh[threadIdx.x][0] : threadIdx.x == 4 ? (float)B : 0.f;
}

}  // namespace gmvae
