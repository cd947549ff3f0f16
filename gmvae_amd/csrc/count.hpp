// GMVAE_LIK_POISSON / GMVAE_LIK_NEG_BINOMIAL: the decoder's likelihood on counts, x fp32 [B][D] >= 0 (GMVAE_X_F32), lambda the
// LOG-mean.  Every network reads t = log1p(x); the likelihood's target is x itself.
//   Poisson             log p = x l - exp(l) - lgamma(x + 1)                                  g = exp(l) - x
//   negative binomial   log p = lgamma(x + r) - lgamma(r) - lgamma(x + 1) - x sp(-u) - r sp(u)   g = (r + x) sigmoid(u) - x
//                       r_d = exp(rho_d), u = l - rho_d, sp = softplus;  d log p / d rho = r (psi(x + r) - psi(r) - sp(u)) + g
// The terms that do not depend on lambda are per (b, d), not per row: count_rows sums them once per example in fp64 --
//   c_b = sum_d [lgamma(x + r_d) - lgamma(r_d)] - lgamma(x + 1)      (the bracket under the negative binomial alone)
// -- and the epilogue adds c_b to each of the example's S rows.  So no lgamma runs in the R D epilogue (it would be recomputed S
// times, and an fp64 lgamma inside gemm_grouped would set the register count of every instance of that kernel), and the
// difference lgamma(x + r) - lgamma(r) is an fp64 difference: 0 exactly at x = 0, 1e-12 at r = e^8.
//   count_rows           one read of x: t = log1p(x) as fp32 [B][D] and c [B]
//   count_term           one element of the likelihood epilogue of gemm.hpp (EPI_LIK with LIK_POIS / LIK_NB): the lambda-dependent
//                        part of log p, g, sp(u) and softplus(l) - log1p(x) (tail[5]: the mean's error on the scale the networks see)
//   count_disp_partial / count_disp_finish   rho's gradient, shaped like liksig.hpp's pair: a row-weighted column reduction in fp64
//                        over the stored g and sp(u) planes, then the slab partials in index order into slab 0 of rho's range
// One owner per output, fixed-order sums, no atomics: eager, captured and data-parallel steps give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmvae {

// Problem::lik beside LIK_XF32 (the kind field is 0): which count likelihood the epilogue evaluates
enum { LIK_POIS = 16, LIK_NB = 32, LIK_COUNT = LIK_POIS | LIK_NB };

// softplus(v) = max(v, 0) + log1p(exp(-|v|)): finite for every finite v
__device__ __forceinline__ float count_sp(const float v) { return fmaxf(v, 0.f) + log1pf(expf(-fabsf(v))); }

// One element.  lp: log p without the terms of c_b; g: d(-log p) / d lambda; spu: sp(u) (the negative binomial's, what rho's
// gradient reads); df: softplus(l) - log1p(x) = log1p(mean) - t.
//   NB: sigmoid(u) and 1 - sigmoid(u) both from a = exp(-|u|), so g = r sigmoid(u) - x (1 - sigmoid(u)) loses nothing at either
//   end, and lambda is never exponentiated alone: finite for every finite l and rho.
template <bool NB>
__device__ __forceinline__ void count_term(const float l, const float x, const float rho, const float r, float& lp, float& g,
                                           float& spu, float& df) {
  df = count_sp(l) - log1pf(x);
  if constexpr (NB) {
    const float u = l - rho;
    const float a = expf(-fabsf(u)), l1 = log1pf(a), s = 1.f / (1.f + a);
    spu = fmaxf(u, 0.f) + l1;
    const float spm = fmaxf(-u, 0.f) + l1;                       // sp(-u)
    const float sg = u >= 0.f ? s : a * s, om = u >= 0.f ? a * s : s;      // sigmoid(u), 1 - sigmoid(u)
    lp = -fmaf(x, spm, r * spu);
    g = fmaf(r, sg, -x * om);
  } else {
    const float e = expf(l);                                     // (no clamp: l > 88 gives inf, a step GMVAE_OPT_CLIP_NORM skips)
    spu = 0.f;
    lp = fmaf(x, l, -e);
    g = e - x;
  }
}

// digamma in fp64: the recurrence psi(v) = psi(v + 1) - 1 / v up to an argument >= 6, then the asymptotic series
//   psi(v) ~ ln v - 1/(2v) - 1/(12 v^2) + 1/(120 v^4) - 1/(252 v^6) + 1/(240 v^8) - 1/(132 v^10) + 691/(32760 v^12)
// (v > 0; the first dropped term is 1/(12 v^14): 1e-12 at v = 6)
__host__ __device__ inline double count_digamma(double v) {
  double s = 0.0;
  while (v < 6.0) { s -= 1.0 / v; v += 1.0; }
  const double i = 1.0 / v, i2 = i * i;
  const double ser = i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0 - i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0 - i2 * (691.0 / 32760.0))))));
  return s + log(v) - 0.5 * i - ser;
}

// c's addend of one element: -lgamma(x + 1), and lgamma(x + r) - lgamma(r) under the negative binomial (r = exp(rho) in fp64)
template <bool NB>
__device__ __forceinline__ double count_const(const float x, const double r) {
  double c = -lgamma((double)x + 1.0);
  if constexpr (NB) c += (x > 0.f) ? lgamma((double)x + r) - lgamma(r) : 0.0;
  return c;
}

// A workgroup per example (grid-stride over b), 256 threads.  Rows that start 16-byte aligned in both buffers (D % 4 == 0 on
// aligned bases) go as float4, every other shape float by float.  Each thread sums its elements in index order in fp64; the 256
// sums meet in a fixed tree through LDS.  rho: [D] under the negative binomial, else null.
__global__ __launch_bounds__(256) void count_rows(const float* __restrict__ x, const float* __restrict__ rho, float* __restrict__ tf,
                                                  float* __restrict__ c, const int B, const int D) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const bool vec = (D & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(tf)) & 15) == 0;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const long long o = (long long)b * D;
    double acc = 0.0;
    if (vec) {
      const float4* const x4 = reinterpret_cast<const float4*>(x + o);
      float4* const o4 = reinterpret_cast<float4*>(tf + o);
      for (int i = t; i < (D >> 2); i += 256) {
        const float4 xv = x4[i];
        o4[i] = make_float4(log1pf(xv.x), log1pf(xv.y), log1pf(xv.z), log1pf(xv.w));
        const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += rho ? count_const<true>(xe[j], exp((double)rho[4 * i + j])) : count_const<false>(xe[j], 0.0);
      }
    } else {
      for (int i = t; i < D; i += 256) {
        const float xv = x[o + i];
        tf[o + i] = log1pf(xv);
        acc += rho ? count_const<true>(xv, exp((double)rho[i])) : count_const<false>(xv, 0.0);
      }
    }
    red[t] = acc;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
      if (t < k) red[t] += red[t + k];
      __syncthreads();
    }
    if (t == 0) c[b] = (float)red[0];
    __syncthreads();
  }
}

// ---- rho's gradient:  d loss / d rho_d = -sum_r rw_r { r_d [psi(x_bd + r_d) - psi(r_d) - sp(u_rd)] + g_rd },  b = r / S
constexpr int kCdCols = 64, kCdRowLanes = 16;

__device__ __forceinline__ double count_disp_term(const float x, const float g, const float sp, const double r, const double psr) {
  const double dps = (x > 0.f) ? count_digamma((double)x + r) - psr : 0.0;
  return -(r * (dps - (double)sp) + (double)g);
}

// grid (ceil(D / 64), slabs), 256 threads: 16 row lanes x 16 column quads (liksig_partial's shape; liksig_slab_rows /
// liksig_slabs size the slabs).  Dp = pad4(D): part's row length.  part is fp64: the addends of one column cancel where the
// model fits (mean ~ x), so the sums stay in fp64 until count_disp_finish rounds once.
__global__ __launch_bounds__(256) void count_disp_partial(const float* __restrict__ g, const float* __restrict__ sp, const float* __restrict__ x,
                                                          const float* __restrict__ rw, const float* __restrict__ rho,
                                                          double* __restrict__ part, const int R, const int D, const int Dp,
                                                          const int rs, const int S) {
  __shared__ double red[kCdRowLanes][kCdCols + 2];
  const int tid = threadIdx.x, c4 = tid % (kCdCols / 4), rr = tid / (kCdCols / 4);
  const int nb = blockIdx.x * kCdCols + 4 * c4;
  const int r0 = blockIdx.y * rs, r1 = (R - r0 < rs) ? R : r0 + rs;      // (r0 < R: the grid has ceil(R / rs) slabs)
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (nb < D) {
    double rd[4], psr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { rd[j] = exp((double)rho[nb + j < D ? nb + j : D - 1]); psr[j] = count_digamma(rd[j]); }
    const bool vec = (D & 3) == 0 && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(sp) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
    for (int r = r0 + rr; r < r1; r += kCdRowLanes) {
      const long long o = (long long)r * D + nb, ox = (long long)(r / S) * D + nb;
      const double wr = rw ? (double)rw[r] : 1.0;
      if (vec) {                                                           // (every row quad starts 16-byte aligned and lies inside D)
        const float4 gv = *reinterpret_cast<const float4*>(g + o), sv = *reinterpret_cast<const float4*>(sp + o);
        const float4 xv = *reinterpret_cast<const float4*>(x + ox);
        acc[0] += wr * count_disp_term(xv.x, gv.x, sv.x, rd[0], psr[0]);
        acc[1] += wr * count_disp_term(xv.y, gv.y, sv.y, rd[1], psr[1]);
        acc[2] += wr * count_disp_term(xv.z, gv.z, sv.z, rd[2], psr[2]);
        acc[3] += wr * count_disp_term(xv.w, gv.w, sv.w, rd[3], psr[3]);
      } else {                                                             // (the scalar path: any D, any alignment)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (nb + j < D) acc[j] += wr * count_disp_term(x[ox + j], g[o + j], sp[o + j], rd[j], psr[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[rr][4 * c4 + j] = acc[j];
  __syncthreads();
  if (tid < kCdCols) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < kCdRowLanes; ++k) t += red[k][tid];
    const int n = blockIdx.x * kCdCols + tid;
    if (n < Dp) part[(long long)blockIdx.y * Dp + n] = n < D ? t : 0.0;
  }
}

// slabs: the gradient buffer's split-K slabs [ns][P]; off: rho's offset in a slab.
__global__ __launch_bounds__(256) void count_disp_finish(const double* __restrict__ part, const int nslab, float* __restrict__ slabs,
                                                         const long long P, const int ns, const long long off, const int Dp) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= Dp) return;
  double t = 0.0;
  for (int s = 0; s < nslab; ++s) t += part[(long long)s * Dp + n];
  slabs[off + n] = (float)t;
  for (int k = 1; k < ns; ++k) slabs[(long long)k * P + off + n] = 0.f;
}

}  // namespace gmvae
