// GMVAE_LIK_*: the decoder's likelihood on grey-level bytes, t = x / 255 in [0, 1].  One-parameter exponential families
//   log p(t | lambda) = (t lambda - A(lambda)) / phi + c(t)          mean A'(lambda), gradient at the logits (A' - t) / phi
//   grey Bernoulli         A = softplus         A' = sigmoid                         phi = 1        c = 0   (no density on [0, 1])
//   continuous Bernoulli   A = log((e^l - 1)/l)  A' = 1/(1 - e^-l) - 1/l              phi = 1        c = 0
//   Gaussian, fixed sigma  A = l^2 / 2           A' = l                               phi = sigma^2  c = -t^2/(2 sigma^2) - ln sigma - ln(2 pi)/2
//   lik_rows   bytes -> t as fp32 [B][D]: what every network that reads x takes
//   lik_term   one element of the likelihood epilogue of gemm.hpp (EPI_LIK): its log-probability term and A' - t
//   lik_tail   tail[5] = sum_b mean_s sum_d (A' - t)^2 from the epilogue's squared-error partials, tail[6] = B D, tail[7] = 0
// One owner per output, fixed-order reductions, no atomics: eager and captured steps give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmvae {

enum { LIK_BERNOULLI = 0, LIK_GREY = 1, LIK_CB = 2, LIK_GAUSS = 3 };      // (GMVAE_LIK_* >> 11)

// t = b / 255, correctly rounded without a division: one Newton step on the product with the rounded reciprocal (255 / 255 is
// exactly 1, 0 exactly 0).  lik_rows and the epilogue share it: the networks and the likelihood see the same t.
__device__ __forceinline__ float lik_t(const unsigned b) {
  const float f = (float)b, r = 1.f / 255.f;
  const float q = f * r;
  return fmaf(fmaf(-q, 255.f, f), r, q);
}

// The per-workgroup constants of the Gaussian: 1 / sigma^2 and -ln sigma - ln(2 pi) / 2 from the workspace cell.
struct LikConst { float is2, cst; };
__device__ __forceinline__ LikConst lik_const(const int kind, const float* __restrict__ sigma) {
  LikConst k = {1.f, 0.f};
  if (kind == LIK_GAUSS) {
    const float s = *sigma;
    k.is2 = 1.f / (s * s);
    k.cst = -logf(s) - 0.918938533204672742f;
  }
  return k;
}
// Problem::lik carries two further bits beside the kind: the target is x itself as fp32 (GMVAE_X_F32), and the Gaussian's scale
// is per column and learned, sigma_d = exp(rho_d) (GMVAE_LIK_SCALE_LEARNED; liksig.hpp has rho's gradient)
enum { LIK_KIND_MASK = 3, LIK_RHO = 4, LIK_XF32 = 8 };
// ... the same two constants of one column from rho_d: exp(-2 rho) and -rho - ln(2 pi) / 2
__device__ __forceinline__ LikConst lik_const_rho(const float rho) {
  LikConst k;
  k.is2 = expf(-2.f * rho);
  k.cst = -rho - 0.918938533204672742f;
  return k;
}

// Continuous Bernoulli: (A, A') of one logit, no branch.
//   |l| < 1    the series in h = l / 2:  A = h + log(sinh h / h) = h + h^2/6 - h^4/180 + h^6/2835 - h^8/37800
//                                        A' = 1/2 + (coth h - 1/h) / 2 = 1/2 + (h/3 - h^3/45 + 2 h^5/945 - h^7/4725) / 2
//              (first dropped terms at |h| = 1/2: 2e-9 and 2e-8; both closed forms cancel there -- at l = 1e-3 the fp32 closed A'
//               is off by 1e-2, at l = 0 it is 0/0)
//   |l| >= 1   with a = |l|, e = exp(-a), om = 1 - e in [0.63, 1]:  A = max(l, 0) + log(om / a),  p = 1/om - 1/a (no
//              cancellation: 1/om >= 1 >= 1/a, the difference >= 0.58), A' = l > 0 ? p : 1 - p.  e flushes to 0 from a = 88:
//              A = max(l, 0) - log a, A' = 1 - 1/a or 1/a, both exact to rounding.
// The closed form's reciprocal and logarithm take max(a, 1): they stay finite where the series is chosen.
__device__ __forceinline__ void lik_cb(const float l, float& A, float& Ap) {
  const float h = 0.5f * l, h2 = h * h;
  const float As = h + h2 * fmaf(h2, fmaf(h2, fmaf(h2, -1.f / 37800.f, 1.f / 2835.f), -1.f / 180.f), 1.f / 6.f);
  const float Aps = fmaf(0.5f * h, fmaf(h2, fmaf(h2, fmaf(h2, -1.f / 4725.f, 2.f / 945.f), -1.f / 45.f), 1.f / 3.f), 0.5f);
  const float a = fmaxf(fabsf(l), 1.f);
  const float e = __builtin_amdgcn_exp2f(a * -1.44269504088896341f);
  const float om = 1.f - e, ra = __builtin_amdgcn_rcpf(a);
  const float Ac = fmaxf(l, 0.f) + __builtin_amdgcn_logf(om * ra) * 0.693147180559945309f;
  const float p = __builtin_amdgcn_rcpf(om) - ra;
  const float Apc = l > 0.f ? p : 1.f - p;
  const bool small = fabsf(l) < 1.f;
  A = small ? As : Ac;
  Ap = small ? Aps : Apc;
}

// One element: lp = (t l - A) / phi + c(t), df = A' - t (the caller scales the gradient by 1 / phi and squares df).
// The Gaussian term is written -(l - t)^2 / (2 sigma^2) + cst: the same number as (t l - l^2/2) / sigma^2 - t^2 / (2 sigma^2) + cst
// without the cancellation between its addends.
template <int KIND>
__device__ __forceinline__ void lik_term(const float l, const float t, const LikConst k, float& lp, float& df) {
  if constexpr (KIND == LIK_GREY) {
    const float e = __builtin_amdgcn_exp2f(fabsf(l) * -1.44269504088896341f);
    const float ope = 1.f + e, rcp = __builtin_amdgcn_rcpf(ope);
    lp = fmaf(t, l, -fmaxf(l, 0.f)) - __builtin_amdgcn_logf(ope) * 0.693147180559945309f;
    df = (l >= 0.f ? rcp : e * rcp) - t;
  } else if constexpr (KIND == LIK_CB) {
    float A, Ap;
    lik_cb(l, A, Ap);
    lp = fmaf(t, l, -A);
    df = Ap - t;
  } else {
    df = l - t;
    lp = fmaf(df * df, -0.5f * k.is2, k.cst);
  }
}

// A workgroup per example (grid-stride over b).  Rows that start 16-byte aligned in both buffers (D % 16 == 0 on aligned bases)
// go as 16-byte words of bytes -> four float4, every other shape byte by byte.
__global__ __launch_bounds__(256) void lik_rows(const unsigned char* __restrict__ x, float* __restrict__ tf, const int B, const int D) {
  const int t = threadIdx.x;
  const bool vec = (D & 15) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(tf)) & 15) == 0;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const long long o = (long long)b * D;
    if (vec) {
      const uint4* const x4 = reinterpret_cast<const uint4*>(x + o);
      float4* const o4 = reinterpret_cast<float4*>(tf + o);
      for (int i = t; i < (D >> 4); i += 256) {
        const uint4 xv = x4[i];
        const unsigned w[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o4[4 * i + j] = make_float4(lik_t(w[j] & 0xffu), lik_t((w[j] >> 8) & 0xffu), lik_t((w[j] >> 16) & 0xffu), lik_t(w[j] >> 24));
      }
    } else {
      for (int i = t; i < D; i += 256) tf[o + i] = lik_t(x[o + i]);
    }
  }
}

// One workgroup.  spart [B S][nparts]: the squared-error sums per row and column tile.  fp64 sums in a fixed order.
__global__ __launch_bounds__(1024) void lik_tail(const float* __restrict__ spart, const int nparts, float* __restrict__ tail,
                                                  const int B, const int S, const int D) {
  __shared__ double red[1024];
  const int t = threadIdx.x;
  double a5 = 0.;
  for (int b = t; b < B; b += 1024) {
    const float* const sp = spart + (long long)b * S * nparts;
    double h = 0.;
    for (long long i = 0; i < (long long)S * nparts; ++i) h += (double)sp[i];
    a5 += h / (double)S;
  }
  red[t] = a5;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) { tail[5] = (float)red[0]; tail[6] = (float)((double)B * (double)D); tail[7] = 0.f; }
}

}  // namespace gmvae
