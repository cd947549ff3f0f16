// gmvae_impute's kernels and their host launch functions (impute.hpp; the host path is iw_run in gmvae_hip.hip).  A translation
// unit -- and a device code object -- of its own: the training step's code object does not move (build_hip.py).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "aux.hpp"      // noise_vals
#include "impute.hpp"

namespace gmvae {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double im_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double im_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
// exp(v - m) of a log weight: a weight of exactly 0 (-inf) adds nothing, also while m is still -inf; a NaN stays one
__device__ __forceinline__ double im_wexp(const double v, const double m) {
  return v > -INFINITY ? exp(v - m) : (v == -INFINITY ? 0. : (double)NAN);
}
// (key, s) in front of (key2, s2): the larger key, ties to the lower s; a NaN key is in front of nothing
__device__ __forceinline__ bool im_better(const double k, const int s, const double k2, const int s2) {
  return k > k2 || (k == k2 && s < s2);
}

// A wave per batch row.  The chunk's samples s < n - s0 of rows_ws [B S][4] (.w = log w) and hid_s = the sum of hpart [b S + s][.]
// in ascending order, in fp64, into state [b] = (m, sum e, sum e^2, mh, sum exp(log w + hid - mh)) rescaled to the new maxima; the
// weights e_s = exp(log w_s - m) as fp32 to wgt, exp(m_old - m) to factor (0 on the first chunk), log w to logw_out [B][n].
// Draw j keeps argmax_s (log w_s + g_sj), g = -ln(-ln u), u = column 4 ceil(K / 4) + j of the u stream of Philox row
// (row0 + b) n + s0 + s: per lane over its samples in ascending s, then over the lanes, then against the key kept from the earlier
// chunks (strictly larger wins: ties go to the lower s); the winner's index and z go to the outputs.
__global__ __launch_bounds__(256) void impute_merge(const ImputeArgs a) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const int S = a.S, cnt = (int)min((unsigned long long)S, a.n - a.s0), np = a.nparts;
  const bool first = a.s0 == 0;
  const float* const rw = a.rows_ws + b * S * 4;
  const float* const hp = a.hpart ? a.hpart + b * S * np : nullptr;
  auto hid_of = [&](const int s) {
    double h = 0.;
    if (hp)
      for (int j = 0; j < np; ++j) h += (double)hp[(long long)s * np + j];
    return h;
  };
  double mx = -INFINITY, mhx = -INFINITY;
  for (int s = lane; s < cnt; s += 64) {
    const double lw = rw[4 * s + 3];
    mx = fmax(mx, lw);
    mhx = fmax(mhx, lw + hid_of(s));
  }
  mx = im_wave_max(mx); mhx = im_wave_max(mhx);
  double* const st = a.state + 8 * b;
  const double m_old = first ? -INFINITY : st[0], mh_old = first ? -INFINITY : st[3];
  const double m = fmax(m_old, mx), mh = fmax(mh_old, mhx);
  const double f = m_old > -INFINITY ? exp(m_old - m) : 0., fh = mh_old > -INFINITY ? exp(mh_old - mh) : 0.;
  double s1 = 0., s2 = 0., sh = 0.;
  for (int s = lane; s < cnt; s += 64) {
    const float lwf = rw[4 * s + 3];
    const double lw = lwf, e = im_wexp(lw, m);
    a.wgt[b * S + s] = (float)e;
    s1 += e; s2 += e * e;
    sh += im_wexp(lw + hid_of(s), mh);
    if (a.logw_out) a.logw_out[(unsigned long long)b * a.n + a.s0 + s] = lwf;
  }
  s1 = im_wave_sum(s1); s2 = im_wave_sum(s2); sh = im_wave_sum(sh);
  if (lane == 0) {
    st[1] = first ? s1 : st[1] * f + s1;
    st[2] = first ? s2 : st[2] * f * f + s2;
    st[4] = first ? sh : st[4] * fh + sh;
    st[0] = m; st[3] = mh;
    a.factor[b] = f;
  }
  if (a.M < 1 || (!a.draw_index_out && !a.draw_z_out)) return;
  const unsigned qK = (unsigned)(a.K + 3) / 4;
  const unsigned long long prow = (a.row0 + (unsigned long long)b) * a.n + a.s0;
  for (int q = 0; q < (a.M + 3) / 4; ++q) {
    double key[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bs[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    for (int s = lane; s < cnt; s += 64) {
      float u[4];
      noise_vals(prow + s, qK + q, true, a.seed, a.step, u);
      const double lw = rw[4 * s + 3];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double k = lw - log(-log((double)u[j]));
        if (im_better(k, s, key[j], bs[j])) { key[j] = k; bs[j] = s; }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (4 * q + j >= a.M) break;                 // (wave-uniform)
      double k = key[j];
      int s = bs[j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double k2 = __shfl_xor(k, o, 64);
        const int s2 = __shfl_xor(s, o, 64);
        if (im_better(k2, s2, k, s)) { k = k2; s = s2; }
      }
      if (s == INT_MAX) { s = 0; k = -INFINITY; }  // (every key a NaN: the chunk's first sample)
      const long long slot = b * a.M + 4 * q + j;
      if (!first && !(k > a.keys[slot])) continue;  // (wave-uniform: every lane read the same key; its writer is below, behind the read)
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) {
        a.keys[slot] = k;
        if (a.draw_index_out) a.draw_index_out[slot] = (long long)(a.s0 + (unsigned long long)s);
      }
      if (a.draw_z_out)
        for (int l = lane; l < a.L; l += 64) a.draw_z_out[slot * a.L + l] = a.z[(b * S + s) * a.L + l];
    }
  }
}

// acc[b][col0 .. col0 + 63] of one batch row and one 64-column tile of W.  Wave w takes the 16-row blocks w, w + 4, ... of the
// chunk's samples and all four 16-column MFMA tiles: A = h rows (a 16-byte load per lane and 16 k), B = the tile of W from LDS in
// the order the loads of A give k -- lane (lk, ln), element j: k = 16 kq + 4 lk + j --, lambda = the product + c; each lane adds
// e_s sigmoid(lambda_s) of its four rows of a block in fp32 and the block's sum to an fp64 partial per tile.  Rows at or past the chunk's count are predicated off in the
// loads and in the epilogue (the last chunk's unused rows hold stale values).  The partials meet over lk by two lane exchanges,
// then over the waves in the order 0 .. 3 in LDS; thread col < 64 -- the one owner of (b, col0 + col) -- writes the accumulator.
// kStage = false (H > kImputeLdsRows): the same with B read from global memory.
template <bool kStage>
__global__ __launch_bounds__(256) void impute_fold(const ImputeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_w[];      // [KQ][4][64][4]; afterwards the waves' partials [4][64] fp64
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 15, lk = lane >> 4;
  const int H = a.H, D = a.D, S = a.S, KQ = (H + 15) / 16;
  const int tiles = (D + kImputeTile - 1) / kImputeTile;
  const long long b = blockIdx.x / tiles;
  const int col0 = (int)(blockIdx.x % tiles) * kImputeTile;
  const int cnt = (int)min((unsigned long long)S, a.n - a.s0);
  const float* __restrict__ W = a.W;
  if (kStage) {
    for (int e = tid; e < KQ * 16 * kImputeTile; e += 256) {
      const int k = e >> 6, c = e & 63;
      const float v = (k < H && col0 + c < D) ? W[(long long)k * D + col0 + c] : 0.f;
      s_w[((((k >> 4) * 4 + ((k >> 2) & 3)) * kImputeTile + c) << 2) + (k & 3)] = v;
    }
    __syncthreads();
  }
  float cb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int col = col0 + 16 * t + ln;
    cb[t] = col < D ? (a.bias[col] + a.bias_const) + (a.bias2 ? a.bias2[col] : 0.f) : 0.f;
  }
  double part[4] = {0., 0., 0., 0.};
  const float* const hb = a.h + b * S * H;
  const float* const wg = a.wgt + b * S;
  const bool hvec = (H & 3) == 0 && (reinterpret_cast<uintptr_t>(a.h) & 15) == 0;
  const int nblk = (cnt + 15) / 16;
  for (int blk = wave; blk < nblk; blk += 4) {
    const int s = blk * 16 + ln;
    const bool live = s < cnt;
    const float* const hr = hb + (long long)(live ? s : 0) * H;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kq = 0; kq < KQ; ++kq) {
      const int k = 16 * kq + 4 * lk;
      float4 av = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live) {
        if (hvec) {
          if (k < H) av = *reinterpret_cast<const float4*>(hr + k);
        } else {
          if (k < H) av.x = hr[k];
          if (k + 1 < H) av.y = hr[k + 1];
          if (k + 2 < H) av.z = hr[k + 2];
          if (k + 3 < H) av.w = hr[k + 3];
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float4 bv;
        if (kStage) {
          bv = *reinterpret_cast<const float4*>(s_w + (((kq * 4 + lk) * kImputeTile + 16 * t + ln) << 2));
        } else {
          const int col = col0 + 16 * t + ln;
          const bool c_ok = col < D;
          bv.x = (c_ok && k < H) ? W[(long long)k * D + col] : 0.f;
          bv.y = (c_ok && k + 1 < H) ? W[(long long)(k + 1) * D + col] : 0.f;
          bv.z = (c_ok && k + 2 < H) ? W[(long long)(k + 2) * D + col] : 0.f;
          bv.w = (c_ok && k + 3 < H) ? W[(long long)(k + 3) * D + col] : 0.f;
        }
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[t], 0, 0, 0);
      }
    }
    // the block's four rows of a lane in fp32 (weights and sigmoids in [0, 1]: four terms), then one fp64 add per tile; sigmoid
    // on the hardware exp and reciprocal (1 ulp each; exp(-lambda) = inf gives exactly 0, 0 gives exactly 1)
    float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int sr = blk * 16 + lk * 4 + r;        // the row of acc[.][r]
      if (sr < cnt) {
        const float w = wg[sr];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float lam = acc[t][r] + cb[t];
          const float p = __builtin_amdgcn_rcpf(1.f + __expf(-lam));
          ps[t] = fmaf(w, p, ps[t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) part[t] += (double)ps[t];
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    part[t] += __shfl_xor(part[t], 16, 64);
    part[t] += __shfl_xor(part[t], 32, 64);
  }
  double* const s_red = reinterpret_cast<double*>(s_w);
  __syncthreads();                                 // (every wave has read its last B operand)
  if (lk == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) s_red[wave * kImputeTile + 16 * t + ln] = part[t];
  }
  __syncthreads();
  if (tid < kImputeTile && col0 + tid < D) {
    const double tot = ((s_red[tid] + s_red[kImputeTile + tid]) + s_red[2 * kImputeTile + tid]) + s_red[3 * kImputeTile + tid];
    double* const p = a.acc + b * (long long)((D + 3) / 4 * 4) + col0 + tid;
    *p = a.s0 == 0 ? tot : *p * a.factor[b] + tot;
  }
}

// thread e = b D + d: mean [b][d] = acc / sum e as fp32; the thread of d = 0 also writes the row's stats [4] = (bound -- iw_merge's --,
// ESS = (sum e)^2 / sum e^2, cond_loglik = (mh + ln sum_h) - (m + ln sum e) -- exactly 0 for a row with nothing missing --, the
// largest normalised weight 1 / sum e) and slots [4] = (-bound, ESS, cond_loglik, the row's missing pixels) for iw_tail.  A row
// without a positive finite sum of weights (all -inf, or a NaN) gives NaN in mean, ESS, cond_loglik and the largest weight.
__global__ __launch_bounds__(256) void impute_finish(const ImputeArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)a.B * a.D) return;
  const long long b = e / a.D;
  const int d = (int)(e - b * a.D);
  const double* const st = a.state + 8 * b;
  const double s1 = st[1];
  const bool ok = s1 > 0. && s1 < INFINITY;
  if (a.mean_out) a.mean_out[e] = ok ? (float)(a.acc[b * (long long)((a.D + 3) / 4 * 4) + d] / s1) : NAN;
  if (d != 0) return;
  const float missing = a.mcnt ? a.mcnt[2 * b] : 0.f;
  const float bound = a.bound[b];
  float ess = NAN, cond = NAN, wmax = NAN;
  if (ok) {
    ess = (float)(s1 * s1 / st[2]);
    cond = missing == 0.f ? 0.f : (float)((st[3] + log(st[4])) - (st[0] + log(s1)));
    wmax = (float)(1. / s1);
  }
  if (a.stats_out) *reinterpret_cast<float4*>(a.stats_out + 4 * b) = make_float4(bound, ess, cond, wmax);
  *reinterpret_cast<float4*>(a.slots + 4 * b) = make_float4(-bound, ess, cond, missing);
}

}  // namespace

int impute_launch_merge(hipStream_t st, const ImputeArgs& a) {
  hipLaunchKernelGGL(impute_merge, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int impute_launch_fold(hipStream_t st, const ImputeArgs& a) {
  const int tiles = (a.D + kImputeTile - 1) / kImputeTile, KQ = (a.H + 15) / 16;
  const dim3 grid((unsigned)((long long)a.B * tiles));
  if (a.H <= kImputeLdsRows) {
    const size_t lds = (size_t)KQ * 16 * kImputeTile * sizeof(float);      // (>= the 2 KiB of the waves' partials)
    hipLaunchKernelGGL(impute_fold<true>, grid, dim3(256), lds < 2048 ? 2048 : lds, st, a);
  } else {
    hipLaunchKernelGGL(impute_fold<false>, grid, dim3(256), 2048, st, a);
  }
  return (int)hipGetLastError();
}

int impute_launch_finish(hipStream_t st, const ImputeArgs& a) {
  hipLaunchKernelGGL(impute_finish, dim3((unsigned)(((long long)a.B * a.D + 255) / 256)), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace gmvae
