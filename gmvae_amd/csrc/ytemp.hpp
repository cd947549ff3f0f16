// The Gumbel-softmax head under GmvaeDims::sched_flags & (GMVAE_Y_TEMP_DEV | GMVAE_Y_STRAIGHT_THROUGH):
//   GMVAE_Y_TEMP_DEV          the temperature T is READ FROM DEVICE MEMORY (one float of the workspace's "y_temperature" slots), so
//                             that the steps of one captured graph can anneal it; 1 / T is formed as the host forms it (one
//                             correctly rounded division): a slot holding the float of dims->temperature gives the same bits
//   GMVAE_Y_STRAIGHT_THROUGH  the step consumes y_hard = e_{argmax_k (logits_bk + g_rk)} (lowest index on ties; the argmax does
//                             not depend on T) and keeps the relaxed sample y_soft = softmax_k((logits_bk + g_rk) / T) for the
//                             backward: da = y_soft (dy - y_soft . dy), autograd of y = y_soft + stopgrad(y_hard - y_soft)
// The kernels here stand where y_head_fwd, y_head_bwd and y_head_bwd_w (kernels.hpp, wobj.hpp) stand in the general schedule, with
// their three K regimes, their operations and their summation order: without GMVAE_Y_STRAIGHT_THROUGH they give those kernels' bits.
// `tau` null: T by value (invT), as those kernels take it.  Fixed summation orders, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace gmvae {

// 1 / T of the step: the slot's (read by every thread: one scalar load per row), or the host's
__device__ __forceinline__ float ytemp_inv(const float* __restrict__ tau, const float invT) {
  return tau ? 1.f / tau[0] : invT;
}

// y_head_fwd (kernels.hpp) with T from `tau` and, with y_soft given (straight-through), y = the one-hot row at the argmax of the
// perturbed logits and y_soft = the relaxed sample.  One wave per row r (four rows per wave at K <= 16).
__global__ void y_head_fwd_t(const float* __restrict__ logits, const float* __restrict__ u, const float* __restrict__ tau,
                             float* __restrict__ y, float* __restrict__ y_soft, float* __restrict__ nent, int R, int S, int K,
                             float invT0) {
  const float invT = ytemp_inv(tau, invT0);
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  if (K <= 16) {
    const int sub = lane >> 4, k = lane & 15;
    for (long long r4 = ((long long)blockIdx.x * wpb + (threadIdx.x >> 6)) * 4; r4 < R; r4 += (long long)gridDim.x * wpb * 4) {
      const long long r = r4 + sub;
      const bool rv = r < R, kv = rv && k < K;
      const long long rc = rv ? r : R - 1;
      const int b = (int)(rc / S);
      const float lgk = k < K ? logits[(long long)b * K + k] : 0.f;
      const float p = kv ? lgk + -logf(-logf(u[rc * K + k])) : -INFINITY;      // the perturbed logit, before 1 / T
      const float a = kv ? p * invT : -INFINITY;
      float mx = a;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 16));
      float se = kv ? expf(a - mx) : 0.f;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) se += __shfl_xor(se, o, 16);
      const float lse = mx + logf(se);
      if (y_soft) {
        float pm = p;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) pm = fmaxf(pm, __shfl_xor(pm, o, 16));
        int am = (kv && p == pm) ? k : 16;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o, 16));
        if (kv) {
          y_soft[r * K + k] = expf(a - lse);
          y[r * K + k] = k == am ? 1.f : 0.f;
        }
      } else if (kv) {
        y[r * K + k] = expf(a - lse);
      }
      // once per x (the row of its first sample): entropy of q(y|x)
      const float lga[1] = {k < K ? lgk : -INFINITY};
      float lpa[1];
      cat_log_softmax<Sub16, 1, true>(lga, lpa);
      const float lp = lpa[0];
      float ne = k < K ? expf(lp) * lp : 0.f;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) ne += __shfl_xor(ne, o, 16);
      if (rv && k == 0 && r == (long long)b * S) nent[b] = ne;
    }
    return;
  }
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < R; r += gridDim.x * wpb) {
    const int b = r / S;
    const float* lg = logits + (long long)b * K;
    if (K <= 64) {
      const bool kv = lane < K;
      const float p = kv ? lg[lane] + -logf(-logf(u[(long long)r * K + lane])) : -INFINITY;
      const float a = kv ? p * invT : -INFINITY;
      const float mx = wave_max(a);
      const float se = wave_sum(kv ? expf(a - mx) : 0.f);
      const float lse = mx + logf(se);
      if (y_soft) {
        const float pm = wave_max(p);
        const int am = -(int)wave_max((kv && p == pm) ? (float)-lane : -64.f);      // the lowest lane at the maximum
        if (kv) {
          y_soft[(long long)r * K + lane] = expf(a - lse);
          y[(long long)r * K + lane] = lane == am ? 1.f : 0.f;
        }
      } else if (kv) {
        y[(long long)r * K + lane] = expf(a - lse);
      }
    } else {
    float mx = -INFINITY;
    for (int k = lane; k < K; k += 64) {
      const float g = -logf(-logf(u[(long long)r * K + k]));
      mx = fmaxf(mx, (lg[k] + g) * invT);
    }
    mx = wave_max(mx);
    float se = 0.f;
    for (int k = lane; k < K; k += 64) {
      const float g = -logf(-logf(u[(long long)r * K + k]));
      se += expf((lg[k] + g) * invT - mx);
    }
    se = wave_sum(se);
    const float lse = mx + logf(se);
    if (y_soft) {
      float pm = -INFINITY;
      int ak = K;                                  // (a lane walks its k upwards: the first at its maximum stays)
      for (int k = lane; k < K; k += 64) {
        const float p = lg[k] + -logf(-logf(u[(long long)r * K + k]));
        if (p > pm) { pm = p; ak = k; }
      }
      const float pw = wave_max(pm);
      // (k < 2^24: exact as a float)
      const int am = -(int)wave_max((ak < K && pm == pw) ? (float)-ak : -(float)K);
      for (int k = lane; k < K; k += 64) {
        const float g = -logf(-logf(u[(long long)r * K + k]));
        y_soft[(long long)r * K + k] = expf((lg[k] + g) * invT - lse);
        y[(long long)r * K + k] = k == am ? 1.f : 0.f;
      }
    } else {
    for (int k = lane; k < K; k += 64) {
      const float g = -logf(-logf(u[(long long)r * K + k]));
      y[(long long)r * K + k] = expf((lg[k] + g) * invT - lse);
    }
    }
    }
    if (r == b * S) {       // once per x: entropy of q(y|x)
      float m2, l2;
      row_lse_parts(lg, K, lane, m2, l2);
      float ne = 0.f;
      for (int k = lane; k < K; k += 64) {
        const float lp = (lg[k] - m2) - l2;
        ne += expf(lp) * lp;
      }
      ne = wave_sum(ne);
      if (lane == 0) nent[b] = ne;
    }
  }
}

// y_head_bwd (W = false) / y_head_bwd_w (W = true: the entropy term under beta_y a_b, wts and act as wobj.hpp's) with T from `tau`:
//   dlogits_b = sum_s ys (dy - ys . dy) / T + [beta_y a_b] pi (log pi - nent_b)
// ys = the relaxed sample: the workspace's "y" without GMVAE_Y_STRAIGHT_THROUGH, its "y_soft" under it (dy is then the data
// gradient at y_hard).  Both of y_head_bwd's paths with its operations in its order.
template <bool W>
__global__ __launch_bounds__(512) void y_head_bwd_t(const float* __restrict__ logits, const float* __restrict__ ys_,
                                                    const float* __restrict__ dy, const float* __restrict__ nent,
                                                    const float* __restrict__ wts, const float* __restrict__ act,
                                                    const float* __restrict__ tau, float* __restrict__ dlogits, int B, int S,
                                                    int K, float invT0) {
  __shared__ float red[8][64];
  const float invT = ytemp_inv(tau, invT0);
  const float* __restrict__ y = ys_;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float by = 0.f;
  if (W) by = wts[1];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* lg = logits + (long long)b * K;
    float m2, l2;
    row_lse_parts(lg, K, lane, m2, l2);
    const float ne = nent[b];
    float cy = 0.f;
    if (W) cy = by * act[b];
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
        if (W) dlogits[(long long)b * K + lane] = t * invT + cy * (expf(lp) * (lp - ne));
        else dlogits[(long long)b * K + lane] = t * invT + expf(lp) * (lp - ne);
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
        if (W) dlogits[(long long)b * K + k] = t * invT + cy * (expf(lp) * (lp - ne));
        else dlogits[(long long)b * K + k] = t * invT + expf(lp) * (lp - ne);
      }
      __syncthreads();
    }
  }
}

}  // namespace gmvae
