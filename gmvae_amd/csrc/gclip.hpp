// GMVAE_OPT_CLIP_NORM: tf.clip_by_global_norm in front of TF-Adam, on the batch-mean gradient, with no division by the norm.
//   g      the gradient SUMS grads[0, P) (P = P_padded: the padding words are zero and count),  count = grads[P + 4]
//   SS     = sum_i g_i^2                 C = the threshold (one float the caller keeps in device memory)
//   norm   = sqrt(SS) / count            the global norm of the mean gradient, before clipping
//   d      = max(count, sqrt(SS) / C)    g_i / d = (g_i / count) min(1, C / norm)
// Adam applies gj = g_i (1 / d): adam_update with d where the count stood.  SS = 0 gives d = count; C = +inf never clips.
// The step is SKIPPED (params, m, v keep their bits) unless C > 0, SS is finite and the loss sum grads[P] is finite.
//
// SS is a two-stage fixed-order reduction, no atomics and no fp32 accumulation (g^2 overflows fp32 above 1.8e19 and vanishes
// below 1e-23): partial k covers elements [1024 k, 1024 (k + 1)) -- ONE 256-thread block of 16-byte loads, which is also the
// block of finalize_grads that holds those sums in registers -- each square exact in fp64 (fp32 x fp32), a thread's four added
// in element order, the block's 256 by a fixed tree; the partials are then added in index order.  One device function per
// stage (gclip_block_ss, gclip_record), shared by every kernel that runs it: the eager entry, the train graphs and the
// data-parallel forms give the same bits.
// The record, 4 floats: [0] norm, [1] d, [2] 1 if d > count (the step was clipped) else 0, [3] the guard -- the loss sum, or NaN
// where the step is to be skipped.  adam_tf(..., gscale_dev = &rec[1], loss_sum_dev = &rec[3]) is its consumer; gclip_finish_adam
// is the same statement in one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.hpp"

namespace gmvae {

constexpr int kClipBlock = 256;                       // threads; 4 elements each
constexpr int kClipSpan = 4 * kClipBlock;             // elements per partial

struct ClipRec {
  float norm, d, clipped, guard;
};

// stage 1: the block's partial.  Every thread of the block calls it (a thread past the end of the buffer passes zeros).
__device__ __forceinline__ void gclip_block_ss(const float4 a, double* __restrict__ part) {
  __shared__ double red[kClipBlock];
  const double x = (double)a.x, y = (double)a.y, z = (double)a.z, w = (double)a.w;
  red[threadIdx.x] = ((x * x + y * y) + z * z) + w * w;       // (fp32 x fp32 is exact in fp64; no contraction changes a product that is exact)
  __syncthreads();
#pragma unroll
  for (int o = kClipBlock >> 1; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// stage 2: the partials in index order, then the statement in fp64, rounded to fp32 once.  Uniform over the launch: every
// thread that calls it reads the same words and forms the same record.
__device__ __forceinline__ ClipRec gclip_record(const double* __restrict__ part, const int nparts, const float count,
                                                const float loss_sum, const float C) {
  double ss = 0.0;
  int k = 0;
  for (; k + 8 <= nparts; k += 8) {                    // (eight loads in flight; the adds stay in index order)
    double t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = part[k + j];
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += t[j];
  }
  for (; k < nparts; ++k) ss += part[k];
  const double root = sqrt(ss), cnt = (double)count, over = root / (double)C;
  const double d = over > cnt ? over : cnt;            // (a NaN on either side ends in a skip below)
  const bool ok = C > 0.f && __builtin_isfinite(ss) && __builtin_isfinite(loss_sum);
  ClipRec r;
  r.norm = (float)(root / cnt);
  r.d = (float)d;
  r.clipped = (ok && over > cnt) ? 1.f : 0.f;
  r.guard = ok ? loss_sum : __builtin_nanf("");
  return r;
}

// the partials of a buffer that is already summed (gmvae_grad_clip; behind the data-parallel all-reduce)
__global__ __launch_bounds__(kClipBlock) void gclip_partials(const float* __restrict__ g, long long P, double* __restrict__ part) {
  const long long i4 = ((long long)blockIdx.x * kClipBlock + threadIdx.x) * 4;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i4 < P) a = *reinterpret_cast<const float4*>(g + i4);       // (P % 4 == 0: a 16-byte load never straddles the end)
  gclip_block_ss(a, part);
}

// finalize_grads under the bit: grads[i] = the fixed-order sum over the split-K slabs (and the mixture-prior partials), as
// there, with no AdamTail; block k also leaves partial k of the sum of squares, from the sums it holds in registers.
__global__ __launch_bounds__(kClipBlock) void finalize_grads_ss(const float* __restrict__ slabs, int nslab, long long P,
                                                                float* __restrict__ grads, const float* __restrict__ gmp_part,
                                                                int gmp_n, int gmp_len, long long gmp_off, const SlabX sx,
                                                                double* __restrict__ part) {
  const long long i4 = ((long long)blockIdx.x * kClipBlock + threadIdx.x) * 4;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i4 < P) {
    a = slab_sum4(slabs + i4, P, slab_count(sx, i4, nslab));
    if (gmp_part && i4 >= gmp_off && i4 < gmp_off + gmp_len) {
      const float* p0 = gmp_part + (i4 - gmp_off);
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
      for (int g = 0; g < gmp_n; ++g) {
        const float4 o = *reinterpret_cast<const float4*>(p0 + (long long)g * gmp_len);
        acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
      }
      a = acc;
    }
    *reinterpret_cast<float4*>(grads + i4) = a;
  }
  gclip_block_ss(a, part);
}

// the record alone: one block (gmvae_grad_clip, whose caller runs adam_tf_step on the record)
__global__ __launch_bounds__(64) void gclip_finish(const double* __restrict__ part, int nparts, const float* __restrict__ tail,
                                                   const float* __restrict__ clip_norm, float* __restrict__ rec) {
  const ClipRec r = gclip_record(part, nparts, tail[4], tail[0], *clip_norm);
  if (threadIdx.x == 0) { rec[0] = r.norm; rec[1] = r.d; rec[2] = r.clipped; rec[3] = r.guard; }
}

// the record and TF-Adam on it in ONE launch (the train graphs; the data-parallel forms behind gclip_partials): every block
// forms the record from the partials (the same words, the same bits), block 0 writes it and this step's tail log, and the
// update is adam_tf's on (gscale = 1 / d, guard) -- adam_update, the one statement of the step.
__global__ __launch_bounds__(kClipBlock) void gclip_finish_adam(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                const float* __restrict__ g, long long P, float lr, float b1,
                                                                float b2, float eps, const uint64_t* __restrict__ t_dev,
                                                                const double* __restrict__ part, int nparts,
                                                                const float* __restrict__ clip_norm, float* __restrict__ rec,
                                                                float* __restrict__ tail_log) {
  const ClipRec r = gclip_record(part, nparts, g[P + 4], g[P], *clip_norm);
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) { rec[0] = r.norm; rec[1] = r.d; rec[2] = r.clipped; rec[3] = r.guard; }
    if (tail_log && threadIdx.x < 8) tail_log[threadIdx.x] = g[P + threadIdx.x];
  }
  if (!__builtin_isfinite(r.guard)) return;            // skipped: params, m, v keep their bits
  const unsigned long long t = *t_dev;
  const float gscale = 1.f / r.d;
  const float lr_t = (float)((double)lr * sqrt(1.0 - pow((double)b2, (double)t)) / (1.0 - pow((double)b1, (double)t)));
  const float omb1 = 1.f - b1, omb2 = 1.f - b2;
  const long long i4 = ((long long)blockIdx.x * kClipBlock + threadIdx.x) * 4;
  if (i4 >= P) return;
  float4 pp = *reinterpret_cast<float4*>(p + i4), mm = *reinterpret_cast<float4*>(m + i4), vv = *reinterpret_cast<float4*>(v + i4);
  const float4 gg = *reinterpret_cast<const float4*>(g + i4);
  float pa[4] = {pp.x, pp.y, pp.z, pp.w}, ma[4] = {mm.x, mm.y, mm.z, mm.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
  const float ga[4] = {gg.x, gg.y, gg.z, gg.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) adam_update(pa[j], ma[j], va[j], ga[j], gscale, lr_t, omb1, omb2, eps);
  *reinterpret_cast<float4*>(p + i4) = make_float4(pa[0], pa[1], pa[2], pa[3]);
  *reinterpret_cast<float4*>(m + i4) = make_float4(ma[0], ma[1], ma[2], ma[3]);
  *reinterpret_cast<float4*>(v + i4) = make_float4(va[0], va[1], va[2], va[3]);
}

}  // namespace gmvae
