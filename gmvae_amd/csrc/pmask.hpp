// GMVAE_OBJ_PIXEL_MASK: a per-example observation mask m_bd (uint8 [B][D], observed iff non-zero, x's layout and stride).
//   pmask_rows   x~ = m ? x : 0 -- what every network that reads x takes (zero imputation) -- and the example's two counts
//   pmask_tail   tail[5] = sum_b mean_s (-hid_bs) from the masked Bernoulli epilogue's held-out partials (gemm.hpp, Problem::part2),
//                tail[6] = sum_b sum_d (1 - m_bd), tail[7] = sum_b sum_d m_bd
// One owner per output, fixed-order reductions, no atomics: eager and captured steps give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmvae {

// per byte of a word: 0x80 where the byte is non-zero
__device__ __forceinline__ unsigned pmask_nz(const unsigned w) { return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u; }

// A workgroup per example (grid-stride over b).  Rows that start 16-byte aligned in all three buffers (D % 16 == 0 on aligned
// bases) go as 16-byte words, every other shape byte by byte.  cnt [B][2] = (missing, observed) as floats: exact (D < 2^24).
__global__ __launch_bounds__(256) void pmask_rows(const unsigned char* __restrict__ x, const unsigned char* __restrict__ m,
                                                   unsigned char* __restrict__ xt, float* __restrict__ cnt, const int B,
                                                   const int D) {
  __shared__ int red[4];
  const int t = threadIdx.x;
  const bool vec = (D & 15) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(xt)) & 15) == 0;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const long long o = (long long)b * D;
    int obs = 0;
    if (vec) {
      const uint4* const x4 = reinterpret_cast<const uint4*>(x + o);
      const uint4* const m4 = reinterpret_cast<const uint4*>(m + o);
      uint4* const o4 = reinterpret_cast<uint4*>(xt + o);
      for (int i = t; i < (D >> 4); i += 256) {
        const uint4 xv = x4[i], mv = m4[i];
        const unsigned n0 = pmask_nz(mv.x), n1 = pmask_nz(mv.y), n2 = pmask_nz(mv.z), n3 = pmask_nz(mv.w);
        obs += __popc(n0) + __popc(n1) + __popc(n2) + __popc(n3);
        o4[i] = make_uint4(xv.x & ((n0 >> 7) * 0xffu), xv.y & ((n1 >> 7) * 0xffu), xv.z & ((n2 >> 7) * 0xffu), xv.w & ((n3 >> 7) * 0xffu));
      }
    } else {
      for (int i = t; i < D; i += 256) {
        const bool ob = m[o + i] != 0;
        obs += ob ? 1 : 0;
        xt[o + i] = ob ? x[o + i] : (unsigned char)0;
      }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) obs += __shfl_xor(obs, s, 64);
    __syncthreads();                               // (the previous example's sums are read)
    if ((t & 63) == 0) red[t >> 6] = obs;
    __syncthreads();
    if (t == 0) {
      const int n = red[0] + red[1] + red[2] + red[3];
      cnt[2 * (long long)b] = (float)(D - n);
      cnt[2 * (long long)b + 1] = (float)n;
    }
  }
}

// One workgroup.  hpart [B S][nparts]: the held-out Bernoulli sums per row and column tile; cnt [B][2] as above.  fp64 sums (the
// counts stay exact while B D < 2^53; as floats in the tail while B D < 2^24).
__global__ __launch_bounds__(1024) void pmask_tail(const float* __restrict__ hpart, const int nparts, const float* __restrict__ cnt,
                                                    float* __restrict__ tail, const int B, const int S) {
  __shared__ double red[3][1024];
  const int t = threadIdx.x;
  double a5 = 0., a6 = 0., a7 = 0.;
  for (int b = t; b < B; b += 1024) {
    const float* const hp = hpart + (long long)b * S * nparts;
    double h = 0.;
    for (long long i = 0; i < (long long)S * nparts; ++i) h += (double)hp[i];
    a5 -= h / (double)S;
    a6 += (double)cnt[2 * (long long)b];
    a7 += (double)cnt[2 * (long long)b + 1];
  }
  red[0][t] = a5; red[1][t] = a6; red[2][t] = a7;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; red[2][t] += red[2][t + o]; }
    __syncthreads();
  }
  if (t == 0) { tail[5] = (float)red[0][0]; tail[6] = (float)red[1][0]; tail[7] = (float)red[2][0]; }
}

}  // namespace gmvae
