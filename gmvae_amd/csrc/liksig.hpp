// GMVAE_LIK_SCALE_LEARNED: the gradient of the Gaussian decoder's log-scale rho [D], sigma_d = exp(rho_d).
//   d loss / d rho_d = sum_r rw_r (1 - sigma_d^2 g_rd^2)        g = (lambda - t) / sigma^2 [R][D], the likelihood epilogue's stored C
//                                                               rw = the backward's row weights [R], or 1 (null)
// Under IWAE the row weights exist only behind the row terms, so the sum cannot ride in the epilogue: it is a pass of its own over
// g, bandwidth-bound (R D floats read once, 16 bytes per lane, lanes along the columns).
//   liksig_partial   a workgroup per (row slab x strip of 64 columns): 16 row lanes x 16 column quads; each thread sums its rows in
//                    index order, the 16 row lanes are summed in lane order through LDS -> part [slabs][pad4(D)]
//   liksig_finish    a thread per column: the slab partials in index order -> slab 0 of the gradient buffer's split-K slabs, 0 to
//                    the other slabs of rho's range (and to the pad columns), so finalize_grads / finalize_grads_ss sum rho's
//                    range like every other entry
// One owner per output, fixed-order sums, no atomics: eager, captured and data-parallel steps give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmvae {

constexpr int kLsigCols = 64, kLsigRowLanes = 16, kLsigMaxSlabs = 256;

// rows per slab: 64 (four per thread), doubled until at most kLsigMaxSlabs slabs
static inline int liksig_slab_rows(const long long R) {
  int rs = 64;
  while ((R + rs - 1) / rs > kLsigMaxSlabs) rs *= 2;
  return rs;
}
static inline int liksig_slabs(const long long R) {
  const int rs = liksig_slab_rows(R);
  return (int)((R + rs - 1) / rs);
}

// grid (ceil(D / 64), slabs), 256 threads.  Dp = pad4(D): part's row length.
__global__ __launch_bounds__(256) void liksig_partial(const float* __restrict__ g, const float* __restrict__ rw,
                                                      const float* __restrict__ rho, float* __restrict__ part, const int R,
                                                      const int D, const int Dp, const int rs) {
  __shared__ float red[kLsigRowLanes][kLsigCols + 4];
  const int tid = threadIdx.x, c4 = tid % (kLsigCols / 4), rr = tid / (kLsigCols / 4);
  const int nb = blockIdx.x * kLsigCols + 4 * c4;
  const int r0 = blockIdx.y * rs, r1 = (R - r0 < rs) ? R : r0 + rs;      // (r0 < R: the grid has ceil(R / rs) slabs)
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (nb < D) {
    float s2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s2[j] = expf(2.f * rho[nb + j < D ? nb + j : D - 1]);
    if ((D & 3) == 0 && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {      // (every row quad starts 16-byte aligned and lies inside D)
#pragma unroll 4
      for (int r = r0 + rr; r < r1; r += kLsigRowLanes) {
        const float4 c = *reinterpret_cast<const float4*>(g + (long long)r * D + nb);
        const float wr = rw ? rw[r] : 1.f;
        acc[0] = fmaf(wr, fmaf(-s2[0] * c.x, c.x, 1.f), acc[0]);
        acc[1] = fmaf(wr, fmaf(-s2[1] * c.y, c.y, 1.f), acc[1]);
        acc[2] = fmaf(wr, fmaf(-s2[2] * c.z, c.z, 1.f), acc[2]);
        acc[3] = fmaf(wr, fmaf(-s2[3] * c.w, c.w, 1.f), acc[3]);
      }
    } else {                                                               // (the scalar path: any D, any alignment)
      for (int r = r0 + rr; r < r1; r += kLsigRowLanes) {
        const float* const gr = g + (long long)r * D;
        const float wr = rw ? rw[r] : 1.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (nb + j < D) { const float c = gr[nb + j]; acc[j] = fmaf(wr, fmaf(-s2[j] * c, c, 1.f), acc[j]); }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[rr][4 * c4 + j] = acc[j];
  __syncthreads();
  if (tid < kLsigCols) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < kLsigRowLanes; ++k) t += red[k][tid];
    const int n = blockIdx.x * kLsigCols + tid;
    if (n < Dp) part[(long long)blockIdx.y * Dp + n] = n < D ? t : 0.f;
  }
}

// slabs: the gradient buffer's split-K slabs [ns][P]; off: rho's offset in a slab.
__global__ __launch_bounds__(256) void liksig_finish(const float* __restrict__ part, const int nslab, float* __restrict__ slabs,
                                                     const long long P, const int ns, const long long off, const int Dp) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= Dp) return;
  float t = 0.f;
  for (int s = 0; s < nslab; ++s) t += part[(long long)s * Dp + n];
  slabs[off + n] = t;
  for (int k = 1; k < ns; ++k) slabs[(long long)k * P + off + n] = 0.f;
}

}  // namespace gmvae
