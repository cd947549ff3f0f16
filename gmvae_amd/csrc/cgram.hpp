// The centred fp64 Gram tile ("centred Gram") that gmvae_mmd's rbf form (csrc/twosample.hpp) and gmvae_sinkhorn (csrc/sinkhorn.hpp)
// are built around: squared distances from the expanded square n_i + n_j - 2 zc_i . zc_j on the rows centred by the pooled mean
// (fp64; n_i = |zc_i|^2), the dot products on v_mfma_f64_16x16x4_f64.  Defined here once:
//   the tile's geometry and the limits of the two planning rules (cg_slabs, cg_mean_slices);
//   the row source of a kernel: one array (CgRows) or the pooled pair x, then y (CgPooled), chosen at compile time;
//   the tile (cg_fetch, cg_stage, cg_mfma): a workgroup of eight waves owns kCgRows = 32 rows i and walks column tiles of kCgCols =
//     64 rows j.  Per tile, D in chunks of kCgDChunk = 32 staged as fp32 [32][33] and [64][33] (and the mean's chunk), each chunk
//     loaded into registers while the one before it is summed -- by the kernel's own sum, or by cg_mfma: wave w owns the 16 x 16
//     block (w >> 2, w & 3) of the tile, eight MFMA steps a chunk, the operands centred on the way in (A: lane & 15 the row,
//     lane >> 4 the dimension of the step; D: entry c of a lane is row (lane >> 4) + 4 c, column lane & 15);
//   the three launches in front (cg_setup in csrc/twosample.hip): cg_mean_part and cg_mean_fold (the pooled mean: row slices, then
//     the slices in order), cg_norms (a wave per row).
// Fixed-order fp64 sums, no float atomics: two runs give the same bits.
// This header DEFINES kernels (the last section), so it belongs to one translation unit: csrc/twosample.hip, which holds the host
// sides of both evaluators.  Everything above that section is constants and inline device functions and could be split off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmvae {

constexpr int kCgBlock = 512;             // a tile kernel: eight waves
constexpr int kCgSmallBlock = 256;        // the set-up kernels
constexpr int kCgRows = 32;               // rows i of a workgroup: two 16-row MFMA blocks
constexpr int kCgCols = 64;               // rows j of a column tile: four 16-column MFMA blocks
constexpr int kCgDChunk = 32;             // dimensions staged at a time
constexpr int kCgStage = (kCgRows + kCgCols) * kCgDChunk / kCgBlock;      // floats of a chunk a thread stages
constexpr int kCgZld = kCgDChunk + 1;     // the staged rows' leading dimension (floats)
constexpr int kCgKld = kCgCols + 1;       // the result tile's (doubles)
constexpr int kCgMaxSlabs = 16;
constexpr int kCgFillGroups = 256;        // the slabs fill about this many workgroups where the row tiles alone do not
constexpr int kCgMeanSlices = 64;         // row slices of the mean, 1024 rows each at least

typedef double cg_d4 __attribute__((ext_vector_type(4)));

// the slabs the column tiles are cut into; a caller may own fewer where they do not divide
__host__ __device__ static inline int cg_slabs(int row_tiles, int col_tiles) {
  int s = row_tiles >= kCgFillGroups ? 1 : (kCgFillGroups + row_tiles - 1) / row_tiles;
  s = s > kCgMaxSlabs ? kCgMaxSlabs : s;
  return s > col_tiles ? col_tiles : s;
}

// the row slices of the mean's first pass over N pooled rows
struct CgSlices {
  int slices, rows;
};
__host__ __device__ static inline CgSlices cg_mean_slices(int N) {
  int ms = (N + 1023) / 1024;
  ms = ms > kCgMeanSlices ? kCgMeanSlices : ms;
  CgSlices s;
  s.rows = (N + ms - 1) / ms;
  s.slices = (N + s.rows - 1) / s.rows;
  return s;
}

// row g, dimension d of one array z [N][D] ...
struct CgRows {
  const float* z;
  __device__ __forceinline__ float at(const int g, const int d, const int D) const { return z[(size_t)g * D + d]; }
};
// ... and of the pooled rows x [n][D], then y
struct CgPooled {
  const float* x;
  int n;
  const float* y;
  __device__ __forceinline__ float at(const int g, const int d, const int D) const {
    return g < n ? x[(size_t)g * D + d] : y[(size_t)(g - n) * D + d];
  }
};

// A tile kernel's pass over D.  A chunk of kCgDChunk dimensions of the 32 rows i and the 64 rows j of a column tile is kCgStage
// floats a thread, held in the kernel's `pre` and loaded a chunk ahead, so that the loads' latency runs under the sums.  Per chunk
// the kernel calls cg_stage, then its fetch of the next chunk -- of this tile, or the first of the tile behind it --, then its sum
// (cg_mfma, or its own).  The fetch is a lambda of the kernel around cg_fetch, and the kernel calls it itself: with the calls in
// here, mmd_tiles and sk_tiles come out with other register budgets (profiles/gram_tile_refactor_notes.md).

// chunk dc of the rows i = [i_off + i0, ...) of i_cnt and the rows j = [j_off + j0, ...) of j_cnt into pre (a row past its count
// and a dimension past D as 0)
template <class Src>
__device__ __forceinline__ void cg_fetch(float (&pre)[kCgStage], const Src& src, const int D, const int i_off, const int i_cnt,
                                         const int j_off, const int j_cnt, const int i0, const int j0, const int dc) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int u = 0; u < kCgStage; ++u) {
    const int s = tid + u * kCgBlock, r = s / kCgDChunk, d = dc + (s % kCgDChunk);
    const bool row = r < kCgRows;
    const int local = row ? i0 + r : j0 + (r - kCgRows);
    pre[u] = local < (row ? i_cnt : j_cnt) && d < D ? src.at((row ? i_off : j_off) + local, d, D) : 0.f;
  }
}

// pre into s_z ([kCgRows + kCgCols][kCgZld]: the rows i, then the rows j) and, if kCentre, the mean's chunk into s_mean [kCgDChunk]
template <bool kCentre>
__device__ __forceinline__ void cg_stage(const float (&pre)[kCgStage], const int dc, const int D, float* const s_z, double* const s_mean,
                                         const double* __restrict__ mean) {
  const int tid = threadIdx.x;
  __syncthreads();      // the previous chunk's sums have read s_z
#pragma unroll
  for (int u = 0; u < kCgStage; ++u) {
    const int s = tid + u * kCgBlock;
    s_z[(s / kCgDChunk) * kCgZld + (s % kCgDChunk)] = pre[u];
  }
  if (kCentre && tid < kCgDChunk) s_mean[tid] = dc + tid < D ? mean[dc + tid] : 0.0;
  __syncthreads();
}

// the staged chunk onto the wave's 16 x 16 block (rb, cb) = (wave >> 2, wave & 3) of zc_i . zc_j, eight MFMA steps; l15 = lane & 15,
// l4 = lane >> 4, entry c of dot is row 16 rb + l4 + 4 c, column 16 cb + l15 of the tile (a dimension past D: 0 - 0; a row past
// its count: -mean, never used)
__device__ __forceinline__ void cg_mfma(const float* const s_z, const double* const s_mean, const int rb, const int cb, const int l15,
                                        const int l4, cg_d4& dot) {
  const float* __restrict__ ai = s_z + (16 * rb + l15) * kCgZld + l4;
  const float* __restrict__ bj = s_z + kCgRows * kCgZld + (16 * cb + l15) * kCgZld + l4;
#pragma unroll
  for (int kk = 0; kk < kCgDChunk / 4; ++kk) {
    const double m = s_mean[4 * kk + l4];
    dot = __builtin_amdgcn_mfma_f64_16x16x4f64((double)ai[4 * kk] - m, (double)bj[4 * kk] - m, dot, 0, 0, 0);
  }
}

// ------------------------------------------------------------------------------------------------ kernels (one translation unit)
// the pooled mean, first pass: workgroup (x, y) adds the rows of slice y in 64 columns; thread (r, c) the rows r, r + 4, ... in order
template <class Src>
__global__ __launch_bounds__(kCgSmallBlock) void cg_mean_part(const Src src, const int N, const int D, const int rows_per_slice,
                                                               double* __restrict__ part) {
  __shared__ double s[4][64];
  const int tid = threadIdx.x, r = tid >> 6, cl = tid & 63, c = blockIdx.x * 64 + cl;
  const int lo = blockIdx.y * rows_per_slice, hi = lo + rows_per_slice < N ? lo + rows_per_slice : N;
  double a = 0.0;
  if (c < D)
    for (int i = lo + r; i < hi; i += 4) a += (double)src.at(i, c, D);
  s[r][cl] = a;
  __syncthreads();
  if (r == 0 && c < D) part[(size_t)blockIdx.y * D + c] = ((s[0][cl] + s[1][cl]) + s[2][cl]) + s[3][cl];
}

// ... second pass: the slices in order
__global__ __launch_bounds__(kCgSmallBlock) void cg_mean_fold(const double* __restrict__ part, const int slices, const int N, const int D,
                                                               double* __restrict__ mean) {
  const int d = blockIdx.x * kCgSmallBlock + threadIdx.x;
  if (d >= D) return;
  double a = 0.0;
  for (int s = 0; s < slices; ++s) a += part[(size_t)s * D + d];
  mean[d] = a / (double)N;
}

// |z_i - mean|^2: a wave per row, a lane the dimensions lane, lane + 64, ... in order, then the lanes by six exchanges
template <class Src>
__global__ __launch_bounds__(kCgSmallBlock) void cg_norms(const Src src, const int N, const int D, const double* __restrict__ mean,
                                                           double* __restrict__ nrm) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (kCgSmallBlock / 64) + (threadIdx.x >> 6);
  if (i >= N) return;      // (uniform in the wave)
  double a = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double e = (double)src.at(i, d, D) - mean[d];
    a = fma(e, e, a);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m);
  if (lane == 0) nrm[i] = a;
}

}  // namespace gmvae
