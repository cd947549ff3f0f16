// The squared-distance tile that csrc/tsne.hpp and csrc/neigh.hpp share (tsne.hpp's header states it and gives its constants): a
// lane owns a row, tiles of kTsTile points are staged in LDS as doubles and read back as broadcasts, the differences and their sum
// are fp64.  Only inline code here: both translation units include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmvae {

constexpr int kTsBlock = 256;        // threads = points (or rows) of a block
constexpr int kTsTile = 32;          // points j per tile; slices begin at multiples of it
constexpr int kTsDims = 64;          // dimensions staged per round
constexpr int kTsLd = kTsDims + 2;   // LDS row stride (doubles)
constexpr int kTsMaxSlices = 64;
constexpr int kTsTargetBlocks = 1024;

// slices of the j range for a grid of n lanes
static inline int ts_slices(int64_t n) {
  const int64_t blocks = (n + kTsBlock - 1) / kTsBlock;
  const int64_t ns = (kTsTargetBlocks + blocks - 1) / blocks;
  return (int)(ns < 1 ? 1 : ns > kTsMaxSlices ? kTsMaxSlices : ns);
}

// N points cut into at most ns slices of whole tiles
struct TsSplit {
  int per_slice, used;
};
static inline TsSplit ts_split(int64_t N, int ns) {
  const int64_t units = (N + kTsTile - 1) / kTsTile;
  const int per = (int)((units + ns - 1) / ns) * kTsTile;
  return TsSplit{per, (int)((N + per - 1) / per)};
}

// acc[ct] = |c_i - c_(c0 + ct)|^2 for the tile's points below c_hi (a point past c_hi is staged as zeros: the caller drops its
// sum); ci: this lane's row.  Every thread of the block calls it (it synchronises).
__device__ __forceinline__ void ts_tile_d2(double (&acc)[kTsTile], double (*s_c)[kTsLd], const float* __restrict__ codes,
                                           const float* __restrict__ ci, const int L, const int c0, const int c_hi, const int tid) {
  const int ct_st = tid >> 3, j_st = tid & 7;      // staging: 8 threads per point
  const int cs = c0 + ct_st;
  const bool cvalid = cs < c_hi;
#pragma unroll
  for (int i = 0; i < kTsTile; ++i) acc[i] = 0.0;
  for (int d0 = 0; d0 < L; d0 += kTsDims) {
    const int dn = min(kTsDims, L - d0), dn8 = (dn + 7) & ~7;
    __syncthreads();
    for (int j = j_st; j < dn8; j += 8) s_c[ct_st][j] = (cvalid && j < dn) ? (double)codes[(size_t)cs * L + d0 + j] : 0.0;
    __syncthreads();
    for (int d = 0; d < dn8; d += 8) {
      double zz[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) zz[j] = (d + j < dn) ? (double)ci[d0 + d + j] : 0.0;
#pragma unroll
      for (int ct = 0; ct < kTsTile; ++ct) {
        const double2* __restrict__ q = reinterpret_cast<const double2*>(&s_c[ct][d]);
        const double2 a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
        const double av[8] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y};
        double a = acc[ct];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const double r = zz[j] - av[j];
          a = fma(r, r, a);
        }
        acc[ct] = a;
      }
    }
  }
}

}  // namespace gmvae
