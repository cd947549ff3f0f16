// gmvae_knn_* (include/gmvae_hip.h; host side: csrc/neigh.hip): exact brute-force nearest neighbours of queries q [Nq][L] among
// references r [Nr][L], the rank of given candidates in the same order, and distance sums per class.  Model independent.  The
// statement is tests/neigh_ref.py.
//   D_ij = sum_d (q_id - r_jd)^2 in the difference form, fp64 differences and sum, by tsne.hpp's ts_tile_d2 (csrc/d2tile.hpp; never the expanded
//   square: aggpost.hpp's header gives the reason -- codes 1e3 from the origin and 1 apart lose every digit of D there -- and so
//   never the matrix cores);  d_ij = D_ij rounded once to fp32, a non-finite one counts as +inf.
// ORDER: reference j precedes j' for query i when (d_ij, j) < (d_ij', j') lexicographically -- ties in distance go to the smaller
// index.  d_ij >= +0, so its fp32 bit pattern orders as an unsigned integer, and the pair is the 64-bit key (bits(d_ij) << 32) | j.
// It is a TOTAL order of distinct keys, so the k first references, and the number of references in front of a candidate, are
// functions of the row of d alone: no result depends on tiling, slicing or the chunk of queries a call was given.  With
// self_offset >= 0 query i IS reference self_offset + i, and that reference is left out of query i's order.
// Stages (what was chosen, and why):
//   knn_dist writes d [Nq][Nr] (fp32) into the workspace: tsne_dist's shape -- a lane owns a query, a 256-thread block 256 queries,
//   tiles of kTsTile references staged in LDS as doubles and read back as broadcasts, grid.y slices the j range (ts_slices, ts_split)
//   so that a chunk of a few hundred queries still fills the chip.  search and ranks both start with it: the identity
//   ranks(search) = t is exact because both read the same stored row.
//   knn_select, a wave per stored row, every wave of the block in step (the block's barriers order the LDS traffic): a radix select
//   of the k-th key on bits(d), four passes of 8 bits from the top, each a histogram of the rows' elements that match the prefix so
//   far in 256 LDS integer counters (integer atomics: counts do not depend on their order), a scan of the counters by the wave, and
//   the bucket that holds the k-th.  That leaves the k-th distance T and how many references at exactly T are still wanted, `need`.
//   One more pass in ascending j gathers every element below T and the first `need` at T (ballots give each its slot, so ties go to
//   the smaller index) into LDS, k keys in all; they are ordered by counting, for each, the keys in front of it (k <= 256: at most
//   1024 broadcast reads per lane), and written to their rank.  Five passes over a stored row; what they cost next to
//   the distance stage, and what was tried, is in profiles/neigh_notes.md.
//   knn_rank, a wave per stored row: kNnCand candidates' keys in registers per pass over the row, every lane counts the keys in
//   front of each over its share of j, an integer xor tree adds the lanes.  A candidate outside [0, Nr), or self, gets -1.
//   knn_class: a pass of its own that rebuilds D by the same ts_tile_d2 and adds sqrt(D) (fp64 square root of the fp64 D) to the
//   lane's sum for the reference's class.  The class of a reference is the same for every lane of the block, so the sums are laid
//   out [class][lane] -- in LDS for C <= kNnLdsClasses (32 KiB; conflict-free, the lanes of a wave read consecutive doubles), in the
//   workspace [slice][C][Nq] for more classes (coalesced, and the block's C x 256 doubles stay in the L2): one owner per sum, added
//   in ascending j.  The j range is cut into slices of kNnSlice references WHATEVER Nq is, and knn_fold adds the slices in slice
//   order, so the sums do not depend on the chunk of queries either.  A label outside [0, C) contributes nowhere.
// No float atomics, one owner per output, fixed-order folds: two runs give the same bits, on any workspace contents.
// Every index written is a j < Nr that the gather pass visited (the slots are zeroed first), whatever the inputs hold.
// Constants: kTsBlock = 256 lanes a block, kTsTile = 32 references a tile (d2tile.hpp); kNnWave = 64 lanes per row in the row stages,
// so 4 rows a block; kNnMaxK = 256 (the k, m and C gates; 256 counters and 256 gathered keys per wave: 12 KiB of LDS a block);
// kNnCand = 8 candidates per pass of knn_rank; kNnSlice = 1024 references per slice of knn_class (32 tiles; a chunk of 1,100
// queries against 60,000 references is then 295 blocks); kNnLdsClasses = 16.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "d2tile.hpp"

namespace gmvae {

constexpr int kNnWave = 64;
constexpr int kNnRows = kTsBlock / kNnWave;      // stored rows per block of the row stages
constexpr int kNnMaxK = 256;
constexpr int kNnCand = 8;
constexpr int kNnSlice = 1024;
constexpr int kNnLdsClasses = 16;
static_assert(kNnSlice % kTsTile == 0, "slices begin at multiples of the tile");

static inline int nn_class_slices(int64_t Nr) { return (int)((Nr + kNnSlice - 1) / kNnSlice); }

// bits of d as the order's key: non-finite -> +inf
__device__ __forceinline__ float nn_clean(const float d) { return (d < INFINITY) ? d : INFINITY; }      // (NaN < inf is false)

// d [Nq][Nr]: one slice of the j range per blockIdx.y
__global__ __launch_bounds__(kTsBlock) void knn_dist(const float* __restrict__ q, const int Nq, const float* __restrict__ r,
                                                     const int Nr, const int L, const int per_slice, float* __restrict__ d) {
  __shared__ __attribute__((aligned(16))) double s_c[kTsTile][kTsLd];
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * kTsBlock + tid;
  const bool live = i < Nq;
  const float* __restrict__ qi = q + (size_t)(live ? i : 0) * L;      // (a lane past the end computes on query 0 and writes nothing)
  const int c_lo = (int)blockIdx.y * per_slice, c_hi = min(Nr, c_lo + per_slice);
  for (int c0 = c_lo; c0 < c_hi; c0 += kTsTile) {
    double acc[kTsTile];
    ts_tile_d2(acc, s_c, r, qi, L, c0, c_hi, tid);
    if (live) {
      float* __restrict__ o = d + (size_t)i * Nr + c0;
#pragma unroll
      for (int ct = 0; ct < kTsTile; ++ct)
        if (c0 + ct < c_hi) o[ct] = nn_clean((float)acc[ct]);
    }
  }
}

__device__ __forceinline__ int nn_wave_sum(int v) {
#pragma unroll
  for (int o = kNnWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the first k references of every stored row in the order (d, j), ascending.  Every wave of the block runs every barrier (a wave
// past the last row works on row 0 and writes nothing).
__global__ __launch_bounds__(kTsBlock) void knn_select(const float* __restrict__ d, const int Nq, const int Nr, const int k,
                                                       const long long self_offset, int32_t* __restrict__ idx_out,
                                                       float* __restrict__ d2_out) {
  __shared__ int s_hist[kNnRows][kNnMaxK];
  __shared__ unsigned long long s_key[kNnRows][kNnMaxK];
  const int lane = threadIdx.x & (kNnWave - 1), w = threadIdx.x / kNnWave;
  const long long row = (long long)blockIdx.x * kNnRows + w;
  const bool live = row < Nq;
  const long long i = live ? row : 0;
  const uint32_t* __restrict__ bits = reinterpret_cast<const uint32_t*>(d) + (size_t)i * Nr;
  const long long self = self_offset >= 0 ? self_offset + i : -1;
  int* const hist = s_hist[w];
  unsigned long long* const keys = s_key[w];
  uint32_t prefix = 0, mask = 0;
  int need = k;      // the (need)-th smallest among the elements that match the prefix is the k-th of the row
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int b = lane; b < kNnMaxK; b += kNnWave) hist[b] = 0;
    __syncthreads();
    for (int j = lane; j < Nr; j += kNnWave) {
      const uint32_t u = bits[j];
      if (j != self && (u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1);
    }
    __syncthreads();
    // lane l holds the counters 4 l .. 4 l + 3; an inclusive scan over the lanes, then the bucket that holds the need-th
    const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
    const int own = h0 + h1 + h2 + h3;
    int incl = own;
#pragma unroll
    for (int o = 1; o < kNnWave; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    const int excl = incl - own;
    const bool mine = excl < need && need <= incl;      // exactly one lane: the row holds at least k elements
    int bucket = 0, before = excl;
    if (mine) {
      if (need > before + h0) {
        before += h0;
        bucket = 1;
        if (need > before + h1) {
          before += h1;
          bucket = 2;
          if (need > before + h2) {
            before += h2;
            bucket = 3;
          }
        }
      }
      bucket += 4 * lane;
    }
    const unsigned long long who = __ballot(mine);
    const int src = who ? __ffsll((long long)who) - 1 : 0;
    bucket = __shfl(bucket, src);
    before = __shfl(before, src);
    need -= before;
    prefix |= (uint32_t)bucket << shift;
    mask |= 255u << shift;
    __syncthreads();      // (the counters are read before the next pass clears them)
  }
  // prefix = bits(T), the k-th distance; k - need elements lie below it, and the first `need` at T complete the k
  const int below = k - need;
  for (int t = lane; t < kNnMaxK; t += kNnWave) keys[t] = ((unsigned long long)0x7F800000u << 32);
  __syncthreads();
  int n_lt = 0, n_eq = 0;
  for (int j0 = 0; j0 < Nr; j0 += kNnWave) {
    const int j = j0 + lane;
    const bool in = j < Nr && j != self;
    const uint32_t u = in ? bits[j] : 0xFFFFFFFFu;
    const bool lt = in && u < prefix, eq = in && u == prefix;
    const unsigned long long m_lt = __ballot(lt), m_eq = __ballot(eq);
    const unsigned long long lower = (1ull << lane) - 1ull;
    int slot = -1;
    if (lt) slot = n_lt + __popcll(m_lt & lower);
    if (eq) {
      const int e = n_eq + __popcll(m_eq & lower);
      if (e < need) slot = below + e;
    }
    if (slot >= 0 && slot < k) keys[slot] = ((unsigned long long)u << 32) | (uint32_t)j;
    n_lt += __popcll(m_lt);
    n_eq += __popcll(m_eq);
  }
  __syncthreads();
  for (int t = lane; t < k; t += kNnWave) {
    const unsigned long long mine = keys[t];
    int rank = 0;
    for (int s = 0; s < k; ++s) rank += keys[s] < mine ? 1 : 0;
    if (live) {
      if (idx_out) idx_out[(size_t)i * k + rank] = (int32_t)(uint32_t)(mine & 0xFFFFFFFFull);
      if (d2_out) d2_out[(size_t)i * k + rank] = __uint_as_float((uint32_t)(mine >> 32));
    }
  }
}

// rank [Nq][m]: the references (self left out) strictly in front of cand [i][t] in query i's order; -1 for self or no reference
__global__ __launch_bounds__(kTsBlock) void knn_rank(const float* __restrict__ d, const int Nq, const int Nr,
                                                     const long long self_offset, const int32_t* __restrict__ cand, const int m,
                                                     int32_t* __restrict__ rank_out) {
  const int lane = threadIdx.x & (kNnWave - 1);
  const long long i = (long long)blockIdx.x * kNnRows + threadIdx.x / kNnWave;
  if (i >= Nq) return;      // (the whole wave leaves; no block-wide synchronisation below)
  const uint32_t* __restrict__ bits = reinterpret_cast<const uint32_t*>(d) + (size_t)i * Nr;
  const long long self = self_offset >= 0 ? self_offset + i : -1;
  for (int t0 = 0; t0 < m; t0 += kNnCand) {
    unsigned long long ck[kNnCand];
    bool ok[kNnCand];
    int cnt[kNnCand];
#pragma unroll
    for (int g = 0; g < kNnCand; ++g) {
      const int c = t0 + g < m ? cand[(size_t)i * m + t0 + g] : -1;
      ok[g] = c >= 0 && c < Nr && c != self;
      ck[g] = ok[g] ? (((unsigned long long)bits[c] << 32) | (uint32_t)c) : 0ull;
      cnt[g] = 0;
    }
    for (int j = lane; j < Nr; j += kNnWave) {
      if (j == self) continue;
      const unsigned long long key = ((unsigned long long)bits[j] << 32) | (uint32_t)j;
#pragma unroll
      for (int g = 0; g < kNnCand; ++g) cnt[g] += key < ck[g] ? 1 : 0;
    }
#pragma unroll
    for (int g = 0; g < kNnCand; ++g) {
      const int total = nn_wave_sum(cnt[g]);
      if (lane == 0 && t0 + g < m) rank_out[(size_t)i * m + t0 + g] = ok[g] ? total : -1;
    }
  }
}

// part [slice][C][Nq]: the sums of sqrt(D_ij) per class over one slice of kNnSlice references, added in ascending j
template <bool kLds>
__global__ __launch_bounds__(kTsBlock) void knn_class(const float* __restrict__ q, const int Nq, const float* __restrict__ r,
                                                      const int Nr, const int L, const int32_t* __restrict__ labels, const int C,
                                                      double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double s_c[kTsTile][kTsLd];
  __shared__ int s_lab[kTsTile];
  __shared__ double s_sum[kLds ? kNnLdsClasses : 1][kTsBlock];
  const int tid = threadIdx.x;
  const long long gi = (long long)blockIdx.x * kTsBlock + tid;
  const bool live = gi < Nq;
  const long long i = live ? gi : 0;      // (a lane past the end computes on query 0 and writes nothing)
  const float* __restrict__ qi = q + (size_t)i * L;
  double* __restrict__ mine = part + (size_t)blockIdx.y * C * Nq + (size_t)i;      // class c at mine[c Nq]
  if (kLds) {
    for (int c = 0; c < C; ++c) s_sum[c][tid] = 0.0;
  } else if (live) {
    for (int c = 0; c < C; ++c) mine[(size_t)c * Nq] = 0.0;
  }
  const int c_lo = (int)blockIdx.y * kNnSlice, c_hi = min(Nr, c_lo + kNnSlice);
  for (int c0 = c_lo; c0 < c_hi; c0 += kTsTile) {
    __syncthreads();
    if (tid < kTsTile) s_lab[tid] = c0 + tid < c_hi ? labels[c0 + tid] : -1;
    double acc[kTsTile];
    ts_tile_d2(acc, s_c, r, qi, L, c0, c_hi, tid);      // (its barriers publish s_lab)
#pragma unroll
    for (int ct = 0; ct < kTsTile; ++ct) {
      const int c = s_lab[ct];      // the same for every lane of the block
      if (c < 0 || c >= C) continue;
      const double s = sqrt(acc[ct]);
      if (kLds)
        s_sum[c][tid] += s;
      else if (live)
        mine[(size_t)c * Nq] += s;
    }
  }
  if (kLds && live)
    for (int c = 0; c < C; ++c) mine[(size_t)c * Nq] = s_sum[c][tid];
}

// sums [Nq][C] = the slices' parts [slice][C][Nq] added in slice order
__global__ __launch_bounds__(kTsBlock) void knn_fold(double* __restrict__ sums, const double* __restrict__ part, const int Nq,
                                                     const int C, const int ns) {
  const unsigned long long e = (unsigned long long)blockIdx.x * kTsBlock + threadIdx.x;      // e = c Nq + i
  const unsigned long long E = (unsigned long long)Nq * C;
  if (e >= E) return;
  double v = 0.0;
  for (int s = 0; s < ns; ++s) v += part[(size_t)s * E + e];
  const unsigned long long c = e / (unsigned long long)Nq, i = e % (unsigned long long)Nq;
  sums[i * C + c] = v;
}

}  // namespace gmvae
