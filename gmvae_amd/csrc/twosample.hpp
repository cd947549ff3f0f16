// gmvae_mmd (include/gmvae_hip.h; host side: csrc/twosample.hip): the kernel two-sample test of Gretton et al. 2012 -- the unbiased
// MMD^2 of P splits of one pooled sample z [N][D], split 0 the observed one, the others its permutation null.  Model independent.
// The statement is tests/twosample_ref.py:
//   d2_ij = sum_d (z_id - z_jd)^2
//   rbf:    k_ij = (1/Q) sum_q exp(-gamma_q d2_ij)   (fp64 exp: an fp32 one sits sixty times above the test's gate)
//   energy: k_ij = -sqrt(d2_ij)
//   K0 = K with a zero diagonal; e_p = row p of E [P][N] (uint8, non-zero = first sample), n_p = sum e_p, m_p = N - n_p
//   a_p = e_p^T K0 e_p, b_p = e_p^T K0 1, c = 1^T K0 1
//   mmd2[p] = a / (n (n - 1)) + (c - 2 b + a) / (m (m - 1)) - 2 (b - a) / (n m), NaN where n < 2 or m < 2
//   row_all = K0 1, row_first = K0 e_0
// Nothing N^2 in memory, nothing synchronises with the host.  d2 comes in one of two forms:
//   energy: from differences, each taken and squared in fp64 and added in ascending d: two equal rows give d2 = 0 and so exactly
//     k = 0, and sqrt sees no cancellation.  Two launches.
//   rbf:    the kernel is translation invariant, so from the centred Gram tile of csrc/cgram.hpp -- an eighth of the difference
//     form's time at D = 784 (profiles/twosample_notes.md) --, with its three small launches in front.  Five launches.
// mmd_tiles<NT, kEnergy>: a workgroup of eight waves owns kCgRows = 32 rows i, a slab of column tiles of kCgCols = 64 rows j
// (blockIdx.y; the slabs follow from N alone, mmd_plan) and a chunk of PC = 128 NT splits (blockIdx.z; NT in {1, 2, 4, 8} from P,
// so up to 1024 splits share one pass over the Gram matrix).  Per column tile:
//   stage E:  the tile's bytes of the chunk's splits, [PC][16] words of four j each (a split past P and a row past N as 0);
//   gram:     cgram.hpp's pass over D in chunks (cg_fetch, cg_stage).  rbf: its MFMA steps (cg_mfma); energy: thread (ty, tx) owns
//             the four pairs (ty, tx + 16 c).  Then the kernel function, 0 on the diagonal and past N, into the K tile [32][65]
//             (fp64);
//   row sums: thread i < 32 adds its row of the tile in ascending j onto its running sum: (K0 1)_i over the slab;
//   T += K E: wave w owns the chunk's columns [16 NT w, 16 NT (w + 1)).  Per step of four j it reads its two K operands (one per
//             16-row block) and, per 16 splits, a word of E whose byte becomes 0.0 / 1.0 on the way into the MFMA's B operand
//             (A: lane & 15 the row, lane >> 4 the j of the step; B: lane & 15 the split; D: entry g of a lane is row (lane >> 4) +
//             4 g, column lane & 15 -- csrc/linprobe.hpp's use).  The 2 NT accumulator tiles of a wave take turns, so no MFMA
//             waits for the one before it; 8 VGPRs a lane each: 128 at NT = 8, which leaves room for two waves a SIMD.
// At the end the workgroup folds a: sum_i E[i, p] T[i, p] (a lane's eight rows in order, then the four lane groups by two
// exchanges) and b: sum_i E[i, p] rowsum_i (a thread per split, ascending i) into partials [row tile][slab][P]; chunk 0 also
// leaves c's partial and, per slab, the row sums and column 0 of T for row_all and row_first.
// A split's column of T depends on no other column, and its partials on neither the chunk nor the wave it rides in: mmd2[p] is the
// same bits whatever other splits the call holds.
// mmd_finish: a workgroup per split counts n_p (integers), adds the partials of a, b and c over the workgroups in index order
// (256 runs of consecutive workgroups, then the runs in order) and finishes mmd2[p]; further workgroups add the slabs' row sums in
// slab order into row_all and row_first.
// One owner per output, fixed-order fp64 sums, no float atomics: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cgram.hpp"

namespace gmvae {

constexpr int kMmdWaves = kCgBlock / 64;
constexpr int kMmdSmallBlock = 256;        // mmd_finish
constexpr int kMmdMaxQ = 8;                // bandwidths of the rbf kernel
constexpr int kMmdMaxNT = 8;               // 16-split accumulator tiles per wave and row block: a chunk of 128 NT splits
constexpr int kMmdEld = kCgCols / 4 + 1;   // the staged splits' leading dimension (words of four j)
constexpr int kMmdKindRbf = 0, kMmdKindEnergy = 1;

struct MmdGamma {
  double g[kMmdMaxQ];
};

// the launches' shape.  The slabs and slices, and so the order of every sum, follow from N alone; the chunk only from P.
struct MmdPlan {
  int row_tiles, col_tiles, slabs, tiles_per_slab, nt, p_chunks;
  CgSlices mean;
  size_t groups;      // row_tiles * slabs: the workgroups that own partials
  size_t lds;
};
__host__ __device__ static inline MmdPlan mmd_plan(int N, int P) {
  MmdPlan p;
  p.row_tiles = (N + kCgRows - 1) / kCgRows;
  p.col_tiles = (N + kCgCols - 1) / kCgCols;
  const int s = cg_slabs(p.row_tiles, p.col_tiles);
  p.tiles_per_slab = (p.col_tiles + s - 1) / s;
  p.slabs = (p.col_tiles + p.tiles_per_slab - 1) / p.tiles_per_slab;
  p.nt = P <= 128 ? 1 : P <= 256 ? 2 : P <= 512 ? 4 : 8;
  p.p_chunks = (P + 128 * p.nt - 1) / (128 * p.nt);
  p.groups = (size_t)p.row_tiles * p.slabs;
  p.mean = cg_mean_slices(N);
  p.lds = 8 * ((size_t)kCgRows * kCgKld + kCgRows + kCgDChunk) + 4 * ((size_t)(kCgRows + kCgCols) * kCgZld + (size_t)128 * p.nt * kMmdEld);
  return p;
}

// the workspace, in doubles: a and b [groups][P], c [groups], the slabs' row sums and column 0 of T, [slabs][N] each; for rbf the
// mean's slices [mean_slices][D], the mean [D] and the centred rows' squared norms [N]
struct MmdLayout {
  size_t a, b, c, row_all, row_first, mean_part, mean, nrm, end;
};
__host__ __device__ static inline MmdLayout mmd_layout(const MmdPlan& p, int N, int D, int P) {
  MmdLayout o;
  o.a = 0;
  o.b = o.a + p.groups * (size_t)P;
  o.c = o.b + p.groups * (size_t)P;
  o.row_all = o.c + p.groups;
  o.row_first = o.row_all + (size_t)p.slabs * N;
  o.mean_part = o.row_first + (size_t)p.slabs * N;
  o.mean = o.mean_part + (size_t)p.mean.slices * D;
  o.nrm = o.mean + (size_t)D;
  o.end = o.nrm + (size_t)N;
  return o;
}

template <int NT, bool kEnergy>
__global__ __launch_bounds__(kCgBlock) void mmd_tiles(const float* __restrict__ z, const int N, const int D, const uint8_t* __restrict__ E,
                                                       const int P, const MmdGamma gam, const int Q, const int tiles_per_slab,
                                                       const int col_tiles, const int words_ok, const double* __restrict__ mean,
                                                       const double* __restrict__ nrm, double* __restrict__ part_a,
                                                       double* __restrict__ part_b, double* __restrict__ part_c,
                                                       double* __restrict__ part_row_all, double* __restrict__ part_row_first) {
  extern __shared__ __attribute__((aligned(16))) char mmd_smem[];
  constexpr int PC = 128 * NT;
  double* const s_k = reinterpret_cast<double*>(mmd_smem);             // [kCgRows][kCgKld]
  double* const s_rs = s_k + kCgRows * kCgKld;                        // [kCgRows]
  double* const s_mean = s_rs + kCgRows;                              // [kCgDChunk] (rbf)
  float* const s_zi = reinterpret_cast<float*>(s_mean + kCgDChunk);   // [kCgRows][kCgZld] (cg_stage: s_zj follows it)
  float* const s_zj = s_zi + kCgRows * kCgZld;                        // [kCgCols][kCgZld]
  uint32_t* const s_e = reinterpret_cast<uint32_t*>(s_zj + kCgCols * kCgZld);      // [PC][kMmdEld]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int i0 = blockIdx.x * kCgRows, slab = blockIdx.y, p0 = blockIdx.z * PC;
  const int jt_lo = slab * tiles_per_slab, jt_hi = jt_lo + tiles_per_slab < col_tiles ? jt_lo + tiles_per_slab : col_tiles;
  const int wave_p = p0 + wave * 16 * NT;      // the wave's first split

  cg_d4 acc[2][NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    acc[0][ct] = cg_d4{0.0, 0.0, 0.0, 0.0};
    acc[1][ct] = cg_d4{0.0, 0.0, 0.0, 0.0};
  }
  double rs = 0.0;      // (threads 0 .. 31: the row's sum over the slab)

  float pre[kCgStage];
  auto fetch = [&](const int j0, const int dc) { cg_fetch(pre, CgRows{z}, D, 0, N, 0, N, i0, j0, dc); };
  if (jt_lo < jt_hi) fetch(jt_lo * kCgCols, 0);

  for (int jt = jt_lo; jt < jt_hi; ++jt) {
    const int j0 = jt * kCgCols;
    __syncthreads();      // the previous tile's products have read s_k and s_e
    for (int s = tid; s < PC * (kCgCols / 4); s += kCgBlock) {
      const int pl = s >> 4, w = s & 15, gp = p0 + pl, j = j0 + 4 * w;
      uint32_t v = 0;
      if (gp < P && j < N) {
        const uint8_t* __restrict__ src = E + (size_t)gp * N + j;
        if (words_ok && j + 3 < N) {
          v = *reinterpret_cast<const uint32_t*>(src);
        } else {
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if (j + b < N) v |= (uint32_t)src[b] << (8 * b);
        }
      }
      s_e[pl * kMmdEld + w] = v;
    }
    // d2 of the thread's four entries of the tile: (e_row, e_col + 16 c) under energy, (e_row + 4 c, e_col) under rbf
    double d2[4] = {0.0, 0.0, 0.0, 0.0};
    cg_d4 dot = {0.0, 0.0, 0.0, 0.0};
    const int rb = wave >> 2, cb = wave & 3;      // rbf: the wave's block of the tile
    for (int dc = 0; dc < D; dc += kCgDChunk) {
      cg_stage<!kEnergy>(pre, dc, D, s_zi, s_mean, mean);
      if (dc + kCgDChunk < D)
        fetch(j0, dc + kCgDChunk);
      else if (jt + 1 < jt_hi)
        fetch(j0 + kCgCols, 0);
      if (kEnergy) {
        const int dn = D - dc < kCgDChunk ? D - dc : kCgDChunk;
        const float* __restrict__ ai = s_zi + (tid >> 4) * kCgZld;
        const float* __restrict__ bj = s_zj + (tid & 15) * kCgZld;
        for (int d = 0; d < dn; ++d) {
          const double a0 = (double)ai[d];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const double e0 = a0 - (double)bj[16 * c * kCgZld + d];
            d2[c] = fma(e0, e0, d2[c]);
          }
        }
      } else {
        cg_mfma(s_zi, s_mean, rb, cb, l15, l4, dot);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int li = kEnergy ? tid >> 4 : 16 * rb + l4 + 4 * c, lj = kEnergy ? (tid & 15) + 16 * c : 16 * cb + l15;
      const int gi = i0 + li, gj = j0 + lj;
      double k = 0.0;
      if (gi < N && gj < N && gi != gj) {
        if (kEnergy) {
          k = d2[c] > 0.0 ? -sqrt(d2[c]) : 0.0;
        } else {
          const double v = fmax(nrm[gi] + nrm[gj] - 2.0 * dot[c], 0.0);
          double s = 0.0;
          for (int q = 0; q < Q; ++q) s += exp(-gam.g[q] * v);
          k = s / (double)Q;
        }
      }
      s_k[li * kCgKld + lj] = k;
    }
    __syncthreads();
    if (tid < kCgRows) {
      const double* __restrict__ kr = s_k + tid * kCgKld;
      for (int j = 0; j < kCgCols; ++j) rs += kr[j];
    }
    if (wave_p < P) {      // (uniform in the wave: the MFMA runs with every lane on; a split past P is staged as 0)
      const double* __restrict__ k0 = s_k + l15 * kCgKld + l4;
      const uint32_t* __restrict__ we = s_e + (wave * NT * 16 + l15) * kMmdEld;
      const int sh = 8 * l4;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const double a0 = k0[4 * ks], a1 = k0[16 * kCgKld + 4 * ks];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          const double b = ((we[ct * 16 * kMmdEld + ks] >> sh) & 0xffu) ? 1.0 : 0.0;
          acc[0][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][ct], 0, 0, 0);
          acc[1][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][ct], 0, 0, 0);
        }
      }
    }
  }

  const size_t grp = (size_t)blockIdx.x * gridDim.y + slab;
  // a: a lane's eight rows in order, then the four lane groups
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    const int gp = wave_p + 16 * ct + l15;
    double s = 0.0;
    if (gp < P) {
      const uint8_t* __restrict__ e = E + (size_t)gp * N;
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int i = i0 + 16 * rb + l4 + 4 * g;
          if (i < N && e[i]) s += acc[rb][ct][g];
        }
      }
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (l4 == 0 && gp < P) part_a[grp * P + gp] = s;
    if (gp == 0) {      // column 0 of T: (K0 e_0)_i over the slab
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int i = i0 + 16 * rb + l4 + 4 * g;
          if (i < N) part_row_first[(size_t)slab * N + i] = acc[rb][ct][g];
        }
      }
    }
  }
  if (tid < kCgRows) {
    s_rs[tid] = rs;
    if (blockIdx.z == 0 && i0 + tid < N) part_row_all[(size_t)slab * N + i0 + tid] = rs;
  }
  __syncthreads();
  for (int pl = tid; pl < PC; pl += kCgBlock) {
    const int gp = p0 + pl;
    if (gp < P) {
      const uint8_t* __restrict__ e = E + (size_t)gp * N;
      double s = 0.0;
      for (int r = 0; r < kCgRows; ++r)
        if (i0 + r < N && e[i0 + r]) s += s_rs[r];
      part_b[grp * P + gp] = s;
    }
  }
  if (blockIdx.z == 0 && tid == 0) {
    double c = 0.0;
    for (int r = 0; r < kCgRows; ++r) c += s_rs[r];
    part_c[grp] = c;
  }
}

// workgroup p < P: n_p, the partials in index order, mmd2[p]; the workgroups behind them: row_all and row_first, 256 rows each
__global__ __launch_bounds__(kMmdSmallBlock) void mmd_finish(const uint8_t* __restrict__ E, const int N, const int P, const int groups,
                                                             const int slabs, const double* __restrict__ part_a,
                                                             const double* __restrict__ part_b, const double* __restrict__ part_c,
                                                             const double* __restrict__ part_row_all,
                                                             const double* __restrict__ part_row_first, double* __restrict__ mmd2,
                                                             double* __restrict__ row_all, double* __restrict__ row_first) {
  __shared__ double s_a[kMmdSmallBlock], s_b[kMmdSmallBlock], s_c[kMmdSmallBlock];
  __shared__ int s_n[kMmdSmallBlock];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= P) {
    const int i = ((int)blockIdx.x - P) * kMmdSmallBlock + tid;
    if (i < N) {
      double ra = 0.0, rf = 0.0;
      for (int s = 0; s < slabs; ++s) {
        ra += part_row_all[(size_t)s * N + i];
        rf += part_row_first[(size_t)s * N + i];
      }
      if (row_all) row_all[i] = ra;
      if (row_first) row_first[i] = rf;
    }
    return;
  }
  const int p = blockIdx.x;
  const uint8_t* __restrict__ e = E + (size_t)p * N;
  int cnt = 0;
  for (int i = tid; i < N; i += kMmdSmallBlock) cnt += e[i] ? 1 : 0;
  const int run = (groups + kMmdSmallBlock - 1) / kMmdSmallBlock;
  const int g_lo = tid * run, g_hi = g_lo + run < groups ? g_lo + run : groups;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int g = g_lo; g < g_hi; ++g) {
    a += part_a[(size_t)g * P + p];
    b += part_b[(size_t)g * P + p];
    c += part_c[g];
  }
  s_a[tid] = a;
  s_b[tid] = b;
  s_c[tid] = c;
  s_n[tid] = cnt;
  __syncthreads();
  if (tid == 0) {
    double A = 0.0, B = 0.0, Cc = 0.0;
    int n = 0;
    for (int t = 0; t < kMmdSmallBlock; ++t) {
      A += s_a[t];
      B += s_b[t];
      Cc += s_c[t];
      n += s_n[t];
    }
    const int m = N - n;
    double out = NAN;
    if (n >= 2 && m >= 2) {
      const double dn = (double)n, dm = (double)m;
      out = A / (dn * (dn - 1.0)) + (Cc - 2.0 * B + A) / (dm * (dm - 1.0)) - 2.0 * (B - A) / (dn * dm);
    }
    mmd2[p] = out;
  }
}

}  // namespace gmvae
