// gmvae_pca_*, gmvae_sym_eigh (include/gmvae_hip.h; host side: csrc/pca.hip): principal component analysis of N rows x [N][D] (fp32)
// and the small dense symmetric eigensolver under it.  Model independent.  The statement is tests/pca_ref.py:
//   mu = (1/N) sum_n x_n,  C = (1/(N - 1)) sum_n (x_n - mu)(x_n - mu)^T   (centred in fp64 BEFORE the product, never the expanded square)
//   D <= 128: C = U diag(w) U^T by cyclic Jacobi; components = the first k eigenvectors, eigenvalues descending
//   D  > 128: subspace iteration on the stored C from an orthonormal V0 [D][m]: n_iter times W = C V, G = W^T W = R R^T (Cholesky),
//             V = W R^-T; then W = C V, T = 1/2 (V^T W + W^T V) = Q diag(theta) Q^T by the same solver, components = the first k
//             columns of V Q, residual_j = |W q_j - theta_j V q_j|_2
// Every eigenvector is signed so that its entry of largest magnitude (the first such index) is positive.
// Kernels, in launch order (nothing synchronises with the host; every loop has a fixed trip count):
//   pca_moments:  a workgroup per (row slice, chunk of <= 256 columns); thread (r, d) adds the rows r, r + R, ... of column d in fp64,
//                 eight loads in flight, the R runs added in order (linprobe_moments' shape).
//   pca_mean:     a thread per column adds the slices in index order: mu.
//   pca_cov:      a workgroup owns one 64 x 64 macro-block (bi >= bj) of C and one slice of the rows.  Tiles of 64 rows of the two
//                 column blocks are staged as x - mu in fp64 (a row past the end, and a column past D, as 0); wave w owns the four
//                 16 x 16 blocks of block row w and multiplies them by v_mfma_f64_16x16x4_f64 in linprobe_gram's operand and result
//                 layout (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], result row (lane >> 4) + 4 g, column
//                 lane & 15); the sums stay in registers over the whole slice.  The number of slices comes from the number of
//                 macro-blocks (pca_plan): one macro-block (D <= 64) still gets kPcaCovTarget workgroups, and from 23 macro-block
//                 rows on (D > 1408) there is ONE slice, which writes C itself -- no partials.
//   pca_cov_fold: more than one slice: the owner of an entry adds the slices' partials in index order and scales by 1 / (N - 1).
//                 C is stored as the FULL matrix [D][D] in the workspace, the upper triangle a copy of the lower one written by
//                 the same owner (so the products C V below read rows of C), and bit-symmetric.
//   pca_stats:    one workgroup: tr C in a fixed order, the verdict word (ok) and info = 0.
//   D <= 128:     pca_dense: one workgroup, the solver on C.
//   D  > 128:     pca_gemm (W = C V), pca_orth (one workgroup: G = W^T W on the MFMA, mff_factor_lds of csrc/mixfit_common.hpp, the
//                 transposed inverse factor to the workspace), pca_gemm (V = W R^-T), n_iter times; then pca_gemm, pca_ritz (one
//                 workgroup: T, the solver, Q sorted by eigenvalue), pca_gemm twice (V Q, W Q) and pca_finish (a workgroup per
//                 component: the sign, the residual in a fixed order).  A pivot of G that is not > 0 (the data's rank is below m)
//                 clears the verdict word, sets info = 1 + the pivot's index and fills every output but mean, stats[0] and
//                 stats[2] with NaN; the later launches read the verdict and return (linprobe_setup's rule).
//   pca_transform: a workgroup owns a row slice and walks it in tiles of 32 rows; the component image [k][D] is streamed through LDS
//                 in chunks of 64 columns beside the tile's x - mu (fp64); a thread owns up to four (row quad, component) items,
//                 16 fp64 accumulators, added in ascending d, scaled and rounded once to fp32.
// The dense solver (pca_jacobi_lds; shared by gmvae_sym_eigh, pca_dense and pca_ritz): cyclic Jacobi in ONE workgroup of kMfBlock
// threads, round-robin ordering -- with ne = n rounded up to even, round r of a sweep pairs (ne - 1, r) and ((r + k) mod (ne - 1),
// (r - k) mod (ne - 1)) for k = 1 .. ne / 2 - 1: ne / 2 disjoint pairs, ne - 1 rounds per sweep; an index >= n is the bye of an odd
// n.  A pair (p < q) rotates by t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_qq - a_pp) / (2 a_pq), c = 1 / sqrt(t^2
// + 1), s = t c; a pair with a_pq == 0 is skipped.  The matrix lives in LDS as the FULL square [n][n | 1] (132,096 bytes at n =
// 128; not packed) and stays bit-symmetric: an item is the 2 x 2 block (pair k's rows, pair l's columns), k >= l, rotated from
// both sides in registers and written to its place and to its mirror image; the diagonal blocks take a_pp - t a_pq, a_qq + t a_pq
// and an exact 0.  The eigenvectors live in the workspace as ROWS [n][n] (both matrices do not fit in 160 KiB), rotated in the same
// phase: two barriers a round.  Exactly n_sweeps sweeps; offdiag = max |off-diagonal| / max |diagonal| afterwards (0 where the
// diagonal is 0, NaN where an entry is) is the convergence readout.
// One owner per sum, fixed-order fp64 folds, no float atomics: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mixfit_common.hpp"

namespace gmvae {

constexpr int kPcaMaxD = 4096;            // C is then 128 MiB of the workspace
constexpr int kPcaMaxM = 128;             // the dense solver's bound: the matrix in LDS
constexpr int kPcaMb = 64;                // the edge of a macro-block of C, and the rows of a staged tile
constexpr int kPcaMbPad = kPcaMb + 1;
constexpr int kPcaCovTarget = 512;        // workgroups pca_cov aims at: two a CU (66,560 bytes of LDS each)
constexpr int kPcaGramRows = 32;          // rows per staged tile of pca_gram_acc
constexpr int kPcaGramSlots = 9;          // 16 x 16 blocks a wave owns at most: 36 lower blocks at m = 128 over four waves
constexpr int kPcaGemmK = 32;             // the K chunk of pca_gemm
constexpr int kPcaTrTile = 32;            // rows per tile of pca_transform
constexpr int kPcaTrChunk = 64;           // ... and columns per chunk of the component image
constexpr int kPcaTrMaxGroups = 1024;
constexpr int kPcaAuxDoubles = 3 * 64 + kMfBlock + 2 * kPcaMaxM;      // the solver's c, s, t per pair; a reduction; w; the signs
constexpr int kPcaAuxInts = 2 * 64 + kPcaMaxM;                         // ... p, q per pair; the ranks

// the workspace, in doubles: the header (ok, info), mu [D], C [D][D], the moments' partials, the covariance partials, the solver's
// eigenvectors [m][m], and for D > 128 V, W, Y = V Q, Z = W Q [D][m] each, R^-T [m][m], Q sorted [m][m], theta [m]
struct PcaLayout {
  size_t mean, c, mpart, cpart, vt, v, w, y, z, cinvt, qs, theta, end;
};
struct PcaPlan {
  int mgroups, mper, mcw, mchunks;       // pca_moments: row slices, rows per slice, columns per chunk, chunks
  int nmb, nblk, slices, cper;           // pca_cov: macro-block rows, macro-blocks, row slices, rows per slice
  int tgroups, tper;                     // pca_transform
  size_t lds_solve, lds_orth, lds_tr;
};
static inline PcaPlan pca_plan(int64_t N, int D, int m, int k) {
  PcaPlan p;
  MfPlan s;
  mf_plan_groups(s, N, 64, kMfMaxGroups);
  p.mgroups = s.groups;
  p.mper = s.per_group;
  p.mcw = D < kMfBlock ? D : kMfBlock;
  p.mchunks = (D + p.mcw - 1) / p.mcw;
  p.nmb = (D + kPcaMb - 1) / kPcaMb;
  p.nblk = p.nmb * (p.nmb + 1) / 2;
  int64_t want = kPcaCovTarget / p.nblk;
  want = want < 1 ? 1 : want;
  mf_plan_groups(s, N, kPcaMb, want);
  p.slices = s.groups;
  p.cper = s.per_group;
  mf_plan_groups(s, N, kPcaTrTile, kPcaTrMaxGroups);
  p.tgroups = s.groups;
  p.tper = s.per_group;
  const size_t ms = (size_t)(m | 1), sq = (size_t)m * ms, st2 = 2 * (size_t)kPcaGramRows * ms, tri = (size_t)mff_tri(m);
  const size_t aux = 8 * (size_t)kPcaAuxDoubles + 4 * (size_t)kPcaAuxInts;
  p.lds_solve = aux + 8 * (sq > st2 ? sq : st2);                                         // 138,752 bytes at m = 128
  p.lds_orth = 8 * (tri + (tri > st2 / 2 ? tri : st2 / 2));                              // 132,096 bytes at m = 128
  p.lds_tr = 8 * ((size_t)(k + kPcaTrTile) * (kPcaTrChunk + 1));                         // 83,200 bytes at k = 128
  return p;
}
__host__ __device__ static inline PcaLayout pca_layout(int D, int m, int mgroups, int slices, int nblk) {
  PcaLayout o;
  const size_t dm = D > kPcaMaxM ? (size_t)D * m : 0;
  o.mean = 8;
  o.c = o.mean + (size_t)D;
  o.mpart = o.c + (size_t)D * D;
  o.cpart = o.mpart + (size_t)mgroups * D;
  o.vt = o.cpart + (slices > 1 ? (size_t)slices * nblk * kPcaMb * kPcaMb : 0);
  o.v = o.vt + (size_t)m * m;
  o.w = o.v + dm;
  o.y = o.w + dm;
  o.z = o.y + dm;
  o.cinvt = o.z + dm;
  o.qs = o.cinvt + (size_t)m * m;
  o.theta = o.qs + (size_t)m * m;
  o.end = o.theta + (size_t)m;
  return o;
}

// (bi, bj), bi >= bj, of entry b of a lower triangle packed by rows
__device__ __forceinline__ void pca_tri_decode(const int b, int& bi, int& bj) {
  bi = 0;
  bj = b;
  while (bj > bi) {
    bj -= bi + 1;
    ++bi;
  }
}

__global__ __launch_bounds__(kMfBlock) void pca_moments(const float* __restrict__ x, const int N, const int D, const int per_group,
                                                         const int cw, double* __restrict__ mpart) {
  __shared__ double s_red[kMfBlock];
  const int tid = threadIdx.x;
  const int64_t g_lo = (int64_t)blockIdx.x * per_group, g_hi = g_lo + per_group < N ? g_lo + per_group : N;
  const int R = kMfBlock / cw, r = tid / cw, d = blockIdx.y * cw + (tid - r * cw);
  double acc = 0.0;
  if (r < R && d < D) {
    for (int64_t n0 = g_lo + r; n0 < g_hi; n0 += 8 * R) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t n = n0 + (int64_t)u * R;
        v[u] = n < g_hi ? x[(size_t)n * D + d] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += (double)v[u];
    }
  }
  s_red[tid] = acc;
  __syncthreads();
  if (tid < cw && d < D) {
    double sx = 0.0;
    for (int q = 0; q < R; ++q) sx += s_red[q * cw + tid];
    mpart[(size_t)blockIdx.x * D + d] = sx;
  }
}

__global__ __launch_bounds__(kMfBlock) void pca_mean(const double* __restrict__ mpart, const int G, const int N, const int D,
                                                      double* __restrict__ mean, double* __restrict__ mean_out) {
  const int d = blockIdx.x * kMfBlock + threadIdx.x;
  if (d >= D) return;
  double a = 0.0;
  for (int g = 0; g < G; ++g) a += mpart[(size_t)g * D + d];
  a /= (double)N;
  mean[d] = a;
  mean_out[d] = a;
}

// entry (i, j) of macro-block (bi, bj): to C and to its mirror image, by the one owner of the entry on or below the diagonal
__device__ __forceinline__ void pca_cov_store(double* __restrict__ C, const int D, const int bi, const int bj, const int i, const int j,
                                              const double v) {
  const int gi = kPcaMb * bi + i, gj = kPcaMb * bj + j;
  if (gi < D && gj <= gi) {
    C[(size_t)gi * D + gj] = v;
    C[(size_t)gj * D + gi] = v;
  }
}

__global__ __launch_bounds__(kMfBlock) void pca_cov(const float* __restrict__ x, const int N, const int D, const double* __restrict__ mean,
                                                     const int per_group, const int slices, const double scale, double* __restrict__ C,
                                                     double* __restrict__ cpart) {
  extern __shared__ __attribute__((aligned(16))) char pca_smem[];
  double* const sI = reinterpret_cast<double*>(pca_smem);      // [64][65]: the tile's columns of block bi, centred
  int bi, bj;
  pca_tri_decode((int)blockIdx.x, bi, bj);
  double* const sJ = bi == bj ? sI : sI + kPcaMb * kPcaMbPad;   // ... and of block bj
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, nn = lane >> 4;
  const int col = tid & 63, rsub = tid >> 6, ci = kPcaMb * bi + col, cj = kPcaMb * bj + col;
  const double mi = ci < D ? mean[ci] : 0.0, mj = cj < D ? mean[cj] : 0.0;
  const int64_t g_lo = (int64_t)blockIdx.y * per_group, g_hi = g_lo + per_group < N ? g_lo + per_group : N;
  const int ncb = bi == bj ? wave + 1 : 4;      // (uniform in the wave) a diagonal macro-block: the blocks on or below the diagonal
  mff_d4 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc[cb] = mff_d4{0.0, 0.0, 0.0, 0.0};
  for (int64_t r0 = g_lo; r0 < g_hi; r0 += kPcaMb) {
    float vi[16], vj[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int64_t n = r0 + rsub + 4 * p;
      vi[p] = (n < g_hi && ci < D) ? x[(size_t)n * D + ci] : NAN;
      vj[p] = (bi != bj && n < g_hi && cj < D) ? x[(size_t)n * D + cj] : NAN;
    }
    __syncthreads();      // the previous tile's products have read the stage
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int r = rsub + 4 * p;
      const bool in = r0 + r < g_hi;
      sI[r * kPcaMbPad + col] = (in && ci < D) ? (double)vi[p] - mi : 0.0;
      if (bi != bj) sJ[r * kPcaMbPad + col] = (in && cj < D) ? (double)vj[p] - mj : 0.0;
    }
    __syncthreads();
    for (int n0 = 0; n0 < kPcaMb; n0 += 4) {
      const int m = n0 + nn;
      const double av = sI[m * kPcaMbPad + 16 * wave + l15];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        if (cb < ncb) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, sJ[m * kPcaMbPad + 16 * cb + l15], acc[cb], 0, 0, 0);
    }
  }
  double* const part = cpart + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kPcaMb * kPcaMb);
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = 16 * wave + nn + 4 * g, j = 16 * cb + l15;
      if (slices == 1)
        pca_cov_store(C, D, bi, bj, i, j, acc[cb][g] * scale);
      else
        part[i * kPcaMb + j] = acc[cb][g];
    }
}

__global__ __launch_bounds__(kMfBlock) void pca_cov_fold(const double* __restrict__ cpart, const int slices, const int D, const double scale,
                                                          double* __restrict__ C) {
  int bi, bj;
  pca_tri_decode((int)blockIdx.x, bi, bj);
  const int e = blockIdx.y * kMfBlock + threadIdx.x;
  const double* __restrict__ src = cpart + (size_t)blockIdx.x * (kPcaMb * kPcaMb) + e;
  const size_t stride = (size_t)gridDim.x * (kPcaMb * kPcaMb);
  double a = 0.0;
  for (int s = 0; s < slices; ++s) a += src[(size_t)s * stride];
  pca_cov_store(C, D, bi, bj, e / kPcaMb, e % kPcaMb, a * scale);
}

// one workgroup: tr C, the diagonal in strided runs added in order; the verdict word; the outputs that every path sets
__global__ __launch_bounds__(kMfBlock) void pca_stats(const double* __restrict__ C, const int N, const int D, double* __restrict__ hdr,
                                                       double* __restrict__ stats, int32_t* __restrict__ info_out) {
  __shared__ double s_red[kMfBlock];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int d = tid; d < D; d += kMfBlock) a += C[(size_t)d * D + d];
  s_red[tid] = a;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int q = 0; q < kMfBlock; ++q) t += s_red[q];
    stats[0] = t;
    stats[1] = 0.0;
    stats[2] = (double)N;
    stats[3] = 0.0;
    hdr[0] = 1.0;
    hdr[1] = 0.0;
    if (info_out) info_out[0] = 0;
  }
}

// The solver's LDS behind the matrix: c, s, t [64] each, a reduction [kMfBlock], w [128], the signs [128]; p, q [64] each, the ranks [128]
struct PcaAux {
  double *c, *s, *t, *red, *w, *sign;
  int *p, *q, *rank;
};
__device__ __forceinline__ PcaAux pca_aux(char* const base) {
  PcaAux o;
  o.c = reinterpret_cast<double*>(base);
  o.s = o.c + 64;
  o.t = o.s + 64;
  o.red = o.t + 64;
  o.w = o.red + kMfBlock;
  o.sign = o.w + kPcaMaxM;
  o.p = reinterpret_cast<int*>(o.sign + kPcaMaxM);
  o.q = o.p + 64;
  o.rank = o.q + 64;
  return o;
}

// Cyclic Jacobi on a [n][ns] (LDS, bit-symmetric on entry), the eigenvectors as the ROWS of Vt [n][n] (global).  Called behind a
// barrier; ends behind one, with w, rank (descending, ties by index), sign (of row i of Vt, if kSign) in `x` and offdiag returned.
template <bool kSign>
__device__ __forceinline__ double pca_jacobi_lds(double* const a, const int ns, const int n, const int n_sweeps, double* __restrict__ Vt,
                                                 const int tid, const PcaAux x) {
  for (int s = tid; s < n * n; s += kMfBlock) Vt[s] = (s / n == s % n) ? 1.0 : 0.0;
  const int ne = (n + 1) & ~1, np = ne >> 1, ring = ne - 1;
  __syncthreads();
  for (int sweep = 0; sweep < n_sweeps; ++sweep) {
    for (int r = 0; r < ring; ++r) {
      if (tid < np) {
        const int u = tid == 0 ? ne - 1 : (r + tid) % ring, v = tid == 0 ? r : (r - tid + ring) % ring;
        const int p = u < v ? u : v, q = u < v ? v : u;
        double c = 1.0, s = 0.0, t = 0.0;
        if (q < n) {
          const double apq = a[q * ns + p];
          if (apq != 0.0) {
            const double theta = (a[q * ns + q] - a[p * ns + p]) / (2.0 * apq);
            t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            c = 1.0 / sqrt(t * t + 1.0);
            s = t * c;
          }
        }
        x.c[tid] = c;
        x.s[tid] = s;
        x.t[tid] = t;
        x.p[tid] = p;
        x.q[tid] = q < n ? q : -1;      // (-1: the bye of an odd n; p alone is then a row and a column)
      }
      __syncthreads();
      for (int it = tid; it < np * np; it += kMfBlock) {
        const int k = it / np, l = it - k * np;
        if (l > k) continue;
        const int pk = x.p[k], qk = x.q[k], pl = x.p[l], ql = x.q[l];
        if (k == l) {
          if (qk < 0 || x.t[k] == 0.0) continue;
          const double apq = a[qk * ns + pk], t = x.t[k];
          a[pk * ns + pk] -= t * apq;
          a[qk * ns + qk] += t * apq;
          a[qk * ns + pk] = 0.0;
          a[pk * ns + qk] = 0.0;
          continue;
        }
        const double ck = x.c[k], sk = x.s[k], cl = x.c[l], sl = x.s[l];
        const double b00 = a[pk * ns + pl], b01 = ql >= 0 ? a[pk * ns + ql] : 0.0;
        const double b10 = qk >= 0 ? a[qk * ns + pl] : 0.0, b11 = (qk >= 0 && ql >= 0) ? a[qk * ns + ql] : 0.0;
        const double t00 = ck * b00 - sk * b10, t01 = ck * b01 - sk * b11, t10 = sk * b00 + ck * b10, t11 = sk * b01 + ck * b11;
        const double n00 = cl * t00 - sl * t01, n01 = sl * t00 + cl * t01, n10 = cl * t10 - sl * t11, n11 = sl * t10 + cl * t11;
        a[pk * ns + pl] = n00;
        a[pl * ns + pk] = n00;
        if (ql >= 0) {
          a[pk * ns + ql] = n01;
          a[ql * ns + pk] = n01;
        }
        if (qk >= 0) {
          a[qk * ns + pl] = n10;
          a[pl * ns + qk] = n10;
        }
        if (qk >= 0 && ql >= 0) {
          a[qk * ns + ql] = n11;
          a[ql * ns + qk] = n11;
        }
      }
      for (int it = tid; it < np * n; it += kMfBlock) {
        const int k = it / n, i = it - k * n, p = x.p[k], q = x.q[k];
        if (q < 0 || x.t[k] == 0.0) continue;
        const double c = x.c[k], s = x.s[k], vp = Vt[p * n + i], vq = Vt[q * n + i];
        Vt[p * n + i] = c * vp - s * vq;
        Vt[q * n + i] = s * vp + c * vq;
      }
      __syncthreads();
    }
  }
  // the readout: maxima do not depend on the order they are taken in
  double off = 0.0, dia = 0.0;
  bool bad = false;
  for (int s = tid; s < n * n; s += kMfBlock) {
    const int i = s / n, j = s - i * n;
    if (j > i) continue;
    const double v = fabs(a[i * ns + j]);
    bad = bad || v != v;
    if (i == j)
      dia = v > dia ? v : dia;
    else
      off = v > off ? v : off;
  }
  x.red[tid] = bad ? NAN : off;
  __syncthreads();
  if (tid == 0) {
    double m = 0.0;
    bool b = false;
    for (int q = 0; q < kMfBlock; ++q) {
      b = b || x.red[q] != x.red[q];
      m = x.red[q] > m ? x.red[q] : m;
    }
    x.c[0] = b ? NAN : m;
  }
  __syncthreads();
  off = x.c[0];
  __syncthreads();
  x.red[tid] = dia;
  if (tid < n) x.w[tid] = a[tid * ns + tid];
  __syncthreads();
  if (tid == 0) {
    double m = 0.0;
    for (int q = 0; q < kMfBlock; ++q) m = x.red[q] > m ? x.red[q] : m;
    x.c[0] = m;
  }
  if (tid < n) {
    const double wi = x.w[tid];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (x.w[j] > wi || (x.w[j] == wi && j < tid)) ? 1 : 0;
    x.rank[tid] = rank;
    double sg = 1.0;
    if (kSign) {
      const double* __restrict__ row = Vt + (size_t)tid * n;
      double best = -1.0;
      for (int j = 0; j < n; ++j) {
        const double v = row[j], m = fabs(v);
        if (m > best) {      // (strictly: the first index of the largest magnitude)
          best = m;
          sg = v < 0.0 ? -1.0 : 1.0;
        }
      }
    }
    x.sign[tid] = sg;
  }
  __syncthreads();
  dia = x.c[0];
  return off != off ? off : (dia > 0.0 ? off / dia : 0.0);
}

// a [n][ns] <- the lower triangle of src [n][n] and its mirror image
__device__ __forceinline__ void pca_load_sym(const double* __restrict__ src, const int n, const int ns, double* const a, const int tid) {
  for (int s = tid; s < n * n; s += kMfBlock) {
    const int i = s / n, j = s - i * n;
    a[i * ns + j] = j <= i ? src[s] : src[(size_t)j * n + i];
  }
}

// gmvae_sym_eigh: w_out descending, V_out [n][n] with the eigenvectors in its columns
__global__ __launch_bounds__(kMfBlock) void pca_eigh(const double* __restrict__ A, const int n, const int n_sweeps, double* __restrict__ Vt,
                                                      double* __restrict__ w_out, double* __restrict__ V_out,
                                                      double* __restrict__ offdiag_out) {
  extern __shared__ __attribute__((aligned(16))) char pca_smem[];
  const int tid = threadIdx.x, ns = n | 1;
  const PcaAux x = pca_aux(pca_smem);
  double* const a = reinterpret_cast<double*>(pca_smem + 8 * kPcaAuxDoubles + 4 * kPcaAuxInts);
  pca_load_sym(A, n, ns, a, tid);
  __syncthreads();
  const double off = pca_jacobi_lds<true>(a, ns, n, n_sweeps, Vt, tid, x);
  if (tid < n) w_out[x.rank[tid]] = x.w[tid];
  for (int s = tid; s < n * n; s += kMfBlock) {
    const int i = s / n, j = s - i * n;
    V_out[(size_t)j * n + x.rank[i]] = x.sign[i] * Vt[s];
  }
  if (tid == 0 && offdiag_out) *offdiag_out = off;
}

// D <= 128: the solver on C; components [k][D], variance [k], residual = 0, stats[1] = offdiag
__global__ __launch_bounds__(kMfBlock) void pca_dense(const double* __restrict__ C, const int D, const int k, const int n_sweeps,
                                                       double* __restrict__ Vt, double* __restrict__ components, double* __restrict__ variance,
                                                       double* __restrict__ residual, double* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) char pca_smem[];
  const int tid = threadIdx.x, ns = D | 1;
  const PcaAux x = pca_aux(pca_smem);
  double* const a = reinterpret_cast<double*>(pca_smem + 8 * kPcaAuxDoubles + 4 * kPcaAuxInts);
  pca_load_sym(C, D, ns, a, tid);
  __syncthreads();
  const double off = pca_jacobi_lds<true>(a, ns, D, n_sweeps, Vt, tid, x);
  if (tid < D && x.rank[tid] < k) {
    variance[x.rank[tid]] = x.w[tid];
    residual[x.rank[tid]] = 0.0;
  }
  for (int s = tid; s < D * D; s += kMfBlock) {
    const int i = s / D, j = s - i * D;
    if (x.rank[i] < k) components[(size_t)x.rank[i] * D + j] = x.sign[i] * Vt[s];
  }
  if (tid == 0) stats[1] = off;
}

// The lower 16 x 16 blocks of A^T B (and, kTwo, of B^T A) for A, B [D][m] in global memory, in registers: block b = wave + 4 slot of
// the triangle packed by rows.  Tiles of kPcaGramRows rows are staged in sA (and sB), [rows][m | 1]; a row past D as 0.
template <bool kTwo>
__device__ __forceinline__ void pca_gram_acc(const double* __restrict__ A, const double* __restrict__ B, const int D, const int m,
                                             double* const sA, double* const sB, const int tid, mff_d4 (&acc1)[kPcaGramSlots],
                                             mff_d4 (&acc2)[kPcaGramSlots]) {
  const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, nn = lane >> 4, ms = m | 1, nb = (m + 15) >> 4, nblk = nb * (nb + 1) / 2;
#pragma unroll
  for (int sl = 0; sl < kPcaGramSlots; ++sl) {
    acc1[sl] = mff_d4{0.0, 0.0, 0.0, 0.0};
    acc2[sl] = mff_d4{0.0, 0.0, 0.0, 0.0};
  }
  for (int r0 = 0; r0 < D; r0 += kPcaGramRows) {
    __syncthreads();
    for (int s = tid; s < kPcaGramRows * m; s += kMfBlock) {
      const int r = s / m, c = s - r * m;
      const bool in = r0 + r < D;
      sA[r * ms + c] = in ? A[(size_t)(r0 + r) * m + c] : 0.0;
      if (kTwo) sB[r * ms + c] = in ? B[(size_t)(r0 + r) * m + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int sl = 0; sl < kPcaGramSlots; ++sl) {
      const int b = wave + 4 * sl;
      if (b < nblk) {      // (uniform in the wave)
        int bi, bj;
        pca_tri_decode(b, bi, bj);
        const int ia = 16 * bi + l15, ib = 16 * bj + l15;
        for (int n0 = 0; n0 < kPcaGramRows; n0 += 4) {
          const int row = (n0 + nn) * ms;
          const double a_i = ia < m ? sA[row + ia] : 0.0, b_j = ib < m ? sB[row + ib] : 0.0;
          acc1[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_i, b_j, acc1[sl], 0, 0, 0);
          if (kTwo) {
            const double b_i = ia < m ? sB[row + ia] : 0.0, a_j = ib < m ? sA[row + ib] : 0.0;
            acc2[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(b_i, a_j, acc2[sl], 0, 0, 0);
          }
        }
      }
    }
  }
  __syncthreads();      // the stage may be overwritten
}

__device__ __forceinline__ void pca_fail_fill(const int tid, const int D, const int k, double* __restrict__ components,
                                              double* __restrict__ variance, double* __restrict__ residual, double* __restrict__ stats) {
  for (size_t s = tid; s < (size_t)k * D; s += kMfBlock) components[s] = NAN;
  if (tid < k) {
    variance[tid] = NAN;
    residual[tid] = NAN;
  }
  if (tid == 0) {
    stats[1] = NAN;
    stats[3] = NAN;
  }
}

// one workgroup: G = W^T W, its Cholesky factor R and R^-1 (mff_factor_lds); cinvt [t][j] = R^-1[j][t], so that V = W cinvt
__global__ __launch_bounds__(kMfBlock) void pca_orth(double* __restrict__ hdr, const double* __restrict__ W, const int D, const int m,
                                                      const int k, double* __restrict__ cinvt, double* __restrict__ components,
                                                      double* __restrict__ variance, double* __restrict__ residual, double* __restrict__ stats,
                                                      int32_t* __restrict__ info_out) {
  extern __shared__ __attribute__((aligned(16))) char pca_smem[];
  if (hdr[0] == 0.0) return;      // an earlier factorisation failed (every thread reads the same verdict)
  const int tid = threadIdx.x, P = mff_tri(m), wave = tid >> 6, lane = tid & 63, l15 = lane & 15, nn = lane >> 4;
  double* const a = reinterpret_cast<double*>(pca_smem);      // [P]: G, then R
  double* const xi = a + P;                                   // [P]: the stage, then the identity, then R^-1
  mff_d4 acc[kPcaGramSlots], unused[kPcaGramSlots];
  pca_gram_acc<false>(W, W, D, m, xi, xi, tid, acc, unused);
  const int nb = (m + 15) >> 4, nblk = nb * (nb + 1) / 2;
#pragma unroll
  for (int sl = 0; sl < kPcaGramSlots; ++sl) {
    const int b = wave + 4 * sl;
    if (b < nblk) {
      int bi, bj;
      pca_tri_decode(b, bi, bj);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = 16 * bi + nn + 4 * g, j = 16 * bj + l15;
        if (i < m && j <= i) a[mff_tri(i) + j] = acc[sl][g];
      }
    }
  }
  for (int s = tid; s < m * m; s += kMfBlock) {
    const int i = s / m, j = s - i * m;
    if (j <= i) xi[mff_tri(i) + j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  double sum_ln;
  const int info = mff_factor_lds(a, xi, m, tid, sum_ln);
  __syncthreads();
  if (info != 0) {
    pca_fail_fill(tid, D, k, components, variance, residual, stats);
    if (tid == 0) {
      hdr[0] = 0.0;
      hdr[1] = (double)info;
      if (info_out) info_out[0] = info;
    }
    return;
  }
  for (int s = tid; s < m * m; s += kMfBlock) {
    const int t = s / m, j = s - t * m;
    cinvt[s] = t <= j ? xi[mff_tri(j) + t] : 0.0;
  }
}

// one workgroup: T = 1/2 (V^T W + W^T V), the solver; theta descending and qs [t][rank] = the eigenvectors in columns (unsigned: the
// sign belongs to the component V q, pca_finish)
__global__ __launch_bounds__(kMfBlock) void pca_ritz(const double* __restrict__ hdr, const double* __restrict__ V, const double* __restrict__ W,
                                                      const int D, const int m, const int n_sweeps, double* __restrict__ Vt,
                                                      double* __restrict__ qs, double* __restrict__ theta, double* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) char pca_smem[];
  if (hdr[0] == 0.0) return;
  const int tid = threadIdx.x, ns = m | 1, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, nn = lane >> 4;
  const PcaAux x = pca_aux(pca_smem);
  double* const a = reinterpret_cast<double*>(pca_smem + 8 * kPcaAuxDoubles + 4 * kPcaAuxInts);
  mff_d4 acc1[kPcaGramSlots], acc2[kPcaGramSlots];
  pca_gram_acc<true>(V, W, D, m, a, a + kPcaGramRows * ns, tid, acc1, acc2);
  const int nb = (m + 15) >> 4, nblk = nb * (nb + 1) / 2;
#pragma unroll
  for (int sl = 0; sl < kPcaGramSlots; ++sl) {
    const int b = wave + 4 * sl;
    if (b < nblk) {
      int bi, bj;
      pca_tri_decode(b, bi, bj);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = 16 * bi + nn + 4 * g, j = 16 * bj + l15;
        if (i < m && j <= i) {
          const double v = 0.5 * (acc1[sl][g] + acc2[sl][g]);
          a[i * ns + j] = v;
          a[j * ns + i] = v;
        }
      }
    }
  }
  __syncthreads();
  const double off = pca_jacobi_lds<false>(a, ns, m, n_sweeps, Vt, tid, x);
  if (tid < m) theta[x.rank[tid]] = x.w[tid];
  for (int s = tid; s < m * m; s += kMfBlock) {
    const int i = s / m, t = s - i * m;
    qs[(size_t)t * m + x.rank[i]] = Vt[s];
  }
  if (tid == 0) stats[1] = off;
}

// Out [rows][ldo] (columns col0 .. col0 + 63 of `cols`) = A [rows][lda] (K columns) . B [K][ldb]: a workgroup owns 64 rows and 64
// columns, wave w the 16 rows of block row w; A and B are staged in chunks of kPcaGemmK of the summed index (entries past the edges
// as 0) and multiplied on the fp64 MFMA, the chunks in ascending order.
__global__ __launch_bounds__(kMfBlock) void pca_gemm(const double* __restrict__ hdr, const double* __restrict__ A, const int lda,
                                                      const double* __restrict__ B, const int ldb, double* __restrict__ Out, const int ldo,
                                                      const int rows, const int K, const int cols) {
  __shared__ __attribute__((aligned(16))) double sA[kPcaMb * (kPcaGemmK + 1)];
  __shared__ __attribute__((aligned(16))) double sB[kPcaGemmK * kPcaMbPad];
  if (hdr[0] == 0.0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, nn = lane >> 4;
  const int row0 = blockIdx.x * kPcaMb, col0 = blockIdx.y * kPcaMb;
  mff_d4 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc[cb] = mff_d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += kPcaGemmK) {
    __syncthreads();
    for (int s = tid; s < kPcaMb * kPcaGemmK; s += kMfBlock) {
      const int r = s / kPcaGemmK, c = s - r * kPcaGemmK;
      sA[r * (kPcaGemmK + 1) + c] = (row0 + r < rows && k0 + c < K) ? A[(size_t)(row0 + r) * lda + k0 + c] : 0.0;
    }
    for (int s = tid; s < kPcaGemmK * kPcaMb; s += kMfBlock) {
      const int r = s / kPcaMb, c = s - r * kPcaMb;
      sB[r * kPcaMbPad + c] = (k0 + r < K && col0 + c < cols) ? B[(size_t)(k0 + r) * ldb + col0 + c] : 0.0;
    }
    __syncthreads();
    for (int kk = 0; kk < kPcaGemmK; kk += 4) {
      const double av = sA[(16 * wave + l15) * (kPcaGemmK + 1) + kk + nn];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, sB[(kk + nn) * kPcaMbPad + 16 * cb + l15], acc[cb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = row0 + 16 * wave + nn + 4 * g, j = col0 + 16 * cb + l15;
      if (i < rows && j < cols) Out[(size_t)i * ldo + j] = acc[cb][g];
    }
}

// a workgroup per component j: the sign from Y[:, j] = V q_j, the residual |Z[:, j] - theta_j Y[:, j]|_2 (strided runs, then the runs in
// order), the outputs
__global__ __launch_bounds__(kMfBlock) void pca_finish(const double* __restrict__ hdr, const double* __restrict__ Y, const double* __restrict__ Z,
                                                        const double* __restrict__ theta, const int D, const int m,
                                                        double* __restrict__ components, double* __restrict__ variance,
                                                        double* __restrict__ residual) {
  __shared__ double s_val[kMfBlock];
  __shared__ int s_idx[kMfBlock];
  __shared__ double s_sign;
  if (hdr[0] == 0.0) return;
  const int tid = threadIdx.x, j = blockIdx.x;
  const double th = theta[j];
  double best = -1.0, r2 = 0.0;
  int arg = 0;
  for (int d = tid; d < D; d += kMfBlock) {
    const double y = Y[(size_t)d * m + j], z = Z[(size_t)d * m + j] - th * y, mag = fabs(y);
    r2 = fma(z, z, r2);
    if (mag > best) {
      best = mag;
      arg = d;
    }
  }
  s_val[tid] = best;
  s_idx[tid] = arg;
  __syncthreads();
  if (tid == 0) {
    double b = -1.0;
    int at = 0;
    for (int q = 0; q < kMfBlock; ++q)
      if (s_val[q] > b || (s_val[q] == b && s_idx[q] < at)) {
        b = s_val[q];
        at = s_idx[q];
      }
    s_sign = Y[(size_t)at * m + j] < 0.0 ? -1.0 : 1.0;
  }
  __syncthreads();
  s_val[tid] = r2;
  __syncthreads();
  const double sg = s_sign;
  for (int d = tid; d < D; d += kMfBlock) components[(size_t)j * D + d] = sg * Y[(size_t)d * m + j];
  if (tid == 0) {
    double t = 0.0;
    for (int q = 0; q < kMfBlock; ++q) t += s_val[q];
    residual[j] = sqrt(t);
    variance[j] = th;
  }
}

// z_out [N][k] = ((x - mean) . components^T) . scale, fp32
__global__ __launch_bounds__(kMfBlock) void pca_transform(const float* __restrict__ x, const int N, const int D, const int k,
                                                           const double* __restrict__ mean, const double* __restrict__ components,
                                                           const double* __restrict__ scale, const int per_group, float* __restrict__ z_out) {
  extern __shared__ __attribute__((aligned(16))) char pca_smem[];
  constexpr int cs = kPcaTrChunk + 1, quads = kPcaTrTile / 4;
  double* const s_c = reinterpret_cast<double*>(pca_smem);      // [k][65]: a chunk of the component image
  double* const s_x = s_c + k * cs;                             // [32][65]: the tile's x - mean in that chunk
  const int tid = threadIdx.x;
  const int64_t g_lo = (int64_t)blockIdx.x * per_group, g_hi = g_lo + per_group < N ? g_lo + per_group : N;
  for (int64_t r0 = g_lo; r0 < g_hi; r0 += kPcaTrTile) {
    const int rows = (int)(g_hi - r0 < kPcaTrTile ? g_hi - r0 : kPcaTrTile);
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int d0 = 0; d0 < D; d0 += kPcaTrChunk) {
      const int dc = D - d0 < kPcaTrChunk ? D - d0 : kPcaTrChunk;
      __syncthreads();
      for (int s = tid; s < k * kPcaTrChunk; s += kMfBlock) {
        const int j = s >> 6, d = s & 63;
        s_c[j * cs + d] = d < dc ? components[(size_t)j * D + d0 + d] : 0.0;
      }
      for (int s = tid; s < kPcaTrTile * kPcaTrChunk; s += kMfBlock) {
        const int r = s >> 6, d = s & 63;
        s_x[r * cs + d] = (r < rows && d < dc) ? (double)x[(size_t)(r0 + r) * D + d0 + d] - mean[d0 + d] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int it = tid + u * kMfBlock;      // item g k + j: the rows 4 g .. 4 g + 3 of component j
        if (it < quads * k) {
          const int g = it / k, j = it - g * k;
          const double* __restrict__ cj = s_c + j * cs;
          const double* __restrict__ x0 = s_x + 4 * g * cs;
          for (int d = 0; d < kPcaTrChunk; ++d) {
            const double c = cj[d];
            acc[u][0] = fma(x0[d], c, acc[u][0]);
            acc[u][1] = fma(x0[cs + d], c, acc[u][1]);
            acc[u][2] = fma(x0[2 * cs + d], c, acc[u][2]);
            acc[u][3] = fma(x0[3 * cs + d], c, acc[u][3]);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = tid + u * kMfBlock;
      if (it < quads * k) {
        const int g = it / k, j = it - g * k;
        const double sc = scale ? scale[j] : 1.0;
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (4 * g + v < rows) z_out[(size_t)(r0 + 4 * g + v) * k + j] = (float)(acc[u][v] * sc);
      }
    }
  }
}

}  // namespace gmvae
