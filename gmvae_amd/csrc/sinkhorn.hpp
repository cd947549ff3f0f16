// gmvae_sinkhorn (include/gmvae_hip.h; host side: csrc/sinkhorn.hip): the debiased Sinkhorn divergence (Genevay et al. 2018; Feydy
// et al. 2019) between two weighted samples x [n][D] and y [m][D] under the cost C(u, v) = 1/2 |u - v|^2.  Model independent.
// The statement is tests/sinkhorn_ref.py:
//   softmin_e(pts, h, w)(u) = -e log sum_j w_j exp((h_j - C(u, pts_j)) / e)
//   all four potentials start at 0; for t < T, e = eps[t]:
//     half A: f <- softmin(y, g, b) at x;  p <- (p + softmin(x, p, a) at x) / 2;  q <- (q + softmin(y, q, b) at y) / 2
//     half B: g <- softmin(x, f, a) at y;  p and q once more
//   last pass at e = eps[T]: f' = softmin(y, g, b) at x, p' = softmin(x, p, a) at x, q' = softmin(y, q, b) at y, none averaged
//   part_x = <a, f' - p'>, part_y = <b, g - q'>, S = part_x + part_y, marginal_err = max_i |expm1((f_i - f'_i) / eps[T])|
// Nothing n m in memory, nothing synchronises with the host, e is read from the device.  The cost comes from the expanded square
// (n_i + n_j) / 2 - zc_i . zc_j on the rows centred by the pooled mean (fp64; n_i = |zc_i|^2), clamped at 0, the dot products on
// v_mfma_f64_16x16x4_f64 -- csrc/twosample.hpp's form for rbf, and its three launches in front (sk_mean_part, sk_mean_fold,
// sk_norms over the pooled rows: x's, then y's); sk_logw leaves log w - log sum w and sum w of both samples.
// A softmin is a row-wise log-sum-exp over a cost matrix.  The two or three of a half-step depend on nothing of each other, so
// they are the PROBLEMS of one launch (blockIdx.z): a problem is (the rows it is evaluated at, the columns it sums over, h, log w),
// rows and columns each a range of the pooled rows.
// sk_tiles: a workgroup of eight waves owns kSkRows = 32 rows i of its problem and a slab of column tiles of kSkCols = 64 rows j
// (blockIdx.y; the slabs follow from n and m alone, sk_plan; a problem with fewer tiles than slabs leaves its last slabs empty:
// (-inf, 0)).  A workgroup whose row tile lies past its problem's rows leaves before any barrier.  Per column tile:
//   gram:   D in chunks of kSkDChunk = 32 staged as fp32 [32][33] and [64][33] (and the mean's chunk), each chunk loaded into
//           registers while the one before it is summed; wave w owns the 16 x 16 block (w >> 2, w & 3) of the tile, eight MFMA
//           steps a chunk, the operands centred on the way in (A: lane & 15 the row, lane >> 4 the dimension of the step; D: entry
//           c of a lane is row (lane >> 4) + 4 c, column lane & 15);
//   s tile: s_ij = logw_j + (h_j - C_ij) / e into the tile [32][65] (fp64); C_ii = 0 exactly on a symmetric problem, -inf in a
//           column past the end;
//   max:    thread i < 32 takes its row's largest s of the tile and with it the row's new running maximum M';
//   exp:    every thread turns its four entries into exp(s - M') (fp64 exp), 0 for -inf;
//   sum:    thread i < 32 adds its row of the tile in ascending j and folds it in: sum <- sum exp(M - M') + tile, M <- M'.
// At the end the row's (M, sum) over the slab goes to [problem][slab][row].
// sk_fold: a thread per row and problem merges the slabs' pairs in slab order (an empty pair is skipped), applies -e (log sum +
// M), averages with the old value on the symmetric problems and writes the potential -- in place: the tile launch that read it
// has finished.  On the last pass it also leaves |expm1((f_i - f'_i) / e)| per row.
// sk_finish: one workgroup: the two weighted sums (256 runs of consecutive rows, then the runs in order) and the largest error.
// One owner per output, fixed-order fp64 sums, no float atomics: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace gmvae {

constexpr int kSkBlock = 512;             // sk_tiles: eight waves
constexpr int kSkSmallBlock = 256;        // every other kernel here
constexpr int kSkRows = 32;               // rows i of a workgroup: two 16-row MFMA blocks
constexpr int kSkCols = 64;               // rows j of a column tile: four 16-column MFMA blocks
constexpr int kSkDChunk = 32;             // dimensions staged at a time
constexpr int kSkStage = (kSkRows + kSkCols) * kSkDChunk / kSkBlock;      // floats of a chunk a thread of sk_tiles stages
constexpr int kSkMaxSlabs = 16;
constexpr int kSkFillGroups = 256;        // the slabs fill about this many workgroups a problem where the row tiles alone do not
constexpr int kSkMeanSlices = 64;         // row slices of the mean, 1024 rows each at least
constexpr int kSkKld = kSkCols + 1;       // the s tile's leading dimension (doubles)
constexpr int kSkZld = kSkDChunk + 1;     // the staged rows' (floats)
constexpr int kSkProblems = 3;

typedef double sk_d4 __attribute__((ext_vector_type(4)));

// the launches' shape: the slabs and slices, and so the order of every sum, follow from (n, m) alone
struct SkPlan {
  int R;               // max(n, m): the rows of the larger problem
  int row_tiles;       // of the larger problem: the grid's x
  int slabs;
  int mean_slices, rows_per_slice;
};
__host__ __device__ static inline SkPlan sk_plan(int n, int m) {
  SkPlan p;
  p.R = n > m ? n : m;
  p.row_tiles = (p.R + kSkRows - 1) / kSkRows;
  const int col_tiles = (p.R + kSkCols - 1) / kSkCols;
  int s = p.row_tiles >= kSkFillGroups ? 1 : (kSkFillGroups + p.row_tiles - 1) / p.row_tiles;
  s = s > kSkMaxSlabs ? kSkMaxSlabs : s;
  p.slabs = s > col_tiles ? col_tiles : s;
  const int N = n + m;
  int ms = (N + 1023) / 1024;
  ms = ms > kSkMeanSlices ? kSkMeanSlices : ms;
  p.rows_per_slice = (N + ms - 1) / ms;
  p.mean_slices = (N + p.rows_per_slice - 1) / p.rows_per_slice;
  return p;
}

// the workspace, in doubles: the slabs' maxima and sums [3][slabs][R] each, the last pass's error per row of x [n], the
// normalised log-weights [n + m] (x's, then y's), sum a and sum b, the centred rows' squared norms [n + m], the mean's slices
// [mean_slices][D] and the mean [D]
struct SkLayout {
  size_t part_max, part_sum, err, logw, wsum, nrm, mean_part, mean, end;
};
__host__ __device__ static inline SkLayout sk_layout(const SkPlan& p, int n, int m, int D) {
  SkLayout o;
  o.part_max = 0;
  o.part_sum = o.part_max + (size_t)kSkProblems * p.slabs * p.R;
  o.err = o.part_sum + (size_t)kSkProblems * p.slabs * p.R;
  o.logw = o.err + (size_t)n;
  o.wsum = o.logw + (size_t)n + m;
  o.nrm = o.wsum + 2;
  o.mean_part = o.nrm + (size_t)n + m;
  o.mean = o.mean_part + (size_t)p.mean_slices * D;
  o.end = o.mean + (size_t)D;
  return o;
}

// a softmin of a half-step: evaluated at the pooled rows [row_off, row_off + row_cnt), summed over [col_off, col_off + col_cnt)
struct SkProb {
  int row_off, row_cnt, col_off, col_cnt;
  int tiles_per_slab, col_tiles, sym, avg;      // sym: rows and columns are the same points; avg: dst <- (dst + softmin) / 2
  const double* h;                              // [col_cnt]: the potential inside the sum
  const double* logw;                           // [col_cnt]
  double* dst;                                  // [row_cnt]
  double* err;                                  // [row_cnt] or NULL: |expm1((dst_old - softmin) / e)|
};
struct SkProbs {
  SkProb p[kSkProblems];
};
__device__ static inline SkProb sk_pick(const SkProbs& P, const int z) { return z == 0 ? P.p[0] : z == 1 ? P.p[1] : P.p[2]; }

// pooled row g < n + m, dimension d
__device__ static inline float sk_at(const float* __restrict__ x, const int n, const float* __restrict__ y, const int D, const int g,
                                     const int d) {
  return g < n ? x[(size_t)g * D + d] : y[(size_t)(g - n) * D + d];
}

// the pooled mean, first pass: workgroup (x, y) adds the rows of slice y in 64 columns; thread (r, c) the rows r, r + 4, ... in order
__global__ __launch_bounds__(kSkSmallBlock) void sk_mean_part(const float* __restrict__ x, const int n, const float* __restrict__ y, const int m,
                                                               const int D, const int rows_per_slice, double* __restrict__ part) {
  __shared__ double s[4][64];
  const int tid = threadIdx.x, r = tid >> 6, cl = tid & 63, c = blockIdx.x * 64 + cl, N = n + m;
  const int lo = blockIdx.y * rows_per_slice, hi = lo + rows_per_slice < N ? lo + rows_per_slice : N;
  double a = 0.0;
  if (c < D)
    for (int i = lo + r; i < hi; i += 4) a += (double)sk_at(x, n, y, D, i, c);
  s[r][cl] = a;
  __syncthreads();
  if (r == 0 && c < D) part[(size_t)blockIdx.y * D + c] = ((s[0][cl] + s[1][cl]) + s[2][cl]) + s[3][cl];
}

// ... second pass: the slices in order
__global__ __launch_bounds__(kSkSmallBlock) void sk_mean_fold(const double* __restrict__ part, const int slices, const int N, const int D,
                                                               double* __restrict__ mean) {
  const int d = blockIdx.x * kSkSmallBlock + threadIdx.x;
  if (d >= D) return;
  double a = 0.0;
  for (int s = 0; s < slices; ++s) a += part[(size_t)s * D + d];
  mean[d] = a / (double)N;
}

// |z_i - mean|^2 of the pooled rows: a wave per row, a lane the dimensions lane, lane + 64, ... in order, then the lanes by six
// exchanges
__global__ __launch_bounds__(kSkSmallBlock) void sk_norms(const float* __restrict__ x, const int n, const float* __restrict__ y, const int m,
                                                           const int D, const double* __restrict__ mean, double* __restrict__ nrm) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (kSkSmallBlock / 64) + (threadIdx.x >> 6);
  if (i >= n + m) return;      // (uniform in the wave)
  double a = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double e = (double)sk_at(x, n, y, D, i, d) - mean[d];
    a = fma(e, e, a);
  }
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) a += __shfl_xor(a, k);
  if (lane == 0) nrm[i] = a;
}

// workgroup 0: a [n] -> logw[0 .. n), wsum[0]; workgroup 1: b [m] -> logw[n ..), wsum[1].  The sum: 256 runs of consecutive
// entries, then the runs in order.  No weights: uniform, log w = -log count and the sum 1.
__global__ __launch_bounds__(kSkSmallBlock) void sk_logw(const double* __restrict__ a, const int n, const double* __restrict__ b, const int m,
                                                          double* __restrict__ logw, double* __restrict__ wsum) {
  __shared__ double s_run[kSkSmallBlock];
  __shared__ double s_tot;
  const int tid = threadIdx.x, second = blockIdx.x;
  const double* __restrict__ w = second ? b : a;
  const int cnt = second ? m : n;
  double* __restrict__ out = logw + (second ? n : 0);
  if (!w) {      // (uniform in the workgroup)
    const double l = -log((double)cnt);
    for (int i = tid; i < cnt; i += kSkSmallBlock) out[i] = l;
    if (tid == 0) wsum[second] = 1.0;
    return;
  }
  const int run = (cnt + kSkSmallBlock - 1) / kSkSmallBlock;
  const int lo = tid * run < cnt ? tid * run : cnt, hi = lo + run < cnt ? lo + run : cnt;
  double s = 0.0;
  for (int i = lo; i < hi; ++i) s += w[i];
  s_run[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < kSkSmallBlock; ++k) t += s_run[k];
    s_tot = t;
    wsum[second] = t;
  }
  __syncthreads();
  const double lt = log(s_tot);
  for (int i = tid; i < cnt; i += kSkSmallBlock) out[i] = log(w[i]) - lt;
}

__global__ __launch_bounds__(kSkBlock) void sk_tiles(const float* __restrict__ x, const int n, const float* __restrict__ y, const int D,
                                                      const SkProbs probs, const int slabs, const int R, const double* __restrict__ eps,
                                                      const double* __restrict__ mean, const double* __restrict__ nrm,
                                                      double* __restrict__ part_max, double* __restrict__ part_sum) {
  __shared__ double s_k[kSkRows * kSkKld];      // the s tile, then its exponentials
  __shared__ double s_mean[kSkDChunk];
  __shared__ double s_h[kSkCols], s_lw[kSkCols], s_nj[kSkCols];      // the tile's columns: h, log w, the squared norm
  __shared__ double s_ni[kSkRows], s_mx[kSkRows];                    // the rows' squared norms and new running maxima
  __shared__ float s_zi[(kSkRows + kSkCols) * kSkZld];               // [kSkRows][kSkZld], then s_zj [kSkCols][kSkZld]
  float* const s_zj = s_zi + kSkRows * kSkZld;

  const SkProb pb = sk_pick(probs, blockIdx.z);
  const int i0 = blockIdx.x * kSkRows;
  if (i0 >= pb.row_cnt) return;      // (uniform in the workgroup, before any barrier: the grid is sized by the larger problem)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int slab = blockIdx.y;
  const int jt_lo = slab * pb.tiles_per_slab;
  const int jt_hi = jt_lo + pb.tiles_per_slab < pb.col_tiles ? jt_lo + pb.tiles_per_slab : pb.col_tiles;
  const double inv_eps = 1.0 / eps[0];
  const int rb = wave >> 2, cb = wave & 3;      // the wave's block of the tile

  double M = -INFINITY, S = 0.0;      // (threads 0 .. 31: the row's running maximum and sum over the slab)
  if (tid < kSkRows) s_ni[tid] = i0 + tid < pb.row_cnt ? nrm[pb.row_off + i0 + tid] : 0.0;

  // a chunk of kSkDChunk dimensions of the 32 rows i and the 64 rows j, kSkStage floats a thread: loaded into registers a chunk
  // ahead, so that the loads' latency runs under the sums (a row past the end and a dimension past D as 0)
  float pre[kSkStage];
  auto fetch = [&](const int j0, const int dc) {
#pragma unroll
    for (int u = 0; u < kSkStage; ++u) {
      const int s = tid + u * kSkBlock, r = s / kSkDChunk, d = dc + (s % kSkDChunk);
      const int local = r < kSkRows ? i0 + r : j0 + (r - kSkRows);
      const bool ok = (r < kSkRows ? local < pb.row_cnt : local < pb.col_cnt) && d < D;
      pre[u] = ok ? sk_at(x, n, y, D, (r < kSkRows ? pb.row_off : pb.col_off) + local, d) : 0.f;
    }
  };
  if (jt_lo < jt_hi) fetch(jt_lo * kSkCols, 0);

  for (int jt = jt_lo; jt < jt_hi; ++jt) {
    const int j0 = jt * kSkCols;
    __syncthreads();      // the previous tile's sums have read s_k, its s tile s_h, s_lw and s_nj
    if (tid < kSkCols) {
      const int j = j0 + tid;
      const bool ok = j < pb.col_cnt;
      s_h[tid] = ok ? pb.h[j] : 0.0;
      s_lw[tid] = ok ? pb.logw[j] : -INFINITY;
      s_nj[tid] = ok ? nrm[pb.col_off + j] : 0.0;
    }
    sk_d4 dot = {0.0, 0.0, 0.0, 0.0};
    for (int dc = 0; dc < D; dc += kSkDChunk) {
      __syncthreads();      // the previous chunk's sums have read s_zi and s_zj
#pragma unroll
      for (int u = 0; u < kSkStage; ++u) {
        const int s = tid + u * kSkBlock;
        s_zi[(s / kSkDChunk) * kSkZld + (s % kSkDChunk)] = pre[u];      // (s_zj follows s_zi)
      }
      if (tid < kSkDChunk) s_mean[tid] = dc + tid < D ? mean[dc + tid] : 0.0;
      __syncthreads();
      // the next chunk -- of this tile or the first of the next -- is on its way while this one is summed
      if (dc + kSkDChunk < D)
        fetch(j0, dc + kSkDChunk);
      else if (jt + 1 < jt_hi)
        fetch(j0 + kSkCols, 0);
      const float* __restrict__ ai = s_zi + (16 * rb + l15) * kSkZld + l4;
      const float* __restrict__ bj = s_zj + (16 * cb + l15) * kSkZld + l4;
#pragma unroll
      for (int kk = 0; kk < kSkDChunk / 4; ++kk) {      // (a dimension past D: 0 - 0; a row past the end: -mean, never used)
        const double mu = s_mean[4 * kk + l4];
        dot = __builtin_amdgcn_mfma_f64_16x16x4f64((double)ai[4 * kk] - mu, (double)bj[4 * kk] - mu, dot, 0, 0, 0);
      }
    }
    // the thread's four entries of the tile: rows 16 rb + l4 + 4 c, column 16 cb + l15
    const int lj = 16 * cb + l15, gj = j0 + lj;
    double sv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int li = 16 * rb + l4 + 4 * c, gi = i0 + li;
      double s = -INFINITY;
      if (gi < pb.row_cnt && gj < pb.col_cnt) {
        const double cost = pb.sym && gi == gj ? 0.0 : fmax(0.5 * (s_ni[li] + s_nj[lj]) - dot[c], 0.0);
        s = s_lw[lj] + (s_h[lj] - cost) * inv_eps;
      }
      sv[c] = s;
      s_k[li * kSkKld + lj] = s;
    }
    __syncthreads();
    double Mn = M;
    if (tid < kSkRows) {
      const double* __restrict__ kr = s_k + tid * kSkKld;
      for (int j = 0; j < kSkCols; ++j) Mn = fmax(Mn, kr[j]);
      s_mx[tid] = Mn;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int li = 16 * rb + l4 + 4 * c;
      s_k[li * kSkKld + lj] = sv[c] == -INFINITY ? 0.0 : exp(sv[c] - s_mx[li]);
    }
    __syncthreads();
    if (tid < kSkRows) {
      const double* __restrict__ kr = s_k + tid * kSkKld;
      double ts = 0.0;
      for (int j = 0; j < kSkCols; ++j) ts += kr[j];
      S = (M == -INFINITY ? 0.0 : S * exp(M - Mn)) + ts;
      M = Mn;
    }
  }
  if (tid < kSkRows && i0 + tid < pb.row_cnt) {
    const size_t at = ((size_t)blockIdx.z * slabs + slab) * R + i0 + tid;
    part_max[at] = M;
    part_sum[at] = S;
  }
}

// thread i of problem blockIdx.y: the slabs' pairs in slab order, -e (log sum + M), the potential
__global__ __launch_bounds__(kSkSmallBlock) void sk_fold(const SkProbs probs, const int slabs, const int R, const double* __restrict__ eps,
                                                          const double* __restrict__ part_max, const double* __restrict__ part_sum) {
  const SkProb pb = sk_pick(probs, blockIdx.y);
  const int i = blockIdx.x * kSkSmallBlock + threadIdx.x;
  if (i >= pb.row_cnt) return;
  double M = -INFINITY, S = 0.0;
  for (int s = 0; s < slabs; ++s) {
    const size_t at = ((size_t)blockIdx.y * slabs + s) * R + i;
    const double m2 = part_max[at], s2 = part_sum[at];
    if (m2 == -INFINITY) continue;      // an empty slab: nothing to merge, and no -inf - -inf
    const double Mn = fmax(M, m2);
    S = (M == -INFINITY ? 0.0 : S * exp(M - Mn)) + s2 * exp(m2 - Mn);
    M = Mn;
  }
  const double e = eps[0];
  const double v = -e * (log(S) + M);
  const double old = pb.dst[i];
  if (pb.err) pb.err[i] = fabs(expm1((old - v) / e));
  pb.dst[i] = pb.avg ? 0.5 * (old + v) : v;
}

// one workgroup: part_x = sum_i a_i (f_i - p_i) / sum a, part_y likewise, each as 256 runs of consecutive rows and then the runs in
// order; the largest of err [n]; out = (part_x + part_y, part_x, part_y, marginal_err)
__global__ __launch_bounds__(kSkSmallBlock) void sk_finish(const double* __restrict__ a, const int n, const double* __restrict__ b, const int m,
                                                            const double* __restrict__ wsum, const double* __restrict__ f,
                                                            const double* __restrict__ g, const double* __restrict__ p,
                                                            const double* __restrict__ q, const double* __restrict__ err,
                                                            double* __restrict__ out) {
  __shared__ double s_x[kSkSmallBlock], s_y[kSkSmallBlock], s_e[kSkSmallBlock];
  const int tid = threadIdx.x;
  double sx = 0.0, sy = 0.0, se = 0.0;
  {
    const int run = (n + kSkSmallBlock - 1) / kSkSmallBlock;
    const int lo = tid * run < n ? tid * run : n, hi = lo + run < n ? lo + run : n;
    const double un = 1.0 / (double)n, tot = wsum[0];
    for (int i = lo; i < hi; ++i) {
      sx += (a ? a[i] / tot : un) * (f[i] - p[i]);
      se = fmax(se, err[i]);
    }
  }
  {
    const int run = (m + kSkSmallBlock - 1) / kSkSmallBlock;
    const int lo = tid * run < m ? tid * run : m, hi = lo + run < m ? lo + run : m;
    const double un = 1.0 / (double)m, tot = wsum[1];
    for (int i = lo; i < hi; ++i) sy += (b ? b[i] / tot : un) * (g[i] - q[i]);
  }
  s_x[tid] = sx;
  s_y[tid] = sy;
  s_e[tid] = se;
  __syncthreads();
  if (tid == 0) {
    double X = 0.0, Y = 0.0, E = 0.0;
    for (int t = 0; t < kSkSmallBlock; ++t) {
      X += s_x[t];
      Y += s_y[t];
      E = fmax(E, s_e[t]);
    }
    out[0] = X + Y;
    out[1] = X;
    out[2] = Y;
    out[3] = E;
  }
}

}  // namespace gmvae
