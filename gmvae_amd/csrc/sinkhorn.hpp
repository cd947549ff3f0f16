// gmvae_sinkhorn (include/gmvae_hip.h; host side: csrc/twosample.hip): the debiased Sinkhorn divergence (Genevay et al. 2018; Feydy
// et al. 2019) between two weighted samples x [n][D] and y [m][D] under the cost C(u, v) = 1/2 |u - v|^2.  Model independent.
// The statement is tests/sinkhorn_ref.py:
//   softmin_e(pts, h, w)(u) = -e log sum_j w_j exp((h_j - C(u, pts_j)) / e)
//   all four potentials start at 0; for t < T, e = eps[t]:
//     half A: f <- softmin(y, g, b) at x;  p <- (p + softmin(x, p, a) at x) / 2;  q <- (q + softmin(y, q, b) at y) / 2
//     half B: g <- softmin(x, f, a) at y;  p and q once more
//   last pass at e = eps[T]: f' = softmin(y, g, b) at x, p' = softmin(x, p, a) at x, q' = softmin(y, q, b) at y, none averaged
//   part_x = <a, f' - p'>, part_y = <b, g - q'>, S = part_x + part_y, marginal_err = max_i |expm1((f_i - f'_i) / eps[T])|
// Nothing n m in memory, nothing synchronises with the host, e is read from the device.  The cost (n_i + n_j) / 2 - zc_i . zc_j,
// clamped at 0, comes from the centred Gram tile of csrc/cgram.hpp over the pooled rows (x's, then y's), with its three launches in
// front; sk_logw leaves log w - log sum w and sum w of both samples.
// A softmin is a row-wise log-sum-exp over a cost matrix.  The two or three of a half-step depend on nothing of each other, so
// they are the PROBLEMS of one launch (blockIdx.z): a problem is (the rows it is evaluated at, the columns it sums over, h, log w),
// rows and columns each a range of the pooled rows.
// sk_tiles: a workgroup of eight waves owns kCgRows = 32 rows i of its problem and a slab of column tiles of kCgCols = 64 rows j
// (blockIdx.y; the slabs follow from n and m alone, sk_plan; a problem with fewer tiles than slabs leaves its last slabs empty:
// (-inf, 0)).  A workgroup whose row tile lies past its problem's rows leaves before any barrier.  Per column tile:
//   gram:   cgram.hpp's pass over D in chunks (cg_fetch, cg_stage, cg_mfma): the wave's four entries of zc_i . zc_j;
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

#include "cgram.hpp"

namespace gmvae {

constexpr int kSkSmallBlock = 256;        // every kernel here but sk_tiles
constexpr int kSkProblems = 3;

// the launches' shape: the slabs and slices, and so the order of every sum, follow from (n, m) alone
struct SkPlan {
  int R;               // max(n, m): the rows of the larger problem
  int row_tiles;       // of the larger problem: the grid's x
  int slabs;
  CgSlices mean;
};
__host__ __device__ static inline SkPlan sk_plan(int n, int m) {
  SkPlan p;
  p.R = n > m ? n : m;
  p.row_tiles = (p.R + kCgRows - 1) / kCgRows;
  const int col_tiles = (p.R + kCgCols - 1) / kCgCols;
  p.slabs = cg_slabs(p.row_tiles, col_tiles);
  p.mean = cg_mean_slices(n + m);
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
  o.mean = o.mean_part + (size_t)p.mean.slices * D;
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

__global__ __launch_bounds__(kCgBlock) void sk_tiles(const float* __restrict__ x, const int n, const float* __restrict__ y, const int D,
                                                      const SkProbs probs, const int slabs, const int R, const double* __restrict__ eps,
                                                      const double* __restrict__ mean, const double* __restrict__ nrm,
                                                      double* __restrict__ part_max, double* __restrict__ part_sum) {
  __shared__ double s_k[kCgRows * kCgKld];      // the s tile, then its exponentials
  __shared__ double s_mean[kCgDChunk];
  __shared__ double s_h[kCgCols], s_lw[kCgCols], s_nj[kCgCols];      // the tile's columns: h, log w, the squared norm
  __shared__ double s_ni[kCgRows], s_mx[kCgRows];                    // the rows' squared norms and new running maxima
  __shared__ float s_zi[(kCgRows + kCgCols) * kCgZld];               // the staged rows i, then j (cg_stage)

  const SkProb pb = sk_pick(probs, blockIdx.z);
  const int i0 = blockIdx.x * kCgRows;
  if (i0 >= pb.row_cnt) return;      // (uniform in the workgroup, before any barrier: the grid is sized by the larger problem)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int slab = blockIdx.y;
  const int jt_lo = slab * pb.tiles_per_slab;
  const int jt_hi = jt_lo + pb.tiles_per_slab < pb.col_tiles ? jt_lo + pb.tiles_per_slab : pb.col_tiles;
  const double inv_eps = 1.0 / eps[0];
  const int rb = wave >> 2, cb = wave & 3;      // the wave's block of the tile

  double M = -INFINITY, S = 0.0;      // (threads 0 .. 31: the row's running maximum and sum over the slab)
  if (tid < kCgRows) s_ni[tid] = i0 + tid < pb.row_cnt ? nrm[pb.row_off + i0 + tid] : 0.0;

  float pre[kCgStage];
  auto fetch = [&](const int j0, const int dc) {
    cg_fetch(pre, CgPooled{x, n, y}, D, pb.row_off, pb.row_cnt, pb.col_off, pb.col_cnt, i0, j0, dc);
  };
  if (jt_lo < jt_hi) fetch(jt_lo * kCgCols, 0);

  for (int jt = jt_lo; jt < jt_hi; ++jt) {
    const int j0 = jt * kCgCols;
    __syncthreads();      // the previous tile's sums have read s_k, its s tile s_h, s_lw and s_nj
    if (tid < kCgCols) {
      const int j = j0 + tid;
      const bool ok = j < pb.col_cnt;
      s_h[tid] = ok ? pb.h[j] : 0.0;
      s_lw[tid] = ok ? pb.logw[j] : -INFINITY;
      s_nj[tid] = ok ? nrm[pb.col_off + j] : 0.0;
    }
    cg_d4 dot = {0.0, 0.0, 0.0, 0.0};
    for (int dc = 0; dc < D; dc += kCgDChunk) {
      cg_stage<true>(pre, dc, D, s_zi, s_mean, mean);
      if (dc + kCgDChunk < D)
        fetch(j0, dc + kCgDChunk);
      else if (jt + 1 < jt_hi)
        fetch(j0 + kCgCols, 0);
      cg_mfma(s_zi, s_mean, rb, cb, l15, l4, dot);
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
      s_k[li * kCgKld + lj] = s;
    }
    __syncthreads();
    double Mn = M;
    if (tid < kCgRows) {
      const double* __restrict__ kr = s_k + tid * kCgKld;
      for (int j = 0; j < kCgCols; ++j) Mn = fmax(Mn, kr[j]);
      s_mx[tid] = Mn;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int li = 16 * rb + l4 + 4 * c;
      s_k[li * kCgKld + lj] = sv[c] == -INFINITY ? 0.0 : exp(sv[c] - s_mx[li]);
    }
    __syncthreads();
    if (tid < kCgRows) {
      const double* __restrict__ kr = s_k + tid * kCgKld;
      double ts = 0.0;
      for (int j = 0; j < kCgCols; ++j) ts += kr[j];
      S = (M == -INFINITY ? 0.0 : S * exp(M - Mn)) + ts;
      M = Mn;
    }
  }
  if (tid < kCgRows && i0 + tid < pb.row_cnt) {
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
