// gmvae_linprobe_* (include/gmvae_hip.h; host side: csrc/linprobe.hip): a linear probe -- multinomial logistic regression with an
// l2 penalty -- fitted to N codes x [N][L] with labels y [N], and its predictions.  Model independent.  The statement is
// tests/linprobe_ref.py:
//   a label outside [0, C) marks the row unlabelled (weight 0); n = the labelled rows, xbar = their mean
//   p_n = softmax((x_n - xbar) W + b),  f = -(1/n) sum_labelled ln p_n[y_n] + (l2 / 2) |W|_F^2
//   A = 1/2 (1/n) sum_labelled (x_n - xbar)(x_n - xbar)^T + l2 I    (Boehning: the Hessian of f in W is <= I_C (x) A, in b <= 1/2 I)
//   FISTA in that metric, unit steps: at the extrapolated point V, G_W = (1/n) sum (x_n - xbar)^T (p_n - e_y) + l2 V_W and
//   G_b = (1/n) sum (p_n - e_y); Theta' = (V_W - A^-1 G_W, V_b - 2 G_b); V' = Theta' + beta (Theta' - Theta), beta from the host
// Three launches of set-up, then two launches per iteration; nothing synchronises with the host.
// The set-up (one workgroup doing all of it took 15.9 ms at N = 60,000, L = 64 -- a quarter of a 300-iteration fit;
// profiles/linprobe_notes.md -- so the two sweeps over the rows are spread over row slices):
//   linprobe_moments: a workgroup per row slice; thread (r, d) adds the labelled rows r, r + R, ... of column d in fp64 (R =
//     kMfBlock / L; eight loads in flight), the R runs added in order: sum x [L] and the labelled rows, per slice.
//   linprobe_gram: every workgroup first adds the slices' moments in index order (lp_mean_lds: the same bits everywhere) for n and
//     xbar; then the centred Gram sums of its slice as the full-covariance M-step forms S2 (csrc/mixfit_full.hpp; that text sits
//     inside its pass and is not shared: csrc/mixfit.hpp says what sharing a pass's steps cost) with weights 0 / 1: tiles of 64
//     rows staged as x - xbar in fp64 (an unlabelled row, and a row past the end, as 0), a wave owns 16 x 16 blocks (bi >= bj) and
//     multiplies them by v_mfma_f64_16x16x4_f64 in that kernel's operand and result layout; the sums stay in LDS, in the packed
//     lower triangle, and go to the slice's partials at the end.
//   linprobe_setup: ONE workgroup adds the slices' Gram sums in index order, A = sums / (2 n) + l2 I, mff_factor_lds
//     (csrc/mixfit_common.hpp, shared with mixfit_full_factor) leaves C^-1, and A^-1 = C^-T C^-1 goes to the workspace, every entry
//     summed in the same order as its mirror image: bit-symmetric.  It also zeroes Theta, V, W_out and b_out and fills the history
//     with NaN, so a failed set-up -- info_out[0] = j + 1 for a pivot j that is not > 0, or -1 where no row is labelled -- leaves
//     exactly that: the later launches of the fit read the verdict and return.
// linprobe_pass: a workgroup of kMfBlock threads owns a contiguous slice of `per_group` rows and walks it in tiles of T rows (lp_plan).
// LDS, all dynamic: V_W as fp32 [L][C], resident (64 KiB at the C L gate), and the constant b'_c = V_b,c - sum_d xbar_d V_W,dc
// [C] (fp64; the products with the ROUNDED V_W, so that the centring is the one the logits use); per tile the staged codes
// [T][L | 1] (fp32), the logits and then the residuals [T][C | 1] (fp64), and per row the max, ln of the sum, 1 / sum, -ln p[y], the
// label and whether the row is classified correctly.  logit_nc = sum_d x_nd V_dc + b'_c: every product of two fp32 numbers is exact
// in fp64, and the sum is fp64.  Per tile:
//   stage:   the tile's T L floats: one coalesced sweep; the labels;
//   logits:  an item per thread is four rows of one class (mixfit_pass's shape);
//   rows:    a thread per row: the max and its FIRST index, fp32 exponentials summed in fp64, ln p[y];
//   sweep:   kAccum: the residual r_nc = p_nc - [c = y_n] (0 in an unlabelled row) replaces the logit; else log p is written;
//   sums:    kAccum: a thread owns the slots (c, d) = tid, tid + kMfBlock, ... of sum_n x_nd r_nc (d = L: sum_n r_nc), fp64, added
//            to the workgroup's partials by a plain load, add, store (the first tile stores only); no atomics.  The sums are of
//            the RAW codes; linprobe_update centres them: sum (x - xbar) r = sum x r - xbar sum r.
// Three more sums a workgroup -- labelled rows, correct ones, sum -ln p[y] -- by wave 0 in a fixed tree.
// With kAccum = false the pass reads W, b (fp32, un-centred) instead of V: gmvae_linprobe_predict, whose linprobe_sums folds the three.
// linprobe_update: a workgroup per class c folds its L + 1 slots as mixfit_update does (mf_fold_run), forms G, applies A^-1 (read
// by columns: coalesced, and the same numbers by symmetry) and the factor-2 bias step, extrapolates, and writes column c of Theta
// and V; |V_W,c|^2 goes to a double-buffered [2][C] so that workgroup 0 of the NEXT launch has the penalty of the point its loss
// belongs to.  The last launch writes W_out, b_out = b - xbar W and grad_max (a max of non-negative floats by their bit patterns:
// an integer max, which no order of arrival changes).
// One owner per sum, fixed-order fp64 folds, no float atomics: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mixfit_common.hpp"

namespace gmvae {

constexpr int kLpMaxL = 128;              // the set-up factors A in LDS: mixfit_full_factor's bound
constexpr int kLpMaxC = 256;              // one thread per class in the image's constant; one workgroup per class in the update
constexpr int kLpMaxCL = 16384;           // the C L gate: V_W is then 64 KiB of fp32
constexpr int kLpSetupTile = 64;          // rows per tile of linprobe_gram: 16 rows for each of the four waves

// the workspace, in doubles: the header (n, whether the set-up succeeded), xbar [L], A^-1 [L][L], Theta and V [C][L + 1] each (the
// bias is entry L of a class), |V_W,c|^2 [2][C], then the workgroups' partials [groups][stride]
struct LpLayout {
  size_t xbar, ainv, theta, v, colsq, part;
};
__host__ __device__ static inline LpLayout lp_layout(int L, int C) {
  LpLayout o;
  o.xbar = 4;
  o.ainv = o.xbar + (size_t)L;
  o.theta = o.ainv + (size_t)L * L;
  o.v = o.theta + (size_t)C * (L + 1);
  o.colsq = o.v + (size_t)C * (L + 1);
  o.part = o.colsq + 2 * (size_t)C;
  return o;
}

// the pass's shape (MfPlan) and the set-up's: rows per tile, rows per workgroup, workgroups, doubles per workgroup's partials -- the
// Gram sums' packed lower triangle [L (L + 1) / 2], sum x [L] and the labelled rows --, LDS bytes of linprobe_gram and linprobe_setup
struct LpPlan : MfPlan {
  int setup_tile, setup_per_group, setup_groups, setup_stride;
  size_t lds_gram, lds_setup;
};
static inline size_t lp_lds_bytes(int L, int C, int T) {
  const size_t Lp = (size_t)(L | 1), Cp = (size_t)(C | 1);
  return 8 * ((size_t)C + (size_t)T * (Cp + 4)) + 4 * ((size_t)L * C + (size_t)T * (Lp + 2));
}
static inline LpPlan lp_plan(int64_t N, int L, int C) {
  LpPlan p;
  MfPlan s;
  mf_plan_groups(s, N, kLpSetupTile, kMfMaxGroups);
  p.setup_tile = s.tile;
  p.setup_per_group = s.per_group;
  p.setup_groups = s.groups;
  p.setup_stride = mff_tri(L) + L + 1;
  p.lds_gram = 8 * ((size_t)mff_tri(L) + (size_t)kLpSetupTile * (size_t)(L | 1) + (size_t)L + 1);      // 133,128 bytes at L = 128
  p.lds_setup = 8 * (2 * (size_t)mff_tri(L) + (size_t)L + 1);                                           // 133,128 bytes at L = 128
  const size_t image = lp_lds_bytes(L, C, 0), row = lp_lds_bytes(L, C, 1) - image;
  int64_t T = (int64_t)(((size_t)kMfLdsBytes - image) / row);      // >= 40 inside the gate: image <= 67,584 and row <= 2,356 bytes
  T = T > kMfMaxTile ? kMfMaxTile : T;
  T = T > N ? N : T;
  mf_plan_groups(p, N, T, kMfMaxGroups);
  p.stride = C * (L + 1) + 3;      // sum x r and sum r [C][L + 1], then the labelled rows, the correct ones, sum -ln p[y]
  p.lds = lp_lds_bytes(L, C, (int)T);
  return p;
}
// doubles behind LpLayout::part: the set-up's partials and then, in their place, the pass's
static inline uint64_t lp_part_doubles(const LpPlan& p) {
  const uint64_t a = (uint64_t)p.groups * (uint64_t)p.stride, b = (uint64_t)p.setup_groups * (uint64_t)p.setup_stride;
  return a > b ? a : b;
}

__device__ __forceinline__ bool lp_labelled(const int y, const int C) { return (unsigned)y < (unsigned)C; }

// n and xbar from linprobe_moments' partials, the workgroups added in index order: s_xbar [L + 1] ends as xbar and, at [L], n.
// The same code in linprobe_gram and linprobe_setup, so the same bits in every workgroup.  Ends behind a barrier.
__device__ __forceinline__ double lp_mean_lds(const double* __restrict__ spart, const int Gs, const int sstride, const int L, const int tid,
                                              double* const s_xbar) {
  if (tid <= L) {
    const double* __restrict__ src = spart + mff_tri(L) + tid;
    double a = 0.0;
    for (int g = 0; g < Gs; ++g) a += src[(size_t)g * sstride];
    s_xbar[tid] = a;
  }
  __syncthreads();
  const double n = s_xbar[L];
  __syncthreads();
  if (tid < L) s_xbar[tid] = n > 0.0 ? s_xbar[tid] / n : 0.0;
  __syncthreads();
  return n;
}

// the labelled rows of a workgroup's slice and their sum: thread (r, d) adds the rows r, r + R, ... of column d in order, eight loads
// in flight; the R runs are added in order
__global__ __launch_bounds__(kMfBlock) void linprobe_moments(const float* __restrict__ codes, const int32_t* __restrict__ labels, const int N,
                                                              const int L, const int C, const int per_group, double* __restrict__ spart,
                                                              const int sstride) {
  __shared__ double s_red[kMfBlock];
  const int tid = threadIdx.x;
  const int64_t g_lo = (int64_t)blockIdx.x * per_group, g_hi = g_lo + per_group < N ? g_lo + per_group : N;
  double* const out = spart + (size_t)blockIdx.x * sstride + mff_tri(L);
  const int R = kMfBlock / L, r = tid / L, d = tid - r * L;
  double acc = 0.0;
  int cnt = 0;
  if (r < R) {
    for (int64_t n0 = g_lo + r; n0 < g_hi; n0 += 8 * R) {
      float v[8];
      int yy[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t n = n0 + (int64_t)u * R;
        const bool in = n < g_hi;
        yy[u] = in ? labels[n] : -1;
        v[u] = in ? codes[(size_t)n * L + d] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool lab = lp_labelled(yy[u], C);
        acc += lab ? (double)v[u] : 0.0;
        cnt += lab ? 1 : 0;
      }
    }
  }
  s_red[tid] = acc;
  __syncthreads();
  if (tid < L) {
    double sx = 0.0;
    for (int q = 0; q < R; ++q) sx += s_red[q * L + tid];
    out[tid] = sx;
  }
  __syncthreads();
  s_red[tid] = (double)cnt;
  __syncthreads();
  if (tid == 0) {
    double n = 0.0;
    for (int q = 0; q < R; ++q) n += s_red[q * L];      // (counts: exact)
    out[L] = n;
  }
}

// the centred Gram sums of a workgroup's slice, into the packed lower triangle of its partials
__global__ __launch_bounds__(kMfBlock) void linprobe_gram(const float* __restrict__ codes, const int32_t* __restrict__ labels, const int N,
                                                           const int L, const int C, const int T, const int per_group, const int Gs,
                                                           double* __restrict__ spart, const int sstride) {
  extern __shared__ __attribute__((aligned(16))) char lp_smem[];
  const int tid = threadIdx.x, Lp = L | 1, P = mff_tri(L);
  double* const a = reinterpret_cast<double*>(lp_smem);      // [P]
  double* const s_dz = a + P;                                // [T][Lp]
  double* const s_xbar = s_dz + T * Lp;                      // [L + 1]
  const double n = lp_mean_lds(spart, Gs, sstride, L, tid, s_xbar);
  if (!(n > 0.0)) return;      // (every thread of every workgroup: linprobe_setup then reports -1 and reads no sum)
  for (int s = tid; s < P; s += kMfBlock) a[s] = 0.0;
  const int wave = tid >> 6, lane = tid & 63, nb = (L + 15) >> 4, nblk = nb * (nb + 1) / 2;
  const int nL0 = tid / L, dL0 = tid - nL0 * L, stepL_n = kMfBlock / L, stepL_d = kMfBlock - stepL_n * L;
  const int64_t g_lo = (int64_t)blockIdx.x * per_group, g_hi = g_lo + per_group < N ? g_lo + per_group : N;
  for (int64_t r0 = g_lo; r0 < g_hi; r0 += T) {
    const int rows = (int)(g_hi - r0 < T ? g_hi - r0 : T);
    __syncthreads();      // the zeroed sums are in place; the previous tile's products have read s_dz
    {
      const float* __restrict__ src = codes + (size_t)r0 * L;
      int nn = nL0, dd = dL0;
      for (int i = tid; i < T * L; i += kMfBlock) {
        const bool on = nn < rows && lp_labelled(labels[r0 + nn], C);
        s_dz[nn * Lp + dd] = on ? (double)src[i] - s_xbar[dd] : 0.0;
        MF_ADVANCE(nn, dd, stepL_n, stepL_d, L);
      }
    }
    __syncthreads();
    for (int b = wave; b < nblk; b += kMfBlock >> 6) {      // (uniform in the wave: the MFMA runs with every lane on)
      int bi = 0, bj = b;
      while (bj > bi) {
        bj -= bi + 1;
        ++bi;
      }
      const int ia = 16 * bi + (lane & 15), ib = 16 * bj + (lane & 15), nn = lane >> 4;
      mff_d4 sum = {0.0, 0.0, 0.0, 0.0};
      for (int n0 = 0; n0 < T; n0 += 16) {      // (T is a multiple of 16; the rows from `rows` to T are staged as 0)
        double av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int m = n0 + 4 * u + nn;
          av[u] = ia < L ? s_dz[m * Lp + ia] : 0.0;
          bv[u] = ib < L ? s_dz[m * Lp + ib] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) sum = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], sum, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {      // one owner lane per entry on or below the diagonal
        const int i = 16 * bi + nn + 4 * g;
        if (i < L && ib <= i) a[mff_tri(i) + ib] += sum[g];
      }
    }
  }
  __syncthreads();
  double* __restrict__ out = spart + (size_t)blockIdx.x * sstride;
  for (int s = tid; s < P; s += kMfBlock) out[s] = a[s];
}

// one workgroup: folds the Gram partials in index order, builds A, factors it, writes A^-1 and the fit's starting state
__global__ __launch_bounds__(kMfBlock) void linprobe_setup(const double* __restrict__ spart, const int Gs, const int sstride, const int L,
                                                            const int C, const double l2, const int n_iter, double* __restrict__ ws,
                                                            float* __restrict__ W_out, float* __restrict__ b_out, float* __restrict__ hist,
                                                            float* __restrict__ grad_max_out, int32_t* __restrict__ info_out) {
  extern __shared__ __attribute__((aligned(16))) char lp_smem[];
  const int tid = threadIdx.x, P = mff_tri(L);
  double* const a = reinterpret_cast<double*>(lp_smem);      // [P]: the Gram sums, then A, then its factor
  double* const x = a + P;                                   // [P]: the identity, then C^-1
  double* const s_xbar = x + P;                              // [L + 1]
  const LpLayout lay = lp_layout(L, C);
  const double n = lp_mean_lds(spart, Gs, sstride, L, tid, s_xbar);
  int info = n > 0.0 ? 0 : -1;
  if (info == 0) {
    const double scale = 0.5 / n;
    for (int s = tid; s < P; s += kMfBlock) {
      const double* __restrict__ src = spart + s;
      double v = 0.0;
      for (int g = 0; g < Gs; ++g) v += src[(size_t)g * sstride];
      a[s] = v * scale;
    }
    __syncthreads();
    {
      const int i0 = tid / L, step_i = kMfBlock / L;
      for (int s = tid, i = i0, j = tid - i0 * L; s < L * L; s += kMfBlock) {
        if (j <= i) x[mff_tri(i) + j] = i == j ? 1.0 : 0.0;
        if (i == j) a[mff_tri(i) + i] += l2;
        MF_ADVANCE(i, j, step_i, kMfBlock - step_i * L, L);
      }
    }
    __syncthreads();
    double sum_ln;
    info = mff_factor_lds(a, x, L, tid, sum_ln);
    __syncthreads();
    if (info == 0) {
      double* __restrict__ ainv = ws + lay.ainv;
      const int i0 = tid / L, step_i = kMfBlock / L;
      for (int s = tid, i = i0, j = tid - i0 * L; s < L * L; s += kMfBlock) {
        double v = 0.0;
        for (int t = i > j ? i : j; t < L; ++t) v = fma(x[mff_tri(t) + i], x[mff_tri(t) + j], v);
        ainv[s] = v;
        MF_ADVANCE(i, j, step_i, kMfBlock - step_i * L, L);
      }
    }
  }
  for (int s = tid; s < 2 * C * (L + 1) + 2 * C; s += kMfBlock) ws[lay.theta + s] = 0.0;      // Theta, V and both |V_W,c|^2
  for (int s = tid; s < L * C; s += kMfBlock) W_out[s] = 0.f;
  for (int s = tid; s < C; s += kMfBlock) b_out[s] = 0.f;
  if (hist)
    for (int s = tid; s < n_iter; s += kMfBlock) hist[s] = NAN;
  if (tid < L) ws[lay.xbar + tid] = s_xbar[tid];
  if (tid == 0) {
    ws[0] = n;
    ws[1] = info == 0 ? 1.0 : 0.0;
    if (grad_max_out) *grad_max_out = info == 0 && n_iter > 0 ? 0.f : NAN;
    if (info_out) info_out[0] = info;
  }
}

template <bool kAccum>
__global__ __launch_bounds__(kMfBlock) void linprobe_pass(const float* __restrict__ codes, const int32_t* __restrict__ labels, const int N,
                                                           const int L, const int C, const double* __restrict__ ws,
                                                           const float* __restrict__ Wf, const float* __restrict__ bf, const int T,
                                                           const int per_group, float* __restrict__ log_prob_out,
                                                           int32_t* __restrict__ pred_out, double* __restrict__ part, const int stride) {
  extern __shared__ __attribute__((aligned(16))) char lp_smem[];
  const int tid = threadIdx.x, Lp = L | 1, Cp = C | 1, L1 = L + 1;
  if (kAccum && ws[1] == 0.0) return;      // the set-up failed (every thread of every workgroup reads the same verdict)
  double* const s_bp = reinterpret_cast<double*>(lp_smem);      // [C]
  double* const s_l = s_bp + C;                                 // [T][Cp]: the logits, then the residuals
  double* const s_m = s_l + T * Cp;                             // [T]
  double* const s_ls = s_m + T;                                 // [T]
  double* const s_inv = s_ls + T;                               // [T]
  double* const s_nll = s_inv + T;                              // [T]
  float* const s_V = reinterpret_cast<float*>(s_nll + T);       // [L][C]
  float* const s_x = s_V + L * C;                               // [T][Lp]
  int* const s_y = reinterpret_cast<int*>(s_x + T * Lp);        // [T]: the label, -1 in an unlabelled row
  int* const s_hit = s_y + T;                                   // [T]

  const int nL0 = tid / L, dL0 = tid - nL0 * L, stepL_n = kMfBlock / L, stepL_d = kMfBlock - stepL_n * L;
  const int nC0 = tid / C, cC0 = tid - nC0 * C, stepC_n = kMfBlock / C, stepC_d = kMfBlock - stepC_n * C;
  const int c10 = tid / L1, d10 = tid - c10 * L1, step1_c = kMfBlock / L1, step1_d = kMfBlock - step1_c * L1;
  if (kAccum) {
    const LpLayout lay = lp_layout(L, C);
    const double* __restrict__ Vg = ws + lay.v;
    for (int s = tid, c = c10, d = d10; s < C * L1; s += kMfBlock) {
      if (d < L) s_V[d * C + c] = (float)Vg[s];
      MF_ADVANCE(c, d, step1_c, step1_d, L1);
    }
    __syncthreads();
    if (tid < C) {
      const double* __restrict__ xbar = ws + lay.xbar;
      double bp = Vg[(size_t)tid * L1 + L];
      for (int d = 0; d < L; ++d) bp = fma(-xbar[d], (double)s_V[d * C + tid], bp);
      s_bp[tid] = bp;
    }
  } else {
    for (int s = tid; s < L * C; s += kMfBlock) s_V[s] = Wf[s];
    if (tid < C) s_bp[tid] = (double)bf[tid];
  }

  const int64_t g_lo = (int64_t)blockIdx.x * per_group, g_hi = g_lo + per_group < N ? g_lo + per_group : N;
  double* const gpart = part + (size_t)blockIdx.x * stride;
  double cnt_acc = 0.0, hit_acc = 0.0, nll_acc = 0.0;      // (thread 0's)
  for (int64_t r0 = g_lo; r0 < g_hi; r0 += T) {
    const int rows = (int)(g_hi - r0 < T ? g_hi - r0 : T);
    __syncthreads();      // the image is in place; the previous tile's sums have read s_x and s_l
    {
      const float* __restrict__ src = codes + (size_t)r0 * L;
      int n = nL0, d = dL0;
      for (int i = tid; i < rows * L; i += kMfBlock) {
        s_x[n * Lp + d] = src[i];
        MF_ADVANCE(n, d, stepL_n, stepL_d, L);
      }
      if (tid < rows) {
        const int y = labels ? labels[r0 + tid] : -1;
        s_y[tid] = lp_labelled(y, C) ? y : -1;
      }
    }
    __syncthreads();
    {
      const int quads = (rows + 3) >> 2;      // item g C + c: the rows 4 g .. 4 g + 3 (a row past the end repeats the last one) of class c
      for (int i = tid, g = nC0, c = cC0; i < quads * C; i += kMfBlock) {
        const int last = rows - 1, n0 = 4 * g;
        const float* __restrict__ z0 = s_x + (n0 < last ? n0 : last) * Lp;
        const float* __restrict__ z1 = s_x + (n0 + 1 < last ? n0 + 1 : last) * Lp;
        const float* __restrict__ z2 = s_x + (n0 + 2 < last ? n0 + 2 : last) * Lp;
        const float* __restrict__ z3 = s_x + (n0 + 3 < last ? n0 + 3 : last) * Lp;
        const float* __restrict__ vc = s_V + c;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
        for (int d = 0; d < L; ++d) {
          const double v = (double)vc[d * C];
          q0 = fma((double)z0[d], v, q0);
          q1 = fma((double)z1[d], v, q1);
          q2 = fma((double)z2[d], v, q2);
          q3 = fma((double)z3[d], v, q3);
        }
        const double bp = s_bp[c];
        double* __restrict__ o = s_l + n0 * Cp + c;
        o[0] = q0 + bp;
        if (n0 + 1 < rows) o[Cp] = q1 + bp;
        if (n0 + 2 < rows) o[2 * Cp] = q2 + bp;
        if (n0 + 3 < rows) o[3 * Cp] = q3 + bp;
        MF_ADVANCE(g, c, stepC_n, stepC_d, C);
      }
    }
    __syncthreads();
    if (tid < rows) {
      const double* __restrict__ lr = s_l + tid * Cp;
      double m = -INFINITY;
      int arg = 0;
      for (int c = 0; c < C; ++c)
        if (lr[c] > m) {      // (strictly: the first maximal index)
          m = lr[c];
          arg = c;
        }
      if (!(m > -INFINITY)) m = 0.0;
      double s = 0.0;
      for (int c = 0; c < C; ++c) s += (double)expf((float)(lr[c] - m));
      const double ls = log(s);
      const int y = s_y[tid];
      s_m[tid] = m;
      s_ls[tid] = ls;
      s_inv[tid] = 1.0 / s;
      s_nll[tid] = y >= 0 ? ls - (lr[y] - m) : 0.0;
      s_hit[tid] = y >= 0 && arg == y ? 1 : 0;
      if (!kAccum && pred_out) pred_out[r0 + tid] = arg;
    }
    __syncthreads();
    if (tid < 64) {      // the tile's three sums: lanes over the rows, a fixed tree
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
      for (int n = tid; n < rows; n += 64) {
        a0 += s_y[n] >= 0 ? 1.0 : 0.0;
        a1 += (double)s_hit[n];
        a2 += s_nll[n];
      }
      cnt_acc += mf_wave_sum(a0);
      hit_acc += mf_wave_sum(a1);
      nll_acc += mf_wave_sum(a2);
    }
    for (int i = tid, n = nC0, c = cC0; i < rows * C; i += kMfBlock) {
      const double t = s_l[n * Cp + c] - s_m[n];
      if (kAccum) {
        const int y = s_y[n];
        const double p = (double)expf((float)t) * s_inv[n];
        s_l[n * Cp + c] = y < 0 ? 0.0 : (c == y ? p - 1.0 : p);
      } else if (log_prob_out) {
        log_prob_out[(size_t)r0 * C + i] = (float)(t - s_ls[n]);
      }
      MF_ADVANCE(n, c, stepC_n, stepC_d, C);
    }
    if (kAccum) {
      __syncthreads();
      const bool first = r0 == g_lo;
      for (int s = tid, c = c10, d = d10; s < C * L1; s += kMfBlock) {
        const double* __restrict__ rc = s_l + c;
        double a = 0.0;
        if (d < L) {
          const float* __restrict__ xd = s_x + d;
          for (int n = 0; n < rows; ++n) a = fma((double)xd[n * Lp], rc[n * Cp], a);
        } else {
          for (int n = 0; n < rows; ++n) a += rc[n * Cp];
        }
        if (!first) a += gpart[s];
        gpart[s] = a;
        MF_ADVANCE(c, d, step1_c, step1_d, L1);
      }
    }
  }
  if (tid == 0) {
    double* const o = gpart + (kAccum ? C * L1 : 0);
    o[0] = cnt_acc;
    o[1] = hit_acc;
    o[2] = nll_acc;
  }
}

// one workgroup per class
__global__ __launch_bounds__(kMfBlock) void linprobe_update(const double* __restrict__ part, const int G, const int stride, const int L,
                                                             const int C, const double l2, const double beta, const int it, const int last,
                                                             double* __restrict__ ws, float* __restrict__ W_out, float* __restrict__ b_out,
                                                             float* __restrict__ hist, float* __restrict__ grad_max_out) {
  __shared__ double s_p[kMfFoldSlots][kMfFoldParts + 1];
  __shared__ double s_g[kLpMaxL + 2];      // the folded sums: d < L, sum r, and (workgroup 0) sum -ln p[y]
  __shared__ double s_gw[kLpMaxL + 1];     // G
  __shared__ double s_t[kLpMaxL + 1];      // Theta'
  __shared__ double s_v[kLpMaxL + 1];      // V'
  if (ws[1] == 0.0) return;                // the set-up failed
  const int tid = threadIdx.x, q = tid / kMfFoldParts, p = tid % kMfFoldParts, c = blockIdx.x, L1 = L + 1;
  const LpLayout lay = lp_layout(L, C);
  const double n = ws[0];
  const double* __restrict__ xbar = ws + lay.xbar;
  const double* __restrict__ ainv = ws + lay.ainv;
  double* __restrict__ theta = ws + lay.theta + (size_t)c * L1;
  double* __restrict__ V = ws + lay.v + (size_t)c * L1;
  double* __restrict__ colsq = ws + lay.colsq;
  const int nslots = L1 + (c == 0 ? 1 : 0);
  for (int s0 = 0; s0 < nslots; s0 += kMfFoldSlots) {
    const int s = s0 + q;
    if (s < nslots) s_p[q][p] = mf_fold_run(part, G, stride, s <= L ? (size_t)c * L1 + s : (size_t)C * L1 + 2, p);
    __syncthreads();
    if (s < nslots && p == 0) {
      double a = 0.0;
      for (int j = 0; j < kMfFoldParts; ++j) a += s_p[q][j];
      s_g[s] = a;
    }
    __syncthreads();
  }
  const double Sr = s_g[L];
  // (the centring's product rounded on its own, not contracted into an fma: where one row is labelled, x r - xbar r is then exactly
  // 0, as in the statement, and not the rounding error of x r)
  if (tid < L) {
    double centred;
    {
#pragma clang fp contract(off)
      const double shift = xbar[tid] * Sr;
      centred = s_g[tid] - shift;
    }
    s_gw[tid] = centred / n + l2 * V[tid];
  }
  if (tid == L) s_gw[L] = Sr / n;
  __syncthreads();
  if (tid <= L) {
    double th;
    if (tid < L) {
      double a = 0.0;
      for (int e = 0; e < L; ++e) a = fma(ainv[(size_t)e * L + tid], s_gw[e], a);      // (A^-1 is bit-symmetric: its column is its row)
      th = V[tid] - a;
    } else {
      th = V[L] - 2.0 * s_gw[L];
    }
    const double vn = th + beta * (th - theta[tid]);
    theta[tid] = th;
    V[tid] = vn;
    s_t[tid] = th;
    s_v[tid] = vn;
  }
  __syncthreads();
  if (last && tid < L) W_out[(size_t)tid * C + c] = (float)s_t[tid];
  if (tid == 0) {
    double sq = 0.0;
    for (int d = 0; d < L; ++d) sq = fma(s_v[d], s_v[d], sq);
    colsq[((it + 1) & 1) * C + c] = sq;
    if (c == 0) {      // f(V_it): the penalty of the point this launch's sums were taken at, left by the previous launch
      double reg = 0.0;
      for (int k = 0; k < C; ++k) reg += colsq[(it & 1) * C + k];
      if (hist) hist[it] = (float)(s_g[L + 1] / n + 0.5 * l2 * reg);
    }
    if (last) {
      double bo = s_t[L];
      for (int d = 0; d < L; ++d) bo = fma(-xbar[d], s_t[d], bo);
      b_out[c] = (float)bo;
      if (grad_max_out) {
        double gm = 0.0;
        bool bad = false;
        for (int d = 0; d <= L; ++d) {
          const double g = fabs(s_gw[d]);
          bad = bad || g != g;
          gm = g > gm ? g : gm;
        }
        // non-negative floats are ordered as their bit patterns, and the quiet NaN lies above +inf: an integer max
        atomicMax(reinterpret_cast<unsigned int*>(grad_max_out), bad ? 0x7fc00000u : __float_as_uint((float)gm));
      }
    }
  }
}

// gmvae_linprobe_predict: the three sums of the G workgroups, folded in index order
__global__ __launch_bounds__(64) void linprobe_sums(const double* __restrict__ part, const int G, double* __restrict__ sums_out) {
  __shared__ double s_p[3][kMfFoldParts + 1];
  const int tid = threadIdx.x, q = tid / kMfFoldParts, p = tid % kMfFoldParts;
  if (q < 3) s_p[q][p] = mf_fold_run(part, G, 3, (size_t)q, p);
  __syncthreads();
  if (tid < 3) {
    double a = 0.0;
    for (int j = 0; j < kMfFoldParts; ++j) a += s_p[tid][j];
    sums_out[tid] = a;
  }
}

}  // namespace gmvae
