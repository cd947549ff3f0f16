// gmvae_mixture_logpdf_*: the log-density of a weighted diagonal-Gaussian mixture at M query points, streamed over chunks of
// components (include/gmvae_hip.h).  Model independent: Engine.aggregate_posterior feeds it the aggregate posterior
// q(z) = 1/N sum_n q(z|x_n) (one component per example, K per example for the GMVAE) and the mixture priors.
//   s_mc   = logw_c + sum_d log N(z_md; mu_cd, sigma_cd)        log_joint_m = logsumexp_c s_mc - log_norm
//   t_mcd  = logw_c + log N(z_md; mu_cd, sigma_cd)              log_dim_md  = logsumexp_c t_mcd - log_norm
//   log_own_m = logsumexp over the components c with (c_first + c) / comps_per_owner == query_owner[m] of s_mc
// Arithmetic: the difference form r = (z - mu) (1 / sigma) on the vector units, fp32 (never the expanded square: with sigma
// down to 2e-9 its terms reach 1e17 and cancel).  A tile of components gives a max and an fp32 sum of exp(. - max) -- two
// passes over the tile for the per-dimension terms, so one exponential per (query, component, dimension) --; tiles, slices and
// calls fold into an fp64 (max, sum) by ap_fold.  State: ApState {max, sum}, sum == 0 meaning EMPTY (a zeroed workspace is the
// empty state; a filled state has sum >= 1 up to rounding, its largest term being exp(0)), so a max of 0 is never read as a value and a
// state whose terms are all around -4e7 stays finite.
// Parallelism: a lane owns one query; a 256-thread block 256 queries; grid.y splits the chunk's components into slices whose
// partial states go to the workspace and fold in slice order (aggpost_fold), so 1,024 queries still fill the chip; the
// per-dimension kernel also splits the dimensions, 8 per block (grid.z): its state of 8 dimensions (fp64 max and sum, fp32 tile
// max and sum) and the 8 z values fit a lane's registers at any L.  The joint kernel keeps 32 components' sums of r^2 in
// registers and walks the dimensions 8 at a time, at any L.  Component data are staged in LDS as (mu, 1 / sigma, log terms):
// every lane of a wave reads the same address (a broadcast), the reciprocal and the logarithm are paid once per block.
// One owner per state, fixed-order folds, no atomics: two calls give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmvae {

constexpr int kApBlock = 256;        // threads = queries of a block
constexpr int kApJointTile = 32;     // aggpost_joint: components per tile (their sums live in registers)
constexpr int kApJointDims = 128;    // ... dimensions staged per round
constexpr int kApJointLd = kApJointDims + 4;      // ... LDS row stride (16-byte rows, staging stores spread over the banks)
constexpr int kApDimDims = 8;        // aggpost_dim: dimensions per block
constexpr int kApDimTile = 128;      // ... components per tile
constexpr int kApSliceUnit = 128;    // slices begin at multiples of this many components (both kernels' tiles divide it)
constexpr int kApMaxSlices = 64;
constexpr int kApTargetBlocks = 1024;
constexpr float kApHalfLog2Pi = 0.91893853320467274178f;

struct ApState {
  double m, s;      // running max and sum of exp(. - m); s == 0: empty
};

// one (max, sum) folded into a running state; (m, s) with s == 0 is nothing
__device__ __forceinline__ void ap_fold(double& M, double& S, const double m, const double s) {
  if (!(s > 0.0)) return;
  if (!(S > 0.0)) { M = m; S = s; return; }
  if (m > M) { S = S * exp(M - m) + s; M = m; }
  else S += s * exp(m - M);
}

// slices of a kernel's grid at these sizes -- per_dim 0: the joint kernel's, 1: the per-dimension kernel's -- a function of M and L
// alone: the workspace is sized by it
static inline int ap_slices(int64_t M, int L, int per_dim) {
  int64_t blocks = (M + kApBlock - 1) / kApBlock;
  if (per_dim) blocks *= (L + kApDimDims - 1) / kApDimDims;
  int64_t ns = (kApTargetBlocks + blocks - 1) / blocks;
  return (int)(ns < 1 ? 1 : ns > kApMaxSlices ? kApMaxSlices : ns);
}

// states of one slice (and of the running state): joint [M], own [M], then per dimension [M][L]
static inline uint64_t ap_states(int64_t M, int L, int per_dim) {
  return (uint64_t)M * 2 + (per_dim ? (uint64_t)M * (uint64_t)L : 0);
}

// partial states of a call: the joint kernel's slices hold a joint and an own state per query, the per-dimension kernel's one
// per (query, dimension)
static inline uint64_t ap_part_states(int64_t M, int L, int per_dim) {
  return (uint64_t)ap_slices(M, L, 0) * 2 * (uint64_t)M + (per_dim ? (uint64_t)ap_slices(M, L, 1) * (uint64_t)M * (uint64_t)L : 0);
}

// a chunk of C components cut into at most ns slices of whole kApSliceUnit units
struct ApSplit {
  int per_slice, used;      // components per slice; slices that hold a component (<= ns)
};
static inline ApSplit ap_split(int64_t C, int ns) {
  const int64_t units = (C + kApSliceUnit - 1) / kApSliceUnit;
  const int per = (int)((units + ns - 1) / ns) * kApSliceUnit;
  return ApSplit{per, (int)((C + per - 1) / per)};
}

// joint (and own) terms of one slice of the chunk: part_joint / part_own [slice][M]
__global__ __launch_bounds__(kApBlock) void aggpost_joint(const float* __restrict__ z, const int M, const int L,
                                                          const float* __restrict__ mu, const float* __restrict__ sigma,
                                                          const float* __restrict__ logw, const int C, const long long c_first,
                                                          const long long cpo, const long long* __restrict__ qown,
                                                          const int per_slice, ApState* __restrict__ part_joint,
                                                          ApState* __restrict__ part_own) {
  __shared__ __attribute__((aligned(16))) float s_mu[kApJointTile][kApJointLd];
  __shared__ __attribute__((aligned(16))) float s_inv[kApJointTile][kApJointLd];
  __shared__ float s_lwc[kApJointTile];
  const int tid = threadIdx.x;
  const long long m = (long long)blockIdx.x * kApBlock + tid;
  const bool live = m < M;
  const float* __restrict__ zr = z + (size_t)(live ? m : 0) * L;      // (a lane past the end computes on row 0 and writes nothing)
  const int c_lo = (int)blockIdx.y * per_slice, c_hi = min(C, c_lo + per_slice);
  // the query's own components, as chunk-local indices [own_lo, own_lo + own_n), clipped to the chunk
  int own_lo = 0, own_n = 0;
  if (qown && live) {
    const long long lo = qown[m] * cpo - c_first, a = max(lo, 0ll), b = min(lo + cpo, (long long)C);
    if (b > a) { own_lo = (int)a; own_n = (int)(b - a); }
  }
  double Mj = 0.0, Sj = 0.0, Mo = 0.0, So = 0.0;
  const int ct_st = tid >> 3, j_st = tid & 7;      // staging: 8 threads per component
  for (int c0 = c_lo; c0 < c_hi; c0 += kApJointTile) {
    float acc[kApJointTile];
#pragma unroll
    for (int i = 0; i < kApJointTile; ++i) acc[i] = 0.f;
    const int cs = c0 + ct_st;
    const bool cvalid = cs < c_hi;
    float lsum = 0.f;      // - sum_d log sigma over this thread's dimensions of component cs
    for (int d0 = 0; d0 < L; d0 += kApJointDims) {
      const int dn = min(kApJointDims, L - d0), dn8 = (dn + 7) & ~7;
      __syncthreads();
      for (int j = j_st; j < dn8; j += 8) {
        float mv = 0.f, iv = 0.f;
        if (cvalid && j < dn) {
          const size_t o = (size_t)cs * L + d0 + j;
          const float sg = sigma[o];
          mv = mu[o];
          iv = 1.f / sg;
          lsum -= logf(sg);
        }
        s_mu[ct_st][j] = mv;
        s_inv[ct_st][j] = iv;
      }
      if (d0 + kApJointDims >= L) {      // the last round: the component's constant, its 8 partials added by a fixed tree
        float t = lsum;
        t += __shfl_xor(t, 1);
        t += __shfl_xor(t, 2);
        t += __shfl_xor(t, 4);
        if (j_st == 0) s_lwc[ct_st] = cvalid ? logw[cs] + (t - (float)L * kApHalfLog2Pi) : -INFINITY;
      }
      __syncthreads();
      for (int d = 0; d < dn8; d += 8) {
        float zz[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) zz[j] = (d + j < dn) ? zr[d0 + d + j] : 0.f;
#pragma unroll
        for (int ct = 0; ct < kApJointTile; ++ct) {
          const float4 a0 = *reinterpret_cast<const float4*>(&s_mu[ct][d]), a1 = *reinterpret_cast<const float4*>(&s_mu[ct][d + 4]);
          const float4 b0 = *reinterpret_cast<const float4*>(&s_inv[ct][d]), b1 = *reinterpret_cast<const float4*>(&s_inv[ct][d + 4]);
          const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
          const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
          float a = acc[ct];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float r = (zz[j] - av[j]) * bv[j];
            a = fmaf(r, r, a);
          }
          acc[ct] = a;
        }
      }
    }
    // the tile's terms, its max and its fp32 sum; the own components' likewise, from the same terms
    float tm = -INFINITY, tmo = -INFINITY;
#pragma unroll
    for (int ct = 0; ct < kApJointTile; ++ct) {
      const float s = s_lwc[ct] - 0.5f * acc[ct];
      acc[ct] = s;
      tm = fmaxf(tm, s);
      if ((unsigned)(c0 + ct - own_lo) < (unsigned)own_n) tmo = fmaxf(tmo, s);
    }
    if (tm > -INFINITY) {
      float ts = 0.f, tso = 0.f;
#pragma unroll
      for (int ct = 0; ct < kApJointTile; ++ct) {
        ts += __expf(acc[ct] - tm);
        if ((unsigned)(c0 + ct - own_lo) < (unsigned)own_n) tso += __expf(acc[ct] - tmo);
      }
      ap_fold(Mj, Sj, (double)tm, (double)ts);
      ap_fold(Mo, So, (double)tmo, (double)tso);
    }
  }
  if (live) {
    const size_t o = (size_t)blockIdx.y * M + m;
    part_joint[o] = ApState{Mj, Sj};
    part_own[o] = ApState{Mo, So};
  }
}

// per-dimension terms of one slice of the chunk, dimensions [8 blockIdx.z, + 8): part_dim [slice][M][L]
__global__ __launch_bounds__(kApBlock) void aggpost_dim(const float* __restrict__ z, const int M, const int L,
                                                        const float* __restrict__ mu, const float* __restrict__ sigma,
                                                        const float* __restrict__ logw, const int C, const int per_slice,
                                                        ApState* __restrict__ part_dim) {
  __shared__ __attribute__((aligned(16))) float s_mu[kApDimTile][kApDimDims];
  __shared__ __attribute__((aligned(16))) float s_inv[kApDimTile][kApDimDims];
  __shared__ __attribute__((aligned(16))) float s_lc[kApDimTile][kApDimDims];
  const int tid = threadIdx.x;
  const long long m = (long long)blockIdx.x * kApBlock + tid;
  const bool live = m < M;
  const int d0 = (int)blockIdx.z * kApDimDims, dn = min(kApDimDims, L - d0);
  const int c_lo = (int)blockIdx.y * per_slice, c_hi = min(C, c_lo + per_slice);
  float zz[kApDimDims];
  {
    const float* __restrict__ zr = z + (size_t)(live ? m : 0) * L + d0;
#pragma unroll
    for (int j = 0; j < kApDimDims; ++j) zz[j] = j < dn ? zr[j] : 0.f;
  }
  double Md[kApDimDims], Sd[kApDimDims];
#pragma unroll
  for (int j = 0; j < kApDimDims; ++j) Md[j] = Sd[j] = 0.0;
  for (int c0 = c_lo; c0 < c_hi; c0 += kApDimTile) {
    const int nct = min(kApDimTile, c_hi - c0);
    __syncthreads();
    for (int e = tid; e < kApDimTile * kApDimDims; e += kApBlock) {
      const int ct = e >> 3, j = e & 7;
      float mv = 0.f, iv = 0.f, lc = -INFINITY;
      if (ct < nct && j < dn) {
        const size_t o = (size_t)(c0 + ct) * L + d0 + j;
        const float sg = sigma[o];
        mv = mu[o];
        iv = 1.f / sg;
        lc = logw[c0 + ct] - logf(sg) - kApHalfLog2Pi;
      }
      s_mu[ct][j] = mv;
      s_inv[ct][j] = iv;
      s_lc[ct][j] = lc;
    }
    __syncthreads();
    float tm[kApDimDims], ts[kApDimDims];
#pragma unroll
    for (int j = 0; j < kApDimDims; ++j) tm[j] = -INFINITY;
#pragma unroll 4
    for (int ct = 0; ct < nct; ++ct) {
      const float4 a0 = *reinterpret_cast<const float4*>(&s_mu[ct][0]), a1 = *reinterpret_cast<const float4*>(&s_mu[ct][4]);
      const float4 b0 = *reinterpret_cast<const float4*>(&s_inv[ct][0]), b1 = *reinterpret_cast<const float4*>(&s_inv[ct][4]);
      const float4 l0 = *reinterpret_cast<const float4*>(&s_lc[ct][0]), l1 = *reinterpret_cast<const float4*>(&s_lc[ct][4]);
      const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      const float lv[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
#pragma unroll
      for (int j = 0; j < kApDimDims; ++j) {
        const float r = (zz[j] - av[j]) * bv[j];
        tm[j] = fmaxf(tm[j], fmaf(-0.5f * r, r, lv[j]));
      }
    }
    // (a dimension whose terms are all -inf keeps an empty tile: exp(-inf - 0) = 0)
#pragma unroll
    for (int j = 0; j < kApDimDims; ++j) { ts[j] = 0.f; tm[j] = tm[j] > -INFINITY ? tm[j] : 0.f; }
#pragma unroll 4
    for (int ct = 0; ct < nct; ++ct) {
      const float4 a0 = *reinterpret_cast<const float4*>(&s_mu[ct][0]), a1 = *reinterpret_cast<const float4*>(&s_mu[ct][4]);
      const float4 b0 = *reinterpret_cast<const float4*>(&s_inv[ct][0]), b1 = *reinterpret_cast<const float4*>(&s_inv[ct][4]);
      const float4 l0 = *reinterpret_cast<const float4*>(&s_lc[ct][0]), l1 = *reinterpret_cast<const float4*>(&s_lc[ct][4]);
      const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      const float lv[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
#pragma unroll
      for (int j = 0; j < kApDimDims; ++j) {
        const float r = (zz[j] - av[j]) * bv[j];
        ts[j] += __expf(fmaf(-0.5f * r, r, lv[j]) - tm[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kApDimDims; ++j) ap_fold(Md[j], Sd[j], (double)tm[j], (double)ts[j]);
  }
  if (live) {
    ApState* __restrict__ o = part_dim + ((size_t)blockIdx.y * M + m) * L + d0;
#pragma unroll
    for (int j = 0; j < kApDimDims; ++j)
      if (j < dn) o[j] = ApState{Md[j], Sd[j]};
  }
}

// the slices' partial states folded into the running state, in slice order: run [E], part [ns][E]
__global__ __launch_bounds__(kApBlock) void aggpost_fold(ApState* __restrict__ run, const ApState* __restrict__ part,
                                                         const unsigned long long E, const int ns) {
  const unsigned long long e = (unsigned long long)blockIdx.x * kApBlock + threadIdx.x;
  if (e >= E) return;
  ApState r = run[e];
  for (int s = 0; s < ns; ++s) {
    const ApState p = part[(size_t)s * E + e];
    ap_fold(r.m, r.s, p.m, p.s);
  }
  run[e] = r;
}

// the outputs from the running state: max + log(sum) - log_norm (own: no log_norm); an empty state is -inf
__global__ __launch_bounds__(kApBlock) void aggpost_finish(const ApState* __restrict__ run, const unsigned long long M,
                                                           const unsigned long long E, const double log_norm,
                                                           float* __restrict__ log_joint, float* __restrict__ log_own,
                                                           float* __restrict__ log_dim) {
  const unsigned long long e = (unsigned long long)blockIdx.x * kApBlock + threadIdx.x;
  if (e >= E) return;
  float* const out = e < M ? (log_joint ? log_joint + e : nullptr)
                   : e < 2 * M ? (log_own ? log_own + (e - M) : nullptr)
                               : (log_dim ? log_dim + (e - 2 * M) : nullptr);
  if (!out) return;
  const ApState r = run[e];
  const double sub = (e >= M && e < 2 * M) ? 0.0 : log_norm;
  *out = r.s > 0.0 ? (float)(r.m + log(r.s) - sub) : -INFINITY;
}

}  // namespace gmvae
