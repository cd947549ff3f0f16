// gmvae_iw_bound on every shape and schedule the one-launch evaluation (evalf.hpp) does not take: per chunk of S samples a strided
// Philox fill of eps / u, the forward with that explicit noise (its per-sample rows [B S][4] in the workspace), and iw_merge, which
// folds the chunk into the fp64 row state (evalf.hpp iw_fold).  The last chunk adds iw_tail: the batch sums in a fixed order.
// gmvae_iw_bound_enum_y (y summed out over K) is the same loop at S K rows per batch row with iw_merge_enum in iw_merge's place.
// gmvae_posterior_y is that loop with iw_merge_post in the merge's place (the fold kept per component), then iw_post_finish.
// gmvae_posterior_component (VAE_GMP) is gmvae_iw_bound's loop with the mixture's logsumexp left open: evalf_rows_v<7, 64> per chunk
// at the evalf sizes, iw_merge_comp in iw_merge's place everywhere else; then iw_post_comp_finish and iw_tail.
#pragma once
#include "evalf.hpp"

namespace gmvae {

// eps [B S][L], u [B S][K] (either may be null) of one chunk: row b S + s draws Philox row (row0 + b) n + s0 + s
__global__ __launch_bounds__(256) void iw_noise_fill(float* eps, float* u, const int B, const int S, const int L, const int K,
                                                     const unsigned long long row0, const unsigned long long n,
                                                     const unsigned long long s0, const unsigned long long seed,
                                                     const unsigned long long step) {
  const unsigned long long rows = (unsigned long long)B * S;
  const unsigned qe = eps ? (unsigned)(L + 3) / 4 : 0u, qu = u ? (unsigned)(K + 3) / 4 : 0u;
  const unsigned long long n_e = rows * qe;
  unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_e + rows * qu) return;
  const bool is_u = i >= n_e;
  if (is_u) i -= n_e;
  const unsigned qpr = is_u ? qu : qe;
  const unsigned long long row = i / qpr;
  const unsigned quad = (unsigned)(i - row * qpr);
  const unsigned long long b = row / (unsigned)S;
  float o[4];
  noise_vals((row0 + b) * n + s0 + (row - b * (unsigned)S), quad, is_u, seed, step, o);
  const int w = is_u ? K : L;
  float* const dst = (is_u ? u : eps) + row * (unsigned long long)w + quad * 4;
  if ((w & 3) == 0) {
    *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((int)quad * 4 + j < w) dst[j] = o[j];
  }
}

// a wave per batch row: the chunk's samples s < n - s0 of rows_ws [B S][4] (log p(x|z), log q, log p, log w) in fp64, folded into
// iw_state; on the last chunk the row's (-bound, mean nll, mean kl) go to slots [B][4] for iw_tail
__global__ __launch_bounds__(256) void iw_merge(const EvalArgs a) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const int S = a.S, cnt = (int)min((unsigned long long)S, a.iw_n - a.iw_s0);
  const float* const rw = a.rows_ws + b * S * 4;
  float mx = -INFINITY;
  for (int s = lane; s < cnt; s += 64) mx = fmaxf(mx, rw[4 * s + 3]);
  mx = Wave64::max(mx);
  double se = 0., slw = 0., nl = 0., kl = 0.;
  for (int s = lane; s < cnt; s += 64) {
    const float4 v = *reinterpret_cast<const float4*>(rw + 4 * s);
    se += exp((double)v.w - (double)mx);
    slw += v.w;
    nl -= v.x;
    kl += (double)v.y - (double)v.z;
  }
  se = iw_wave_sum(se); slw = iw_wave_sum(slw); nl = iw_wave_sum(nl); kl = iw_wave_sum(kl);
  float o_loss, o_nl, o_kl;
  iw_fold(a, b, lane, mx, se, slw, nl, kl, o_loss, o_nl, o_kl);
  if (a.iw_final && lane == 0) *reinterpret_cast<float4*>(a.slots + 4 * b) = make_float4(o_loss, o_nl, o_kl, 0.f);
}

// gmvae_iw_bound_enum_y: a wave per batch row b, y summed out.  The chunk's rows_ws [B S K][4] (row (b S + s) K + k: log p(x|z),
// log q, log p, log w' = log p(x|z) + log p(z|e_k) - log q(z|x,e_k)) of its samples s < n - s0, with q = softmax(logits_b) and
// nent_b = sum_k q_k ln q_k (row_lse_parts and the arithmetic of ymarg_rows), fold into iw_state as
//   max and sum of exp over (s, k) of log w';  sum log w += sum_s (sum_k q_k log w'_sk - nent_b);  nll, kl: q-weighted sums.
// On the last chunk the row's (-bound, mean nll, mean kl, nent_b) go to slots [B][4] for iw_tail.
__global__ __launch_bounds__(256) void iw_merge_enum(const EvalArgs a, const float* __restrict__ logits, const int K) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const float* const lg = logits + b * K;
  float m, l;
  row_lse_parts(lg, K, lane, m, l);
  float ne = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float lpi = (lg[k] - m) - l, q = expf(lpi);
    ne += q * lpi;
  }
  ne = wave_sum(ne);
  const int cnt = (int)min((unsigned long long)a.S, a.iw_n - a.iw_s0), nr = cnt * K;
  const float* const rw = a.rows_ws + b * a.S * K * 4;
  float mx = -INFINITY;
  for (int j = lane; j < nr; j += 64) mx = fmaxf(mx, rw[4 * j + 3]);
  mx = Wave64::max(mx);
  double se = 0., slw = 0., nl = 0., kl = 0.;
  for (int j = lane; j < nr; j += 64) {
    const float4 v = *reinterpret_cast<const float4*>(rw + 4 * j);
    const int k = j % K;
    const double q = expf((lg[k] - m) - l);
    se += exp((double)v.w - (double)mx);
    slw += q * v.w;
    nl -= q * v.x;
    kl += q * ((double)v.y - (double)v.z);
  }
  se = iw_wave_sum(se); slw = iw_wave_sum(slw) - (double)cnt * ne; nl = iw_wave_sum(nl); kl = iw_wave_sum(kl);
  float o_loss, o_nl, o_kl;
  iw_fold(a, b, lane, mx, se, slw, nl, kl, o_loss, o_nl, o_kl);
  if (a.iw_final && lane == 0) *reinterpret_cast<float4*>(a.slots + 4 * b) = make_float4(o_loss, o_nl, o_kl, ne);
}

// one workgroup: tail[0..2] = the sums of slots [B][4] over b (fixed order: strided fp64 partials, then a fixed tree), tail[3] =
// nent_tail[3] (the sum of -H(q(y|x)) over the batch from the last chunk's forward: it does not depend on the noise) or, with
// nent_tail null, the same sum of slots[b][3] (iw_merge_enum's nent_b), tail[4] = B
__global__ __launch_bounds__(256) void iw_tail(const float* slots, const int B, const float* nent_tail, float* tail) {
  __shared__ double red[4][256];
  const int t = threadIdx.x;
  double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
  for (int b = t; b < B; b += 256) { s0 += slots[4 * b]; s1 += slots[4 * b + 1]; s2 += slots[4 * b + 2]; s3 += slots[4 * b + 3]; }
  red[0][t] = s0; red[1][t] = s1; red[2][t] = s2; red[3][t] = s3;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) { red[0][t] += red[0][t + h]; red[1][t] += red[1][t + h]; red[2][t] += red[2][t + h]; red[3][t] += red[3][t + h]; }
    __syncthreads();
  }
  if (t == 0) {
    tail[0] = (float)red[0][0]; tail[1] = (float)red[1][0]; tail[2] = (float)red[2][0];
    tail[3] = nent_tail ? nent_tail[3] : (float)red[3][0]; tail[4] = (float)B; tail[5] = 0.f; tail[6] = 0.f; tail[7] = 0.f;
  }
}

// gmvae_posterior_y: the chunk's rows_ws [B S K][4] (as iw_merge_enum reads them; only .w = log w'_bsk is used) folded PER COMPONENT
// into post [B][K][3] fp64: (max_s log w', sum_s exp(log w' - max), sum_s exp(2 (log w' - max))) over the samples s < n - s0.
// A wave per batch row.  The components go in tiles of Kt = min(64, K - k0); inside a tile lane g Kt + k (g < G = 64 / Kt) walks
// the samples g, g + G, ... of component k0 + k, so at K = 10 sixty of the 64 lanes work (K = 80: a 64-wide tile, then a 16-wide
// one at G = 4).  The G partial sums of a component meet in lane k by lane shuffles in the order g = 0 .. G - 1, and that lane --
// the only owner of (b, k) -- writes the state on the first chunk and rescales and rewrites it on later ones (plain stores).
__global__ __launch_bounds__(256) void iw_merge_post(const float* __restrict__ rows_ws, double* __restrict__ post, const int B,
                                                     const int S, const int K, const unsigned long long n,
                                                     const unsigned long long s0) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int cnt = (int)min((unsigned long long)S, n - s0);
  const float* const rw = rows_ws + b * S * K * 4;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int Kt = min(64, K - k0), G = 64 / Kt;
    const int g = lane / Kt, kl = lane - g * Kt;
    const bool on = g < G;
    const float* const col = rw + 4 * (k0 + kl) + 3;
    float mx = -INFINITY;
    if (on)
      for (int s = g; s < cnt; s += G) mx = fmaxf(mx, col[4 * (long long)s * K]);
    for (int j = 1; j < G; ++j) mx = fmaxf(mx, __shfl(mx, ((g + j) % G) * Kt + kl, 64));   // (max: the same in any order)
    double p1 = 0., p2 = 0.;
    if (on)
      for (int s = g; s < cnt; s += G) {
        const double e = exp((double)col[4 * (long long)s * K] - (double)mx);
        p1 += e;
        p2 += e * e;
      }
    double s1 = 0., s2 = 0.;
    for (int j = 0; j < G; ++j) { s1 += __shfl(p1, j * Kt + kl, 64); s2 += __shfl(p2, j * Kt + kl, 64); }
    if (lane < Kt) {
      double* const st = post + (b * K + k0 + lane) * 3;
      double m = mx;
      if (s0 != 0) {
        const double m0 = st[0];
        m = fmax(m0, (double)mx);
        const double r0 = exp(m0 - m), r1 = exp((double)mx - m);
        s1 = st[1] * r0 + s1 * r1;
        s2 = st[2] * r0 * r0 + s2 * r1 * r1;
      }
      st[0] = m; st[1] = s1; st[2] = s2;
    }
  }
}

// gmvae_posterior_y after the last chunk: a wave per batch row b, lanes over k.  From post [B][K][3] and q = softmax(logits_b)
// (row_lse_parts, as iw_merge_enum):  l_k = max_k + ln(sum_k) - ln n -> log_joint;  bound = logsumexp_k l_k;  ln r_k = l_k - bound
// -> log_post;  H(r) = -sum r ln r;  KL(q || r) = sum_k q_k (ln q_k - ln r_k);  ESS = (sum_k e^{M_k - M} sum_k)^2 /
// sum_k e^{2 (M_k - M)} sumsq_k.  (bound, H, KL, ESS) -> stats [B][4]; (-bound, H, KL, ESS) -> slots [B][4] for iw_tail.
__global__ __launch_bounds__(256) void iw_post_finish(const double* __restrict__ post, const float* __restrict__ logits,
                                                      const int B, const int K, const unsigned long long n,
                                                      float* __restrict__ log_joint, float* __restrict__ log_post,
                                                      float* __restrict__ stats, float* __restrict__ slots) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const double* const st = post + b * K * 3;
  const float* const lg = logits + b * K;
  float m, l;
  row_lse_parts(lg, K, lane, m, l);
  const double ln_n = log((double)n);
  double M = -INFINITY;
  for (int k = lane; k < K; k += 64) M = fmax(M, st[3 * k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) M = fmax(M, __shfl_xor(M, o, 64));
  double a1 = 0., a2 = 0.;                            // sums of w and w^2 over (s, k), in units of e^M and e^{2M}
  for (int k = lane; k < K; k += 64) {
    const double r = exp(st[3 * k] - M);
    a1 += r * st[3 * k + 1];
    a2 += r * r * st[3 * k + 2];
  }
  a1 = iw_wave_sum(a1); a2 = iw_wave_sum(a2);
  const double bound = M + log(a1) - ln_n;
  double h = 0., kl = 0.;
  for (int k = lane; k < K; k += 64) {
    const double lj = st[3 * k] + log(st[3 * k + 1]) - ln_n, lr = lj - bound;
    const float lq = (lg[k] - m) - l;
    h -= exp(lr) * lr;
    kl += (double)expf(lq) * ((double)lq - lr);
    if (log_joint) log_joint[b * K + k] = (float)lj;
    if (log_post) log_post[b * K + k] = (float)lr;
  }
  h = iw_wave_sum(h); kl = iw_wave_sum(kl);
  if (lane == 0) {
    const float ess = (float)(a1 * a1 / a2);
    if (stats) *reinterpret_cast<float4*>(stats + 4 * b) = make_float4((float)bound, (float)h, (float)kl, ess);
    *reinterpret_cast<float4*>(slots + 4 * b) = make_float4((float)-bound, (float)h, (float)kl, ess);
  }
}

// gmvae_posterior_component on the general schedule: the chunk's rows_ws [B S][4] (log p(x|z), log q, log p(z), log w) and the
// forward's z [B S][L] folded PER COMPONENT into state [B][K][2] fp64 = (max_s log w_bsk, sum_s exp(log w_bsk - max)), with
//   log w_bsk = log p(x|z) - log q + comp_k(z),  comp_k = cst[k] - 1/2 sum_l ((z_l - loc_kl) inv_kl)^2
// recomputed from z in the log domain as mixture_logprob_tiled does (inv, cst: gmp_consts) -- never from the responsibilities, which
// underflow for far components --, and the row's own weights (.w) into ess [B][3] (evalf.hpp pc_fold_ess).  A wave per batch row;
// lanes as iw_merge_post: component tiles of Kt = min(64, K - k0), lane g Kt + k walks the samples g, g + G, ... (G = 64 / Kt) with a
// running (max, sum) pair in fp64, the G pairs of a component meet in lane k in the order g = 0 .. G - 1, and that lane -- the only
// owner of (b, k) -- writes the state (plain stores).
__global__ __launch_bounds__(256) void iw_merge_comp(const float* __restrict__ rows_ws, const float* __restrict__ z,
                                                     const float* __restrict__ loc, const float* __restrict__ inv,
                                                     const float* __restrict__ cst, double* __restrict__ state,
                                                     double* __restrict__ ess, const int B, const int S, const int L, const int K,
                                                     const unsigned long long n, const unsigned long long s0) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int cnt = (int)min((unsigned long long)S, n - s0);
  const float* const rw = rows_ws + b * S * 4;
  const float* const zb = z + b * S * L;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int Kt = min(64, K - k0), G = 64 / Kt;
    const int g = lane / Kt, kl = lane - g * Kt;
    const bool on = g < G;
    const float* const lc = loc + (long long)(k0 + kl) * L;
    const float* const iv = inv + (long long)(k0 + kl) * L;
    const float ck = cst[k0 + kl];
    double m = -INFINITY, acc = 0.;
    if (on)
      for (int s = g; s < cnt; s += G) {
        const float* const zs = zb + (long long)s * L;
        float q = 0.f;
        for (int l = 0; l < L; ++l) { const float t = (zs[l] - lc[l]) * iv[l]; q = fmaf(t, t, q); }
        const double lw = (double)((rw[4 * s] - rw[4 * s + 1]) + (ck - 0.5f * q));
        if (lw > m) { acc = acc * exp(m - lw) + 1.; m = lw; }
        else if (lw > -INFINITY) acc += exp(lw - m);   // (a weight of exactly 0 adds nothing)
      }
    double M = -INFINITY;
    for (int j = 0; j < G; ++j) M = fmax(M, __shfl(m, j * Kt + kl, 64));
    double s1 = 0.;
    for (int j = 0; j < G; ++j) {
      const double mj = __shfl(m, j * Kt + kl, 64), aj = __shfl(acc, j * Kt + kl, 64);
      s1 += aj == 0. ? 0. : aj * exp(mj - M);          // (a group without samples: (-inf, 0))
    }
    if (lane < Kt) pc_fold(state + (b * K + k0 + lane) * 2, s0 == 0, M, s1);
  }
  float mr = -INFINITY;
  for (int s = lane; s < cnt; s += 64) mr = fmaxf(mr, rw[4 * s + 3]);
  mr = Wave64::max(mr);
  double e1 = 0., e2 = 0.;
  for (int s = lane; s < cnt; s += 64) {
    const double e = rw[4 * s + 3] > -INFINITY ? exp((double)rw[4 * s + 3] - (double)mr) : 0.;
    e1 += e; e2 += e * e;
  }
  e1 = iw_wave_sum(e1); e2 = iw_wave_sum(e2);
  if (lane == 0) pc_fold_ess(ess + b * 3, s0 == 0, (double)mr, e1, e2);
}

// gmvae_posterior_component after the last chunk: a wave per batch row b, lanes over k (any K: strided).  From state [B][K][2], ess
// [B][3] and ln pi = log_softmax(mixture_logits), all in fp64:  l_k = max_k + ln(sum_k) - ln n -> log_joint (fp32; the rest from it);  bound = logsumexp_k l_k;
// ln r_k = l_k - bound -> log_post;  H(r) = -sum r ln r;  KL(r || pi) = sum_k r_k (ln r_k - ln pi_k);  ESS = (sum_s w)^2 / sum_s w^2.
// (bound, H, KL, ESS) -> stats [B][4]; (-bound, H, KL, ESS) -> slots [B][4] for iw_tail.
__global__ __launch_bounds__(256) void iw_post_comp_finish(const double* __restrict__ state, const double* __restrict__ ess,
                                                           const float* __restrict__ mixlog, const int B, const int K,
                                                           const unsigned long long n, float* __restrict__ log_joint,
                                                           float* __restrict__ log_post, float* __restrict__ stats,
                                                           float* __restrict__ slots) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const double* const st = state + b * K * 2;
  const double ln_n = log((double)n);
  // l_k as log_joint reports it: rounded to fp32 FIRST, so that bound, ln r, H and KL are functions of the call's own log_joint
  auto lj_of = [&](const int k) { return (double)(float)(st[2 * k] + log(st[2 * k + 1]) - ln_n); };
  double pm = -INFINITY, M = -INFINITY;
  for (int k = lane; k < K; k += 64) { pm = fmax(pm, (double)mixlog[k]); M = fmax(M, lj_of(k)); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { pm = fmax(pm, __shfl_xor(pm, o, 64)); M = fmax(M, __shfl_xor(M, o, 64)); }
  double pe = 0., a1 = 0.;
  for (int k = lane; k < K; k += 64) {
    pe += exp((double)mixlog[k] - pm);
    a1 += exp(lj_of(k) - M);
  }
  pe = iw_wave_sum(pe); a1 = iw_wave_sum(a1);
  const double plse = pm + log(pe), bound = M + log(a1);
  double h = 0., kl = 0.;
  for (int k = lane; k < K; k += 64) {
    const double lj = lj_of(k), lr = lj - bound, r = exp(lr);
    h -= r * lr;
    kl += r * (lr - ((double)mixlog[k] - plse));
    if (log_joint) log_joint[b * K + k] = (float)lj;
    if (log_post) log_post[b * K + k] = (float)lr;
  }
  h = iw_wave_sum(h); kl = iw_wave_sum(kl);
  if (lane == 0) {
    const double* const es = ess + b * 3;
    const float e = (float)(es[1] * es[1] / es[2]);
    if (stats) *reinterpret_cast<float4*>(stats + 4 * b) = make_float4((float)bound, (float)h, (float)kl, e);
    *reinterpret_cast<float4*>(slots + 4 * b) = make_float4((float)-bound, (float)h, (float)kl, e);
  }
}

}  // namespace gmvae
