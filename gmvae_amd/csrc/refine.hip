// gmvae_refine: the host side of csrc/refine.hpp (include/gmvae_hip.h).  A translation unit -- and so a device code object -- of its
// own, for the reason csrc/tsne.hip gives: the training step's code object is what it was without these kernels, and so is
// gmvae_ais's (csrc/ais.hpp is included here, not edited).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gmvae_hip.h"
#include "refine.hpp"

using namespace refine_tu;

namespace {

int aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

constexpr int kRefineLaunchSteps = 256;      // steps (or rounds) per launch unless GMVAE_REFINE_LAUNCH_STEPS says otherwise

// Everything gmvae_refine refuses that does not need a pointer: gmvae_ais's sizes and likelihood, the counts.
int refine_check(const GmvaeDims* d, int model, int n_steps, int n_samples, int n_eval_rounds) {
  if (!d) return GMVAE_E_NULL;
  if (model < 0 || model > 2) return GMVAE_E_MODEL;
  if (d->B < 1 || d->D < 1 || d->L < 1 || d->L > kAisMaxL) return GMVAE_E_DIMS;
  if (model != GMVAE_MODEL_VAE && (d->K < 1 || d->K > kAisMaxK)) return GMVAE_E_DIMS;
  if (d->n_hidden < 0 || d->n_hidden > kAisMaxHidden) return GMVAE_E_DIMS;
  for (int i = 0; i < d->n_hidden; ++i)
    if (d->hidden[i] < 1 || d->hidden[i] > kAisMaxWidth) return GMVAE_E_DIMS;
  if (d->hidden_act < GMVAE_ACT_RELU || d->hidden_act > GMVAE_ACT_ELU) return GMVAE_E_DIMS;
  if (d->gen_bias_vec ? d->gen_bias_len != d->D : d->gen_bias_len != 0) return GMVAE_E_DIMS;
  if (d->sched_flags & (GMVAE_LIK_MASK | GMVAE_OBJ_PIXEL_MASK | GMVAE_X_F32 | GMVAE_LIK_SCALE_LEARNED)) return GMVAE_E_DIMS;
  if (n_samples != 1 && n_samples != 2 && n_samples != 4 && n_samples != 8 && n_samples != 16) return GMVAE_E_DIMS;
  if (n_steps < 0 || n_eval_rounds < 1 || (long long)n_steps + n_eval_rounds > (1 << 24)) return GMVAE_E_DIMS;
  const uint64_t end = d->row0 + (uint64_t)d->B;
  if (end < d->row0 || end > ((1ull << 38) - 1) / (uint64_t)n_samples) return GMVAE_E_DIMS;      // ((row0 + B) S < 2^38: Philox's row field)
  if ((uint64_t)d->B * (uint64_t)n_samples > (1ull << 30)) return GMVAE_E_DIMS;
  if (ais_lds(d->L, d->n_hidden, d->hidden).total > kAisLdsLimit) return GMVAE_E_DIMS;
  return 0;
}

uint64_t up256(uint64_t b) { return (b + 255) / 256 * 256; }

// Workspace: the prior table, the examples' state, the rows' running sums, the per-example bounds.  O(B (L + S)), independent of
// n_steps and n_eval_rounds.
struct RefineWs {
  uint64_t prior_c, prior_lw, prior_mu, prior_sg, acc, fin, phi, cnt, total;
};
RefineWs refine_ws(const GmvaeDims& d, int model, int n_samples) {
  RefineWs w;
  const uint64_t Kp = model == GMVAE_MODEL_VAE ? 1 : (uint64_t)d.K, L = (uint64_t)d.L, B = (uint64_t)d.B;
  uint64_t o = 0;
  w.prior_c = o; o += up256(Kp * sizeof(double));
  w.prior_lw = o; o += up256(Kp * sizeof(float));
  w.prior_mu = o; o += up256(Kp * L * sizeof(float));
  w.prior_sg = o; o += up256(Kp * L * sizeof(float));
  w.acc = o; o += up256(B * (uint64_t)n_samples * 8 * sizeof(double));
  w.fin = o; o += up256(B * 4 * sizeof(double));
  w.phi = o; o += up256(B * 6 * L * sizeof(float));
  w.cnt = o; o += up256(B * sizeof(int));
  w.total = o;
  return w;
}

const float* find_param(const float* params, const GmvaeParamEntry* e, int n, const char* name) {
  for (int i = 0; i < n; ++i)
    if (!strcmp(e[i].name, name)) return params + e[i].offset;
  return nullptr;
}

}  // namespace

extern "C" {

int gmvae_refine_workspace_bytes(const GmvaeDims* dims, int model, int n_samples, uint64_t* bytes) {
  if (int e = refine_check(dims, model, 0, n_samples, 1)) return e;
  if (!bytes) return GMVAE_E_NULL;
  *bytes = refine_ws(*dims, model, n_samples).total;
  return 0;
}

int gmvae_refine(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, const float* start, int n_steps,
                 int n_samples, int n_eval_rounds, float lr, float beta1, float beta2, float adam_eps, const float* eps,
                 float* phi_out, float* trace_out, float* stats_out, float* tail, void* workspace, uint64_t seed, uint64_t step,
                 void* stream) {
  if (int e = refine_check(dims, model, n_steps, n_samples, n_eval_rounds)) return e;
  if (!(lr > 0.f) || !(lr < INFINITY)) return GMVAE_E_DIMS;
  if (!(beta1 >= 0.f) || !(beta1 < 1.f) || !(beta2 >= 0.f) || !(beta2 < 1.f) || !(adam_eps >= 0.f) || !(adam_eps < INFINITY))
    return GMVAE_E_DIMS;
  if (!x || !params || !start || !tail || !workspace) return GMVAE_E_NULL;
  if (!aligned_to(params, 16) || !aligned_to(start, 4) || !aligned_to(eps, 4) || !aligned_to(phi_out, 4) ||
      !aligned_to(trace_out, 4) || !aligned_to(stats_out, 4) || !aligned_to(tail, 4) || !aligned_to(workspace, 256) ||
      !aligned_to(dims->gen_bias_vec, 4))
    return GMVAE_E_ALIGN;
  const GmvaeDims& d = *dims;

  // the decoder and the prior's parameters by name (gmvae_param_layout: the reference's variable names)
  GmvaeDims dl = d;
  dl.S = 1;
  dl.sched_flags = 0;
  int n_ent = 0;
  if (int e = gmvae_param_layout(&dl, model, nullptr, 0, &n_ent)) return e;
  GmvaeParamEntry* ent = static_cast<GmvaeParamEntry*>(malloc(sizeof(GmvaeParamEntry) * (size_t)n_ent));
  if (!ent) return GMVAE_E_SMALL;
  if (int e = gmvae_param_layout(&dl, model, ent, n_ent, &n_ent)) { free(ent); return e; }

  const RefineWs w = refine_ws(d, model, n_samples);
  char* const ws = static_cast<char*>(workspace);
  RefineArgs ra;
  memset(&ra, 0, sizeof(ra));
  AisArgs& a = ra.a;
  a.D = d.D; a.L = d.L; a.n_hidden = d.n_hidden; a.act = d.hidden_act;
  for (int i = 0; i < d.n_hidden; ++i) a.hidden[i] = d.hidden[i];
  a.C = n_samples;
  a.n = (long long)d.B * n_samples;
  a.enc = 0;                                      // A = log p(z), B = log p(x|z)
  a.Kp = model == GMVAE_MODEL_VAE ? 1 : d.K;
  bool found = true;
  char name[64];
  for (int i = 0; i <= d.n_hidden; ++i) {
    snprintf(name, sizeof(name), "decoder_fcnet/linear_%d/w", i);
    a.w[i] = find_param(params, ent, n_ent, name);
    snprintf(name, sizeof(name), "decoder_fcnet/linear_%d/b", i);
    a.b[i] = find_param(params, ent, n_ent, name);
    found = found && a.w[i] && a.b[i];
  }
  AisPrep p;
  memset(&p, 0, sizeof(p));
  p.model = model; p.L = d.L; p.Kp = a.Kp;
  p.raw_sigma_bias = d.raw_sigma_bias; p.sigma_min = d.sigma_min;
  if (model == GMVAE_MODEL_VAE_GMP) {
    p.p0 = find_param(params, ent, n_ent, "loc");
    p.p1 = find_param(params, ent, n_ent, "raw_scale_diag");
    p.p2 = find_param(params, ent, n_ent, "mixture_logits");
    found = found && p.p0 && p.p1 && p.p2;
  } else if (model == GMVAE_MODEL_GMVAE) {
    p.p0 = find_param(params, ent, n_ent, "prior_gmm_fcnet/linear_0/w");
    p.p1 = find_param(params, ent, n_ent, "prior_gmm_fcnet/linear_0/b");
    found = found && p.p0 && p.p1;
  }
  free(ent);
  if (!found) return GMVAE_E_MODEL;
  p.lw = reinterpret_cast<float*>(ws + w.prior_lw);
  p.cst = reinterpret_cast<double*>(ws + w.prior_c);
  p.mu = reinterpret_cast<float*>(ws + w.prior_mu);
  p.sg = reinterpret_cast<float*>(ws + w.prior_sg);

  a.gen_bias = d.gen_bias_init;
  a.gen_bias_vec = static_cast<const float*>(d.gen_bias_vec);
  a.x = x;
  a.prior_lw = p.lw; a.prior_c = p.cst; a.prior_mu = p.mu; a.prior_sg = p.sg;
  const int total = n_steps + n_eval_rounds;      // the timeline: the steps, then the rounds
  a.T = total;                                    // (ais_noise keys the draw of t by step (T + 1) + t)
  a.eps = eps;
  a.row_base = d.row0 * (uint64_t)n_samples; a.seed = seed; a.step = step;
  ra.B = d.B; ra.S = n_samples; ra.n_steps = n_steps;
  ra.lr = lr; ra.b1 = beta1; ra.b2 = beta2; ra.aeps = adam_eps;
  ra.start = start;
  ra.phi = reinterpret_cast<float*>(ws + w.phi);
  ra.cnt = reinterpret_cast<int*>(ws + w.cnt);
  ra.acc = reinterpret_cast<double*>(ws + w.acc);
  ra.trace = trace_out;

  // steps per launch: no single launch runs long on a shared card (GMVAE_REFINE_LAUNCH_STEPS: the tests' cut; the result does
  // not depend on it)
  int cap = kRefineLaunchSteps;
  if (const char* s = getenv("GMVAE_REFINE_LAUNCH_STEPS")) {
    const int v = atoi(s);
    if (v >= 1) cap = v;
  }
  const unsigned lds = ais_lds(d.L, d.n_hidden, a.hidden).total;
  hipStream_t st = static_cast<hipStream_t>(stream);
  (void)hipGetLastError();
  if (lds > 64u * 1024u) {
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(refine_run), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)kAisLdsLimit))
      return (int)e;
  }
  hipLaunchKernelGGL(ais_prep, dim3(1), dim3(kAisThreads), 0, st, p);
  const unsigned panels = (unsigned)((a.n + kAisRows - 1) / kAisRows);
  for (int t_lo = 0; t_lo < total;) {
    const int t_hi = (int)(((long long)t_lo + cap < total) ? t_lo + cap : total) - 1;
    ra.t_lo = t_lo; ra.t_hi = t_hi;
    hipLaunchKernelGGL(refine_run, dim3(panels), dim3(kAisThreads), lds, st, ra);
    t_lo = t_hi + 1;
  }
  double* const fin = reinterpret_cast<double*>(ws + w.fin);
  hipLaunchKernelGGL(refine_finish, dim3((unsigned)((d.B + kAisThreads - 1) / kAisThreads)), dim3(kAisThreads), 0, st, ra.phi, start,
                     ra.cnt, ra.acc, d.B, d.L, n_samples, n_eval_rounds, phi_out, stats_out, fin);
  hipLaunchKernelGGL(ais_tail, dim3(1), dim3(kAisThreads), 0, st, fin, d.B, tail);
  return (int)hipGetLastError();
}

}  // extern "C"
