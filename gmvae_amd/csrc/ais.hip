// gmvae_ais: the host side of csrc/ais.hpp (include/gmvae_hip.h).  A translation unit -- and so a device code object -- of its own,
// for the reason csrc/tsne.hip gives: the training step's code object, and with it the placement of the one-launch step's code,
// is what it was without these kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gmvae_hip.h"
#include "ais.hpp"

using namespace gmvae;

namespace {

int aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

constexpr int kAisLaunchTemps = 32;      // transitions per launch unless GMVAE_AIS_LAUNCH_TEMPS says otherwise

// Everything gmvae_ais refuses that does not need a pointer: the sizes csrc/ais.hpp takes, the plain Bernoulli on {0, 1}, the counts.
int ais_check(const GmvaeDims* d, int model, int base_K, int n_temps, int n_chains, int n_leapfrog) {
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
  if (base_K < 0 || base_K > kAisMaxK) return GMVAE_E_DIMS;
  if (n_temps < 1 || n_temps > (1 << 24) || n_chains < 1 || n_leapfrog < 1) return GMVAE_E_DIMS;
  const uint64_t end = d->row0 + (uint64_t)d->B;
  if (end < d->row0 || end > ((1ull << 38) - 1) / (uint64_t)n_chains) return GMVAE_E_DIMS;      // ((row0 + B) C < 2^38: Philox's row field)
  if ((uint64_t)d->B * (uint64_t)n_chains > (1ull << 30)) return GMVAE_E_DIMS;
  if (ais_lds(d->L, d->n_hidden, d->hidden).total > kAisLdsLimit) return GMVAE_E_DIMS;
  return 0;
}

uint64_t up256(uint64_t b) { return (b + 255) / 256 * 256; }

// Workspace: the prior table, the base's constants, the chains' state, the per-example sums.  O(B C L), independent of T.
struct AisWs {
  uint64_t st_bits, prior_c, prior_lw, prior_mu, prior_sg, base_c, st_d, fin, st_z, st_gA, st_gB, st_eps, st_acc, total;
};
AisWs ais_ws(const GmvaeDims& d, int model, int base_K, int n_chains) {
  AisWs w;
  const uint64_t Kp = model == GMVAE_MODEL_VAE ? 1 : (uint64_t)d.K, L = (uint64_t)d.L, n = (uint64_t)d.B * (uint64_t)n_chains;
  uint64_t o = 0;
  w.st_bits = o; o += up256(n * sizeof(uint64_t));      // (first: include/gmvae_hip.h documents it)
  w.prior_c = o; o += up256(Kp * sizeof(double));
  w.prior_lw = o; o += up256(Kp * sizeof(float));
  w.prior_mu = o; o += up256(Kp * L * sizeof(float));
  w.prior_sg = o; o += up256(Kp * L * sizeof(float));
  w.base_c = o; o += up256((uint64_t)d.B * (uint64_t)base_K * sizeof(double));
  w.st_d = o; o += up256(n * 4 * sizeof(double));
  w.fin = o; o += up256((uint64_t)d.B * 4 * sizeof(double));
  w.st_z = o; o += up256(n * L * sizeof(float));
  w.st_gA = o; o += up256(n * L * sizeof(float));
  w.st_gB = o; o += up256(n * L * sizeof(float));
  w.st_eps = o; o += up256(n * sizeof(float));
  w.st_acc = o; o += up256(n * sizeof(int));
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

int gmvae_ais_workspace_bytes(const GmvaeDims* dims, int model, int base_K, int n_chains, uint64_t* bytes) {
  if (int e = ais_check(dims, model, base_K, 1, n_chains, 1)) return e;
  if (!bytes) return GMVAE_E_NULL;
  *bytes = ais_ws(*dims, model, base_K, n_chains).total;
  return 0;
}

int gmvae_ais(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, const float* base, int base_K,
              const float* betas_dev, int n_temps, int n_chains, int n_leapfrog, float step0, float step_up, float step_down,
              const float* eps, const float* u, float* logw_out, float* bound_out, float* stats_out, float* z_out, float* tail,
              void* workspace, uint64_t seed, uint64_t step, void* stream) {
  if (int e = ais_check(dims, model, base_K, n_temps, n_chains, n_leapfrog)) return e;
  if (!(step0 > 0.f) || !(step_up > 0.f) || !(step_down > 0.f) || !(step0 < INFINITY) || !(step_up < INFINITY) ||
      !(step_down < INFINITY))
    return GMVAE_E_DIMS;
  if ((base != nullptr) != (base_K > 0)) return base ? GMVAE_E_DIMS : GMVAE_E_NULL;
  if (!x || !params || !betas_dev || !tail || !workspace) return GMVAE_E_NULL;
  if (!aligned_to(params, 16) || !aligned_to(base, 4) || !aligned_to(betas_dev, 4) || !aligned_to(eps, 4) || !aligned_to(u, 4) ||
      !aligned_to(logw_out, 4) || !aligned_to(bound_out, 4) || !aligned_to(stats_out, 4) || !aligned_to(z_out, 4) ||
      !aligned_to(tail, 4) || !aligned_to(workspace, 256) || !aligned_to(dims->gen_bias_vec, 4))
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

  const AisWs w = ais_ws(d, model, base_K, n_chains);
  char* const ws = static_cast<char*>(workspace);
  AisArgs a;
  memset(&a, 0, sizeof(a));
  a.D = d.D; a.L = d.L; a.n_hidden = d.n_hidden; a.act = d.hidden_act;
  for (int i = 0; i < d.n_hidden; ++i) a.hidden[i] = d.hidden[i];
  a.C = n_chains;
  a.n = (long long)d.B * n_chains;
  a.enc = base_K > 0;
  a.Kp = model == GMVAE_MODEL_VAE ? 1 : d.K;
  a.Kb = base_K;
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
  p.model = model; p.L = d.L; p.Kp = a.Kp; p.Kb = base_K;
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
  p.base = base;
  p.base_c = reinterpret_cast<double*>(ws + w.base_c);

  a.gen_bias = d.gen_bias_init;
  a.gen_bias_vec = static_cast<const float*>(d.gen_bias_vec);
  a.x = x;
  a.prior_lw = p.lw; a.prior_c = p.cst; a.prior_mu = p.mu; a.prior_sg = p.sg;
  a.base = base; a.base_c = p.base_c;
  a.betas = betas_dev;
  a.T = n_temps; a.n_leap = n_leapfrog;
  a.step0 = fminf(fmaxf(step0, kAisStepMin), kAisStepMax); a.step_up = step_up; a.step_down = step_down;
  a.eps = eps; a.u = u;
  a.row_base = d.row0 * (uint64_t)n_chains; a.seed = seed; a.step = step;
  a.st_z = reinterpret_cast<float*>(ws + w.st_z);
  a.st_gA = reinterpret_cast<float*>(ws + w.st_gA);
  a.st_gB = reinterpret_cast<float*>(ws + w.st_gB);
  a.st_d = reinterpret_cast<double*>(ws + w.st_d);
  a.st_eps = reinterpret_cast<float*>(ws + w.st_eps);
  a.st_acc = reinterpret_cast<int*>(ws + w.st_acc);
  a.st_bits = reinterpret_cast<unsigned long long*>(ws + w.st_bits);
  a.z_out = z_out;

  // transitions per launch: no single launch runs long on a shared card (GMVAE_AIS_LAUNCH_TEMPS: the tests' cut; the result
  // does not depend on it)
  int cap = kAisLaunchTemps;
  if (const char* s = getenv("GMVAE_AIS_LAUNCH_TEMPS")) {
    const int v = atoi(s);
    if (v >= 1) cap = v;
  }
  const unsigned lds = ais_lds(d.L, d.n_hidden, a.hidden).total;
  hipStream_t st = static_cast<hipStream_t>(stream);
  (void)hipGetLastError();
  if (lds > 64u * 1024u) {
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ais_run), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)kAisLdsLimit))
      return (int)e;
  }
  hipLaunchKernelGGL(ais_prep, dim3(1u + (a.enc ? (unsigned)d.B : 0u)), dim3(kAisThreads), 0, st, p);
  const unsigned panels = (unsigned)((a.n + kAisRows - 1) / kAisRows);
  // the start (t = 0) rides on the first launch: transitions 0 .. cap, then cap more per launch
  for (int t_lo = 0; t_lo <= n_temps;) {
    const int t_hi = (int)(((long long)t_lo + cap < n_temps) ? t_lo + cap : n_temps);
    a.t_lo = t_lo; a.t_hi = t_hi;
    hipLaunchKernelGGL(ais_run, dim3(panels), dim3(kAisThreads), lds, st, a);
    t_lo = t_hi + 1;
  }
  double* const fin = reinterpret_cast<double*>(ws + w.fin);
  hipLaunchKernelGGL(ais_finish, dim3((unsigned)((d.B + kAisThreads - 1) / kAisThreads)), dim3(kAisThreads), 0, st, a.st_d, a.st_eps,
                     a.st_acc, d.B, n_chains, n_temps, logw_out, bound_out, stats_out, fin);
  hipLaunchKernelGGL(ais_tail, dim3(1), dim3(kAisThreads), 0, st, fin, d.B, tail);
  return (int)hipGetLastError();
}

}  // extern "C"
