// gmvae_ais, gmvae_refine, gmvae_simulate and gmvae_ais_reverse: the host side of csrc/ais.hpp, csrc/refine.hpp and csrc/bdmc.hpp
// (include/gmvae_hip.h).  ONE translation unit for these entry points, because the kernels of ais.hpp are plain definitions: a library defines them once, so whatever evaluates
// with ais_eval is hosted here.  A unit -- and so a device code object -- apart from the training step's, for the reason
// csrc/tsne.hip gives: the training step's code object, and with it the placement of the one-launch step's code, is what it was
// without these kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gmvae_hip.h"
#include "ais.hpp"
#include "bdmc.hpp"
#include "hostutil.hpp"
#include "refine.hpp"

using namespace gmvae;

namespace {

constexpr int kAisLaunchTemps = 32;          // transitions per launch unless GMVAE_AIS_LAUNCH_TEMPS says otherwise
constexpr int kRefineLaunchSteps = 256;      // steps (or rounds) per launch unless GMVAE_REFINE_LAUNCH_STEPS says otherwise

// ---- the size gates: what an entry point refuses before it needs a pointer, in this order -- check_model (the sizes csrc/ais.hpp
// takes, the plain Bernoulli on {0, 1}), its own counts, check_rows (per_example >= 1 chains or samples per example)
int check_model(const GmvaeDims* d, int model) {
  if (!d) return GMVAE_E_NULL;
  if (model < 0 || model > 2) return GMVAE_E_MODEL;
  if (d->B < 1 || d->D < 1 || d->L < 1 || d->L > kAisMaxL) return GMVAE_E_DIMS;
  if (model != GMVAE_MODEL_VAE && (d->K < 1 || d->K > kAisMaxK)) return GMVAE_E_DIMS;
  if (d->n_hidden < 0 || d->n_hidden > kAisMaxHidden) return GMVAE_E_DIMS;
  for (int i = 0; i < d->n_hidden; ++i)
    if (d->hidden[i] < 1 || d->hidden[i] > kAisMaxWidth) return GMVAE_E_DIMS;
  if (d->hidden_act < GMVAE_ACT_RELU || d->hidden_act > GMVAE_ACT_ELU) return GMVAE_E_DIMS;
  if (d->gen_bias_vec ? d->gen_bias_len != d->D : d->gen_bias_len != 0) return GMVAE_E_DIMS;
  if (d->sched_flags & (GMVAE_LIK_MASK | GMVAE_OBJ_PIXEL_MASK | GMVAE_X_F32 | GMVAE_LIK_SCALE_LEARNED | GMVAE_LIK_POISSON | GMVAE_LIK_NEG_BINOMIAL)) return GMVAE_E_DIMS;
  return 0;
}
int check_rows(const GmvaeDims* d, int per_example) {
  const uint64_t end = d->row0 + (uint64_t)d->B;
  if (end < d->row0 || end > ((1ull << 38) - 1) / (uint64_t)per_example) return GMVAE_E_DIMS;      // ((row0 + B) C < 2^38: Philox's row field)
  if ((uint64_t)d->B * (uint64_t)per_example > (1ull << 30)) return GMVAE_E_DIMS;
  if (ais_lds(d->L, d->n_hidden, d->hidden).total > kAisLdsLimit) return GMVAE_E_DIMS;
  return 0;
}
int ais_check(const GmvaeDims* d, int model, int base_K, int n_temps, int n_chains, int n_leapfrog) {
  if (int e = check_model(d, model)) return e;
  if (base_K < 0 || base_K > kAisMaxK) return GMVAE_E_DIMS;
  if (n_temps < 1 || n_temps > (1 << 24) || n_chains < 1 || n_leapfrog < 1) return GMVAE_E_DIMS;
  return check_rows(d, n_chains);
}
int refine_check(const GmvaeDims* d, int model, int n_steps, int n_samples, int n_eval_rounds) {
  if (int e = check_model(d, model)) return e;
  if (n_samples != 1 && n_samples != 2 && n_samples != 4 && n_samples != 8 && n_samples != 16) return GMVAE_E_DIMS;
  if (n_steps < 0 || n_eval_rounds < 1 || (long long)n_steps + n_eval_rounds > (1 << 24)) return GMVAE_E_DIMS;
  return check_rows(d, n_samples);
}

// ---- the workspaces
template <class T>
T* at(char* ws, uint64_t offset) { return reinterpret_cast<T*>(ws + offset); }
int prior_K(const GmvaeDims& d, int model) { return model == GMVAE_MODEL_VAE ? 1 : d.K; }

// the prior table ais_prep builds: constants [Kp] (fp64), ln pi [Kp], mu [Kp][L], sigma [Kp][L]
struct PriorWs {
  uint64_t c, lw, mu, sg;
};
PriorWs carve_prior(uint64_t& o, uint64_t Kp, uint64_t L) {
  PriorWs w;
  w.c = o; o += up256(Kp * sizeof(double));
  w.lw = o; o += up256(Kp * sizeof(float));
  w.mu = o; o += up256(Kp * L * sizeof(float));
  w.sg = o; o += up256(Kp * L * sizeof(float));
  return w;
}

// gmvae_ais: the accept records, the prior table, the base's constants, the chains' state, the per-example sums.  O(B C L),
// independent of T.
struct AisWs {
  PriorWs prior;
  uint64_t st_bits, base_c, st_d, fin, st_z, st_gA, st_gB, st_eps, st_acc, total;
};
AisWs ais_ws(const GmvaeDims& d, int model, int base_K, int n_chains) {
  AisWs w;
  const uint64_t L = (uint64_t)d.L, n = (uint64_t)d.B * (uint64_t)n_chains;
  uint64_t o = 0;
  w.st_bits = o; o += up256(n * sizeof(uint64_t));      // (first: include/gmvae_hip.h documents it)
  w.prior = carve_prior(o, (uint64_t)prior_K(d, model), L);
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

// gmvae_refine: the prior table, the rows' running sums, the per-example bounds, the examples' state.  O(B (L + S)), independent
// of n_steps and n_eval_rounds.
struct RefineWs {
  PriorWs prior;
  uint64_t acc, fin, phi, cnt, total;
};
RefineWs refine_ws(const GmvaeDims& d, int model, int n_samples) {
  RefineWs w;
  const uint64_t L = (uint64_t)d.L, B = (uint64_t)d.B;
  uint64_t o = 0;
  w.prior = carve_prior(o, (uint64_t)prior_K(d, model), L);
  w.acc = o; o += up256(B * (uint64_t)n_samples * 8 * sizeof(double));
  w.fin = o; o += up256(B * 4 * sizeof(double));
  w.phi = o; o += up256(B * 6 * L * sizeof(float));
  w.cnt = o; o += up256(B * sizeof(int));
  w.total = o;
  return w;
}

// ---- the model into the evaluation's and ais_prep's arguments (both zeroed first): the sizes, the decoder and the prior's
// parameters by name (gmvae_param_layout: the reference's variable names), the bias, x, the prior table in the workspace.  What
// is the entry point's own -- rows, base, schedule, noise, state -- the caller fills in afterwards.
const float* find_param(const float* params, const GmvaeParamEntry* e, int n, const char* name) {
  for (int i = 0; i < n; ++i)
    if (!strcmp(e[i].name, name)) return params + e[i].offset;
  return nullptr;
}
int bind_model(const GmvaeDims& d, int model, const float* params, const uint8_t* x, char* ws, const PriorWs& w, AisArgs& a,
               AisPrep& p) {
  GmvaeDims dl = d;
  dl.S = 1;
  dl.sched_flags = 0;
  int n_ent = 0;
  if (int e = gmvae_param_layout(&dl, model, nullptr, 0, &n_ent)) return e;
  GmvaeParamEntry* ent = static_cast<GmvaeParamEntry*>(malloc(sizeof(GmvaeParamEntry) * (size_t)n_ent));
  if (!ent) return GMVAE_E_SMALL;
  if (int e = gmvae_param_layout(&dl, model, ent, n_ent, &n_ent)) { free(ent); return e; }

  memset(&a, 0, sizeof(a));
  a.D = d.D; a.L = d.L; a.n_hidden = d.n_hidden; a.act = d.hidden_act;
  for (int i = 0; i < d.n_hidden; ++i) a.hidden[i] = d.hidden[i];
  a.Kp = prior_K(d, model);
  bool found = true;
  char name[64];
  for (int i = 0; i <= d.n_hidden; ++i) {
    snprintf(name, sizeof(name), "decoder_fcnet/linear_%d/w", i);
    a.w[i] = find_param(params, ent, n_ent, name);
    snprintf(name, sizeof(name), "decoder_fcnet/linear_%d/b", i);
    a.b[i] = find_param(params, ent, n_ent, name);
    found = found && a.w[i] && a.b[i];
  }
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
  p.cst = at<double>(ws, w.c); p.lw = at<float>(ws, w.lw); p.mu = at<float>(ws, w.mu); p.sg = at<float>(ws, w.sg);
  a.gen_bias = d.gen_bias_init;
  a.gen_bias_vec = static_cast<const float*>(d.gen_bias_vec);
  a.x = x;
  a.prior_lw = p.lw; a.prior_c = p.cst; a.prior_mu = p.mu; a.prior_sg = p.sg;
  return 0;
}

// ---- the launches
// transitions, steps or rounds per launch: no single launch runs long on a shared card (the variable is the tests' cut; the
// result does not depend on it)
int launch_cap(const char* env_name, int cap) {
  if (const char* s = getenv(env_name)) {
    const int v = atoi(s);
    if (v >= 1) cap = v;
  }
  return cap;
}

// clears the sticky error, then lets `kernel` take more than 64 KB of dynamic LDS where the sizes ask for it
template <class Kernel>
int raise_lds(Kernel kernel, unsigned lds) {
  (void)hipGetLastError();
  if (lds <= 64u * 1024u) return 0;
  return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAisLdsLimit);
}

// the common tail: one thread per example runs `finish(args..., fin)`, then ais_tail folds fin [B][4] into `tail`
template <class Kernel, class... Args>
int finish_and_tail(hipStream_t st, int B, double* fin, float* tail, Kernel finish, Args... args) {
  hipLaunchKernelGGL(finish, dim3((unsigned)((B + kAisThreads - 1) / kAisThreads)), dim3(kAisThreads), 0, st, args..., fin);
  hipLaunchKernelGGL(ais_tail, dim3(1), dim3(kAisThreads), 0, st, fin, B, tail);
  return (int)hipGetLastError();
}

// ---- gmvae_ais and gmvae_ais_reverse: one host path.  reverse: the chains start at z_start [B][L] and run T .. 1 (csrc/bdmc.hpp).
int run_chains(bool reverse, const GmvaeDims* dims, int model, const uint8_t* x, const float* params, const float* base, int base_K,
               const float* z_start, const float* betas_dev, int n_temps, int n_chains, int n_leapfrog, float step0, float step_up,
               float step_down, const float* eps, const float* u, float* logw_out, float* bound_out, float* stats_out, float* z_out,
               float* tail, void* workspace, uint64_t seed, uint64_t step, void* stream) {
  if (int e = ais_check(dims, model, base_K, n_temps, n_chains, n_leapfrog)) return e;
  if (!(step0 > 0.f) || !(step_up > 0.f) || !(step_down > 0.f) || !(step0 < INFINITY) || !(step_up < INFINITY) ||
      !(step_down < INFINITY))
    return GMVAE_E_DIMS;
  if ((base != nullptr) != (base_K > 0)) return base ? GMVAE_E_DIMS : GMVAE_E_NULL;
  if (!x || !params || !betas_dev || !tail || !workspace || (reverse && !z_start)) return GMVAE_E_NULL;
  if (!aligned_to(params, 16) || !aligned_to(base, 4) || !aligned_to(betas_dev, 4) || !aligned_to(eps, 4) || !aligned_to(u, 4) ||
      !aligned_to(logw_out, 4) || !aligned_to(bound_out, 4) || !aligned_to(stats_out, 4) || !aligned_to(z_out, 4) ||
      !aligned_to(tail, 4) || !aligned_to(workspace, 256) || !aligned_to(dims->gen_bias_vec, 4) || !aligned_to(z_start, 4))
    return GMVAE_E_ALIGN;
  const GmvaeDims& d = *dims;
  const AisWs w = ais_ws(d, model, base_K, n_chains);
  char* const ws = static_cast<char*>(workspace);
  RevArgs ra;
  AisArgs& a = ra.a;
  AisPrep p;
  if (int e = bind_model(d, model, params, x, ws, w.prior, a, p)) return e;
  ra.z_start = z_start;
  p.Kb = base_K; p.base = base; p.base_c = at<double>(ws, w.base_c);
  a.C = n_chains;
  a.n = (long long)d.B * n_chains;
  a.enc = base_K > 0;
  a.Kb = base_K; a.base = base; a.base_c = p.base_c;
  a.betas = betas_dev;
  a.T = n_temps; a.n_leap = n_leapfrog;
  a.step0 = fminf(fmaxf(step0, kAisStepMin), kAisStepMax); a.step_up = step_up; a.step_down = step_down;
  a.eps = eps; a.u = u;
  a.row_base = d.row0 * (uint64_t)n_chains; a.seed = seed; a.step = step;
  a.st_z = at<float>(ws, w.st_z); a.st_gA = at<float>(ws, w.st_gA); a.st_gB = at<float>(ws, w.st_gB);
  a.st_d = at<double>(ws, w.st_d); a.st_eps = at<float>(ws, w.st_eps); a.st_acc = at<int>(ws, w.st_acc);
  a.st_bits = at<unsigned long long>(ws, w.st_bits);
  a.z_out = z_out;

  const int cap = launch_cap("GMVAE_AIS_LAUNCH_TEMPS", kAisLaunchTemps);
  const unsigned lds = ais_lds(d.L, d.n_hidden, a.hidden).total;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int e = reverse ? raise_lds(bdmc_rev_run, lds) : raise_lds(ais_run, lds)) return e;
  hipLaunchKernelGGL(ais_prep, dim3(1u + (a.enc ? (unsigned)d.B : 0u)), dim3(kAisThreads), 0, st, p);
  const unsigned panels = (unsigned)((a.n + kAisRows - 1) / kAisRows);
  if (!reverse) {
    // the start (t = 0) rides on the first launch: transitions 0 .. cap, then cap more per launch
    for (int t_lo = 0; t_lo <= n_temps;) {
      const int t_hi = (int)(((long long)t_lo + cap < n_temps) ? t_lo + cap : n_temps);
      a.t_lo = t_lo; a.t_hi = t_hi;
      hipLaunchKernelGGL(ais_run, dim3(panels), dim3(kAisThreads), lds, st, a);
      t_lo = t_hi + 1;
    }
  } else {
    // descending, the mirror image: the start (t = T + 1) and transitions T .. T + 1 - cap, then cap more per launch down to 1
    for (int t_hi = n_temps + 1; t_hi >= 1;) {
      const int t_lo = t_hi - cap > 1 ? t_hi - cap : 1;
      a.t_lo = t_lo; a.t_hi = t_hi;
      hipLaunchKernelGGL(bdmc_rev_run, dim3(panels), dim3(kAisThreads), lds, st, ra);
      t_hi = t_lo - 1;
    }
  }
  return finish_and_tail(st, d.B, at<double>(ws, w.fin), tail, ais_finish, a.st_d, a.st_eps, a.st_acc, d.B, n_chains, n_temps,
                         reverse ? -1.0 : 1.0, logw_out, bound_out, stats_out);
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
  return run_chains(false, dims, model, x, params, base, base_K, nullptr, betas_dev, n_temps, n_chains, n_leapfrog, step0, step_up,
                    step_down, eps, u, logw_out, bound_out, stats_out, z_out, tail, workspace, seed, step, stream);
}

int gmvae_ais_reverse_workspace_bytes(const GmvaeDims* dims, int model, int base_K, int n_chains, uint64_t* bytes) {
  return gmvae_ais_workspace_bytes(dims, model, base_K, n_chains, bytes);      // (the chains' state is the forward chains')
}

int gmvae_ais_reverse(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, const float* base, int base_K,
                      const float* z_start, const float* betas_dev, int n_temps, int n_chains, int n_leapfrog, float step0,
                      float step_up, float step_down, const float* eps, const float* u, float* logw_out, float* bound_out,
                      float* stats_out, float* z_out, float* tail, void* workspace, uint64_t seed, uint64_t step, void* stream) {
  return run_chains(true, dims, model, x, params, base, base_K, z_start, betas_dev, n_temps, n_chains, n_leapfrog, step0, step_up,
                    step_down, eps, u, logw_out, bound_out, stats_out, z_out, tail, workspace, seed, step, stream);
}

int gmvae_simulate_workspace_bytes(const GmvaeDims* dims, int model, uint64_t* bytes) {
  if (int e = ais_check(dims, model, 0, 1, 1, 1)) return e;
  if (!bytes) return GMVAE_E_NULL;
  uint64_t o = 0;
  (void)carve_prior(o, (uint64_t)prior_K(*dims, model), (uint64_t)dims->L);
  *bytes = o;
  return 0;
}

int gmvae_simulate(const GmvaeDims* dims, int model, const float* params, const float* eps, const float* u, const float* ux,
                   float* z_out, int32_t* k_out, uint8_t* x_out, float* prob_out, void* workspace, uint64_t seed, uint64_t step,
                   void* stream) {
  if (int e = ais_check(dims, model, 0, 1, 1, 1)) return e;
  if (!params || !z_out || !k_out || !x_out || !workspace) return GMVAE_E_NULL;
  if (!aligned_to(params, 16) || !aligned_to(eps, 4) || !aligned_to(u, 4) || !aligned_to(ux, 4) || !aligned_to(z_out, 4) ||
      !aligned_to(k_out, 4) || !aligned_to(x_out, 4) || !aligned_to(prob_out, 4) || !aligned_to(workspace, 256) ||
      !aligned_to(dims->gen_bias_vec, 4))
    return GMVAE_E_ALIGN;
  const GmvaeDims& d = *dims;
  uint64_t o = 0;
  const PriorWs w = carve_prior(o, (uint64_t)prior_K(d, model), (uint64_t)d.L);
  SimArgs sa;
  memset(&sa, 0, sizeof(sa));
  AisArgs& a = sa.a;
  AisPrep p;
  if (int e = bind_model(d, model, params, nullptr, static_cast<char*>(workspace), w, a, p)) return e;
  a.C = 1;
  a.n = d.B;
  a.T = 1;                                        // (ais_noise keys the draw of t by step (T + 1) + t: 2 step, and 2 step + 1 the pixels)
  a.eps = eps; a.u = u;
  a.row_base = d.row0; a.seed = seed; a.step = step;
  sa.ux = ux;
  sa.z_out = z_out; sa.k_out = k_out; sa.x_out = x_out; sa.prob_out = prob_out;
  const unsigned lds = ais_lds(d.L, d.n_hidden, a.hidden).total;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int e = raise_lds(sim_rows, lds)) return e;
  hipLaunchKernelGGL(ais_prep, dim3(1), dim3(kAisThreads), 0, st, p);
  hipLaunchKernelGGL(sim_rows, dim3((unsigned)((d.B + kAisRows - 1) / kAisRows)), dim3(kAisThreads), lds, st, sa);
  return (int)hipGetLastError();
}

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
  const RefineWs w = refine_ws(d, model, n_samples);
  char* const ws = static_cast<char*>(workspace);
  RefineArgs ra;
  memset(&ra, 0, sizeof(ra));
  AisArgs& a = ra.a;
  AisPrep p;
  if (int e = bind_model(d, model, params, x, ws, w.prior, a, p)) return e;

  a.C = n_samples;
  a.n = (long long)d.B * n_samples;
  a.enc = 0;                                      // A = log p(z), B = log p(x|z)
  const int total = n_steps + n_eval_rounds;      // the timeline: the steps, then the rounds
  a.T = total;                                    // (ais_noise keys the draw of t by step (T + 1) + t)
  a.eps = eps;
  a.row_base = d.row0 * (uint64_t)n_samples; a.seed = seed; a.step = step;
  ra.B = d.B; ra.S = n_samples; ra.n_steps = n_steps;
  ra.lr = lr; ra.b1 = beta1; ra.b2 = beta2; ra.aeps = adam_eps;
  ra.start = start;
  ra.phi = at<float>(ws, w.phi); ra.cnt = at<int>(ws, w.cnt); ra.acc = at<double>(ws, w.acc);
  ra.trace = trace_out;

  const int cap = launch_cap("GMVAE_REFINE_LAUNCH_STEPS", kRefineLaunchSteps);
  const unsigned lds = ais_lds(d.L, d.n_hidden, a.hidden).total;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int e = raise_lds(refine_run, lds)) return e;
  hipLaunchKernelGGL(ais_prep, dim3(1), dim3(kAisThreads), 0, st, p);
  const unsigned panels = (unsigned)((a.n + kAisRows - 1) / kAisRows);
  for (int t_lo = 0; t_lo < total;) {
    const int t_hi = (int)(((long long)t_lo + cap < total) ? t_lo + cap : total) - 1;
    ra.t_lo = t_lo; ra.t_hi = t_hi;
    hipLaunchKernelGGL(refine_run, dim3(panels), dim3(kAisThreads), lds, st, ra);
    t_lo = t_hi + 1;
  }
  return finish_and_tail(st, d.B, at<double>(ws, w.fin), tail, refine_finish, ra.phi, start, ra.cnt, ra.acc, d.B, d.L, n_samples,
                         n_eval_rounds, phi_out, stats_out);
}

}  // extern "C"
