/*
 * gmvae_hip.h -- C ABI of libgmvae_hip.so: the MI355X (gfx950) implementation
 * of the one hot path of mazrk7/gmvae: the VAE / VAE_GMP / GMVAE single-sample
 * ELBO training step (+ the IWAE n_samples extension).
 *
 * The reference has NO FFI/plugin API (it is pure TF1 graph Python); the
 * boundary it exposes is the Python object protocol of scripts/vae.py and
 * scripts/gmvae.py.  gmvae_amd/{base,vae,gmvae}.py mirror that protocol and
 * bind the entry points below with ctypes.  Each entry point cites the
 * reference call site(s) whose arithmetic it replaces (paths relative to the
 * upstream repo).
 *
 * Conventions
 *   - every function returns 0 on success, a positive hipError_t on a HIP
 *     failure, or a negative GMVAE_E_* code on a bad argument; nothing throws;
 *   - no allocation and no synchronisation inside: the caller owns every
 *     buffer (device memory, 16-byte aligned) including the workspace, whose
 *     size is queried with gmvae_workspace_bytes() and which must be zeroed
 *     ONCE after allocation and then used with ONE set of dims (padding words
 *     are never written again; it also holds the epoch counter and the error
 *     word of the in-launch hand-offs of the fused schedule: a hand-off that
 *     times out -- the schedule needs the whole device to itself -- poisons
 *     that step's loss and gradients with NaN and sets the error word, after
 *     which waits no longer block; re-zero the workspace to clear it);
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*), is
 *     asynchronous and graph-capturable; no global state;
 *   - all float tensors are fp32 row-major; x is uint8/bool {0,1} [B,D] (uint8 grey levels 0..255 under GMVAE_LIK_*; float [B,D] under GMVAE_X_F32);
 *   - sample-dependent tensors have R = B*S rows, row r = b*S + s.
 */
#ifndef GMVAE_HIP_H_
#define GMVAE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMVAE_MAX_HIDDEN 8
#define GMVAE_TAIL 8          /* floats appended to the gradient buffer */
#define GMVAE_ABI_VERSION 7   /* 5: + gmvae_dp_profile, gmvae_forward_profile; 6: GmvaeDims.hidden_act appended; 7: + gmvae_comm_count, GMVAE_E_TIMEOUT */

enum { GMVAE_MODEL_VAE = 0, GMVAE_MODEL_VAE_GMP = 1, GMVAE_MODEL_GMVAE = 2 };

enum {
  GMVAE_E_NULL = -1,      /* required pointer is NULL            */
  GMVAE_E_DIMS = -2,      /* non-positive / unsupported sizes    */
  GMVAE_E_MODEL = -3,     /* unknown model id                    */
  GMVAE_E_ALIGN = -4,     /* pointer not 16-byte aligned         */
  GMVAE_E_NET = -5,       /* unknown sub-network id              */
  GMVAE_E_SMALL = -6,     /* caller array too small              */
  GMVAE_E_TIMEOUT = -7    /* gmvae_comm_init: a rank did not join within GMVAE_COMM_INIT_TIMEOUT seconds */
};

/* Sizes + the hyper-parameters scripts/runners.py:78-101 binds
 * (sigma_min=0, raw_sigma_bias=0.5, temperature=1; gen_bias_init=0 from
 * scripts/gmvae.py:285).  hidden[] = fcnet_hidden_sizes. */
typedef struct GmvaeDims {
  int32_t B;                          /* rows of x on this device            */
  int32_t D;                          /* data_size                           */
  int32_t L;                          /* latent_size                         */
  int32_t K;                          /* mixture_components (1 for plain VAE)*/
  int32_t S;                          /* IWAE samples; 1 == the reference    */
  int32_t n_hidden;
  int32_t hidden[GMVAE_MAX_HIDDEN];
  float sigma_min;
  float raw_sigma_bias;
  float temperature;
  float gen_bias_init;
  /* Data parallel (no reference counterpart; scripts/runners.py:193 pins one device): global index of this
   * device's first batch row, rank * B for equal shards, 0 on a single device.  It enters ONLY the Philox counters
   * of the in-kernel noise (eps, u) and of gmvae_binarize: row b of this device draws what row row0 + b of the
   * single-device step on the whole global batch draws, so G shards reproduce the 1-device step on G*B rows.
   * Sizes, layouts and the workspace do not depend on it.  The Philox counter holds 38 bits of the row: gmvae_step,
   * gmvae_forward, the graphs and gmvae_workspace_bytes return GMVAE_E_DIMS if (row0 + B)*S >= 2^38 ((row0 + B)*S*K with y
   * summed out); the evaluators bound their own rows (below). */
  uint64_t row0;
  /* ABI v3 -- vector bias_init of ConditionalBernoulli (scripts/base.py:102-103 "a scalar or vector Tensor that is added
   * to the output of the fully connected network", e.g. the logit of the training-set mean; added at base.py:135):
   * device pointer to gen_bias_len == D fp32 values, or NULL / 0 for the scalar form alone.  The decoder logits are
   * MLP(z) + gen_bias_init + gen_bias_vec[j].  It is a constant of the model (no gradient), read by the decoder
   * output layer's epilogue; steps with a vector run the schedules whose decoder layer is a grouped-GEMM launch. */
  const float* gen_bias_vec;
  int32_t gen_bias_len;
  /* ABI v4 -- schedule and objective flags (the v3 `reserved_` word; 0 = the default schedules).  GMVAE_SCHED_SAFE: only schedules in which
   * no workgroup waits for another workgroup of its own launch (one workgroup per 16-row panel, the first layer as a launch
   * of its own): slower (4 launches per step instead of 2), never stalling when something else holds part of the device.  A
   * caller sets it after a hand-off timeout (the workspace's error word) -- per call, not per process.  It changes neither
   * sizes, layouts nor the workspace. */
  int32_t sched_flags;
  /* ABI v6 -- hidden_activation_fn of every conditional's MLP (scripts/base.py:19,90,153 take any callable; gmvae.py:282 and
   * vae.py:196 pass ONE to all networks; default tf.nn.relu): GMVAE_ACT_*.  Steps with an activation other than ReLU run the
   * general schedule (one grouped-GEMM launch per dependency level: the activation in the forward epilogue, its derivative --
   * a function of the kept activation -- in the data-gradient epilogue). */
  int32_t hidden_act;
} GmvaeDims;
enum { GMVAE_SCHED_SAFE = 1,
       /* forward-only calls (gmvae_forward): the operand images a previous gmvae_forward left in THIS workspace were built from
        * the parameters as they still are (an evaluation walks a split batch by batch on fixed parameters): evalf_prep is skipped.
        * The caller vouches for it; gmvae_amd.Engine tracks every writer of its parameter buffer. */
       GMVAE_SCHED_EVAL_IMAGES_VALID = 2,
       /* objective (GMVAE only, S == 1): y summed out exactly over its K values instead of one Gumbel-softmax draw --
        *   L_b = sum_k q(k|x_b) [ -log p(x_b|z_bk) + log q(z_bk|x_b,k) - log p(z_bk|k) ] + sum_k q_bk ln q_bk,
        *   z_bk = mu_q(x_b, e_k) + sigma_q(x_b, e_k) eps_bk.
        * UNLIKE the schedule bits it changes sizes and the workspace: the sample-dependent tensors have R = B*K rows, row
        * r = b*K + k with y_r = e_k; eps is [B*K, L] (NULL: Philox row (row0 + b)*K + k, gmvae_noise_fill's keying at
        * row_base = row0*K), u is not used.  Tail: [0] sum_b L_b, [1] sum_b sum_k q_bk nll_bk, [2] the same of kl_bk, [3] sum_b
        * nent_b, [4] B.  gmvae_forward: row_terms [B*K,4] = logpx, logq, logp, log w' = logpx + logp - logq (no nent term);
        * z_out [B*K,L]; y_out [B*K,K] the one-hot rows; logits_out [B,K].  Takes the general schedule (gmvae_step_schedule:
        * "general+marginal"); every entry point that runs a step honours it; gmvae_iw_bound refuses it (GMVAE_E_DIMS; the
        * bound with y summed out is gmvae_iw_bound_enum_y, which ignores the bit).
        * GMVAE_E_MODEL for the VAE family; GMVAE_E_DIMS if S != 1 or B*K > 2^30. */
       GMVAE_OBJ_MARGINAL_Y = 4,
       /* objective (GMVAE only, any S >= 1): y summed out exactly over its K values as under GMVAE_OBJ_MARGINAL_Y, z
        * importance-weighted over S samples per component --
        *   log w'_bsk = log p(x_b|z_bsk) + log p(z_bsk|e_k) - log q(z_bsk|x_b,e_k),
        *   l_bk = -( logsumexp_s log w'_bsk - ln S ),   L_b = sum_k q_bk l_bk + sum_k q_bk ln q_bk,
        *   z_bsk = mu_q(x_b, e_k) + sigma_q(x_b, e_k) eps_bsk.
        * -L_b is a lower bound on log p(x_b) + ln K (for each k the IWAE bound in z; the q-weighted sum over k adds a Gibbs step);
        * mean_logw_b <= -L_b <= bound_b of gmvae_iw_bound_enum_y at n_samples = S on the same noise.  At S == 1 it is
        * GMVAE_OBJ_MARGINAL_Y's objective, step for step the same bits.  The sample-dependent tensors have R = B*S*K rows, row
        * r = (b*S + s)*K + k with y_r = e_k; eps is [B*S*K, L] (NULL: Philox row ((row0 + b)*S + s)*K + k, gmvae_noise_fill's
        * keying at row_base = row0*S*K and gmvae_iw_bound_enum_y's at n_samples = S), u is not used.  The workspace's per-row
        * buffers lie where the Gumbel objective's lie at S*K samples.  Tail: [0] sum_b L_b, [1] sum_b sum_k q_bk mean_s nll_bsk,
        * [2] the same of kl_bsk, [3] sum_b nent_b, [4] B.  gmvae_forward: row_terms [B*S*K,4] = logpx, logq, logp, log w';
        * z_out [B*S*K,L]; y_out [B*S*K,K] the one-hot rows; logits_out [B,K].  Takes the general schedule
        * (gmvae_step_schedule: "general+marginal_iw"); every entry point that runs a step honours it; gmvae_iw_bound refuses it
        * (GMVAE_E_DIMS); gmvae_iw_bound_enum_y ignores it.  GMVAE_E_MODEL for the VAE family; GMVAE_E_DIMS if it is set
        * together with GMVAE_OBJ_MARGINAL_Y, B*S*K > 2^30 or (row0 + B)*S*K >= 2^38. */
       GMVAE_OBJ_MARGINAL_Y_IW = 8,
       /* gradient estimator of the INFERENCE network (encoder / encoder_gmm) on the importance-weighted bounds: the doubly
        * reparameterised gradient (Tucker et al. 2018, "DReG"; at S == 1 the path-derivative "sticking the landing" estimator
        * of Roeder et al. 2017) instead of the plain reparameterised one.  Unbiased for the same bound; the bound, the tail and
        * every generative gradient (decoder, prior network, mixture prior, encoder_y through the closed-form dlogits) are the
        * standard step's.  With w the row weight of the step (softmax_s(log w) for the VAE family, q_bk softmax_s(log w'_bsk)
        * under GMVAE_OBJ_MARGINAL_Y_IW, q_bk under GMVAE_OBJ_MARGINAL_Y, 1 at S == 1), dz the decoder's data gradient (scaled
        * by w), pterm = d(-log p(z))/dz and v = softmax_s(log w) of the row's own sample group (1 at S == 1), loss = -bound:
        *   standard:  dmu_q = dz + w pterm                       dsig_q = dmu_q eps - w / sig_q
        *   DReG:      dmu_q = v (dz + w pterm - w eps / sig_q)   dsig_q = dmu_q eps
        * -- the score of q through its own parameters is dropped, the path through z keeps d log q / dz = -eps / sig_q (the
        * clamped sig_q where sigma_min is active; draw_q and its sigma_min mask are unchanged).  Total weight on the path:
        * softmax_s^2 for the VAE family, q_bk softmax_s^2 under GMVAE_OBJ_MARGINAL_Y_IW.
        * Covers the VAE and VAE_GMP at any S >= 1 and the GMVAE under GMVAE_OBJ_MARGINAL_Y / GMVAE_OBJ_MARGINAL_Y_IW.  REFUSED
        * (GMVAE_E_DIMS from gmvae_workspace_bytes and every entry point that runs a step, before any launch) for the Gumbel
        * GMVAE: its relaxed y is reparameterised too, its bound carries an analytic entropy term in place of log q(y), and
        * the prior network's backward would have to run twice (w for its weights, w v for the y path).
        * A step with the bit takes the general schedule at every S (gmvae_step_schedule appends "+dreg": "general+dreg",
        * "general+marginal_iw+dreg"); every entry point that runs a step honours it (gmvae_step, the train and pipeline
        * graphs, gmvae_dp_step / gmvae_dp_graph_create, the bench and profile loops); forward-only entries ignore it;
        * gmvae_iw_bound* and gmvae_posterior_* mask it off.  The workspace grows by B*S*K floats under GMVAE_OBJ_MARGINAL_Y_IW
        * at S > 1 (v, behind every other buffer) and is otherwise the same size and layout.  No atomics: eager and captured
        * steps give the same bits. */
       GMVAE_GRAD_DREG = 16,
       /* semi-supervised objective (GMVAE only, together with GMVAE_OBJ_MARGINAL_Y or GMVAE_OBJ_MARGINAL_Y_IW): the component of
        * some examples is OBSERVED and clamps y for them -- the labelled half of Kingma et al.'s M2 objective next to the
        * unlabelled half the marginal objectives already are.  With l_bk the per-component term of the marginal objective
        * (nll_bk + kl_bk at S == 1; -(logsumexp_s log w'_bsk - ln S) under GMVAE_OBJ_MARGINAL_Y_IW), q_b = softmax(logits_b),
        * c_b the observed component of example b (any value outside [0, K) means unlabelled; -1 is conventional) and
        * alpha >= 0 the classification weight:
        *   unlabelled:  L_b = sum_k q_bk l_bk + sum_k q_bk ln q_bk      (the marginal objective, the same bits)
        *   labelled:    L_b = l_bc + alpha (-ln q_bc)                   (no entropy term; the uniform -ln p(y) left out)
        *     row weights  rw_r = [k == c] at S == 1, [k == c] softmax_s(log w'_bsc)_s at S > 1
        *     dlogits_bj = alpha (q_bj - [j == c])
        *     GMVAE_GRAD_DREG's second weight softmax_s(log w'_bsk)_s is unchanged for every k.
        * Tail: [0] sum_b L_b; [1], [2] the weighted nll / kl sums with [k == c] in place of q_bk for a labelled example; [3] sum_b
        * nent_b (a labelled example adds 0); [4] B; [5] sum over the labelled examples of -ln q_bc (NOT multiplied by alpha);
        * [6] the number of labelled examples; [7] the number of labelled examples with argmax_k q_bk == c_b (the argmax of the
        * logits, lowest index on ties).  At S == 1 [0] = [1] + [2] + [3] + alpha [5] up to rounding (at S > 1 [0] is below it, as
        * under GMVAE_OBJ_MARGINAL_Y_IW without the bit: [1] and [2] are means over s); the data-parallel all-reduce sums
        * all eight slots, so [7] / [6] is the classification accuracy on the labelled part of the global batch.
        * The workspace grows BEHIND every other buffer (behind GMVAE_GRAD_DREG's v too) by three regions, each rounded up to
        * 256 bytes as every workspace buffer is:
        *   "labels"      int32 [GMVAE_LABEL_SLOTS][B4], B4 = B rounded up to a multiple of 4 (each slot starts 16-byte aligned)
        *   "sup_weight"  one float, alpha, at the start of its cell
        *   (unnamed)     float [B][3]: the per-example (-ln q_bc, labelled, hit) the step's kernels hand to each other
        * i.e. by r256(4 * GMVAE_LABEL_SLOTS * B4) + 256 + r256(12 * B) bytes; gmvae_workspace_offset answers for the two
        * names.  The CALLER writes "labels" and "sup_weight"; the library only reads them.  A zeroed workspace therefore means
        * "component 0 observed for every example, alpha = 0": a caller always fills both before the first step (gmvae_amd.Engine
        * does: -1 everywhere, its sup_weight).  Without the bit, sizes, layout and the answer for those two names
        * (GMVAE_E_NET) are what they were.
        * Who reads which slot: gmvae_step, gmvae_forward, gmvae_dp_step, the bench and profile loops read slot 0; step i of
        * gmvae_train_graph_create's and gmvae_dp_graph_create's graph reads slot i (n_steps > GMVAE_LABEL_SLOTS: GMVAE_E_DIMS);
        * gmvae_train_graph_create_pipeline refuses the bit (GMVAE_E_DIMS: it gathers its batches by index inside the graph and
        * has no label gather); gmvae_iw_bound* and gmvae_posterior_* mask the bit off.  GMVAE_E_MODEL for the VAE family,
        * GMVAE_E_DIMS for the Gumbel GMVAE -- from gmvae_workspace_bytes and every entry point that runs or sizes a step,
        * before any launch.  gmvae_step_schedule appends "+labels"; the suffixes come in the fixed order
        *   <schedule> [+marginal | +marginal_iw] [+labels] [+dreg] [+planes]
        * ("general+marginal_iw+labels", "general+marginal+labels+dreg").  A step whose labels are all -1 is the step without
        * the bit, bit for bit.  No atomics: eager and captured steps give the same bits. */
       GMVAE_OBJ_LABELS = 32,
       /* weighted objective (all three models, S == 1 only): the KL terms of the bound carry weights that a step READS FROM
        * DEVICE MEMORY -- beta_z >= 0 on the z term (beta-VAE), beta_y >= 0 on the y term and lambda >= 0 nats of free bits
        * on the y term (the minimum-information constraint of Dilokthanakul et al. 2016) -- so that the steps of one captured
        * graph can follow a KL warm-up.  With nll, kl = log q(z|.) - log p(z|.) and nent_b = sum_k q_bk ln q_bk the terms
        * of the objective without the bit, KL(q(y|x_b) || uniform) = nent_b + ln K (the ln K stays out of the loss):
        *   VAE, VAE_GMP:                    L_b = nll_b + beta_z kl_b                        (beta_y and lambda are ignored)
        *   GMVAE, Gumbel y:                 L_b = nll_b + beta_z kl_b + beta_y ne'_b
        *   GMVAE, GMVAE_OBJ_MARGINAL_Y:     L_b = sum_k q_bk (nll_bk + beta_z kl_bk) + beta_y ne'_b
        *   ne'_b = max(nent_b, lambda - ln K),  a_b = [nent_b > lambda - ln K]  (1: the floor is inactive)
        *   lambda == 0 switches the floor off whatever the rounding: a_b = 1, ne'_b = nent_b.
        * Gradients: the y term adds beta_y a_b q_bj (ln q_bj - nent_b) to dlogits (under GMVAE_OBJ_MARGINAL_Y the closed form
        * is dlogits_bj = q_bj (l_bj - sum_k q_bk l_bk) + beta_y a_b q_bj (ln q_bj - nent_b), l_bk = nll_bk + beta_z kl_bk); the
        * decoder path keeps the row weight rw (1, or q_bk); whatever differentiates the KL part -- the prior term and the
        * -1/sigma_q of the z head's backward, the prior network's and the mixture prior's gradients -- takes
        * rwk_r = beta_z rw_r in rw's place.  At weights (1, 1, 0) the objective is the one without the bit (equal at the
        * parity gates, not bit for bit: the fp64 sum forming l_bk is ordered differently).
        * Tail: [0] sum_b L_b (weighted, with the floor); [1], [2], [3] the UNWEIGHTED nll, kl and nent sums of the objective
        * without the bit; [4] B; [5] B beta_z; [6] B beta_y; [7] sum_b (1 - a_b), the examples whose y term sits on its floor
        * (0 for the VAE family).  The data-parallel all-reduce sums all eight slots: [5] / [4] and [6] / [4] give the weights
        * back, [7] / [4] the floor's share.  gmvae_forward: row_terms' log w stays the row's unweighted importance weight.
        * The workspace grows BEHIND every other buffer by regions rounded up to 256 bytes each as every workspace buffer is:
        *   "obj_weights"  float [GMVAE_LABEL_SLOTS][4] = (beta_z, beta_y, lambda, 0 reserved) per slot
        *   "rwk"          float [R], R = B (B K under GMVAE_OBJ_MARGINAL_Y): beta_z rw
        *   "y_floor"      float [B]: a_b
        * and, where the dims have no per-example partials [B][4] yet (S == 1 without GMVAE_OBJ_MARGINAL_Y), those; all three names
        * answer through gmvae_workspace_offset.  The CALLER writes "obj_weights"; the library only reads it.  A zeroed
        * workspace means weights (0, 0, 0): a caller fills the slots before the first step (gmvae_amd.Engine does).
        * Who reads which slot: gmvae_step, gmvae_forward, gmvae_dp_step, the bench and profile loops read slot 0; step i of
        * gmvae_train_graph_create's and gmvae_dp_graph_create's graph reads slot i (n_steps > GMVAE_LABEL_SLOTS: GMVAE_E_DIMS);
        * gmvae_train_graph_create_pipeline refuses the bit (GMVAE_E_DIMS); gmvae_iw_bound* and gmvae_posterior_* mask the bit
        * off; gmvae_forward honours it.  GMVAE_E_DIMS if S != 1 or together with GMVAE_OBJ_MARGINAL_Y_IW, GMVAE_GRAD_DREG or
        * GMVAE_OBJ_LABELS -- from gmvae_workspace_bytes and every entry point that runs or sizes a step, before any launch.
        * Every step with the bit takes the general schedule; gmvae_step_schedule appends "+weights" behind the objective:
        *   <schedule> [+marginal | +marginal_iw] [+labels] [+weights] [+dreg] [+planes]
        * ("general+weights", "general+marginal+weights").  No atomics: eager and captured steps give the same bits. */
       GMVAE_OBJ_WEIGHTS = 64,
       /* Gumbel-softmax temperature from DEVICE MEMORY (GMVAE with the Gumbel draw only, any S >= 1): the step ignores
        * dims->temperature and reads T of y = softmax((logits + g) / T) (scripts/gmvae.py:238-240) from the workspace, so that
        * the steps of one captured graph can anneal it (Jang et al. 2017, Maddison et al. 2017).  The workspace grows BEHIND
        * every other buffer by one region rounded up to 256 bytes:
        *   "y_temperature"  float [GMVAE_LABEL_SLOTS]: one temperature per slot
        * (gmvae_workspace_offset answers for the name).  The CALLER writes it; the library only reads it.  A zeroed workspace
        * means T = 0 (1 / T = inf: NaN everywhere): a caller fills the slots before the first step (gmvae_amd.Engine does).
        * The kernel forms 1.f / T as the host does without the bit: a slot that holds the same float as dims->temperature gives
        * the step without the bit on the general schedule, bit for bit.
        * Who reads which slot: gmvae_step, gmvae_forward, gmvae_dp_step, the bench and profile loops read slot 0; step i of
        * gmvae_train_graph_create's and gmvae_dp_graph_create's graph reads slot i (n_steps > GMVAE_LABEL_SLOTS: GMVAE_E_DIMS);
        * gmvae_train_graph_create_pipeline refuses the bit (GMVAE_E_DIMS); gmvae_forward honours it; gmvae_iw_bound* and
        * gmvae_posterior_* mask it off and draw at dims->temperature.  GMVAE_E_MODEL for the VAE family; GMVAE_E_DIMS together
        * with GMVAE_OBJ_MARGINAL_Y or GMVAE_OBJ_MARGINAL_Y_IW (those objectives draw no y; GMVAE_OBJ_LABELS and GMVAE_GRAD_DREG
        * therefore cannot co-occur) -- from gmvae_workspace_bytes and every entry point that runs or sizes a step, before any
        * launch.  Combines with GMVAE_OBJ_WEIGHTS (S == 1) and with GMVAE_Y_STRAIGHT_THROUGH.  Every step with the bit takes the
        * general schedule; gmvae_step_schedule appends "+temp" behind "+weights":
        *   <schedule> [+marginal | +marginal_iw] [+labels] [+weights] [+temp] [+st] [+dreg] [+planes]
        * ("general+temp", "general+weights+temp+st").  Without the bit, sizes, layout and the answer for the name (GMVAE_E_NET)
        * are what they were.  No atomics: eager and captured steps give the same bits. */
       GMVAE_Y_TEMP_DEV = 128,
       /* straight-through y (same domain and refusals as GMVAE_Y_TEMP_DEV; independent of it: without that bit T is
        * dims->temperature): with a_rk = (logits_bk + g_rk) / T and the relaxed sample y_soft = softmax_k a_rk, the step
        * CONSUMES the one-hot y_hard = e_{argmax_k (logits_bk + g_rk)} (lowest index on ties; the argmax does not depend on T):
        * encoder_gmm's first layer, prior_gmm, their weight gradients, y_out and the workspace's "y" all hold one-hot rows -- what
        * generate_samples, gmvae_iw_bound_enum_y and gmvae_posterior_y feed those networks.  Backward: dy, the data gradient at
        * y_hard, is pulled through the relaxed sample, da = y_soft (dy - sum_k y_soft dy), dlogits_b = sum_s da / T + the entropy
        * term -- autograd of y = y_soft + stopgrad(y_hard - y_soft) (Jang et al. 2017's ST Gumbel-softmax).  The analytic entropy
        * term and the tail are unchanged.  The workspace grows BEHIND every other buffer ("y_temperature" too) by
        *   "y_soft"  float [R][K], R = B S: the relaxed sample, rounded up to 256 bytes
        * present only under this bit (else GMVAE_E_NET).  gmvae_forward honours the bit (y_out one-hot); gmvae_iw_bound and the
        * posteriors mask it off -- for a straight-through model the estimators that match its one-hot y are
        * gmvae_iw_bound_enum_y and gmvae_posterior_y.  The pipeline graph takes it (without GMVAE_Y_TEMP_DEV).  General
        * schedule; gmvae_step_schedule appends "+st" behind "+temp".  No atomics: eager and captured steps give the same bits. */
       GMVAE_Y_STRAIGHT_THROUGH = 256,
       /* per-example observation mask (all three models; the GMVAE with the Gumbel draw only; any S >= 1, any hidden_act, with
        * or without gen_bias_vec, any D >= 1): m_bd in {0, 1}, uint8 with x's layout and stride, OBSERVED iff the byte is
        * non-zero; row r = b S + s belongs to example b.
        *   networks that read x (encoder_y, encoder_gmm, encoder, and their first layers' weight gradients) read
        *     x~_bd = m_bd x_bd                                         (zero imputation)
        *   logpx_r = sum_d m_bd (x_bd lambda_rd - softplus lambda_rd)   (a bound on log p(x_observed))
        *   g_rd    = m_bd (sigmoid(lambda_rd) - x_bd)                   (the gradient at the logits)
        *   hid_r   = sum_d (1 - m_bd)(x_bd lambda_rd - softplus lambda_rd)   (held out: in no gradient, not part of the loss)
        * and everything downstream -- log q, log p, nent, the IWAE weights, every backward GEMM, TF-Adam -- is the step's own.
        * x at a missing pixel is read by hid alone: a caller who knows the truth there gets the imputation score, one who does
        * not a meaningless but finite tail[5]; the loss, the gradients and tail[0..4] do not depend on it, bit for bit.
        * Tail: [0..4] as without the bit, on the masked terms; [5] sum_b mean_s (-hid_bs); [6] sum_b sum_d (1 - m_bd), the missing
        * pixels; [7] sum_b sum_d m_bd, the observed ones (both exact while B D < 2^24); the data-parallel all-reduce sums all
        * eight slots: [5] / [6] is the imputation -log-likelihood per missing pixel.  gmvae_forward's row_terms carry the masked
        * logpx, and log w is built from it.
        * The workspace grows BEHIND every other buffer by regions rounded up to 256 bytes each:
        *   "pixel_mask"  uint8 [GMVAE_LABEL_SLOTS][r256(B D)], r256 = rounded up to a multiple of 256: one mask per slot
        *   (unnamed)     uint8 [B D]: x~;  float [R][nparts]: the held-out partials beside the epilogue's own;  float [B][2]: the counts
        * (gmvae_workspace_offset answers for the name; GMVAE_E_NET without the bit).  The CALLER writes "pixel_mask"; the library
        * only reads it.  A zeroed workspace means "nothing observed": a caller fills the slots before the first step
        * (gmvae_amd.Engine does: all ones).
        * Who reads which slot: gmvae_step, gmvae_forward, gmvae_dp_step, gmvae_iw_bound, the bench and profile loops read slot 0;
        * step i of gmvae_train_graph_create's and gmvae_dp_graph_create's graph reads slot i (n_steps > GMVAE_LABEL_SLOTS:
        * GMVAE_E_DIMS); gmvae_train_graph_create_pipeline refuses the bit (GMVAE_E_DIMS).  gmvae_iw_bound honours it -- the bound
        * on log p(x_observed), through the general chunk passes at every size, noise keying unchanged, tail[5..7] = 0 --;
        * gmvae_iw_bound_enum_y, gmvae_posterior_y and gmvae_posterior_component return GMVAE_E_DIMS (masking the bit off would
        * silently score the unobserved pixels).
        * REFUSED (GMVAE_E_DIMS from gmvae_workspace_bytes and every entry point that runs or sizes a step, before any launch)
        * together with GMVAE_OBJ_MARGINAL_Y, GMVAE_OBJ_MARGINAL_Y_IW, GMVAE_GRAD_DREG, GMVAE_OBJ_LABELS, GMVAE_OBJ_WEIGHTS,
        * GMVAE_Y_TEMP_DEV or GMVAE_Y_STRAIGHT_THROUGH.
        * Every step with the bit takes the general schedule -- no one-launch, skinny, chain, evalf or plane path -- and
        * gmvae_step_schedule gives "general+mask".  At the config-5 sizes, where the step without the bit runs its top decoder
        * layer as bf16 piece products ("+planes"), the masked step runs those GEMMs on the fp32 MFMA loop: the sizes then
        * multiply there.  The masked Bernoulli epilogue (fp32 C, interior and edge tiles) keeps the observed and the held-out
        * sums as two chains; nothing assumes D % 4 == 0 (the 4-byte interior path's alignment conditions extend to the mask).
        * No atomics: eager and captured steps give the same bits. */
       GMVAE_OBJ_PIXEL_MASK = 512,
       /* optimizer (all three models, any S, together with every combination of the bits above that is legal without it): the
        * gradient is clipped by its GLOBAL NORM in front of TF-Adam -- tf.clip_by_global_norm on the batch-mean gradient, written so
        * that nothing is divided by the norm.  With g the gradient SUMS grads[0, P_padded), count = grads[P_padded + 4],
        * SS = sum_i g_i^2 and C the threshold:
        *   norm = sqrt(SS) / count                 the global norm of the mean gradient, before clipping
        *   d    = max(count, sqrt(SS) / C)         g_i / d = (g_i / count) min(1, C / norm)
        * and Adam applies g_i (1 / d): adam_tf_step's statement with d where the count stood.  SS = 0 gives d = count (no 0 / 0);
        * C = +inf never clips and only reports.  The step is SKIPPED -- params, m and v keep their bits, the step counter advances,
        * as for a poisoned step -- unless C > 0 (zero, negative, NaN: skipped), SS is finite (any NaN or +-inf gradient element:
        * skipped) and the loss sum grads[P_padded] is finite.
        * SS is a two-stage fixed-order reduction without float atomics: partial k covers elements [1024 k, 1024 (k + 1)), every
        * square exact in fp64, fp64 sums in a fixed order inside the block, the partials added in index order; sqrt, the division by
        * (double)C and the max in fp64, ONE rounding to fp32.  The padding words of the gradient buffer count towards SS: they are
        * zero after every step (the split-K slabs' padding is never written).  The record, 4 floats:
        *   [0] norm   [1] d   [2] 1.0 if d > count (the step was clipped) else 0.0   [3] the guard: the loss sum, or NaN where the
        *   step is skipped
        * shaped for adam_tf_step(..., grad_scale_dev = &rec[1], loss_sum_dev = &rec[3]).
        * The workspace grows BEHIND every other buffer by three regions, each rounded up to 256 bytes:
        *   "clip_norm"  one float, C, at the start of its cell
        *   "grad_clip"  float [GMVAE_LABEL_SLOTS][4]: the records
        *   (unnamed)    double [ceil(P_padded / 1024)]: the partials
        * (gmvae_workspace_offset answers for the two names; GMVAE_E_NET without the bit).  The CALLER writes "clip_norm"; the library
        * only reads it.  A zeroed workspace means C = 0, every step skipped: a caller fills it before the first step
        * (gmvae_amd.Engine does).  The library writes "grad_clip".
        * Who writes which record: gmvae_dp_step and gmvae_bench_loop write record 0; step i of gmvae_train_graph_create's,
        * gmvae_train_graph_create_pipeline's and gmvae_dp_graph_create's graph writes record i (n_steps > GMVAE_LABEL_SLOTS:
        * GMVAE_E_DIMS from all three; the pipeline graph ACCEPTS the bit -- it has nothing to gather).  In the data-parallel forms
        * the norm is taken on the ALL-REDUCED buffer with the global count: every rank forms the same bits, the replicas stay
        * identical.  gmvae_step sizes and schedules by the bit but runs no optimizer and writes no record (the eager path is
        * gmvae_grad_clip on its buffer, then adam_tf_step on the record).  The forward-only entries take the schedule they take
        * without the bit; gmvae_iw_bound* and gmvae_posterior_* mask it off.  gmvae_train_profile and gmvae_dp_profile return
        * GMVAE_E_DIMS (they stamp the fused optimizer launches); gmvae_step_profile honours it.
        * A training step with the bit takes the general schedule: finalize_grads leaves the partials (it holds every gradient
        * element in registers), one launch forms the record and applies TF-Adam -- ONE launch more than the same step without the
        * bit; behind an all-reduce the reduced buffer gets a partials pass of its own.  gmvae_step_schedule appends "+clip" behind
        * "+dreg":
        *   <schedule> [+marginal | +marginal_iw] [+labels] [+weights] [+temp] [+st] [+mask] [+dreg] [+clip] [+planes]
        * ("general+clip", "general+marginal_iw+labels+dreg+clip").  The eager call, the 1-step graph, the n-step graph and the
        * one-rank data-parallel forms of a step give the same record and the same update, bit for bit. */
       GMVAE_OPT_CLIP_NORM = 1024,
       /* the decoder's likelihood, a two-bit FIELD (all three models; the GMVAE with the Gumbel draw only; any S >= 1, any
        * hidden_act, with or without gen_bias_vec, any D >= 1).  0 is the Bernoulli on x in {0, 1}, untouched.  With the field x
        * stays uint8 [B, D] but carries the GREY LEVEL 0..255: t_bd = x_bd / 255; row r = b S + s belongs to example b; lambda_rd
        * is the decoder's output, MLP(z) + gen_bias_init + gen_bias_vec[d].  A one-parameter exponential family,
        *   log p(t | lambda) = (t lambda - A(lambda)) / phi + c(t):
        *   GMVAE_LIK_GREY_BERNOULLI   A = softplus               A' = sigmoid                 phi = 1        c = 0
        *                              Bernoulli cross-entropy on soft targets: NOT a normalised density on [0, 1]
        *   GMVAE_LIK_CONT_BERNOULLI   A = log((e^l - 1) / l)      A' = 1/(1 - e^-l) - 1/l      phi = 1        c = 0
        *                              (A(0) = 0, A'(0) = 1/2; Loaiza-Ganem & Cunningham 2019: a density on [0, 1])
        *   GMVAE_LIK_GAUSSIAN         A = l^2 / 2                 A' = l                       phi = sigma^2
        *                              c = -t^2 / (2 sigma^2) - ln sigma - ln(2 pi) / 2         (mean lambda, fixed scale sigma)
        *   networks that read x (encoder_y, encoder_gmm, encoder, and their first layers' weight gradients) read t as fp32
        *   logpx_r = sum_d [(t_bd lambda_rd - A(lambda_rd)) / phi + c(t_bd)]
        *   g_rd    = (A'(lambda_rd) - t_bd) / phi                    (the gradient at the logits; A'(lambda) is the mean image)
        * and everything downstream -- log q, log p, nent, the IWAE weights, every backward GEMM, TF-Adam -- is the step's own.
        * The continuous Bernoulli's A and A' come from series in lambda / 2 below |lambda| = 1 (both closed forms cancel around
        * 0, where Xavier-initialised logits sit) and from forms in exp(-|lambda|) above, finite at |lambda| = 100 and beyond.
        * Tail: [0..4] keep their meanings ([1] = sum_b mean_s (-logpx), constants included: it may be negative);
        * [5] sum_b mean_s sum_d (A'(lambda_rd) - t_bd)^2, the squared reconstruction error; [6] B D; [7] 0: [5] / [6] is the
        * per-pixel MSE; the data-parallel all-reduce sums all eight slots.  gmvae_forward's row_terms carry the new logpx, and
        * log w is built from it.
        * The workspace grows BEHIND every other buffer but GMVAE_OPT_CLIP_NORM's by regions rounded up to 256 bytes each:
        *   "lik_sigma"   under GMVAE_LIK_GAUSSIAN alone: one float, sigma, at the start of its cell
        *   (unnamed)     float [B D]: t;  float [R][nparts]: the squared-error partials beside the epilogue's own
        * (gmvae_workspace_offset answers for the name under the Gaussian; GMVAE_E_NET otherwise; "clip_norm" and "grad_clip" keep
        * resolving when both features are on).  The CALLER writes "lik_sigma"; the library only reads it, from device memory, once
        * per workgroup of the logits launch (which forms 1 / sigma^2 and ln sigma itself): a captured graph follows the cell.  A
        * zeroed workspace means sigma = 0, a non-finite step: a caller fills it before the first step (gmvae_amd.Engine does).
        * Who honours the field: gmvae_step, gmvae_forward, gmvae_train_graph_create, gmvae_dp_step, gmvae_dp_graph_create, the
        * bench and profile loops; gmvae_iw_bound -- the bound on log p(t) under the likelihood, through the general chunk passes
        * at every size, noise keying unchanged, tail[5..7] = 0 --; gmvae_train_graph_create_pipeline refuses it (GMVAE_E_DIMS:
        * that graph binarises inside); gmvae_iw_bound_enum_y, gmvae_posterior_y and gmvae_posterior_component return GMVAE_E_DIMS
        * (masking the field off would silently score Bernoulli).
        * REFUSED (GMVAE_E_DIMS from gmvae_workspace_bytes and every entry point that runs or sizes a step, before any launch)
        * together with GMVAE_OBJ_MARGINAL_Y, GMVAE_OBJ_MARGINAL_Y_IW, GMVAE_GRAD_DREG, GMVAE_OBJ_LABELS, GMVAE_OBJ_WEIGHTS,
        * GMVAE_Y_TEMP_DEV, GMVAE_Y_STRAIGHT_THROUGH or GMVAE_OBJ_PIXEL_MASK; GMVAE_OPT_CLIP_NORM combines.
        * Every step with the field takes the general schedule -- no one-launch, skinny, chain, evalf or plane path (under the
        * Gaussian the gradient at the logits is not bounded by 1, the planes' fixed scale assumes it is: at the config-5 sizes the
        * top decoder layer runs the fp32 MFMA loop, as the masked step does) -- and gmvae_step_schedule appends "+grey", "+cb" or
        * "+gauss" behind where "+mask" stands: "general+cb", "general+gauss+clip".  The likelihood epilogue (gemm.hpp EPI_LIK:
        * fp32 C, interior and edge tiles) keeps the log-probability terms and the squared errors as two chains per row, finished
        * in fp64; nothing assumes D % 4 == 0.  No atomics: eager and captured steps give the same bits. */
       GMVAE_LIK_GREY_BERNOULLI = 1 << 11,
       GMVAE_LIK_CONT_BERNOULLI = 2 << 11,
       GMVAE_LIK_GAUSSIAN = 3 << 11,
       GMVAE_LIK_MASK = 3 << 11,
       /* real-valued data: x points to float [B][D], any finite values, NOT bytes.  The parameter keeps its type
        * (const uint8_t* x) and the library reinterprets it as const float*; the pointer must be 16-byte aligned
        * (GMVAE_E_ALIGN), and step s of a train graph reads the floats at x + s B D.  Requires GMVAE_LIK_GAUSSIAN (GMVAE_E_DIMS
        * with any other value of the field): t_bd = x_bd itself.  The networks' first layers and their weight gradients take x
        * as the fp32 operand -- no t pass, no t region in the workspace --, and the likelihood epilogue reads its target as a
        * float on every tile path (interior, last column tile, element by element where D % 4 != 0 or a row is unaligned).
        * tail[5] and tail[6] stay the squared error and B D.  "general+gauss+f32". */
       GMVAE_X_F32 = 1 << 13,
       /* the Gaussian's scale per dimension and learned: sigma_d = exp(rho_d), rho = "decoder/log_sigma" [1, D], the LAST entry
        * of the parameter layout (gmvae_param_count / gmvae_param_layout report it under this bit alone; P_padded grows by D
        * rounded up to 4; without the bit the layout is unchanged).  Requires GMVAE_LIK_GAUSSIAN (GMVAE_E_DIMS otherwise); byte
        * or fp32 input.  The "lik_sigma" cell is absent (GMVAE_E_NET).
        *   log p(t_bd | lambda_rd) = -(lambda_rd - t_bd)^2 / (2 sigma_d^2) - rho_d - ln(2 pi) / 2
        *   g_rd = (lambda_rd - t_bd) / sigma_d^2                  (the epilogue loads rho per column quad, as the bias)
        *   d loss / d rho_d = sum_r rw_r (1 - sigma_d^2 g_rd^2)   (rw: the backward's row weights, 1 where the step has none)
        * The last line is a launch pair of its own behind the backward's row weights (liksig.hpp): a row-weighted column
        * reduction over the stored g [R][D], fixed order, no atomics, then the slab partials summed in index order into the
        * gradient buffer's slabs -- a SUM like every other entry, so TF-Adam, GMVAE_OPT_CLIP_NORM, the data-parallel all-reduce
        * and checkpoints treat rho as any other parameter.  "general+gauss+lsig", "general+gauss+f32+lsig+clip".
        * Both bits: honoured and refused exactly where GMVAE_LIK_GAUSSIAN is (above). */
       GMVAE_LIK_SCALE_LEARNED = 1 << 14,
       /* count data: x is float [B][D] holding finite values >= 0 (integer-valued in practice; nothing assumes it, lgamma takes
        * reals), lambda_rd -- the decoder's output exactly as above -- is the LOG-MEAN.  Two bits, mutually exclusive; each
        * requires GMVAE_X_F32 (so x 16-byte aligned, GMVAE_E_ALIGN), the GMVAE_LIK_* field 0 and GMVAE_LIK_SCALE_LEARNED clear
        * (GMVAE_E_DIMS otherwise).  Networks that read x read t_bd = log1p(x_bd) as fp32; the likelihood's target is x_bd.
        *   GMVAE_LIK_POISSON        log p = x l - exp(l) - lgamma(x + 1)                     g = exp(l) - x
        *                            (no clamp: l > 88 gives a non-finite step, which GMVAE_OPT_CLIP_NORM skips)
        *   GMVAE_LIK_NEG_BINOMIAL   mean exp(l), inverse dispersion r_d = exp(rho_d), u = l - rho_d, sp = softplus:
        *                            log p = lgamma(x + r) - lgamma(r) - lgamma(x + 1) - x sp(-u) - r sp(u)
        *                            g = (r + x) sigmoid(u) - x
        *                            d log p / d rho_d = r [psi(x + r) - psi(r) - sp(u)] + g         (psi = digamma)
        *                            (lambda is never exponentiated alone: finite for every finite lambda and rho)
        * rho = "decoder/log_dispersion" [1, D] is the LAST entry of the parameter layout under GMVAE_LIK_NEG_BINOMIAL, in the
        * slot and with the padding rules of "decoder/log_sigma": TF-Adam, GMVAE_OPT_CLIP_NORM, the all-reduce and checkpoints see
        * an ordinary parameter.  Its gradient is a launch pair behind the backward's row weights (count.hpp: fp64 digamma by
        * recurrence to an argument >= 6 and the asymptotic series; a row-weighted fixed-order fp64 column reduction over the stored
        * g and sp(u) planes, no atomics, slab 0 of rho's range written and the other slabs zeroed).
        * The terms of log p that do not depend on lambda are summed once per example in fp64 by the rows pass that also writes
        * t (c_b = sum_d [lgamma(x + r_d) - lgamma(r_d)] - lgamma(x + 1), an fp64 difference) and added to each of its S rows.
        * Tail: [0..4] keep their meanings ([1] includes every constant); [5] = sum_b mean_s sum_d (log1p(exp lambda_rd) -
        * log1p(x_bd))^2, the squared error of the mean on the scale the networks see; [6] = B D; [7] = 0.
        * The workspace grows where GMVAE_LIK_*'s regions stand: float [B D] t, float [R][nparts] the squared-error partials, float
        * [B] c; under the negative binomial float [R D] sp(u) and the dispersion pass's fp64 slab partials.
        * Honoured and refused exactly where GMVAE_LIK_GAUSSIAN | GMVAE_X_F32 is: the general schedule only; GMVAE_OPT_CLIP_NORM
        * combines, every other objective bit returns GMVAE_E_DIMS; gmvae_iw_bound gives the bound on log p(x) under the count
        * likelihood; the pipeline graph and every other evaluator (*_enum_y, posterior_*, impute, ais*, simulate, refine) refuse
        * before any launch.  gmvae_step_schedule appends "+pois" or "+nb" where "+gauss" stands: "general+nb+f32+clip". */
       GMVAE_LIK_POISSON = 1 << 15,
       GMVAE_LIK_NEG_BINOMIAL = 1 << 16 };
#define GMVAE_LABEL_SLOTS 32  /* label sets (GMVAE_OBJ_LABELS) / weight rows (GMVAE_OBJ_WEIGHTS) / temperatures (GMVAE_Y_TEMP_DEV) / masks (GMVAE_OBJ_PIXEL_MASK) a workspace holds: the most steps of one train graph */
enum { GMVAE_ACT_RELU = 0, GMVAE_ACT_TANH = 1, GMVAE_ACT_SIGMOID = 2, GMVAE_ACT_ELU = 3 };

/* One tensor of the flat parameter buffer.  Names are the reference's TF
 * variable names (scripts/base.py:53,60 '<name>_fcnet/linear_<i>/{w,b}';
 * scripts/vae.py:233-238 'loc','raw_scale_diag','mixture_logits'), in the
 * reference's variable-creation order. */
typedef struct GmvaeParamEntry {
  char name[64];
  int32_t rows;                       /* w: in  ; b: 1 ; loc: K              */
  int32_t cols;                       /* w: out ; b: out                     */
  uint64_t offset;                    /* in floats, multiple of 4            */
} GmvaeParamEntry;

/* sub-network ids for gmvae_mlp_forward */
enum {
  GMVAE_NET_ENCODER_Y = 0,            /* scripts/gmvae.py:340-345            */
  GMVAE_NET_PRIOR_GMM = 1,            /* scripts/gmvae.py:321-327            */
  GMVAE_NET_ENCODER_GMM = 2,          /* scripts/gmvae.py:347-353            */
  GMVAE_NET_DECODER = 3,              /* scripts/gmvae.py:331-336, vae.py:254-259 */
  GMVAE_NET_ENCODER = 4               /* scripts/vae.py:262-268              */
};

int gmvae_abi_version(void);

/* Replaces variable creation in create_vae / create_gmvae
 * (scripts/vae.py:191-271, scripts/gmvae.py:277-356): sizes of the flat
 * buffer.  P_padded counts the 16-byte alignment padding, P_real does not
 * (166,618 for GMVAE D=784 H=64 L=64 K=10). */
int gmvae_param_count(const GmvaeDims* dims, int model, uint64_t* P_padded, uint64_t* P_real);
int gmvae_param_layout(const GmvaeDims* dims, int model, GmvaeParamEntry* out, int max_entries, int* n_entries);

int gmvae_workspace_bytes(const GmvaeDims* dims, int model, uint64_t* bytes);

/* TrainableGMVAE.run_model (scripts/gmvae.py:223-274) /
 * TrainableVAE.run_model (scripts/vae.py:153-188) PLUS the reverse-mode pass
 * of opt.compute_gradients (scripts/runners.py:182).
 *   x     uint8 [B,D]
 *   eps   fp32 [B*S,L]  N(0,1) noise     (MultivariateNormalDiag.sample)
 *   u     fp32 [B*S,K]  U[tiny,1) noise  (RelaxedOneHotCategorical.sample; GMVAE only)
 *         eps/u NULL => generated in-kernel by Philox4x32-10(seed, step)
 *   grads fp32 [P_padded + GMVAE_TAIL], OUT: SUMS over this device's rows of
 *         d loss_b / d theta (NOT divided by B), then the tail
 *         [0] sum_b loss_b  [1] sum nll  [2] sum kl  [3] sum nent  [4] B
 *         (nll/kl are averaged over S inside a row group) -- one RCCL
 *         all-reduce(SUM) of this buffer makes it global; adam_tf_step's
 *         grad_scale = 1/tail[4] turns sums into the reference's batch means.
 *   step_dev (may be NULL): device-resident step counter for hipGraph replay: TWO uint64 words, [0] the counter,
 *         [1] a scratch copy the step's launches hand to each other (every entry point that takes step_dev).
 *         When given it overrides `step` for the Philox stream and is
 *         incremented once per call (after the noise is drawn), so that
 *         adam_tf_step(t_dev = step_dev) later on the stream sees t = step+1.
 */
int gmvae_step(const GmvaeDims* dims, int model, const uint8_t* x, const float* eps, const float* u,
               const float* params, float* grads, void* workspace, uint64_t seed, uint64_t step,
               uint64_t* step_dev, void* stream);

/* Forward only (eval: scripts/runners.py:324-333).  tail: float[GMVAE_TAIL]
 * as above.  row_terms (may be NULL): fp32 [B*S,4] = logpx, logq, logp, logw.
 * z_out (may be NULL) [B*S,L]; y_out (may be NULL, GMVAE) [B*S,K];
 * logits_out (may be NULL, GMVAE) [B,K] = q_y.distribution.logits. */
int gmvae_forward(const GmvaeDims* dims, int model, const uint8_t* x, const float* eps, const float* u,
                  const float* params, float* tail, float* row_terms, float* z_out, float* y_out,
                  float* logits_out, void* workspace, uint64_t seed, uint64_t step, void* stream);

/* The importance-weighted bound at n_samples importance samples per row (the IWAE estimate of log p(x) for VAE / VAE_GMP; for
 * the GMVAE the project's A15 bound -- relaxed y, the analytic -sum pi ln pi term -- that gmvae_forward reports at S = n),
 * streamed in chunks of dims->S samples (the last chunk may be partial): memory does not grow with n_samples.
 * Noise of sample s (0 <= s < n_samples) of batch row b: Philox row (dims->row0 + b) * n_samples + s, so the result does not
 * depend on the chunk size, the batch size or the sharding.  With n_samples == dims->S this is exactly gmvae_forward's keying
 * (row0*S + b*S + s).
 *   bound_out [B] (may be NULL): logsumexp_s(log w_bs) - log n;  mean_logw_out [B] (may be NULL): mean_s log w_bs;
 *   tail [GMVAE_TAIL]: as gmvae_forward's at S = n (sum of -bound, the per-row means of nll / kl, nent, count B).
 * The workspace (its size from gmvae_iw_bound_workspace_bytes at the same dims; zeroed once, one set of dims) holds the forward's
 * workspace at S = the chunk and the per-row running state (max and sum of exp, sums of log w, nll and kl, in fp64), which the
 * first chunk initialises.  One call enqueues ceil(n_samples / S) chunk passes on `stream`; at the reference's default sizes
 * (the ones evalf.hpp takes) ONE launch per chunk after the first layers.  It prepares its operand images itself, once per
 * call (dims->sched_flags' GMVAE_SCHED_EVAL_IMAGES_VALID is ignored).  GMVAE_E_DIMS if n_samples == 0 or
 * (row0 + B) * n_samples >= 2^38; GMVAE_E_ALIGN for unaligned x, params, outputs or workspace. */
int gmvae_iw_bound_workspace_bytes(const GmvaeDims* dims, int model, uint64_t* bytes);
int gmvae_iw_bound(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, uint64_t n_samples,
                   float* bound_out, float* mean_logw_out, float* tail, void* workspace, uint64_t seed, uint64_t step,
                   void* stream);

/* The GMVAE's importance-weighted bound with y summed out exactly over its K components (an importance-sampling estimate of
 * log p(x) for the model's discrete y; q(y|x) cancels out of it), n_samples samples of z per component, streamed in chunks of
 * dims->S samples per component:
 *   bound_b = logsumexp_{s < n, k < K} log w'_bsk - log n,
 *   log w'_bsk = log p(x_b|z_bsk) + log p(z_bsk|e_k) - log q(z_bsk|x_b,e_k),  z_bsk = mu_q(x_b,e_k) + sigma_q(x_b,e_k) eps_bsk,
 * which is log p(x_b) + ln K for a uniform p(y) (the + ln K is left out, as in GMVAE_OBJ_MARGINAL_Y's objective).  It depends on
 * the generative model and q(z|x,y) only: the same for a GMVAE trained with either objective.  GMVAE only (GMVAE_E_MODEL for
 * the VAE family); the GMVAE_OBJ_MARGINAL_Y and GMVAE_OBJ_MARGINAL_Y_IW bits of dims->sched_flags are ignored (the result is
 * the same with or without them).
 * Noise of sample s of component k of batch row b: Philox row ((dims->row0 + b) * n_samples + s) * K + k -- independent of the
 * chunk, the batch and the sharding; at n_samples == 1 the marginal gmvae_forward's keying ((row0 + b) * K + k).
 *   bound_out [B] (may be NULL): bound_b;  mean_logw_out [B] (may be NULL): sum_k q_bk mean_s log w'_bsk - sum_k q_bk ln q_bk
 *   (<= bound_b for every draw; at n_samples == 1 it is -L_b of the marginal objective);
 *   tail [GMVAE_TAIL]: [0] sum_b -bound_b, [1] sum_b sum_k q_bk mean_s nll_bsk, [2] the same of kl, [3] sum_b nent_b, [4] B,
 *   [5..7] 0 (at n_samples == 1, [1..4] are the marginal gmvae_forward's).
 * The workspace (its size from gmvae_iw_bound_enum_y_workspace_bytes at the same dims; zeroed once) holds the marginal forward's
 * at B * S * K rows and the per-row fp64 running state.  Per chunk: a strided noise fill, the forward (general schedule, y = e_k
 * as gather-adds), one merge launch; the tail once.  Fixed-order reductions: two calls give the same bits.  GMVAE_E_DIMS if
 * n_samples == 0, (row0 + B) * n_samples * K >= 2^38 or B * S * K > 2^30; GMVAE_E_ALIGN for unaligned x, params, outputs or
 * workspace. */
int gmvae_iw_bound_enum_y_workspace_bytes(const GmvaeDims* dims, int model, uint64_t* bytes);
int gmvae_iw_bound_enum_y(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, uint64_t n_samples,
                          float* bound_out, float* mean_logw_out, float* tail, void* workspace, uint64_t seed, uint64_t step,
                          void* stream);

/* The GMVAE's own posterior over its component y, p(y = k | x_b) ~ p(x_b | y = k) p(y = k) (normalised over k) with a uniform p(y), by importance
 * sampling per component: gmvae_iw_bound_enum_y's samples and weights (the same log w'_bsk, Philox rows, chunks of dims->S
 * samples per component, limits and error codes; the GMVAE_OBJ_MARGINAL_Y* bits ignored; GMVAE_E_MODEL for the VAE family) with
 * the logsumexp kept per component instead of folded over (s, k):
 *   l_bk = logsumexp_{s < n} log w'_bsk - log n      (an estimate of log p(x_b | y = k); no +/- ln K, as the bound above)
 *   r_bk = softmax_k l_bk                             (the model's posterior; the uniform p(y) cancels)
 *   log_joint_out [B][K] (may be NULL): l_bk;
 *   log_post_out [B][K] (may be NULL): ln r_bk = l_bk - logsumexp_j l_bj (usable as gmvae_cluster_acc's logits: its argmax);
 *   stats_out [B][4] (may be NULL): [0] bound_b = logsumexp_k l_bk (the value gmvae_iw_bound_enum_y reports),
 *     [1] H(r_b) = -sum_k r_bk ln r_bk, [2] KL(q_b || r_b) = sum_k q_bk (ln q_bk - ln r_bk), q_b = softmax of encoder_y's logits,
 *     [3] ESS_b = (sum_{s,k} w)^2 / sum_{s,k} w^2, w = exp(log w'_bsk): the effective sample size, in [1, n K];
 *   tail [GMVAE_TAIL]: [0] sum_b -bound_b, [1] sum_b H(r_b), [2] sum_b KL(q_b || r_b), [3] sum_b ESS_b, [4] B, [5..7] 0.
 * Two identities: bound_b is gmvae_iw_bound_enum_y's on the same dims, seed and step; and -L_b = bound_b - KL(q_b || r_b) for
 * GMVAE_OBJ_MARGINAL_Y_IW's objective L_b at S = n_samples on the same noise (KL(q || r) is exactly the part of that bound's gap
 * the y-encoder is responsible for).
 * The workspace (its size from gmvae_posterior_y_workspace_bytes at the same dims; zeroed once) is gmvae_iw_bound_enum_y's plus
 * the per-(row, component) fp64 running state [B][K][3] (max, sum of exp, sum of exp of twice), which the first chunk writes.
 * Per chunk: the strided noise fill, the forward, one merge launch; then one finishing launch and the tail.  Results do not
 * depend on the chunk, the batch or the sharding beyond fp32 summation order; fixed-order reductions, no float atomics: two
 * calls give the same bits.  GMVAE_E_DIMS if n_samples == 0, (row0 + B) * n_samples * K >= 2^38 or B * S * K > 2^30;
 * GMVAE_E_ALIGN for unaligned x, params, outputs or workspace; GMVAE_E_NULL for a missing x, params, tail or workspace. */
int gmvae_posterior_y_workspace_bytes(const GmvaeDims* dims, int model, uint64_t* bytes);
int gmvae_posterior_y(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, uint64_t n_samples,
                      float* log_joint_out, float* log_post_out, float* stats_out, float* tail, void* workspace, uint64_t seed,
                      uint64_t step, void* stream);

/* The VAE_GMP's own posterior over the component k of its learned mixture prior, p(k | x_b) ~ pi_k p(x_b | k), by importance
 * sampling.  The component enters neither the encoder nor the decoder, so ONE sample z_bs = mu_q(x_b) + sigma_q(x_b) eps_bs serves
 * all K components: gmvae_iw_bound's samples (the same Philox rows (row0 + b) n + s, chunks of dims->S samples, limits and error
 * codes) with the mixture's logsumexp left open,
 *   log w_bsk = log p(x_b | z_bs) + ln pi_k + log N(z_bs; loc_k, s_k) - log q(z_bs | x_b)     (pi = softmax(mixture_logits),
 *                                                                                              s = softplus(raw_scale_diag))
 *   l_bk = logsumexp_{s < n} log w_bsk - log n        (an estimate of log p(x_b, k))
 *   r_bk = softmax_k l_bk                              (the model's posterior)
 *   log_joint_out [B][K] (may be NULL): l_bk;
 *   log_post_out [B][K] (may be NULL): ln r_bk (usable as gmvae_cluster_acc's logits: its argmax);
 *   stats_out [B][4] (may be NULL): [0] bound_b = logsumexp_k l_bk (gmvae_iw_bound's bound: logsumexp_k log w_bsk = log w_bs),
 *     [1] H(r_b) = -sum_k r_bk ln r_bk, [2] KL(r_b || pi) = sum_k r_bk (ln r_bk - ln pi_k) (its mean over a split estimates the
 *     mutual information I(x; k)), [3] ESS_b = (sum_s w_bs)^2 / sum_s w_bs^2, w_bs = sum_k w_bsk: the effective sample size of
 *     gmvae_iw_bound's own weights, in [1, n];
 *   tail [GMVAE_TAIL]: [0] sum_b -bound_b, [1] sum_b H(r_b), [2] sum_b KL(r_b || pi), [3] sum_b ESS_b, [4] B, [5..7] 0.
 * Every component term stays in the log domain (never log w_bs + ln of a responsibility, which underflows): l_bk is finite and
 * accurate for components far from z.  GMVAE_MODEL_VAE_GMP only: GMVAE_E_MODEL for the VAE and the GMVAE.
 * The workspace (its size from gmvae_posterior_component_workspace_bytes at the same dims; zeroed once) is gmvae_iw_bound's plus
 * the per-(row, component) fp64 running state [B][K][2] (max, sum of exp), the per-row [3] of the effective sample size and the
 * chunk's [B S][max(K, L)] component terms or latents.  At the reference's default sizes one launch per chunk (the fold inside
 * it); elsewhere the strided noise fill, the forward and one merge launch; then one finishing launch and the tail.  One owner per
 * (row, component), fixed-order reductions, no float atomics: two calls give the same bits; the result does not depend on the
 * chunk, the batch or the sharding beyond the forward's own summation order and the fp64 rounding of the folds.  (The one-launch
 * schedule is not taken at S = 1 with more than 8 batch rows per workgroup, as for gmvae_forward: such a call runs the general
 * loop, whose summation order follows B * S.)  GMVAE_E_DIMS if n_samples == 0,
 * (row0 + B) * n_samples >= 2^38 or B * S > 2^30; GMVAE_E_ALIGN for unaligned x, params, outputs or workspace; GMVAE_E_NULL for a
 * missing x, params, tail or workspace.  Every check happens before any launch. */
int gmvae_posterior_component_workspace_bytes(const GmvaeDims* dims, int model, uint64_t* bytes);
int gmvae_posterior_component(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, uint64_t n_samples,
                              float* log_joint_out, float* log_post_out, float* stats_out, float* tail, void* workspace,
                              uint64_t seed, uint64_t step, void* stream);

/* Imputation of the missing pixels by self-normalised importance sampling (Mattei & Frellsen, MIWAE, 2019) on gmvae_iw_bound's
 * own weights: the same samples (Philox rows (row0 + b) n + s, chunks of dims->S samples, limits and error codes), the same
 * log w_bs -- under GMVAE_OBJ_PIXEL_MASK from the observed pixels alone, the mask read from slot 0; without the bit every pixel
 * is observed and the result is the posterior-mean reconstruction.  With w~_bs = softmax_s log w_bs, lambda_bs the decoder's
 * logits at z_bs (gen_bias_init included, scalar or vector) and hid_bs the held-out Bernoulli term (GMVAE_OBJ_PIXEL_MASK above):
 *   mean_out [B][D] (may be NULL): p^_bd = sum_s w~_bs sigmoid(lambda_bsd) ~ E[x_d | x_observed], at EVERY pixel, observed or not;
 *   stats_out [B][4] (may be NULL): [0] bound_b = logsumexp_s log w_bs - log n, gmvae_iw_bound's bound bit for bit;
 *     [1] ESS_b = (sum_s w_bs)^2 / sum_s w_bs^2, in [1, n]; [2] cond_loglik_b = logsumexp_s (log w_bs + hid_bs) -
 *     logsumexp_s log w_bs ~ log p(x_missing | x_observed) at the x given (the proper score of an imputation; exactly 0 for a
 *     row with nothing missing; x at a missing pixel is read by this output alone); [3] max_s w~_bs;
 *   logw_out [B][n] (may be NULL): log w_bs -- the one output whose size follows n;
 *   draw_index_out [B][M] int64 and draw_z_out [B][M][L] (each may be NULL; M = n_draws in 0 .. 16): sampling-importance-
 *     resampling by the Gumbel-max rule, draw m keeps s* = argmax_s (log w_bs + g_bsm), g = -ln(-ln u), u = column
 *     4 ceil(K / 4) + m of the u stream of sample s's Philox row (behind the columns the forward itself may read); ties go to
 *     the lower s; draw_z is that sample's z: decoding it and drawing the missing pixels gives one multiple imputation;
 *   tail [GMVAE_TAIL]: [0] sum_b -bound_b, [1] sum_b ESS_b, [2] sum_b cond_loglik_b, [3] sum_b of the missing pixels, [4] B, [5..7] 0.
 * A weight of exactly 0 (log w = -inf) contributes nothing and makes no NaN; a row whose weights are all 0, or that holds a NaN,
 * gives NaN in mean_out and stats_out[1..3].  Every size takes the general chunk passes (never the one-launch evaluation: the
 * decoder's top activation is read back from the workspace); per chunk the strided noise fill, the forward, iw_merge, then
 * impute_merge (a wave per row: the fp64 fold of the weights, the draws' reservoirs) and impute_fold (csrc/impute.hip: the output
 * layer recomputed as fp32 MFMA products against a 64-column tile of its weights held in LDS, sigmoid and the weighted sum over the
 * chunk's samples in the epilogue, fp64 accumulators [B][pad4(D)] in the workspace -- the [B n D] mean images are never stored);
 * then impute_finish and the tail.  One owner per output, fixed-order reductions, no float atomics: two calls give the same bits;
 * the result does not depend on the chunk, the batch or the sharding beyond the forward's own summation order and the fp64
 * rounding of the folds.  The workspace (its size from gmvae_impute_workspace_bytes at the same dims and n_draws; zeroed once) is
 * gmvae_iw_bound's plus the chunk's z and weights, the per-row state and the accumulators.
 * GMVAE_E_DIMS for a GMVAE_LIK_* other than Bernoulli, GMVAE_OBJ_MARGINAL_Y*, n_draws outside 0 .. 16, n_samples == 0 or
 * (row0 + B) * n_samples >= 2^38; GMVAE_E_ALIGN for unaligned x, params, outputs or workspace; GMVAE_E_NULL for a missing x,
 * params, tail or workspace.  Every check happens before any launch. */
int gmvae_impute_workspace_bytes(const GmvaeDims* dims, int model, int n_draws, uint64_t* bytes);
int gmvae_impute(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, uint64_t n_samples, int n_draws,
                 float* mean_out, float* stats_out, float* logw_out, int64_t* draw_index_out, float* draw_z_out,
                 float* tail, void* workspace, uint64_t seed, uint64_t step, void* stream);

/* The log-density of a weighted diagonal-Gaussian mixture at M query points, streamed over chunks of components (model
 * independent; Engine.aggregate_posterior runs the aggregate posterior q(z) = 1/N sum_n q(z|x_n) and the mixture priors through
 * it).  Components c < C of a chunk: logw [C] (finite or -inf: a -inf component contributes nothing and yields no NaN), mu [C][L],
 * sigma [C][L]; queries z [M][L]; all fp32 in device memory.  PRECONDITION: sigma > 0 (as the step's own -log q terms assume;
 * nothing clamps it here).  Per query m, over the components of every chunk accumulated since the workspace was zeroed:
 *   log_joint [m]  = logsumexp_c (logw_c + sum_d log N(z_md; mu_cd, sigma_cd)) - log_norm
 *   log_dim [m][d] = logsumexp_c (logw_c + log N(z_md; mu_cd, sigma_cd)) - log_norm     (per_dim != 0 only: it is L times the
 *                    exponentials, and a call with per_dim == 0 launches none of it)
 *   log_own [m]    = the logsumexp of log_joint restricted to the components of the query's own example, no log_norm subtracted
 *                    (query_owner != NULL only).  Components are laid out example-major: global component c_first + c belongs to
 *                    example (c_first + c) / comps_per_owner, and query_owner [M] (int64) names each query's example.  It comes
 *                    from the same fp32 terms as log_joint, so log q(z|x) - log q(z) carries no rounding of its own.
 * gmvae_mixture_logpdf_accumulate folds one chunk into the running state of the M queries (c_first: the global index of the
 * chunk's first component); gmvae_mixture_logpdf_finish writes the outputs (each may be NULL; log_dim_out is ignored at
 * per_dim == 0; a state no component has reached gives -inf).  M, L and per_dim must be the same in the size query, in every
 * accumulate and in finish: they fix the workspace's layout.
 * The workspace (gmvae_mixture_logpdf_workspace_bytes; a ZEROED workspace is the empty state, so zero it before the first chunk
 * of every evaluation) holds an fp64 (max, sum of exp(. - max)) per query, per own and per (query, dimension), and as many again
 * per slice of a chunk: memory grows with M (and M L under per_dim), never with the number of components.  A sum of 0 marks an
 * empty state, so log-densities of -1e4 to -1e7 (far components) come out finite.  Arithmetic: r = (z - mu) (1 / sigma) in fp32
 * on the vector units; per tile of components a max and an fp32 sum of exponentials; fp64 across tiles, slices and calls.  One
 * owner per state, fixed-order folds, no float atomics: two calls give the same bits; chunking changes only the fp64 fold order.
 * Checks, before any launch, in this order: GMVAE_E_DIMS (M, L or C < 1, M or C > 2^30, L > 2^16, c_first < 0, comps_per_owner < 1
 * with a query_owner); GMVAE_E_NULL (z, mu, sigma, logw, workspace, bytes); GMVAE_E_ALIGN (float arrays 4 bytes, query_owner 8,
 * the workspace 16). */
int gmvae_mixture_logpdf_workspace_bytes(int64_t M, int L, int per_dim, uint64_t* bytes);
int gmvae_mixture_logpdf_accumulate(const float* z, int64_t M, int L, const float* mu, const float* sigma, const float* logw,
                                    int64_t C, int64_t c_first, int64_t comps_per_owner, const int64_t* query_owner, int per_dim,
                                    void* workspace, void* stream);
int gmvae_mixture_logpdf_finish(int64_t M, int L, int per_dim, double log_norm, float* log_joint_out, float* log_dim_out,
                                float* log_own_out, const void* workspace, void* stream);

/* Exact t-SNE of N codes into two dimensions on the device (model independent; gmvae_amd.tsne.embed, utils.reduce_dimensionality
 * and run_eval's --embed_latent go through it; the reference's evaluation does the same with scikit-learn, scripts/utils.py:148-153).
 * O(N^2) per iteration, no tree, no FFT; memory grows with N (and rows N for the affinity stage), never with N^2.
 * codes [N][L], beta / logz / entropy [N], y / vel / gains / grad_out [N][2], kl_history [n_iter], stats_out [4]: fp32 in device
 * memory.  d2_ij = sum_d (c_id - c_jd)^2 in the difference form, fp64 differences and sum.
 *   gmvae_tsne_affinities, for the rows i in [r0, r0 + rows): the beta_i > 0 at which the entropy of p_{j|i} = exp(-beta_i d2_ij -
 *     logz_i), logz_i = logsumexp_{j != i}(-beta_i d2_ij), is ln(perplexity): beta = 1, doubled or halved until the root is
 *     bracketed, then bisected until fp32 cannot split the bracket (at most 100 halvings; H's sums in fp64), which leaves
 *     |H_i - ln perplexity| far inside 1e-5 and beta, logz and p_{j|i} at the root where H is flat in beta.  The customary stop
 *     at |H_i - ln perplexity| <= 1e-5 is deliberately NOT applied: where a row's nearest neighbours nearly tie it leaves logz
 *     2.6e-4 off the root (csrc/tsne.hpp).  It writes beta, logz and
 *     entropy (the H_i reached) at [r0, r0 + rows) and nothing else outside the workspace; a row's result does not depend on
 *     (r0, rows), so a caller may chunk the rows to bound the workspace.  A row with no root -- a point with at least `perplexity`
 *     exact duplicates -- keeps the last beta tried and reports the entropy reached there.
 *   gmvae_tsne_gradient, at the embedding y with p_ij = (p_{j|i} + p_{i|j}) / 2N, p_ii = 0, w_ij = 1 / (1 + |y_i - y_j|^2),
 *     Z = sum_{i != j} w_ij:  grad_out_i = 4 sum_j (exaggeration p_ij - w_ij / Z) w_ij (y_i - y_j);  stats_out (may be NULL) =
 *     {Z, sum p ln w, KL, sum p ln p} with KL = sum p ln p - sum p ln w + ln Z over i != j (the un-exaggerated P; p = 0
 *     contributes 0).
 *   gmvae_tsne_run: n_iter iterations of (gradient; scikit-learn's _gradient_descent update without recentring: gains += 0.2
 *     where vel grad < 0, else gains *= 0.8, floored at 0.01; vel = momentum vel - lr gains grad; y += vel) enqueued on `stream`
 *     with no host synchronisation: exaggeration and momentum 0.5 for the iterations it < exaggeration_iters, then 1 and 0.8.
 *     y holds the initial embedding on entry and the result on return; vel and gains are the caller's state (0 and 1 to begin
 *     with).  kl_history (may be NULL) [it] = the KL at the embedding iteration `it` started from.
 * The workspace (gmvae_tsne_workspace_bytes(N, L, rows): rows = the most rows an affinity call will take, 1 if none) holds the
 * pairwise pass's fp64 partial sums per point and slice and the chunk's d2 [rows][N]; it needs no initialisation, and every call
 * leaves it free for the next.  The caller owns every other byte: no call writes outside its outputs and the workspace.
 * One owner per sum, fixed-order fp64 folds, no float atomics: two calls give the same bits.
 * Checks, before any launch, in this order: GMVAE_E_DIMS (N < 4, N > 2^20, L < 1, L > 2^16, perplexity outside (1, N - 1),
 * rows < 1, r0 < 0 or r0 + rows > N, n_iter < 0); GMVAE_E_NULL (any pointer not marked "may be NULL"); GMVAE_E_ALIGN (float
 * arrays 4 bytes, the workspace 16). */
int gmvae_tsne_workspace_bytes(int64_t N, int L, int64_t rows, uint64_t* bytes);
int gmvae_tsne_affinities(const float* codes, int64_t N, int L, float perplexity, int64_t r0, int64_t rows, float* beta,
                          float* logz, float* entropy, void* workspace, void* stream);
int gmvae_tsne_gradient(const float* codes, int64_t N, int L, const float* beta, const float* logz, const float* y,
                        float exaggeration, float* grad_out, float* stats_out, void* workspace, void* stream);
int gmvae_tsne_run(const float* codes, int64_t N, int L, const float* beta, const float* logz, float* y, float* vel,
                   float* gains, int n_iter, int exaggeration_iters, float exaggeration, float lr, float* kl_history,
                   void* workspace, void* stream);

/* A K-component diagonal Gaussian mixture fitted to N codes by EM on the device, and the responsibilities of a given mixture
 * (model independent; gmvae_amd.mixfit.fit / assign, model.fit_latent_mixture, model.init_prior_from_mixture and run_eval's
 * --fit_latent_mixture go through it; the reference has no counterpart).  The statement is tests/mixfit_ref.py.
 * codes z [N][L], logw [K], mu / sigma [K][L], log_resp_out [N][K], lse_out [N], loglik_history [n_iter], counts_out [K]: fp32 in
 * device memory.  A logw entry may be -inf: such a component contributes nothing and yields no NaN.  PRECONDITION: sigma > 0 (as
 * for gmvae_mixture_logpdf_*; nothing clamps it here).
 *   E-step:  l_nk = logw_k - 1/2 sum_d ((z_nd - mu_kd) / sigma_kd)^2 - sum_d ln sigma_kd - (L/2) ln 2 pi (the difference form, fp64
 *     on the vector units: log r is a difference of numbers of the size of l, csrc/mixfit.hpp);  lse_n = logsumexp_k l_nk,
 *     max-subtracted;  log r_nk = l_nk - lse_n;  r_nk = exp(log r_nk), an fp32 exponential.
 *   M-step, centred at the current mean (the differences z_nd - mu_kd come first; no sum r z^2 - mean^2 form anywhere):
 *     R_k = sum_n r_nk, S1_kd = sum_n r_nk (z_nd - mu_kd), S2_kd = sum_n r_nk (z_nd - mu_kd)^2, all three in fp64;
 *     R'_k = R_k + 10 * 2^-52 (scikit-learn's constant), m_kd = S1_kd / R'_k, mu'_kd = mu_kd + m_kd,
 *     sigma'_kd = sqrt(max(S2_kd / R'_k - m_kd^2, 0) + reg_covar), logw'_k = ln(R'_k / sum_j R'_j).  No component is special-cased:
 *     an empty one keeps its mean, gets sigma = sqrt(reg_covar) and a weight of about 10 * 2^-52 / N.
 *   gmvae_mixfit_assign: the E-step at the given parameters: log_resp_out and lse_out (each may be NULL).
 *   gmvae_mixfit_run: n_iter iterations enqueued on `stream` with no host synchronisation, two launches each: iteration `it` runs
 *     the E-step at the current parameters, records loglik_history [it] = 1/N sum_n lse_n (may be NULL; the value the iteration
 *     started from, as kl_history does), then applies the M-step to logw, mu and sigma in place.  counts_out (may be NULL) = R_k of
 *     the last iteration.  n_iter = 0 is a valid call that changes nothing.
 * Sizes: 1 <= N <= 2^24, 1 <= L <= 4096, 1 <= K <= 256 and K L <= 16,384 -- the parameter image (mu and 1 / sigma) stays resident
 * in the LDS of every workgroup, and at K L = 16,384 it takes 128 KiB of the 160 KiB; nothing needs to be a multiple of anything.
 * The workspace (gmvae_mixfit_workspace_bytes(N, L, K)) holds the workgroups' fp64 partial sums, K (2 L + 1) + 1 values for each of
 * at most 256 workgroups, and nothing per row; it needs no initialisation, and every call leaves it free for the next.  The caller
 * owns every other byte: no call writes outside its outputs, the parameters (run) and the workspace.
 * One owner per sum, fixed-order fp64 folds, no float atomics: two calls give the same bits.
 * Checks, before any launch, in this order: GMVAE_E_DIMS (N < 1, N > 2^24, L < 1, L > 4096, K < 1, K > 256, K L > 16,384, n_iter < 0,
 * reg_covar not finite and > 0); GMVAE_E_NULL (any pointer not marked "may be NULL"); GMVAE_E_ALIGN (float arrays 4 bytes, the
 * workspace 16). */
int gmvae_mixfit_workspace_bytes(int64_t N, int L, int K, uint64_t* bytes);
int gmvae_mixfit_assign(const float* codes, int64_t N, int L, int K, const float* logw, const float* mu, const float* sigma,
                        float* log_resp_out, float* lse_out, void* workspace, void* stream);
int gmvae_mixfit_run(const float* codes, int64_t N, int L, int K, float* logw, float* mu, float* sigma, float reg_covar,
                     int n_iter, float* loglik_history, float* counts_out, void* workspace, void* stream);

/* The same with FULL covariances: a K-component Gaussian mixture with one L x L covariance per component, fitted by EM on the
 * device (scikit-learn's GaussianMixture default, covariance_type = 'full'; gmvae_amd.mixfit.fit(covariance="full") / assign,
 * model.fit_latent_mixture(covariance="full") and run_eval's --mixture_covariance=full go through it).  The statement is
 * tests/mixfit_full_ref.py; the kernels are csrc/mixfit_full.hpp.
 * codes z [N][L], logw [K], mu [K][L], cov [K][L][L], log_resp_out [N][K], lse_out [N], loglik_history [n_iter], counts_out [K]:
 * fp32 in device memory; info_out [K]: int32.  Only the lower triangle of cov (diagonal included) is read.  A logw entry may be -inf.
 *   Factor, on the device in fp64, a workgroup per component: C_k = the lower Cholesky factor of that triangle, pivots
 *     p_j = a_jj - sum_{i<j} C_ji^2.  A pivot that is not > 0 (NaN included) gives info_k = j + 1 for the first such j (LAPACK's
 *     convention), else info_k = 0.  A component with info_k != 0 is absent from that E-step: l_nk = -inf for every n, exactly as a
 *     logw_k of -inf behaves, and no NaN anywhere else.  W_k = C_k^-1 and sum_d ln C_k,dd go to the workspace.
 *   E-step:  l_nk = logw_k - 1/2 |W_k (z_n - mu_k)|^2 - sum_d ln C_k,dd - (L/2) ln 2 pi, a triangular product in fp64;  lse, log r
 *     and r as in gmvae_mixfit_*.
 *   M-step, centred at the current mean (no sum r z z^T - mean mean^T form anywhere):  R_k = sum_n r_nk, S1_kd = sum_n r_nk
 *     (z_nd - mu_kd), S2_kde = sum_n r_nk (z_nd - mu_kd) (z_ne - mu_ke), all in fp64 (S2 on v_mfma_f64_16x16x4_f64, the blocks on or
 *     below the diagonal only);  R'_k = R_k + 10 * 2^-52, m = S1 / R', mu' = mu + m, cov'_kde = S2_kde / R' - m_d m_e, its diagonal
 *     max(., 0) + reg_covar, written to both triangles (bit-symmetric);  logw'_k = ln(R'_k / sum_j R'_j).  No component is
 *     special-cased: an empty or absent one keeps its mean and gets cov' = reg_covar I, so it is positive definite again in the
 *     next iteration.
 *   gmvae_mixfit_full_assign: factor and the E-step at the given parameters: log_resp_out, lse_out and info_out (each may be NULL);
 *     info_out = this call's info_k.  Two launches.
 *   gmvae_mixfit_full_run: n_iter iterations enqueued on `stream` with no host synchronisation, three launches each (factor, pass,
 *     update): iteration `it` factors, runs the E-step, records loglik_history [it] = 1/N sum_n lse_n (may be NULL), then applies
 *     the M-step to logw, mu and cov in place (rounded to fp32: the arrays are fp32).  counts_out (may be NULL) = R_k of the last
 *     iteration.  info_out (may be NULL): iteration 0 stores its info_k, a later iteration stores only over a 0 -- the caller sees a
 *     component's first failure and initialises nothing.  n_iter = 0 is a valid call that changes nothing.
 * Sizes: 1 <= N <= 2^24, 1 <= L <= 128 (one component's packed fp64 triangle is 66,048 bytes, and the factor kernel holds two in
 * the 160 KiB LDS), 1 <= K <= 256 and K L^2 <= 2^20; nothing needs to be a multiple of anything.
 * The workspace (gmvae_mixfit_full_workspace_bytes(N, L, K)), with P = L (L + 1) / 2, is
 *     8 (K P + K + G (K (P + L + 1) + 1)) bytes rounded up to 16:  W [K][P], sum ln C_dd [K], and for each of G row slices the partial
 *     sums S2 [K][P], S1 [K][L], R [K] and sum lse (all fp64), nothing per row;
 *     G = ceil(N / per), per = ceil(tiles / g) T, tiles = ceil(N / T), g = min(tiles, 256, floor(2^23 / (K (P + L + 1) + 1))),
 *     T = min(64, floor((163,840 - 8 (P + L)) / (8 ((L | 1) + (K | 1) + 3) + 4 (L | 1)))) rounded down to a multiple of 4 -- so at most
 *     256 slices and 64 MiB of partial sums.
 * It needs no initialisation, and every call leaves it free for the next.  The caller owns every other byte: no call writes
 * outside its non-NULL outputs, the parameters (run) and the workspace.
 * One owner per sum, fixed-order fp64 folds, no float atomics: two calls give the same bits, on any workspace contents.
 * Checks, before any launch, in this order: GMVAE_E_DIMS (N < 1, N > 2^24, L < 1, L > 128, K < 1, K > 256, K L^2 > 2^20, n_iter < 0,
 * reg_covar not finite and > 0); GMVAE_E_NULL (any pointer not marked "may be NULL"); GMVAE_E_ALIGN (float and int32 arrays 4
 * bytes, the workspace 16). */
int gmvae_mixfit_full_workspace_bytes(int64_t N, int L, int K, uint64_t* bytes);
int gmvae_mixfit_full_assign(const float* codes, int64_t N, int L, int K, const float* logw, const float* mu, const float* cov,
                             float* log_resp_out, float* lse_out, int32_t* info_out, void* workspace, void* stream);
int gmvae_mixfit_full_run(const float* codes, int64_t N, int L, int K, float* logw, float* mu, float* cov, float reg_covar,
                          int n_iter, float* loglik_history, float* counts_out, int32_t* info_out, void* workspace, void* stream);

/* Exact brute-force nearest neighbours of queries q [Nq][L] among references r [Nr][L] (fp32, device memory), the rank of given
 * candidates in the same order, and distance sums per class (model independent; gmvae_amd.neighbours -- knn, the k-NN classifier,
 * the silhouette, trustworthiness and continuity --, model.neighbour_scores and run_eval's --neighbour_scores go through it; the
 * reference has no counterpart).  The statement is tests/neigh_ref.py; the kernels are csrc/neigh.hpp.
 *   Distance: D_ij = sum_d (q_id - r_jd)^2 in the difference form, fp64 differences and sum (never |q|^2 + |r|^2 - 2 q.r, so never
 *     the matrix cores);  d_ij = D_ij rounded once to fp32;  a non-finite d_ij counts as +inf.
 *   Order: reference j precedes j' for query i when (d_ij, j) < (d_ij', j') lexicographically: ties in distance go to the smaller
 *     index.  A total order, so every result below is independent of tiling, slicing and of how the caller chunks the queries.
 *   Self: with self_offset >= 0 query i is reference row self_offset + i, which is left out of the order for that query; with
 *     self_offset = -1 nothing is left out.
 *   gmvae_knn_search: idx_out [Nq][k] (int32) and d2_out [Nq][k] (fp32) = the first k references in that order and their d,
 *     ascending; either may be NULL, not both.
 *   gmvae_knn_ranks: for candidates cand [Nq][m] (int32), rank_out [Nq][m] (int32) = the number of references (self left out) that
 *     strictly precede cand[i][t] in query i's order; a candidate equal to self or outside [0, Nr) gets -1.  search and ranks build
 *     d by the same device code: ranks(idx of search)[i][t] == t exactly.
 *   gmvae_knn_class_sums: for labels [Nr] (int32), sums_out [Nq][C] (fp64) = sum over {j: labels_j = c} of sqrt(D_ij): the fp64
 *     square root of the fp64 D, added in ascending j within slices of 1024 references, the slices in slice order.  A label outside
 *     [0, C) contributes nowhere (an unlabelled reference).  Self is not excluded: it contributes sqrt(0).
 * Sizes: 1 <= Nq <= 2^30, 1 <= Nr <= 2^24, 1 <= L <= 4096, 1 <= k, m <= 256, k <= Nr - (self_offset >= 0 ? 1 : 0), 1 <= C <= 256,
 * self_offset in {-1} or [0, Nr - Nq]; nothing needs to be a multiple of anything.
 * The workspace (gmvae_knn_workspace_bytes(Nq, Nr, L, k, C), which reads no device memory) holds d [Nq][Nr] or the class sums'
 * parts per slice, whichever is larger: it follows Nq Nr -- the caller chooses Nq per call and chunks a larger set of queries --,
 * needs no initialisation, and every call leaves it free for the next.  The caller owns every other byte: no call writes outside
 * its outputs and the workspace, and every index written is in [0, Nr) whatever the inputs hold, NaN included.
 * Everything is enqueued on `stream` with no host synchronisation.  One owner per output, integer counters, fixed-order fp64 folds,
 * no float atomics: two calls give the same bits.
 * Checks, before any launch, in this order: GMVAE_E_DIMS (the sizes above); GMVAE_E_NULL (any pointer not marked "may be NULL", or
 * both of search's outputs); GMVAE_E_ALIGN (float and int arrays 4 bytes, sums_out 8, the workspace 16). */
int gmvae_knn_workspace_bytes(int64_t Nq, int64_t Nr, int L, int k, int C, uint64_t* bytes);
int gmvae_knn_search(const float* q, int64_t Nq, const float* r, int64_t Nr, int L, int k, int64_t self_offset, int32_t* idx_out,
                     float* d2_out, void* workspace, void* stream);
int gmvae_knn_ranks(const float* q, int64_t Nq, const float* r, int64_t Nr, int L, int64_t self_offset, const int32_t* cand, int m,
                    int32_t* rank_out, void* workspace, void* stream);
int gmvae_knn_class_sums(const float* q, int64_t Nq, const float* r, int64_t Nr, int L, const int32_t* labels, int C,
                         double* sums_out, void* workspace, void* stream);

/* A linear probe: multinomial logistic regression with an l2 penalty fitted to codes x [N][L] (fp32, device memory) with labels
 * y [N] (int32), and its predictions (model independent; gmvae_amd.linprobe, model.linear_probe and run_eval's --linear_probe go
 * through it; the reference has no counterpart).  The statement is tests/linprobe_ref.py; the kernels are csrc/linprobe.hpp.
 *   Labels: a label outside [0, C) marks the row unlabelled -- weight 0 in the fit, left out of predict's sums.  n = the labelled
 *     rows, xbar = their mean (fp64).
 *   Model: p_n = softmax((x_n - xbar) W + b);  f(W, b) = -(1/n) sum_labelled ln p_n[y_n] + (l2 / 2) |W|_F^2  (the bias is free).
 *   Metric, built once: A = 1/2 (1/n) sum_labelled (x_n - xbar)(x_n - xbar)^T + l2 I in fp64 (Boehning's bound: the Hessian of f in
 *     W is <= I_C (x) A, in b <= 1/2 I; the centring decouples the two), its Cholesky factor, A^-1.
 *   gmvae_linprobe_fit: FISTA in that metric with unit steps, Theta_0 = V_0 = 0: at the extrapolated point V, G_W = (1/n) sum
 *     (x_n - xbar)^T (p_n - e_y) + l2 V_W and G_b = (1/n) sum (p_n - e_y); Theta' = (V_W - A^-1 G_W, V_b - 2 G_b); V' = Theta' +
 *     beta (Theta' - Theta), beta = (t - 1) / t', t' = (1 + sqrt(1 + 4 t^2)) / 2, t_0 = 1 (computed on the host in fp64, one per
 *     launch).  No line search, no stopping rule: 3 + 2 n_iter launches enqueued on `stream` with no host synchronisation.
 *     Outputs: W_out [L][C] and b_out [C] = b - xbar W, so that the UN-centred logits x W_out + b_out are the model's;
 *     loss_history [n_iter] (may be NULL), entry it = f at the point iteration it evaluated; grad_max_out [1] (may be NULL) = max
 *     |G| at the last evaluated point (NaN if n_iter = 0); info_out [1] (int32, may be NULL) = 0, j + 1 for the first pivot j of
 *     the factorisation that is not > 0, or -1 if no row is labelled -- W_out and b_out are then 0 and the history NaN.
 *   gmvae_linprobe_predict: log_prob_out [N][C] = ln softmax(x W + b) and pred_out [N] (int32) = its FIRST maximal index (either
 *     may be NULL); with labels (may be NULL) sums_out [3] (fp64, may be NULL) = the labelled rows, those with pred = y, and sum
 *     -ln p[y] over them (all 0 without labels).
 * Arithmetic: the logits are fp64 sums of exact products of fp32 numbers (V_W rounded to fp32 for the pass), the exponentials fp32,
 * every sum over rows and the whole update fp64.  One owner per sum, fixed-order folds, no float atomics: two calls give the same bits.
 * Sizes: 1 <= N <= 2^24, 1 <= L <= 128, 2 <= C <= 256, C L <= 16,384, n_iter >= 0, l2 finite and > 0.
 * The workspace (gmvae_linprobe_workspace_bytes(N, L, C), which reads no device memory) holds xbar, A^-1, Theta, V and the
 * workgroups' partial sums (at most 256 row slices', nothing per row); it needs no initialisation, and fit and predict may share it
 * one after the other.
 * Checks, before any launch, in this order: GMVAE_E_DIMS (the sizes above); GMVAE_E_NULL (any pointer not marked "may be NULL");
 * GMVAE_E_ALIGN (float and int32 arrays 4 bytes, sums_out 8, the workspace 16). */
int gmvae_linprobe_workspace_bytes(int64_t N, int L, int C, uint64_t* bytes);
int gmvae_linprobe_fit(const float* codes, const int32_t* labels, int64_t N, int L, int C, double l2, int n_iter, float* W_out,
                       float* b_out, float* loss_history, float* grad_max_out, int32_t* info_out, void* workspace, void* stream);
int gmvae_linprobe_predict(const float* codes, const int32_t* labels, int64_t N, int L, int C, const float* W, const float* b,
                           float* log_prob_out, int32_t* pred_out, double* sums_out, void* workspace, void* stream);

/* The kernel two-sample test (Gretton et al. 2012): the unbiased MMD^2 between two samples for P splits of one pooled sample
 * z [N][D] (fp32, device memory) -- split 0 the observed one, the others the permutation null (model independent;
 * gmvae_amd.twosample, model.sample_test and run_eval's --sample_test go through it; the reference has no counterpart).  The
 * statement is tests/twosample_ref.py; the kernels are csrc/twosample.hpp.
 *   Splits: assign [P][N] (uint8, device memory), non-zero where the point belongs to the first sample; n_p = the non-zero entries
 *     of row p and m_p = N - n_p are counted on the device, so the rows may differ in size.
 *   Distance: d2_ij = sum_d (z_id - z_jd)^2 in fp64.  GMVAE_MMD_ENERGY: from differences, each taken and squared in fp64 and added
 *     in ascending d.  GMVAE_MMD_RBF: the kernel is translation invariant, so from the expanded square |zc_i|^2 + |zc_j|^2 -
 *     2 zc_i . zc_j on the rows centred by the pooled mean, all fp64, clamped at 0 (tests/test_twosample_cpu.py: the two forms
 *     differ by 3e-6 of the test's gate on its cases).
 *   Kernel: GMVAE_MMD_RBF: k = (1/Q) sum_q exp(-gamma[q] d2), 1 <= Q <= 8, gamma [Q] (fp64, HOST memory, read before the
 *     launches; finite and >= 0), the exponential fp64.  GMVAE_MMD_ENERGY: k = -sqrt(d2) -- MMD^2 is then the energy distance --,
 *     gamma and Q ignored (gamma may be NULL); two equal rows give exactly k = 0.
 *   Statistic: K0 = K with a zero diagonal, e = row p of assign as 0 / 1; a = e^T K0 e, b = e^T K0 1, c = 1^T K0 1 (fp64);
 *     mmd2 [P] (fp64): mmd2[p] = a / (n (n - 1)) + (c - 2 b + a) / (m (m - 1)) - 2 (b - a) / (n m), NaN where n < 2 or m < 2.
 *   Rows of split 0: row_all [N] = K0 1 and row_first [N] = K0 e_0 (fp64; either may be NULL): the witness function's sums.
 * Nothing of size N^2 is stored: the workspace (gmvae_mmd_workspace_bytes(N, D, P), which reads no device memory) holds the
 * workgroups' partial sums of a and b -- ceil(N / 32) row tiles times at most 16 column slabs, P doubles each --, 2 N doubles
 * per slab for the two row outputs and, for the rbf kernel's centring, at most 65 D + N doubles; it needs no initialisation.  Two
 * launches (energy) or five (rbf: the mean in two, the norms, the tiles, the finish) enqueued on `stream` with no host
 * synchronisation.
 * One owner per output, fixed-order fp64 sums (the order follows from N alone), no float atomics: two calls give the same bits, and
 * mmd2[p] does not depend on which other splits the call holds.
 * Sizes: 2 <= N <= 2^20, 1 <= D <= 4096, 1 <= P <= 4096.
 * Checks, before any launch, in this order: GMVAE_E_DIMS (the sizes above); GMVAE_E_MODEL (the kernel kind); GMVAE_E_DIMS (Q, a
 * gamma that is negative or not finite) and GMVAE_E_NULL (gamma) under GMVAE_MMD_RBF; GMVAE_E_NULL (z, assign, mmd2, workspace);
 * GMVAE_E_ALIGN (z 4 bytes, the fp64 outputs 8, the workspace 16). */
#define GMVAE_MMD_RBF 0
#define GMVAE_MMD_ENERGY 1
int gmvae_mmd_workspace_bytes(int N, int D, int P, uint64_t* bytes);
int gmvae_mmd(const float* z, int N, int D, const uint8_t* assign, int P, int kernel, const double* gamma, int Q, double* mmd2,
              double* row_all, double* row_first, void* workspace, void* stream);

/* The debiased Sinkhorn divergence (Genevay et al. 2018; Feydy et al. 2019) between two weighted samples x [n][D] and y [m][D]
 * (fp32, device memory) under the cost C(u, v) = 1/2 |u - v|^2: a transport distance in the data's own units, next to gmvae_mmd's
 * verdict (model independent; gmvae_amd.sinkhorn, model.sample_distance and run_eval's --sample_distance go through it; the
 * reference has no counterpart).  The statement is tests/sinkhorn_ref.py; the kernels are csrc/sinkhorn.hpp.
 *   Weights: a [n], b [m] (fp64, device memory), positive; either may be NULL: uniform.  log a - log sum a is taken in fp64 on the
 *     device, and the outputs' weighted sums divide by sum a, so the weights need not be normalised to the last bit.
 *   Schedule: eps_dev [n_iter + 1] (fp64, DEVICE memory, read by the kernels; positive, not checked): the temperature of iteration
 *     t < n_iter and, last, of the final pass.
 *   Cost: from the expanded square (|zc_i|^2 + |zc_j|^2) / 2 - zc_i . zc_j on the rows centred by the mean of the pooled sample, all
 *     fp64, clamped at 0 (tests/test_sinkhorn_cpu.py measures the form against differences in longdouble); C_ii = 0 exactly where a
 *     sample is compared with itself.
 *   Softmin: softmin_e(pts, h, w)(u) = -e log sum_j w_j exp((h_j - C(u, pts_j)) / e), the exponential fp64, a running (max, sum) per
 *     row.
 *   Iteration: f, g, p, q start at 0.  For t < n_iter, e = eps_dev[t]: f <- softmin(y, g, b) at x, p <- (p + softmin(x, p, a) at x) /
 *     2, q <- (q + softmin(y, q, b) at y) / 2; then g <- softmin(x, f, a) at y with the new f, and p and q averaged once more.  Last
 *     pass at e = eps_dev[n_iter]: f' = softmin(y, g, b) at x, p' = softmin(x, p, a) at x, q' = softmin(y, q, b) at y, not averaged.
 *   Outputs (fp64, device memory): f [n] = f', g [m], p [n] = p', q [m] = q'; out [4] = (S, part_x, part_y, marginal_err) with
 *     part_x = <a, f' - p'>, part_y = <b, g - q'>, S = part_x + part_y and marginal_err = max_i |expm1((f_i - f'_i) / eps_dev[n_iter])|,
 *     the relative error of the transport plan's row marginals (the column marginals are exact after the second half-step): the
 *     convergence readout.  S is not converged unless marginal_err is small, and it has no zero point at finite n.
 * Nothing of size n m is stored: the workspace (gmvae_sinkhorn_workspace_bytes(n, m, D), which reads no device memory) holds a
 * (max, sum) pair per row, problem and column slab -- at most 2 * 3 * 16 max(n, m) doubles --, 3 (n + m) doubles per row and at most
 * 65 D for the mean; it needs no initialisation.  Four set-up launches, two per half-step (the half-step's three softmins are the
 * problems of one launch) and one at the end, enqueued on `stream` with no host synchronisation.
 * One owner per output, fixed-order fp64 sums (the order follows from n and m alone), no float atomics: two calls give the same bits.
 * Sizes: 1 <= n, m <= 2^20, 1 <= D <= 4096, 1 <= n_iter <= 100000.
 * Checks, before any launch, in this order: GMVAE_E_DIMS (the sizes above); GMVAE_E_NULL (x, y, eps_dev, f, g, p, q, out,
 * workspace); GMVAE_E_ALIGN (x and y 4 bytes, every fp64 array 8, the workspace 16). */
int gmvae_sinkhorn_workspace_bytes(int64_t n, int64_t m, int D, uint64_t* bytes);
int gmvae_sinkhorn(const float* x, int64_t n, const float* y, int64_t m, int D, const double* a /* [n], nullable = uniform */,
                   const double* b /* [m], nullable = uniform */, const double* eps_dev /* [n_iter + 1], device */, int n_iter,
                   double* f, double* g, double* p, double* q, double* out /* [4]: S, part_x, part_y, marginal_err */,
                   void* workspace, void* stream);

/* Principal component analysis of N rows x [N][D] (fp32, device memory), and the small dense symmetric eigensolver under it (model
 * independent; gmvae_amd.pca, model.latent_pca, tsne.embed(init="pca") and run_eval's --latent_pca, --pca_baseline, --sample_frechet
 * and --tsne_init go through it; the reference has no counterpart).  The statement is tests/pca_ref.py; the kernels are
 * csrc/pca.hpp.
 *   mu = (1/N) sum_n x_n and C = (1/(N - 1)) sum_n (x_n - mu)(x_n - mu)^T in fp64, every row centred BEFORE the product (never the
 *     expanded square), on the fp64 MFMA; C stays in the workspace.
 *   gmvae_sym_eigh: A [n][n] (fp64, symmetric; the lower triangle is read), n <= 128 -> w_out [n] descending (ties by original index)
 *     and V_out [n][n] with the eigenvectors in its COLUMNS, each signed so that its entry of largest magnitude (the first such
 *     index) is positive; offdiag_out [1] (may be NULL) = max |off-diagonal| / max |diagonal| of the rotated matrix, the convergence
 *     readout (0 where the diagonal is 0).  Cyclic Jacobi in one workgroup, round-robin ordering, EXACTLY n_sweeps sweeps; its
 *     workspace is n n doubles.
 *   gmvae_pca_fit: D <= 128 (then m = D): the solver on C; components_out [k][D] = the first k eigenvectors as rows, variance_out
 *     [k] their eigenvalues, residual_out [k] = 0.  D > 128: subspace iteration on the stored C (no further pass over x) from V0
 *     [D][m] (fp64, orthonormal columns, device memory): n_iter times W = C V, G = W^T W = R R^T, V = W R^-T; then W = C V, T = 1/2
 *     (V^T W + W^T V) = Q diag(theta) Q^T by the solver; components = the first k columns of V Q (signed as above), variance =
 *     theta, residual_j = |W q_j - theta_j V q_j|_2: the result is converged only as far as residual says.  mean_out [D]; stats_out
 *     [4] = tr C, the solver's offdiag, N, reserved (0); info_out [1] (int32, may be NULL) = 0, or 1 + the index of the first
 *     pivot of a factorisation of G that is not > 0 (the data's rank is below m): every output is then NaN except mean_out,
 *     stats_out[0] and stats_out[2].  At most 6 launches for D <= 128 and 10 + 3 n_iter and one copy for D > 128, none synchronising
 *     with the host.
 *   gmvae_pca_transform: z_out [N][k] (fp32) = ((x - mean) . components^T) . scale (scale [k] may be NULL = 1): every product an fp64
 *     product of an fp64-centred value, the sums fp64 in ascending d, rounded once.  Needs no workspace.
 * One owner per sum, fixed-order fp64 folds, no float atomics: two calls give the same bits.
 * Sizes: 2 <= N <= 2^24 (transform: 1 <= N), 1 <= D <= 4096, 1 <= k <= m <= min(D, 128), m = D where D <= 128, n_iter >= 0,
 * n_sweeps >= 1.  The workspace (gmvae_pca_workspace_bytes(N, D, m), which reads no device memory) needs no initialisation.
 * Checks, before any launch, in this order: GMVAE_E_DIMS (the sizes above); GMVAE_E_NULL (any pointer not marked "may be NULL"; V0
 * may be NULL where D <= 128); GMVAE_E_ALIGN (x and z_out 4 bytes, every fp64 array 8, the workspace 16). */
int gmvae_pca_workspace_bytes(int64_t N, int D, int m, uint64_t* bytes);
int gmvae_pca_fit(const float* x, int64_t N, int D, int k, int m, int n_iter, int n_sweeps, const double* V0, double* mean_out,
                  double* components_out, double* variance_out, double* residual_out, double* stats_out, int32_t* info_out,
                  void* workspace, void* stream);
int gmvae_pca_transform(const float* x, int64_t N, int D, int k, const double* mean, const double* components, const double* scale,
                        float* z_out, void* stream);
int gmvae_sym_eigh(const double* A, int n, int n_sweeps, double* w_out, double* V_out, double* offdiag_out, void* workspace,
                   void* stream);

/* log p(x) by annealed importance sampling (AIS) with Hamiltonian Monte Carlo transitions (Neal 2001; Wu, Burda, Salakhutdinov &
 * Grosse 2017): the generative model alone, so -- unlike gmvae_iw_bound* -- its gap does not depend on the inference network, and
 * it tightens towards log p(x) as n_temps grows (Engine.ais_bound, model.ais_bound and run_gmvae --mode=eval --ais_chains go
 * through it; the reference has no counterpart).  The statement is tests/ais_ref.py; the kernels are csrc/ais.hpp.
 *   Prior: p(z) = sum_k pi_k N(z; mu_k, diag sigma_k^2), built from `params` by a prep launch -- VAE: one standard normal;
 *     VAE_GMP: loc, softplus(raw_scale_diag), log_softmax(mixture_logits); GMVAE: pi_k = 1 / K, (mu_k, sigma_k) = prior_gmm's
 *     normal head at e_k (sigma_min, raw_sigma_bias as gmvae_forward).  So for the GMVAE the estimate is of log p(x) ITSELF, the
 *     uniform p(y) inside: gmvae_iw_bound_enum_y's bound minus ln K.
 *   Base r_b: base == NULL, base_K == 0: the prior.  Else the caller's table, one record of base_K (1 + 2 L) floats per example:
 *     ln w [base_K], mu [base_K][L], sigma [base_K][L] (sigma > 0; the inference mixture sum_k q(k|x_b) q(z|x_b,e_k), one
 *     Gaussian for the VAE family).
 *   Likelihood: gmvae_forward's Bernoulli term on x in {0, 1} -- the decoder MLP at dims' sizes, gen_bias_init / gen_bias_vec, any
 *     hidden_act, the activation's derivative taken from the activation (ReLU' = 0 at a pre-activation <= 0).
 *   Path: betas_dev, n_temps + 1 floats on the device, 0 = beta_0 < ... < beta_T = 1 (not checked; beta_0 is taken as 0),
 *     f_t = r^(1 - beta_t) (p p(x|.))^beta_t; with the prior as the base it is p(z) p(x|z)^beta_t, the prior evaluated once.
 *   Chain (b, c), c < n_chains: at t = 0 a component of the base by inverse CDF of its weights with one uniform, z_0 = mu_k +
 *     sigma_k eps.  At t = 1 .. T: log w += (beta_t - beta_{t-1}) (log p(z) + log p(x|z) - log r(z)) at z_{t-1}; then one HMC
 *     transition on f_t -- a fresh momentum ~ N(0, I), n_leapfrog leapfrog steps of size e (half step, full steps, half step on
 *     the momentum), H = -log f_t(z) + |p|^2 / 2, accepted iff ln u < H_old - H_new, a non-finite H_new rejects --; then
 *     e <- clip(e * (accepted ? step_up : step_down), 1e-4, 1), e = step0 at the start, per chain.  step_up = step_down = 1 turns
 *     the adaptation off: that is the strictly valid AIS (an adapted step size depends on the chain's past).  The transition at
 *     beta_T is run; z_T is an approximate posterior sample.
 *   Noise: chain (b, c) is Philox row (dims->row0 + b) n_chains + c, and its draw at transition t (t = 0: the start) is what
 *     gmvae_noise_fill(eps, u, rows, L, 1, row_base, seed, step (n_temps + 1) + t) returns: eps = z_0's noise or the momentum,
 *     u[0] = the component's or the accept's uniform.  eps [n_temps + 1][B n_chains][L] and u [n_temps + 1][B n_chains] (each
 *     may be NULL: Philox) replace the draw.  Results do not depend on the batch, the sharding or the launches.
 *   Outputs (each may be NULL but tail): logw_out [B][n_chains]; bound_out [B] = logsumexp_c log w_bc - ln n_chains;
 *     stats_out [B][4] = the bound, the effective sample size (sum w)^2 / sum w^2 of the chains' weights, the mean acceptance rate,
 *     the mean final step size; z_out [B n_chains][L] = z_T; tail [GMVAE_TAIL] = the sums over b of -bound, ESS, acceptance rate
 *     and step size, [4] = B, [5..7] = 0.
 * One workgroup owns 16 chains for every temperature of a launch (a panel may span examples and be ragged at the end); the layer
 * products run on the fp32 matrix cores, element-wise work in fp32, the sums over D and L and H itself in fp64.  The call
 * enqueues the prep launch, launches of at most 32 transitions each (GMVAE_AIS_LAUNCH_TEMPS in the environment sets another cap;
 * the chain state is carried in the workspace, and the result does not depend on the cap), and two finishing launches, with no
 * host synchronisation.  The workspace (gmvae_ais_workspace_bytes at the same dims, base_K and n_chains; 256-byte aligned; needs
 * no initialisation) is O(B n_chains L), independent of n_temps; after the call its first B n_chains 64-bit words hold the chains'
 * accept records, bit t - 1 of word b n_chains + c set iff transition t <= 64 of chain (b, c) was accepted.  No workgroup waits for another, no atomics, fixed-order sums:
 * two calls give the same bits.
 * Sizes: n_hidden <= 3, hidden widths <= 512, L <= 128, K <= 64 (VAE: K is ignored), base_K <= 64, any D >= 1, B n_chains <= 2^30.
 * Checks, before any launch, in this order: GMVAE_E_NULL (dims); GMVAE_E_MODEL; GMVAE_E_DIMS (the sizes above; any GMVAE_LIK_*
 * field other than the Bernoulli, GMVAE_X_F32, GMVAE_LIK_SCALE_LEARNED or GMVAE_OBJ_PIXEL_MASK in dims->sched_flags -- the other
 * bits are ignored --; n_temps, n_chains or n_leapfrog < 1; (row0 + B) n_chains >= 2^38; a step size or factor that is not
 * positive and finite; base without base_K); GMVAE_E_NULL (x, params, betas_dev, tail, workspace, base with base_K > 0);
 * GMVAE_E_ALIGN (params 16 bytes, the workspace 256, every other array 4). */
int gmvae_ais_workspace_bytes(const GmvaeDims* dims, int model, int base_K, int n_chains, uint64_t* bytes);
int gmvae_ais(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, const float* base, int base_K,
              const float* betas_dev, int n_temps, int n_chains, int n_leapfrog, float step0, float step_up, float step_down,
              const float* eps, const float* u, float* logw_out, float* bound_out, float* stats_out, float* z_out, float* tail,
              void* workspace, uint64_t seed, uint64_t step, void* stream);

/* Bidirectional Monte Carlo (Grosse, Ghahramani & Adams 2015; the validation of Wu, Burda, Salakhutdinov & Grosse 2017): an UPPER
 * bound on log p(x) beside gmvae_ais's lower one, on data the model itself generates.  gmvae_simulate draws (z*, x) ~ p(z) p(x|z),
 * so z* is an exact posterior sample for x; gmvae_ais_reverse runs gmvae_ais's chain backwards from z*, beta = 1 down to 0.  The
 * reversal of a Metropolis-corrected HMC kernel is the kernel itself, and the ratio of the reverse to the forward path density is
 * w Z_0 / Z_T, so the reverse weights have E[w_rev] = 1 / p(x): -(logsumexp_c log w_rev - ln n_chains) bounds log p(x) from above in
 * expectation.  The two bounds bracket log p(x), and their difference bounds the bias of gmvae_ais at these settings ON DATA
 * DISTRIBUTED AS THE MODEL'S OWN SAMPLES; for a real x there is no exact posterior sample and so no upper bound.
 * (Engine.simulate, Engine.ais_bound_reverse, Engine.bdmc_gap, model.bdmc_gap and run_gmvae --mode=eval --bdmc_examples go through
 * them; the reference has no counterpart.)  The statement is tests/bdmc_ref.py; the kernels are csrc/bdmc.hpp.
 *
 * gmvae_simulate, example b < dims->B: a component k of the prior table (gmvae_ais's) by inverse CDF of its weights with one
 *   uniform; z* = mu_k + sigma_k eps; lambda = decoder(z*) + gen_bias_init / gen_bias_vec (any hidden_act); x_d = [u_d <
 *   sigmoid(lambda_d)].  Outputs: z_out [B][L]; k_out [B] (for the GMVAE this is y); x_out [B][D] bytes 0 / 1; prob_out [B][D] =
 *   sigmoid(lambda) (may be NULL).
 *   Noise: example b is Philox row dims->row0 + b; eps and the component's uniform are what gmvae_noise_fill(eps, u, B, L, 1, row0,
 *   seed, 2 step) returns, the pixel uniforms the u of gmvae_noise_fill(NULL, u, B, 1, D, row0, seed, 2 step + 1).  eps [B][L],
 *   u [B] and ux [B][D] (each may be NULL: Philox) replace the draws.
 *   The workspace (gmvae_simulate_workspace_bytes; 256-byte aligned; needs no initialisation) holds the prior table.  Two
 *   launches, no host synchronisation; one workgroup owns 16 examples.
 *   Checks, before any launch, in this order: gmvae_ais's GMVAE_E_NULL (dims), GMVAE_E_MODEL and GMVAE_E_DIMS on the sizes, the
 *   likelihood and mask bits and row0 + B < 2^38; GMVAE_E_NULL (params, z_out, k_out, x_out, workspace); GMVAE_E_ALIGN (params 16
 *   bytes, the workspace 256, every other array 4 -- x_out included).
 *
 * gmvae_ais_reverse: gmvae_ais's arguments, sizes, gates, workspace layout and guarantees, with z_start [B][L] after base_K.
 *   Chain (b, c) starts at z_T = z_start[b] -- all n_chains chains of an example from the one exact sample.  For t = T .. 1: first
 *   one HMC transition on f_t from the current point, exactly gmvae_ais's (fresh momentum, n_leapfrog leapfrog steps, H in fp64,
 *   accepted iff ln u < H_old - H_new, a non-finite H_new rejects, the same step-size update and clip); then
 *   log w_rev -= (beta_t - beta_{t-1}) (log p(z) + log p(x|z) - log r(z)) at the NEW point z_{t-1}.
 *   Noise: chain (b, c) is Philox row (dims->row0 + b) n_chains + c at step (n_temps + 1) + t for transition t, exactly as
 *   gmvae_ais keys it (index 0 is unused): a caller that runs both directions separates them by `step` or `seed`.  eps
 *   [n_temps + 1][B n_chains][L] and u [n_temps + 1][B n_chains] have gmvae_ais's layout, slot 0 ignored.
 *   Outputs (each may be NULL but tail): logw_out = log w_rev; bound_out [B] = -(logsumexp_c log w_rev - ln n_chains), the upper
 *   bound; stats_out [B][4] = that bound, the effective sample size of the reverse weights, the mean acceptance rate, the mean
 *   final step size; z_out = z_0; tail = the sums over b laid out as gmvae_ais's, with ITS sign convention in slot 0: [0] = the
 *   sum of -bound (here sum_b logsumexp_c log w_rev - ln n_chains), [1..3] the sums of ESS, acceptance rate and step size,
 *   [4] = B, [5..7] = 0.  The accept record is gmvae_ais's: bit t - 1 of the chain's word for transition t <= 64.
 *   Launches hold at most 32 transitions, descending in t (GMVAE_AIS_LAUNCH_TEMPS sets another cap; the result does not depend on
 *   it).  Checks: gmvae_ais's, in its order, with z_start added to the GMVAE_E_NULL and the 4-byte GMVAE_E_ALIGN checks. */
int gmvae_simulate_workspace_bytes(const GmvaeDims* dims, int model, uint64_t* bytes);
int gmvae_simulate(const GmvaeDims* dims, int model, const float* params, const float* eps, const float* u, const float* ux,
                   float* z_out, int32_t* k_out, uint8_t* x_out, float* prob_out, void* workspace, uint64_t seed, uint64_t step,
                   void* stream);
int gmvae_ais_reverse_workspace_bytes(const GmvaeDims* dims, int model, int base_K, int n_chains, uint64_t* bytes);
int gmvae_ais_reverse(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, const float* base, int base_K,
                      const float* z_start, const float* betas_dev, int n_temps, int n_chains, int n_leapfrog, float step0,
                      float step_up, float step_down, const float* eps, const float* u, float* logw_out, float* bound_out,
                      float* stats_out, float* z_out, float* tail, void* workspace, uint64_t seed, uint64_t step, void* stream);

/* Per-example refinement of q(z|x): the two parts of the inference gap log p(x) - L[q(z|x)] (Cremer, Li & Duvenaud 2018).  For each
 * example a local Gaussian q_phi(z) = N(m, diag e^{2 s}) starts at the caller's (mu_0, sigma_0) and climbs the example's own ELBO by
 * stochastic gradient ascent; the ELBO and the importance-weighted bound of the start and of the refined phi* are then evaluated on
 * common noise.  L[phi*] - L[q(z|x)] is the amortisation gap, log p(x) - L[phi*] the approximation gap (Engine.refine_posterior,
 * model.inference_gaps and run_gmvae --mode=eval --refine_steps go through it; the reference has no counterpart).  The statement
 * is tests/refine_ref.py; the kernels are csrc/refine.hpp, the evaluation csrc/ais.hpp's, the host side csrc/ais.hip.
 *   Target: log p(x, z) = log p(z) + log p(x|z), prior and likelihood exactly as gmvae_ais takes them (y summed out for the GMVAE).
 *   Start: start [B][2 L] = mu_0 [L], sigma_0 [L] per example (sigma_0 > 0), s_0 = ln sigma_0.
 *   Step t = 1 .. n_steps, n_samples = S draws eps_s: z_s = m + e^s eps_s, g_s = grad_z log p(x, z_s);
 *     L-hat_t = 1/S sum_s log p(x, z_s) + sum_l s_l + L/2 (1 + ln 2 pi);  dm = 1/S sum_s g_s;  ds = 1/S sum_s g_s e^s eps_s + 1;
 *     then one ASCENT step of adam_tf_step's update on the 2 L parameters (lr, beta1, beta2, adam_eps, the example's own count;
 *     alpha_t from fp64 pow), and s clamped to [-20, 5].  An example whose gradient is not finite, or has an element of 2^63.5
 *     (1.3e19) or more in magnitude -- its square is at the edge of fp32, and the update's second moment would become inf --,
 *     skips that update: moments and count untouched.
 *   Evaluation: n_eval_rounds rounds of S fresh draws, N = n_eval_rounds S; log w = log p(x, z) - log q_phi(z) at phi* and at phi_0
 *     on the SAME eps; the ELBO = mean log w, the importance-weighted bound = logsumexp log w - ln N, sums in fp64.
 *   Noise: row (b, s) is Philox row (dims->row0 + b) S + s, and its draw at t (steps 0 .. n_steps - 1, then the rounds) is what
 *     gmvae_noise_fill(eps, NULL-able u, rows, L, 1, row_base, seed, step (n_steps + n_eval_rounds + 1) + t) returns.
 *     eps [n_steps + n_eval_rounds][B S][L] (may be NULL: Philox) replaces the draw.  Results do not depend on the batch, the
 *     sharding or the launches.
 *   Outputs (each may be NULL but tail): phi_out [B][2 L] = m*, sigma* = e^{s*}; trace_out [n_steps][B] = L-hat_t before the
 *     update of step t; stats_out [B][8] = elbo_start, elbo_refined, iw_start, iw_refined, the effective sample size of the N
 *     weights at phi*, updates applied, mean_l |m* - mu_0| / sigma_0, mean_l ln(sigma* / sigma_0); tail [GMVAE_TAIL] = the sums
 *     over b of the first four, [4] = B, [5..7] = 0.  n_steps = 0 is legal: phi* = phi_0.
 * One workgroup owns 16 rows (samples) for every step of a launch; an example's S samples lie in one panel and its first row owns
 * the optimizer state.  The call enqueues the prior's prep launch, launches of at most 256 steps or rounds each
 * (GMVAE_REFINE_LAUNCH_STEPS in the environment sets another cap; the state is carried in the workspace, and the result does not
 * depend on the cap), and two finishing launches, with no host synchronisation.  The workspace (gmvae_refine_workspace_bytes at
 * the same dims and n_samples; 256-byte aligned; needs no initialisation) is O(B (L + S)), independent of n_steps.  No workgroup
 * waits for another, no atomics, fixed-order sums: two calls give the same bits.
 * Sizes: those of gmvae_ais (n_hidden <= 3, widths <= 512, L <= 128, K <= 64, any D >= 1), B S <= 2^30.
 * Checks, before any launch, in this order: GMVAE_E_NULL (dims); GMVAE_E_MODEL; GMVAE_E_DIMS (the sizes above; the likelihood and
 * mask bits gmvae_ais refuses; n_samples not in {1, 2, 4, 8, 16}; n_steps < 0; n_eval_rounds < 1; n_steps + n_eval_rounds > 2^24;
 * (row0 + B) S >= 2^38; lr not positive and finite; beta1 or beta2 outside [0, 1); adam_eps negative or not finite);
 * GMVAE_E_NULL (x, params, start, tail, workspace); GMVAE_E_ALIGN (params 16 bytes, the workspace 256, every other array 4). */
int gmvae_refine_workspace_bytes(const GmvaeDims* dims, int model, int n_samples, uint64_t* bytes);
int gmvae_refine(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, const float* start, int n_steps,
                 int n_samples, int n_eval_rounds, float lr, float beta1, float beta2, float adam_eps, const float* eps,
                 float* phi_out, float* trace_out, float* stats_out, float* tail, void* workspace, uint64_t seed, uint64_t step,
                 void* stream);

/* tf.compat.v1.train.AdamOptimizer.apply_gradients (scripts/runners.py:181-183):
 * epsilon is added to the UN-corrected sqrt(v).  t = 1-based step count.
 * t_dev (may be NULL): device pointer overriding t (graph replay).
 * g = grads[i] * grad_scale.  grad_scale_dev (may be NULL): device pointer to
 * a count; when given, grad_scale = 1 / (*grad_scale_dev) overrides.
 * loss_sum_dev (may be NULL): device pointer to the step's loss sum (tail[0] of the gradient buffer).  When it
 * holds a non-finite value -- a hand-off of the fused schedule timed out and poisoned the step, on this or (after
 * the all-reduce) on any rank -- the update is SKIPPED: params, m and v keep their values (the step counter still
 * advances; the caller sees the NaN loss and the workspace error word). */
int adam_tf_step(float* params, float* m, float* v, const float* grads, uint64_t P, float lr, float beta1,
                 float beta2, float epsilon, uint64_t t, const uint64_t* t_dev, float grad_scale,
                 const float* grad_scale_dev, const float* loss_sum_dev, void* stream);

/* GMVAE_OPT_CLIP_NORM's statement on a gradient buffer, for the eager path: grads [P + GMVAE_TAIL] (P a multiple of 4: P_padded)
 * holds gradient sums and the tail, clip_norm_dev one float C, rec_out float[4] receives the record (norm, d, clipped, guard),
 * scratch holds the fp64 partials (gmvae_grad_clip_scratch_bytes(P) bytes, 16-byte aligned).  Two launches on `stream`; then
 * adam_tf_step(..., grad_scale_dev = rec_out + 1, loss_sum_dev = rec_out + 3) applies the clipped update or skips it.
 * GMVAE_E_NULL; GMVAE_E_DIMS (P == 0 or P % 4); GMVAE_E_ALIGN (grads, scratch). */
int gmvae_grad_clip_scratch_bytes(uint64_t P, uint64_t* bytes);
int gmvae_grad_clip(const float* grads, uint64_t P, const float* clip_norm_dev, float* rec_out, void* scratch, void* stream);

/* One conditional network's MLP (scripts/base.py:66-67,133-135,196-198):
 * out[rows, out_dim] = MLP(concat(in, in2)) (+ gen_bias_init for the decoder).
 * `in` is uint8 when in_is_u8 else fp32.  in2 is y for ENCODER_GMM, else NULL.
 * The distribution heads (softplus, sigmoid, softmax) are applied by the
 * Python distribution objects on top of this. `B` in dims is ignored; rows is used. */
int gmvae_mlp_forward(const GmvaeDims* dims, int model, int net, const void* in, int in_is_u8,
                      const float* in2, int rows, const float* params, float* out, void* workspace,
                      void* stream);

/* Dynamic binarisation of the reference's input pipeline on the device (scripts/runners.py:44-47 `_preprocess`:
 * image = pixel / 255.; x = image < uniform -- note P[x = 1] = 1 - pixel/255 -- re-drawn on every pass).
 * pixels: uint8 [n_rows][D] resident in HBM (MNIST: 60000 x 784 = 47 MB); idx: int32 [B] source rows of this batch
 * (an epoch permutation kept on the device) or NULL for rows row0 .. row0+B-1; x_out: uint8 [B][D] of 0/1, the
 * layout gmvae_step takes.  The uniforms are Philox4x32-10 keyed by (seed, step or *step_dev) and the element's
 * position in the GLOBAL batch (row out_row0 + b, column), so a step is reproducible and a sharded batch draws what
 * the whole batch would (out_row0 = GmvaeDims::row0).  D % 4 == 0; pixels and x_out 4-byte aligned. */
int gmvae_binarize(const uint8_t* pixels, uint64_t n_rows, const int32_t* idx, uint64_t row0, int B, int D,
                   uint64_t seed, uint64_t step, const uint64_t* step_dev, uint8_t* x_out, uint64_t out_row0,
                   void* stream);

/* The noise gmvae_step draws when eps/u are NULL, as arrays: eps ~ N(0,1) [rows][L], u ~ U[tiny,1) [rows][K]
 * (either pointer may be NULL).  Philox4x32-10, counter = (global row row_base + r, quad of the row, stream, step or
 * *step_dev), key = seed: gmvae_step(dims, ..., seed, step) with dims->row0 = row_base and rows = B*S draws exactly
 * these values, in every schedule (tests feed them to the CPU oracle). */
int gmvae_noise_fill(float* eps, float* u, uint64_t rows, int L, int K, uint64_t row_base, uint64_t seed, uint64_t step,
                     const uint64_t* step_dev, void* stream);

/* utils.cluster_acc (scripts/utils.py:173-191) on device.  scratch: int32
 * [K*n_labels + B] (histogram, zeroed by the callee, then per-row argmax);
 * acc_out float[1].  Mode ties resolve to the smallest label. */
int gmvae_cluster_acc(const float* logits, const int64_t* labels, int B, int K, int n_labels,
                      int32_t* scratch, float* acc_out, void* stream);

/* ---- measurement / test hooks (not used by the reference-facing API) ---- */

/* One GEMM through the same grouped fp32-MFMA kernel the step uses.
 * cfg: tile configuration (0 small 32x32, 1 medium 64x64, 2 large 128x128, -1 auto); 4 / 5: the pre-split bf16-triple planes
 *      (5 reuses the planes of the previous cfg-4 call); 6 / 7: the f16-pair planes likewise; 8: the weight-stationary row
 *      kernels (NN K = 64; NT K = 128 with `bias` as a ReLU mask [M][N]; NT K = 512 or 640 = 512 + 128, N = 64, with `bias`
 *      as an addend [M][N]); shapes a form does not take are refused (GMVAE_E_DIMS).
 * trans 0 (NN): C[M,N] = act(A[M,K] W[K,N] + bias)
 * trans 1 (NT): C[M,N] = A[M,K] W[N,K]^T
 * trans 2 (TN): C[s][M(+1),N] = A[K,M]^T W[K,N] split over K into `splitk` slabs
 *               of (M+1)*N floats; bias != NULL requests the bias gradient
 *               (column sums of W over the slab's K range) at row M.
 * a_is_u8: A holds uint8. */
int gmvae_gemm_test(const void* A, int a_is_u8, const float* W, const float* bias, float* C, int M, int N,
                    int K, int trans, int relu, int cfg, int splitk, void* stream);

/* Runs the full step `iters` times with hipEvents around EVERY launch (on
 * `stream`) and returns, per launch ("level"), its name [48 chars each], mean
 * microseconds and the algorithmic FLOPs (2*M*N*K summed over its GEMMs,
 * 0 for row-local kernels).  Synchronises the stream: measurement only.
 * gmvae_train_profile does the same for the steady-state TRAINING step of a train graph (Philox noise, TF-Adam
 * fused into the last launch, first layer inside mega_fwd_bwd where that schedule applies): a three-step graph (an
 * untimed step, then two steps whose launches stamp the device wall clock per workgroup) replayed `iters` times, so
 * the kernels run back to back as in a train graph; it advances params / m / v / *step_dev like 3 * iters real steps.
 * usec = in-kernel span (last workgroup end - first workgroup start); usec_timeline (may be NULL) = the launch's share
 * of the step's timeline: first workgroup start of the NEXT launch - its own (dispatch and end-of-kernel write-back
 * included: the interval rocprofv3 --kernel-trace reports; the shares of a step's launches add up to the step). */
int gmvae_train_profile(const GmvaeDims* dims, int model, const uint8_t* x, float* params, float* m, float* v,
                        float* grads, void* workspace, uint64_t seed, uint64_t* step_dev, float lr, int iters,
                        int max_levels, int* n_levels, char* names, float* usec, float* usec_timeline, double* flops,
                        void* stream);
/* The data-parallel step's timeline (scripts/runners.py:231-232 has no counterpart: the reference is single-device; SURVEY.md
 * 8(e)): three consecutive steps of gmvae_dp_graph_create's graph (RCCL all-reduce node included) in ONE graph, replayed
 * `iters` times; the launches of steps 2 and 3 stamp the device wall clock.  out[5], microseconds, means: [0] in-kernel span of
 * a step's gradient launch(es); [1] their last workgroup's end -> first block of the Adam launch (the all-reduce window: the
 * RCCL node and the launch boundaries around it); [2] span of the Adam launch; [3] its end -> the next step's first workgroup;
 * [4] the step.  names / n_levels (may be NULL): the gradient launches' names.  COLLECTIVE over `comm`: same iters on every rank. */
int gmvae_dp_profile(const GmvaeDims* dims, int model, const uint8_t* x, float* params, float* m, float* v, float* grads,
                     void* workspace, uint64_t seed, uint64_t* step_dev, float lr, void* comm, int iters, float* out,
                     int max_levels, int* n_levels, char* names, void* stream);
/* The forward-only evaluation (gmvae_forward with in-kernel Philox noise; scripts/runners.py:324-333 reuses the model's loss
 * for the -log p(x) bound) timed: per launch with hipEvents (names / usec / flops as gmvae_step_profile), and *usec_total =
 * microseconds per forward when ONE captured forward is replayed `iters` times back to back. */
int gmvae_forward_profile(const GmvaeDims* dims, int model, const uint8_t* x, const float* params, float* tail, void* workspace,
                          uint64_t seed, int iters, int max_levels, int* n_levels, char* names, float* usec, double* flops,
                          float* usec_total, void* stream);
int gmvae_step_profile(const GmvaeDims* dims, int model, const uint8_t* x, const float* eps, const float* u,
                       const float* params, float* grads, void* workspace, uint64_t seed, int iters,
                       int max_levels, int* n_levels, char* names, float* usec, double* flops, void* stream);

/* `iters` full training steps (gmvae_step in Philox mode + adam_tf_step) issued from C on `stream` and
 * timed with hipEvents: mode 0 = eager launches, mode 1 = one hipGraph captured here and replayed.
 * Synchronises: measurement only. */
int gmvae_bench_loop(const GmvaeDims* dims, int model, const uint8_t* x, float* params, float* m, float* v,
                     float* grads, void* workspace, uint64_t* step_dev, int iters, int mode, float* usec_per_step,
                     void* stream);

/* One full training step -- Philox noise + gmvae_step + adam_tf_step(t = *step_dev, grad_scale =
 * 1/count from the tail) -- captured ONCE into a hipGraph owned by the library, for replay with a single
 * call per step (the sess.run([train_op, global_step]) of scripts/runners.py:231-232).  All pointers
 * are baked into the graph: copy each new batch into `x` before launching.
 * n_steps >= 1 consecutive steps go into the one graph; `x` then holds n_steps batches back to back
 * ([n_steps][B][D]: the next n_steps batches of the input pipeline).  One launch per n_steps steps amortises
 * the ~6 us the GPU idles between two graph launches (measured, profiles/): the kernels inside a graph run
 * back to back.
 * tail_log (may be NULL): fp32 [n_steps][GMVAE_TAIL]; step s of a launch also writes its tail (loss sums + count,
 * all-reduced in the data-parallel graph) to row s: the per-step losses the reference's logging and early-stopping
 * hooks see (scripts/runners.py:198-200,222-228), read once per launch instead of once per step. */
int gmvae_train_graph_create(const GmvaeDims* dims, int model, const uint8_t* x, int n_steps, float* params, float* m,
                             float* v, float* grads, void* workspace, uint64_t seed, uint64_t* step_dev, float lr,
                             float beta1, float beta2, float epsilon, float* tail_log, void** graph_out);
/* The same graph with the input pipeline inside: before each of its n_steps steps, gmvae_binarize draws that
 * step's batch from the resident uint8 `pixels` [n_rows][D] -- rows idx[s][0..B) of the int32 device buffer
 * idx [n_steps][B], which the caller refills (an epoch permutation) before every launch -- into x_scratch
 * [n_steps][B][D], with uniforms keyed by the device step counter: a new draw every step, nothing crosses PCIe. */
int gmvae_train_graph_create_pipeline(const GmvaeDims* dims, int model, const uint8_t* pixels, uint64_t n_rows,
                                      const int32_t* idx, uint8_t* x_scratch, int n_steps, float* params, float* m, float* v,
                                      float* grads, void* workspace, uint64_t seed, uint64_t* step_dev, float lr,
                                      float beta1, float beta2, float epsilon, float* tail_log, void** graph_out);
int gmvae_train_graph_launch(void* graph, void* stream);
int gmvae_train_graph_destroy(void* graph);

/* ---- data parallel over RCCL (no reference counterpart: the reference is single-device, scripts/runners.py:193).
 * RCCL is bound with dlopen(rccl_path or "librccl.so") at first use.  Rank 0 calls gmvae_comm_unique_id and
 * distributes the 128 bytes by any means (torch.distributed broadcast in gmvae_amd); every rank then calls
 * gmvae_comm_init.  gmvae_dp_step = gmvae_step (Philox mode) -> ONE all-reduce(SUM) of grads[P_padded + TAIL]
 * -> adam_tf_step with grad_scale = 1/tail[4], all enqueued on `stream`.  gmvae_dp_graph_create warms RCCL up
 * with one all-reduce of the (scratch) gradient buffer and changes no training state.
 * Return codes >= 1000 are 1000 + ncclResult_t. */
int gmvae_comm_unique_id(const char* rccl_path, char* out128);
/* gmvae_comm_init is BOUNDED: ncclCommInitRank runs on a helper thread and GMVAE_E_TIMEOUT comes back after
 * GMVAE_COMM_INIT_TIMEOUT seconds (environment, default 180) if some rank never joined -- the caller should then exit non-zero
 * (the helper thread stays inside RCCL).  gmvae_comm_count: the number of ranks the communicator actually spans (ncclCommCount). */
int gmvae_comm_init(const char* rccl_path, const char* id128, int rank, int world, void** comm);
int gmvae_comm_count(void* comm, int* nranks);
int gmvae_comm_destroy(void* comm);
int gmvae_dp_step(const GmvaeDims* dims, int model, const uint8_t* x, float* params, float* m, float* v,
                  float* grads, void* workspace, uint64_t seed, uint64_t* step_dev, float lr, float beta1,
                  float beta2, float epsilon, void* comm, void* stream);
int gmvae_dp_graph_create(const GmvaeDims* dims, int model, const uint8_t* x, int n_steps, float* params, float* m, float* v,
                          float* grads, void* workspace, uint64_t seed, uint64_t* step_dev, float lr, float beta1,
                          float beta2, float epsilon, void* comm, float* tail_log, void** graph_out);

/* Debugging aid: byte offset inside the workspace of a named intermediate ("hy1","hg1","hd1","y",
 * "logits","qp","pp","z","g","dqp","dpp","dlogits","dbuf0".."dbuf2","s1","s4", ...; "labels" and "sup_weight" under GMVAE_OBJ_LABELS; "obj_weights", "rwk" and "y_floor" under GMVAE_OBJ_WEIGHTS; "y_temperature" under GMVAE_Y_TEMP_DEV; "y_soft" under GMVAE_Y_STRAIGHT_THROUGH; "pixel_mask" under GMVAE_OBJ_PIXEL_MASK; "clip_norm" and "grad_clip" under GMVAE_OPT_CLIP_NORM; "lik_sigma" under GMVAE_LIK_GAUSSIAN without GMVAE_LIK_SCALE_LEARNED; "he<i>" / "hg<i>" / "hd<i>", i >= 1:
 * the kept input activation of layer i of the encoder (encoder_y for GMVAE) / encoder_gmm / decoder -- the parity
 * tests read the ReLU masks of a step from them). */
int gmvae_workspace_offset(const GmvaeDims* dims, int model, const char* name, uint64_t* byte_offset);

/* Debugging aid: device wall-clock stamps of the skinny schedule's launches ([10 launches][1024 blocks][8] uint64 at
 * 100 MHz).  host_out == NULL arms it (allocates the buffer; steps enqueued or captured afterwards stamp into it);
 * otherwise the buffer is copied to host_out.  tools/skstamps.py. */
int gmvae_debug_sk_stamps(unsigned long long* host_out);
/* Disarms it and frees the buffer.  Destroy every train graph captured while it was armed FIRST (their kernel arguments
 * hold the buffer's address). */
int gmvae_debug_sk_stamps_free(void);

/* Which schedule a TRAINING step of these sizes takes, as text (<= 47 chars + NUL into out48): "mega2", "mega", "skinny",
 * "fused" or "general", with "+marginal" appended under GMVAE_OBJ_MARGINAL_Y ("+marginal_iw" under
 * GMVAE_OBJ_MARGINAL_Y_IW), then "+labels" under GMVAE_OBJ_LABELS, "+weights" under GMVAE_OBJ_WEIGHTS, "+temp" under GMVAE_Y_TEMP_DEV, "+st" under GMVAE_Y_STRAIGHT_THROUGH, "+mask" under GMVAE_OBJ_PIXEL_MASK, "+grey" / "+cb" / "+gauss" under GMVAE_LIK_*, "+pois" / "+nb" under GMVAE_LIK_POISSON / GMVAE_LIK_NEG_BINOMIAL, "+f32" under GMVAE_X_F32, "+lsig" under GMVAE_LIK_SCALE_LEARNED, "+dreg" under GMVAE_GRAD_DREG, "+clip" under GMVAE_OPT_CLIP_NORM, and "+planes" appended where the top decoder layer's GEMMs run as bf16 piece products on pre-split
 * operands (gemm.hpp plane_rounds3).  Host-side, reads the same environment switches as the step.  bench.py prices its
 * roofline line with it. */
int gmvae_step_schedule(const GmvaeDims* dims, int model, char* out48);

/* Debugging aid: resident workgroups per CU the HIP runtime reports for a kernel of the library
 * (which: 0/1/2 = grouped GEMM small/medium/large configuration, 3 = mega_fwd_bwd, 4 = finalize_adam). */
int gmvae_kernel_occupancy(int which, int* blocks_per_cu);

#ifdef __cplusplus
}
#endif
#endif /* GMVAE_HIP_H_ */
