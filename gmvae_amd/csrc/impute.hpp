// gmvae_impute (include/gmvae_hip.h; the statement is tests/impute_ref.py): imputation of the missing pixels by self-normalised
// importance sampling on gmvae_iw_bound's weights (Mattei & Frellsen, MIWAE, 2019).  This header holds what the host path in
// gmvae_hip.hip (iw_run, kind IW_IMPUTE) and the kernels' translation unit (impute.hip) share: the argument record and the three
// HOST launch functions.  The kernels themselves are defined in impute.hip alone -- a device code object of its own, so that the
// training step's code object does not move (build_hip.py).
// Per chunk of S samples, behind the general forward (rows_ws [B S][4], hd[top] [B S][H], z [B S][L], hpart [B S][nparts]):
//   impute_merge   a wave per batch row: log w of the chunk's samples folded in fp64 into state [B][8] = (m = max log w, sum e,
//                  sum e^2, mh = max (log w + hid), sum exp(log w + hid - mh)), e = exp(log w - m); the chunk's weights e as fp32
//                  [B S] and the factor exp(m_old - m) [B] for the fold; the M reservoirs of the draws; log w to logw_out.
//   impute_fold    acc[b][d] <- acc[b][d] factor_b + sum_{s in chunk} e_bs sigmoid(h_bs . W_d + c_d): fp32 products on the matrix
//                  cores (v_mfma_f32_16x16x4_f32), the 64-column tile of W staged in LDS once per workgroup, fp64 accumulators.
// and after the last chunk
//   impute_finish  mean = acc / sum e as fp32, stats [B][4] and the slots [B][4] that iw_tail sums.
// One owner per output, fixed-order reductions, no float atomics: two calls give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmvae {

constexpr int kImputeMaxDraws = 16;
constexpr int kImputeTile = 64;          // columns of W per workgroup of impute_fold: 16 per MFMA tile, 4 tiles per wave
constexpr int kImputeLdsRows = 256;      // the staged form holds up to this many rows of W (64 KiB of LDS); wider layers read W from L2

struct ImputeArgs {
  int B, S, D, H, L, K, M;               // batch rows, samples per chunk, pixels, width of the decoder's top activation, latent size, components, draws
  int nparts;                            // column tiles of the logits launch: hpart [B S][nparts]
  unsigned long long n, s0, row0, seed, step;
  const float* rows_ws;                  // [B S][4]: .w = log w
  const float* hpart;                    // held-out Bernoulli partials, or null: every pixel observed
  const float* mcnt;                     // [B][2] (missing, observed), or null
  const float* z;                        // [B S][L]
  const float* h;                        // hd[top] [B S][H], post-activation
  const float* W;                        // [H][D], the decoder's output layer
  const float* bias;                     // [D]
  const float* bias2;                    // gen_bias_init as a vector [D], or null
  float bias_const;                      // gen_bias_init as a scalar
  double* state;                         // [B][8]
  double* keys;                          // [B][M]: the reservoirs' best keys
  float* wgt;                            // [B S]: the chunk's weights exp(log w - m)
  double* factor;                        // [B]: exp(m_old - m), 0 on the first chunk
  double* acc;                           // [B][pad4(D)]
  const float* bound;                    // [B]: iw_merge's bound (the last chunk)
  float *mean_out, *stats_out, *logw_out, *draw_z_out, *slots;
  long long* draw_index_out;
};

int impute_launch_merge(hipStream_t st, const ImputeArgs& a);
int impute_launch_fold(hipStream_t st, const ImputeArgs& a);
int impute_launch_finish(hipStream_t st, const ImputeArgs& a);

}  // namespace gmvae
