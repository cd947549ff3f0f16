// TF1 AdamOptimizer / ApplyAdam (scripts/runners.py:181-183):
//   lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v EMA; theta -= lr_t*m/(sqrt(v)+eps)
// A header of its own, so that a code object that wants the update and none of the training step's kernels (csrc/refine.hpp) takes
// this statement and does not restate it.
#pragma once
#include <hip/hip_runtime.h>

namespace gmvae {

// ONE statement of the update for every kernel that applies it (adam_tf, finalize_adam's two thread maps, adam_tf_img):
// the roundings are pinned with explicit intrinsics, so the same inputs give the same bits whichever kernel ran
// (the compiler contracts a*b+c differently from one kernel to the next otherwise).
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, const float g, const float gscale, const float lr_t,
                                            const float omb1, const float omb2, const float eps) {
  const float gj = __fmul_rn(g, gscale);
  m = __fmaf_rn(__fsub_rn(gj, m), omb1, m);
  v = __fmaf_rn(__fmaf_rn(gj, gj, -v), omb2, v);
  p = __fsub_rn(p, __fdiv_rn(__fmul_rn(m, lr_t), __fadd_rn(__fsqrt_rn(v), eps)));
}

}  // namespace gmvae
