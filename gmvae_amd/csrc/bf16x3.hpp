// An fp32 value as three bf16 pieces, hi + mid + lo = v EXACTLY: each piece is the truncation of what is left to 16 bits (sign,
// exponent, 7 mantissa bits: 8 significant bits), each residual is exact (Sterbenz), and three pieces cover the 24-bit
// significand.  A product of a piece with a value that is exact in bf16 (a byte: 8 significant bits) is exact in fp32, so a
// contraction on the bf16 matrix cores over such products rounds only in its fp32 accumulation -- like the fp32 MFMA form, at 3
// v_mfma_f32_16x16x32_bf16 (16 cycles each) per 32 contraction steps instead of 8 v_mfma_f32_16x16x4_f32 (32 cycles each).
// Used by the uint8 weight-gradient tiles (dwadam.hpp) and the one-launch step's first layer (mega2.hpp).
// For |v| below about 2^-102 the lo piece is a subnormal bf16, which the matrix core may flush: an error of at most
// 2^-126 x 255 per product.
#pragma once
#include <hip/hip_runtime.h>

namespace gmvae {

__device__ __forceinline__ unsigned pack_hi16(const float f1, const float f0) {     // (bf16 bits of f0) | (bf16 bits of f1) << 16, truncating
  return __builtin_amdgcn_perm(__float_as_uint(f1), __float_as_uint(f0), 0x07060302u);
}
// the pieces of two values, packed as pairs {v0's, v1's}: and, sub, and, sub per value and three v_perm per pair
__device__ __forceinline__ void split3_bf16(const float v0, const float v1, unsigned& hi, unsigned& mid, unsigned& lo) {
  hi = pack_hi16(v1, v0);
  const float r0 = v0 - __uint_as_float(__float_as_uint(v0) & 0xffff0000u), r1 = v1 - __uint_as_float(__float_as_uint(v1) & 0xffff0000u);
  mid = pack_hi16(r1, r0);
  const float s0 = r0 - __uint_as_float(__float_as_uint(r0) & 0xffff0000u), s1 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
  lo = pack_hi16(s1, s0);
}

}  // namespace gmvae
