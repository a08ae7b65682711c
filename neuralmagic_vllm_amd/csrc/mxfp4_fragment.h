// The MXFP4 operand helpers of the block-scaled fp4 MFMA (include/nmx.h "MXFP4 on the native layout"): the
// activation quantiser of one 32-value block and the scaled MFMA of one tile.
// Shared by mxfp4_native.hip (the dense GEMM and the quantiser op) and moe_mxfp4.hip (the grouped form and silu_and_mul + quantiser).
#pragma once
#include "nmx_common.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

// ---- the activation quantiser of the contract (include/nmx.h): ONE lane, ONE block -----------------------------------------
// x = the block's 32 values (64 bytes, k order). amax on the bit patterns (|x| of finite values orders like its bits: 16 v_and +
// 16 v_pk_max_u16), its exponent through fp32 (a subnormal fp16 amax is a normal float), scale byte = biased exponent - 2 clamped
// at 0 - which is e + 127 with e = clamp(floor(log2 amax) - 2, -127, ..) and e = -127 for amax = 0. The 16 packed converts divide
// by 2^e (given as a float: byte << 23, and 2^-127 = 0x00400000 for byte 0), round to nearest even on the e2m1 grid and saturate
// at +-6; byte j of the result = codes of k = 2 j (low nibble) and 2 j + 1.
template <typename scalar_t>
__device__ __forceinline__ uint32_t mx_cvt_word(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, float sc) {
  uint32_t o = 0;
  if constexpr (__is_same(scalar_t, f16)) {
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(o, __builtin_bit_cast(f16x2, d0), sc, 0);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(o, __builtin_bit_cast(f16x2, d1), sc, 1);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(o, __builtin_bit_cast(f16x2, d2), sc, 2);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(o, __builtin_bit_cast(f16x2, d3), sc, 3);
  } else {
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, d0), sc, 0);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, d1), sc, 1);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, d2), sc, 2);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(o, __builtin_bit_cast(bf16x2, d3), sc, 3);
  }
  return o;
}

template <typename scalar_t>
__device__ __forceinline__ u32x4 mx_quant_block(const u32x4 (&x)[4], uint32_t& scale_byte) {
  u16x2 m = {0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) m = __builtin_elementwise_max(m, __builtin_bit_cast(u16x2, x[i][j] & 0x7fff7fffu));
  const uint32_t amax = m[0] > m[1] ? m[0] : m[1];
  float af;
  if constexpr (__is_same(scalar_t, f16)) af = (float)__builtin_bit_cast(f16, (uint16_t)amax);
  else af = __builtin_bit_cast(float, amax << 16);
  const int biased = (int)(__builtin_bit_cast(uint32_t, af) >> 23);  // (the sign bit is clear)
  scale_byte = (uint32_t)max(biased - 2, 0);
  const float sc = __builtin_bit_cast(float, max(scale_byte << 23, 0x00400000u));
  u32x4 q;
#pragma unroll
  for (int w = 0; w < 4; ++w) q[w] = mx_cvt_word<scalar_t>(x[w][0], x[w][1], x[w][2], x[w][3], sc);
  return q;
}

// tile T of a 64-column group: the weights' scale byte T of `ws` (op_sel), the activations' in byte 0 of `bs`
template <int T>
__device__ __forceinline__ f32x4 mx_mfma(u32x4 w, uint32_t ws, u32x4 b, uint32_t bs, f32x4 c) {
  const i32x8 wa = {(int)w[0], (int)w[1], (int)w[2], (int)w[3], 0, 0, 0, 0};
  const i32x8 ba = {(int)b[0], (int)b[1], (int)b[2], (int)b[3], 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa, ba, c, 4, 4, T, (int)ws, 0, (int)bs);
}

}  // namespace
