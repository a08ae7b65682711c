// The 4-bit weight fragment of the CDNA4-native W4A16 layout (include/nmx.h): packed word -> MFMA A operand.
// Shared by w4a16_native.hip (the GEMM) and moe_w4a16.hip (its grouped form over expert-sorted rows).
#pragma once
#include "nmx_common.h"

namespace {

template <typename scalar_t>
__device__ __forceinline__ f32x4 mfma_w4(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (__is_same(scalar_t, f16))
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// (q & mask) | magic as ONE v_and_or_b32 (mask in an SGPR, magic in a VGPR: a VOP3 cannot carry two literals)
__device__ __forceinline__ uint32_t and_or_w4(uint32_t q, uint32_t mask, uint32_t magic) {
  uint32_t r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(q), "s"(mask), "v"(magic));
  return r;
}

// One packed word -> the lane's A fragment (8 values q - 8, exact). fp16: 1 shift + 4 v_and_or_b32 + 2 v_pk_add_f16 + 2 v_pk_fma_f16
// = 9 VALU (1024 + q - 1032; (1024 + 16 q) / 16 - 72). bf16 has no packed arithmetic on gfx950: every code goes through fp32
// (128 + q as the float 0x4300'0000 | q << 16, minus 136), then v_cvt_pk_bf16_f32 per pair.
template <typename scalar_t>
__device__ __forceinline__ u32x4 w4_fragment(uint32_t w, uint32_t magic) {
  if constexpr (__is_same(scalar_t, f16)) {
    const f16x2 sub = __builtin_bit_cast(f16x2, 0x64086408u), r16 = __builtin_bit_cast(f16x2, 0x2c002c00u),
                n72 = __builtin_bit_cast(f16x2, 0xd480d480u);
    const uint32_t w8 = w >> 8;
    const f16x2 p0 = __builtin_bit_cast(f16x2, and_or_w4(w, 0x000f000fu, magic)) - sub;
    const f16x2 p1 = __builtin_bit_cast(f16x2, and_or_w4(w, 0x00f000f0u, magic)) * r16 + n72;
    const f16x2 p2 = __builtin_bit_cast(f16x2, and_or_w4(w8, 0x000f000fu, magic)) - sub;
    const f16x2 p3 = __builtin_bit_cast(f16x2, and_or_w4(w8, 0x00f000f0u, magic)) * r16 + n72;
    return u32x4{__builtin_bit_cast(uint32_t, p0), __builtin_bit_cast(uint32_t, p1), __builtin_bit_cast(uint32_t, p2),
                 __builtin_bit_cast(uint32_t, p3)};
  } else {
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // pair i = codes 2 i, 2 i + 1 = nibbles i, i + 4
      const float lo = __builtin_bit_cast(float, ((w << (16 - 4 * i)) & 0x000f0000u) | 0x43000000u) - 136.f;
      const float hi = __builtin_bit_cast(float, ((w >> (4 * i)) & 0x000f0000u) | 0x43000000u) - 136.f;
      union { bf16 h[2]; uint32_t u; } pk;
      pk.h[0] = (bf16)lo;
      pk.h[1] = (bf16)hi;
      o[i] = pk.u;
    }
    return o;
  }
}

// The zero-point form (fp16; include/nmx.h "zeros_native"): 8 values q - z, exact. The two wave-uniform addends
// of w4_fragment become per-lane ones: zlo = (1024 + z, 1024 + z) is subtracted from the low nibbles' 1024 + q, zhi =
// (64 + z, 64 + z) from the high nibbles' (1024 + 16 q) / 16. Same 9 VALU per word (the subtractions are source modifiers).
__device__ __forceinline__ u32x4 w4_fragment_zp(uint32_t w, uint32_t magic, f16x2 zlo, f16x2 zhi) {
  const f16x2 r16 = __builtin_bit_cast(f16x2, 0x2c002c00u);
  const uint32_t w8 = w >> 8;
  const f16x2 p0 = __builtin_bit_cast(f16x2, and_or_w4(w, 0x000f000fu, magic)) - zlo;
  const f16x2 p1 = __builtin_bit_cast(f16x2, and_or_w4(w, 0x00f000f0u, magic)) * r16 - zhi;
  const f16x2 p2 = __builtin_bit_cast(f16x2, and_or_w4(w8, 0x000f000fu, magic)) - zlo;
  const f16x2 p3 = __builtin_bit_cast(f16x2, and_or_w4(w8, 0x00f000f0u, magic)) * r16 - zhi;
  return u32x4{__builtin_bit_cast(uint32_t, p0), __builtin_bit_cast(uint32_t, p1), __builtin_bit_cast(uint32_t, p2),
               __builtin_bit_cast(uint32_t, p3)};
}

// A lane's zero row of one 128-k unit (4 fp16 values 1024 + z, tiles 0..3) -> the packed addends of its four tiles, once per
// unit: one v_perm_b32 and one v_pk_add_f16 (-960: 1024 + z -> 64 + z, exact) per tile.
struct W4Zeros {
  f16x2 lo[4], hi[4];
};
__device__ __forceinline__ W4Zeros w4_zero_addends(u32x2 z) {
  const f16x2 n960 = __builtin_bit_cast(f16x2, 0xe380e380u);
  W4Zeros o;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    o.lo[t] = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0u, z[t >> 1], (t & 1) ? 0x03020302u : 0x01000100u));
    o.hi[t] = o.lo[t] + n960;
  }
  return o;
}

}  // namespace
