// W4A16 on a weight layout made for gfx950 (include/nmx.h "CDNA4-native W4A16"): the GPTQ checkpoint tensors
// are rewritten ONCE into the order v_mfma_f32_16x16x32_{f16,bf16} consumes with the WEIGHTS as its A operand and natural-k
// activations as B, and the GEMM streams that order with one 16-byte load per lane and 32-k step. No reference counterpart (the
// reference repacks GPTQ -> Marlin at load, gptq_marlin.py:330-420, into the fragment order of NVIDIA's mma.m16n8k16).
//
//   qweight_native  int32 [K / 128][N / 64][step s = 0..3][lane l = 16 g + r][tile t = 0..3]
//       word (u, c, s, l, t) = the 8 codes of column n = 64 c + 16 t + r at k = 128 u + 32 s + 8 g + j, code j in nibble
//       P[j] = [0, 4, 1, 5, 2, 6, 3, 7]: (w & 0x000f000f), (w & 0x00f000f0) and the same masks on w >> 8 are the fp16 pairs
//       (k0,k1) (k2,k3) (k4,k5) (k6,k7) of the lane's A fragment. A lane's 16 bytes = its fragment words of the wave's four
//       16-column tiles for ONE 32-k step, so the register is free - and re-issued two units ahead - right after that step.
//   scales_native   scalar [G][N / 64][g][t][j] = scales[G][64 c + 16 t + 4 g + j]: the 16 scales of a lane's accumulators
//       (D row 4 g + j of tile t) are 32 contiguous bytes. The scales multiply the fp32 accumulators of a 128-k unit, not the
//       weights: (q - 8) * s cannot be formed by one fp16 FMA on the magic-number form (the addend -1032 s needs 19 bits).
//   zeros_native    fp16 [G][N / 64][r][t] = 1024 + z[G][64 c + 16 t + r] (AWQ, fp16, one group per 128 k): the zero points of a
//       lane's column in its four tiles are 8 contiguous bytes; W[k, n] = (q - z) * s.
#include "w4a16_fragment.h"

#include <stdlib.h>

namespace {

struct W4Params {
  const void* a;          // [M, K]
  const int32_t* qw;      // qweight_native
  const void* scales;     // scales_native
  void* c;                // [M, N]
  float* partial;         // [k_splits, M, N] fp32 slabs (k_splits > 1)
  int M, N, K, num_groups, k_splits;
  int xcd_per;            // > 0: XCDs per K split (2 / 4 / 8 splits, the split is chosen by the workgroup id % 8)
  const void* zeros;      // zeros_native (the zero-point form only)
};

struct W4Cfg { int mt, nw, splits; };

// element o of scales_native (shared by the 4- and the 8-bit repack)
__device__ __forceinline__ void repack_scale(int64_t o, const uint16_t* __restrict__ scales, uint16_t* __restrict__ snative, int N,
                                             int G) {
  if (o < (int64_t)G * N) {
    const int C = N / 64;
    const int j = (int)(o & 3), t = (int)(o >> 2) & 3, g = (int)(o >> 4) & 3;
    const int64_t gc = o >> 6;
    const int c = (int)(gc % C), grp = (int)(gc / C);
    snative[o] = scales[(int64_t)grp * N + 64 * c + 16 * t + 4 * g + j];
  }
}

// ---- repack: GPTQ checkpoint qweight [K / 8, N] (code k % 8 of row k / 8 at bits 4 (k % 8)) + scales [G, N] -> the native pair.
// Native word (u, c, s, 16 g + r, t) is checkpoint word (16 u + 4 s + g, 64 c + 16 t + r) with its nibbles moved j -> P[j].
__global__ void w4a16_repack_kernel(const uint32_t* __restrict__ qweight, const uint16_t* __restrict__ scales,
                                    uint32_t* __restrict__ qnative, uint16_t* __restrict__ snative, int K, int N, int G) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t words = (int64_t)(K / 8) * N;
  const int C = N / 64;
  if (o < words) {
    const int t = (int)(o & 3), l = (int)(o >> 2) & 63, s = (int)(o >> 8) & 3;
    const int64_t uc = o >> 10;
    const int c = (int)(uc % C), u = (int)(uc / C);
    const int kk = 16 * u + 4 * s + (l >> 4), n = 64 * c + 16 * t + (l & 15);
    const uint32_t w = qweight[(int64_t)kk * N + n];
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) r |= ((w >> (4 * j)) & 0xfu) << (4 * ((j >> 1) + 4 * (j & 1)));
    qnative[o] = r;
  }
  repack_scale(o, scales, snative, N, G);
}

// ---- repack of an AWQ checkpoint: qweight [K, N / 8] and qzeros [K / 128, N / 8] (W[k, 8 c + j] in nibble O[j], O = [0, 4, 1, 5,
// 2, 6, 3, 7]) + scales [K / 128, N] fp16 -> the native triple. The checkpoint packs along N, the native word along K: a native
// word gathers one nibble position of 8 source words down K. A workgroup takes one 128-k unit x 256 columns (4 column groups):
// its 128 x 32 source words go through LDS - a wave reads two whole 128-byte rows per pass - and every thread then builds 16
// native words from it (8 LDS reads each, the 16 lanes of a tile pair on 2 words of a row: broadcasts), written as 4 KiB runs.
// zeros_native [G][N / 64][r][t] = fp16 (1024 + z) of column 64 c + 16 t + r, element o by thread o; scales: repack_scale.
__global__ __launch_bounds__(256) void awq_native_repack_kernel(const uint32_t* __restrict__ qweight, const uint32_t* __restrict__ qzeros,
                                                                const uint16_t* __restrict__ scales, uint32_t* __restrict__ qnative,
                                                                uint16_t* __restrict__ snative, uint16_t* __restrict__ znative, int K, int N) {
  __shared__ uint32_t tile[128][33];  // (+ 1: the 8 rows of a native word on 8 banks)
  const int C = N / 64, NW = N / 8, CW = (C + 3) / 4;
  const int u = blockIdx.x / CW, cw = blockIdx.x % CW;
  for (int e = threadIdx.x; e < 128 * 32; e += 256) {
    const int row = e >> 5, w = e & 31;
    if (32 * cw + w < NW) tile[row][w] = qweight[(int64_t)(128 * u + row) * NW + 32 * cw + w];
  }
  __syncthreads();
  const int ngroups = min(4, C - 4 * cw);
  for (int e = threadIdx.x; e < ngroups * 1024; e += 256) {  // word (s, l = 16 g + r, t) of column group 4 cw + (e >> 10)
    const int t = e & 3, l = (e >> 2) & 63, s = (e >> 8) & 3;
    const int n = 64 * (e >> 10) + 16 * t + (l & 15);  // column inside the tile
    const int sh = 4 * ((n & 1) * 4 + ((n & 7) >> 1));  // O[n % 8]
    const int row = 32 * s + 8 * (l >> 4);
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) r |= ((tile[row + j][n >> 3] >> sh) & 0xfu) << (4 * ((j >> 1) + 4 * (j & 1)));
    qnative[((int64_t)u * C + 4 * cw) * 1024 + e] = r;
  }
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (grid: K / 128 * CW * 256 >= K / 128 * N threads)
  const int G = K / 128;
  if (o < (int64_t)G * N) {
    const int t = (int)(o & 3), r = (int)(o >> 2) & 15;
    const int64_t gc = o >> 6;
    const int n = 64 * (int)(gc % C) + 16 * t + r;
    const uint32_t z = (qzeros[(gc / C) * NW + (n >> 3)] >> (4 * ((n & 1) * 4 + ((n & 7) >> 1)))) & 0xfu;
    znative[o] = (uint16_t)(0x6400u | z);  // fp16 1024 + z
  }
  repack_scale(o, scales, snative, N, G);
}

// ---- the GEMM. c [M, N] = a [M, K] . W, W[k, n] = (q - 8) * s[group(k), n].
// D = W^T-tile (A operand, 16 columns x 32 k) x activations (B operand, 32 k x 16 rows): lane (g, r) of tile t holds rows
// m = r, columns 16 t + 4 g + 0..3 - four consecutive outputs, one 8-byte store.
//   STAGED = false (MT = 1, up to 16 rows): NW waves on ONE 64-column group, every wave its own K slice in units of 128 k; a
//     lane's B fragment is 16 contiguous bytes of its activation row straight from global memory, no LDS and no barrier in the
//     loop; the NW slices are summed through LDS with one barrier.
//   STAGED = true (MT = 2 / 4): 4 waves on 4 ADJACENT column groups sharing one K slice; the (16 MT) x 128-k activation tile of
//     a unit is fetched once per workgroup (MT 16-byte loads per thread, a unit ahead), written to a double-buffered LDS image
//     with chunk ^ (row & 15) swizzle and read as fragments by all four waves: one barrier per unit.
// Weights never touch LDS: one raw_buffer_load (dwordx4) per lane and 32-k step, issued in one fixed order two units ahead
// (2 x 4 KiB per wave in flight), waits counted by hipcc. GROUPED: one scale row per 128-k unit, applied to the unit's fp32
// accumulators; channel-wise scales are applied once, in the epilogue. (GROUPED at MT = 4 holds 64 + 64 accumulators: it takes
// more than the 256 registers of two workgroups per CU, so that one form is compiled for one.)
// ZP (fp16, GROUPED): W[k, n] = (q - z[group(k), n]) * s[group(k), n]. The lane's zero row of a unit (8 bytes of zeros_native: its
// column's zero point in each of the four tiles) is loaded right after the unit's scale row, in the same ring; compute_unit
// turns it into the packed addends of w4_fragment_zp before the unit's first step.
template <typename scalar_t, int MT, int NW, bool GROUPED, bool STAGED, bool ZP = false>
__global__ __launch_bounds__(64 * NW, (GROUPED && MT == 4) ? 1 : 2) void w4a16_gemm_kernel(const W4Params p) {
  static_assert(STAGED ? NW == 4 : MT == 1, "staged: 4 waves = 4 column groups; unstaged: one 16-row tile");
  static_assert(!ZP || (GROUPED && __is_same(scalar_t, f16)), "zero points: fp16, one zero row per 128-k unit");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int N = p.N, K = p.K, M = p.M;
  const int C = N / 64, total_units = K / 128;

  // workgroup -> (column workgroup, K split). With 2 / 4 / 8 splits the XCD (= workgroup id % 8) selects the split: 8 / splits
  // XCDs share one split's slice of the activations, each on its own column workgroups.
  const int ncolwg = STAGED ? (C + 3) / 4 : C;
  int colwg, split;
  if (p.xcd_per > 0) {
    const int lin = blockIdx.x;
    split = (lin & 7) / p.xcd_per;
    colwg = (lin >> 3) * p.xcd_per + (lin & 7) % p.xcd_per;
  } else {
    colwg = blockIdx.x;
    split = blockIdx.y;
  }
  if (colwg >= ncolwg) return;  // padding workgroup (whole workgroup: no barrier is skipped)
  const int cg = STAGED ? colwg * 4 + wave : colwg;
  const bool col_ok = cg < C;
  const int cl = min(cg, C - 1);  // column group used for the loads (a wave past N computes a valid group again, never stored)
  const int m0 = blockIdx.z * (16 * MT);

  // K slice in units of 128 k
  constexpr int SLICES = STAGED ? 1 : NW;
  const int workers = p.k_splits * SLICES;
  const int per = (total_units + workers - 1) / workers;
  const int worker = split * SLICES + (STAGED ? 0 : wave);
  const int u0 = min(worker * per, total_units), u1 = min(u0 + per, total_units);

  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(p.qw), 0, (K / 2) * N, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, M * K * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.scales), 0, p.num_groups * N * 2, 0x00020000);
  const int unit_bytes = C * 4096;  // one 128-k unit of all column groups
  const int w_voff = cl * 4096 + lane * 16;
  const int s_voff = (cl * 4 + g) * 32;
  const __amdgpu_buffer_rsrc_t rs_z = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.zeros), 0, ZP ? p.num_groups * N * 2 : 0, 0x00020000);
  const int z_voff = (cl * 16 + r) * 8;
  constexpr int kPast = 0x7ff00000;  // beyond every descriptor: the load returns zeros
  // unstaged: the lane's own row; staged: chunk e = tid + 256 i of the tile image (row e >> 4, 16-byte chunk e & 15)
  int a_voff[STAGED ? MT : 1], a_lds[STAGED ? MT : 1];
  if constexpr (STAGED) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int e = threadIdx.x + 256 * i, row = e >> 4, ch = e & 15;
      a_voff[i] = (m0 + row < M) ? ((m0 + row) * K + 8 * ch) * 2 : kPast;
      a_lds[i] = row * 256 + ((ch ^ (row & 15)) * 16);
    }
  } else {
    a_voff[0] = (m0 + r < M) ? ((m0 + r) * K + 8 * g) * 2 : kPast;
    a_lds[0] = 0;
  }

  constexpr int kTile = MT * 4096;  // staged activation image of one unit
  __shared__ __attribute__((aligned(16))) char smem[STAGED ? 2 * kTile : NW * 4096];

  struct Unit {
    u32x4 q[4];
    u32x4 a[STAGED ? 1 : 4];
    u32x4 s[2];
    u32x2 z;
  };
  // loads of one 32-k step / the scale row of unit u (past the slice: the last unit again, never consumed). sched_barrier pins
  // the issue order: prologue and loop must queue the loads alike, or the merged wait counts at the loop head degrade.
  auto load_step = [&](int u, int ks, Unit& U) {
    u = min(u, total_units - 1);
    U.q[ks] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, w_voff, u * unit_bytes + ks * 1024, 2);  // aux 2: non-temporal
    if constexpr (!STAGED) U.a[ks] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_voff[0], (u * 128 + ks * 32) * 2, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto load_scales = [&](int u, Unit& U) {
    if constexpr (GROUPED) {
      u = min(u, total_units - 1);  // one group per unit
      U.s[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff, u * N * 2, 0);
      U.s[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff + 16, u * N * 2, 0);
      if constexpr (ZP) U.z = __builtin_amdgcn_raw_buffer_load_b64(rs_z, z_voff, u * N * 2, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto load_unit = [&](int u, Unit& U) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) load_step(u, ks, U);
    load_scales(u, U);
  };
  u32x4 areg[STAGED ? MT : 1];
  auto stage_load = [&](int u) {
    if constexpr (STAGED) {
      u = min(u, total_units - 1);
#pragma unroll
      for (int i = 0; i < MT; ++i) areg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_voff[i], u * 256, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto stage_store = [&](char* buf) {
    if constexpr (STAGED) {
#pragma unroll
      for (int i = 0; i < MT; ++i) *reinterpret_cast<u32x4*>(buf + a_lds[i]) = areg[i];
    }
  };

  f32x4 acc[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint32_t magic = 0x64006400u;

  // consumes unit U (activations: its own registers, or the LDS image buf) and re-issues each register set for unit `next`
  // as soon as it is free
  auto compute_unit = [&](Unit& U, int next, const char* buf, bool reissue) {
    f32x4 gacc[GROUPED ? MT : 1][4];
    W4Zeros zp;
    if constexpr (ZP) zp = w4_zero_addends(U.z);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      u32x4 bf[MT];
      if constexpr (STAGED) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          bf[mt] = *reinterpret_cast<const u32x4*>(buf + (16 * mt + r) * 256 + (((4 * ks + g) ^ r) * 16));
      } else {
        bf[0] = U.a[ks];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        u32x4 wf;
        if constexpr (ZP) wf = w4_fragment_zp(U.q[ks][t], magic, zp.lo[t], zp.hi[t]);
        else wf = w4_fragment<scalar_t>(U.q[ks][t], magic);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          if constexpr (GROUPED) gacc[mt][t] = mfma_w4<scalar_t>(wf, bf[mt], ks == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : gacc[mt][t]);
          else acc[mt][t] = mfma_w4<scalar_t>(wf, bf[mt], acc[mt][t]);
        }
      }
      if (reissue) load_step(next, ks, U);
    }
    if constexpr (GROUPED) {
      union { u32x4 v[2]; scalar_t e[16]; } raw;
      raw.v[0] = U.s[0];
      raw.v[1] = U.s[1];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float sv = Scalar<scalar_t>::to_f32(raw.e[4 * t + j]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt][t][j] = __builtin_fmaf(sv, gacc[mt][t][j], acc[mt][t][j]);
        }
      if (reissue) load_scales(next, U);
    }
  };

  Unit ua, ub;
  char* const buf0 = smem;
  char* const buf1 = smem + (STAGED ? kTile : 0);
  if (u0 < u1) {
    stage_load(u0);
    load_unit(u0, ua);
    load_unit(u0 + 1, ub);
    if constexpr (STAGED) {
      stage_store(buf0);
      stage_load(u0 + 1);
      __syncthreads();
    }
    // whole pairs, then a peeled odd unit (its loads are already in ua; nothing is re-issued). Staged: a unit reads the image
    // the previous iteration wrote before its barrier, and writes the other one, which every wave finished reading before that
    // same barrier.
    int u = u0;
    for (; u + 1 < u1; u += 2) {
      compute_unit(ua, u + 2, buf0, true);
      if constexpr (STAGED) {
        stage_store(buf1);
        stage_load(u + 2);
        __syncthreads();
      }
      compute_unit(ub, u + 3, buf1, true);
      if constexpr (STAGED) {
        stage_store(buf0);
        stage_load(u + 3);
        __syncthreads();
      }
    }
    if (u < u1) compute_unit(ua, u, buf0, false);
  }

  // ---- epilogue ----
  scalar_t* const cptr = reinterpret_cast<scalar_t*>(p.c);
  if constexpr (STAGED) {
    if (!col_ok) return;
    union { u32x4 v[2]; scalar_t e[16]; } sc;
    if constexpr (!GROUPED) {
      sc.v[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff, 0, 0);
      sc.v[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff + 16, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m0 + 16 * mt + r;
      if (m >= M) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 v = acc[mt][t];
        if constexpr (!GROUPED) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] *= Scalar<scalar_t>::to_f32(sc.e[4 * t + j]);
        }
        const int64_t off = (int64_t)m * N + cg * 64 + 16 * t + 4 * g;
        if (p.k_splits == 1) {
          union { scalar_t h[4]; u32x2 u; } o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o.h[j] = Scalar<scalar_t>::from_f32(v[j]);
          *reinterpret_cast<u32x2*>(cptr + off) = o.u;
        } else {
          *reinterpret_cast<f32x4*>(p.partial + (int64_t)split * M * N + off) = v;
        }
      }
    }
  } else {
    // sum the NW K slices through LDS: thread e < 256 owns float4 e of the workgroup's [4 tiles][64 lanes] image
    f32x4* red = reinterpret_cast<f32x4*>(smem);
#pragma unroll
    for (int t = 0; t < 4; ++t) red[(wave * 4 + t) * 64 + lane] = acc[0][t];
    __syncthreads();
    for (int e = threadIdx.x; e < 256; e += 64 * NW) {
      f32x4 v = red[e];
#pragma unroll
      for (int w = 1; w < NW; ++w) v += red[w * 256 + e];
      const int t = e >> 6, el = e & 63, eg = el >> 4;
      const int m = m0 + (el & 15);
      if (m >= M) continue;
      if constexpr (!GROUPED) {
        union { u32x2 u; scalar_t e[4]; } sc;
        sc.u = *reinterpret_cast<const u32x2*>(reinterpret_cast<const scalar_t*>(p.scales) + (cg * 4 + eg) * 16 + 4 * t);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] *= Scalar<scalar_t>::to_f32(sc.e[j]);
      }
      const int64_t off = (int64_t)m * N + cg * 64 + 16 * t + 4 * eg;
      if (p.k_splits == 1) {
        union { scalar_t h[4]; u32x2 u; } o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.h[j] = Scalar<scalar_t>::from_f32(v[j]);
        *reinterpret_cast<u32x2*>(cptr + off) = o.u;
      } else {
        *reinterpret_cast<f32x4*>(p.partial + (int64_t)split * M * N + off) = v;
      }
    }
  }
}

// ---- the tall GEMM (MT = 8): 128 rows per workgroup, every weight fragment converted ONCE per workgroup and used against 8
// B fragments. 4 waves on 4 adjacent column groups share one K slice, as the staged form above; a wave owns
// one 64-column group x 128 rows = 32 f32x4 accumulators (128 registers; GROUPED doubles them for the unit's sums: one wave per
// SIMD, one workgroup per CU). The 128-row x 128-k activation image of a unit (32 KiB) is fetched once per workgroup a unit
// ahead (8 x 16-byte loads per thread), double-buffered in LDS with the same swizzle, one barrier per unit.
// Weight stream: a ring of 8 dwordx4 registers per lane = the wave's steps of the next 2 units, each slot re-issued two units
// ahead right after its step; the loop body is 2 units so that every slot is a fixed register and the LDS image is j & 1. A
// slice of any length (0, 1, odd) leaves the loop after its last unit; loads past the slice read the last unit again and are
// never consumed. GROUPED: one scale row in flight, a unit ahead. No scratch, except bf16 GROUPED (about 200 bytes per lane with
// 256 accumulators; a one-unit ring and one or two fragments per pass did not remove it).
template <typename scalar_t, bool GROUPED>
__global__ __launch_bounds__(256, 1) void w4a16_tall_kernel(const W4Params p) {
  constexpr int RT = 8;  // 16-row tiles
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int N = p.N, K = p.K, M = p.M;
  const int C = N / 64, total_units = K / 128;

  const int ncolwg = (C + 3) / 4;
  int colwg, split;
  if (p.xcd_per > 0) {  // as w4a16_gemm_kernel: the XCD selects the K split
    const int lin = blockIdx.x;
    split = (lin & 7) / p.xcd_per;
    colwg = (lin >> 3) * p.xcd_per + (lin & 7) % p.xcd_per;
  } else {
    colwg = blockIdx.x;
    split = blockIdx.y;
  }
  if (colwg >= ncolwg) return;  // padding workgroup (whole workgroup: no barrier is skipped)
  const int cg = colwg * 4 + wave;
  const bool col_ok = cg < C;
  const int cl = min(cg, C - 1);
  const int m0 = blockIdx.z * (16 * RT);
  const int per = (total_units + p.k_splits - 1) / p.k_splits;
  const int u0 = min(split * per, total_units), u1 = min(u0 + per, total_units);  // may be empty: the slab gets zeros

  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(p.qw), 0, (K / 2) * N, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, M * K * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.scales), 0, p.num_groups * N * 2, 0x00020000);
  const int unit_bytes = C * 4096;
  const int w_voff = cl * 4096 + lane * 16;
  const int s_voff = (cl * 4 + g) * 32;
  constexpr int kPast = 0x7ff00000;
  // chunk e = tid + 256 i of the tile image: row e >> 4 = 16 i + (tid >> 4), 16-byte chunk tid & 15
  int a_voff[RT];
  const int a_row = threadIdx.x >> 4, a_ch = threadIdx.x & 15;
  const int a_lds = a_row * 256 + ((a_ch ^ a_row) * 16);  // + 4096 i
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    const int row = m0 + 16 * i + a_row;
    a_voff[i] = row < M ? (row * K + 8 * a_ch) * 2 : kPast;
  }
  int b_lds[4];  // the lane's B fragment of step ks, row tile 0 (+ 4096 mt)
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) b_lds[ks] = r * 256 + (((4 * ks + g) ^ r) * 16);

  constexpr int kTile = RT * 4096;
  __shared__ __attribute__((aligned(16))) char smem[2 * kTile];

  u32x4 q[8], sc[2], areg[RT];
  auto load_step = [&](int u, int slot) {  // slot = 4 * (unit & 1) + step
    u = min(u, total_units - 1);
    q[slot] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, w_voff, u * unit_bytes + (slot & 3) * 1024, 2);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto load_scales = [&](int u) {
    if constexpr (GROUPED) {
      u = min(u, total_units - 1);
      sc[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff, u * N * 2, 0);
      sc[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff + 16, u * N * 2, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto stage_load = [&](int u) {
    u = min(u, total_units - 1);
#pragma unroll
    for (int i = 0; i < RT; ++i) areg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_voff[i], u * 256, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto stage_store = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < RT; ++i) *reinterpret_cast<u32x4*>(buf + a_lds + 4096 * i) = areg[i];
  };

  f32x4 acc[RT][4];
#pragma unroll
  for (int mt = 0; mt < RT; ++mt)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint32_t magic = 0x64006400u;

  // unit u = unit j of the trip: its steps from ring slots 4 j .., activations from image buf
  auto compute_unit = [&](int u, int j, const char* buf) {
    f32x4 gacc[GROUPED ? RT : 1][4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      // the step's four fragments first, then the row tiles one LDS read ahead of their MFMAs: few registers live
      u32x4 wf[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) wf[t] = w4_fragment<scalar_t>(q[4 * j + ks][t], magic);
      u32x4 b0 = *reinterpret_cast<const u32x4*>(buf + b_lds[ks]);
#pragma unroll
      for (int mt = 0; mt < RT; ++mt) {
        const u32x4 b1 = *reinterpret_cast<const u32x4*>(buf + b_lds[ks] + 4096 * (mt + 1 < RT ? mt + 1 : mt));
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if constexpr (GROUPED) gacc[mt][t] = mfma_w4<scalar_t>(wf[t], b0, ks == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : gacc[mt][t]);
          else acc[mt][t] = mfma_w4<scalar_t>(wf[t], b0, acc[mt][t]);
        }
        b0 = b1;
        if constexpr (GROUPED) __builtin_amdgcn_sched_barrier(0);  // keeps the reads from being hoisted: 256 accumulators
      }
      load_step(u + 2, 4 * j + ks);
    }
    if constexpr (GROUPED) {
      union { u32x4 v[2]; scalar_t e[16]; } raw;
      raw.v[0] = sc[0];
      raw.v[1] = sc[1];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float sv = Scalar<scalar_t>::to_f32(raw.e[4 * t + jj]);
#pragma unroll
          for (int mt = 0; mt < RT; ++mt) acc[mt][t][jj] = __builtin_fmaf(sv, gacc[mt][t][jj], acc[mt][t][jj]);
        }
      load_scales(u + 1);
    }
  };

  char* const buf0 = smem;
  char* const buf1 = smem + kTile;
  if (u0 < u1) {
    stage_load(u0);
#pragma unroll
    for (int slot = 0; slot < 8; ++slot) load_step(u0 + (slot >> 2), slot);  // the order in which the loop re-issues them
    load_scales(u0);
    stage_store(buf0);
    stage_load(u0 + 1);
    __syncthreads();
    // Unit j of a trip reads image j, written before the previous barrier, and writes the other one, which every wave
    // finished reading before that same barrier.
    [&] {
      for (int u = u0;; u += 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          compute_unit(u + j, j, j ? buf1 : buf0);
          stage_store(j ? buf0 : buf1);
          stage_load(u + j + 2);
          __syncthreads();
          if (u + j + 1 >= u1) return;
        }
      }
    }();
  }

  // ---- epilogue: scale (channel-wise), store ----
  if (!col_ok) return;
  scalar_t* const cptr = reinterpret_cast<scalar_t*>(p.c);
  union { u32x4 v[2]; scalar_t e[16]; } cs;
  if constexpr (!GROUPED) {
    cs.v[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff, 0, 0);
    cs.v[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff + 16, 0, 0);
  }
#pragma unroll
  for (int mt = 0; mt < RT; ++mt) {
    const int m = m0 + 16 * mt + r;
    if (m >= M) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 v = acc[mt][t];
      if constexpr (!GROUPED) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] *= Scalar<scalar_t>::to_f32(cs.e[4 * t + j]);
      }
      const int64_t off = (int64_t)m * N + cg * 64 + 16 * t + 4 * g;
      if (p.k_splits == 1) {
        union { scalar_t h[4]; u32x2 u; } o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.h[j] = Scalar<scalar_t>::from_f32(v[j]);
        *reinterpret_cast<u32x2*>(cptr + off) = o.u;
      } else {
        *reinterpret_cast<f32x4*>(p.partial + (int64_t)split * M * N + off) = v;
      }
    }
  }
}

// ======== 8 bits (include/nmx.h "8-bit form") ===========================================================
//   qweight_native  int32 [K / 128][N / 64][step s = 0..3][half h = 0..1][lane l = 16 g + r][word 2 (t & 1) + j], tile t = 2 h + ..
//       word (u, c, s, h, l, 2 (t & 1) + j) = the 4 codes of column n = 64 c + 16 t + r at k = 128 u + 32 s + 8 g + 4 j + i, code i
//       in byte i: it IS checkpoint word (32 u + 8 s + 2 g + j, n) - the repack only moves words. A lane's 16 bytes = the two
//       complete A fragments of tiles 2 h, 2 h + 1 for one 32-k step: two loads per lane and step, 8 KiB per unit and group.
//   scales_native as above. W[k, n] = (q - 128) * s[group(k), n].

// Two words -> the lane's A fragment (8 values q - 128, exact), no shift. fp16: v_perm_b32 against 0x64 bytes makes the pair
// (1024 + b0, 1024 + b1), one v_pk_add_f16 of -1152 finishes it: 4 + 4 = 8 VALU. bf16 (no packed arithmetic; 0x4300 | b holds 7
// bits): v_cvt_f32_ubyteN, minus 128, v_cvt_pk_bf16_f32 per pair = 20 VALU; q - 128 has 8 significant bits, exact in bf16.
// (as asm: written as (float)(byte) - 128.f the subtraction is folded into integer SDWA adds and the pairs are re-packed by hand,
// about 30 VALU per fragment)
template <int B>
__device__ __forceinline__ float ubyte_f32(uint32_t w) {
  float f;
  if constexpr (B == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(w));
  else if constexpr (B == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(w));
  else if constexpr (B == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(w));
  else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(w));
  return f;
}

template <typename scalar_t, int H>  // pair H = bytes 2 H, 2 H + 1 of w
__device__ __forceinline__ uint32_t w8_pair(uint32_t w) {
  if constexpr (__is_same(scalar_t, f16)) {
    const f16x2 n1152 = __builtin_bit_cast(f16x2, 0xe480e480u);
    const uint32_t pair = __builtin_amdgcn_perm(0x64646464u, w, H ? 0x04030402u : 0x04010400u);
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2, pair) + n1152);
  } else {
    union { bf16 h[2]; uint32_t u; } pk;
    pk.h[0] = (bf16)(ubyte_f32<2 * H>(w) - 128.f);
    pk.h[1] = (bf16)(ubyte_f32<2 * H + 1>(w) - 128.f);
    return pk.u;
  }
}

template <typename scalar_t>
__device__ __forceinline__ u32x4 w8_fragment(uint32_t w0, uint32_t w1) {
  return u32x4{w8_pair<scalar_t, 0>(w0), w8_pair<scalar_t, 1>(w0), w8_pair<scalar_t, 0>(w1), w8_pair<scalar_t, 1>(w1)};
}

// Native word o is checkpoint word (32 u + 8 s + 2 g + j, 64 c + 16 t + r), unchanged.
__global__ void w8a16_repack_kernel(const uint32_t* __restrict__ qweight, const uint16_t* __restrict__ scales,
                                    uint32_t* __restrict__ qnative, uint16_t* __restrict__ snative, int K, int N, int G) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int C = N / 64;
  if (o < (int64_t)(K / 4) * N) {
    const int j = (int)(o & 1), t = 2 * ((int)(o >> 8) & 1) + ((int)(o >> 1) & 1), l = (int)(o >> 2) & 63, s = (int)(o >> 9) & 3;
    const int64_t uc = o >> 11;
    const int c = (int)(uc % C), u = (int)(uc / C);
    const int kk = 32 * u + 8 * s + 2 * (l >> 4) + j, n = 64 * c + 16 * t + (l & 15);
    qnative[o] = qweight[(int64_t)kk * N + n];
  }
  repack_scale(o, scales, snative, N, G);
}

// ---- the 8-bit GEMM: the forms, epilogues, K slabs and workgroup mapping of w4a16_gemm_kernel (above) on twice the weight
// bytes. Weight stream: a ring of ONE unit = 8 dwordx4 registers per lane (4 steps x 2 halves, 32 VGPRs - what the 4-bit kernel
// holds for two units); a half is converted, fed to its 2 MT MFMAs and re-issued for the next unit at once, so a wave keeps 8 KiB
// of weights in flight, the same bytes as the 4-bit kernel's two units. The last unit of a slice is peeled and re-issues nothing:
// no weight byte is read twice or past the slice. Staged: the two LDS images alternate by a run-time offset (one unit per trip).
template <typename scalar_t, int MT, int NW, bool GROUPED, bool STAGED>
__global__ __launch_bounds__(64 * NW, (GROUPED && MT == 4) ? 1 : 2) void w8a16_gemm_kernel(const W4Params p) {
  static_assert(STAGED ? NW == 4 : MT == 1, "staged: 4 waves = 4 column groups; unstaged: one 16-row tile");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int N = p.N, K = p.K, M = p.M;
  const int C = N / 64, total_units = K / 128;

  const int ncolwg = STAGED ? (C + 3) / 4 : C;
  int colwg, split;
  if (p.xcd_per > 0) {  // as w4a16_gemm_kernel: the XCD selects the K split
    const int lin = blockIdx.x;
    split = (lin & 7) / p.xcd_per;
    colwg = (lin >> 3) * p.xcd_per + (lin & 7) % p.xcd_per;
  } else {
    colwg = blockIdx.x;
    split = blockIdx.y;
  }
  if (colwg >= ncolwg) return;  // padding workgroup (whole workgroup: no barrier is skipped)
  const int cg = STAGED ? colwg * 4 + wave : colwg;
  const bool col_ok = cg < C;
  const int cl = min(cg, C - 1);  // a wave past N computes a valid group again, never stored
  const int m0 = blockIdx.z * (16 * MT);

  constexpr int SLICES = STAGED ? 1 : NW;
  const int workers = p.k_splits * SLICES;
  const int per = (total_units + workers - 1) / workers;
  const int worker = split * SLICES + (STAGED ? 0 : wave);
  const int u0 = min(worker * per, total_units), u1 = min(u0 + per, total_units);

  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(p.qw), 0, K * N, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, M * K * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.scales), 0, p.num_groups * N * 2, 0x00020000);
  const int unit_bytes = C * 8192;  // one 128-k unit of all column groups
  const int w_voff = cl * 8192 + lane * 16;
  const int s_voff = (cl * 4 + g) * 32;
  constexpr int kPast = 0x7ff00000;  // beyond every descriptor: the load returns zeros
  int a_voff[STAGED ? MT : 1], a_lds[STAGED ? MT : 1];
  if constexpr (STAGED) {  // chunk e = tid + 256 i of the tile image (row e >> 4, 16-byte chunk e & 15)
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int e = threadIdx.x + 256 * i, row = e >> 4, ch = e & 15;
      a_voff[i] = (m0 + row < M) ? ((m0 + row) * K + 8 * ch) * 2 : kPast;
      a_lds[i] = row * 256 + ((ch ^ (row & 15)) * 16);
    }
  } else {
    a_voff[0] = (m0 + r < M) ? ((m0 + r) * K + 8 * g) * 2 : kPast;
    a_lds[0] = 0;
  }

  constexpr int kTile = MT * 4096;  // staged activation image of one unit
  __shared__ __attribute__((aligned(16))) char smem[STAGED ? 2 * kTile : NW * 4096];

  u32x4 q[4][2], areg[STAGED ? MT : 4], sc[2];  // the ring; activations (unstaged: the unit's B fragments); the unit's scale row
  // the loads of unit u (always inside the slice), queued in one order by prologue and loop (sched_barrier pins it)
  auto load_half = [&](int u, int ks, int h) {
    q[ks][h] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, w_voff, u * unit_bytes + ks * 2048 + h * 1024, 2);  // aux 2: non-temporal
    __builtin_amdgcn_sched_barrier(0);
  };
  auto load_a = [&](int u, int ks) {
    if constexpr (!STAGED) {
      areg[ks] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_voff[0], (u * 128 + ks * 32) * 2, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto load_scales = [&](int u) {
    if constexpr (GROUPED) {  // one group per unit
      sc[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff, u * N * 2, 0);
      sc[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff + 16, u * N * 2, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto stage_load = [&](int u) {
    if constexpr (STAGED) {
      u = min(u, total_units - 1);  // a unit past the slice: fetched again, never read
#pragma unroll
      for (int i = 0; i < MT; ++i) areg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_voff[i], u * 256, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto stage_store = [&](char* buf) {
    if constexpr (STAGED) {
#pragma unroll
      for (int i = 0; i < MT; ++i) *reinterpret_cast<u32x4*>(buf + a_lds[i]) = areg[i];
    }
  };

  f32x4 acc[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // consumes the ring (activations: areg, or the LDS image buf); reissue: every register set is loaded for unit `next` as soon
  // as it is free
  auto compute_unit = [&](int next, const char* buf, bool reissue) {
    f32x4 gacc[GROUPED ? MT : 1][4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      u32x4 bf[MT];
      if constexpr (STAGED) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          bf[mt] = *reinterpret_cast<const u32x4*>(buf + (16 * mt + r) * 256 + (((4 * ks + g) ^ r) * 16));
      } else {
        bf[0] = areg[ks];
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int t = 2 * h; t < 2 * h + 2; ++t) {
          const u32x4 wf = w8_fragment<scalar_t>(q[ks][h][2 * (t & 1)], q[ks][h][2 * (t & 1) + 1]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            if constexpr (GROUPED) gacc[mt][t] = mfma_w4<scalar_t>(wf, bf[mt], ks == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : gacc[mt][t]);
            else acc[mt][t] = mfma_w4<scalar_t>(wf, bf[mt], acc[mt][t]);
          }
        }
        if (reissue) load_half(next, ks, h);
      }
      if (reissue) load_a(next, ks);
    }
    if constexpr (GROUPED) {
      union { u32x4 v[2]; scalar_t e[16]; } raw;
      raw.v[0] = sc[0];
      raw.v[1] = sc[1];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float sv = Scalar<scalar_t>::to_f32(raw.e[4 * t + j]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt][t][j] = __builtin_fmaf(sv, gacc[mt][t][j], acc[mt][t][j]);
        }
      if (reissue) load_scales(next);
    }
  };

  if (u0 < u1) {
    stage_load(u0);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      load_half(u0, ks, 0);
      load_half(u0, ks, 1);
      load_a(u0, ks);
    }
    load_scales(u0);
    int cur = 0;  // the image this unit reads; the other one is written for the next
    if constexpr (STAGED) {
      stage_store(smem);
      stage_load(u0 + 1);
      __syncthreads();
    }
    // A unit reads the image written before the previous barrier and writes the other one, which every wave finished reading
    // before that same barrier.
    int u = u0;
    for (; u + 1 < u1; ++u) {
      compute_unit(u + 1, smem + cur, true);
      if constexpr (STAGED) {
        cur ^= kTile;
        stage_store(smem + cur);
        stage_load(u + 2);
        __syncthreads();
      }
    }
    compute_unit(u, smem + cur, false);
  }

  // ---- epilogue (as w4a16_gemm_kernel) ----
  scalar_t* const cptr = reinterpret_cast<scalar_t*>(p.c);
  if constexpr (STAGED) {
    if (!col_ok) return;
    union { u32x4 v[2]; scalar_t e[16]; } cs;
    if constexpr (!GROUPED) {
      cs.v[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff, 0, 0);
      cs.v[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff + 16, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m0 + 16 * mt + r;
      if (m >= M) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 v = acc[mt][t];
        if constexpr (!GROUPED) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] *= Scalar<scalar_t>::to_f32(cs.e[4 * t + j]);
        }
        const int64_t off = (int64_t)m * N + cg * 64 + 16 * t + 4 * g;
        if (p.k_splits == 1) {
          union { scalar_t h[4]; u32x2 u; } o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o.h[j] = Scalar<scalar_t>::from_f32(v[j]);
          *reinterpret_cast<u32x2*>(cptr + off) = o.u;
        } else {
          *reinterpret_cast<f32x4*>(p.partial + (int64_t)split * M * N + off) = v;
        }
      }
    }
  } else {
    // sum the NW K slices through LDS: thread e < 256 owns float4 e of the workgroup's [4 tiles][64 lanes] image
    f32x4* red = reinterpret_cast<f32x4*>(smem);
#pragma unroll
    for (int t = 0; t < 4; ++t) red[(wave * 4 + t) * 64 + lane] = acc[0][t];
    __syncthreads();
    for (int e = threadIdx.x; e < 256; e += 64 * NW) {
      f32x4 v = red[e];
#pragma unroll
      for (int w = 1; w < NW; ++w) v += red[w * 256 + e];
      const int t = e >> 6, el = e & 63, eg = el >> 4;
      const int m = m0 + (el & 15);
      if (m >= M) continue;
      if constexpr (!GROUPED) {
        union { u32x2 u; scalar_t e[4]; } cs;
        cs.u = *reinterpret_cast<const u32x2*>(reinterpret_cast<const scalar_t*>(p.scales) + (cg * 4 + eg) * 16 + 4 * t);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] *= Scalar<scalar_t>::to_f32(cs.e[j]);
      }
      const int64_t off = (int64_t)m * N + cg * 64 + 16 * t + 4 * eg;
      if (p.k_splits == 1) {
        union { scalar_t h[4]; u32x2 u; } o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.h[j] = Scalar<scalar_t>::from_f32(v[j]);
        *reinterpret_cast<u32x2*>(cptr + off) = o.u;
      } else {
        *reinterpret_cast<f32x4*>(p.partial + (int64_t)split * M * N + off) = v;
      }
    }
  }
}

// ---- dispatch --------------------------------------------------------------------------------------------------------
// mt: 16-row tiles per workgroup (1: the unstaged form, 2 / 4: staged, 8: the tall kernel), nw: waves of the unstaged form
// (4 / 8), splits: K splits across workgroups - only to fill the 256 CUs, and only while every wave keeps >= 2 units (the tall
// kernel: >= 4). NMX_W4A16 = "mt,nw,splits" forces any of them for sweeps and tests (0 = keep the default).
// tall = false (the zero-point form has no 128-row kernel): a forced mt = 8 falls to 4, as at 8 bits.
W4Cfg w4_pick(int M, int N, int K, bool tall = true) {
  W4Cfg c;
  // Measured (tools/lean_sweep.py N: family, Llama-3-8B shapes): the unstaged form wins at M = 1 everywhere and
  // at M = 16 on qkv / o; at M = 16 the big matrices (down, gate_up: >= 24 MiB of weights) take the staged 32-row tile
  // (16.9 vs 19.3 us, 9.9 vs 10.7), and at M = 64 the small ones (qkv, o) take two 32-row blocks (10.9 vs 11.6, 7.9 vs 9.7).
  const bool big = (int64_t)K * N / 2 >= (24ll << 20);
  c.mt = M <= 8 ? 1 : (M <= 16 ? (big ? 2 : 1) : (M <= 32 ? 2 : (M <= 64 && !big ? 2 : 4)));
  // The tall kernel (mt = 8) is never the default: at one workgroup per CU it beat MT = 4 on one measured point only (gate_up
  // at M = 256, fp16 group 128, 82.2 vs 85.1 us) and loses by 1.1 - 1.7x on every other shape at M = 128 / 256
  // (profiles/w4a16_tall_ab.txt); bf16 and channel-wise were not measured and its bf16 GROUPED form spills.
  c.nw = 4;
  c.splits = 1;
  int f_mt = 0, f_nw = 0, f_splits = 0;
  if (const char* e = nmx_tune(NMX_TUNE_W4A16)) sscanf(e, "%d,%d,%d", &f_mt, &f_nw, &f_splits);
  if (f_mt == 1 || f_mt == 2 || f_mt == 4 || f_mt == 8) c.mt = f_mt;
  if (c.mt == 8 && !tall) c.mt = 4;
  if (c.mt == 1 && f_nw == 8) c.nw = 8;
  const int units = K / 128, groups = N / 64;
  const int row_blocks = ceil_div(M, 16 * c.mt);
  const int wgs = (c.mt == 1 ? groups : ceil_div(groups, 4)) * row_blocks;
  const int slices = c.mt == 1 ? c.nw : 1;
  const int min_units = c.mt == 8 ? 4 : 2;
  while (wgs * c.splits * 2 <= 256 && units / (slices * c.splits * 2) >= min_units && c.splits < 16) c.splits *= 2;
  if (f_splits >= 1) c.splits = f_splits;
  c.splits = std::max(1, std::min(std::min(c.splits, units), 64));
  return c;
}

template <typename scalar_t, bool GROUPED, bool ZP = false>
int w4_launch(const W4Params& p, const W4Cfg& cfg, hipStream_t stream) {
  const int C = p.N / 64;
  const int ncolwg = cfg.mt == 1 ? C : ceil_div(C, 4);
  dim3 grid(ncolwg, p.k_splits, ceil_div(p.M, 16 * cfg.mt));
  if (p.xcd_per > 0) grid = dim3(ceil_div(ncolwg, p.xcd_per) * 8, 1, grid.z);
  if (!ZP && cfg.mt == 8) w4a16_tall_kernel<scalar_t, GROUPED><<<grid, 256, 0, stream>>>(p);  // (ZP: w4_pick never says 8)
  else if (cfg.mt == 1 && cfg.nw == 8) w4a16_gemm_kernel<scalar_t, 1, 8, GROUPED, false, ZP><<<grid, 512, 0, stream>>>(p);
  else if (cfg.mt == 1) w4a16_gemm_kernel<scalar_t, 1, 4, GROUPED, false, ZP><<<grid, 256, 0, stream>>>(p);
  else if (cfg.mt == 2) w4a16_gemm_kernel<scalar_t, 2, 4, GROUPED, true, ZP><<<grid, 256, 0, stream>>>(p);
  else w4a16_gemm_kernel<scalar_t, 4, 4, GROUPED, true, ZP><<<grid, 256, 0, stream>>>(p);
  NMX_LAUNCH_CHECK();
  return NMX_OK;
}

// The 8-bit dispatch: w4_pick's rules (same override, same split rule) without the tall form - a forced mt = 8 falls to 4.
W4Cfg w8_pick(int M, int N, int K) {
  W4Cfg c;
  // Thresholds in weight BYTES (K * N at 8 bits). Measured (tools/lean_sweep.py, LEAN_SWEEP_BITS=8, Llama-3-8B shapes, fp16 group
  // 128, M = 1 / 16 / 64; DESIGN.md 3.1n8, profiles/w8a16_native_ab.txt): M = 1 the unstaged form everywhere; M = 16 the 24 MiB
  // threshold carried over from w4_pick holds (o, 16 MiB: MT = 1 5.5 vs 6.3 us; qkv, 24 MiB: level; down, gate_up: MT = 2 12.7 vs
  // 13.0, 20.5 vs 23.4); M = 64 two 32-row blocks win up to down's 56 MiB (qkv 11.2 vs 11.7, o 8.3 vs 9.7, down 17.6 vs 18.0 -
  // 18.9) and MT = 4 on gate_up's 112 MiB (29.5 vs 31.5): the threshold there is put at 64 MiB. M = 8 and 32 are carried over
  // from w4_pick, not measured.
  const int64_t bytes = (int64_t)K * N;
  const bool big = bytes >= (24ll << 20);
  c.mt = M <= 8 ? 1 : (M <= 16 ? (big ? 2 : 1) : (M <= 32 ? 2 : (M <= 64 && bytes < (64ll << 20) ? 2 : 4)));
  c.nw = 4;
  c.splits = 1;
  int f_mt = 0, f_nw = 0, f_splits = 0;
  if (const char* e = nmx_tune(NMX_TUNE_W4A16)) sscanf(e, "%d,%d,%d", &f_mt, &f_nw, &f_splits);
  if (f_mt == 1 || f_mt == 2 || f_mt == 4) c.mt = f_mt;
  if (f_mt == 8) c.mt = 4;  // no 128-row form at 8 bits
  if (c.mt == 1 && f_nw == 8) c.nw = 8;
  const int units = K / 128, groups = N / 64;
  const int row_blocks = ceil_div(M, 16 * c.mt);
  const int wgs = (c.mt == 1 ? groups : ceil_div(groups, 4)) * row_blocks;
  const int slices = c.mt == 1 ? c.nw : 1;
  while (wgs * c.splits * 2 <= 256 && units / (slices * c.splits * 2) >= 2 && c.splits < 16) c.splits *= 2;
  // 8 waves where the 4-wave grid already has a workgroup or more per CU and so gets no K split: twice the weight bytes in flight
  // per CU (measured on gate_up at M = 1 only: 19.7 vs 21.1 us; with a K split, as on qkv / o / down, 4 waves win)
  if (c.mt == 1 && f_nw == 0 && c.splits == 1 && wgs >= 256 && units >= 16) c.nw = 8;
  if (f_splits >= 1) c.splits = f_splits;
  c.splits = std::max(1, std::min(std::min(c.splits, units), 64));
  return c;
}

template <typename scalar_t, bool GROUPED>
int w8_launch(const W4Params& p, const W4Cfg& cfg, hipStream_t stream) {
  const int C = p.N / 64;
  const int ncolwg = cfg.mt == 1 ? C : ceil_div(C, 4);
  dim3 grid(ncolwg, p.k_splits, ceil_div(p.M, 16 * cfg.mt));
  if (p.xcd_per > 0) grid = dim3(ceil_div(ncolwg, p.xcd_per) * 8, 1, grid.z);
  if (cfg.mt == 1 && cfg.nw == 8) w8a16_gemm_kernel<scalar_t, 1, 8, GROUPED, false><<<grid, 512, 0, stream>>>(p);
  else if (cfg.mt == 1) w8a16_gemm_kernel<scalar_t, 1, 4, GROUPED, false><<<grid, 256, 0, stream>>>(p);
  else if (cfg.mt == 2) w8a16_gemm_kernel<scalar_t, 2, 4, GROUPED, true><<<grid, 256, 0, stream>>>(p);
  else w8a16_gemm_kernel<scalar_t, 4, 4, GROUPED, true><<<grid, 256, 0, stream>>>(p);
  NMX_LAUNCH_CHECK();
  return NMX_OK;
}

// zeros_native != nullptr: the zero-point form (4 bits, fp16, one group per 128 k)
int w4_common(int bits, const void* a, const int32_t* qweight_native, const void* scales_native, void* c, void* scratch,
              int64_t scratch_bytes, int size_m, int size_n, int size_k, int num_groups, int dtype, int defer,
              int* splits_out, hipStream_t stream, const void* zeros_native = nullptr) {
  if (splits_out != nullptr) *splits_out = 1;
  if (zeros_native != nullptr) {
    NMX_CHECK(dtype == NMX_F16, NMX_ERR_UNSUPPORTED, "w4a16_zp_gemm only supports float16");
    NMX_CHECK(nmx_awq_native_supported(size_n, size_k, num_groups), NMX_ERR_UNSUPPORTED,
              "w4a16_zp_gemm: size_k = %d must be a multiple of 128, size_n = %d of 64, num_groups = %d size_k / 128", size_k, size_n,
              num_groups);
    NMX_CHECK((uintptr_t)zeros_native % 8 == 0, NMX_ERR_INVALID_ARG, "w4a16_zp_gemm: zeros_native must be 8-byte aligned");
  }
  NMX_CHECK(dtype == NMX_F16 || dtype == NMX_BF16, NMX_ERR_UNSUPPORTED, "w4a16_gemm only supports bfloat16 and float16");
  NMX_CHECK(size_m >= 0 && size_n > 0 && size_k > 0, NMX_ERR_INVALID_ARG, "w4a16_gemm: size_m = %d, size_n = %d, size_k = %d", size_m,
            size_n, size_k);
  NMX_CHECK(nmx_w4a16_supported(size_n, size_k, num_groups, bits, 0), NMX_ERR_UNSUPPORTED,
            "w4a16_gemm: size_k = %d must be a multiple of 128, size_n = %d of 64, num_groups = %d one or size_k / 128", size_k, size_n,
            num_groups);
  NMX_CHECK((int64_t)size_m * size_k * 2 <= 0x7ff00000ll && (int64_t)size_k * size_n * bits < (1ll << 34) && (int64_t)size_m * size_n < (1ll << 31),
            NMX_ERR_UNSUPPORTED, "w4a16_gemm: operand beyond the 2 GiB a buffer descriptor addresses");
  NMX_CHECK(a != nullptr && qweight_native != nullptr && scales_native != nullptr && c != nullptr, NMX_ERR_INVALID_ARG,
            "w4a16_gemm: null operand");
  NMX_CHECK(((uintptr_t)a % 16 == 0) && ((uintptr_t)qweight_native % 16 == 0) && ((uintptr_t)scales_native % 16 == 0) &&
                ((uintptr_t)c % 8 == 0) && ((uintptr_t)scratch % 16 == 0),
            NMX_ERR_INVALID_ARG, "w4a16_gemm: operands must be 16-byte aligned");
  if (size_m == 0) return NMX_OK;
  W4Cfg cfg = bits == 8 ? w8_pick(size_m, size_n, size_k) : w4_pick(size_m, size_n, size_k, zeros_native == nullptr);
  const int64_t slab = (int64_t)size_m * size_n * sizeof(float);
  if (scratch == nullptr) scratch_bytes = 0;
  if ((int64_t)cfg.splits * slab > scratch_bytes) cfg.splits = (int)std::max<int64_t>(1, scratch_bytes / slab);  // fewer splits, never past the scratch
  W4Params p;
  p.a = a; p.qw = qweight_native; p.scales = scales_native; p.c = c; p.partial = reinterpret_cast<float*>(scratch);
  p.M = size_m; p.N = size_n; p.K = size_k; p.num_groups = num_groups; p.k_splits = cfg.splits; p.zeros = zeros_native;
  const char* xs = nmx_tune(NMX_TUNE_GEMM_XCD_SPLIT);
  const bool xcd = (xs == nullptr || atoi(xs) != 0) && (cfg.splits == 2 || cfg.splits == 4 || cfg.splits == 8);
  p.xcd_per = xcd ? 8 / cfg.splits : 0;
  int rc;
  if (zeros_native != nullptr) rc = w4_launch<f16, true, true>(p, cfg, stream);
  else if (bits == 8) {
    if (dtype == NMX_F16) rc = num_groups > 1 ? w8_launch<f16, true>(p, cfg, stream) : w8_launch<f16, false>(p, cfg, stream);
    else rc = num_groups > 1 ? w8_launch<bf16, true>(p, cfg, stream) : w8_launch<bf16, false>(p, cfg, stream);
  } else if (dtype == NMX_F16) rc = num_groups > 1 ? w4_launch<f16, true>(p, cfg, stream) : w4_launch<f16, false>(p, cfg, stream);
  else rc = num_groups > 1 ? w4_launch<bf16, true>(p, cfg, stream) : w4_launch<bf16, false>(p, cfg, stream);
  if (rc != NMX_OK || cfg.splits == 1) return rc;
  if (defer) {
    *splits_out = cfg.splits;
    return NMX_OK;
  }
  return nmx_splitk_reduce(c, p.partial, cfg.splits, size_m, size_n, dtype, stream);
}

}  // namespace

extern "C" int nmx_w4a16_supported(int size_n, int size_k, int num_groups, int num_bits, int has_act_order) {
  return (num_bits == 4 || num_bits == 8) && !has_act_order && size_n > 0 && size_k > 0 && size_k % 128 == 0 && size_n % 64 == 0 &&
                 (num_groups == 1 || num_groups == size_k / 128)
             ? 1 : 0;
}

extern "C" int nmx_w4a16_repack(const int32_t* qweight, const void* scales, int32_t* qweight_native, void* scales_native,
                                int size_k, int size_n, int num_groups, int dtype, nmx_stream_t stream) {
  NMX_CHECK(dtype == NMX_F16 || dtype == NMX_BF16, NMX_ERR_UNSUPPORTED, "w4a16_repack only supports bfloat16 and float16 scales");
  NMX_CHECK(nmx_w4a16_supported(size_n, size_k, num_groups, 4, 0), NMX_ERR_UNSUPPORTED,
            "w4a16_repack: size_k = %d must be a multiple of 128, size_n = %d of 64, num_groups = %d one or size_k / 128", size_k, size_n,
            num_groups);
  NMX_CHECK(qweight != nullptr && scales != nullptr && qweight_native != nullptr && scales_native != nullptr &&
                qweight != qweight_native && scales != scales_native,
            NMX_ERR_INVALID_ARG, "w4a16_repack: null or aliased operand");
  const int64_t words = (int64_t)(size_k / 8) * size_n;
  w4a16_repack_kernel<<<(unsigned)ceil_div64(words, 256), 256, 0, (hipStream_t)stream>>>(
      reinterpret_cast<const uint32_t*>(qweight), reinterpret_cast<const uint16_t*>(scales), reinterpret_cast<uint32_t*>(qweight_native),
      reinterpret_cast<uint16_t*>(scales_native), size_k, size_n, num_groups);
  NMX_LAUNCH_CHECK();
  return NMX_OK;
}

extern "C" int nmx_w4a16_gemm_plan(int size_m, int size_n, int size_k, int* mt, int* nw, int* splits) {
  NMX_CHECK(mt != nullptr && nw != nullptr && splits != nullptr, NMX_ERR_INVALID_ARG, "w4a16_gemm_plan: null output");
  NMX_CHECK(size_m > 0 && size_n > 0 && size_k >= 128, NMX_ERR_INVALID_ARG, "w4a16_gemm_plan: size_m = %d, size_n = %d, size_k = %d", size_m,
            size_n, size_k);
  const W4Cfg c = w4_pick(size_m, size_n, size_k);
  *mt = c.mt;
  *nw = c.nw;
  *splits = c.splits;
  return NMX_OK;
}

extern "C" int64_t nmx_w4a16_gemm_scratch_bytes(int size_m, int size_n, int size_k) {
  if (size_m <= 0 || size_n <= 0 || size_k < 128) return 0;
  const int splits = w4_pick(size_m, size_n, size_k).splits;
  return splits > 1 ? (int64_t)splits * size_m * size_n * sizeof(float) : 0;
}

extern "C" int nmx_w4a16_gemm(const void* a, const int32_t* qweight_native, const void* scales_native, void* c, void* scratch,
                              int64_t scratch_bytes, int size_m, int size_n, int size_k, int num_groups, int dtype,
                              nmx_stream_t stream) {
  return w4_common(4, a, qweight_native, scales_native, c, scratch, scratch_bytes, size_m, size_n, size_k, num_groups, dtype, 0, nullptr,
                   (hipStream_t)stream);
}

extern "C" int nmx_w4a16_gemm_deferred(const void* a, const int32_t* qweight_native, const void* scales_native, void* c, void* scratch,
                                       int64_t scratch_bytes, int size_m, int size_n, int size_k, int num_groups, int dtype,
                                       int* splits_out, nmx_stream_t stream) {
  NMX_CHECK(splits_out != nullptr, NMX_ERR_INVALID_ARG, "splits_out is null");
  return w4_common(4, a, qweight_native, scales_native, c, scratch, scratch_bytes, size_m, size_n, size_k, num_groups, dtype, 1, splits_out,
                   (hipStream_t)stream);
}

// ---- zero points (AWQ): the same entries with zeros_native; no 128-row form ----
extern "C" int nmx_awq_native_supported(int size_n, int size_k, int num_groups) {
  return nmx_w4a16_supported(size_n, size_k, num_groups, 4, 0) && num_groups == size_k / 128 ? 1 : 0;
}

extern "C" int nmx_awq_native_repack(const int32_t* qweight, const int32_t* qzeros, const void* scales, int32_t* qweight_native,
                                     void* scales_native, void* zeros_native, int size_k, int size_n, int num_groups,
                                     nmx_stream_t stream) {
  NMX_CHECK(nmx_awq_native_supported(size_n, size_k, num_groups), NMX_ERR_UNSUPPORTED,
            "awq_native_repack: size_k = %d must be a multiple of 128, size_n = %d of 64, num_groups = %d size_k / 128", size_k, size_n,
            num_groups);
  NMX_CHECK(qweight != nullptr && qzeros != nullptr && scales != nullptr && qweight_native != nullptr && scales_native != nullptr &&
                zeros_native != nullptr && qweight != qweight_native && scales != scales_native,
            NMX_ERR_INVALID_ARG, "awq_native_repack: null or aliased operand");
  const int64_t blocks = (int64_t)(size_k / 128) * ceil_div(size_n / 64, 4);
  NMX_CHECK(blocks < (1ll << 31), NMX_ERR_UNSUPPORTED, "awq_native_repack: weight too large");
  awq_native_repack_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(
      reinterpret_cast<const uint32_t*>(qweight), reinterpret_cast<const uint32_t*>(qzeros), reinterpret_cast<const uint16_t*>(scales),
      reinterpret_cast<uint32_t*>(qweight_native), reinterpret_cast<uint16_t*>(scales_native), reinterpret_cast<uint16_t*>(zeros_native),
      size_k, size_n);
  NMX_LAUNCH_CHECK();
  return NMX_OK;
}

extern "C" int nmx_w4a16_zp_gemm_plan(int size_m, int size_n, int size_k, int* mt, int* nw, int* splits) {
  NMX_CHECK(mt != nullptr && nw != nullptr && splits != nullptr, NMX_ERR_INVALID_ARG, "w4a16_zp_gemm_plan: null output");
  NMX_CHECK(size_m > 0 && size_n > 0 && size_k >= 128, NMX_ERR_INVALID_ARG, "w4a16_zp_gemm_plan: size_m = %d, size_n = %d, size_k = %d",
            size_m, size_n, size_k);
  const W4Cfg c = w4_pick(size_m, size_n, size_k, false);
  *mt = c.mt;
  *nw = c.nw;
  *splits = c.splits;
  return NMX_OK;
}

extern "C" int64_t nmx_w4a16_zp_gemm_scratch_bytes(int size_m, int size_n, int size_k) {
  if (size_m <= 0 || size_n <= 0 || size_k < 128) return 0;
  const int splits = w4_pick(size_m, size_n, size_k, false).splits;
  return splits > 1 ? (int64_t)splits * size_m * size_n * sizeof(float) : 0;
}

extern "C" int nmx_w4a16_zp_gemm(const void* a, const int32_t* qweight_native, const void* scales_native, const void* zeros_native,
                                 void* c, void* scratch, int64_t scratch_bytes, int size_m, int size_n, int size_k, int num_groups,
                                 int dtype, nmx_stream_t stream) {
  NMX_CHECK(zeros_native != nullptr, NMX_ERR_INVALID_ARG, "w4a16_zp_gemm: null operand");
  return w4_common(4, a, qweight_native, scales_native, c, scratch, scratch_bytes, size_m, size_n, size_k, num_groups, dtype, 0, nullptr,
                   (hipStream_t)stream, zeros_native);
}

extern "C" int nmx_w4a16_zp_gemm_deferred(const void* a, const int32_t* qweight_native, const void* scales_native,
                                          const void* zeros_native, void* c, void* scratch, int64_t scratch_bytes, int size_m,
                                          int size_n, int size_k, int num_groups, int dtype, int* splits_out, nmx_stream_t stream) {
  NMX_CHECK(splits_out != nullptr, NMX_ERR_INVALID_ARG, "splits_out is null");
  NMX_CHECK(zeros_native != nullptr, NMX_ERR_INVALID_ARG, "w4a16_zp_gemm: null operand");
  return w4_common(4, a, qweight_native, scales_native, c, scratch, scratch_bytes, size_m, size_n, size_k, num_groups, dtype, 1, splits_out,
                   (hipStream_t)stream, zeros_native);
}

// ---- 8 bits: the same entries on the 8-bit form of the layout ----
extern "C" int nmx_w8a16_repack(const int32_t* qweight, const void* scales, int32_t* qweight_native, void* scales_native,
                                int size_k, int size_n, int num_groups, int dtype, nmx_stream_t stream) {
  NMX_CHECK(dtype == NMX_F16 || dtype == NMX_BF16, NMX_ERR_UNSUPPORTED, "w8a16_repack only supports bfloat16 and float16 scales");
  NMX_CHECK(nmx_w4a16_supported(size_n, size_k, num_groups, 8, 0), NMX_ERR_UNSUPPORTED,
            "w8a16_repack: size_k = %d must be a multiple of 128, size_n = %d of 64, num_groups = %d one or size_k / 128", size_k, size_n,
            num_groups);
  NMX_CHECK(qweight != nullptr && scales != nullptr && qweight_native != nullptr && scales_native != nullptr &&
                qweight != qweight_native && scales != scales_native,
            NMX_ERR_INVALID_ARG, "w8a16_repack: null or aliased operand");
  const int64_t words = (int64_t)(size_k / 4) * size_n;
  w8a16_repack_kernel<<<(unsigned)ceil_div64(words, 256), 256, 0, (hipStream_t)stream>>>(
      reinterpret_cast<const uint32_t*>(qweight), reinterpret_cast<const uint16_t*>(scales), reinterpret_cast<uint32_t*>(qweight_native),
      reinterpret_cast<uint16_t*>(scales_native), size_k, size_n, num_groups);
  NMX_LAUNCH_CHECK();
  return NMX_OK;
}

extern "C" int nmx_w8a16_gemm_plan(int size_m, int size_n, int size_k, int* mt, int* nw, int* splits) {
  NMX_CHECK(mt != nullptr && nw != nullptr && splits != nullptr, NMX_ERR_INVALID_ARG, "w8a16_gemm_plan: null output");
  NMX_CHECK(size_m > 0 && size_n > 0 && size_k >= 128, NMX_ERR_INVALID_ARG, "w8a16_gemm_plan: size_m = %d, size_n = %d, size_k = %d", size_m,
            size_n, size_k);
  const W4Cfg c = w8_pick(size_m, size_n, size_k);
  *mt = c.mt;
  *nw = c.nw;
  *splits = c.splits;
  return NMX_OK;
}

extern "C" int64_t nmx_w8a16_gemm_scratch_bytes(int size_m, int size_n, int size_k) {
  if (size_m <= 0 || size_n <= 0 || size_k < 128) return 0;
  const int splits = w8_pick(size_m, size_n, size_k).splits;
  return splits > 1 ? (int64_t)splits * size_m * size_n * sizeof(float) : 0;
}

extern "C" int nmx_w8a16_gemm(const void* a, const int32_t* qweight_native, const void* scales_native, void* c, void* scratch,
                              int64_t scratch_bytes, int size_m, int size_n, int size_k, int num_groups, int dtype,
                              nmx_stream_t stream) {
  return w4_common(8, a, qweight_native, scales_native, c, scratch, scratch_bytes, size_m, size_n, size_k, num_groups, dtype, 0, nullptr,
                   (hipStream_t)stream);
}

extern "C" int nmx_w8a16_gemm_deferred(const void* a, const int32_t* qweight_native, const void* scales_native, void* c, void* scratch,
                                       int64_t scratch_bytes, int size_m, int size_n, int size_k, int num_groups, int dtype,
                                       int* splits_out, nmx_stream_t stream) {
  NMX_CHECK(splits_out != nullptr, NMX_ERR_INVALID_ARG, "splits_out is null");
  return w4_common(8, a, qweight_native, scales_native, c, scratch, scratch_bytes, size_m, size_n, size_k, num_groups, dtype, 1, splits_out,
                   (hipStream_t)stream);
}
