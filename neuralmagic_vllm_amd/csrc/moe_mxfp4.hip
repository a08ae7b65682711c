// Grouped MXFP4 GEMM over expert-sorted rows on the block-scaled fp4 MFMA (include/nmx.h "MXFP4 mixture-of-experts", DESIGN.md
// 3.1mf4): the expert GEMMs of an MXFP4 MoE layer as ONE launch each, and silu_and_mul fused with the activation quantiser.
// The weights are the stacked outputs of nmx_mxfp4_repack, one (qweight_native, scales_native) pair per expert. Unlike
// mxfp4_gemm_kernel the activations arrive QUANTISED - codes and E8M0 bytes in the format nmx_mxfp4_quant writes: a token row is
// gathered by topk experts times every column workgroup, and quantising it in the loop would repeat that work tens to hundreds of
// times. The loop has no conversion VALU at all; the gather is 16 code bytes + 1 scale byte per lane and unit.
//
//   out[id, :] = cast((A[id / a_row_div, :] . W_e^T) * [topk_weights[id]])
//   for every sorted pair id of block z (block_rows entries of sorted_token_ids), e = expert_ids[z]; A and W_e as dequantised.
#include "mxfp4_fragment.h"

#include <stdlib.h>

#include <utility>

namespace {

struct MoeMxParams {
  const uint8_t* a_q;          // [a_rows, K / 2] codes
  const uint8_t* a_scale;      // [a_rows, K / 32] E8M0 bytes
  const uint8_t* qw;           // [E][K / 128][64 N] qweight_native per expert
  const int32_t* scales;       // [E][K / 128][N] scales_native per expert
  void* out;                   // [num_valid, N]
  float* partial;              // [k_splits, num_valid, N] fp32 slabs (k_splits > 1)
  const float* topk_weights;   // [num_valid] or null
  const int32_t* sorted_token_ids;
  const int32_t* expert_ids;
  const int32_t* num_tokens_post_padded;
  int N, K, k_splits, num_valid, a_rows, a_row_div, num_experts;
};

// MT = 1 (block_rows = 16, unstaged): 4 waves on ONE 64-column group of the block's expert, every wave its own K slice in units of
//   128 k. Per unit lane (g, r) loads 4 weight chunks (dwordx4, non-temporal), the weight-scale dword, its B operand - the 16 code
//   bytes of row sorted_token_ids[16 z + r] / a_row_div at block 4 u + g - and that block's scale BYTE (buffer_load_ubyte: it
//   lands zero-extended in byte 0, where the MFMA's op_sel 0 reads it, with no shift by g), then issues 4 MFMAs that share B. The
//   row offsets are loop invariants; the 4 slices are summed through LDS with one barrier.
// MT = 2 / 4 (block_rows = 32 / 64, staged): 4 waves on 4 ADJACENT column groups sharing one K slice. Wave w < MT copies row tile
//   w a unit ahead - one dwordx4 and one byte per lane, through registers - into the fragment-ordered image of 3.1f4 (chunk
//   64 mt + lane, the scale bytes behind the chunks, 1088 MT bytes, double-buffered, one barrier per unit): writes and reads are
//   1 KiB linear per wave. A wave past N / 64 computes a valid group, stores nothing.
// Padding slots (id >= num_valid) get an offset past both activation descriptors: code 0, scale 0, never stored.
// Weights never touch LDS: one raw_buffer_load per lane and tile in one fixed issue order, two units ahead, through descriptors
// whose base is the block's expert (64-bit arithmetic) and whose range is that one expert's tensor.
// Grid: x = column workgroups, y = K split, z = block. k_splits > 1: the routing-weighted fp32 results go to slab [y, num_valid, N];
// every valid id is written by exactly one block in every split, so the slabs need no zeroing.
template <typename scalar_t, int MT>
__global__ __launch_bounds__(256, 2) void moe_mxfp4_kernel(const MoeMxParams p) {
  constexpr bool STAGED = MT > 1;
  constexpr int BR = 16 * MT, NW = 4;
  const int blk = blockIdx.z;
  if (blk * BR >= p.num_tokens_post_padded[0]) return;  // the whole workgroup, before any barrier
  const int expert = __builtin_amdgcn_readfirstlane(min(max(p.expert_ids[blk], 0), p.num_experts - 1));
  const int32_t* const ids = p.sorted_token_ids + blk * BR;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int N = p.N, K = p.K;
  const int C = N / 64, total_units = K / 128;

  const int cg = STAGED ? blockIdx.x * 4 + wave : blockIdx.x;
  const bool col_ok = cg < C;
  const int cl = min(cg, C - 1);  // column group used for the loads (a wave past N computes a valid group again, never stored)
  const int split = blockIdx.y;

  // K slice in units of 128 k
  constexpr int SLICES = STAGED ? 1 : NW;
  const int workers = p.k_splits * SLICES;
  const int per = (total_units + workers - 1) / workers;
  const int worker = split * SLICES + (STAGED ? 0 : wave);
  const int u0 = min(worker * per, total_units), u1 = min(u0 + per, total_units);

  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.qw + (int64_t)expert * (K / 2) * N), 0, (K / 2) * N, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<int32_t*>(p.scales + (int64_t)expert * total_units * N), 0, total_units * C * 256, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.a_q), 0, p.a_rows * (K / 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_as = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.a_scale), 0, p.a_rows * (K / 32), 0x00020000);
  const int unit_bytes = C * 4096;  // one 128-k unit of all column groups
  const int w_voff = cl * 4096 + lane * 16;
  const int s_voff = (cl * 64 + lane) * 4;
  constexpr int kPast = 0x7ff00000;  // beyond every descriptor: the load returns zeros
  // the lane's block of a unit: row r of the wave's row tile (unstaged: the only one; staged: tile `wave`, stagers only), block g
  const bool stager = STAGED && wave < MT;
  int a_voff = kPast, as_voff = kPast;
  if (!STAGED || stager) {
    const int id = ids[(STAGED ? 16 * wave : 0) + r];
    if (id >= 0 && id < p.num_valid) {
      const int row = id / p.a_row_div;
      a_voff = row * (K / 2) + 16 * g;
      as_voff = row * (K / 32) + g;
    }
  }

  constexpr int kImg = MT * 1088;  // staged image of one unit: 64 MT chunks of 16 bytes, then 64 MT scale bytes
  __shared__ __attribute__((aligned(16))) char smem[STAGED ? 2 * kImg : NW * 4096];

  struct Unit {
    u32x4 q[4];
    uint32_t s;
    u32x4 b;      // unstaged: the lane's B operand
    uint8_t bs;   //           and its scale byte, widened only where it is consumed: a zero-extension next to the load makes the
  };              //           compiler wait for the unit's loads two units early (seen in the generated code as s_waitcnt vmcnt(1))
  // loads of tile t / the scale word and the activations of unit u (past the slice: the last unit again, never consumed).
  // sched_barrier pins the issue order: prologue and loop must queue the loads alike, or the merged wait counts at the loop head
  // degrade. The activations are issued LAST: every MFMA of a unit reads them, so their registers are free only after tile 3.
  auto load_tile = [&](int u, int t, Unit& U) {
    u = min(u, total_units - 1);
    U.q[t] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, w_voff, u * unit_bytes + t * 1024, 2);  // aux 2: non-temporal
    __builtin_amdgcn_sched_barrier(0);
  };
  auto load_scales = [&](int u, Unit& U) {
    u = min(u, total_units - 1);
    U.s = __builtin_amdgcn_raw_buffer_load_b32(rs_s, s_voff, u * C * 256, 0);
    if constexpr (!STAGED) {
      U.b = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_voff, u * 64, 0);
      U.bs = __builtin_amdgcn_raw_buffer_load_b8(rs_as, as_voff, u * 4, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto load_unit = [&](int u, Unit& U) {
#pragma unroll
    for (int t = 0; t < 4; ++t) load_tile(u, t, U);
    load_scales(u, U);
  };
  u32x4 areg;
  uint32_t asreg;
  auto stage_load = [&](int u) {
    if constexpr (STAGED) {
      if (stager) {
        u = min(u, total_units - 1);
        areg = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_voff, u * 64, 0);
        asreg = __builtin_amdgcn_raw_buffer_load_b8(rs_as, as_voff, u * 4, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto stage_store = [&](char* buf) {
    if constexpr (STAGED) {
      if (stager) {
        *reinterpret_cast<u32x4*>(buf + threadIdx.x * 16) = areg;
        *reinterpret_cast<uint8_t*>(buf + MT * 1024 + threadIdx.x) = (uint8_t)asreg;
      }
    }
  };

  f32x4 acc[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // consumes unit U (activations: its own registers, or the LDS image buf) and re-issues each register set for unit `next`
  // as soon as it is free
  auto compute_unit = [&](Unit& U, int next, const char* buf, bool reissue) {
    u32x4 bq[MT];
    uint32_t bs[MT];
    if constexpr (STAGED) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        bq[mt] = *reinterpret_cast<const u32x4*>(buf + (64 * mt + lane) * 16);
        bs[mt] = *reinterpret_cast<const uint8_t*>(buf + MT * 1024 + 64 * mt + lane);
      }
    } else {
      bq[0] = U.b;
      bs[0] = U.bs;
    }
    auto tile = [&](auto tc) {
      constexpr int t = decltype(tc)::value;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt][t] = mx_mfma<t>(U.q[t], U.s, bq[mt], bs[mt], acc[mt][t]);
      if (reissue) load_tile(next, t, U);
    };
    tile(std::integral_constant<int, 0>{});
    tile(std::integral_constant<int, 1>{});
    tile(std::integral_constant<int, 2>{});
    tile(std::integral_constant<int, 3>{});
    if (reissue) load_scales(next, U);
  };

  Unit ua, ub;
  char* const buf0 = smem;
  char* const buf1 = smem + (STAGED ? kImg : 0);
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
    // same barrier. (u0, u1 are the same for the 4 waves of a staged workgroup: every wave meets every barrier.)
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

  // ---- epilogue: routing weight (fp32), scatter to the pair id ----
  scalar_t* const optr = reinterpret_cast<scalar_t*>(p.out);
  float* const slab = p.partial + (int64_t)split * p.num_valid * N;
  // v = the 4 consecutive outputs of row id at column n: one 8-byte store, or 16 bytes into the split's slab
  auto store4 = [&](f32x4 v, int id, int n) {
    if (p.topk_weights != nullptr) v *= p.topk_weights[id];
    const int64_t off = (int64_t)id * N + n;
    if (p.k_splits == 1) {
      union { scalar_t h[4]; u32x2 u; } o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o.h[j] = Scalar<scalar_t>::from_f32(v[j]);
      *reinterpret_cast<u32x2*>(optr + off) = o.u;
    } else {
      *reinterpret_cast<f32x4*>(slab + off) = v;
    }
  };
  if constexpr (STAGED) {
    if (!col_ok) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int id = ids[16 * mt + r];
      if (id < 0 || id >= p.num_valid) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) store4(acc[mt][t], id, cg * 64 + 16 * t + 4 * g);
    }
  } else {
    // sum the 4 K slices through LDS: thread e < 256 owns float4 e of the workgroup's [4 tiles][64 lanes] image
    f32x4* red = reinterpret_cast<f32x4*>(smem);
#pragma unroll
    for (int t = 0; t < 4; ++t) red[(wave * 4 + t) * 64 + lane] = acc[0][t];
    __syncthreads();
    const int e = threadIdx.x;
    f32x4 v = red[e];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += red[w * 256 + e];
    const int t = e >> 6, el = e & 63;
    const int id = ids[el & 15];
    if (id < 0 || id >= p.num_valid) return;
    store4(v, id, cg * 64 + 16 * t + 4 * (el >> 4));
  }
}

// ---- nmx_silu_and_mul_mxfp4_quant: one lane per 32-value block of the result. The lane reads its 64 bytes of gate and of up,
// computes silu_and_mul in act_and_mul_kernel's arithmetic (elementwise.hip: silu in fp32 rounded to scalar_t, times up, rounded
// again) and hands the ROUNDED block to the quantiser: the outputs are those of nmx_mxfp4_quant on nmx_silu_and_mul's output.
template <typename scalar_t>
__global__ __launch_bounds__(256) void silu_and_mul_mxfp4_quant_kernel(const scalar_t* __restrict__ x, u32x4* __restrict__ out_q,
                                                                       uint8_t* __restrict__ out_scale, int inter, int64_t blocks) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= blocks) return;
  const int per_row = inter / 32;
  const int64_t row = b / per_row;
  const int kb = (int)(b - row * per_row);
  const scalar_t* const gate = x + row * 2 * inter + 32 * kb;
  union V { u32x4 u; scalar_t e[8]; };
  V ga[4], up[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ga[i].u = reinterpret_cast<const u32x4*>(gate)[i];
    up[i].u = reinterpret_cast<const u32x4*>(gate + inter)[i];
  }
  u32x4 y[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    V o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.e[j] = rnd_mul<scalar_t>(silu_rnd<scalar_t>(ga[i].e[j]), up[i].e[j]);
    y[i] = o.u;
  }
  uint32_t sb;
  out_q[b] = mx_quant_block<scalar_t>(y, sb);
  out_scale[b] = (uint8_t)sb;
}

// ---- dispatch --------------------------------------------------------------------------------------------------------
// The split rule of moe_w4_splits (moe_w4a16.hip): K splits only fill the 256 CUs. The host knows no histogram, so it takes an
// UPPER estimate of the occupied blocks: sum_e ceil(cnt_e / B) <= (numel + nz (B - 1)) / B with nz = min(E, numel) experts hit.
// Every wave keeps >= 2 units, at most 4 splits. NMX_MOE_MXFP4 = "splits" forces 1, 2 or 4 (sweeps and tests).
int moe_mx_splits(int num_valid, int n, int k, int num_experts, int block_rows) {
  const int units = k / 128, groups = n / 64;
  const int64_t blocks = ((int64_t)num_valid + (int64_t)std::min(num_experts, num_valid) * (block_rows - 1)) / block_rows;
  const int64_t wgs = blocks * (block_rows == 16 ? groups : ceil_div(groups, 4));
  const int slices = block_rows == 16 ? 4 : 1;
  int splits = 1;
  while (wgs * splits * 2 <= 256 && units / (slices * splits * 2) >= 2 && splits < 4) splits *= 2;
  if (const char* e = nmx_tune(NMX_TUNE_MOE_MXFP4)) {
    const int f = atoi(e);
    if (f == 1 || f == 2 || f == 4) splits = f;
  }
  return std::max(1, std::min(splits, units));
}

template <typename scalar_t>
int moe_mx_launch(const MoeMxParams& p, int block_rows, int max_blocks, hipStream_t stream) {
  const int C = p.N / 64;
  if (block_rows == 16) moe_mxfp4_kernel<scalar_t, 1><<<dim3(C, p.k_splits, max_blocks), 256, 0, stream>>>(p);
  else if (block_rows == 32) moe_mxfp4_kernel<scalar_t, 2><<<dim3(ceil_div(C, 4), p.k_splits, max_blocks), 256, 0, stream>>>(p);
  else moe_mxfp4_kernel<scalar_t, 4><<<dim3(ceil_div(C, 4), p.k_splits, max_blocks), 256, 0, stream>>>(p);
  NMX_LAUNCH_CHECK();
  return NMX_OK;
}

bool moe_mx_shape_ok(int num_valid, int n, int k, int num_experts, int block_rows) {
  return num_valid >= 0 && num_experts >= 1 && (block_rows == 16 || block_rows == 32 || block_rows == 64) && n > 0 && k >= 128 &&
         k % 128 == 0 && n % 64 == 0;
}

}  // namespace

extern "C" int nmx_moe_mxfp4_mm_plan(int num_valid, int n, int k, int num_experts, int block_rows, int* splits) {
  NMX_CHECK(splits != nullptr, NMX_ERR_INVALID_ARG, "moe_mxfp4_mm_plan: null output");
  NMX_CHECK(moe_mx_shape_ok(num_valid, n, k, num_experts, block_rows), NMX_ERR_INVALID_ARG,
            "moe_mxfp4_mm_plan: num_valid = %d, n = %d, k = %d, num_experts = %d, block_rows = %d", num_valid, n, k, num_experts, block_rows);
  *splits = moe_mx_splits(num_valid, n, k, num_experts, block_rows);
  return NMX_OK;
}

extern "C" int64_t nmx_moe_mxfp4_mm_scratch_bytes(int num_valid, int n, int k, int num_experts, int block_rows) {
  if (!moe_mx_shape_ok(num_valid, n, k, num_experts, block_rows) || num_valid == 0) return 0;
  const int splits = moe_mx_splits(num_valid, n, k, num_experts, block_rows);
  return splits > 1 ? (int64_t)splits * num_valid * n * sizeof(float) : 0;
}

extern "C" int nmx_moe_mxfp4_mm(void* out, const uint8_t* a_q, const uint8_t* a_scale, const uint8_t* qweight_native,
                                const int32_t* scales_native, const float* topk_weights, const int32_t* sorted_token_ids,
                                const int32_t* expert_ids, const int32_t* num_tokens_post_padded, void* scratch, int64_t scratch_bytes,
                                int num_valid, int a_rows, int a_row_div, int n, int k, int num_experts, int block_rows, int max_blocks,
                                int dtype, nmx_stream_t stream) {
  NMX_CHECK(dtype == NMX_F16 || dtype == NMX_BF16, NMX_ERR_UNSUPPORTED, "moe_mxfp4_mm: float16 / bfloat16 output only");
  NMX_CHECK(block_rows == 16 || block_rows == 32 || block_rows == 64, NMX_ERR_INVALID_ARG, "moe_mxfp4_mm: block size 16, 32 or 64, got %d",
            block_rows);
  NMX_CHECK(nmx_mxfp4_supported(n, k), NMX_ERR_UNSUPPORTED, "moe_mxfp4_mm: k = %d must be a multiple of 128, n = %d of 64", k, n);
  NMX_CHECK(num_valid >= 0 && a_rows >= 0 && a_row_div >= 1 && num_experts >= 1 && max_blocks >= 0 && max_blocks <= 65535 &&
                (int64_t)num_valid <= (int64_t)a_rows * a_row_div,
            NMX_ERR_INVALID_ARG, "moe_mxfp4_mm: num_valid = %d, a_rows = %d, a_row_div = %d, num_experts = %d, max_blocks = %d", num_valid,
            a_rows, a_row_div, num_experts, max_blocks);
  NMX_CHECK((int64_t)(k / 2) * n <= 0x7ff00000ll && (int64_t)a_rows * (k / 2) <= 0x7ff00000ll && (int64_t)num_valid * n * 2 < (1ll << 31),
            NMX_ERR_UNSUPPORTED, "moe_mxfp4_mm: one expert's weights, a_q or out beyond the 2 GiB a 32-bit buffer offset addresses");
  if (num_valid == 0 || max_blocks == 0) return NMX_OK;
  NMX_CHECK(out != nullptr && a_q != nullptr && a_scale != nullptr && qweight_native != nullptr && scales_native != nullptr &&
                sorted_token_ids != nullptr && expert_ids != nullptr && num_tokens_post_padded != nullptr,
            NMX_ERR_INVALID_ARG, "moe_mxfp4_mm: null operand");
  NMX_CHECK(((uintptr_t)a_q % 16 == 0) && ((uintptr_t)qweight_native % 16 == 0) && ((uintptr_t)scales_native % 4 == 0) &&
                ((uintptr_t)out % 8 == 0) && ((uintptr_t)scratch % 16 == 0),
            NMX_ERR_INVALID_ARG, "moe_mxfp4_mm: operands must be 16-byte aligned");
  int splits = moe_mx_splits(num_valid, n, k, num_experts, block_rows);
  const int64_t slab = (int64_t)num_valid * n * sizeof(float);
  if (scratch == nullptr) scratch_bytes = 0;
  if ((int64_t)splits * slab > scratch_bytes) splits = (int)std::max<int64_t>(1, scratch_bytes / slab);  // fewer splits, never past the scratch
  MoeMxParams p;
  p.a_q = a_q; p.a_scale = a_scale; p.qw = qweight_native; p.scales = scales_native; p.out = out;
  p.partial = reinterpret_cast<float*>(scratch); p.topk_weights = topk_weights; p.sorted_token_ids = sorted_token_ids;
  p.expert_ids = expert_ids; p.num_tokens_post_padded = num_tokens_post_padded;
  p.N = n; p.K = k; p.k_splits = splits; p.num_valid = num_valid; p.a_rows = a_rows; p.a_row_div = a_row_div; p.num_experts = num_experts;
  const hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == NMX_F16 ? moe_mx_launch<f16>(p, block_rows, max_blocks, s) : moe_mx_launch<bf16>(p, block_rows, max_blocks, s);
  if (rc != NMX_OK || splits == 1) return rc;
  return nmx_splitk_reduce(out, p.partial, splits, num_valid, n, dtype, stream);
}

extern "C" int nmx_silu_and_mul_mxfp4_quant(uint8_t* out_q, uint8_t* out_scale, const void* x, int rows, int inter, int dtype,
                                            nmx_stream_t stream) {
  NMX_CHECK(dtype == NMX_F16 || dtype == NMX_BF16, NMX_ERR_UNSUPPORTED, "silu_and_mul_mxfp4_quant only supports bfloat16 and float16");
  NMX_CHECK(rows >= 0 && inter > 0 && inter % 32 == 0, NMX_ERR_INVALID_ARG,
            "silu_and_mul_mxfp4_quant: rows = %d, the intermediate size %d must be a multiple of 32", rows, inter);
  NMX_CHECK(out_q != nullptr && out_scale != nullptr && x != nullptr, NMX_ERR_INVALID_ARG, "silu_and_mul_mxfp4_quant: null operand");
  NMX_CHECK(((uintptr_t)out_q % 16 == 0) && ((uintptr_t)x % 16 == 0), NMX_ERR_INVALID_ARG,
            "silu_and_mul_mxfp4_quant: out_q and x must be 16-byte aligned");
  const int64_t blocks = (int64_t)rows * (inter / 32);
  if (blocks == 0) return NMX_OK;
  NMX_CHECK(ceil_div64(blocks, 256) < (1ll << 31), NMX_ERR_UNSUPPORTED, "silu_and_mul_mxfp4_quant: input too large");
  const unsigned grid = (unsigned)ceil_div64(blocks, 256);
  if (dtype == NMX_F16)
    silu_and_mul_mxfp4_quant_kernel<f16><<<grid, 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const f16*>(x),
                                                                                 reinterpret_cast<u32x4*>(out_q), out_scale, inter, blocks);
  else
    silu_and_mul_mxfp4_quant_kernel<bf16><<<grid, 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const bf16*>(x),
                                                                                  reinterpret_cast<u32x4*>(out_q), out_scale, inter, blocks);
  NMX_LAUNCH_CHECK();
  return NMX_OK;
}
