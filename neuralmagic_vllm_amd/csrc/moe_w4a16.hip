// Grouped W4A16 GEMM over expert-sorted rows on the CDNA4-native layout (include/nmx.h "int4 mixture-of-experts", DESIGN.md
// 3.1m): the expert GEMMs of a GPTQ int4 MoE layer as ONE launch each. No reference counterpart (the reference's fused_moe has
// no int4 form at this revision). The weights are the stacked outputs of nmx_w4a16_repack, one (qweight_native, scales_native)
// pair per expert; the kernel is w4a16_gemm_kernel (w4a16_native.hip) with its rows GATHERED through sorted_token_ids and its
// results SCATTERED to the pair id, the expert's tensors selected by the block - nothing is read on the host.
//
//   out[id, :] = cast((a[id / a_row_div, :] . W_e) * [topk_weights[id]]),  W_e[k, n] = (q_e[k, n] - 8) * s_e[group(k), n]
//   for every sorted pair id of block z (block_rows entries of sorted_token_ids), e = expert_ids[z].
#include "w4a16_fragment.h"

#include <stdlib.h>

namespace {

struct MoeW4Params {
  const void* a;               // [a_rows, K]
  const int32_t* qw;           // [E][K / 128][16 N] qweight_native per expert
  const void* scales;          // [E][G][N] scales_native per expert
  void* out;                   // [num_valid, N]
  float* partial;              // [k_splits, num_valid, N] fp32 slabs (k_splits > 1)
  const float* topk_weights;   // [num_valid] or null
  const int32_t* sorted_token_ids;
  const int32_t* expert_ids;
  const int32_t* num_tokens_post_padded;
  int N, K, num_groups, k_splits, num_valid, a_rows, a_row_div, num_experts;
};

// STAGED = false: block_rows = 16, the decode form. 4 waves on ONE 64-column group of the block's expert, every wave its own K
//   slice in units of 128 k; lane (g, r)'s B fragment is 16 contiguous bytes of row sorted_token_ids[16 z + r] / a_row_div,
//   straight from global memory; the 4 slices are summed through LDS with one barrier.
// STAGED = true: block_rows = 64 (MT = 4). 4 waves on 4 ADJACENT column groups sharing one K slice; every thread resolves the
//   rows of its 4 16-byte chunks once, before the loop; the gathered 64 x 128-k image of a unit goes to the double-buffered,
//   chunk ^ (row & 15)-swizzled LDS a unit ahead: one barrier per unit. A wave past N / 64 computes a valid group, stores nothing.
// Padding slots (id >= num_valid) get an offset past the activation descriptor: they read zeros and are never stored.
// Weights never touch LDS: one raw_buffer_load (dwordx4) per lane and 32-k step in one fixed issue order, two units ahead,
// through a descriptor whose base is the block's expert (64-bit arithmetic) and whose range is that one expert's tensor.
// Grid: x = column workgroups, y = K split, z = block. Split y > 0 or k_splits > 1: the routing-weighted fp32 results go to slab
// [y, num_valid, N]; every valid id is written by exactly one block in every split, so the slabs need no zeroing.
template <typename scalar_t, bool GROUPED, bool STAGED>
__global__ __launch_bounds__(256, (GROUPED && STAGED) ? 1 : 2) void moe_w4a16_kernel(const MoeW4Params p) {
  constexpr int MT = STAGED ? 4 : 1, BR = 16 * MT, NW = 4;
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

  const int64_t w_words = (int64_t)(K / 8) * N;  // one expert
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(p.qw + expert * w_words), 0, (K / 2) * N, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, p.a_rows * K * 2, 0x00020000);
  const scalar_t* const sc_e = reinterpret_cast<const scalar_t*>(p.scales) + (int64_t)expert * p.num_groups * N;
  const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<scalar_t*>(sc_e), 0, p.num_groups * N * 2, 0x00020000);
  const int unit_bytes = C * 4096;  // one 128-k unit of all column groups
  const int w_voff = cl * 4096 + lane * 16;
  const int s_voff = (cl * 4 + g) * 32;
  constexpr int kPast = 0x7ff00000;  // beyond every descriptor: the load returns zeros
  // unstaged: the lane's own row; staged: chunk e = tid + 256 i of the tile image (row e >> 4, 16-byte chunk e & 15)
  int a_voff[MT], a_lds[MT];
  if constexpr (STAGED) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int e = threadIdx.x + 256 * i, row = e >> 4, ch = e & 15;
      const int id = ids[row];
      a_voff[i] = (id >= 0 && id < p.num_valid) ? ((id / p.a_row_div) * K + 8 * ch) * 2 : kPast;
      a_lds[i] = row * 256 + ((ch ^ (row & 15)) * 16);
    }
  } else {
    const int id = ids[r];
    a_voff[0] = (id >= 0 && id < p.num_valid) ? ((id / p.a_row_div) * K + 8 * g) * 2 : kPast;
    a_lds[0] = 0;
  }

  constexpr int kTile = MT * 4096;  // staged activation image of one unit
  __shared__ __attribute__((aligned(16))) char smem[STAGED ? 2 * kTile : NW * 4096];

  struct Unit {
    u32x4 q[4];
    u32x4 a[STAGED ? 1 : 4];
    u32x4 s[2];
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
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto load_unit = [&](int u, Unit& U) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) load_step(u, ks, U);
    load_scales(u, U);
  };
  u32x4 areg[MT];
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
        const u32x4 wf = w4_fragment<scalar_t>(U.q[ks][t], magic);
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

  // ---- epilogue: channel-wise scale, routing weight (fp32), scatter to the pair id ----
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
    union { u32x4 v[2]; scalar_t e[16]; } sc;
    if constexpr (!GROUPED) {
      sc.v[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff, 0, 0);
      sc.v[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, s_voff + 16, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int id = ids[16 * mt + r];
      if (id < 0 || id >= p.num_valid) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 v = acc[mt][t];
        if constexpr (!GROUPED) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] *= Scalar<scalar_t>::to_f32(sc.e[4 * t + j]);
        }
        store4(v, id, cg * 64 + 16 * t + 4 * g);
      }
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
    const int t = e >> 6, el = e & 63, eg = el >> 4;
    const int id = ids[el & 15];
    if (id < 0 || id >= p.num_valid) return;
    if constexpr (!GROUPED) {
      union { u32x2 u; scalar_t e[4]; } sc;
      sc.u = *reinterpret_cast<const u32x2*>(sc_e + (cg * 4 + eg) * 16 + 4 * t);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] *= Scalar<scalar_t>::to_f32(sc.e[j]);
    }
    store4(v, id, cg * 64 + 16 * t + 4 * eg);
  }
}

// ---- dispatch --------------------------------------------------------------------------------------------------------
// K splits across workgroups only fill the 256 CUs (Mixtral's w2 at batch 1: 64 column workgroups x 2 occupied blocks). The host
// knows no histogram, so it takes an UPPER estimate of the occupied blocks: sum_e ceil(cnt_e / B) <= (numel + nz (B - 1)) / B with
// nz = min(E, numel) experts hit. Every wave keeps >= 2 units. NMX_MOE_W4A16 = "splits" forces 1, 2 or 4 (sweeps and tests).
int moe_w4_splits(int num_valid, int n, int k, int num_experts, int block_rows) {
  const int units = k / 128, groups = n / 64;
  const int64_t blocks = ((int64_t)num_valid + (int64_t)std::min(num_experts, num_valid) * (block_rows - 1)) / block_rows;
  const int64_t wgs = blocks * (block_rows == 16 ? groups : ceil_div(groups, 4));
  const int slices = block_rows == 16 ? 4 : 1;
  int splits = 1;
  while (wgs * splits * 2 <= 256 && units / (slices * splits * 2) >= 2 && splits < 4) splits *= 2;
  if (const char* e = nmx_tune(NMX_TUNE_MOE_W4A16)) {
    const int f = atoi(e);
    if (f == 1 || f == 2 || f == 4) splits = f;
  }
  return std::max(1, std::min(splits, units));
}

template <typename scalar_t, bool GROUPED>
int moe_w4_launch(const MoeW4Params& p, int block_rows, int max_blocks, hipStream_t stream) {
  const int C = p.N / 64;
  if (block_rows == 16) moe_w4a16_kernel<scalar_t, GROUPED, false><<<dim3(C, p.k_splits, max_blocks), 256, 0, stream>>>(p);
  else moe_w4a16_kernel<scalar_t, GROUPED, true><<<dim3(ceil_div(C, 4), p.k_splits, max_blocks), 256, 0, stream>>>(p);
  NMX_LAUNCH_CHECK();
  return NMX_OK;
}

bool moe_w4_shape_ok(int num_valid, int n, int k, int num_experts, int block_rows) {
  return num_valid >= 0 && num_experts >= 1 && (block_rows == 16 || block_rows == 64) && n > 0 && k >= 128 && k % 128 == 0 && n % 64 == 0;
}

}  // namespace

extern "C" int nmx_moe_w4a16_mm_plan(int num_valid, int n, int k, int num_experts, int block_rows, int* splits) {
  NMX_CHECK(splits != nullptr, NMX_ERR_INVALID_ARG, "moe_w4a16_mm_plan: null output");
  NMX_CHECK(moe_w4_shape_ok(num_valid, n, k, num_experts, block_rows), NMX_ERR_INVALID_ARG,
            "moe_w4a16_mm_plan: num_valid = %d, n = %d, k = %d, num_experts = %d, block_rows = %d", num_valid, n, k, num_experts, block_rows);
  *splits = moe_w4_splits(num_valid, n, k, num_experts, block_rows);
  return NMX_OK;
}

extern "C" int64_t nmx_moe_w4a16_mm_scratch_bytes(int num_valid, int n, int k, int num_experts, int block_rows) {
  if (!moe_w4_shape_ok(num_valid, n, k, num_experts, block_rows) || num_valid == 0) return 0;
  const int splits = moe_w4_splits(num_valid, n, k, num_experts, block_rows);
  return splits > 1 ? (int64_t)splits * num_valid * n * sizeof(float) : 0;
}

extern "C" int nmx_moe_w4a16_mm(void* out, const void* a, const int32_t* qweight_native, const void* scales_native,
                                const float* topk_weights, const int32_t* sorted_token_ids, const int32_t* expert_ids,
                                const int32_t* num_tokens_post_padded, void* scratch, int64_t scratch_bytes, int num_valid, int a_rows,
                                int a_row_div, int n, int k, int num_groups, int num_experts, int block_rows, int max_blocks, int dtype,
                                nmx_stream_t stream) {
  NMX_CHECK(dtype == NMX_F16 || dtype == NMX_BF16, NMX_ERR_UNSUPPORTED, "moe_w4a16_mm: float16 / bfloat16 only");
  NMX_CHECK(block_rows == 16 || block_rows == 64, NMX_ERR_INVALID_ARG, "moe_w4a16_mm: block size 16 or 64, got %d", block_rows);
  NMX_CHECK(nmx_w4a16_supported(n, k, num_groups, 4, 0), NMX_ERR_UNSUPPORTED,
            "moe_w4a16_mm: k = %d must be a multiple of 128, n = %d of 64, num_groups = %d one or k / 128", k, n, num_groups);
  NMX_CHECK(num_valid >= 0 && a_rows >= 0 && a_row_div >= 1 && num_experts >= 1 && max_blocks >= 0 && max_blocks <= 65535 &&
                (int64_t)num_valid <= (int64_t)a_rows * a_row_div,
            NMX_ERR_INVALID_ARG, "moe_w4a16_mm: num_valid = %d, a_rows = %d, a_row_div = %d, num_experts = %d, max_blocks = %d", num_valid,
            a_rows, a_row_div, num_experts, max_blocks);
  NMX_CHECK((int64_t)(k / 2) * n <= 0x7ff00000ll && (int64_t)a_rows * k * 2 <= 0x7ff00000ll && (int64_t)num_valid * n * 2 < (1ll << 31),
            NMX_ERR_UNSUPPORTED, "moe_w4a16_mm: one expert's weights, a or out beyond the 2 GiB a 32-bit buffer offset addresses");
  if (num_valid == 0 || max_blocks == 0) return NMX_OK;
  NMX_CHECK(out != nullptr && a != nullptr && qweight_native != nullptr && scales_native != nullptr && sorted_token_ids != nullptr &&
                expert_ids != nullptr && num_tokens_post_padded != nullptr,
            NMX_ERR_INVALID_ARG, "moe_w4a16_mm: null operand");
  NMX_CHECK(((uintptr_t)a % 16 == 0) && ((uintptr_t)qweight_native % 16 == 0) && ((uintptr_t)scales_native % 16 == 0) &&
                ((uintptr_t)out % 8 == 0) && ((uintptr_t)scratch % 16 == 0),
            NMX_ERR_INVALID_ARG, "moe_w4a16_mm: operands must be 16-byte aligned");
  int splits = moe_w4_splits(num_valid, n, k, num_experts, block_rows);
  const int64_t slab = (int64_t)num_valid * n * sizeof(float);
  if (scratch == nullptr) scratch_bytes = 0;
  if ((int64_t)splits * slab > scratch_bytes) splits = (int)std::max<int64_t>(1, scratch_bytes / slab);  // fewer splits, never past the scratch
  MoeW4Params p;
  p.a = a; p.qw = qweight_native; p.scales = scales_native; p.out = out; p.partial = reinterpret_cast<float*>(scratch);
  p.topk_weights = topk_weights; p.sorted_token_ids = sorted_token_ids; p.expert_ids = expert_ids;
  p.num_tokens_post_padded = num_tokens_post_padded;
  p.N = n; p.K = k; p.num_groups = num_groups; p.k_splits = splits; p.num_valid = num_valid; p.a_rows = a_rows; p.a_row_div = a_row_div;
  p.num_experts = num_experts;
  const hipStream_t s = (hipStream_t)stream;
  int rc;
  if (dtype == NMX_F16) rc = num_groups > 1 ? moe_w4_launch<f16, true>(p, block_rows, max_blocks, s) : moe_w4_launch<f16, false>(p, block_rows, max_blocks, s);
  else rc = num_groups > 1 ? moe_w4_launch<bf16, true>(p, block_rows, max_blocks, s) : moe_w4_launch<bf16, false>(p, block_rows, max_blocks, s);
  if (rc != NMX_OK || splits == 1) return rc;
  return nmx_splitk_reduce(out, p.partial, splits, num_valid, n, dtype, stream);
}
