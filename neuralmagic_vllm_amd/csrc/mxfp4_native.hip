// MXFP4 linear layers on the block-scaled fp4 MFMA of gfx950 (include/nmx.h "MXFP4 on the native layout"):
// v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = blgp = 4 takes e2m1 elements for both operands and one E8M0 scale per lane -
// a lane supplies 32 consecutive k of one row, exactly one MX block - so neither the weights nor the activations are converted
// to 16 bits: the weights are streamed as they are stored, the activations are quantised by the lane that feeds them.
//
//   qweight_native  bytes [K / 128][N / 16][lane l = 16 g + i][16]: the 16 bytes (32 codes, low nibble = even k) of column
//       n = 16 T + i at k = 128 u + 32 g .. + 31 - the lane's whole A operand of tile T for one 128-k unit. The four tiles of a
//       64-column group are 4 KiB contiguous: the work split, the load ring and the slabs of w4a16_gemm_kernel carry over.
//   scales_native   uint32 [K / 128][N / 64][lane l = 16 g + i]: byte t = the E8M0 scale of column 64 c + 16 t + i, block 4 u + g;
//       one dword per lane and unit, op_sel picks the tile's byte.
// The activations are the B operand: lane (g, r) holds row r, k = 128 u + 32 g .. + 31 and the block's scale in byte 0.
// D: lane (g, r) of tile t holds columns 16 t + 4 g + 0..3 of row r (as 3.1n).
#include "mxfp4_fragment.h"

#include <stdlib.h>

#include <utility>

namespace {

struct MxParams {
  const void* a;           // [M, K] fp16 / bf16
  const void* qw;          // qweight_native
  const uint32_t* scales;  // scales_native
  void* c;                 // [M, N]
  float* partial;          // [k_splits, M, N] fp32 slabs (k_splits > 1)
  int M, N, K, k_splits;
  int xcd_per;             // > 0: XCDs per K split (2 / 4 / 8 splits, the split is chosen by the workgroup id % 8)
};

struct MxCfg { int mt, nw, splits; };

// ---- nmx_mxfp4_quant: one lane per block, 64 bytes in, 16 + 1 bytes out ------------------------------------------------------
template <typename scalar_t>
__global__ __launch_bounds__(256) void mxfp4_quant_kernel(const u32x4* __restrict__ in, u32x4* __restrict__ out_q,
                                                          uint8_t* __restrict__ out_scale, int64_t blocks) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= blocks) return;
  u32x4 x[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = in[4 * b + i];
  uint32_t sb;
  out_q[b] = mx_quant_block<scalar_t>(x, sb);
  out_scale[b] = (uint8_t)sb;
}

// ---- nmx_mxfp4_repack: checkpoint weight [N, K / 2] + weight_scale [N, K / 32] -> the native pair; 16-byte chunk o / dword o by
// thread o. Chunk (u, T, 16 g + i) is checkpoint chunk (row 16 T + i, block 4 u + g), bytes unchanged.
__global__ __launch_bounds__(256) void mxfp4_repack_kernel(const u32x4* __restrict__ weight, const uint8_t* __restrict__ scale,
                                                           u32x4* __restrict__ qnative, uint32_t* __restrict__ snative, int K, int N) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int KB = K / 32, C = N / 64;
  const int l = (int)(o & 63), g = l >> 4, i = l & 15;
  if (o < (int64_t)KB * N) {
    const int64_t ut = o >> 6;
    const int T = (int)(ut % (N / 16)), u = (int)(ut / (N / 16));
    qnative[o] = weight[(int64_t)(16 * T + i) * KB + 4 * u + g];
  }
  if (o < (int64_t)(K / 128) * C * 64) {
    const int64_t uc = o >> 6;
    const int c = (int)(uc % C), u = (int)(uc / C);
    uint32_t w = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) w |= (uint32_t)scale[(int64_t)(64 * c + 16 * t + i) * KB + 4 * u + g] << (8 * t);
    snative[o] = w;
  }
}

// ---- the GEMM. c [M, N] = Q(a) . W^T-native, Q = mx_quant_block per row and 32-k block.
//   STAGED = false (MT = 1, up to 16 rows): NW waves on ONE 64-column group, every wave its own K slice in units of 128 k. Per
//     unit a lane loads the 64 bytes of its row's block straight from global memory, quantises them in registers and issues
//     4 scaled MFMAs (one per tile) that share the B operand and its scale. No LDS and no barrier in the loop; the NW slices
//     are summed through LDS with one barrier.
//   STAGED = true (MT = 2 / 4): 4 waves on 4 ADJACENT column groups sharing one K slice. The (16 MT) x 128-k activation tile of a
//     unit is quantised ONCE per workgroup: wave w < MT loads row tile w (a unit ahead, the lane mapping of the unstaged form),
//     quantises it and writes the image in FRAGMENT order - chunk 64 mt + lane, scale byte 64 mt + lane behind the chunks - so
//     both the 16-byte writes and the 16-byte fragment reads of a wave are 1 KiB linear: conflict-free without a swizzle. The
//     image is 1088 MT bytes (the fp16 image of 3.1n: 4096 MT), double-buffered, one barrier per unit; a wave reads MT
//     fragments and issues 4 MT MFMAs.
// Weights never touch LDS: one raw_buffer_load (dwordx4) per lane and tile plus one dword of scales per unit, issued in one
// fixed order two units ahead (2 x 4 KiB per wave in flight).
template <typename scalar_t, int MT, int NW, bool STAGED>
__global__ __launch_bounds__(64 * NW, 2) void mxfp4_gemm_kernel(const MxParams p) {
  static_assert(STAGED ? NW == 4 && MT <= 4 : MT == 1, "staged: 4 waves = 4 column groups; unstaged: one 16-row tile");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int N = p.N, K = p.K, M = p.M;
  const int C = N / 64, total_units = K / 128;

  // workgroup -> (column workgroup, K split); with 2 / 4 / 8 splits the XCD (= workgroup id % 8) selects the split (3.1n)
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

  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.qw), 0, (K / 2) * N, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, M * K * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(p.scales), 0, total_units * C * 256, 0x00020000);
  const int unit_bytes = C * 4096;  // one 128-k unit of all column groups
  const int w_voff = cl * 4096 + lane * 16;
  const int s_voff = (cl * 64 + lane) * 4;
  constexpr int kPast = 0x7ff00000;  // beyond every descriptor: the load returns zeros
  // the lane's block of a unit: row r of the wave's row tile (unstaged: the only one; staged: tile `wave`), k = 32 g .. + 31.
  // Rows past M are fed zeros (code 0, scale byte 0) and never stored.
  const int a_row = m0 + (STAGED ? 16 * wave : 0) + r;
  const int a_voff = a_row < M ? (a_row * K + 32 * g) * 2 : kPast;
  const bool stager = STAGED && wave < MT;

  constexpr int kImg = MT * 1088;  // staged image of one unit: 64 MT chunks of 16 bytes, then 64 MT scale bytes
  __shared__ __attribute__((aligned(16))) char smem[STAGED ? 2 * kImg : NW * 4096];

  struct Unit {
    u32x4 q[4];
    u32x4 a[STAGED ? 1 : 4];
    uint32_t s;
  };
  // loads of tile t / the scale word of unit u (past the slice: the last unit again, never consumed). sched_barrier pins the
  // issue order: prologue and loop must queue the loads alike, or the merged wait counts at the loop head degrade.
  auto load_tile = [&](int u, int t, Unit& U) {
    u = min(u, total_units - 1);
    U.q[t] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, w_voff, u * unit_bytes + t * 1024, 2);  // aux 2: non-temporal
    if constexpr (!STAGED) U.a[t] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_voff + 16 * t, u * 256, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto load_scales = [&](int u, Unit& U) {
    u = min(u, total_units - 1);
    U.s = __builtin_amdgcn_raw_buffer_load_b32(rs_s, s_voff, u * C * 256, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto load_unit = [&](int u, Unit& U) {
#pragma unroll
    for (int t = 0; t < 4; ++t) load_tile(u, t, U);
    load_scales(u, U);
  };
  u32x4 areg[4];
  auto stage_load = [&](int u) {
    if constexpr (STAGED) {
      if (stager) {
        u = min(u, total_units - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) areg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_voff + 16 * i, u * 256, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto stage_store = [&](char* buf) {
    if constexpr (STAGED) {
      if (stager) {
        uint32_t sb;
        const u32x4 q = mx_quant_block<scalar_t>(areg, sb);
        *reinterpret_cast<u32x4*>(buf + threadIdx.x * 16) = q;
        *reinterpret_cast<uint8_t*>(buf + MT * 1024 + threadIdx.x) = (uint8_t)sb;
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
      bq[0] = mx_quant_block<scalar_t>(U.a, bs[0]);
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
  auto store = [&](f32x4 v, int m, int col) {
    const int64_t off = (int64_t)m * N + col;
    if (p.k_splits == 1) {
      union { scalar_t h[4]; u32x2 u; } o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o.h[j] = Scalar<scalar_t>::from_f32(v[j]);
      *reinterpret_cast<u32x2*>(cptr + off) = o.u;
    } else {
      *reinterpret_cast<f32x4*>(p.partial + (int64_t)split * M * N + off) = v;
    }
  };
  if constexpr (STAGED) {
    if (!col_ok) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m0 + 16 * mt + r;
      if (m >= M) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) store(acc[mt][t], m, cg * 64 + 16 * t + 4 * g);
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
      const int t = e >> 6, el = e & 63;
      const int m = m0 + (el & 15);
      if (m < M) store(v, m, cg * 64 + 16 * t + 4 * (el >> 4));
    }
  }
}

// ---- dispatch ------------------------------------------------------------------------------------------------------------------
// mt: 16-row tiles per workgroup (1: the unstaged form, 2 / 4: staged), nw: waves of the unstaged form (4 / 8), splits: K splits
// across workgroups - only to fill the 256 CUs, and only while every wave keeps >= 2 units (the rule of w4_pick).
// NMX_MXFP4 = "mt,nw,splits" forces any of them for sweeps and tests (0 = keep the default).
MxCfg mx_pick(int M, int N, int K) {
  MxCfg c;
  // Measured (tools/lean_sweep.py F: family, Llama-3-8B shapes, fp16, M = 1 / 16 / 64; DESIGN.md 3.1f4, profiles/mxfp4_native_ab.txt):
  // M = 1 the unstaged form with 4 waves everywhere (8 waves lose 0.5 - 1.8 us). M = 16: the unstaged form on o (8.3 vs 9.5 us),
  // level on qkv and down, the staged 32-row tile on gate_up (18.0 vs 22.6): the 24 MiB threshold of w4_pick, in fp4 bytes. M = 64:
  // two 32-row blocks beat the 64-row tile on all four shapes (qkv 14.0 vs 16.7, o 12.9 vs 17.9, gate_up 24.4 vs 28.5, down 19.4
  // vs 20.4; 207 registers at MT = 4). M = 8, 32 and everything above 64 (row blocks of 64) are not measured.
  const bool big = (int64_t)K * N / 2 >= (24ll << 20);
  c.mt = M <= 8 ? 1 : (M <= 16 ? (big ? 2 : 1) : (M <= 64 ? 2 : 4));
  c.nw = 4;
  c.splits = 1;
  int f_mt = 0, f_nw = 0, f_splits = 0;
  if (const char* e = nmx_tune(NMX_TUNE_MXFP4)) sscanf(e, "%d,%d,%d", &f_mt, &f_nw, &f_splits);
  if (f_mt == 1 || f_mt == 2 || f_mt == 4) c.mt = f_mt;
  if (c.mt == 1 && f_nw == 8) c.nw = 8;
  const int units = K / 128, groups = N / 64;
  const int row_blocks = ceil_div(M, 16 * c.mt);
  const int wgs = (c.mt == 1 ? groups : ceil_div(groups, 4)) * row_blocks;
  const int slices = c.mt == 1 ? c.nw : 1;
  while (wgs * c.splits * 2 <= 256 && units / (slices * c.splits * 2) >= 2 && c.splits < 16) c.splits *= 2;
  if (f_splits >= 1) c.splits = f_splits;
  c.splits = std::max(1, std::min(std::min(c.splits, units), 64));
  return c;
}

template <typename scalar_t>
int mx_launch(const MxParams& p, const MxCfg& cfg, hipStream_t stream) {
  const int C = p.N / 64;
  const int ncolwg = cfg.mt == 1 ? C : ceil_div(C, 4);
  dim3 grid(ncolwg, p.k_splits, ceil_div(p.M, 16 * cfg.mt));
  if (p.xcd_per > 0) grid = dim3(ceil_div(ncolwg, p.xcd_per) * 8, 1, grid.z);
  if (cfg.mt == 1 && cfg.nw == 8) mxfp4_gemm_kernel<scalar_t, 1, 8, false><<<grid, 512, 0, stream>>>(p);
  else if (cfg.mt == 1) mxfp4_gemm_kernel<scalar_t, 1, 4, false><<<grid, 256, 0, stream>>>(p);
  else if (cfg.mt == 2) mxfp4_gemm_kernel<scalar_t, 2, 4, true><<<grid, 256, 0, stream>>>(p);
  else mxfp4_gemm_kernel<scalar_t, 4, 4, true><<<grid, 256, 0, stream>>>(p);
  NMX_LAUNCH_CHECK();
  return NMX_OK;
}

}  // namespace

extern "C" int nmx_mxfp4_supported(int size_n, int size_k) {
  return size_n > 0 && size_k > 0 && size_k % 128 == 0 && size_n % 64 == 0 ? 1 : 0;
}

extern "C" int nmx_mxfp4_repack(const uint8_t* weight, const uint8_t* weight_scale, void* qweight_native, uint32_t* scales_native,
                                int size_k, int size_n, nmx_stream_t stream) {
  NMX_CHECK(nmx_mxfp4_supported(size_n, size_k), NMX_ERR_UNSUPPORTED,
            "mxfp4_repack: size_k = %d must be a multiple of 128, size_n = %d of 64", size_k, size_n);
  NMX_CHECK(weight != nullptr && weight_scale != nullptr && qweight_native != nullptr && scales_native != nullptr &&
                weight != qweight_native,
            NMX_ERR_INVALID_ARG, "mxfp4_repack: null or aliased operand");
  NMX_CHECK(((uintptr_t)weight % 16 == 0) && ((uintptr_t)qweight_native % 16 == 0) && ((uintptr_t)scales_native % 4 == 0),
            NMX_ERR_INVALID_ARG, "mxfp4_repack: weight and qweight_native must be 16-byte aligned");
  const int64_t chunks = (int64_t)(size_k / 32) * size_n;  // (>= the scale dwords: size_k / 128 * size_n)
  NMX_CHECK(ceil_div64(chunks, 256) < (1ll << 31), NMX_ERR_UNSUPPORTED, "mxfp4_repack: weight too large");
  mxfp4_repack_kernel<<<(unsigned)ceil_div64(chunks, 256), 256, 0, (hipStream_t)stream>>>(
      reinterpret_cast<const u32x4*>(weight), weight_scale, reinterpret_cast<u32x4*>(qweight_native), scales_native, size_k, size_n);
  NMX_LAUNCH_CHECK();
  return NMX_OK;
}

extern "C" int nmx_mxfp4_quant(uint8_t* out_q, uint8_t* out_scale, const void* input, int size_m, int size_k, int dtype,
                               nmx_stream_t stream) {
  NMX_CHECK(dtype == NMX_F16 || dtype == NMX_BF16, NMX_ERR_UNSUPPORTED, "mxfp4_quant only supports bfloat16 and float16");
  NMX_CHECK(size_m >= 0 && size_k > 0 && size_k % 32 == 0, NMX_ERR_INVALID_ARG,
            "mxfp4_quant: size_m = %d, size_k = %d must be a multiple of 32", size_m, size_k);
  NMX_CHECK(out_q != nullptr && out_scale != nullptr && input != nullptr, NMX_ERR_INVALID_ARG, "mxfp4_quant: null operand");
  NMX_CHECK(((uintptr_t)out_q % 16 == 0) && ((uintptr_t)input % 16 == 0), NMX_ERR_INVALID_ARG,
            "mxfp4_quant: out_q and input must be 16-byte aligned");
  const int64_t blocks = (int64_t)size_m * (size_k / 32);
  if (blocks == 0) return NMX_OK;
  NMX_CHECK(ceil_div64(blocks, 256) < (1ll << 31), NMX_ERR_UNSUPPORTED, "mxfp4_quant: input too large");
  const unsigned grid = (unsigned)ceil_div64(blocks, 256);
  if (dtype == NMX_F16)
    mxfp4_quant_kernel<f16><<<grid, 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const u32x4*>(input),
                                                                    reinterpret_cast<u32x4*>(out_q), out_scale, blocks);
  else
    mxfp4_quant_kernel<bf16><<<grid, 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const u32x4*>(input),
                                                                     reinterpret_cast<u32x4*>(out_q), out_scale, blocks);
  NMX_LAUNCH_CHECK();
  return NMX_OK;
}

extern "C" int nmx_mxfp4_gemm_plan(int size_m, int size_n, int size_k, int* mt, int* nw, int* splits) {
  NMX_CHECK(mt != nullptr && nw != nullptr && splits != nullptr, NMX_ERR_INVALID_ARG, "mxfp4_gemm_plan: null output");
  NMX_CHECK(size_m > 0 && size_n > 0 && size_k >= 128, NMX_ERR_INVALID_ARG, "mxfp4_gemm_plan: size_m = %d, size_n = %d, size_k = %d", size_m,
            size_n, size_k);
  const MxCfg c = mx_pick(size_m, size_n, size_k);
  *mt = c.mt;
  *nw = c.nw;
  *splits = c.splits;
  return NMX_OK;
}

extern "C" int64_t nmx_mxfp4_gemm_scratch_bytes(int size_m, int size_n, int size_k) {
  if (size_m <= 0 || size_n <= 0 || size_k < 128) return 0;
  const int splits = mx_pick(size_m, size_n, size_k).splits;
  return splits > 1 ? (int64_t)splits * size_m * size_n * sizeof(float) : 0;
}

extern "C" int nmx_mxfp4_gemm(const void* a, const void* qweight_native, const uint32_t* scales_native, void* c, void* scratch,
                              int64_t scratch_bytes, int size_m, int size_n, int size_k, int dtype, nmx_stream_t stream) {
  NMX_CHECK(dtype == NMX_F16 || dtype == NMX_BF16, NMX_ERR_UNSUPPORTED, "mxfp4_gemm only supports bfloat16 and float16");
  NMX_CHECK(size_m >= 0 && size_n > 0 && size_k > 0, NMX_ERR_INVALID_ARG, "mxfp4_gemm: size_m = %d, size_n = %d, size_k = %d", size_m,
            size_n, size_k);
  NMX_CHECK(nmx_mxfp4_supported(size_n, size_k), NMX_ERR_UNSUPPORTED,
            "mxfp4_gemm: size_k = %d must be a multiple of 128, size_n = %d of 64", size_k, size_n);
  NMX_CHECK((int64_t)size_m * size_k * 2 <= 0x7ff00000ll && (int64_t)size_k * size_n / 2 < (1ll << 31) && (int64_t)size_m * size_n < (1ll << 31),
            NMX_ERR_UNSUPPORTED, "mxfp4_gemm: operand beyond the 2 GiB a buffer descriptor addresses");
  NMX_CHECK(a != nullptr && qweight_native != nullptr && scales_native != nullptr && c != nullptr, NMX_ERR_INVALID_ARG,
            "mxfp4_gemm: null operand");
  NMX_CHECK(((uintptr_t)a % 16 == 0) && ((uintptr_t)qweight_native % 16 == 0) && ((uintptr_t)scales_native % 4 == 0) &&
                ((uintptr_t)c % 8 == 0) && ((uintptr_t)scratch % 16 == 0),
            NMX_ERR_INVALID_ARG, "mxfp4_gemm: operands must be 16-byte aligned");
  if (size_m == 0) return NMX_OK;
  MxCfg cfg = mx_pick(size_m, size_n, size_k);
  const int64_t slab = (int64_t)size_m * size_n * sizeof(float);
  if (scratch == nullptr) scratch_bytes = 0;
  if ((int64_t)cfg.splits * slab > scratch_bytes) cfg.splits = (int)std::max<int64_t>(1, scratch_bytes / slab);  // fewer splits, never past the scratch
  MxParams p;
  p.a = a; p.qw = qweight_native; p.scales = scales_native; p.c = c; p.partial = reinterpret_cast<float*>(scratch);
  p.M = size_m; p.N = size_n; p.K = size_k; p.k_splits = cfg.splits;
  const char* xs = nmx_tune(NMX_TUNE_GEMM_XCD_SPLIT);
  const bool xcd = (xs == nullptr || atoi(xs) != 0) && (cfg.splits == 2 || cfg.splits == 4 || cfg.splits == 8);
  p.xcd_per = xcd ? 8 / cfg.splits : 0;
  const int rc = dtype == NMX_F16 ? mx_launch<f16>(p, cfg, (hipStream_t)stream) : mx_launch<bf16>(p, cfg, (hipStream_t)stream);
  if (rc != NMX_OK || cfg.splits == 1) return rc;
  return nmx_splitk_reduce(c, p.partial, cfg.splits, size_m, size_n, dtype, (hipStream_t)stream);
}
