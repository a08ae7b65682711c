"""Mixture-of-experts forward on the MI355X ops — the part of vllm/model_executor/layers/fused_moe/fused_moe.py that the
fp8 MoE method calls (fused_topk :335-368, fused_experts :402-511, fused_moe :514-585). The reference runs ONE Triton
grouped-GEMM kernel over tokens sorted by expert; here routing is native HIP (topk_softmax, moe_align_block_size) and
the fp8 path runs the two expert GEMMs as ONE grouped launch each over the sorted blocks (`moe_scaled_mm`: rows gathered
through sorted_token_ids, results scattered to their pair id; nothing is read back on the host, so the layer is
graph-capturable like the reference's). Round 3: the unquantised fp16 / bf16 path runs the same grouped kernel (`moe_mm`);
only shapes it does not take (K or N not multiples of 64, fp32 activations) fall back to a per-expert torch.matmul loop that
reads the per-expert row counts on the host. Arithmetic follows the reference: one per-tensor activation scale for the
whole batch (static, or dynamic = max over all tokens), per-expert weight scales, fp32 accumulation, routing weights
applied to the expert outputs before the sum over k."""
from typing import Optional, Tuple

import torch

from neuralmagic_vllm_amd import _custom_ops as ops


def fused_topk(hidden_states: torch.Tensor, gating_output: torch.Tensor, topk: int, renormalize: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    assert hidden_states.shape[0] == gating_output.shape[0], "Number of tokens mismatch"
    m = hidden_states.shape[0]
    topk_weights = torch.empty(m, topk, dtype=torch.float32, device=hidden_states.device)
    topk_ids = torch.empty(m, topk, dtype=torch.int32, device=hidden_states.device)
    token_expert_indicies = torch.empty(m, topk, dtype=torch.int32, device=hidden_states.device)
    ops.topk_softmax(topk_weights, topk_ids, token_expert_indicies, gating_output.float().contiguous())
    if renormalize:
        topk_weights = topk_weights / topk_weights.sum(dim=-1, keepdim=True)
    return topk_weights, topk_ids


def _expert_gemm(x: torch.Tensor, w: torch.Tensor, use_fp8: bool, a_scale: Optional[torch.Tensor], w_scale: Optional[torch.Tensor],
                 out_dtype: torch.dtype) -> torch.Tensor:
    """x [rows, K] (fp8 when use_fp8) @ w[N, K]^T."""
    if use_fp8:
        return ops.cutlass_scaled_mm(x, w.t(), a_scale, w_scale, out_dtype)
    return torch.matmul(x, w.t())


def fused_experts(hidden_states: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, topk_weights: torch.Tensor,
                  topk_ids: torch.Tensor, inplace: bool = False, use_fp8: bool = False, w1_scale: Optional[torch.Tensor] = None,
                  w2_scale: Optional[torch.Tensor] = None, a1_scale: Optional[torch.Tensor] = None,
                  a2_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert hidden_states.shape[1] == w1.shape[2], "Hidden size mismatch"
    assert topk_weights.shape == topk_ids.shape, "topk shape mismatch"
    assert hidden_states.is_contiguous() and w1.is_contiguous() and w2.is_contiguous()
    assert hidden_states.dtype in (torch.float32, torch.float16, torch.bfloat16)
    m, k = hidden_states.shape
    e, n2, _ = w1.shape
    topk = topk_ids.shape[1]
    dev, dt = hidden_states.device, hidden_states.dtype
    numel = m * topk
    if use_fp8 and dt in (torch.float16, torch.bfloat16) and k % 128 == 0 and (n2 // 2) % 128 == 0:
        return _fused_experts_fp8(hidden_states, w1, w2, topk_weights, topk_ids, inplace, w1_scale, w2_scale, a1_scale, a2_scale)
    if not use_fp8 and dt in (torch.float16, torch.bfloat16) and w1.dtype == dt and w2.dtype == dt and k % 64 == 0 and (n2 // 2) % 64 == 0:
        return _fused_experts_half(hidden_states, w1, w2, topk_weights, topk_ids, inplace)
    # tokens sorted by expert (block size 1: no padding needed for per-expert slices)
    sorted_ids = torch.empty(numel, dtype=torch.int32, device=dev)
    expert_of_block = torch.empty(numel, dtype=torch.int32, device=dev)
    post_pad = torch.empty(1, dtype=torch.int32, device=dev)
    ops.moe_align_block_size(topk_ids.contiguous(), e, 1, sorted_ids, expert_of_block, post_pad)
    counts = torch.bincount(expert_of_block.long(), minlength=e).tolist()  # rows per expert (one host read per call)
    src_tok = (sorted_ids // topk).long()                                    # token of every sorted row
    a = hidden_states.index_select(0, src_tok)                               # [numel, K] rows grouped by expert
    if use_fp8:
        a, a1 = ops.scaled_fp8_quant(a, a1_scale)                            # one scale for the whole batch (fused_moe.py:467-472)
    inter = torch.empty(numel, n2 // 2, dtype=dt, device=dev)
    gate_up = torch.empty(numel, n2, dtype=dt, device=dev)
    row = 0
    for ex, cnt in enumerate(counts):
        if cnt:
            gate_up[row:row + cnt] = _expert_gemm(a[row:row + cnt], w1[ex], use_fp8, a1 if use_fp8 else None,
                                                  w1_scale[ex:ex + 1] if use_fp8 else None, dt)
        row += cnt
    ops.silu_and_mul(inter, gate_up)
    if use_fp8:
        inter, a2 = ops.scaled_fp8_quant(inter, a2_scale)
    out_rows = torch.empty(numel, w2.shape[1], dtype=dt, device=dev)
    row = 0
    for ex, cnt in enumerate(counts):
        if cnt:
            out_rows[row:row + cnt] = _expert_gemm(inter[row:row + cnt], w2[ex], use_fp8, a2 if use_fp8 else None,
                                                   w2_scale[ex:ex + 1] if use_fp8 else None, dt)
        row += cnt
    # routing weight per sorted row, then the sum over k per token (fused_moe.py: mul_routed_weight + moe_sum)
    wts = topk_weights.reshape(-1).index_select(0, sorted_ids.long()).to(torch.float32)
    out = hidden_states if inplace else torch.empty_like(hidden_states)
    acc = torch.zeros(m, w2.shape[1], dtype=torch.float32, device=dev)
    acc.index_add_(0, src_tok, out_rows.float() * wts[:, None])
    out.copy_(acc.to(dt))
    return out


def _fused_experts_half(hidden_states, w1, w2, topk_weights, topk_ids, inplace):
    """fused_experts without quantisation (fused_moe.py:402-511, use_fp8 = False) on the grouped MFMA kernel (round 3; rounds 1-2
    looped over the experts with torch.matmul and read the expert histogram on the host): align -> grouped GEMM (gate | up) ->
    silu_and_mul -> grouped GEMM with the routing weight -> sum over k. Every step is a device launch: graph-capturable."""
    m, k = hidden_states.shape
    e, n2, _ = w1.shape
    topk = topk_ids.shape[1]
    dev, dt = hidden_states.device, hidden_states.dtype
    numel = m * topk
    block = 16 if numel <= 16 * e else 64  # get_default_config's BLOCK_SIZE_M (:308-332)
    max_sorted = numel + e * (block - 1)
    sorted_ids = torch.empty(max_sorted, dtype=torch.int32, device=dev)
    expert_ids = torch.empty((max_sorted + block - 1) // block, dtype=torch.int32, device=dev)
    post_pad = torch.empty(1, dtype=torch.int32, device=dev)
    ops.moe_align_block_size(topk_ids.contiguous(), e, block, sorted_ids, expert_ids, post_pad)
    gate_up = torch.empty(numel, n2, dtype=dt, device=dev)
    ops.moe_mm(gate_up, hidden_states, w1, None, sorted_ids, expert_ids, post_pad, topk, block)
    inter = torch.empty(numel, n2 // 2, dtype=dt, device=dev)
    ops.silu_and_mul(inter, gate_up)
    out_rows = torch.empty(numel, w2.shape[1], dtype=dt, device=dev)
    ops.moe_mm(out_rows, inter, w2, topk_weights.float().contiguous(), sorted_ids, expert_ids, post_pad, 1, block)
    out = hidden_states if inplace else torch.empty_like(hidden_states)
    torch.sum(out_rows.view(m, topk, w2.shape[1]), dim=1, out=out)  # moe_sum (:505-510)
    return out


def fused_experts_w4a16(hidden_states: torch.Tensor, w13_q: torch.Tensor, w13_s: torch.Tensor, w2_q: torch.Tensor,
                        w2_s: torch.Tensor, topk_weights: torch.Tensor, topk_ids: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """fused_experts on int4 GPTQ experts held in the CDNA4-native W4A16 layout (extension; no reference counterpart): the pipeline
    of _fused_experts_half with the grouped int4 GEMM (`moe_w4a16_mm`) in place of `moe_mm`. w13_q [E, H / 128, 16 * 2 I] int32 and
    w13_s [E, G, 2 I] (gate | up), w2_q [E, I / 128, 16 H] and w2_s [E, G2, H]: every expert's `w4a16_repack`, stacked. Every step
    is a device launch: graph-capturable."""
    assert topk_weights.shape == topk_ids.shape, "topk shape mismatch"
    assert hidden_states.is_contiguous() and hidden_states.dtype in (torch.float16, torch.bfloat16)
    m, k = hidden_states.shape
    e, _, n2 = w13_s.shape
    h = w2_s.shape[2]
    assert w13_q.shape[1] * 128 == k and h == k and w2_q.shape[1] * 128 == n2 // 2, "Hidden / intermediate size mismatch"
    topk = topk_ids.shape[1]
    dev, dt = hidden_states.device, hidden_states.dtype
    numel = m * topk
    block = 16 if numel <= 16 * e else 64  # as _fused_experts_half
    max_sorted = numel + e * (block - 1)
    sorted_ids = torch.empty(max_sorted, dtype=torch.int32, device=dev)
    expert_ids = torch.empty((max_sorted + block - 1) // block, dtype=torch.int32, device=dev)
    post_pad = torch.empty(1, dtype=torch.int32, device=dev)
    ops.moe_align_block_size(topk_ids.contiguous(), e, block, sorted_ids, expert_ids, post_pad)
    gate_up = torch.empty(numel, n2, dtype=dt, device=dev)
    ops.moe_w4a16_mm(gate_up, hidden_states, w13_q, w13_s, None, sorted_ids, expert_ids, post_pad, topk, block)
    inter = torch.empty(numel, n2 // 2, dtype=dt, device=dev)
    ops.silu_and_mul(inter, gate_up)
    out_rows = torch.empty(numel, h, dtype=dt, device=dev)
    ops.moe_w4a16_mm(out_rows, inter, w2_q, w2_s, topk_weights.float().contiguous(), sorted_ids, expert_ids, post_pad, 1, block)
    out = hidden_states if inplace else torch.empty_like(hidden_states)
    torch.sum(out_rows.view(m, topk, h), dim=1, out=out)  # moe_sum
    return out


def mxfp4_block_rows(numel: int, num_experts: int) -> int:
    """Rows per block of the grouped MXFP4 GEMM. Measured on Mixtral-8x7B shapes (tools/moe_mxfp4_ab.py): 16-row
    blocks are ahead at 2 pairs (42.9 vs 50.5 us), 64-row blocks from 4 pairs per expert on (126 vs 132 us at 32 pairs, 162 vs 200
    at 128, 230 vs 634 at 512) - earlier than the siblings' 16 E, because a staged block costs no conversion here. Between 2 and 32
    pairs nothing is measured; 32-row blocks were never ahead of both."""
    return 16 if numel < 4 * num_experts else 64


def fused_experts_mxfp4(hidden_states: torch.Tensor, w13_q: torch.Tensor, w13_s: torch.Tensor, w2_q: torch.Tensor,
                        w2_s: torch.Tensor, topk_weights: torch.Tensor, topk_ids: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """fused_experts on MXFP4 experts held in the native layout of the fp4 MFMA (extension; no reference counterpart): align ->
    mxfp4_quant (every token row once) -> grouped GEMM (gate | up) -> silu_and_mul fused with the quantiser -> grouped GEMM with the
    routing weight -> sum over k. w13_q [E, H / 128, 64 * 2 I] uint8 and w13_s [E, H / 128, 2 I] int32 (gate | up), w2_q
    [E, I / 128, 64 H] and w2_s [E, I / 128, H]: every expert's `mxfp4_repack`, stacked. Every step is a device launch:
    graph-capturable."""
    assert topk_weights.shape == topk_ids.shape, "topk shape mismatch"
    assert hidden_states.is_contiguous() and hidden_states.dtype in (torch.float16, torch.bfloat16)
    m, k = hidden_states.shape
    e, _, n2 = w13_s.shape
    h = w2_s.shape[2]
    assert w13_q.shape[1] * 128 == k and h == k and w2_q.shape[1] * 128 == n2 // 2, "Hidden / intermediate size mismatch"
    topk = topk_ids.shape[1]
    dev, dt = hidden_states.device, hidden_states.dtype
    numel = m * topk
    block = mxfp4_block_rows(numel, e)
    max_sorted = numel + e * (block - 1)
    sorted_ids = torch.empty(max_sorted, dtype=torch.int32, device=dev)
    expert_ids = torch.empty((max_sorted + block - 1) // block, dtype=torch.int32, device=dev)
    post_pad = torch.empty(1, dtype=torch.int32, device=dev)
    ops.moe_align_block_size(topk_ids.contiguous(), e, block, sorted_ids, expert_ids, post_pad)
    x_q, x_s = ops.mxfp4_quant(hidden_states)
    gate_up = torch.empty(numel, n2, dtype=dt, device=dev)
    ops.moe_mxfp4_mm(gate_up, x_q, x_s, w13_q, w13_s, None, sorted_ids, expert_ids, post_pad, topk, block)
    i_q, i_s = ops.silu_and_mul_mxfp4_quant(gate_up)
    out_rows = torch.empty(numel, h, dtype=dt, device=dev)
    ops.moe_mxfp4_mm(out_rows, i_q, i_s, w2_q, w2_s, topk_weights.float().contiguous(), sorted_ids, expert_ids, post_pad, 1, block)
    out = hidden_states if inplace else torch.empty_like(hidden_states)
    torch.sum(out_rows.view(m, topk, h), dim=1, out=out)  # moe_sum
    return out


def _fused_experts_fp8(hidden_states, w1, w2, topk_weights, topk_ids, inplace, w1_scale, w2_scale, a1_scale, a2_scale):
    """fused_experts with use_fp8 (fused_moe.py:402-511): align -> quantise -> grouped GEMM (gate | up) -> silu_and_mul ->
    quantise -> grouped GEMM with the routing weight -> sum over k. Every step is a device launch."""
    m, k = hidden_states.shape
    e, n2, _ = w1.shape
    topk = topk_ids.shape[1]
    dev, dt = hidden_states.device, hidden_states.dtype
    numel = m * topk
    block = 16 if numel <= 16 * e else 64  # get_default_config's BLOCK_SIZE_M: 16 for decode-size batches, else 64 (:308-332)
    max_sorted = numel + e * (block - 1)
    sorted_ids = torch.empty(max_sorted, dtype=torch.int32, device=dev)
    expert_ids = torch.empty((max_sorted + block - 1) // block, dtype=torch.int32, device=dev)
    post_pad = torch.empty(1, dtype=torch.int32, device=dev)
    ops.moe_align_block_size(topk_ids.contiguous(), e, block, sorted_ids, expert_ids, post_pad)
    a_q, a1 = ops.scaled_fp8_quant(hidden_states, a1_scale)  # one scale for the whole batch (:467-472)
    gate_up = torch.empty(numel, n2, dtype=dt, device=dev)
    ops.moe_scaled_mm(gate_up, a_q, w1, a1, w1_scale.float().contiguous(), None, sorted_ids, expert_ids, post_pad, topk, block)
    inter = torch.empty(numel, n2 // 2, dtype=dt, device=dev)
    ops.silu_and_mul(inter, gate_up)
    i_q, a2 = ops.scaled_fp8_quant(inter, a2_scale)
    out_rows = torch.empty(numel, w2.shape[1], dtype=dt, device=dev)
    ops.moe_scaled_mm(out_rows, i_q, w2, a2, w2_scale.float().contiguous(), topk_weights.float().contiguous(), sorted_ids,
                      expert_ids, post_pad, 1, block)
    out = hidden_states if inplace else torch.empty_like(hidden_states)
    torch.sum(out_rows.view(m, topk, w2.shape[1]), dim=1, out=out)  # moe_sum (:505-510)
    return out


def fused_moe(hidden_states: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, gating_output: torch.Tensor, topk: int,
              renormalize: bool, inplace: bool = False, use_fp8: bool = False, w1_scale: Optional[torch.Tensor] = None,
              w2_scale: Optional[torch.Tensor] = None, a1_scale: Optional[torch.Tensor] = None,
              a2_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fused_moe.py:514-585: w1 [E, 2 N, K] (gate | up), w2 [E, K, N]; returns [M, K]."""
    assert gating_output.shape[1] == w1.shape[0], "Number of experts mismatch"
    topk_weights, topk_ids = fused_topk(hidden_states, gating_output, topk, renormalize)
    return fused_experts(hidden_states, w1, w2, topk_weights, topk_ids, inplace=inplace, use_fp8=use_fp8, w1_scale=w1_scale,
                         w2_scale=w2_scale, a1_scale=a1_scale, a2_scale=a2_scale)
