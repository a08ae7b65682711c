"""GPU tests of the MXFP4 mixture-of-experts path (include/nmx.h "MXFP4 mixture-of-experts"): the grouped GEMM against float64
for the three block forms, every K split, padding slots, empty experts and blocks past the padded length; silu_and_mul fused with
the quantiser bit for bit; the MXFP4MoEMethod layer against a chain that rounds where the kernels do; graph capture."""
import pytest
import torch

from test_mxfp4_gpu import dequant, quant_cpu
from util import compute_max_diff, seed_all

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_EXPERTS = {}


def experts(E, K, N, lo=118, hi=131):
    """E MXFP4 [N, K] experts, made once per shape, on the CPU: (checkpoint weight [E, N, K / 2], weight_scale [E, N, K / 32],
    w_ref fp64 [E, N, K]). Random code bytes; the scale bytes differ per column, block and expert."""
    key = (E, K, N, lo, hi)
    if key not in _EXPERTS:
        seed_all(E + K)
        weight = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8)
        scale = torch.randint(lo, hi, (E, N, K // 32), dtype=torch.uint8)
        _EXPERTS[key] = (weight, scale, torch.stack([dequant(w, s) for w, s in zip(weight, scale)]))
    return _EXPERTS[key]


def native(ops, weight, scale):
    pairs = [ops.mxfp4_repack(w.to(DEV), s.to(DEV)) for w, s in zip(weight, scale)]
    return torch.stack([q for q, _ in pairs]), torch.stack([s for _, s in pairs])


def scaled_randn(rows, k, lo=-8, hi=5):
    """randn times a power of two that differs per row and per 32-k block: a wrong gathered row or scale byte shows"""
    return torch.randn(rows, k) * torch.exp2(torch.randint(lo, hi, (rows, k // 32)).float()).repeat_interleave(32, dim=1)


# K = 128: one unit, one group - the lane -> row / block mapping and the scale bytes. K = 896: 7 units, uneven slices across the 4
# waves and across splits, a peeled odd unit; N = 192: 3 column groups, one staged wave is past N
@pytest.mark.parametrize("K,N,dtype,cfg,div1", [
    (128, 64, torch.float16, "1", False), (896, 192, torch.float16, None, False), (896, 192, torch.float16, "4", True),
    (1024, 256, torch.float16, "2", False), (896, 192, torch.bfloat16, "2", True)])
@pytest.mark.parametrize("m,e,topk,block", [(1, 8, 2, 16), (33, 8, 2, 16), (70, 8, 2, 32), (222, 8, 2, 64), (40, 64, 6, 16)])
def test_grouped_gemm_vs_fp64(ops, tune, m, e, topk, block, K, N, dtype, cfg, div1):
    weight, scale, w_ref = experts(e, K, N)
    qn, sn = native(ops, weight, scale)
    assert qn.shape == (e, K // 128, 64 * N) and sn.shape == (e, K // 128, N)
    seed_all(m)
    numel = m * topk
    ids = torch.stack([torch.randperm(e)[:topk] for _ in range(m)]).int().to(DEV)
    a_q, a_s = quant_cpu(scaled_randn(numel if div1 else m, K))  # on the CPU: the reference does not depend on code under test
    tw = torch.rand(m, topk, device=DEV)
    max_sorted = numel + e * (block - 1)
    sorted_ids = torch.empty(max_sorted, dtype=torch.int32, device=DEV)
    expert_ids = torch.zeros((max_sorted + block - 1) // block, dtype=torch.int32, device=DEV)
    post = torch.empty(1, dtype=torch.int32, device=DEV)
    ops.moe_align_block_size(ids, e, block, sorted_ids, expert_ids, post)
    tune(NMX_MOE_MXFP4=cfg)
    plan = ops.moe_mxfp4_mm_plan(numel, N, K, e, block)
    assert plan == int(cfg) if cfg else plan in (1, 2, 4)
    rows = torch.arange(numel, device=DEV) // (1 if div1 else topk)
    ref = torch.einsum("rk,enk->ren", dequant(a_q, a_s).to(DEV)[rows], w_ref.to(DEV))[torch.arange(numel, device=DEV), ids.flatten().long()]
    a_q, a_s = a_q.to(DEV), a_s.to(DEV)
    for use_tw in (False, True):
        out = torch.full((numel, N), 7.0, dtype=dtype, device=DEV)
        ops.moe_mxfp4_mm(out, a_q, a_s, qn, sn, tw if use_tw else None, sorted_ids, expert_ids, post, 1 if div1 else topk, block)
        want = ref * tw.flatten().double()[:, None] if use_tw else ref
        diff = compute_max_diff(out.double(), want)
        rounded = compute_max_diff(out.double(), want.to(dtype).double())  # the final cast taken out: fp32 accumulation only
        print(f"m={m} e={e} block={block} K={K} N={N} {dtype} splits={plan} tw={use_tw}: {diff:.3e} (rounded reference {rounded:.3e})")
        assert diff < (1e-3 if dtype == torch.float16 else 4e-3) and rounded < 1e-3  # test_mxfp4_gpu.gemm_check's bars


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("m", [1, 17])
def test_silu_and_mul_quant_bit_exact(ops, m, dtype):
    inter = 160
    seed_all(m)
    x = scaled_randn(m, 2 * inter, -6, 5)
    x[0, 32:64] = x[0, inter + 32:inter + 64] = 0  # an all-zero block of the product
    x = x.to(dtype).to(DEV)
    y = torch.empty(m, inter, dtype=dtype, device=DEV)
    ops.silu_and_mul(y, x)
    q, s = ops.silu_and_mul_mxfp4_quant(x)
    q_ref, s_ref = quant_cpu(y.cpu())
    assert q.shape == (m, inter // 2) and s.shape == (m, inter // 32) and s_ref[0, 1] == 0
    assert torch.equal(s.cpu(), s_ref) and torch.equal(q.cpu(), q_ref)


def chain_ref(x, w13, w2, logits, topk, mm=torch.float64):
    """The layer on the CPU, rounding where the kernels do: quant_cpu(x), gate | up rounded to x.dtype, silu rounded, silu * up
    rounded, quant_cpu, w2, routing weight, sum over k. w13 [E, 2 I, H] and w2 [E, H, I] as dequantised; mm = the precision of
    the matmuls (float32 against float64 sets the bar of test_mxfp4_moe_method)."""
    weight, ids = torch.topk(torch.softmax(logits.double(), dim=-1), topk)
    weight = weight / weight.sum(dim=-1, keepdim=True)
    xq = dequant(*quant_cpu(x))
    out = torch.zeros(x.shape[0], w2.shape[1], dtype=torch.float64)
    for t in range(x.shape[0]):
        for j in range(topk):
            h = (xq[t].to(mm) @ w13[ids[t, j]].to(mm).T).to(x.dtype)
            n = h.shape[0] // 2
            act = (torch.nn.functional.silu(h[:n].float()).to(x.dtype).float() * h[n:].float()).to(x.dtype)
            out[t] += weight[t, j] * (dequant(*quant_cpu(act[None]))[0].to(mm) @ w2[ids[t, j]].to(mm).T).double()
    return out


def moe_case(m, e=8, hidden=512, inter=256):
    """(x [m, hidden] fp16, router logits, w13 experts, w2 experts); weight scales 2^-8 .. 2^-4 keep gate | up near 1"""
    w13, w2 = experts(e, hidden, 2 * inter, 119, 124), experts(e, inter, hidden, 119, 124)
    seed_all(m)
    return torch.randn(m, hidden).half(), torch.randn(m, e).half(), w13, w2


@pytest.mark.parametrize("m", [1, 40])
def test_mxfp4_moe_method(ops, m):
    from neuralmagic_vllm_amd.layers.quantization import get_quantization_config
    from neuralmagic_vllm_amd.layers.quantization.mxfp4 import MXFP4MoEMethod
    e, hidden, inter, topk = 8, 512, 256, 2
    x, logits, (q13, s13, w13_ref), (q2, s2, w2_ref) = moe_case(m)
    method = MXFP4MoEMethod(get_quantization_config("mxfp4").from_config({}))
    layer = torch.nn.Module()
    method.create_weights(layer, e, hidden, inter, torch.float16)
    assert layer.w13_weight.shape == q13.shape == (e, 2 * inter, hidden // 2) and layer.w13_weight_scale.shape == s13.shape
    assert layer.w2_weight.shape == q2.shape == (e, hidden, inter // 2) and layer.w2_weight_scale.shape == s2.shape
    for name, t in (("w13_weight", q13), ("w13_weight_scale", s13), ("w2_weight", q2), ("w2_weight_scale", s2)):
        assert getattr(layer, name).dtype == torch.uint8
        getattr(layer, name).data = t.to(DEV)
    method.process_weights_after_loading(layer)
    assert not hasattr(layer, "w13_weight") and not hasattr(layer, "w2_weight_scale")  # the checkpoint tensors are dropped
    assert layer.w13_q.shape == (e, hidden // 128, 128 * inter) and layer.w2_s.shape == (e, inter // 128, hidden)
    out = method.apply(layer, x.to(DEV), logits.to(DEV), topk)
    w13_ptr = layer.w13_q.data_ptr()
    diff = compute_max_diff(out.cpu().double(), chain_ref(x, w13_ref, w2_ref, logits, topk))
    print(f"m={m}: {diff:.3e}")
    # The bar. chain_ref with float32 matmuls against chain_ref in float64 on these inputs gives exactly 0.0 on the CPU (m = 1 and
    # m = 40): products of e2m1 values are exact and the fp32 sums over 512 / 256 of them round to the same fp16 gate | up, so no fp4
    # code flips - and 4 x 0 is a bar that no fp16 output meets, because the layer rounds twice where chain_ref does not: the out
    # rows (fp32 sum times the routing weight -> fp16) and their sum over k (-> fp16). Rounding to fp16 is a mean relative error of
    # 2^-12 / 1.44 = 1.7e-4 (test_mxfp4_gpu.gemm_check); two out rows and the sum are at most 3 x that = 5.1e-4, so the bar is the
    # project's fp16 bar against float64, 1e-3 - the rest is for the fp32 routing weights and for silu's expf differing from the
    # CPU's by an ulp, which rarely flips a code. A dropped top-k term is an error of 0.68 - 0.73 on these inputs (chain_ref with
    # topk = 1 against topk = 2). Observed on the MI355X: 2.54e-4 (m = 1), 2.59e-4 (m = 40).
    assert diff < 1e-3
    assert torch.equal(method.apply(layer, x.to(DEV), logits.to(DEV), topk), out) and layer.w13_q.data_ptr() == w13_ptr  # no second repack


def test_fused_experts_mxfp4_is_graph_capturable(ops, tune):
    from neuralmagic_vllm_amd.layers.fused_moe import fused_experts_mxfp4, fused_topk
    e, hidden, inter, m, topk = 8, 512, 256, 24, 2
    x, logits, (q13, s13, _), (q2, s2, _) = moe_case(m)
    w13_q, w13_s = native(ops, q13, s13)
    w2_q, w2_s = native(ops, q2, s2)
    x, logits = x.to(DEV), logits.float().to(DEV)
    tune(NMX_MOE_MXFP4="2")
    assert ops.moe_mxfp4_mm_plan(m * topk, hidden, inter, e, 16) == 2

    def run():
        tw, ids = fused_topk(x, logits, topk, True)
        return fused_experts_mxfp4(x, w13_q, w13_s, w2_q, w2_s, tw, ids)

    eager = run().clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = run()
        for _ in range(3):
            out.zero_()
            g.replay()
            side.synchronize()
            assert torch.equal(out, eager)
