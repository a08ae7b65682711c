"""GPU tests of the int4 mixture-of-experts path on the CDNA4-native W4A16 layout (include/nmx.h): the grouped GEMM against fp64
for both block forms, every K split, padding slots, empty experts and blocks past the padded length; the GPTQNativeMoEMethod
layer; graph capture."""
import pytest
import torch

from oracle import packing
from util import compute_max_diff, seed_all

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_EXPERTS = {}


def experts(E, K, N, group, dtype=torch.float16, scale=1.0):
    """E quantised [K, N] experts, made once per shape: (w_ref fp64 [E, K, N], checkpoint qweight [E, K / 8, N], scales [E, G, N]),
    all on the GPU. w_ref is what the scales the kernel sees (rounded to dtype) dequantise to."""
    key = (E, K, N, group, dtype, scale)
    if key not in _EXPERTS:
        seed_all(E + K)
        refs, qws, ss = [], [], []
        for _ in range(E):
            _, q_w, s, _, _ = packing.quantize_weights(torch.randn(K, N, dtype=torch.float16) * scale, 4, K if group == -1 else group)
            s = s.to(dtype)
            refs.append(((q_w.reshape(-1, K // s.shape[0], N) - 8).double() * s.double()[:, None, :]).reshape(K, N))
            qws.append(packing.gptq_pack(q_w, 4, K, N))
            ss.append(s)
        _EXPERTS[key] = tuple(torch.stack(t).to(DEV) for t in (refs, qws, ss))
    return _EXPERTS[key]


def native(ops, qweight, scales):
    pairs = [ops.w4a16_repack(q, s) for q, s in zip(qweight, scales)]
    return torch.stack([q for q, _ in pairs]), torch.stack([s for _, s in pairs])


# K = 896: 7 units, uneven slices across the 4 waves and across splits; N = 192: 3 column groups, one staged wave is past N
@pytest.mark.parametrize("K,N,group,dtype,bar,cfg,div1", [
    (896, 192, 128, torch.float16, 1e-3, None, False), (896, 192, 128, torch.float16, 1e-3, "4", True),
    (1024, 256, -1, torch.float16, 1e-3, "2", False), (1024, 256, -1, torch.float16, 1e-3, "1", True),
    (896, 192, 128, torch.bfloat16, 4e-3, "2", True)])
@pytest.mark.parametrize("m,e,topk,block", [(1, 8, 2, 16), (33, 8, 2, 16), (222, 8, 2, 64), (40, 64, 6, 16)])
def test_grouped_gemm_vs_fp64(ops, tune, m, e, topk, block, K, N, group, dtype, bar, cfg, div1):
    w_ref, qweight, scales = experts(e, K, N, group, dtype)
    qn, sn = native(ops, qweight, scales)
    assert qn.shape == (e, K // 128, 16 * N) and sn.shape == scales.shape
    seed_all(m)
    numel = m * topk
    ids = torch.stack([torch.randperm(e)[:topk] for _ in range(m)]).int().to(DEV)
    a = torch.randn(numel if div1 else m, K, device=DEV).to(dtype)
    tw = torch.rand(m, topk, device=DEV)
    max_sorted = numel + e * (block - 1)
    sorted_ids = torch.empty(max_sorted, dtype=torch.int32, device=DEV)
    expert_ids = torch.zeros((max_sorted + block - 1) // block, dtype=torch.int32, device=DEV)
    post = torch.empty(1, dtype=torch.int32, device=DEV)
    ops.moe_align_block_size(ids, e, block, sorted_ids, expert_ids, post)
    tune(NMX_MOE_W4A16=cfg)
    plan = ops.moe_w4a16_mm_plan(numel, N, K, e, block)
    assert plan == int(cfg) if cfg else plan in (1, 2, 4)
    rows = torch.arange(numel, device=DEV) // (1 if div1 else topk)
    ref = torch.einsum("rk,ekn->ren", a.double()[rows], w_ref)[torch.arange(numel, device=DEV), ids.flatten().long()]
    for use_tw in (False, True):
        out = torch.full((numel, N), 7.0, dtype=dtype, device=DEV)
        ops.moe_w4a16_mm(out, a, qn, sn, tw if use_tw else None, sorted_ids, expert_ids, post, 1 if div1 else topk, block)
        want = ref * tw.flatten().double()[:, None] if use_tw else ref
        diff = compute_max_diff(out.double(), want)
        print(f"m={m} e={e} block={block} K={K} N={N} group={group} {dtype} splits={plan} tw={use_tw}: {diff:.3e}")
        assert diff < bar


def moe_fp64(x, w13, w2, logits, topk):
    """tests/test_moe_gpu.py torch_moe in fp64 (renormalised), w13 [E, H, 2 I] and w2 [E, I, H] as dequantised."""
    weight, ids = torch.topk(torch.softmax(logits.double(), dim=-1), topk)
    weight = weight / weight.sum(dim=-1, keepdim=True)
    out = torch.zeros_like(x, dtype=torch.float64)
    for t in range(x.shape[0]):
        for j in range(topk):
            h = x[t].double() @ w13[ids[t, j]]
            n = h.shape[0] // 2
            out[t] += weight[t, j] * ((torch.nn.functional.silu(h[:n]) * h[n:]) @ w2[ids[t, j]])
    return out


def native_config(**kw):
    from neuralmagic_vllm_amd.layers.quantization import get_quantization_config
    return get_quantization_config("gptq_native").from_config({"bits": 4, "group_size": 128, "desc_act": False, "sym": True, **kw})


@pytest.mark.parametrize("group", [128, -1])
@pytest.mark.parametrize("m", [1, 40])
def test_gptq_native_moe_method(ops, m, group):
    from neuralmagic_vllm_amd.layers.quantization.gptq_native import GPTQNativeMoEMethod
    e, hidden, inter, topk = 8, 512, 256, 2
    method = GPTQNativeMoEMethod(native_config(group_size=group))
    layer = torch.nn.Module()
    method.create_weights(layer, e, hidden, inter, torch.float16)
    w13_ref, q13, s13 = experts(e, hidden, 2 * inter, group, scale=0.1)
    w2_ref, q2, s2 = experts(e, inter, hidden, group, scale=0.1)
    assert layer.w13_qweight.shape == q13.shape and layer.w13_scales.shape == s13.shape
    assert layer.w2_qweight.shape == q2.shape and layer.w2_scales.shape == s2.shape
    for name, t in (("w13_qweight", q13), ("w13_scales", s13), ("w2_qweight", q2), ("w2_scales", s2)):
        getattr(layer, name).data = t.clone()
    method.process_weights_after_loading(layer)
    assert not hasattr(layer, "w13_qweight") and layer.w13_q.shape == (e, hidden // 128, 32 * inter)
    seed_all(m)
    x = torch.randn(m, hidden, dtype=torch.float16, device=DEV) / 10
    logits = torch.randn(m, e, dtype=torch.float16, device=DEV)
    out = method.apply(layer, x, logits, topk)
    w13_ptr = layer.w13_q.data_ptr()
    assert torch.allclose(out.double(), moe_fp64(x, w13_ref, w2_ref, logits, topk), atol=1e-2, rtol=0)  # test_fused_moe's bar
    assert torch.equal(method.apply(layer, x, logits, topk), out) and layer.w13_q.data_ptr() == w13_ptr  # no second repack


@pytest.mark.parametrize("kw", [{"desc_act": True, "group_size": 128}, {"bits": 8}])
def test_gptq_native_moe_refuses(ops, kw):
    from neuralmagic_vllm_amd.layers.quantization.gptq_native import GPTQNativeMoEMethod
    with pytest.raises(ValueError):
        GPTQNativeMoEMethod(native_config(**kw)).create_weights(torch.nn.Module(), 8, 512, 256, torch.float16)


def test_fused_experts_w4a16_is_graph_capturable(ops, tune):
    from neuralmagic_vllm_amd.layers.fused_moe import fused_experts_w4a16, fused_topk
    e, hidden, inter, m, topk = 8, 512, 256, 24, 2
    _, q13, s13 = experts(e, hidden, 2 * inter, 128, scale=0.1)
    _, q2, s2 = experts(e, inter, hidden, 128, scale=0.1)
    w13_q, w13_s = native(ops, q13, s13)
    w2_q, w2_s = native(ops, q2, s2)
    seed_all(4)
    x = torch.randn(m, hidden, dtype=torch.float16, device=DEV) / 10
    logits = torch.randn(m, e, device=DEV)
    tune(NMX_MOE_W4A16="2")
    assert ops.moe_w4a16_mm_plan(m * topk, hidden, inter, e, 16) == 2

    def run():
        tw, ids = fused_topk(x, logits, topk, True)
        return fused_experts_w4a16(x, w13_q, w13_s, w2_q, w2_s, tw, ids)

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
