"""GPU tests of the CDNA4-native W4A16 layout (include/nmx.h): repack against a numpy restatement of the contract, the GEMM
against fp64 for every tile shape / K split, the deferred form, the gptq_native layer and graph capture."""
import numpy as np
import pytest
import torch

from oracle import packing
from util import compute_max_diff, seed_all

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def quantized(K, N, group, dtype=torch.float16, seed=0):
    """(w_ref fp64 [K, N], checkpoint qweight [K / 8, N], scales [G, N]) on the GPU."""
    seed_all(seed)
    w_ref, q_w, s, _, _ = packing.quantize_weights(torch.randn(K, N, dtype=torch.float16), 4, K if group == -1 else group)
    s = s.to(dtype)
    if dtype != torch.float16:  # the expected weights are those of the scales the kernel sees
        w_ref = (q_w.reshape(-1, K // s.shape[0], N) - 8).double() * s.double()[:, None, :]
    return w_ref.reshape(K, N).double(), packing.gptq_pack(q_w, 4, K, N).to(DEV), s.to(DEV)


@pytest.mark.parametrize("group", [128, -1])
def test_repack_layout(ops, group):
    K, N = 256, 128
    _, qweight, scales = quantized(K, N, group)
    qn, sn = ops.w4a16_repack(qweight, scales)
    assert qn.shape == (K // 128, N * 16) and sn.shape == scales.shape and sn.dtype == scales.dtype
    # the contract as index arithmetic: word [u][c][s][l = 16 g + r][t] <- column 64 c + 16 t + r, k = 128 u + 32 s + 8 g + j
    u, c, s, g, r, t = np.meshgrid(*[np.arange(d) for d in (K // 128, N // 64, 4, 4, 16, 4)], indexing="ij")
    src = qweight.cpu().numpy().view(np.uint32)[16 * u + 4 * s + g, 64 * c + 16 * t + r]  # codes j at nibble j
    want = np.zeros_like(src)
    for j, pj in enumerate([0, 4, 1, 5, 2, 6, 3, 7]):
        want |= ((src >> np.uint32(4 * j)) & np.uint32(0xf)) << np.uint32(4 * pj)
    assert np.array_equal(qn.cpu().numpy().view(np.uint32).reshape(-1), want.reshape(-1))
    G, c, g, t, j = np.meshgrid(*[np.arange(d) for d in (scales.shape[0], N // 64, 4, 4, 4)], indexing="ij")
    want_s = scales.cpu().view(torch.int16).numpy()[G, 64 * c + 16 * t + 4 * g + j]
    assert np.array_equal(sn.cpu().view(torch.int16).numpy().reshape(-1), want_s.reshape(-1))


_CASES = {}


def gemm_case(K, N, group, dtype):
    """One quantised weight per shape, shared by every row count and split (reference computed once per (shape, m))."""
    key = (K, N, group, dtype)
    if key not in _CASES:
        w_ref, qweight, scales = quantized(K, N, group, dtype, seed=1)
        a = torch.randn(130, K, dtype=dtype)
        _CASES[key] = (w_ref, a, a.double() @ w_ref, qweight, scales)
    return _CASES[key]


@pytest.mark.parametrize("cfg", [None, "0,0,1", "0,0,2", "0,0,3"])
@pytest.mark.parametrize("K,N,group,dtype,bar", [(896, 192, 128, torch.float16, 1e-3), (1024, 256, -1, torch.float16, 1e-3),
                                                 (896, 192, 128, torch.bfloat16, 4e-3)])
@pytest.mark.parametrize("m", [1, 5, 16, 17, 33, 64, 65, 130])
def test_gemm_vs_fp64(ops, tune, m, K, N, group, dtype, bar, cfg):
    _, a, ref, qweight, scales = gemm_case(K, N, group, dtype)
    qn, sn = ops.w4a16_repack(qweight, scales)
    tune(NMX_W4A16=cfg)
    out = ops.w4a16_gemm(a[:m].to(DEV), qn, sn, m, N, K)
    diff = compute_max_diff(out.cpu().double(), ref[:m])
    print(f"m={m} K={K} N={N} group={group} {dtype} cfg={cfg}: {diff:.3e}")
    assert out.shape == (m, N) and diff < bar


@pytest.mark.parametrize("m", [5, 48])
def test_deferred(ops, tune, m):
    K, N = 1024, 256
    _, a, _, qweight, scales = gemm_case(K, N, -1, torch.float16)
    qn, sn = ops.w4a16_repack(qweight, scales)
    a = a[:m].to(DEV)
    tune(NMX_W4A16="0,0,2")
    plain = ops.w4a16_gemm(a, qn, sn, m, N, K)
    g = ops.w4a16_gemm_deferred(a, qn, sn, m, N, K)
    assert g.splits == 2 and g.partial.shape == (2, m, N) and g.partial.dtype == torch.float32
    two = torch.empty(m, N // 2, dtype=torch.float16, device=DEV)
    ops.silu_and_mul(two, plain)
    one = torch.empty_like(two)
    ops.silu_and_mul_splitk(one, g)
    assert torch.equal(one, two)
    assert torch.equal(g.materialize(), plain)


class Layer(torch.nn.Module):
    pass


@pytest.mark.parametrize("bits,group,desc_act", [(4, 128, False), (4, -1, False), (4, 64, True)])
@pytest.mark.parametrize("m", [1, 48])
def test_gptq_native_method(ops, bits, group, desc_act, m):
    from neuralmagic_vllm_amd.layers.quantization import get_quantization_config
    seed_all(0)
    K, N = 512, 384
    cfg = get_quantization_config("gptq_native").from_config({"bits": bits, "group_size": group, "desc_act": desc_act, "sym": True})
    method = cfg.get_quant_method(None)
    layer = Layer()
    method.create_weights(layer, K, [256, 128], K, N, torch.float16)
    w_ref, q_w, s, g_idx, _ = packing.quantize_weights(torch.randn(K, N, dtype=torch.float16), bits, K if group == -1 else group, desc_act)
    if not desc_act:
        g_idx = torch.arange(K, dtype=torch.int32) // (K if group == -1 else group)
    for name, t in (("qweight", packing.gptq_pack(q_w, bits, K, N)), ("scales", s), ("g_idx", g_idx)):
        getattr(layer, name).data.copy_(t)
    for _, p in list(layer.named_parameters()):
        if not p.is_meta:
            p.data = p.data.to(DEV)
    x = torch.randn(3, m, K, dtype=torch.float16)
    bias = torch.randn(N, dtype=torch.float16)
    out = method.apply(layer, x.to(DEV), bias.to(DEV))
    ref = x.double() @ w_ref.double() + bias.double()
    assert out.shape == (3, m, N) and compute_max_diff(out.cpu().double(), ref) < 1e-3
    assert layer.w4a16_native == (not desc_act)
    assert layer.qweight.shape == ((K // 128, N * 16) if layer.w4a16_native else (K // 16, N * 2))
    assert torch.equal(out, method.apply(layer, x.to(DEV), bias.to(DEV)))  # second call: no repack
    two = torch.empty(3, m, N // 2, dtype=torch.float16, device=DEV)
    ops.silu_and_mul(two, method.apply(layer, x.to(DEV)))
    assert torch.equal(method.apply_silu_and_mul(layer, x.to(DEV)), two)


def test_graph_capture(ops, tune):
    m, K, N = 5, 1024, 256
    _, a, _, qweight, scales = gemm_case(K, N, -1, torch.float16)
    qn, sn = ops.w4a16_repack(qweight, scales)
    a = a[:m].to(DEV)
    tune(NMX_W4A16="0,0,2")
    eager = ops.w4a16_gemm(a, qn, sn, m, N, K)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.w4a16_gemm(a, qn, sn, m, N, K)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
