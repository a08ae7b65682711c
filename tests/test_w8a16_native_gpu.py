"""GPU tests of the 8-bit form of the CDNA4-native layout (include/nmx.h): repack against a numpy restatement of the contract,
the GEMM against fp64 for every tile shape / K split, the deferred form, the plan and the gptq_native layer at 8 bits.

Bars are those of the 4-bit file (exact integer operand, fp32 accumulation, one output rounding): 1e-3 fp16, 4e-3 bf16."""
import numpy as np
import pytest
import torch

from oracle import packing
from util import compute_max_diff, seed_all

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CASES = {}


def case(K, N, group, dtype=torch.float16):
    """(w_ref fp64 [K, N], a [130, K], a.double() @ w_ref, checkpoint qweight [K / 4, N], scales [G, N]), once per shape."""
    key = (K, N, group, dtype)
    if key not in _CASES:
        seed_all(1)
        w_ref, q_w, s, _, _ = packing.quantize_weights(torch.randn(K, N, dtype=torch.float16), 8, K if group == -1 else group)
        s = s.to(dtype)
        if dtype != torch.float16:  # the expected weights are those of the scales the kernel sees
            w_ref = (q_w.reshape(-1, K // s.shape[0], N) - 128).double() * s.double()[:, None, :]
        w_ref = w_ref.reshape(K, N).double()
        a = torch.randn(130, K, dtype=dtype)
        _CASES[key] = (w_ref, a, a.double() @ w_ref, packing.gptq_pack(q_w, 8, K, N).to(DEV), s.to(DEV))
    return _CASES[key]


@pytest.mark.parametrize("group", [128, -1])
def test_repack_layout(ops, group):
    K, N = 256, 128
    _, _, _, qweight, scales = case(K, N, group)
    assert ops.w4a16_supported(N, K, scales.shape[0], 8)
    qn, sn = ops.w4a16_repack(qweight, scales, num_bits=8)
    assert qn.shape == (K // 128, N * 32) and sn.shape == scales.shape and sn.dtype == scales.dtype
    # the contract: word [u][c][s][h][l = 16 g + r][w] <- column 64 c + 16 (2 h + (w >> 1)) + r, k = 128 u + 32 s + 8 g + 4 (w & 1) + i
    u, c, s, h, g, r, w = np.meshgrid(*[np.arange(d) for d in (K // 128, N // 64, 4, 2, 4, 16, 4)], indexing="ij")
    want = qweight.cpu().numpy().view(np.uint32)[32 * u + 8 * s + 2 * g + (w & 1), 64 * c + 16 * (2 * h + (w >> 1)) + r]
    assert np.array_equal(qn.cpu().numpy().view(np.uint32).reshape(-1), want.reshape(-1))
    G, c, g, t, j = np.meshgrid(*[np.arange(d) for d in (scales.shape[0], N // 64, 4, 4, 4)], indexing="ij")
    want_s = scales.cpu().view(torch.int16).numpy()[G, 64 * c + 16 * t + 4 * g + j]
    assert np.array_equal(sn.cpu().view(torch.int16).numpy().reshape(-1), want_s.reshape(-1))


@pytest.mark.parametrize("cfg", [None, "0,0,1", "0,0,2", "0,0,3", "1,8,0"])
@pytest.mark.parametrize("K,N,group,dtype,bar", [(896, 192, 128, torch.float16, 1e-3), (1024, 256, -1, torch.float16, 1e-3),
                                                 (896, 192, 128, torch.bfloat16, 4e-3)])
@pytest.mark.parametrize("m", [1, 5, 16, 17, 33, 64, 65, 130])
def test_gemm_vs_fp64(ops, tune, m, K, N, group, dtype, bar, cfg):
    _, a, ref, qweight, scales = case(K, N, group, dtype)
    qn, sn = ops.w4a16_repack(qweight, scales, num_bits=8)
    tune(NMX_W4A16=cfg)
    out = ops.w4a16_gemm(a[:m].to(DEV), qn, sn, m, N, K, num_bits=8)
    diff = compute_max_diff(out.cpu().double(), ref[:m])
    print(f"m={m} K={K} N={N} group={group} {dtype} cfg={cfg}: {diff:.3e}")
    assert out.shape == (m, N) and diff < bar


@pytest.mark.parametrize("m", [5, 48])
def test_deferred(ops, tune, m):
    K, N = 1024, 256
    _, a, _, qweight, scales = case(K, N, -1)
    qn, sn = ops.w4a16_repack(qweight, scales, num_bits=8)
    a = a[:m].to(DEV)
    tune(NMX_W4A16="0,0,2")
    plain = ops.w4a16_gemm(a, qn, sn, m, N, K, num_bits=8)
    g = ops.w4a16_gemm_deferred(a, qn, sn, m, N, K, num_bits=8)
    assert g.splits == 2 and g.partial.shape == (2, m, N) and g.partial.dtype == torch.float32
    two = torch.empty(m, N // 2, dtype=torch.float16, device=DEV)
    ops.silu_and_mul(two, plain)
    one = torch.empty_like(two)
    ops.silu_and_mul_splitk(one, g)
    assert torch.equal(one, two)
    assert torch.equal(g.materialize(), plain)


def test_plan_has_no_tall_form(ops, tune):
    tune(NMX_W4A16="8,0,0")
    assert ops.w4a16_gemm_plan(130, 256, 1024, num_bits=8)[0] == 4
    assert ops.w4a16_gemm_plan(130, 256, 1024)[0] == 8


class Layer(torch.nn.Module):
    pass


@pytest.mark.parametrize("group", [128, -1])
@pytest.mark.parametrize("m", [1, 48])
def test_gptq_native_method(ops, group, m):
    from neuralmagic_vllm_amd.layers.quantization import get_quantization_config
    seed_all(0)
    K, N = 512, 384
    cfg = get_quantization_config("gptq_native").from_config({"bits": 8, "group_size": group, "desc_act": False, "sym": True})
    method = cfg.get_quant_method(None)
    layer = Layer()
    method.create_weights(layer, K, [256, 128], K, N, torch.float16)
    w_ref, q_w, s, _, _ = packing.quantize_weights(torch.randn(K, N, dtype=torch.float16), 8, K if group == -1 else group)
    g_idx = torch.arange(K, dtype=torch.int32) // (K if group == -1 else group)
    for name, t in (("qweight", packing.gptq_pack(q_w, 8, K, N)), ("scales", s), ("g_idx", g_idx)):
        getattr(layer, name).data.copy_(t)
    for _, p in list(layer.named_parameters()):
        if not p.is_meta:
            p.data = p.data.to(DEV)
    x = torch.randn(3, m, K, dtype=torch.float16)
    bias = torch.randn(N, dtype=torch.float16)
    out = method.apply(layer, x.to(DEV), bias.to(DEV))
    ref = x.double() @ w_ref.double() + bias.double()
    assert out.shape == (3, m, N) and compute_max_diff(out.cpu().double(), ref) < 1e-3
    assert layer.w4a16_native is True and layer.qweight.shape == (K // 128, 32 * N)
    assert torch.equal(out, method.apply(layer, x.to(DEV), bias.to(DEV)))  # second call: no repack
    two = torch.empty(3, m, N // 2, dtype=torch.float16, device=DEV)
    ops.silu_and_mul(two, method.apply(layer, x.to(DEV)))
    assert torch.equal(method.apply_silu_and_mul(layer, x.to(DEV)), two)
