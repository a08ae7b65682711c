"""GPU tests of the tall (128 rows per workgroup) W4A16 GEMM on the CDNA4-native layout: forced through NMX_W4A16 = "8,0,s"
against fp64 at every row / column-group / K-split edge, the default dispatch at 256 rows, the deferred form and the layer."""
import ctypes

import pytest
import torch

from oracle import packing
from util import compute_max_diff, seed_all

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHTS = [(896, 192, 128, torch.float16, 1e-3), (1024, 320, -1, torch.float16, 1e-3), (896, 192, 128, torch.bfloat16, 4e-3)]
_CASES = {}


def gemm_case(K, N, group, dtype):
    """One quantised weight per shape, repacked once; 257 activation rows and their fp64 product shared by every case."""
    key = (K, N, group, dtype)
    if key not in _CASES:
        seed_all(1)
        w_ref, q_w, s, _, _ = packing.quantize_weights(torch.randn(K, N, dtype=torch.float16), 4, K if group == -1 else group)
        s = s.to(dtype)
        if dtype != torch.float16:  # the expected weights are those of the scales the kernel sees
            w_ref = (q_w.reshape(-1, K // s.shape[0], N) - 8).double() * s.double()[:, None, :]
        w_ref = w_ref.reshape(K, N).double()
        a = torch.randn(257, K, dtype=dtype)
        _CASES[key] = (a, a.double() @ w_ref, packing.gptq_pack(q_w, 4, K, N).to(DEV), s.to(DEV))
    return _CASES[key]


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("K,N,group,dtype,bar", WEIGHTS)
@pytest.mark.parametrize("m", [65, 127, 128, 129, 200, 256, 257])
def test_tall_vs_fp64(ops, tune, m, K, N, group, dtype, bar, s):
    a, ref, qweight, scales = gemm_case(K, N, group, dtype)
    qn, sn = ops.w4a16_repack(qweight, scales)
    tune(NMX_W4A16=f"8,0,{s}")
    mt, _, splits = ops.w4a16_gemm_plan(m, N, K)
    assert (mt, splits) == (8, s)
    out = ops.w4a16_gemm(a[:m].to(DEV), qn, sn, m, N, K)
    diff = compute_max_diff(out.cpu().double(), ref[:m])
    print(f"m={m} K={K} N={N} group={group} {dtype} s={s}: {diff:.3e}")
    assert out.shape == (m, N) and diff < bar


def test_default_dispatch(ops, tune):
    from neuralmagic_vllm_amd import _lib
    m, (K, N, group, dtype, bar) = 256, WEIGHTS[1]
    a, ref, qweight, scales = gemm_case(K, N, group, dtype)
    qn, sn = ops.w4a16_repack(qweight, scales)
    tune(NMX_W4A16=None)
    mt, _, splits = ops.w4a16_gemm_plan(m, N, K)
    assert mt == 4  # measured: the tall form is no default at any row count, 256 rows stay on 64-row blocks
    need = _lib.lib().nmx_w4a16_gemm_scratch_bytes(ctypes.c_int(m), ctypes.c_int(N), ctypes.c_int(K))
    assert need == (splits * m * N * 4 if splits > 1 else 0)
    out = ops.w4a16_gemm(a[:m].to(DEV), qn, sn, m, N, K)
    assert out.shape == (m, N) and compute_max_diff(out.cpu().double(), ref[:m]) < bar


def test_deferred(ops, tune):
    m, (K, N, group, dtype, _) = 130, WEIGHTS[1]
    a, _, qweight, scales = gemm_case(K, N, group, dtype)
    qn, sn = ops.w4a16_repack(qweight, scales)
    a = a[:m].to(DEV)
    tune(NMX_W4A16="8,0,2")
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


def test_gptq_native_layer(ops, tune):
    from neuralmagic_vllm_amd.layers.quantization import get_quantization_config
    seed_all(0)
    K, N, group = 512, 384, 128
    cfg = get_quantization_config("gptq_native").from_config({"bits": 4, "group_size": group, "desc_act": False, "sym": True})
    method = cfg.get_quant_method(None)
    layer = Layer()
    method.create_weights(layer, K, [256, 128], K, N, torch.float16)
    w_ref, q_w, s, _, _ = packing.quantize_weights(torch.randn(K, N, dtype=torch.float16), 4, group)
    for name, t in (("qweight", packing.gptq_pack(q_w, 4, K, N)), ("scales", s), ("g_idx", torch.arange(K, dtype=torch.int32) // group)):
        getattr(layer, name).data.copy_(t)
    for _, p in list(layer.named_parameters()):
        if not p.is_meta:
            p.data = p.data.to(DEV)
    x = torch.randn(3, 48, K, dtype=torch.float16)  # M = 144
    bias = torch.randn(N, dtype=torch.float16)
    tune(NMX_W4A16="8,0,0")
    assert ops.w4a16_gemm_plan(144, N, K)[0] == 8
    out = method.apply(layer, x.to(DEV), bias.to(DEV))
    ref = x.double() @ w_ref.double() + bias.double()
    assert out.shape == (3, 48, N) and compute_max_diff(out.cpu().double(), ref) < 1e-3
    assert torch.equal(out, method.apply(layer, x.to(DEV), bias.to(DEV)))
