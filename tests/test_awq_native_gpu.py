"""GPU tests of zero points on the CDNA4-native W4A16 layout (include/nmx.h "zeros_native"): the AWQ repack against the pinned
symmetric repack and the contract as index arithmetic, the GEMM against fp64 for every form / K split, the deferred form, the
awq_native layer and graph capture."""
import numpy as np
import pytest
import torch

from oracle import packing
from util import compute_max_diff, seed_all

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CASES = {}


def awq_case(K, N, group=128):
    """One AWQ checkpoint per shape: (codes q [K, N], zero points z [G, N], w fp64 = (q - z) * s, a [130, K], a @ w in fp64,
    qweight, qzeros, scales). A per-column offset of -5 .. 5 on randn makes the zero points differ between adjacent columns and
    between groups and reach 0 and 15 (checked on the CPU for the shapes used here: every value 0 .. 15 occurs, over 80 % of
    adjacent columns and about 40 % of consecutive groups differ) - with z near 8 everywhere the symmetric kernel would pass too."""
    if (K, N, group) not in _CASES:
        seed_all(K + N)
        w = torch.randn(K, N) + torch.linspace(-5, 5, N)[torch.randperm(N)]
        _, qweight, qzeros, scales = packing.awq_quantize(w, group)
        q, z = (torch.stack([(t >> (4 * o)) & 0xf for o in [0, 4, 1, 5, 2, 6, 3, 7]], dim=2).reshape(t.shape[0], N) for t in (qweight, qzeros))
        w_ref = ((q.reshape(-1, group, N) - z[:, None, :]).double() * scales.double()[:, None, :]).reshape(K, N)
        a = torch.randn(130, K, dtype=torch.float16)
        _CASES[K, N, group] = (q, z, w_ref, a, a.double() @ w_ref, qweight.to(DEV), qzeros.to(DEV), scales.to(DEV))
    return _CASES[K, N, group]


def test_repack_layout(ops):
    K, N = 256, 128
    q, z, _, _, _, qweight, qzeros, scales = awq_case(K, N)
    qn, sn, zn = ops.awq_native_repack(qweight, qzeros, scales)
    assert qn.shape == (K // 128, N * 16) and sn.shape == zn.shape == scales.shape and sn.dtype == zn.dtype == torch.float16
    assert torch.equal(qn, ops.w4a16_repack(packing.gptq_pack(q, 4, K, N).to(DEV), scales)[0])  # the pinned word order
    G, c, g, t, j = np.meshgrid(*[np.arange(d) for d in (K // 128, N // 64, 4, 4, 4)], indexing="ij")
    assert np.array_equal(sn.cpu().numpy().reshape(-1), scales.cpu().numpy()[G, 64 * c + 16 * t + 4 * g + j].reshape(-1))
    G, c, r, t = np.meshgrid(*[np.arange(d) for d in (K // 128, N // 64, 16, 4)], indexing="ij")  # [G][c][r][t] = 1024 + z
    assert np.array_equal(zn.cpu().numpy().reshape(-1), (1024 + z.numpy()[G, 64 * c + 16 * t + r]).astype(np.float16).reshape(-1))


@pytest.mark.parametrize("m,cfg", [(m, cfg) for m in (1, 5, 16, 17, 33, 64, 65, 130) for cfg in (None, "0,0,1", "0,0,2", "0,0,3")] +
                         [(130, "1,8,1"), (130, "2,0,1"), (130, "4,0,2"), (130, "8,0,0")])
def test_gemm_vs_fp64(ops, tune, m, cfg):
    K, N = 896, 192  # 7 units: uneven K slices and a peeled odd unit; 3 column groups: one staged wave past N
    _, _, _, a, ref, qweight, qzeros, scales = awq_case(K, N)
    qn, sn, zn = ops.awq_native_repack(qweight, qzeros, scales)
    tune(NMX_W4A16=cfg)
    out = ops.w4a16_gemm(a[:m].to(DEV), qn, sn, m, N, K, zeros_native=zn)
    diff = compute_max_diff(out.cpu().double(), ref[:m])
    plan = ops.w4a16_gemm_plan(m, N, K, zeros_native=zn)
    print(f"m={m} cfg={cfg} plan={plan}: {diff:.3e}")
    assert out.shape == (m, N) and diff < 1e-3
    mt, nw, splits = (int(v) for v in (cfg or "0,0,0").split(","))
    assert all(want == 0 or want == got for want, got in zip((min(mt, 4), nw, splits), plan))  # no 128-row form: mt = 8 reports 4


@pytest.mark.parametrize("m", [5, 48])
def test_deferred(ops, tune, m):
    K, N = 896, 192
    _, _, _, a, _, qweight, qzeros, scales = awq_case(K, N)
    qn, sn, zn = ops.awq_native_repack(qweight, qzeros, scales)
    a = a[:m].to(DEV)
    tune(NMX_W4A16="0,0,2")
    plain = ops.w4a16_gemm(a, qn, sn, m, N, K, zeros_native=zn)
    g = ops.w4a16_gemm_deferred(a, qn, sn, m, N, K, zeros_native=zn)
    assert g.splits == 2 and g.partial.shape == (2, m, N) and g.partial.dtype == torch.float32
    two, one = (torch.empty(m, N // 2, dtype=torch.float16, device=DEV) for _ in range(2))
    ops.silu_and_mul(two, plain)
    ops.silu_and_mul_splitk(one, g)
    assert torch.equal(one, two) and torch.equal(g.materialize(), plain)


class Layer(torch.nn.Module):
    pass


@pytest.mark.parametrize("m,group", [(1, 128), (48, 128), (48, 64)])
def test_awq_native_method(ops, m, group):
    from neuralmagic_vllm_amd.layers.quantization import get_quantization_config
    K, N = 512, 384
    _, _, w_ref, _, _, qweight, qzeros, scales = awq_case(K, N, group)
    method = get_quantization_config("awq_native").from_config({"w_bit": 4, "q_group_size": group, "zero_point": True}).get_quant_method(None)
    layer = Layer()
    method.create_weights(layer, K, [256, 128], K, N, torch.float16)
    for name, t in (("qweight", qweight), ("qzeros", qzeros), ("scales", scales)):
        getattr(layer, name).data = t.clone()
    method.process_weights_after_loading(layer)
    assert layer.w4a16_native == (group == 128)  # groups of 64: the parent's path (awq_gemm on the checkpoint tensors)
    assert all(getattr(layer, name).numel() == 0 for name in ("qweight", "qzeros", "scales")) == layer.w4a16_native
    seed_all(m)
    x, bias = torch.randn(3, m, K, dtype=torch.float16), torch.randn(N, dtype=torch.float16)
    out = method.apply(layer, x.to(DEV), bias.to(DEV))
    assert out.shape == (3, m, N) and compute_max_diff(out.cpu().double(), x.double() @ w_ref + bias.double()) < 1e-3
    assert torch.equal(out, method.apply(layer, x.to(DEV), bias.to(DEV)))
    two = torch.empty(3, m, N // 2, dtype=torch.float16, device=DEV)
    ops.silu_and_mul(two, method.apply(layer, x.to(DEV)))
    assert torch.equal(method.apply_silu_and_mul(layer, x.to(DEV)), two)


def test_graph_capture(ops, tune):
    m, K, N = 5, 896, 192
    _, _, _, a, _, qweight, qzeros, scales = awq_case(K, N)
    qn, sn, zn = ops.awq_native_repack(qweight, qzeros, scales)
    a = a[:m].to(DEV)
    tune(NMX_W4A16="0,0,2")
    eager = ops.w4a16_gemm(a, qn, sn, m, N, K, zeros_native=zn)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.w4a16_gemm(a, qn, sn, m, N, K, zeros_native=zn)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
