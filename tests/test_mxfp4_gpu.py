"""GPU tests of MXFP4 on the native layout (include/nmx.h "MXFP4 on the native layout"): the activation quantiser bit for bit
against the contract written in torch, the repack against the layout as index arithmetic, the GEMM against float64 for every form
and K split, fused against two-step quantisation, and the mxfp4 layer with graph capture."""
import numpy as np
import pytest
import torch

from util import compute_max_diff, seed_all

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E2M1 = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float64)
EVEN_FIRST = torch.tensor([0, 2, 4, 6, 1, 3, 5, 7])  # argmin returns the first minimum: a tie goes to the even code
TIES = [5, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5]  # amax = 5: e = 0, every other value sits exactly between two grid points
K, N = 896, 192  # 7 units: uneven K slices and a peeled odd unit; 3 column groups: one staged wave past N
_CASES = {}


def dequant(q, scale):
    """codes [R, K / 2] uint8 (low nibble = even k), E8M0 bytes [R, K / 32] -> float64 [R, K]"""
    codes = torch.stack([q & 0xf, q >> 4], dim=-1).reshape(q.shape[0], -1).long()
    return E2M1[codes] * torch.exp2(scale.double() - 127).repeat_interleave(32, dim=1)


def quant_cpu(x):
    """The activation quantiser of the contract: [R, K] -> (codes [R, K / 2] uint8, scale bytes [R, K / 32] uint8)"""
    xb = x.double().reshape(x.shape[0], -1, 32)
    amax = xb.abs().amax(dim=2)
    e = (torch.frexp(amax)[1] - 3).clamp(-127, 127)  # frexp: amax = m * 2^exp, m in [0.5, 1): floor(log2) = exp - 1
    e[amax == 0] = -127
    y = (xb * torch.exp2(-e.double())[..., None]).abs().clamp(max=6)
    code = EVEN_FIRST[(y[..., None] - E2M1[EVEN_FIRST]).abs().argmin(dim=-1)] + 8 * torch.signbit(xb)
    code = code.reshape(x.shape[0], -1, 2)
    return (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8), (e + 127).to(torch.uint8)


def case(dtype):
    """(a [130, K], weight [N, K / 2], weight_scale [N, K / 32], float64 reference [130, N]). Rows and 32-k blocks of a carry
    different powers of two; row 0 holds an all-zero block, a block of exact ties and a block whose amax saturates to -6.
    Adjacent columns, tiles and blocks of the weights carry different scale bytes."""
    if dtype not in _CASES:
        seed_all(7)
        a = torch.randn(130, K) * torch.exp2(torch.randint(-6, 7, (130, K // 32)).float()).repeat_interleave(32, dim=1)
        a[0, 32:96] = 0
        a[0, 64:78] = torch.tensor(TIES + [-t for t in TIES])
        a[0, 96:128] = torch.randn(32) * 0.1
        a[0, 97] = -7.5
        a = a.to(dtype)
        weight = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8)
        weight_scale = torch.randint(118, 131, (N, K // 32), dtype=torch.uint8)
        ref = dequant(*quant_cpu(a)) @ dequant(weight, weight_scale).T
        _CASES[dtype] = (a, weight, weight_scale, ref)
    return _CASES[dtype]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("m", [1, 17])
def test_quant_bit_exact(ops, m, dtype):
    a = case(dtype)[0][:m, :256].contiguous()
    q, s = ops.mxfp4_quant(a.to(DEV))
    q_ref, s_ref = quant_cpu(a)
    assert torch.equal(s.cpu(), s_ref) and torch.equal(q.cpu(), q_ref)


def test_repack_layout(ops):
    _, weight, weight_scale, _ = case(torch.float16)
    w, ws, k, n = weight[:128, :128].contiguous(), weight_scale[:128, :8].contiguous(), 256, 128
    qn, sn = ops.mxfp4_repack(w.to(DEV), ws.to(DEV))
    assert qn.shape == (k // 128, n * 64) and qn.dtype == torch.uint8 and sn.shape == (k // 128, n) and sn.dtype == torch.int32
    u, T, g, i, b = np.meshgrid(*[np.arange(d) for d in (k // 128, n // 16, 4, 16, 16)], indexing="ij")
    assert np.array_equal(qn.cpu().numpy().reshape(-1), w.numpy()[16 * T + i, 64 * u + 16 * g + b].reshape(-1))
    u, c, g, i, t = np.meshgrid(*[np.arange(d) for d in (k // 128, n // 64, 4, 16, 4)], indexing="ij")  # byte t of lane 16 g + i
    assert np.array_equal(sn.cpu().view(torch.uint8).numpy().reshape(-1), ws.numpy()[64 * c + 16 * t + i, 4 * u + g].reshape(-1))


def gemm_check(ops, dtype, m, k, n):
    a, weight, weight_scale, ref = case(dtype)
    w, ws = weight[:n, :k // 2].contiguous(), weight_scale[:n, :k // 32].contiguous()
    if (k, n) != (K, N):
        ref = dequant(*quant_cpu(a[:m, :k])) @ dequant(w, ws).T
    qn, sn = ops.mxfp4_repack(w.to(DEV), ws.to(DEV))
    out = ops.mxfp4_gemm(a[:m, :k].contiguous().to(DEV), qn, sn, m, n, k)
    diff = compute_max_diff(out.cpu().double(), ref[:m])
    rounded = compute_max_diff(out.cpu().double(), ref[:m].to(dtype).double())  # the final cast taken out: fp32 accumulation only
    print(f"m={m} k={k} n={n} {dtype} plan={ops.mxfp4_gemm_plan(m, n, k)}: {diff:.3e} (against the rounded reference {rounded:.3e})")
    # Bars of the sibling native tests: 1e-3 fp16, 4e-3 bf16 - rounding an exact result to bf16 alone is a mean relative error of
    # 2^-9 / 1.44 = 1.36e-3 (a quarter ulp over the mean mantissa), so 1e-3 against float64 is out of reach of any bf16 output;
    # with the rounding taken out both dtypes are held to 1e-3.
    assert out.shape == (m, n) and out.dtype == dtype and diff < (1e-3 if dtype == torch.float16 else 4e-3) and rounded < 1e-3


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_gemm_one_unit(ops, dtype):
    """One unit, one column group, 16 rows, scales that differ per lane: the lane -> k mapping, the 4-register operand form and
    the op_sel byte selection of the fp4 MFMA."""
    gemm_check(ops, dtype, 16, 128, 64)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("m,cfg", [(m, cfg) for m in (1, 5, 16, 17, 33, 64, 65, 130) for cfg in (None, "0,0,1", "0,0,2", "0,0,3")] +
                         [(130, "1,8,1"), (130, "2,0,1"), (130, "4,0,2")])
def test_gemm_vs_fp64(ops, tune, m, cfg, dtype):
    tune(NMX_MXFP4=cfg)
    gemm_check(ops, dtype, m, K, N)
    forced = (int(v) for v in (cfg or "0,0,0").split(","))
    assert all(want == 0 or want == got for want, got in zip(forced, ops.mxfp4_gemm_plan(m, N, K)))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("m", [5, 48])
def test_fused_equals_two_step(ops, m, dtype):
    """Requantising a quantised activation is the identity, so the GEMM on dequant(mxfp4_quant(a)) is the same MFMAs on
    mxfp4_quant's bits: equal outputs say that the quantiser inside the GEMM is the op's."""
    a, weight, weight_scale, _ = case(dtype)
    qn, sn = ops.mxfp4_repack(weight.to(DEV), weight_scale.to(DEV))
    a = a[:m].contiguous().to(DEV)
    q, s = ops.mxfp4_quant(a)
    two_step = dequant(q.cpu(), s.cpu()).to(dtype)
    assert torch.equal(two_step.double(), dequant(q.cpu(), s.cpu()))  # representable: nothing is lost on the way back
    assert torch.equal(ops.mxfp4_gemm(a, qn, sn, m, N, K), ops.mxfp4_gemm(two_step.to(DEV), qn, sn, m, N, K))


class Layer(torch.nn.Module):
    pass


def test_mxfp4_layer_and_graph(ops):
    from neuralmagic_vllm_amd.layers.quantization import get_quantization_config
    k, n, dtype = 256, 128, torch.float16
    a, weight, weight_scale, _ = case(dtype)
    w, ws = weight[:n, :k // 2].contiguous(), weight_scale[:n, :k // 32].contiguous()
    method = get_quantization_config("mxfp4").from_config({}).get_quant_method(None)
    layer = Layer()
    method.create_weights(layer, k, [64, 64], k, n, dtype)
    layer.weight.data, layer.weight_scale.data = w.to(DEV), ws.to(DEV)
    x, bias = a[:15, :k].reshape(3, 5, k).contiguous(), torch.randn(n).to(dtype)
    ref = (dequant(*quant_cpu(x.reshape(15, k))) @ dequant(w, ws).T + bias.double()).reshape(3, 5, n)
    x, bias = x.to(DEV), bias.to(DEV)
    eager = method.apply(layer, x, bias)
    assert eager.shape == (3, 5, n) and compute_max_diff(eager.cpu().double(), ref) < 1e-3
    assert layer.weight.numel() == 0 and layer.weight_scale.numel() == 0  # the checkpoint tensors are dropped
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = method.apply(layer, x, bias)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
