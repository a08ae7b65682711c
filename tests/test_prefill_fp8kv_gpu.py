"""context_attention_fwd / PagedAttention.forward_prefix over an fp8 KV cache (k_cache [NB, Hkv, D/16, BS, 16], v_cache
[NB, Hkv, D, BS], uint8 = fp8(value / kv_scale)) against the fp32 torch restatement over the same bytes dequantised.
The bars are those of test_prefill_gpu.py: the conversion is exact and kv_scale enters in fp32."""
import random

import pytest
import torch

from util import ref_prefix_prefill, seed_all

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F8 = {"fp8": torch.float8_e4m3fn, "fp8_e4m3": torch.float8_e4m3fn, "fp8_e5m2": torch.float8_e5m2}
TOL = {torch.float16: dict(atol=2e-3, rtol=2e-3), torch.bfloat16: dict(atol=1.5e-2, rtol=1.5e-2)}


def make_case(heads, D, block_size, dtype, kvd, kv_scale, max_q, min_q=1, batch=4, max_ctx=200, cache_blocks=128):
    H, Hkv = heads
    query_lens = [random.randint(min_q, max_q) for _ in range(batch)]
    ctx_lens = [0, max_ctx - 3] + [random.randint(1, max_ctx) for _ in range(batch - 2)]  # a pure prefill; 197 = 6 * 32 + 5
    T = sum(query_lens)
    q, k, v = (torch.empty(T, h, D).uniform_(-1, 1).to(dtype) for h in (H, Hkv, Hkv))
    kc = (torch.empty(cache_blocks, Hkv, D // 16, block_size, 16).uniform_(-1, 1) / kv_scale).to(F8[kvd]).view(torch.uint8)
    vc = (torch.empty(cache_blocks, Hkv, D, block_size).uniform_(-1, 1) / kv_scale).to(F8[kvd]).view(torch.uint8)
    max_blocks = (max_ctx + block_size - 1) // block_size + 1
    b_loc = torch.randperm(cache_blocks)[:batch * max_blocks].reshape(batch, max_blocks).to(torch.int32)
    for b, c in enumerate(ctx_lens):  # slots of the last block past the context: NaN in both formats
        if c % block_size:
            kc[int(b_loc[b, c // block_size]), :, :, c % block_size:, :] = 0x7f
            vc[int(b_loc[b, c // block_size]), :, :, c % block_size:] = 0x7f
    return dict(q=q, k=k, v=v, k_cache=kc, v_cache=vc, b_loc=b_loc,
                b_start_loc=torch.cumsum(torch.tensor([0] + query_lens[:-1]), 0).to(torch.int32),
                b_seq_len=torch.tensor([a + b for a, b in zip(query_lens, ctx_lens)], dtype=torch.int32),
                b_ctx_len=torch.tensor(ctx_lens, dtype=torch.int32), max_input_len=max(query_lens))


def check(c, dtype, kvd, kv_scale, alibi=None, window=None, out=None):
    from neuralmagic_vllm_amd.attention.ops.prefix_prefill import context_attention_fwd
    if out is None:
        g = {n: (t.to(DEV) if torch.is_tensor(t) else t) for n, t in c.items()}
        out = torch.zeros_like(g["q"])
        context_attention_fwd(g["q"], g["k"], g["v"], out, g["k_cache"], g["v_cache"], g["b_loc"], g["b_start_loc"],
                              g["b_seq_len"], g["b_ctx_len"], g["max_input_len"], None if alibi is None else alibi.to(DEV),
                              window, kv_cache_dtype=kvd, kv_scale=kv_scale)
    deq = [t.view(F8[kvd]).float() * kv_scale for t in (c["k_cache"], c["v_cache"])]
    ref = ref_prefix_prefill(c["q"], c["k"], c["v"], deq[0], deq[1], c["b_loc"], c["b_start_loc"], c["b_seq_len"],
                             c["b_ctx_len"], alibi, window or 0)
    assert not torch.isnan(out).any()
    torch.testing.assert_close(out.cpu().float(), ref, **TOL[dtype])


BASE = (128, 16, torch.float16, "fp8", 0.37)


@pytest.mark.parametrize("D,block_size,dtype,kvd,kv_scale", [
    BASE, (64, 16) + BASE[2:], (256, 16) + BASE[2:], (128, 8) + BASE[2:], (128, 32) + BASE[2:],
    BASE[:2] + (torch.bfloat16, "fp8", 0.37), BASE[:2] + (torch.float16, "fp8_e5m2", 0.37),
    BASE[:2] + (torch.bfloat16, "fp8_e5m2", 1.0), BASE[:4] + (1.0, )])
def test_shared_kernel(ops, D, block_size, dtype, kvd, kv_scale):
    """>= 64 new tokens, head size a multiple of 64: the workgroup-shared kernel (at D = 64 half the threads hold no K piece)."""
    seed_all(0)
    check(make_case((8, 2), D, block_size, dtype, kvd, kv_scale, max_q=150, min_q=64), dtype, kvd, kv_scale)


@pytest.mark.parametrize("heads", [(8, 8), (8, 2), (8, 1)])
@pytest.mark.parametrize("D,max_q,block_size", [(80, 150, 16), (96, 150, 8), (112, 150, 32), (128, 40, 16)])
def test_per_wave_kernel(ops, heads, D, max_q, block_size):
    """Head sizes off the 64 grid (80 and 112: an odd number of 16-byte K chunks) and short chunks."""
    seed_all(1)
    check(make_case(heads, D, block_size, torch.float16, "fp8", 0.37, max_q=max_q), torch.float16, "fp8", 0.37)


@pytest.mark.parametrize("gq", ["1", "2", "11", "12", "14"])
def test_forced_forms(ops, tune, gq):
    seed_all(2)
    tune(NMX_PREFILL_GQ=gq)
    check(make_case((8, 2), 128, 16, torch.bfloat16, "fp8_e5m2", 0.37, max_q=150), torch.bfloat16, "fp8_e5m2", 0.37)


@pytest.mark.parametrize("D", [128, 80])
@pytest.mark.parametrize("mask", ["alibi", "window"])
def test_masking(ops, D, mask):
    """Tiles where the mask-free path must not be taken while the kv_scale factor is applied."""
    seed_all(3)
    c = make_case((8, 2), D, 16, torch.float16, "fp8", 0.37, max_q=150, min_q=64)
    check(c, torch.float16, "fp8", 0.37, alibi=torch.rand(8) * 0.2 if mask == "alibi" else None,
          window=50 if mask == "window" else None)


def test_forward_prefix_and_errors(ops):
    """The public route: the cache written by reshape_and_cache(..., "fp8", kv_scale), read by forward_prefix."""
    from neuralmagic_vllm_amd.attention.ops.paged_attn import PagedAttention
    seed_all(4)
    c = make_case((8, 2), 128, 16, torch.float16, "fp8", 0.37, max_q=100)
    g = {n: (t.to(DEV) if torch.is_tensor(t) else t) for n, t in c.items()}
    slots = torch.cat([c["b_loc"][b, torch.arange(int(n)) // 16].long() * 16 + torch.arange(int(n)) % 16
                       for b, n in enumerate(c["b_ctx_len"])])
    kv = torch.empty(2, len(slots), 2, 128).uniform_(-1, 1).to(torch.float16).to(DEV)
    ops.reshape_and_cache(kv[0], kv[1], g["k_cache"], g["v_cache"], slots.to(DEV), "fp8", 0.37)
    qsl = torch.cat([g["b_start_loc"], torch.tensor([c["q"].shape[0]], dtype=torch.int32, device=DEV)])
    out = PagedAttention.forward_prefix(g["q"], g["k"], g["v"], g["k_cache"], g["v_cache"], g["b_loc"], qsl, g["b_seq_len"],
                                        g["b_ctx_len"], c["max_input_len"], None, None, kv_cache_dtype="fp8", kv_scale=0.37)
    c.update(k_cache=g["k_cache"].cpu(), v_cache=g["v_cache"].cpu())
    check(c, torch.float16, "fp8", 0.37, out=out)
    args = (g["q"], g["k"], g["v"], g["k_cache"], g["v_cache"], g["b_loc"], qsl, g["b_seq_len"], g["b_ctx_len"],
            c["max_input_len"], None, None)
    with pytest.raises(RuntimeError, match="cache of the same dtype"):
        PagedAttention.forward_prefix(*args)
    with pytest.raises(RuntimeError, match="one-byte"):
        PagedAttention.forward_prefix(*args[:3], torch.zeros(4, 2, 16, 16, 8, dtype=torch.float16, device=DEV),
                                      torch.zeros(4, 2, 128, 16, dtype=torch.float16, device=DEV), *args[5:],
                                      kv_cache_dtype="fp8", kv_scale=0.37)
