"""Times the MXFP4 expert chain (mxfp4_quant -> moe_mxfp4_mm w13 -> silu_and_mul_mxfp4_quant -> moe_mxfp4_mm w2) on Mixtral-8x7B
shapes the way a decode step sees it - NL distinct layers captured in one HIP graph, no profiler - against the int4 chain of
fused_experts_w4a16 (moe_w4a16_mm w13 -> silu_and_mul -> moe_w4a16_mm w2) on the same routing, the two alternating REPS times in
one call (every repeat is printed; the minimum is compared). The WHOLE chain is timed because the fp4 design moves the activation
quantiser out of the GEMM into side launches: a GEMM-only comparison would flatter it. Then, per point:
  - the two grouped fp4 GEMMs alone, with the bytes of the experts actually touched over the time;
  - NMX_MOE_MXFP4 = 1 / 2 / 4 once each (the K-split rule of moe_mx_splits is read off these lines);
  - block_rows 16 / 32 / 64 once each (the block rule of fused_experts_mxfp4 is read off these lines).
Routing is uniform (randperm per token), fp16 only.

usage (on the GPU): python3 tools/moe_mxfp4_ab.py [tokens ...] > moe_mxfp4_ab.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from neuralmagic_vllm_amd import _custom_ops as ops  # noqa: E402
from neuralmagic_vllm_amd import _lib  # noqa: E402
from neuralmagic_vllm_amd.layers.fused_moe import mxfp4_block_rows  # noqa: E402
from tools.moe_w4a16_ab import time_graph  # noqa: E402

E, TOPK, H, I = 8, 2, 4096, 14336
NL, REPS = 4, 3
dev = "cuda:0"


def fp4_experts(K, N, gen):
    """One layer's MXFP4 experts [N, K] in the native layout: random codes, scales 2^-8 .. 2^-4."""
    pairs = [ops.mxfp4_repack(torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device=dev, generator=gen),
                              torch.randint(119, 124, (N, K // 32), dtype=torch.uint8, device=dev, generator=gen)) for _ in range(E)]
    return torch.stack([q for q, _ in pairs]), torch.stack([s for _, s in pairs])


def int4_experts(K, N, gen):
    """One layer's int4 experts [K, N], group 128, in the native W4A16 layout (as tools/moe_w4a16_ab.py)."""
    sh = (4 * torch.arange(8, device=dev))[None, :, None]
    pairs = []
    for _ in range(E):
        q = torch.randint(0, 16, (K, N), dtype=torch.int32, device=dev, generator=gen)
        s = (torch.rand(K // 128, N, device=dev, generator=gen) * 0.004 + 0.002).half()
        packed = (q.view(K // 8, 8, N).long() << sh).sum(dim=1)
        pairs.append(ops.w4a16_repack(torch.where(packed >= 2**31, packed - 2**32, packed).to(torch.int32).contiguous(), s))
    return torch.stack([q for q, _ in pairs]), torch.stack([s for _, s in pairs])


def align(ids, numel, block):
    max_sorted = numel + E * (block - 1)
    sorted_ids = torch.empty(max_sorted, dtype=torch.int32, device=dev)
    expert_ids = torch.empty((max_sorted + block - 1) // block, dtype=torch.int32, device=dev)
    post = torch.empty(1, dtype=torch.int32, device=dev)
    ops.moe_align_block_size(ids, E, block, sorted_ids, expert_ids, post)
    return sorted_ids, expert_ids, post


def main():
    tokens = [int(a) for a in sys.argv[1:]] or [1, 16, 64, 256]
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    print(f"# Mixtral-8x7B experts: E={E} top-{TOPK} H={H} I={I} fp16; {NL} distinct layers per graph, {REPS} alternating repeats; us per layer")
    fp4 = [(fp4_experts(H, 2 * I, gen), fp4_experts(I, H, gen)) for _ in range(NL)]
    int4 = [(int4_experts(H, 2 * I, gen), int4_experts(I, H, gen)) for _ in range(NL)]
    for m in tokens:
        numel = m * TOPK
        rule, rule4 = mxfp4_block_rows(numel, E), 16 if numel <= 16 * E else 64  # each chain under its own layer's block rule
        ids = torch.stack([torch.randperm(E, device=dev, generator=gen)[:TOPK] for _ in range(m)]).int()
        touched = int(torch.unique(ids).numel())
        x = torch.randn(m, H, dtype=torch.float16, device=dev, generator=gen)
        tw = torch.rand(numel, device=dev, generator=gen)
        gate_up = torch.empty(numel, 2 * I, dtype=torch.float16, device=dev)
        inter = torch.empty(numel, I, dtype=torch.float16, device=dev)
        out = torch.empty(numel, H, dtype=torch.float16, device=dev)
        x_q, x_s = ops.mxfp4_quant(x)
        i_q, i_s = ops.mxfp4_quant(torch.randn(numel, I, dtype=torch.float16, device=dev, generator=gen))
        routing = {b: align(ids, numel, b) for b in (16, 32, 64)}

        def fp4_chain(block=rule):
            srt, eid, post = routing[block]
            for (q13, s13), (q2, s2) in fp4:
                a_q, a_s = ops.mxfp4_quant(x)
                ops.moe_mxfp4_mm(gate_up, a_q, a_s, q13, s13, None, srt, eid, post, TOPK, block)
                b_q, b_s = ops.silu_and_mul_mxfp4_quant(gate_up)
                ops.moe_mxfp4_mm(out, b_q, b_s, q2, s2, tw, srt, eid, post, 1, block)

        def int4_chain():
            srt, eid, post = routing[rule4]
            for (q13, s13), (q2, s2) in int4:
                ops.moe_w4a16_mm(gate_up, x, q13, s13, None, srt, eid, post, TOPK, rule4)
                ops.silu_and_mul(inter, gate_up)
                ops.moe_w4a16_mm(out, inter, q2, s2, tw, srt, eid, post, 1, rule4)

        def fp4_gemms(block=rule):
            srt, eid, post = routing[block]
            for (q13, s13), (q2, s2) in fp4:
                ops.moe_mxfp4_mm(gate_up, x_q, x_s, q13, s13, None, srt, eid, post, TOPK, block)
                ops.moe_mxfp4_mm(out, i_q, i_s, q2, s2, tw, srt, eid, post, 1, block)

        _lib.set_tuning("NMX_MOE_MXFP4", None)
        plans = (ops.moe_mxfp4_mm_plan(numel, 2 * I, H, E, rule), ops.moe_mxfp4_mm_plan(numel, H, I, E, rule))
        t4, tf = [], []
        for _ in range(REPS):
            tf.append(time_graph(fp4_chain) / NL)
            t4.append(time_graph(int4_chain) / NL)
        tg = min(time_graph(fp4_gemms) / NL for _ in range(REPS))
        by = touched * 3 * H * I * (1 / 2 + 1 / 32) + numel * (H + I) * (1 / 2 + 1 / 32) + 2 * numel * (2 * I + H)
        f = lambda ts: " ".join(f"{t:8.2f}" for t in ts)  # noqa: E731
        print(f"tokens={m:4d} block={rule:2d} (int4 {rule4:2d}) experts_touched={touched} splits(w13, w2)={plans}", flush=True)
        print(f"   mxfp4 chain (quant, w13, silu+quant, w2) us: {f(tf)}   min {min(tf):8.2f}", flush=True)
        print(f"   int4 chain (w13, silu_and_mul, w2)       us: {f(t4)}   min {min(t4):8.2f}   int4 / mxfp4 time = {min(t4) / min(tf):.2f}", flush=True)
        print(f"   mxfp4 GEMMs alone (w13 + w2)             us: min {tg:8.2f}  {by / tg / 1e3:7.0f} GB/s of {by / 1e6:7.1f} MB", flush=True)
        forced = []
        for sp in ("1", "2", "4"):
            _lib.set_tuning("NMX_MOE_MXFP4", sp)
            forced.append(f"splits={sp}: {time_graph(fp4_gemms) / NL:8.2f}")
        _lib.set_tuning("NMX_MOE_MXFP4", None)
        print("   mxfp4 GEMMs forced splits                us: " + "   ".join(forced), flush=True)
        print("   mxfp4 GEMMs by block_rows (auto splits)  us: " +
              "   ".join(f"block={b}: {time_graph(lambda b=b: fp4_gemms(b)) / NL:8.2f}" for b in (16, 32, 64)), flush=True)


if __name__ == "__main__":
    main()
