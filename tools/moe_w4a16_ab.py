"""Times the grouped int4 expert GEMM (moe_w4a16_mm, CDNA4-native layout) on Mixtral-8x7B shapes the way a decode step sees it - a
chain of NL launches over NL distinct expert sets captured in a HIP graph, no profiler - against two yardsticks:
  (a) moe_mm on the SAME experts dequantised to fp16 (the only other graph-capturable path for the model), timed in the same call,
      the two alternating REPS times (the spread between repeats is printed);
  (b) the bytes of the experts actually touched (int4 words + scales, activations, outputs) over the time.
Every point is checked first: relative error of the int4 result against moe_mm on the dequantised weights, same routing.
Then NMX_MOE_W4A16 = 1 / 2 / 4 once each (the K-split rule of moe_w4_splits is read off these lines).

usage (on the GPU): python3 tools/moe_w4a16_ab.py [tokens ...] > moe_w4a16_ab.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from neuralmagic_vllm_amd import _custom_ops as ops  # noqa: E402
from neuralmagic_vllm_amd import _lib  # noqa: E402

E, TOPK, H, I = 8, 2, 4096, 14336
NL, REPS = 4, 3
dev = "cuda:0"


def time_graph(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def make_experts(K, N, gen):
    """One layer's experts: (qweight_native [E, K / 128, 16 N], scales_native [E, K / 128, N], fp16 w [E, N, K] = their dequantised form)."""
    qn, sn, wd = [], [], []
    sh = (4 * torch.arange(8, device=dev))[None, :, None]
    for _ in range(E):
        q = torch.randint(0, 16, (K, N), dtype=torch.int32, device=dev, generator=gen)
        s = (torch.rand(K // 128, N, device=dev, generator=gen) * 0.004 + 0.002).half()
        wd.append(((q - 8).half().view(K // 128, 128, N) * s[:, None, :]).view(K, N).t().contiguous())
        packed = (q.view(K // 8, 8, N).long() << sh).sum(dim=1)  # checkpoint format: code j of a word at bits 4 j
        packed = torch.where(packed >= 2**31, packed - 2**32, packed).to(torch.int32)
        a, b = ops.w4a16_repack(packed.contiguous(), s)
        qn.append(a)
        sn.append(b)
    return torch.stack(qn), torch.stack(sn), torch.stack(wd)


def main():
    tokens = [int(a) for a in sys.argv[1:]] or [1, 16, 64, 256]
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    print(f"# Mixtral-8x7B experts: E={E} top-{TOPK} H={H} I={I} fp16 group 128; {NL} distinct layers per graph, {REPS} alternating repeats")
    for name, K, N in (("w13", H, 2 * I), ("w2", I, H)):
        layers = [make_experts(K, N, gen) for _ in range(NL)]
        for m in tokens:
            numel = m * TOPK
            block = 16 if numel <= 16 * E else 64
            ids = torch.stack([torch.randperm(E, device=dev, generator=gen)[:TOPK] for _ in range(m)]).int()
            touched = int(torch.unique(ids).numel())
            max_sorted = numel + E * (block - 1)
            sorted_ids = torch.empty(max_sorted, dtype=torch.int32, device=dev)
            expert_ids = torch.empty((max_sorted + block - 1) // block, dtype=torch.int32, device=dev)
            post = torch.empty(1, dtype=torch.int32, device=dev)
            ops.moe_align_block_size(ids, E, block, sorted_ids, expert_ids, post)
            first = name == "w13"  # gate | up reads the token rows, down the pair rows and applies the routing weight
            a = torch.randn(m if first else numel, K, dtype=torch.float16, device=dev, generator=gen) / 8
            tw = None if first else torch.rand(numel, device=dev, generator=gen)
            div = TOPK if first else 1
            out = torch.empty(numel, N, dtype=torch.float16, device=dev)

            def run_int4():
                for qn, sn, _ in layers:
                    ops.moe_w4a16_mm(out, a, qn, sn, tw, sorted_ids, expert_ids, post, div, block)

            def run_fp16():
                for _, _, wd in layers:
                    ops.moe_mm(out, a, wd, tw, sorted_ids, expert_ids, post, div, block)

            _lib.set_tuning("NMX_MOE_W4A16", None)
            o4 = torch.zeros_like(out)
            ops.moe_w4a16_mm(o4, a, layers[0][0], layers[0][1], tw, sorted_ids, expert_ids, post, div, block)
            o16 = torch.zeros_like(out)
            ops.moe_mm(o16, a, layers[0][2], tw, sorted_ids, expert_ids, post, div, block)
            err = ((o4.float() - o16.float()).abs().mean() / o16.float().abs().mean()).item()
            by4 = touched * (K * N // 2 + (K // 128) * N * 2) + 2 * a.numel() + 2 * out.numel()
            by16 = touched * K * N * 2 + 2 * a.numel() + 2 * out.numel()
            plan = ops.moe_w4a16_mm_plan(numel, N, K, E, block)
            t4, t16 = [], []
            for _ in range(REPS):
                t4.append(time_graph(run_int4) / NL)
                t16.append(time_graph(run_fp16) / NL)
            f = lambda ts: " ".join(f"{t:8.2f}" for t in ts)  # noqa: E731
            print(f"{name} tokens={m:4d} block={block:2d} experts_touched={touched} relerr_int4_vs_fp16={err:.2e}", flush=True)
            print(f"   moe_w4a16_mm auto(splits={plan}) us: {f(t4)}   min {min(t4):8.2f}  {by4 / min(t4) / 1e3:7.0f} GB/s of {by4 / 1e6:7.1f} MB", flush=True)
            print(f"   moe_mm fp16               us: {f(t16)}   min {min(t16):8.2f}  {by16 / min(t16) / 1e3:7.0f} GB/s of {by16 / 1e6:7.1f} MB   "
                  f"fp16 / int4 time = {min(t16) / min(t4):.2f}", flush=True)
            forced = []
            for sp in ("1", "2", "4"):
                _lib.set_tuning("NMX_MOE_W4A16", sp)
                forced.append(f"splits={sp}: {time_graph(run_int4) / NL:8.2f}")
            _lib.set_tuning("NMX_MOE_W4A16", None)
            print("   moe_w4a16_mm forced        us: " + "   ".join(forced), flush=True)
        del layers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
