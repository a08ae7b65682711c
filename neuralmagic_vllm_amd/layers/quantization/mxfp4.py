"""OCP MXFP4 checkpoints (AMD Quark `w_mxfp4_a_mxfp4` exports) on the block-scaled fp4 MFMA of gfx950 (extension; no reference
counterpart). Opt-in: `quantization="mxfp4"`.

Weights are e2m1 with one E8M0 scale per 32 k: `weight` uint8 [N, K / 2], `weight_scale` uint8 [N, K / 32]. Activations stay
fp16 / bf16 up to the GEMM, which quantises them to MXFP4 per row and 32-k block as it loads them (the contract in include/nmx.h).
The first `apply` repacks the pair with `ops.mxfp4_repack` and drops the checkpoint tensors. There is no other fp4 path to fall
back to: `create_weights` refuses a shard the kernel does not take (K % 128 != 0 or N % 64 != 0).

Mixture-of-experts layers go through `MXFP4MoEMethod`: the experts' pairs stacked, the grouped fp4 GEMM (`ops.moe_mxfp4_mm`) on
activations quantised ONCE per token row by `ops.mxfp4_quant` / `ops.silu_and_mul_mxfp4_quant` (layers/fused_moe.py)."""
from typing import Any, Dict, List, Optional

import torch
from torch.nn.parameter import Parameter

from neuralmagic_vllm_amd import _custom_ops as ops
from neuralmagic_vllm_amd.layers.quantization.base_config import LinearMethodBase, QuantizationConfig, QuantizeMethodBase, set_weight_attrs

MX_BLOCK = 32


class MXFP4Config(QuantizationConfig):

    def __init__(self, block_size: int = MX_BLOCK):
        if block_size != MX_BLOCK:
            raise ValueError(f"mxfp4: the MX block is {MX_BLOCK} k-values, the checkpoint says {block_size}")
        self.block_size = block_size

    def __repr__(self) -> str:
        return f"MXFP4Config(block_size={self.block_size})"

    def get_name(self) -> str:
        return "mxfp4"

    def get_supported_act_dtypes(self) -> List[torch.dtype]:
        return [torch.half, torch.bfloat16]

    @staticmethod
    def get_config_filenames() -> List[str]:
        return ["quant_config.json", "quantize_config.json"]

    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> "MXFP4Config":
        return cls(cls.get_from_keys_or(config, ["block_size", "group_size"], MX_BLOCK))

    def get_quant_method(self, layer: torch.nn.Module) -> Optional["MXFP4LinearMethod"]:
        return MXFP4LinearMethod(self)


class MXFP4LinearMethod(LinearMethodBase):

    def __init__(self, quant_config: MXFP4Config):
        self.quant_config = quant_config

    def create_weights(self, layer: torch.nn.Module, input_size_per_partition: int, output_partition_sizes: List[int],
                       input_size: int, output_size: int, params_dtype: torch.dtype, **extra_weight_attrs):
        out_pp = sum(output_partition_sizes)
        if input_size_per_partition % 128 != 0 or out_pp % 64 != 0:
            raise ValueError(f"mxfp4: a shard with K = {input_size_per_partition}, N = {out_pp} is not supported: K must be a multiple "
                             "of 128 and N of 64 (this can be caused by too large tensor parallel size); there is no other fp4 path")
        weight = Parameter(torch.empty(out_pp, input_size_per_partition // 2, dtype=torch.uint8), requires_grad=False)
        set_weight_attrs(weight, {"input_dim": 1, "output_dim": 0, "packed_dim": 1, "pack_factor": 2})
        weight_scale = Parameter(torch.empty(out_pp, input_size_per_partition // MX_BLOCK, dtype=torch.uint8), requires_grad=False)
        set_weight_attrs(weight_scale, {"input_dim": 1, "output_dim": 0, "packed_dim": 1, "pack_factor": MX_BLOCK})
        for name, prm in (("weight", weight), ("weight_scale", weight_scale)):
            layer.register_parameter(name, prm)
            set_weight_attrs(prm, extra_weight_attrs)
        layer.input_size_per_partition = input_size_per_partition
        layer.output_size_per_partition = out_pp
        layer.mxfp4_native = None

    def process_weights_after_loading(self, layer: torch.nn.Module) -> None:
        if layer.mxfp4_native is not None:
            return
        layer.mxfp4_native = ops.mxfp4_repack(layer.weight.data.contiguous(), layer.weight_scale.data.contiguous())
        for name in ("weight", "weight_scale"):  # the checkpoint tensors are dropped
            getattr(layer, name).data = torch.empty(0, dtype=torch.uint8, device=layer.mxfp4_native[0].device)

    def apply(self, layer: torch.nn.Module, x: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        self.process_weights_after_loading(layer)
        k, n = layer.input_size_per_partition, layer.output_size_per_partition
        reshaped_x = x.reshape(-1, x.shape[-1]).contiguous()
        out = ops.mxfp4_gemm(reshaped_x, *layer.mxfp4_native, reshaped_x.shape[0], n, k)
        if bias is not None:
            out.add_(bias)
        return out.reshape(x.shape[:-1] + (n, ))


class MXFP4MoEMethod(QuantizeMethodBase):
    """Mixture-of-experts method for MXFP4 checkpoints (used the way GPTQNativeMoEMethod is): the experts stay in fp4, repacked once
    into the native layout, and `apply` runs the grouped fp4 GEMMs of layers/fused_moe.py (`fused_experts_mxfp4`). There is no other
    fp4 MoE path to fall back to: `create_weights` refuses what the kernel does not take."""

    def __init__(self, quant_config: MXFP4Config):
        self.quant_config = quant_config

    def create_weights(self, layer: torch.nn.Module, num_experts: int, hidden_size: int, intermediate_size: int,
                       params_dtype: torch.dtype, **extra_weight_attrs):
        if hidden_size % 128 != 0 or intermediate_size % 128 != 0:
            raise ValueError(f"mxfp4 MoE: hidden_size = {hidden_size} and intermediate_size = {intermediate_size} must be multiples of "
                             "128 (this can be caused by too large tensor parallel size); there is no other fp4 path")
        layer.process_after_load = True
        layer.num_experts = num_experts
        for name, size_k, size_n in (("w13", hidden_size, 2 * intermediate_size), ("w2", intermediate_size, hidden_size)):
            weight = Parameter(torch.empty(num_experts, size_n, size_k // 2, dtype=torch.uint8), requires_grad=False)
            weight_scale = Parameter(torch.empty(num_experts, size_n, size_k // MX_BLOCK, dtype=torch.uint8), requires_grad=False)
            for pname, prm in ((f"{name}_weight", weight), (f"{name}_weight_scale", weight_scale)):
                layer.register_parameter(pname, prm)
                set_weight_attrs(prm, extra_weight_attrs)

    def process_weights_after_loading(self, layer: torch.nn.Module) -> None:
        if not getattr(layer, "process_after_load", False):
            return
        layer.process_after_load = False
        for name in ("w13", "w2"):
            weight, scale = getattr(layer, f"{name}_weight").data, getattr(layer, f"{name}_weight_scale").data
            pairs = [ops.mxfp4_repack(weight[ex].contiguous(), scale[ex].contiguous()) for ex in range(layer.num_experts)]
            delattr(layer, f"{name}_weight")  # the checkpoint tensors are dropped
            delattr(layer, f"{name}_weight_scale")
            layer.register_parameter(f"{name}_q", Parameter(torch.stack([q for q, _ in pairs]), requires_grad=False))
            layer.register_parameter(f"{name}_s", Parameter(torch.stack([s for _, s in pairs]), requires_grad=False))

    def apply(self, layer: torch.nn.Module, x: torch.Tensor, router_logits: torch.Tensor, top_k: int, renormalize: bool = True) -> torch.Tensor:
        from neuralmagic_vllm_amd.layers.fused_moe import fused_experts_mxfp4, fused_topk
        self.process_weights_after_loading(layer)
        topk_weights, topk_ids = fused_topk(x, router_logits, top_k, renormalize)
        return fused_experts_mxfp4(x, layer.w13_q, layer.w13_s, layer.w2_q, layer.w2_s, topk_weights, topk_ids)
