"""GPTQ checkpoints served through the CDNA4-native W4A16 / W8A16 layout (extension; no reference counterpart - the reference
repacks GPTQ -> Marlin at load, gptq_marlin.py:330-420). Opt-in: `quantization="gptq_native"`.

Same checkpoint keys and `create_weights` as GPTQMarlinConfig. The first `apply` repacks qweight / scales with
`ops.w4a16_repack` where `ops.w4a16_supported` says yes (4 or 8 bits, channel-wise or 128-k groups, no act-order), remembers
the bits on the layer and drops the checkpoint tensors; every other layer (groups of 32 / 64, act-order) takes the parent's
Marlin path unchanged.

`GPTQNativeMoEMethod(config)` serves int4 mixture-of-experts layers on the same layout (4 bits only, no fallback)."""
from typing import Optional

import torch
from torch.nn.parameter import Parameter

from neuralmagic_vllm_amd import _custom_ops as ops
from neuralmagic_vllm_amd.layers.quantization.base_config import QuantizeMethodBase, replace_tensor, set_weight_attrs
from neuralmagic_vllm_amd.layers.quantization.gptq_marlin import GPTQMarlinConfig, GPTQMarlinLinearMethod, GPTQMarlinState


class GPTQNativeConfig(GPTQMarlinConfig):

    def __repr__(self) -> str:
        return super().__repr__().replace("GPTQMarlinConfig", "GPTQNativeConfig", 1)

    @classmethod
    def get_name(cls) -> str:
        return "gptq_native"

    @classmethod
    def override_quantization_method(cls, hf_quant_cfg, user_quant) -> Optional[str]:
        # never an automatic upgrade: only when the user asked for it by name
        if user_quant == cls.get_name() and cls.is_marlin_compatible(hf_quant_cfg):
            return cls.get_name()
        return None

    def get_quant_method(self, layer: torch.nn.Module) -> Optional["GPTQNativeLinearMethod"]:
        return GPTQNativeLinearMethod(self)


class GPTQNativeLinearMethod(GPTQMarlinLinearMethod):

    def _repack(self, layer: torch.nn.Module) -> None:
        cfg = self.quant_config
        layer.w4a16_native = ops.w4a16_supported(layer.output_size_per_partition, layer.input_size_per_partition,
                                                 layer.scales.shape[0], cfg.weight_bits, cfg.desc_act)
        if not layer.w4a16_native:
            return super()._repack(layer)
        layer.w4a16_bits = cfg.weight_bits
        qweight_native, scales_native = ops.w4a16_repack(layer.qweight, layer.scales, num_bits=layer.w4a16_bits)
        replace_tensor(layer, "qweight", qweight_native)
        replace_tensor(layer, "scales", scales_native)
        layer.g_idx = None  # (no act-order on this path; qzeros stays on the meta device, as on the Marlin path)

    def _ready(self, layer: torch.nn.Module) -> bool:
        if layer.marlin_state == GPTQMarlinState.REPACK:
            layer.marlin_state = GPTQMarlinState.READY
            self._repack(layer)
        return layer.w4a16_native

    def apply(self, layer: torch.nn.Module, x: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not self._ready(layer):
            return super().apply(layer, x, bias)
        reshaped_x = x.reshape(-1, x.shape[-1])
        output = ops.w4a16_gemm(reshaped_x, layer.qweight, layer.scales, reshaped_x.shape[0], layer.output_size_per_partition,
                                layer.input_size_per_partition, num_bits=layer.w4a16_bits)
        if bias is not None:
            output.add_(bias)
        return output.reshape(x.shape[:-1] + (layer.output_size_per_partition, ))

    def apply_silu_and_mul(self, layer: torch.nn.Module, x: torch.Tensor) -> torch.Tensor:
        """SiluAndMul(apply(layer, x)): the deferred GEMM, its K-split slabs summed by the activation kernel. Same values as
        the two calls."""
        if not self._ready(layer):
            return super().apply_silu_and_mul(layer, x)
        reshaped_x = x.reshape(-1, x.shape[-1])
        g = ops.w4a16_gemm_deferred(reshaped_x, layer.qweight, layer.scales, reshaped_x.shape[0], layer.output_size_per_partition,
                                    layer.input_size_per_partition, num_bits=layer.w4a16_bits)
        act = torch.empty((reshaped_x.shape[0], layer.output_size_per_partition // 2), dtype=x.dtype, device=x.device)
        ops.silu_and_mul_splitk(act, g)
        return act.reshape(x.shape[:-1] + (layer.output_size_per_partition // 2, ))


class GPTQNativeMoEMethod(QuantizeMethodBase):
    """Mixture-of-experts method for int4 GPTQ checkpoints (used the way Fp8MoEMethod is): the experts stay in 4 bits, repacked
    once into the native layout, and `apply` runs the grouped int4 GEMMs of layers/fused_moe.py (`fused_experts_w4a16`). There is
    no other int4 MoE path to fall back to: `create_weights` refuses what the kernel does not take."""

    def __init__(self, quant_config: GPTQNativeConfig):
        self.quant_config = quant_config

    def create_weights(self, layer: torch.nn.Module, num_experts: int, hidden_size: int, intermediate_size: int,
                       params_dtype: torch.dtype, **extra_weight_attrs):
        cfg = self.quant_config
        if cfg.weight_bits != 4:
            raise ValueError(f"gptq_native MoE: 4-bit experts only, the checkpoint has bits = {cfg.weight_bits}")
        if cfg.desc_act:
            raise ValueError("gptq_native MoE: act-order (desc_act = True) checkpoints are not supported")
        shapes = {}
        for name, size_k, size_n in (("w13", hidden_size, 2 * intermediate_size), ("w2", intermediate_size, hidden_size)):
            groups = 1 if cfg.group_size == -1 else max(size_k // cfg.group_size, 1)
            if size_k % 8 != 0 or not ops.w4a16_supported(size_n, size_k, groups, cfg.weight_bits, cfg.desc_act):
                raise ValueError(f"gptq_native MoE: {name} with K = {size_k}, N = {size_n}, group_size = {cfg.group_size} is not supported: "
                                 "K must be a multiple of 128, N of 64, and the scale groups channel-wise or 128 k")
            shapes[name] = (size_k, size_n, groups)
        layer.process_after_load = True
        layer.num_experts = num_experts
        for name, (size_k, size_n, groups) in shapes.items():
            qweight = Parameter(torch.empty(num_experts, size_k // 8, size_n, dtype=torch.int32), requires_grad=False)
            scales = Parameter(torch.empty(num_experts, groups, size_n, dtype=params_dtype), requires_grad=False)
            for pname, prm in ((f"{name}_qweight", qweight), (f"{name}_scales", scales)):
                layer.register_parameter(pname, prm)
                set_weight_attrs(prm, extra_weight_attrs)

    def process_weights_after_loading(self, layer: torch.nn.Module) -> None:
        if not getattr(layer, "process_after_load", False):
            return
        layer.process_after_load = False
        for name in ("w13", "w2"):
            qweight, scales = getattr(layer, f"{name}_qweight").data, getattr(layer, f"{name}_scales").data
            pairs = [ops.w4a16_repack(qweight[ex].contiguous(), scales[ex].contiguous()) for ex in range(layer.num_experts)]
            delattr(layer, f"{name}_qweight")  # the checkpoint tensors are dropped
            delattr(layer, f"{name}_scales")
            layer.register_parameter(f"{name}_q", Parameter(torch.stack([q for q, _ in pairs]), requires_grad=False))
            layer.register_parameter(f"{name}_s", Parameter(torch.stack([s for _, s in pairs]), requires_grad=False))

    def apply(self, layer: torch.nn.Module, x: torch.Tensor, router_logits: torch.Tensor, top_k: int, renormalize: bool = True) -> torch.Tensor:
        from neuralmagic_vllm_amd.layers.fused_moe import fused_experts_w4a16, fused_topk
        self.process_weights_after_loading(layer)
        topk_weights, topk_ids = fused_topk(x, router_logits, top_k, renormalize)
        return fused_experts_w4a16(x, layer.w13_q, layer.w13_s, layer.w2_q, layer.w2_s, topk_weights, topk_ids)
