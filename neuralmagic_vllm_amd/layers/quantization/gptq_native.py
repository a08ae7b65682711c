"""GPTQ checkpoints served through the CDNA4-native W4A16 / W8A16 layout (extension; no reference counterpart - the reference
repacks GPTQ -> Marlin at load, gptq_marlin.py:330-420). Opt-in: `quantization="gptq_native"`.

Same checkpoint keys and `create_weights` as GPTQMarlinConfig. The first `apply` repacks qweight / scales with
`ops.w4a16_repack` where `ops.w4a16_supported` says yes (4 or 8 bits, channel-wise or 128-k groups, no act-order), remembers
the bits on the layer and drops the checkpoint tensors; every other layer (groups of 32 / 64, act-order) takes the parent's
Marlin path unchanged."""
from typing import Optional

import torch

from neuralmagic_vllm_amd import _custom_ops as ops
from neuralmagic_vllm_amd.layers.quantization.base_config import replace_tensor
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
