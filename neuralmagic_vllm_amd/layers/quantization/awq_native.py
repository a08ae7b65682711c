"""AWQ checkpoints served through the CDNA4-native W4A16 layout with zero points (extension; no reference counterpart).
Opt-in: `quantization="awq_native"`; `quantization="awq"` is unchanged.

Same checkpoint keys and `create_weights` as AWQConfig. `process_weights_after_loading` repacks qweight / qzeros / scales with
`ops.awq_native_repack` where `ops.awq_native_supported` says yes (K % 128 == 0, N % 64 == 0, groups of 128) and the scales are
fp16, and drops the checkpoint tensors as the parent does; every other layer takes the parent's path unchanged (Marlin repack or
awq_gemm)."""
import os
from typing import Optional

import torch

from neuralmagic_vllm_amd import _custom_ops as ops
from neuralmagic_vllm_amd.layers.quantization.awq import AWQConfig, AWQLinearMethod


class AWQNativeConfig(AWQConfig):

    def __repr__(self) -> str:
        return super().__repr__().replace("AWQConfig", "AWQNativeConfig", 1)

    def get_name(self) -> str:
        return "awq_native"

    def get_quant_method(self, layer: torch.nn.Module) -> Optional["AWQNativeLinearMethod"]:
        return AWQNativeLinearMethod(self)


class AWQNativeLinearMethod(AWQLinearMethod):

    def process_weights_after_loading(self, layer: torch.nn.Module) -> None:
        qw = layer.qweight
        if not qw.is_cuda or getattr(layer, "w4a16_native", None) is not None:
            return
        k, n = qw.shape[0], qw.shape[1] * self.quant_config.pack_factor
        layer.w4a16_native = ops.awq_native_supported(n, k, layer.scales.shape[0]) and layer.scales.dtype == torch.float16
        if not layer.w4a16_native:
            return super().process_weights_after_loading(layer)
        layer.native_q, layer.native_s, layer.native_z = ops.awq_native_repack(qw.data.contiguous(), layer.qzeros.data.contiguous(),
                                                                               layer.scales.data.contiguous())
        layer.native_shape = (k, n)
        # as the parent: the repacked layer never reads the checkpoint layout again for fp16 activations
        if os.environ.get("NMX_AWQ_KEEP_CHECKPOINT_LAYOUT", "0") != "1":
            for name in ("qweight", "qzeros", "scales"):
                getattr(layer, name).data = torch.empty(0, dtype=getattr(layer, name).dtype, device=qw.device)

    def _native(self, layer: torch.nn.Module, x: torch.Tensor) -> bool:
        if not getattr(layer, "w4a16_native", False):
            return False
        if x.dtype != torch.float16:
            if layer.qweight.numel() == 0:
                raise RuntimeError("AWQ layer repacked for fp16 activations was called with " + str(x.dtype) +
                                   " (set NMX_AWQ_KEEP_CHECKPOINT_LAYOUT=1 to keep the checkpoint-layout tensors for other dtypes)")
            return False
        return True

    def apply(self, layer: torch.nn.Module, x: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not self._native(layer, x):
            return super().apply(layer, x, bias)
        k, n = layer.native_shape
        reshaped_x = x.reshape(-1, x.shape[-1]).contiguous()
        out = ops.w4a16_gemm(reshaped_x, layer.native_q, layer.native_s, reshaped_x.shape[0], n, k, zeros_native=layer.native_z)
        if bias is not None:
            out.add_(bias)
        return out.reshape(x.shape[:-1] + (n, ))

    def apply_silu_and_mul(self, layer: torch.nn.Module, x: torch.Tensor) -> torch.Tensor:
        """SiluAndMul(apply(layer, x)): the deferred GEMM, its K-split slabs summed by the activation kernel. Same values as
        the two calls."""
        if not self._native(layer, x):
            y = super().apply(layer, x)
            act = torch.empty(y.shape[:-1] + (y.shape[-1] // 2, ), dtype=y.dtype, device=y.device)
            ops.silu_and_mul(act, y)
            return act
        k, n = layer.native_shape
        reshaped_x = x.reshape(-1, x.shape[-1]).contiguous()
        g = ops.w4a16_gemm_deferred(reshaped_x, layer.native_q, layer.native_s, reshaped_x.shape[0], n, k, zeros_native=layer.native_z)
        act = torch.empty((reshaped_x.shape[0], n // 2), dtype=x.dtype, device=x.device)
        ops.silu_and_mul_splitk(act, g)
        return act.reshape(x.shape[:-1] + (n // 2, ))
