"""CPU tests: the MXFP4 mixture-of-experts method is reached through the existing mxfp4 config (no new quantization name:
gptq_native stays last) and refuses experts the grouped kernel does not take when the weights are created."""
import pytest
import torch


def test_mxfp4_moe_method_refuses_and_registers():
    from neuralmagic_vllm_amd.layers.quantization import QUANTIZATION_METHODS, get_quantization_config
    from neuralmagic_vllm_amd.layers.quantization.mxfp4 import MXFP4MoEMethod
    assert list(QUANTIZATION_METHODS)[-1] == "gptq_native"
    method = MXFP4MoEMethod(get_quantization_config("mxfp4").from_config({}))
    with pytest.raises(ValueError, match="intermediate_size = 192"):
        method.create_weights(torch.nn.Module(), 8, 512, 192, torch.float16)
    layer = torch.nn.Module()
    method.create_weights(layer, 4, 256, 128, torch.bfloat16)
    assert layer.w13_weight.shape == (4, 256, 128) and layer.w13_weight_scale.shape == (4, 256, 8)
    assert layer.w2_weight.shape == (4, 256, 64) and layer.w2_weight_scale.shape == (4, 256, 4) and layer.w2_weight.dtype == torch.uint8
