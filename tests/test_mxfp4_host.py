"""CPU tests: mxfp4 is registered by name (gptq_native stays last), only the 32-value MX block is accepted, and a shard the
kernel does not take is refused when the weights are created."""
import pytest
import torch


def test_mxfp4_registry_and_refusals():
    from neuralmagic_vllm_amd.layers.quantization import QUANTIZATION_METHODS, get_quantization_config
    from neuralmagic_vllm_amd.layers.quantization.mxfp4 import MXFP4Config, MXFP4LinearMethod
    assert get_quantization_config("mxfp4") is MXFP4Config and list(QUANTIZATION_METHODS)[-1] == "gptq_native"
    cfg = MXFP4Config.from_config({"group_size": 32})
    assert cfg.get_name() == "mxfp4" and type(cfg.get_quant_method(None)) is MXFP4LinearMethod
    with pytest.raises(ValueError, match="32"):
        MXFP4Config.from_config({"group_size": 64})
    layer = torch.nn.Module()
    with pytest.raises(ValueError, match="K = 192"):
        cfg.get_quant_method(None).create_weights(layer, 192, [128], 192, 128, torch.float16)
    cfg.get_quant_method(None).create_weights(layer, 256, [64, 64], 256, 128, torch.bfloat16)
    assert layer.weight.shape == (128, 128) and layer.weight_scale.shape == (128, 8) and layer.weight.dtype == torch.uint8
