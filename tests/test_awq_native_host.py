"""CPU test: awq_native is registered by name, gptq_native stays last, and plain awq is what it was."""


def test_awq_native_registry():
    from neuralmagic_vllm_amd.layers.quantization import QUANTIZATION_METHODS, get_quantization_config
    from neuralmagic_vllm_amd.layers.quantization.awq import AWQConfig, AWQLinearMethod
    from neuralmagic_vllm_amd.layers.quantization.awq_native import AWQNativeConfig, AWQNativeLinearMethod
    assert get_quantization_config("awq_native") is AWQNativeConfig and list(QUANTIZATION_METHODS)[-1] == "gptq_native"
    hf = {"w_bit": 4, "q_group_size": 128, "zero_point": True}
    cfg = AWQNativeConfig.from_config(hf)
    assert cfg.get_name() == "awq_native" and type(cfg.get_quant_method(None)) is AWQNativeLinearMethod and "AWQNativeConfig" in repr(cfg)
    assert get_quantization_config("awq") is AWQConfig
    plain = AWQConfig.from_config(hf)
    assert plain.get_name() == "awq" and type(plain.get_quant_method(None)) is AWQLinearMethod
