"""CPU test: gptq_native is registered, opt-in only, and leaves GPTQMarlinConfig's override behaviour alone."""


def test_gptq_native_registry_and_override():
    from neuralmagic_vllm_amd.layers.quantization import QUANTIZATION_METHODS, get_quantization_config
    from neuralmagic_vllm_amd.layers.quantization.gptq_marlin import GPTQMarlinConfig
    from neuralmagic_vllm_amd.layers.quantization.gptq_native import GPTQNativeConfig, GPTQNativeLinearMethod
    assert get_quantization_config("gptq_native") is GPTQNativeConfig and list(QUANTIZATION_METHODS)[-1] == "gptq_native"
    assert issubclass(GPTQNativeConfig, GPTQMarlinConfig) and GPTQNativeConfig.get_name() == "gptq_native"
    ok = {"bits": 4, "group_size": 128, "sym": True, "desc_act": False}
    for user in (None, "gptq_marlin", "marlin", "gptq", "awq"):
        assert GPTQNativeConfig.override_quantization_method(ok, user) is None
    assert GPTQNativeConfig.override_quantization_method(ok, "gptq_native") == "gptq_native"
    assert GPTQNativeConfig.override_quantization_method({**ok, "sym": False}, "gptq_native") is None
    assert GPTQMarlinConfig.override_quantization_method(ok, None) == "gptq_marlin"
    assert GPTQMarlinConfig.override_quantization_method(ok, "gptq_marlin") == "gptq_marlin"
    assert GPTQMarlinConfig.override_quantization_method(ok, "gptq_native") is None
    cfg = GPTQNativeConfig.from_config({"bits": 4, "group_size": 128, "desc_act": False, "sym": True})
    assert isinstance(cfg.get_quant_method(None), GPTQNativeLinearMethod) and "GPTQNativeConfig" in repr(cfg)
