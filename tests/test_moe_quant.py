"""--quantize reaches the Mixtral expert weights (E16 / E18): every MoEBlock
stores packed experts and the engine still generates (CPU)."""

import pytest
import torch


@pytest.mark.parametrize(("method", "qbits", "dims"), [
    ("int8", 8, None),
    ("awq", 4, (128, 256)),  # int4 needs hidden / intermediate % 128 == 0
])
def test_engine_quantized_moe_generates(method, qbits, dims):
    from vllm_tgis_adapter_amd.engine import LLMEngine, SamplingParams
    from vllm_tgis_adapter_amd.engine.config import (
        CacheConfig, EngineConfig, ModelConfig, SchedulerConfig,
    )
    from vllm_tgis_adapter_amd.models.mixtral import MoEBlock

    mc = ModelConfig.from_model_arg("tiny-mixtral", dtype="bfloat16")
    if dims:
        mc.hidden_size, mc.intermediate_size = dims
    eng = LLMEngine(EngineConfig(
        model_config=mc, cache_config=CacheConfig(block_size=16),
        scheduler_config=SchedulerConfig(max_num_seqs=4,
                                         max_num_batched_tokens=512),
        device="cpu", quantization=method, seed=0,
    ))
    blocks = [m for m in eng.worker.model.modules() if isinstance(m, MoEBlock)]
    assert blocks
    for moe in blocks:
        assert moe.quant_bits == qbits
        assert not hasattr(moe, "w13") and not hasattr(moe, "w2")
        assert moe.w13_q.dtype == (torch.int8 if qbits == 8 else torch.uint8)
        assert moe.gate.dtype == torch.bfloat16
    eng.add_request("q", None, [5, 6, 7, 8],
                    SamplingParams(temperature=0.0, max_tokens=8))
    steps, final = 0, None
    while eng.has_unfinished() and steps < 40:
        for o in eng.step():
            if o.finished:
                final = o
        steps += 1
    assert final is not None and len(final.outputs[0].token_ids) == 8
