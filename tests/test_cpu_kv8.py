"""Host side of kv_quant="fp8_e4m3": page pricing, the configuration refusals, and the byte-copy store refusing an FP8 pool."""
import dataclasses

import pytest
import torch

from mini_sglang_amd.engine import EngineConfig, determine_num_pages
from mini_sglang_amd.kvcache import MHAKVCache
from mini_sglang_amd.model import PRESETS


def test_fp8_pages_cost_half():
    cfg = EngineConfig(model=PRESETS["qwen3-14b"], page_size=16, memory_ratio=1.0)
    per_page = 2 * 128 * 8 * 16 * 40  # k|v x head_dim x kv heads x page x layers, at 1 B per element
    budget = per_page * 1000 + (30 << 30)  # free before the model loaded; the model took 30 GiB
    assert determine_num_pages(budget, budget - (30 << 30), cfg) == 500
    assert determine_num_pages(budget, budget - (30 << 30), dataclasses.replace(cfg, kv_quant="fp8_e4m3")) == 1000


@pytest.mark.parametrize("bad", [dict(kv_quant="int8"), dict(model=PRESETS["tiny-d64"]), dict(dtype=torch.float16),
                                 dict(fused_qkv_path=False)], ids=lambda b: next(iter(b)))
def test_config_refuses_what_the_fp8_cache_cannot_serve(bad):
    kw = dict(dict(model=PRESETS["tiny"], kv_quant="fp8_e4m3"), **bad)
    with pytest.raises(ValueError):
        EngineConfig(**kw)
    EngineConfig(**dict(kw, kv_quant=None))  # the same configuration without the option stands


def test_byte_copy_store_refuses_an_fp8_pool():
    pool = MHAKVCache(2, 1, 128, 4, 4, torch.float8_e4m3fn, torch.device("cpu"), k_scale=0.5)
    assert (pool.k_scale, pool.v_scale, pool.dtype) == (0.5, 1.0, torch.float8_e4m3fn)
    kv = torch.zeros((3, 2, 128), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="qk_norm_rope_store"):
        pool.store_kv(kv, kv, torch.arange(3, dtype=torch.int32), 0)
