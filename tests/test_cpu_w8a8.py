"""weight_quant="fp8_block128_a8", host side: the option builds on the CPU, marks the four dense projections for
activation quantisation and nothing else, and is refused on an expert model; unknown values are still refused."""
import pytest
import torch

from mini_sglang_amd import ops
from mini_sglang_amd.model import PRESETS, DenseDecoder

CPU = torch.device("cpu")


def test_a8_option_marks_the_four_dense_projections_only():
    dec = DenseDecoder(PRESETS["tiny"], dtype=torch.bfloat16, device=CPU, weight_quant="fp8_block128_a8")
    w16 = DenseDecoder(PRESETS["tiny"], dtype=torch.bfloat16, device=CPU, weight_quant="fp8_block128")
    for lw, lw16 in zip(dec.layers, w16.layers):
        for k in ("qkv", "o", "gate_up", "down"):
            got, old = getattr(lw, k), getattr(lw16, k)
            assert isinstance(got, ops.Fp8Weight) and got.act_quant == "fp8_group128" and old.act_quant is None
            assert torch.equal(got.q.view(torch.uint8), old.q.view(torch.uint8)) and torch.equal(got.scales, old.scales)
    assert not isinstance(dec.lm_head, ops.Fp8Weight) and not isinstance(dec.embed, ops.Fp8Weight)
    assert dec.weight_bytes() == w16.weight_bytes()


def test_a8_option_is_refused_on_expert_models_and_unknown_values_still_are():
    with pytest.raises(ValueError, match="dense models only"):
        DenseDecoder(PRESETS["tiny-moe"], dtype=torch.bfloat16, device=CPU, weight_quant="fp8_block128_a8")
    with pytest.raises(ValueError, match="weight_quant"):
        DenseDecoder(PRESETS["tiny"], dtype=torch.bfloat16, device=CPU, weight_quant="fp8_block128_a4")
    with pytest.raises(ValueError, match="act_quant"):
        ops.Fp8Weight(torch.zeros((128, 128)).to(torch.float8_e4m3fn), torch.ones((1, 1)), act_quant="int8")
