"""Host side of FP8 expert weights (no GPU): expert-stacked Fp8Weight, the model's byte counts and the checkpoint loader."""
import dataclasses

import pytest
import torch

import refdrive
from mini_sglang_amd import ops
from mini_sglang_amd.model import PRESETS, DenseDecoder

B = 128
CPU = torch.device("cpu")


def _decoder(tp_size=1, tp_rank=0, seed=42):
    cfg = dataclasses.replace(PRESETS["tiny-moe"], moe_intermediate_size=B * tp_size)
    return cfg, DenseDecoder(cfg, dtype=torch.bfloat16, device=CPU, weight_quant="fp8_block128", tp_size=tp_size,
                             tp_rank=tp_rank, seed=seed)


def test_stacked_quantizer_is_the_2d_one_per_expert():
    w = (torch.randn((3, 256, 128), generator=torch.Generator().manual_seed(1)) * 2.0 ** torch.arange(3)[:, None, None]).bfloat16()
    h = ops.quantize_fp8_block128(w)
    assert h.shape == w.shape and h.scales.shape == (3, 2, 1) and h.nbytes() == w.numel() + 4 * 6
    for e in range(3):
        one = ops.quantize_fp8_block128(w[e])
        assert torch.equal(h.q[e].view(torch.uint8), one.q.view(torch.uint8)) and torch.equal(h.scales[e], one.scales)
        assert torch.equal(h.dequantize()[e], one.dequantize())
    with pytest.raises(ValueError):
        ops.Fp8Weight(h.q, h.scales[0])


def test_constructor_and_byte_counts_are_the_hand_count():
    cfg, dec = _decoder()
    H, E, k, I = cfg.hidden_size, cfg.num_experts, cfg.num_experts_per_tok, cfg.moe_intermediate_size
    lw = dec.layers[0]
    assert isinstance(lw.w1, ops.Fp8Weight) and lw.w1.shape == (E, 2 * I, H) and lw.w1.scales.shape == (E, 2, 2)
    assert isinstance(lw.w2, ops.Fp8Weight) and lw.w2.shape == (E, H, I) and lw.w2.scales.shape == (E, 2, 1)
    assert isinstance(lw.qkv, ops.Fp8Weight) and lw.router.dtype == torch.bfloat16
    qd, kvd = cfg.num_qo_heads * 128, cfg.num_kv_heads * 128
    attn, expert = (qd + 2 * kvd) * H + H * qd, 3 * I * H  # one byte each, plus 4 bytes per 128 x 128 block
    w8 = attn + 4 * attn // (B * B) + E * (expert + 4 * expert // (B * B))
    want = 2 * (2 * cfg.vocab_size * H + H) + cfg.num_layers * (w8 + 2 * (E * H + 2 * H + 2 * 128))
    assert dec.weight_bytes() == want
    assert dec.streamed_bytes_per_step() == want - 2 * cfg.vocab_size * H
    idle = E - 3 * k  # three tokens touch at most six of the eight experts
    assert dec.streamed_bytes_per_step(tokens=3) == want - 2 * cfg.vocab_size * H - cfg.num_layers * idle * (expert + 4 * 6)


@pytest.mark.parametrize("rank", [0, 1])
def test_load_hf_state_shards_and_stacks_fp8_experts(rank):
    cfg, dec = _decoder(tp_size=2, tp_rank=rank, seed=1)
    E, I = cfg.num_experts, cfg.moe_intermediate_size  # 256: two 128-row shards
    state = refdrive.seeded_hf_state("tiny", seed=5)
    g = torch.Generator().manual_seed(6)
    want = {}
    for i in range(cfg.num_layers):
        p = f"model.layers.{i}."
        state[p + "mlp.gate.weight"] = torch.randn((E, cfg.hidden_size), generator=g).bfloat16()
        for k in [p + f"self_attn.{n}_proj.weight" for n in "qkvo"]:
            h = ops.quantize_fp8_block128(state[k])
            state[k], state[k + "_scale_inv"] = h.q, h.scales
        for e in range(E):
            for name, shape in (("gate", (I, cfg.hidden_size)), ("up", (I, cfg.hidden_size)), ("down", (cfg.hidden_size, I))):
                k = p + f"mlp.experts.{e}.{name}_proj.weight"
                h = ops.quantize_fp8_block128((torch.randn(shape, generator=g) * 0.02 * (e + 1)).bfloat16())
                state[k], state[k + "_scale_inv"], want[k] = h.q, h.scales, h
    ptrs = [dec.layers[0].w1.q.data_ptr(), dec.layers[0].w2.scales.data_ptr()]
    dec.load_hf_state(state)
    assert ptrs == [dec.layers[0].w1.q.data_ptr(), dec.layers[0].w2.scales.data_ptr()]  # written in place
    rows = slice(rank * B, (rank + 1) * B)
    for i, lw in enumerate(dec.layers):
        assert torch.equal(lw.router, state[f"model.layers.{i}.mlp.gate.weight"])
        for e in range(E):
            gate, up, down = (want[f"model.layers.{i}.mlp.experts.{e}.{n}_proj.weight"] for n in ("gate", "up", "down"))
            assert torch.equal(lw.w1.q[e].view(torch.uint8), torch.cat([gate.q[rows], up.q[rows]]).view(torch.uint8))
            assert torch.equal(lw.w1.scales[e], torch.cat([gate.scales[rank:rank + 1], up.scales[rank:rank + 1]]))
            assert torch.equal(lw.w2.q[e].view(torch.uint8), down.q[:, rows].view(torch.uint8))
            assert torch.equal(lw.w2.scales[e], down.scales[:, rank:rank + 1])
