"""Block-scaled FP8 weights, host side: the load-time quantiser against its formula, the byte count and the checkpoint
loader of a `weight_quant="fp8_block128"` model, and the two configurations it refuses."""
import pytest
import torch

import refdrive
from mini_sglang_amd import ops
from mini_sglang_amd.model import PRESETS, DenseDecoder

B = 128
CPU = torch.device("cpu")


def _expand(s):
    return s.repeat_interleave(B, 0).repeat_interleave(B, 1)


def test_quantizer_matches_its_formula():
    g = torch.Generator().manual_seed(3)
    mag = 2.0 ** torch.tensor([[0, 3, -3], [-3, 0, 3]])  # neighbouring blocks differ by 2^+-3
    w = (torch.randn((256, 384), generator=g) * _expand(mag)).to(torch.bfloat16)
    h = ops.quantize_fp8_block128(w)
    assert h.shape == w.shape and h.q.dtype == torch.float8_e4m3fn and h.scales.shape == (2, 3)
    s = w.float().view(2, B, 3, B).abs().amax(dim=(1, 3)).clamp_min(torch.finfo(torch.float32).tiny) / 448
    q = (w.float() / _expand(s)).to(torch.float8_e4m3fn)
    assert torch.equal(h.scales, s) and torch.equal(h.q.view(torch.uint8), q.view(torch.uint8))
    # e4m3 keeps 3 mantissa bits: half a step is 2^-4 of the value's binade, at most 2^-4 * 448 s = 28 s per block
    # (and half the smallest subnormal step, 2^-10 s, near zero)
    err = (h.dequantize() - w.float()).abs()
    assert bool((err <= torch.maximum(w.float().abs() * 2.0 ** -4, _expand(s) * 2.0 ** -10)).all())


def _tiny(**kw):
    return DenseDecoder(PRESETS["tiny"], dtype=torch.bfloat16, device=CPU, weight_quant="fp8_block128", **kw)


def test_weight_bytes_is_the_hand_count():
    cfg, dec = PRESETS["tiny"], _tiny()
    H, qd, kvd, I = cfg.hidden_size, cfg.num_qo_heads * 128, cfg.num_kv_heads * 128, cfg.intermediate_size
    proj = (qd + 2 * kvd) * H + H * qd + 2 * I * H + H * I  # one byte each, plus 4 bytes per 128 x 128 block
    norms = 2 * H + 2 * 128
    want = 2 * (2 * cfg.vocab_size * H + H) + cfg.num_layers * (proj + 4 * proj // (B * B) + 2 * norms)
    assert dec.weight_bytes() == want
    assert dec.streamed_bytes_per_step() == want - 2 * cfg.vocab_size * H
    assert isinstance(dec.layers[0].qkv, ops.Fp8Weight) and dec.lm_head.dtype == torch.bfloat16 and not dec.gate_up_ilv


def test_load_hf_state_takes_fp8_entries_and_merges_their_scale_grids():
    state = refdrive.seeded_hf_state("tiny", seed=5)
    want = {}
    for k in [k for k in state if k.endswith("_proj.weight")]:
        h = ops.quantize_fp8_block128(state[k] * (3.0 if "k_proj" in k or "up_proj" in k else 1.0))
        state[k], state[k + "_scale_inv"] = h.q, h.scales
        want[k] = h
    dec = _tiny(seed=1)
    dec.load_hf_state(state)
    for i, lw in enumerate(dec.layers):
        p = f"model.layers.{i}."
        for got, names in ((lw.qkv, ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"]), (lw.o, ["self_attn.o_proj"]),
                           (lw.gate_up, ["mlp.gate_proj", "mlp.up_proj"]), (lw.down, ["mlp.down_proj"])):
            hs = [want[p + n + ".weight"] for n in names]
            assert torch.equal(got.q.view(torch.uint8), torch.cat([h.q.view(torch.uint8) for h in hs]))
            assert torch.equal(got.scales, torch.cat([h.scales for h in hs]))


def test_refuses_unaligned_tp_shards_and_moe():
    with pytest.raises(ValueError, match="multiples of"):  # intermediate 512 / 8 ranks = 64 rows per shard
        DenseDecoder(PRESETS["tiny-llama"], dtype=torch.bfloat16, device=CPU, weight_quant="fp8_block128", tp_size=8)
    with pytest.raises(ValueError, match="dense"):
        DenseDecoder(PRESETS["tiny-moe"], dtype=torch.bfloat16, device=CPU, weight_quant="fp8_block128")
