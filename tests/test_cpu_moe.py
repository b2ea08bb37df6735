"""Mixture-of-experts host side: presets, weight accounting and checkpoint loading (no GPU)."""
import dataclasses
import subprocess
import sys

import pytest
import torch

from mini_sglang_amd.model import PRESETS, DenseDecoder

CPU = torch.device("cpu")


def test_dense_presets_have_no_experts_and_moe_presets_do():
    for name, cfg in PRESETS.items():
        assert (cfg.num_experts > 0) == (name in ("qwen3-30b-a3b", "tiny-moe")), name
    big = PRESETS["qwen3-30b-a3b"]
    assert (big.num_layers, big.num_qo_heads, big.num_kv_heads, big.head_dim, big.hidden_size, big.vocab_size) == \
        (48, 32, 4, 128, 2048, 151936)
    assert (big.num_experts, big.num_experts_per_tok, big.moe_intermediate_size, big.norm_topk_prob) == (128, 8, 768, True)


def test_weight_bytes_counts_experts_and_router():
    dec = DenseDecoder(PRESETS["tiny-moe"], dtype=torch.bfloat16, device=CPU)
    H, D, V, E, I = 256, 128, 1024, 8, 96
    layer = 2 * H + (10 + 2 * 2) * D * H + 2 * D + H * 10 * D + E * H + E * 2 * I * H + E * H * I
    assert dec.weight_bytes() == 2 * (2 * V * H + H + 2 * layer)
    # Qwen3-30B-A3B's layer as rank 0 of tp = 8 sees it (E 128, I_l 96, hidden 2048; 4 q heads, 1 replicated kv head),
    # one layer and a 1024-row vocabulary so that it fits a test: 160 MB
    big = dataclasses.replace(PRESETS["qwen3-30b-a3b"], num_layers=1, vocab_size=1024)
    dec = DenseDecoder(big, dtype=torch.bfloat16, device=CPU, tp_size=8)
    H, D, E, I = 2048, 128, 128, 96
    layer = 2 * H + (4 + 2 * 1) * D * H + 2 * D + H * 4 * D + E * H + E * 2 * I * H + E * H * I
    assert dec.weight_bytes() == 2 * (2 * 128 * H + H + layer)
    assert dec.streamed_bytes_per_step(tokens=4) == 2 * (128 * H + H + layer - (E - 4 * 8) * 3 * I * H)


def test_install_registers_the_hip_moe_backend():
    import refdrive

    ref = refdrive.reference_root()
    if ref is None:
        pytest.skip("the reference's package is not present")
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import mini_sglang_amd.minisgl_plugin as p; p.install()\n"
            "from minisgl.moe import SUPPORTED_MOE_BACKENDS as S, BaseMoeBackend as B\n"
            "assert 'hip' in S.supported_names() and 'fused' in S.supported_names()\n"
            "assert isinstance(S['hip'](), B) and type(S['hip']()) is p.HipMoeBackend; print('moe backend ok')"
            % (str(ref), str(refdrive.ROOT)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "moe backend ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("rank", [0, 1])
def test_load_hf_state_stacks_and_shards_experts(rank):
    cfg = PRESETS["tiny-moe"]
    H, E, I, D = cfg.hidden_size, cfg.num_experts, cfg.moe_intermediate_size, cfg.head_dim
    g = torch.Generator().manual_seed(5)

    def t(*shape):
        return torch.randn(shape, generator=g).bfloat16()

    state = {"model.embed_tokens.weight": t(cfg.vocab_size, H), "lm_head.weight": t(cfg.vocab_size, H),
             "model.norm.weight": t(H)}
    for i in range(cfg.num_layers):
        p = f"model.layers.{i}."
        state.update({p + "input_layernorm.weight": t(H), p + "post_attention_layernorm.weight": t(H),
                      p + "self_attn.q_proj.weight": t(cfg.num_qo_heads * D, H),
                      p + "self_attn.k_proj.weight": t(cfg.num_kv_heads * D, H),
                      p + "self_attn.v_proj.weight": t(cfg.num_kv_heads * D, H),
                      p + "self_attn.q_norm.weight": t(D), p + "self_attn.k_norm.weight": t(D),
                      p + "self_attn.o_proj.weight": t(H, cfg.num_qo_heads * D), p + "mlp.gate.weight": t(E, H)})
        for e in range(E):
            q = p + f"mlp.experts.{e}."
            state.update({q + "gate_proj.weight": t(I, H), q + "up_proj.weight": t(I, H), q + "down_proj.weight": t(H, I)})
    dec = DenseDecoder(cfg, dtype=torch.bfloat16, device=CPU, tp_rank=rank, tp_size=2)
    dec.load_hf_state(state)
    h = I // 2
    for i, lw in enumerate(dec.layers):
        p = f"model.layers.{i}."
        assert lw.gate_up is None and lw.down is None
        assert torch.equal(lw.router, state[p + "mlp.gate.weight"])
        for e in range(E):
            q = p + f"mlp.experts.{e}."
            assert torch.equal(lw.w1[e, :h], state[q + "gate_proj.weight"][rank * h:(rank + 1) * h])
            assert torch.equal(lw.w1[e, h:], state[q + "up_proj.weight"][rank * h:(rank + 1) * h])
            assert torch.equal(lw.w2[e], state[q + "down_proj.weight"][:, rank * h:(rank + 1) * h])
