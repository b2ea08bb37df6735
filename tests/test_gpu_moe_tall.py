"""csrc/moe_tall.hip (ops.fused_moe(impl="tall")): the same bits as the rows path, within the rows path's bound of fp64,
under column slabs, token chunks, graph replay and auto dispatch."""
import pytest
import torch

from test_gpu_moe import generate, make_block, make_logits, ref_block

pytestmark = pytest.mark.gpu

# a: two runs of 300 rows = a full 256-row item + one of 44 rows (last block: 12 live), six empty experts
# b: every run shorter than an item and ragged; I = 96 (J = 1 k-grouping); hidden no multiple of 128
# c: one run of 1100 rows over five items and two align segments; three empty experts     d: one token
CASES = {"a": (300, 8, 2, 128, 64, "skewed"), "b": (150, 16, 4, 192, 96, "random"), "c": (1100, 4, 1, 128, 64, "skewed"),
         "d": (1, 8, 2, 128, 64, "random")}


@pytest.mark.parametrize("case", list(CASES))
def test_tall_equals_rows_and_matches_fp64(dev, case):
    from mini_sglang_amd import ops

    T, E, k, hidden, inter, pattern = CASES[case]
    cpu, (x, w1, w2, logits) = make_block(T, E, k, hidden, inter, pattern, dev)
    ref = ref_block(*cpu, k)
    buf = torch.full((T + 2, hidden), float("nan"), dtype=torch.bfloat16, device=dev)
    out = ops.fused_moe(x, w1, w2, logits, k, True, out=buf[:T], impl="tall")
    first = out.clone()
    err, bound = (out.cpu().double() - ref).abs().max().item(), 2.0 ** -7 * ref.abs().max().item()
    print(f"moe tall {case}: max err {err:.3e}, bound {bound:.3e}")
    assert torch.equal(first, ops.fused_moe(x, w1, w2, logits, k, True, impl="rows"))
    assert err <= bound, (err, bound)
    assert torch.isnan(buf[T:]).all()
    assert torch.equal(ops.fused_moe(x, w1, w2, logits, k, True, impl="tall"), first)


def test_column_slabs_and_token_chunks_change_no_bit(dev, monkeypatch):
    """Case (a)'s batch at hidden = 384 (at 128 one slab is all there is): a cap that leaves W = 256 gives slabs of 256 and
    128 columns; a cap that holds only half the tokens gives token chunks."""
    from mini_sglang_amd import ops

    T, E, k, hidden, inter = 300, 8, 2, 384, 64
    _, (x, w1, w2, logits) = make_block(T, E, k, hidden, inter, "skewed", dev)
    free = ops.fused_moe(x, w1, w2, logits, k, True, impl="tall")
    assert torch.equal(free, ops.fused_moe(x, w1, w2, logits, k, True, impl="rows"))
    two_slabs = ops.moe_workspace_bytes_tall(T, E, k, hidden, inter) + T * k * 4 * 128
    chunks = ops.moe_workspace_bytes_tall(T // 2, E, k, hidden, inter)
    assert chunks < ops.moe_workspace_bytes_tall(T, E, k, hidden, inter) < two_slabs
    for cap in (two_slabs, chunks):
        monkeypatch.setattr(ops, "MOE_WORKSPACE_MAX_BYTES", cap)
        assert torch.equal(ops.fused_moe(x, w1, w2, logits, k, True, impl="tall"), free), cap


def test_graph_replay_follows_the_routing(dev):
    from mini_sglang_amd import ops

    T, E, k, hidden, inter = 300, 8, 2, 128, 64
    _, (x, w1, w2, skewed) = make_block(T, E, k, hidden, inter, "skewed", dev)
    random = make_logits(T, E, "random").to(dev)
    eager = {"skewed": ops.fused_moe(x, w1, w2, skewed, k, True, impl="tall"),
             "random": ops.fused_moe(x, w1, w2, random, k, True, impl="tall")}
    assert not torch.equal(eager["random"], eager["skewed"])
    logits, out = random.clone(), torch.empty_like(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.fused_moe(x, w1, w2, logits, k, True, out=out, impl="tall")
    for name in ("skewed", "random", "skewed"):
        logits.copy_(skewed if name == "skewed" else random)
        graph.replay()
        assert torch.equal(out, eager[name]), name


def test_auto_dispatch(dev, monkeypatch):
    from mini_sglang_amd import ops
    from mini_sglang_amd.model import PRESETS

    T, E, k, hidden, inter, pattern = CASES["c"]
    assert T * k >= ops.MOE_TALL_MIN_PAIRS_PER_EXPERT * E
    _, (x, w1, w2, logits) = make_block(T, E, k, hidden, inter, pattern, dev)
    calls = []
    forward_tall = ops.lib().msgl_moe_forward_tall
    monkeypatch.setattr(ops.lib(), "msgl_moe_forward_tall", lambda *a: calls.append(1) or forward_tall(*a))
    assert torch.equal(ops.fused_moe(x, w1, w2, logits, k, True), ops.fused_moe(x, w1, w2, logits, k, True, impl="tall"))
    assert len(calls) == 2
    plain = generate(dev, PRESETS["tiny-moe"], [1], 4)
    assert len(calls) == 2  # 20 prompt tokens stay on the rows path
    monkeypatch.setattr(ops, "MOE_TALL_MIN_PAIRS_PER_EXPERT", 0)
    assert generate(dev, PRESETS["tiny-moe"], [1], 4) == plain and len(calls) > 2
