"""csrc/moe_w8_tall.hip (ops.fused_moe(impl="tall_w8") on Fp8Weight stacks): the same bits as the FP8 rows path, within
its bound of fp64 on the dequantised weights, under column slabs, token chunks, graph replay, auto dispatch and refusals."""
import dataclasses

import pytest
import torch

from test_gpu_moe import generate, make_logits, ref_block
from test_gpu_moe_w8 import make_block

pytestmark = pytest.mark.gpu

# a: two runs of 300 rows = a full 256-row item + one of 44 rows (last block: 12 live), six empty experts, one k block
# b: ragged runs shorter than an item; three k blocks through the two-stage ring; three column tiles in down
# c: one run of 1100 rows over five items and two align segments; gate and up in different scale row groups; two k blocks
#    in down                                                                                 d: one token
CASES = {"a": (300, 8, 2, 128, 128, "skewed"), "b": (150, 16, 4, 384, 128, "random"), "c": (1100, 4, 1, 128, 256, "skewed"),
         "d": (1, 8, 2, 128, 128, "random")}


@pytest.mark.parametrize("case", list(CASES))
def test_tall_w8_equals_rows_and_matches_fp64(dev, case):
    from mini_sglang_amd import ops

    T, E, k, hidden, inter, pattern = CASES[case]
    cpu, (x, w1, w2, logits) = make_block(T, E, k, hidden, inter, pattern, dev)
    ref = ref_block(*cpu, k)
    buf = torch.full((T + 2, hidden), float("nan"), dtype=torch.bfloat16, device=dev)
    out = ops.fused_moe(x, w1, w2, logits, k, True, out=buf[:T], impl="tall_w8")
    err, bound = (out.cpu().double() - ref).abs().max().item(), 2.0 ** -7 * ref.abs().max().item()
    print(f"moe w8 tall {case}: max err {err:.3e}, bound {bound:.3e}")
    assert torch.equal(out, ops.fused_moe(x, w1, w2, logits, k, True, impl="rows"))
    assert err <= bound, (err, bound)
    assert torch.isnan(buf[T:]).all()


def test_column_slabs_and_token_chunks_change_no_bit(dev, monkeypatch):
    """Case (a)'s batch at hidden = 384: a cap that leaves W = 256 gives slabs of 256 and 128 columns; a cap that holds only
    half the tokens gives token chunks."""
    from mini_sglang_amd import ops

    T, E, k, hidden, inter = 300, 8, 2, 384, 128
    _, (x, w1, w2, logits) = make_block(T, E, k, hidden, inter, "skewed", dev)
    free = ops.fused_moe(x, w1, w2, logits, k, True, impl="tall_w8")
    assert torch.equal(free, ops.fused_moe(x, w1, w2, logits, k, True, impl="rows"))
    two_slabs = ops.moe_workspace_bytes_tall(T, E, k, hidden, inter) + T * k * 4 * 128
    chunks = ops.moe_workspace_bytes_tall(T // 2, E, k, hidden, inter)
    assert chunks < ops.moe_workspace_bytes_tall(T, E, k, hidden, inter) < two_slabs
    for cap in (two_slabs, chunks):
        monkeypatch.setattr(ops, "MOE_WORKSPACE_MAX_BYTES", cap)
        assert torch.equal(ops.fused_moe(x, w1, w2, logits, k, True, impl="tall_w8"), free), cap


def test_graph_replay_follows_the_routing(dev):
    from mini_sglang_amd import ops

    T, E, k, hidden, inter = 300, 8, 2, 128, 128
    _, (x, w1, w2, skewed) = make_block(T, E, k, hidden, inter, "skewed", dev)
    random = make_logits(T, E, "random").to(dev)
    eager = {"skewed": ops.fused_moe(x, w1, w2, skewed, k, True, impl="tall_w8"),
             "random": ops.fused_moe(x, w1, w2, random, k, True, impl="tall_w8")}
    assert not torch.equal(eager["random"], eager["skewed"])
    logits, out = random.clone(), torch.empty_like(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.fused_moe(x, w1, w2, logits, k, True, out=out, impl="tall_w8")
    for name in ("skewed", "random", "skewed"):
        logits.copy_(skewed if name == "skewed" else random)
        graph.replay()
        assert torch.equal(out, eager[name]), name


def test_auto_dispatch(dev, monkeypatch):
    from mini_sglang_amd import ops
    from mini_sglang_amd.model import PRESETS

    T, E, k, hidden, inter, pattern = CASES["a"]
    cpu, (x, w1, w2, logits) = make_block(T, E, k, hidden, inter, pattern, dev)
    with pytest.raises(AssertionError, match="tall_w8"):
        ops.fused_moe(x, cpu[1].bfloat16().to(dev), cpu[2].bfloat16().to(dev), logits, k, True, impl="tall_w8")
    model = dataclasses.replace(PRESETS["tiny-moe"], moe_intermediate_size=128)
    shipped = generate(dev, model, [1], 4, weight_quant="fp8_block128")
    calls = []
    forward_tall = ops.lib().msgl_moe_w8_forward_tall
    monkeypatch.setattr(ops.lib(), "msgl_moe_w8_forward_tall", lambda *a: calls.append(1) or forward_tall(*a))
    monkeypatch.setattr(ops, "MOE_W8_TALL_MIN_PAIRS_PER_EXPERT", 0)
    assert torch.equal(ops.fused_moe(x, w1, w2, logits, k, True), ops.fused_moe(x, w1, w2, logits, k, True, impl="rows"))
    assert len(calls) == 1
    assert generate(dev, model, [1], 4, weight_quant="fp8_block128") == shipped and len(calls) > 1


@pytest.mark.parametrize("case", ["hidden 192", "inter 96", "null scale", "misaligned q1", "workspace one byte short"])
def test_refusals_launch_nothing(dev, case):
    from mini_sglang_amd._lib import lib

    T, E, k = 4, 4, 2
    hidden, inter = (192 if case == "hidden 192" else 128), (96 if case == "inter 96" else 128)
    x = torch.ones((T, hidden), dtype=torch.bfloat16, device=dev)
    q1 = torch.zeros(E * 2 * inter * hidden + 16, dtype=torch.uint8, device=dev)
    q2 = torch.zeros(E * hidden * inter, dtype=torch.uint8, device=dev)
    s = torch.ones(E * 8, dtype=torch.float32, device=dev)
    tw = torch.full((T, k), 0.5, dtype=torch.float32, device=dev)
    ids = torch.zeros((T, k), dtype=torch.int32, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    least = lib().msgl_moe_workspace_bytes_tall(T, E, k, 128, 128)
    assert 0 < least <= ws.numel()
    out = torch.full((T, hidden), 7.0, dtype=torch.bfloat16, device=dev)
    rc = lib().msgl_moe_w8_forward_tall(x.data_ptr(), q1.data_ptr() + (8 if case == "misaligned q1" else 0), s.data_ptr(),
                                        q2.data_ptr(), None if case == "null scale" else s.data_ptr(), tw.data_ptr(),
                                        ids.data_ptr(), ws.data_ptr(), least - 1 if case.startswith("workspace") else least,
                                        out.data_ptr(), T, E, k, hidden, inter, None)
    torch.cuda.synchronize()
    assert rc == -1 and lib().msgl_last_error()
    assert bool((out == 7.0).all())
