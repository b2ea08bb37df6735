"""csrc/moe_w8.hip (block-scaled FP8 expert weights) against the fp64 statement of FusedMoe.forward on the dequantised
weights, under graph replay, through the tall route, at its refusals, and inside the 128-wide tiny-moe model."""
import dataclasses

import pytest
import torch

from test_gpu_moe import _OtherRanksAddZeros, generate, make_logits, ref_block, torch_moe

pytestmark = pytest.mark.gpu

BLOCK_CASES = [(1, 8, 2, 128, 128), (5, 8, 2, 256, 128), (33, 16, 4, 384, 256), (70, 8, 2, 128, 128), (17, 128, 8, 256, 128)]


def quantized(shape, g, dev):
    """quantize_fp8_block128 of N(0, 1/K) weights whose block (e, bi, bj) is multiplied by 2^(3 ((e + bi + bj) % 3 - 1)):
    neighbouring blocks, the gate and up row groups and neighbouring experts carry different scales."""
    from mini_sglang_amd import ops

    E, N, K = shape
    e, bi, bj = torch.meshgrid(torch.arange(E), torch.arange(N // 128), torch.arange(K // 128), indexing="ij")
    mag = (2.0 ** (3 * ((e + bi + bj) % 3 - 1))).repeat_interleave(128, 1).repeat_interleave(128, 2)
    h = ops.quantize_fp8_block128((torch.randn(shape, generator=g) / K ** 0.5 * mag).bfloat16())
    return h, ops.Fp8Weight(h.q.to(dev), h.scales.to(dev))


def make_block(T, E, k, hidden, inter, pattern, dev):
    g = torch.Generator().manual_seed(T * 1000 + E)
    x, logits = torch.randn((T, hidden), generator=g).bfloat16(), make_logits(T, E, pattern)
    (c1, w1), (c2, w2) = quantized((E, 2 * inter, hidden), g, dev), quantized((E, hidden, inter), g, dev)
    return (x, c1.dequantize(), c2.dequantize(), logits), (x.to(dev), w1, w2, logits.to(dev))


@pytest.mark.parametrize("pattern", ["random", "skewed"])
@pytest.mark.parametrize("T,E,k,hidden,inter", BLOCK_CASES)
def test_block_matches_fp64(dev, monkeypatch, T, E, k, hidden, inter, pattern):
    from mini_sglang_amd import ops

    cpu, (x, w1, w2, logits) = make_block(T, E, k, hidden, inter, pattern, dev)
    ref = ref_block(*cpu, k)
    buf = torch.full((T + 2, hidden), float("nan"), dtype=torch.bfloat16, device=dev)
    out = ops.fused_moe(x, w1, w2, logits, k, True, out=buf[:T], impl="rows")
    first = out.clone()
    err, bound = (out.cpu().double() - ref).abs().max().item(), 2.0 ** -7 * ref.abs().max().item()
    print(f"moe w8 block {(T, E, k, hidden, inter)} {pattern}: max err {err:.3e}, bound {bound:.3e}")
    assert torch.isfinite(out).all()
    assert err <= bound, (err, bound)
    assert torch.isnan(buf[T:]).all()
    assert torch.equal(ops.fused_moe(x, w1, w2, logits, k, True), first)  # impl None: below the tall threshold
    if T == 33:  # a token's row does not depend on the rest of the batch
        for t in (0, 15, 16, 32):
            assert torch.equal(ops.fused_moe(x[t:t + 1], w1, w2, logits[t:t + 1], k, True)[0], first[t])
    if T == 70:  # token chunks change no bit
        monkeypatch.setattr(ops, "MOE_MAX_CHUNK_TOKENS", 32)
        assert torch.equal(ops.fused_moe(x, w1, w2, logits, k, True, impl="rows"), first)


def test_graph_replay_follows_the_routing(dev):
    from mini_sglang_amd import ops

    T, E, k, hidden, inter = 33, 16, 4, 384, 256
    _, (x, w1, w2, random) = make_block(T, E, k, hidden, inter, "random", dev)
    skewed = make_logits(T, E, "skewed").to(dev)
    eager = {name: ops.fused_moe(x, w1, w2, lg, k, True) for name, lg in (("random", random), ("skewed", skewed))}
    assert not torch.equal(eager["random"], eager["skewed"])
    logits, out = random.clone(), torch.empty_like(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.fused_moe(x, w1, w2, logits, k, True, out=out)
    for name in ("skewed", "random", "skewed"):
        logits.copy_(skewed if name == "skewed" else random)
        graph.replay()
        assert torch.equal(out, eager[name]), name


def test_tall_route_equals_the_bf16_tall_kernel_on_the_dequantised_weights(dev):
    from mini_sglang_amd import ops

    T, E, k, hidden, inter = 300, 4, 2, 128, 128
    cpu, (x, w1, w2, logits) = make_block(T, E, k, hidden, inter, "random", dev)
    want = ops.fused_moe(x, cpu[1].bfloat16().to(dev), cpu[2].bfloat16().to(dev), logits, k, True, impl="tall")
    assert torch.equal(ops.fused_moe(x, w1, w2, logits, k, True, impl="tall"), want)


@pytest.mark.parametrize("case", ["inter 96", "hidden 192", "null scale", "misaligned q1"])
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
    out = torch.full((T, hidden), 7.0, dtype=torch.bfloat16, device=dev)
    rc = lib().msgl_moe_w8_forward(x.data_ptr(), q1.data_ptr() + (8 if case == "misaligned q1" else 0), s.data_ptr(),
                                   q2.data_ptr(), None if case == "null scale" else s.data_ptr(), tw.data_ptr(),
                                   ids.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), T, E, k, hidden, inter, None)
    torch.cuda.synchronize()
    assert rc == -1 and lib().msgl_last_error()
    assert bool((out == 7.0).all())


def _w8_model(tp_size=1):
    from mini_sglang_amd.model import PRESETS

    return dataclasses.replace(PRESETS["tiny-moe"], moe_intermediate_size=128 * tp_size)


def test_tiny_moe_fp8_model_within_twice_the_fp32_floor(dev, monkeypatch):
    """The forced-token protocol of test_gpu_moe: logits with the HIP FP8 expert MLP against the fp32 torch statement on
    the dequantised experts, bounded by twice that statement's own distance from fp64."""
    from mini_sglang_amd import ops

    lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(dev)  # every e4m3 value, exact

    def deq(w):  # Fp8Weight.dequantize() with device operations only, so that it captures
        return lut[w.q.view(torch.uint8).long()] * w.scales.repeat_interleave(128, -2).repeat_interleave(128, -1)

    def on_dequantised(dtype):
        fn = torch_moe(dtype)
        return lambda x, w1, w2, *a, **kw: fn(x, deq(w1), deq(w2), *a, **kw)

    def logits_of(moe_fn):
        rec = []

        def sample(logits, args):  # forced tokens: the three runs see the same inputs whatever their logits
            rec.append(logits.float().cpu())
            return torch.full((logits.shape[0],), 11 * len(rec), dtype=torch.int32, device=logits.device)

        if moe_fn is not None:
            monkeypatch.setattr(ops, "fused_moe", moe_fn)
        generate(dev, _w8_model(), [1], 4, sample, weight_quant="fp8_block128")
        monkeypatch.undo()
        assert len(rec) == 4
        return torch.cat(rec)

    hip, f32, f64 = logits_of(None), logits_of(on_dequantised(torch.float32)), logits_of(on_dequantised(torch.float64))
    dev_hip, floor = (hip - f32).abs().max().item(), (f32 - f64).abs().max().item()
    msg = f"hip vs fp32 {dev_hip:.3e}, fp32 vs fp64 {floor:.3e}, max |logit| {f64.abs().max().item():.3e}"
    print("tiny-moe fp8 logits:", msg)
    assert dev_hip <= 2 * floor, msg


def test_tiny_moe_fp8_tp2_shard_graph_replay_equals_eager(dev):
    outs = [generate(dev, _w8_model(2), bs, 5, tp_size=2, comm=_OtherRanksAddZeros(), weight_quant="fp8_block128")
            for bs in ([1], [])]
    assert outs[0] == outs[1] and len(outs[0][0]) == 5
