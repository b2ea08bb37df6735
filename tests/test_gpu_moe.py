"""csrc/moe.hip against a plain fp64 statement of FusedMoe.forward (routing, expert MLP, slot-ordered sum), under graph
replay, and inside the tiny-moe model."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK_CASES = [(1, 8, 2, 128, 64), (5, 8, 2, 128, 96), (33, 16, 4, 256, 96), (17, 128, 8, 256, 192), (3, 128, 8, 128, 64)]


def make_logits(T, E, pattern, seed=0):
    """Rows of distinct values that are exact in bf16; "skewed": every token has the same row (the same k experts)."""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randperm(E, generator=g) * 0.125 - 8 for _ in range(T)]
    return torch.stack(rows if pattern == "random" else rows[:1] * T).bfloat16()


def ref_route(logits, k, renormalize, dtype=torch.float64):
    p = torch.softmax(logits.to(dtype), dim=-1)
    ids = torch.argsort(p, dim=-1, descending=True, stable=True)[:, :k]  # stable: the lowest index wins a tie
    w = p.gather(1, ids)
    return (w / (w.sum(-1, keepdim=True) + 1e-8) if renormalize else w), ids


def ref_block(x, w1, w2, logits, k, renormalize=True):
    w, ids = ref_route(logits, k, renormalize)
    x, w1, w2, inter = x.double(), w1.double(), w2.double(), w2.shape[2]
    out = torch.zeros_like(x)
    for t in range(x.shape[0]):
        for s in range(k):
            e = int(ids[t, s])
            h = torch.nn.functional.silu(x[t] @ w1[e, :inter].T) * (x[t] @ w1[e, inter:].T)
            out[t] += w[t, s] * (h @ w2[e].T)
    return out


def make_block(T, E, k, hidden, inter, pattern, dev):
    g = torch.Generator().manual_seed(T * 1000 + E)
    x = torch.randn((T, hidden), generator=g).bfloat16()
    w1 = (torch.randn((E, 2 * inter, hidden), generator=g) / hidden ** 0.5).bfloat16()
    w2 = (torch.randn((E, hidden, inter), generator=g) / inter ** 0.5).bfloat16()
    logits = make_logits(T, E, pattern)
    return (x, w1, w2, logits), tuple(t.to(dev) for t in (x, w1, w2, logits))


@pytest.mark.parametrize("T,E,k,renormalize", [(1, 8, 1, True), (5, 8, 2, False), (33, 128, 8, True), (7, 256, 8, True)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_route_matches_fp64_softmax_topk(dev, T, E, k, renormalize, dtype):
    from mini_sglang_amd import ops

    logits = torch.cat([make_logits(T, E, "random"), torch.full((1, E), 1.5).bfloat16()])  # last row: all equal
    w, ids = ops.moe_route(logits.to(dev, dtype), k, renormalize)
    rw, rids = ref_route(logits, k, renormalize)
    assert w.dtype == torch.float32 and ids.dtype == torch.int32
    assert torch.equal(ids.cpu().long(), rids)
    assert (w.cpu().double() - rw).abs().max().item() <= 1e-6
    assert ids[T].tolist() == list(range(k))
    if renormalize:
        assert (w[T].cpu() - 1.0 / k).abs().max().item() <= 1e-6


@pytest.mark.parametrize("pattern", ["random", "skewed"])
@pytest.mark.parametrize("T,E,k,hidden,inter", BLOCK_CASES)
def test_block_matches_fp64(dev, T, E, k, hidden, inter, pattern):
    from mini_sglang_amd import ops

    cpu, (x, w1, w2, logits) = make_block(T, E, k, hidden, inter, pattern, dev)
    ref = ref_block(*cpu, k)
    buf = torch.full((T + 2, hidden), float("nan"), dtype=torch.bfloat16, device=dev)
    out = ops.fused_moe(x, w1, w2, logits, k, True, out=buf[:T])
    first = out.clone()
    err, bound = (out.cpu().double() - ref).abs().max().item(), 2.0 ** -7 * ref.abs().max().item()
    print(f"moe block {(T, E, k, hidden, inter)} {pattern}: max err {err:.3e}, bound {bound:.3e}")
    assert torch.isfinite(out).all()
    assert err <= bound, (err, bound)
    assert torch.isnan(buf[T:]).all()
    assert torch.equal(ops.fused_moe(x, w1, w2, logits, k, True), first)
    if T == 33:  # a token's row does not depend on the rest of the batch
        for t in (0, 15, 16, 32):
            assert torch.equal(ops.fused_moe(x[t:t + 1], w1, w2, logits[t:t + 1], k, True)[0], first[t])


def test_long_expert_runs_token_chunks_and_the_plugin_backend(dev, monkeypatch):
    """70 rows per chosen expert = two work items of one expert (64 + 6 rows); token chunks of 32 change no bit; the
    plugin's backend is fused_moe written into hidden_states."""
    from mini_sglang_amd import ops
    from mini_sglang_amd.minisgl_plugin import HipMoeBackend

    T, E, k, hidden, inter = 70, 8, 2, 128, 64
    cpu, (x, w1, w2, logits) = make_block(T, E, k, hidden, inter, "skewed", dev)
    ref = ref_block(*cpu, k)
    out = ops.fused_moe(x, w1, w2, logits, k, True)
    assert (out.cpu().double() - ref).abs().max().item() <= 2.0 ** -7 * ref.abs().max().item()
    monkeypatch.setattr(ops, "MOE_MAX_CHUNK_TOKENS", 32)
    assert torch.equal(ops.fused_moe(x, w1, w2, logits, k, True), out)
    monkeypatch.undo()
    hs = x.clone()
    got = HipMoeBackend().forward(hs, w1, w2, logits, k, True, "silu", False)
    assert got.data_ptr() == hs.data_ptr() and torch.equal(hs, out)
    with pytest.raises(ValueError):
        HipMoeBackend().forward(hs, w1, w2, logits, k, True, "gelu", False)


def test_graph_replay_follows_the_routing(dev):
    from mini_sglang_amd import ops

    T, E, k, hidden, inter = 33, 16, 4, 256, 96
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


def torch_moe(dtype):
    """ops.fused_moe stated in torch at `dtype` (bf16 `act` at fp32), dense over experts so that it captures."""
    def fn(x, w1, w2, router_logits, topk, renormalize, out=None):
        inter, xf = w2.shape[2], x.to(dtype)
        w, ids = ref_route(router_logits, topk, renormalize, dtype)
        acc = torch.zeros_like(xf)
        for e in range(w1.shape[0]):
            h = torch.nn.functional.silu(xf @ w1[e, :inter].to(dtype).T) * (xf @ w1[e, inter:].to(dtype).T)
            if dtype == torch.float32:
                h = h.bfloat16().to(dtype)
            acc += (w * (ids == e)).sum(-1, keepdim=True) * (h @ w2[e].to(dtype).T)
        return acc.to(x.dtype) if out is None else out.copy_(acc)
    return fn


def generate(dev, model, graph_bs, max_tokens, sample=None, **engine_args):
    """One 20-token prompt through Engine + OfflineRunner (greedy) -> output ids; `sample` replaces the sampler."""
    from mini_sglang_amd.core import SamplingParams
    from mini_sglang_amd.engine import Engine, EngineConfig
    from mini_sglang_amd.offline import OfflineRunner

    eng = Engine(EngineConfig(model=model, max_running_req=4, page_size=4, cuda_graph_bs=graph_bs, max_seq_len_override=128,
                              num_page_override=64, gemm_tune="off", **engine_args), dev)
    eng.sampler.sample = sample or eng.sampler.sample
    runner = OfflineRunner(eng, seed=1)
    prompt = torch.randint(0, 1000, (20,), generator=torch.Generator().manual_seed(2)).tolist()
    runner.generate([prompt], [SamplingParams(temperature=0.0, max_tokens=max_tokens, ignore_eos=True)])
    ids = [runner.output_ids(s) for s in runner.last_states]
    eng.shutdown()
    return ids


def test_tiny_moe_model_within_twice_the_fp32_floor(dev, monkeypatch):
    """Prefill of 20 tokens + 3 graph-replayed decode steps with forced tokens: logits with the HIP expert MLP against
    the fp32 torch statement, bounded by twice that statement's own distance from fp64."""
    from mini_sglang_amd import ops
    from mini_sglang_amd.model import PRESETS

    def logits_of(moe_fn):
        rec = []

        def sample(logits, args):  # forced tokens: the three runs see the same inputs whatever their logits
            rec.append(logits.float().cpu())
            return torch.full((logits.shape[0],), 11 * len(rec), dtype=torch.int32, device=logits.device)

        if moe_fn is not None:
            monkeypatch.setattr(ops, "fused_moe", moe_fn)
        generate(dev, PRESETS["tiny-moe"], [1], 4, sample)
        monkeypatch.undo()
        assert len(rec) == 4
        return torch.cat(rec)

    hip, f32, f64 = logits_of(None), logits_of(torch_moe(torch.float32)), logits_of(torch_moe(torch.float64))
    dev_hip, floor = (hip - f32).abs().max().item(), (f32 - f64).abs().max().item()
    msg = f"hip vs fp32 {dev_hip:.3e}, fp32 vs fp64 {floor:.3e}, max |logit| {f64.abs().max().item():.3e}"
    print("tiny-moe logits:", msg)
    assert dev_hip <= 2 * floor, msg


class _OtherRanksAddZeros:
    """Rank 0's communicator of a tp = 2 group on one GPU: the absent rank contributes zeros."""

    def all_reduce(self, x, op="sum"):
        pass

    def all_gather(self, out, x):
        out[:x.shape[0]].copy_(x)
        out[x.shape[0]:].zero_()


def test_tiny_moe_tp2_shard_graph_replay_equals_eager(dev):
    """The tp > 1 branch (expert shards of I_l = 64, all-reduce + add + norm after the expert MLP), captured and eager."""
    import dataclasses

    from mini_sglang_amd.model import PRESETS

    model = dataclasses.replace(PRESETS["tiny-moe"], moe_intermediate_size=128)
    outs = [generate(dev, model, bs, 5, tp_size=2, comm=_OtherRanksAddZeros()) for bs in ([1], [])]
    assert outs[0] == outs[1] and len(outs[0][0]) == 5
