"""W8A8 projection (csrc/gemm_w8a8.hip): the activation quantiser bit for bit against its torch statement, the FP8 x FP8
GEMM against fp64 of the same quantised operands for every M class and knob set, the routing of ops.linear, graph replay of
the k-sliced path, argument refusals, and the `tiny` engine end to end with weight_quant="fp8_block128_a8".

Weights, activations and the GEMM tolerance (2^-7 * max|ref|) are those of tests/test_gpu_w8.py."""
import ctypes

import pytest
import torch

import parity_stats
import test_gpu_model as tm
from mini_sglang_amd import ops
from oracle import ref_model
from test_gpu_w8 import _check, _weight, _x

pytestmark = pytest.mark.gpu
B = 128
A8_LOGIT_TOL = 1.5 * 6.45e-2  # 1.5 x the measured max |logit error| of the end-to-end run below


def _quant_ref(x):
    """The torch statement of the quantiser, on the CPU in fp32."""
    f = x.float().cpu()
    sx = f.view(f.shape[0], -1, B).abs().amax(-1).clamp_min(torch.finfo(torch.float32).tiny) / 448
    return (f / sx.repeat_interleave(B, 1)).to(torch.float8_e4m3fn), sx


@pytest.mark.parametrize("M,K", [(1, 128), (17, 640), (130, 2048)])
def test_a8_quant_is_bit_exact(dev, M, K):
    x = _x(dev, M, K, seed=M + K)
    x[0, :B] = 0  # amax 0: the FLT_MIN floor
    x[M // 2, K - B:] *= 2.0 ** 10
    x[M - 1, (K // B // 2) * B:][:B] *= 2.0 ** -20
    want_q, want_s = _quant_ref(x)
    xq, sx = ops.a8_quant(x)
    assert torch.equal(sx.cpu(), want_s) and torch.equal(xq.view(torch.uint8).cpu(), want_q.view(torch.uint8))
    # a strided input view into a strided xq view: the neighbours are kept
    xs = torch.full((M + 2, K + 64), 7.0, dtype=torch.bfloat16, device=dev)
    xs[:M, :K] = x
    big = torch.full((M + 2, K + 128), 0x55, dtype=torch.uint8, device=dev)
    ops.a8_quant(xs[:M, :K], out=(big.view(torch.float8_e4m3fn)[:M, :K], sx))
    assert torch.equal(big[:M, :K].cpu(), want_q.view(torch.uint8)) and torch.equal(sx.cpu(), want_s)
    assert bool((big[M:] == 0x55).all()) and bool((big[:, K:] == 0x55).all())


@pytest.fixture(scope="module", params=[(128, 128), (384, 640), (256, 2048)], ids=lambda p: "%dx%d" % p)
def weight(request, dev):
    N, K = request.param
    return _weight(dev, N, K, seed=N + K)


@pytest.mark.parametrize("M", [1, 33, 128, 129, 257, 300])
def test_w8a8_gemm_vs_fp64(dev, weight, M):
    w, wd = weight
    K = w.shape[1]
    x = _x(dev, M, K, seed=M)
    rq, rs = _quant_ref(x)
    ref = (rq.double() * rs.double().repeat_interleave(B, 1)) @ wd.t()
    xq, sx = ops.a8_quant(x)
    out = ops.w8a8_gemm(xq, sx, w)
    _check(out, ref)
    assert torch.equal(out, ops.w8a8_gemm(xq, sx, w))  # same bits on every launch
    knobs = [(128, 1), (256, 1)] + ([(128, 2)] if K >= 256 else []) + ([(128, 5)] if K == 640 else [])
    for tm_, k_slices in knobs:  # the knobs only reorder fp32 sums
        _check(ops.w8a8_gemm(xq, sx, w, tm=tm_, k_slices=k_slices), ref)
    if M == 129:  # a strided out view keeps its neighbours
        big = torch.full((136, w.shape[0] + 128), -3.0, dtype=torch.bfloat16, device=dev)
        assert torch.equal(ops.w8a8_gemm(xq, sx, w, out=big[:M, : w.shape[0]]), out)
        assert bool((big[M:] == -3.0).all()) and bool((big[:, w.shape[0]:] == -3.0).all())


def test_linear_routes_act_quant_weights_from_w8a8_min_m(dev):
    w, _ = _weight(dev, 384, 640, seed=6)
    a8 = ops.Fp8Weight(w.q, w.scales, act_quant="fp8_group128")
    m = ops.W8A8_MIN_M
    x = _x(dev, max(m, 300), 640, seed=7)
    scratch = ops.w8_reserve(dev, 384 * 640)
    scratch.fill_(-3.0)
    assert torch.equal(ops.linear(x[:m], a8), ops.w8a8_linear(x[:m], a8))
    assert bool((scratch == -3.0).all())  # the A8 route dequantises nothing
    assert torch.equal(ops.linear(x[: m - 1], a8), ops.linear(x[: m - 1], w))  # below the threshold: today's route
    assert w.act_quant is None and torch.equal(ops.linear(x[:300], w), ops.linear(x[:300], ops.w8_dequant(w)))  # today's bits


def test_w8a8_gemm_graph_replay_equals_eager(dev):
    w, _ = _weight(dev, 256, 2048, seed=4)
    a8 = ops.Fp8Weight(w.q, w.scales, act_quant="fp8_group128")
    x = _x(dev, 130, 2048, seed=5)
    assert ops.w8a8_plan(130, 256, 2048)[1] > 1  # the k-sliced path: slabs + the reduce launch
    eager = ops.w8a8_linear(x, a8)
    out = torch.empty_like(eager)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.w8a8_linear(x, a8, out=out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ops.w8a8_linear(x, a8, out=out)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("bad", [dict(dtype=1), dict(N=192), dict(K=192), dict(tm=64), dict(slices=0), dict(slices=3),
                                 dict(slices=2, ws_bytes=1024), dict(slices=2, wo=8), dict(ldxq=264), dict(ldq=264),
                                 dict(ldo=130), dict(xo=8), dict(qo=8), dict(so=2)], ids=lambda b: "-".join(b))
def test_w8a8_entry_points_refuse_what_they_cannot_do(dev, bad):
    from mini_sglang_amd import _lib

    w, _ = _weight(dev, 128, 256, seed=8)
    x = _x(dev, 4, 256, seed=8)
    xq, sx = ops.a8_quant(x)
    out = torch.full((4, 128), 5.0, dtype=torch.bfloat16, device=dev)
    ws, p = ops.gemm_workspace(dev), ctypes.c_void_p

    def call(M=4, N=128, K=256, ldxq=256, ldq=256, ldo=128, dtype=_lib.BF16, tm=128, slices=1, ws_bytes=1 << 20, xo=0, qo=0,
             wo=0, so=0):
        return _lib.lib().msgl_w8a8_gemm_nt(p(out.data_ptr()), p(xq.data_ptr() + xo), p(sx.data_ptr() + so), p(w.q.data_ptr() + qo),
                                            p(w.scales.data_ptr()), M, N, K, ldxq, ldq, ldo, dtype, tm, slices,
                                            p(ws.data_ptr() + wo), ws_bytes, None)

    assert call(**bad) == -1
    assert _lib.lib().msgl_last_error()
    q8 = torch.full((4, 256), 0x55, dtype=torch.uint8, device=dev)
    for K, ldx, ldxq, dtype, xo in ((192, 256, 256, _lib.BF16, 0), (256, 260, 256, _lib.BF16, 0), (256, 256, 264, _lib.BF16, 0),
                                    (256, 256, 256, _lib.FP16, 0), (256, 256, 256, _lib.BF16, 8)):
        assert _lib.lib().msgl_a8_quant(p(q8.data_ptr()), p(sx.data_ptr()), p(x.data_ptr() + xo), 4, K, ldx, ldxq, dtype, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((q8 == 0x55).all())  # nothing was launched


def _tiny_logits(dev, weight_quant):
    from mini_sglang_amd.engine import Engine, EngineConfig
    from mini_sglang_amd.model import PRESETS

    cfg = EngineConfig(model=PRESETS["tiny"], dtype=torch.bfloat16, max_running_req=16, page_size=4, cuda_graph_bs=[1, 2, 4, 8],
                       max_seq_len_override=512, num_page_override=1024, seed=42, weight_quant=weight_quant)
    eng = Engine(cfg, dev)
    eng.kv_cache.pool.zero_()
    rec = []
    tm.run(eng, tm.prompts(5), 6, record=rec)  # 5 decode steps
    return cfg, eng, rec


def test_tiny_engine_fp8_block128_a8_teacher_forced_vs_cpu_oracle(dev, monkeypatch):
    """Prefill + graph-replayed decode of the `tiny` engine with every dense projection on the W8A8 path (W8A8_MIN_M = 1, no upper end)
    against oracle.ref_model.forward on the bf16-rounded dequantised weights.  The oracle does not quantise activations, so
    this error cannot be derived: the bound is 1.5 x the max measured on MI355X (the run is deterministic; the margin covers
    the lm_head library plan differing between boxes).  Measured: |err| max 6.45e-2, p99 3.93e-2, mean 1.20e-2 over 30720
    logits of standard deviation 0.32 (W8A16: 1.17e-2 / 6.35e-3 / 1.79e-3)."""
    monkeypatch.setattr(ops, "W8A8_MIN_M", 1)
    monkeypatch.setattr(ops, "W8A8_MAX_M", 1 << 30)
    cfg, eng, rec = _tiny_logits(dev, "fp8_block128_a8")
    m = eng.model
    assert all(getattr(lw, k).act_quant == "fp8_group128" for lw in m.layers for k in ("qkv", "o", "gate_up", "down"))
    layers = [{k: (getattr(lw, k).dequantize().bfloat16().cpu() if k in ("qkv", "o", "gate_up", "down") else getattr(lw, k).cpu())
               for k in ("input_norm", "qkv", "q_norm", "k_norm", "o", "post_norm", "gate_up", "down")} for lw in m.layers]
    w = ref_model.CpuWeights(m.embed.cpu(), layers, m.final_norm.cpu(), m.lm_head.cpu(), m.cos_sin.cpu())
    mc, table = cfg.model, eng.page_table.cpu()
    slots = eng.kv_cache.pool.shape[2] * eng.kv_cache.pool.shape[3]
    kp = [torch.zeros((slots, mc.num_kv_heads, mc.head_dim), dtype=torch.bfloat16) for _ in range(mc.num_layers)]
    vp = [torch.zeros_like(k) for k in kp]
    stats, fails = {}, []
    for r in rec:
        logits = ref_model.forward(mc, w, r["input_ids"], r["positions"], r["out_loc"], kp, vp, table, r["rows"], r["k_lens"],
                                   r["q_lens"], r["phase"] == "prefill").float()[: r["size"]]
        st = parity_stats.logit_error_stats(r["logits"], logits)
        stats = parity_stats.merge_stats(stats, st)
        top2 = logits.topk(2, dim=-1).values
        sure = (top2[:, 0] - top2[:, 1]) > 2 * A8_LOGIT_TOL
        if st["max_abs"] > A8_LOGIT_TOL or not bool((r["logits"].argmax(-1) == logits.argmax(-1))[sure].all()):
            fails.append(parity_stats.fmt(st))
    print(f"\n[teacher-forced tiny fp8_block128_a8] {parity_stats.fmt(stats)}")
    eng.shutdown()
    _, eng16, rec16 = _tiny_logits(dev, "fp8_block128")  # the same prompts as W8A16: the new path really ran
    eng16.shutdown()
    assert any(not torch.equal(a["logits"], b["logits"]) for a, b in zip(rec, rec16))
    assert sum(r["phase"] == "decode" for r in rec) == 5 and not fails, fails
