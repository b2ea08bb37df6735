"""W8A16 projection GEMM (csrc/gemm_w8.hip): block-scaled e4m3 weights against an fp64 reference of the same product,
the dequantiser bit for bit, the batch > 256 route, argument refusals, and the `tiny` engine end to end with
weight_quant="fp8_block128" teacher-forced against the CPU oracle.

Tolerance of the GEMM cases: the project's GEMM rule (tests/test_gpu_gemm.py), 2^-7 * max|ref|."""
import ctypes

import pytest
import torch

import parity_stats
import test_gpu_model as tm
from mini_sglang_amd import ops
from oracle import ref_model

pytestmark = pytest.mark.gpu
B = 128


def _weight(dev, N, K, seed):
    """e4m3 bytes over the whole finite range and scales that jump by 2^+-3 between neighbouring blocks."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    q[(q & 0x7F) == 0x7F] = 0x30  # the two NaN encodings
    bi, bj = torch.meshgrid(torch.arange(N // B), torch.arange(K // B), indexing="ij")
    s = (2.0 ** (3 * ((bi + bj) % 3 - 1).float()) * (1 + torch.rand((N // B, K // B), generator=g)) / 4096).float()
    w = ops.Fp8Weight(q.view(torch.float8_e4m3fn).to(dev), s.to(dev))
    return w, w.dequantize().double().cpu()


def _x(dev, M, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((M, K), generator=g) * 0.5).to(torch.bfloat16).to(dev)


def _check(out, ref):
    tol = 2 ** -7 * max(ref.abs().max().item(), 1e-3)
    assert torch.isfinite(out.float()).all()
    assert (out.double().cpu() - ref).abs().max().item() <= tol


@pytest.fixture(scope="module", params=[(128, 128), (384, 640), (256, 2048)], ids=lambda p: "%dx%d" % p)
def weight(request, dev):
    N, K = request.param
    return _weight(dev, N, K, seed=N + K)


@pytest.mark.parametrize("M", [1, 3, 16, 17, 64, 200, 256])
def test_w8_gemm_vs_fp64(dev, weight, M):
    w, wd = weight
    x = _x(dev, M, w.shape[1], seed=M)
    ref = x.double().cpu() @ wd.t()
    out = ops.w8_gemm(x, w)
    _check(out, ref)
    assert torch.equal(out, ops.w8_gemm(x, w))  # same bits on every launch
    for slices, tiles in ((1, 1), (2, 2)) if w.shape[1] >= 256 and M <= 64 else ((1, 1),):  # the knobs only reorder fp32 sums
        _check(ops.w8_gemm(x, w, slices=slices, row_tiles=tiles), ref)


def test_w8_gemm_strided_views_keep_their_neighbours(dev):
    w, wd = _weight(dev, 384, 640, seed=9)
    xs = torch.full((24, 640 + 64), 7.0, dtype=torch.bfloat16, device=dev)
    xs[:17, :640] = _x(dev, 17, 640, seed=2)
    big = torch.full((24, 384 + 128), -3.0, dtype=torch.bfloat16, device=dev)
    out = ops.w8_gemm(xs[:17, :640], w, out=big[:17, :384])
    _check(out, xs[:17, :640].double().cpu() @ wd.t())
    assert bool((big[17:] == -3.0).all()) and bool((big[:, 384:] == -3.0).all())


def test_w8_gemm_graph_replay_equals_eager(dev):
    w, _ = _weight(dev, 256, 2048, seed=4)
    x = _x(dev, 8, 2048, seed=5)
    eager = ops.w8_gemm(x, w)
    out = torch.empty_like(eager)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.w8_gemm(x, w, out=out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ops.w8_gemm(x, w, out=out)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_w8_dequant_is_bit_exact_and_serves_batches_above_256(dev):
    w, wd = _weight(dev, 384, 640, seed=6)
    want = (w.q.cpu().float() * w.scales.cpu().repeat_interleave(B, 0).repeat_interleave(B, 1)).bfloat16()
    assert torch.equal(ops.w8_dequant(w).cpu(), want)
    x = _x(dev, 300, 640, seed=7)
    _check(ops.linear(x, w), x.double().cpu() @ wd.t())


def test_w8_entry_points_refuse_what_they_cannot_do(dev):
    from mini_sglang_amd import _lib

    w, _ = _weight(dev, 128, 256, seed=8)
    x = _x(dev, 4, 256, seed=8)
    out = torch.full((4, 128), 5.0, dtype=torch.bfloat16, device=dev)
    gemm, p = _lib.lib().msgl_w8_gemm_nt, ctypes.c_void_p

    def call(M=4, N=128, K=256, ldx=256, ldq=256, ldo=128, dtype=_lib.BF16, slices=1, tiles=1, xo=0, qo=0):
        return gemm(p(out.data_ptr()), p(x.data_ptr() + xo), p(w.q.data_ptr() + qo), p(w.scales.data_ptr()), M, N, K, ldx, ldq, ldo,
                    dtype, slices, tiles, None)

    for bad in (dict(dtype=_lib.FP16), dict(M=0), dict(M=257), dict(N=192), dict(K=192), dict(ldx=260), dict(ldq=264),
                dict(ldo=130), dict(xo=8), dict(qo=8), dict(slices=3), dict(slices=4, tiles=4), dict(tiles=3)):
        assert call(**bad) == -1, bad
        assert _lib.lib().msgl_last_error()
    assert _lib.lib().msgl_w8_dequant(p(out.data_ptr()), p(w.q.data_ptr()), p(w.scales.data_ptr()), 128, 192, 192, 192, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())  # nothing was launched


def test_tiny_engine_fp8_block128_teacher_forced_vs_cpu_oracle(dev):
    """Prefill + graph-replayed decode of the `tiny` engine with quantised projections against oracle.ref_model.forward.  The
    oracle computes in the model dtype, so its CpuWeights hold the bf16-ROUNDED dequantisation of each projection (the
    kernel uses the unrounded q * s: that difference is part of the measured error).  Bound: LOGIT_TOL of test_gpu_model.py.
    Measured on MI355X: |err| max 1.17e-2, p99 6.35e-3, mean 1.79e-3."""
    from mini_sglang_amd.engine import Engine, EngineConfig
    from mini_sglang_amd.model import PRESETS

    cfg = EngineConfig(model=PRESETS["tiny"], dtype=torch.bfloat16, max_running_req=16, page_size=4, cuda_graph_bs=[1, 2, 4, 8],
                       max_seq_len_override=512, num_page_override=1024, seed=42, weight_quant="fp8_block128")
    eng = Engine(cfg, dev)
    eng.kv_cache.pool.zero_()
    rec = []
    tm.run(eng, tm.prompts(5), 6, record=rec)  # 5 decode steps
    m = eng.model
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
        sure = (top2[:, 0] - top2[:, 1]) > 2 * tm.LOGIT_TOL
        if st["max_abs"] > tm.LOGIT_TOL or not bool((r["logits"].argmax(-1) == logits.argmax(-1))[sure].all()):
            fails.append(parity_stats.fmt(st))
    print(f"\n[teacher-forced tiny fp8_block128] {parity_stats.fmt(stats)}")
    eng.shutdown()
    assert sum(r["phase"] == "decode" for r in rec) == 5 and not fails, fails
