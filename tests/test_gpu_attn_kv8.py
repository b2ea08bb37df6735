"""GPU parity: the FP8 (e4m3) KV cache of csrc/attn_kv8.hip -- quantising store, decode, prefill -- vs the fp64 oracle on the
dequantised cache, and the `tiny` engine end to end with kv_quant="fp8_e4m3".

Builders in the style of test_gpu_attn_d64.py (permuted pool slots, ragged lengths, extra table rows, q as a strided view of a
fused qkv row); table tails point at a page of byte 0x7f, the e4m3fn NaN.  K and V are randn quantised with the scale under
test, so the dequantised values are ~N(0, 1) whatever the scale and the project's absolute tolerances keep their meaning: the
kernels multiply exactly the values the oracle reads, the only extra operations are two fp32 scale multiplications.
"""
import math

import pytest
import torch

import parity_stats
import test_gpu_model as tm
from oracle import ref_model, ref_ops
from test_gpu_attn_d64 import DECODE_LENS, DECODE_TOL, PREFILL_SPECS, PREFILL_TOL

pytestmark = pytest.mark.gpu

D = 128
F8 = torch.float8_e4m3fn
SCALES = [(1.0, 1.0), (0.37, 1.6)]
KV8_LOGIT_TOL = 1.5 * 4.85e-2  # 1.5 x the measured max |logit error| of the end-to-end run below


@pytest.fixture(scope="module")
def ops(dev):
    from mini_sglang_amd import ops as _ops

    return _ops


def quant(x, scale):
    return (x.float() / scale).clamp(-448, 448).to(F8)


def build(g, specs, hq, hkv, page_size, scales, head_dim=D, dtype=torch.bfloat16):
    """specs: (cached_len, device_len) per request; a decode request is (n - 1, n)."""
    B = len(specs)
    max_seq = (max(dl for _, dl in specs) + 31) // 32 * 32
    pages_per = (max_seq + page_size - 1) // page_size
    n_pages = (B + 3) * pages_per + 2  # + a spare page + the poison page
    k = quant(torch.randn((n_pages * page_size, hkv, head_dim), generator=g), scales[0])
    v = quant(torch.randn((n_pages * page_size, hkv, head_dim), generator=g), scales[1])
    poison = (n_pages - 1) * page_size
    k.view(torch.uint8)[poison:] = 0x7F
    v.view(torch.uint8)[poison:] = 0x7F
    perm = torch.randperm(n_pages - 2, generator=g)
    table = torch.full((B + 3, max_seq), poison, dtype=torch.int32)  # entries past a length must never be dereferenced
    rows = torch.randperm(B + 3, generator=g)[:B].tolist()
    pp = 0
    for (_, dl), row in zip(specs, rows):
        need = (dl + page_size - 1) // page_size
        pg = perm[pp: pp + need].to(torch.int32) * page_size
        pp += need
        table[row, :dl] = (pg.unsqueeze(1) + torch.arange(page_size, dtype=torch.int32)).flatten()[:dl]
    q_lens = [dl - cl for cl, dl in specs]
    qkv = torch.randn((sum(q_lens), (hq + 2 * hkv) * head_dim), generator=g).to(dtype)
    return dict(k=k, v=v, table=table, rows=rows, q_lens=q_lens, k_lens=[dl for _, dl in specs], qkv=qkv, hq=hq, hkv=hkv,
                D=head_dim, scales=scales)


def oracle(c):
    q = c["qkv"][:, : c["hq"] * c["D"]].reshape(-1, c["hq"], c["D"])
    return ref_ops.paged_attention_ref(q, c["k"].double() * c["scales"][0], c["v"].double() * c["scales"][1], c["table"],
                                       c["rows"], c["k_lens"], c["q_lens"], c["D"] ** -0.5, double=True)


def decode_buffers(ops, dev, c, capacity):
    B, hq, d = len(c["k_lens"]), c["hq"], c["D"]
    qkv = c["qkv"].to(dev)
    return dict(q=qkv[:, : hq * d].view(B, hq, d), out=torch.zeros((B, hq, d), dtype=qkv.dtype, device=dev),
                plan=torch.zeros(ops.attn_decode_plan_words(B, capacity), dtype=torch.int32, device=dev),
                ws=torch.empty(ops.attn_decode_workspace_bytes(capacity, hq, d), dtype=torch.uint8, device=dev),
                seq=torch.tensor(c["k_lens"], dtype=torch.int32, device=dev),
                rows=torch.tensor(c["rows"], dtype=torch.int32, device=dev), k=c["k"].to(dev), v=c["v"].to(dev),
                table=c["table"].to(dev))


def launch_decode(ops, c, t, capacity, slot_run, off=0):
    B = len(c["k_lens"])
    k = t["k"] if not off else t["k"].flatten()[off:][: t["k"][1:].numel()].view(-1, c["hkv"], c["D"])  # misaligned view
    ops.attn_decode(t["out"], t["q"], k, t["v"][: k.shape[0]], t["table"], t["rows"], t["seq"], t["plan"], t["ws"], B, B,
                    capacity, 1.0 / math.sqrt(c["D"]), slot_run=slot_run, k_scale=c["scales"][0], v_scale=c["scales"][1])


def run_decode(ops, dev, c, slot_run=1, capacity=None, off=0):
    B = len(c["k_lens"])
    capacity = capacity or max(4 * B, 1024)
    t = decode_buffers(ops, dev, c, capacity)
    ops.attn_decode_plan(t["plan"], t["seq"], B, B, capacity, c["hq"], c["hkv"])
    launch_decode(ops, c, t, capacity, slot_run, off)
    torch.cuda.synchronize()
    return t["out"].cpu()


def run_prefill(ops, dev, c, impl=0, reverse=False):
    hq, d = c["hq"], c["D"]
    qkv = c["qkv"].to(dev)
    T = qkv.shape[0]
    out = torch.zeros((T, hq, d), dtype=qkv.dtype, device=dev)
    qt = ops.prefill_q_tile(impl)
    cu_q = torch.tensor([0] + c["q_lens"]).cumsum(0).to(torch.int32)
    tile_cu = torch.tensor([0] + [(n + qt - 1) // qt for n in c["q_lens"]]).cumsum(0).to(torch.int32)
    total = int(tile_cu[-1])
    order = torch.arange(total - 1, -1, -1, dtype=torch.int32, device=dev) if reverse else None
    ops.attn_prefill(out, qkv[:, : hq * d].view(T, hq, d), c["k"].to(dev), c["v"].to(dev), c["table"].to(dev),
                     torch.tensor(c["rows"], dtype=torch.int32, device=dev),
                     torch.tensor(c["k_lens"], dtype=torch.int32, device=dev), cu_q.to(dev), tile_cu.to(dev),
                     len(c["q_lens"]), total, d ** -0.5, tile_order=order, impl=impl, k_scale=c["scales"][0],
                     v_scale=c["scales"][1])
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("hq,hkv", [(40, 8), (14, 2), (8, 8), (16, 1)])
@pytest.mark.parametrize("page_size,slot_run", [(1, 1), (16, 16), (256, 256), (16, 1)])
def test_decode_matches_oracle(ops, dev, hq, hkv, page_size, slot_run, scales):
    g = torch.Generator().manual_seed(hq * 100 + hkv + page_size + slot_run)
    c = build(g, [(n - 1, n) for n in DECODE_LENS], hq, hkv, page_size, scales)
    out = run_decode(ops, dev, c, slot_run=slot_run)
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.double(), oracle(c), **DECODE_TOL)


def test_decode_long_pieces_split_kv_and_graph_replay(ops, dev):
    """~40 requests of 2500-4200 tokens: every wave runs the ring's steady state, pieces start and end inside requests and
    the merge kernel combines them.  Then one captured launch, replayed after seq_lens changed and the plan was re-made."""
    g = torch.Generator().manual_seed(64)
    lens = [int(x) for x in torch.randint(2500, 4200, (40,), generator=g)] + [1, 15, 16, 17, 33, 49]
    c = build(g, [(n - 1, n) for n in lens], 40, 8, 256, SCALES[1])
    B, cap = len(lens), 1024
    out = run_decode(ops, dev, c, slot_run=256, capacity=cap)
    torch.testing.assert_close(out.double(), oracle(c), **DECODE_TOL)
    assert torch.equal(out, run_decode(ops, dev, c, slot_run=256, capacity=cap))
    # the same cache one step earlier (every request one token shorter, the one-token requests left as they are)
    short = dict(c, k_lens=[max(n - 1, 1) for n in lens])
    want = [run_decode(ops, dev, short, slot_run=256, capacity=cap), out]
    t = decode_buffers(ops, dev, short, cap)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.attn_decode_plan(t["plan"], t["seq"], B, B, cap, 40, 8)
        launch_decode(ops, c, t, cap, 256)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            launch_decode(ops, c, t, cap, 256)
        for k_lens, expect in zip((short["k_lens"], lens), want):
            t["seq"].copy_(torch.tensor(k_lens, dtype=torch.int32))
            ops.attn_decode_plan(t["plan"], t["seq"], B, B, cap, 40, 8)
            t["out"].zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(t["out"].cpu(), expect)


@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("hq,hkv", [(40, 8), (14, 2), (4, 4)])
@pytest.mark.parametrize("page_size", [1, 16])
def test_prefill_matches_oracle_and_decode(ops, dev, hq, hkv, page_size, scales):
    c = build(torch.Generator().manual_seed(hq + page_size), PREFILL_SPECS, hq, hkv, page_size, scales)
    out = run_prefill(ops, dev, c)
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.double(), oracle(c), **PREFILL_TOL)
    assert torch.equal(out, run_prefill(ops, dev, c, impl=4, reverse=True))  # tile_order is a scheduling hint only
    last = (torch.tensor(c["q_lens"]).cumsum(0) - 1).tolist()  # the last query row of each request is a decode step
    dec = run_decode(ops, dev, dict(c, qkv=c["qkv"][last].contiguous(), q_lens=[1] * len(last)))
    torch.testing.assert_close(out[last].float(), dec.float(), **PREFILL_TOL)


@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("norm,loc_dtype", [(True, torch.int32), (False, torch.int64)])
def test_store_quantises_what_the_16_bit_store_writes(ops, dev, norm, loc_dtype, scales):
    hq, hkv, T, slots = 10, 2, 37, 64
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn((T, (hq + 2 * hkv) * D), generator=g)
    qkv[3] *= 600.0  # |x / scale| > 448 in k (without qk-norm) and v: the clamp
    qkv = qkv.to(torch.bfloat16).to(dev)
    qw, kw = ((1 + 0.1 * torch.randn(D, generator=g)).to(torch.bfloat16).to(dev) for _ in range(2))
    pos = torch.randint(0, 500, (T,), generator=g).to(torch.int32).to(dev)
    cs = torch.randn((512, D), generator=g).to(dev)
    loc = torch.randperm(slots, generator=g)[:T].to(loc_dtype).to(dev)
    res = []
    for dt in (torch.bfloat16, F8):
        x = qkv.clone()
        pool = torch.full((2, slots, hkv * D), 0x55, dtype=torch.uint8, device=dev).repeat(1, 1, dt.itemsize).view(dt)
        q, k, v = x.split([hq * D, hkv * D, hkv * D], dim=-1)
        kw_ = dict(k_scale=scales[0], v_scale=scales[1]) if dt == F8 else {}
        ops.qk_norm_rope_store(q, k, v, qw if norm else None, kw if norm else None, 1e-6, pos, cs, pool[0], pool[1], loc, D, **kw_)
        torch.cuda.synchronize()
        res.append((x.cpu(), pool.cpu()))
    (x16, p16), (x8, p8) = res
    assert torch.equal(x16, x8)  # q, k in place and v are the 16-bit path's bits
    want = torch.stack([quant(p16[0], scales[0]), quant(p16[1], scales[1])]).view(torch.uint8)
    written = torch.zeros(slots, dtype=torch.bool)
    written[loc.cpu().long()] = True
    assert torch.equal(p8.view(torch.uint8)[:, written], want[:, written])
    assert bool((p8.view(torch.uint8)[:, ~written] == 0x55).all()) and bool((want[:, written] == 0x7E).any())


def test_refusals_launch_nothing(ops, dev):
    from mini_sglang_amd._lib import MsglError

    g = torch.Generator().manual_seed(6)
    c = build(g, [(39, 40)], 4, 2, 16, SCALES[0])
    cases = [(build(g, [(39, 40)], 4, 2, 16, SCALES[0], head_dim=64), {}), (build(g, [(39, 40)], 4, 2, 16, SCALES[0], dtype=torch.float16), {}),
             (dict(c, scales=(0.0, 1.0)), {}), (dict(c, scales=(1.0, float("nan"))), {}), (c, dict(off=8))]  # off: rows not 16-byte aligned
    outs = []
    for bad, kw in cases:
        t = decode_buffers(ops, dev, bad, 1024)
        ops.attn_decode_plan(t["plan"], t["seq"], 1, 1, 1024, 4, 2)
        with pytest.raises(MsglError):
            launch_decode(ops, bad, t, 1024, 16, **kw)
        outs.append(t["out"])
        if not kw:
            with pytest.raises(MsglError):
                run_prefill(ops, dev, bad)
    with pytest.raises(MsglError):
        run_prefill(ops, dev, c, impl=2)
    try:
        for code in (1, 22, 72):  # one production kernel: no other may be named for it
            ops.attn_decode_select(code)
            with pytest.raises(MsglError):
                launch_decode(ops, c, t, 1024, 16)
    finally:
        ops.attn_decode_select(0)
    torch.cuda.synchronize()
    assert all(bool((o == 0).all()) for o in outs)


def test_tiny_engine_kv_fp8_teacher_forced_vs_cpu_oracle(dev):
    """Prefill + graph-replayed decode of the `tiny` engine with kv_quant="fp8_e4m3" (configuration and prompts of
    test_gpu_w8a8.py::_tiny_logits) against oracle.ref_model.forward, which keeps a 16-bit KV cache: this error cannot be
    derived, the bound is 1.5 x the max measured on MI355X (the run is deterministic; the margin covers the lm_head library
    plan differing between boxes).  Measured: |err| max 4.85e-2, p99 2.93e-2, mean 8.78e-3 over 30720 logits of standard
    deviation 0.32."""
    from mini_sglang_amd.engine import Engine, EngineConfig
    from mini_sglang_amd.model import PRESETS

    recs = {}
    for kvq in ("fp8_e4m3", None):
        cfg = EngineConfig(model=PRESETS["tiny"], dtype=torch.bfloat16, max_running_req=16, page_size=4, cuda_graph_bs=[1, 2, 4, 8],
                           max_seq_len_override=512, num_page_override=1024, seed=42, kv_quant=kvq)
        eng = Engine(cfg, dev)
        assert eng.kv_cache.pool.dtype == (F8 if kvq else torch.bfloat16)
        eng.kv_cache.pool.view(torch.uint8).zero_()
        recs[kvq] = []
        tm.run(eng, tm.prompts(5), 6, record=recs[kvq])  # 5 decode steps
        if kvq:
            w, table = ref_model.weights_from_device_model(eng.model), eng.page_table.cpu()
            slots = eng.kv_cache.pool.shape[2] * eng.kv_cache.pool.shape[3]
        eng.shutdown()
    mc = PRESETS["tiny"]
    kp = [torch.zeros((slots, mc.num_kv_heads, mc.head_dim), dtype=torch.bfloat16) for _ in range(mc.num_layers)]
    vp = [torch.zeros_like(k) for k in kp]
    stats, ok = {}, True
    for r in recs["fp8_e4m3"]:
        logits = ref_model.forward(mc, w, r["input_ids"], r["positions"], r["out_loc"], kp, vp, table, r["rows"], r["k_lens"],
                                   r["q_lens"], r["phase"] == "prefill").float()[: r["size"]]
        stats = parity_stats.merge_stats(stats, parity_stats.logit_error_stats(r["logits"], logits))
        top2 = logits.topk(2, dim=-1).values
        sure = (top2[:, 0] - top2[:, 1]) > 2 * KV8_LOGIT_TOL
        ok = ok and bool((r["logits"].argmax(-1) == logits.argmax(-1))[sure].all())
    print(f"\n[teacher-forced tiny kv fp8_e4m3] {parity_stats.fmt(stats)}")
    assert stats["max_abs"] <= KV8_LOGIT_TOL and ok
    assert any(not torch.equal(a["logits"], b["logits"]) for a, b in zip(recs["fp8_e4m3"], recs[None]))  # the new path really ran
