"""Attention over a 16-bit KV pool against the FP8 (e4m3) pool of csrc/attn_kv8.hip, at Qwen3-14B's head counts (40 / 8, head_dim
128): captured decode attention at batches 64 / 256 with contexts 1 k / 4 k / 16 k, and eager prefill attention at 2 k / 8 k tokens.

    python tools/kv8_bench.py [--out profiles/kv8_bench.json] [--replays 8] [--rounds 9] [--page-size 16]

Same process, same box, alternating: per shape both pools hold the same values (the FP8 one is the 16-bit one quantised with
scales 1.0), the page table scatters pages over the pool, both sides run the same plan, and the two graphs (decode: `--replays`
calls each, rotating over enough layers that K / V come from HBM, not the Infinity Cache) or the two eager calls (prefill) are
timed in turn `--rounds` times; medians of the per-call time.  Algorithmic bytes = K and V rows read once.  No GPU: fails,
nothing is estimated."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mini_sglang_amd import ops  # noqa: E402
from mini_sglang_amd.model import PRESETS  # noqa: E402

F8 = torch.float8_e4m3fn


def timed_us(fn, per_call: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / per_call


def pools(dev, g, layers, slots, hkv, D):
    k16 = [torch.randn((slots, hkv, D), generator=g, device=dev, dtype=torch.bfloat16) for _ in range(2 * layers)]
    return {torch.bfloat16: k16, F8: [t.to(F8) for t in k16]}


def paged_table(dev, g, batch, ctx, page):
    pages = (ctx + page - 1) // page
    perm = torch.randperm(batch * pages, generator=g, device=dev).view(batch, pages).to(torch.int32) * page
    return (perm.unsqueeze(2) + torch.arange(page, dtype=torch.int32, device=dev)).view(batch, -1)[:, : (ctx + 31) // 32 * 32].contiguous()


def row(samples, nbytes, **shape) -> dict:
    us = {k: statistics.median(v) for k, v in samples.items()}
    return dict(**shape, bf16_us=round(us["bf16"], 2), fp8_us=round(us["fp8"], 2), fp8_speedup=round(us["bf16"] / us["fp8"], 3),
                bf16_bytes_per_s=round(2 * nbytes / (us["bf16"] * 1e-6)), fp8_bytes_per_s=round(nbytes / (us["fp8"] * 1e-6)),
                spread_us={k: [round(min(v), 2), round(max(v), 2)] for k, v in samples.items()})


def decode_row(args, dev, g, hq, hkv, D, batch, ctx) -> dict:
    page = args.page_size
    slots = batch * ((ctx + page - 1) // page) * page
    layers = max(1, min(8, (1 << 30) // (slots * hkv * D)))  # >= 1 GiB of FP8 K + V per rotation where that takes <= 8 layers
    kv = pools(dev, g, layers, slots, hkv, D)
    table = paged_table(dev, g, batch, ctx, page)
    seq = torch.full((batch,), ctx, dtype=torch.int32, device=dev)
    cap = max(4096, 4 * batch)
    plan = torch.zeros(ops.attn_decode_plan_words(batch, cap), dtype=torch.int32, device=dev)
    ws = torch.empty(ops.attn_decode_workspace_bytes(cap, hq, D), dtype=torch.uint8, device=dev)
    q = torch.randn((batch, hq, D), generator=g, device=dev, dtype=torch.bfloat16)
    ops.attn_decode_plan(plan, seq, batch, batch, cap, hq, hkv)
    outs, graphs = {}, {}
    for name, dt in (("bf16", torch.bfloat16), ("fp8", F8)):
        out = outs[name] = torch.empty_like(q)

        def call(i, dt=dt, out=out):
            ops.attn_decode(out, q, kv[dt][2 * (i % layers)], kv[dt][2 * (i % layers) + 1], table, None, seq, plan, ws, batch, batch,
                            cap, D ** -0.5, slot_run=page & -page)
        for i in range(layers):
            call(i)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for i in range(args.replays):
                call(i)
        graphs[name].replay()
    samples = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k, gr in graphs.items():
            samples[k].append(timed_us(gr.replay, args.replays))
    diff = (outs["bf16"].float() - outs["fp8"].float()).abs().max().item()  # both hold the last call: the same layer
    return row(samples, 2 * batch * ctx * hkv * D, kind="decode", batch=batch, context=ctx, layers=layers, page_size=page,
               max_abs_diff_fp8_vs_bf16_pool=round(diff, 5))


def prefill_row(args, dev, g, hq, hkv, D, tokens) -> dict:
    kv = pools(dev, g, 1, tokens, hkv, D)
    table = paged_table(dev, g, 1, tokens, 1)
    q = torch.randn((tokens, hq, D), generator=g, device=dev, dtype=torch.bfloat16)
    qt = ops.prefill_q_tile()
    tiles = (tokens + qt - 1) // qt
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    seq, cu_q, tile_cu = i32([tokens]), i32([0, tokens]), i32([0, tiles])
    order = torch.arange(tiles - 1, -1, -1, dtype=torch.int32, device=dev)  # most keys first, as the engine passes it
    outs = {"bf16": torch.empty_like(q), "fp8": torch.empty_like(q)}
    calls = {n: (lambda n=n, dt=dt: ops.attn_prefill(outs[n], q, kv[dt][0], kv[dt][1], table, None, seq, cu_q, tile_cu, 1, tiles,
                                                   D ** -0.5, tile_order=order))
             for n, dt in (("bf16", torch.bfloat16), ("fp8", F8))}
    samples = {k: [] for k in calls}
    for r in range(args.rounds + 2):  # two warm-up rounds
        for k, fn in calls.items():
            t = timed_us(fn, 1)
            if r >= 2:
                samples[k].append(t)
    diff = (outs["bf16"].float() - outs["fp8"].float()).abs().max().item()
    return row(samples, 2 * tokens * hkv * D, kind="prefill", tokens=tokens, causal_flops=2 * 2 * hq * D * tokens * (tokens + 1) // 2,
               max_abs_diff_fp8_vs_bf16_pool=round(diff, 5))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kv8_bench.json"))
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--contexts", default="1024,4096,16384")
    ap.add_argument("--prefill", default="2048,8192")
    ap.add_argument("--page-size", type=int, default=16)
    ap.add_argument("--replays", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kv8_bench needs the GPU"
    dev = torch.device("cuda:0")
    cfg = PRESETS["qwen3-14b"]
    hq, hkv, D = cfg.num_qo_heads, cfg.num_kv_heads, cfg.head_dim
    g = torch.Generator(device=dev).manual_seed(0)
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    rows = []
    for batch in ints(args.batches):
        for ctx in ints(args.contexts):
            rows.append(decode_row(args, dev, g, hq, hkv, D, batch, ctx))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    for tokens in ints(args.prefill):
        rows.append(prefill_row(args, dev, g, hq, hkv, D, tokens))
        print(json.dumps(rows[-1]), flush=True)
    result = dict(model=cfg.name, device=torch.cuda.get_device_name(0), command="python tools/kv8_bench.py",
                  method=f"decode: {args.replays} calls per captured graph rotating over `layers` K/V sets, the bf16 and fp8 graphs "
                         f"replayed in turn, median of {args.rounds}; prefill: eager calls in turn, median of {args.rounds} after two "
                         f"warm-up rounds; bytes_per_s = K and V rows read once over the call time", rows=rows)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
