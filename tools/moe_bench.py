"""One layer's expert MLP at Qwen3-30B-A3B dimensions: ops.fused_moe (csrc/moe.hip) against a per-expert torch loop.

    python tools/moe_bench.py [--out profiles/moe_bench.json] [--tokens 1,16,64,256,...,8192] [--impl both|rows|tall]

`--impl both` times fused_moe(impl="rows") (csrc/moe.hip) at every T and impl="tall" (csrc/moe_tall.hip) at T >= 256, in this
one process, and checks that the two outputs are the same bits; hip_us is the time of the implementation impl=None picks.
HIP path: `--replays` calls inside one captured graph, rotating over `--layers` weight sets (a decode batch's touched
experts would otherwise be served from the Infinity Cache), device events around the replay, median of `--rounds`.
Baseline, same process and box: index_select -> F.linear -> silu * mul -> F.linear -> index_add_ per expert.  The routing
and the per-expert row lists are made before the timed region (they need the host to know the group sizes), so a timed pass
is eager launches only, no host sync; median of `--rounds` passes.
Algorithmic bytes = the touched experts' w1 and w2 plus x in and out.  No GPU: fails, nothing is estimated.

    python tools/moe_bench.py --w8 [--out profiles/moe_w8_tall_bench.json] [--tokens 256,512,1024,2048,4096,8192]

`--w8`: the same layer with block-scaled FP8 experts (csrc/moe_w8.hip).  Per T one captured graph each for bf16 fused_moe
(impl=None), FP8 impl="rows" and, from T = 256, FP8 impl="tall" (dequantise + csrc/moe_tall.hip) and FP8 impl="tall_w8"
(csrc/moe_w8_tall.hip, `w8_tall_native`, checked to be the bits of FP8 rows); the graphs are replayed in turn, round by
round, in this one process, median per graph.  FP8 bytes = 1 per expert weight + 4 per block."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mini_sglang_amd import ops  # noqa: E402
from mini_sglang_amd.model import PRESETS  # noqa: E402

PEAK_BYTES_PER_S = 8e12
PEAK_BF16_FLOPS = 2.5e15


def timed_us(fn, rounds: int, per_call: int) -> float:
    samples = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b) * 1e3 / per_call)
    return statistics.median(samples)


def expert_groups(weights, ids):
    """[(expert, token rows, their routing weights [n, 1])]: the host-side grouping, made once outside the timed loop."""
    groups = []
    for e in ids.unique().tolist():
        tok, slot = (ids == e).nonzero(as_tuple=True)
        groups.append((e, tok, weights[tok, slot].unsqueeze(1)))
    return groups


def torch_loop(x, w1, w2, groups, out):
    acc = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    inter = w2.shape[2]
    for e, tok, wgt in groups:
        h = F.linear(x.index_select(0, tok), w1[e])
        y = F.linear(F.silu(h[:, :inter]) * h[:, inter:], w2[e])
        acc.index_add_(0, tok, y.float() * wgt)
    return out.copy_(acc)


def w8_main(args, dev) -> None:
    cfg = PRESETS["qwen3-30b-a3b"]
    H, I, E, k = cfg.hidden_size, cfg.moe_intermediate_size, cfg.num_experts, cfg.num_experts_per_tok
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, std):
        return (torch.randn(shape, generator=g, device=dev) * std).bfloat16()

    sets = [(rnd(E, 2 * I, H, std=H ** -0.5), rnd(E, H, I, std=I ** -0.5)) for _ in range(args.layers)]
    qsets = [(ops.quantize_fp8_block128(w1), ops.quantize_fp8_block128(w2)) for w1, w2 in sets]
    ops.moe_w8_reserve(dev, E, H, I)
    rows = []
    for T in [int(t) for t in args.tokens.split(",")]:
        x, logits, out = rnd(T, H, std=1.0), rnd(T, E, std=1.0), torch.empty((T, H), dtype=torch.bfloat16, device=dev)
        replays = args.replays if T <= 256 else 4
        cases = [("bf16", sets, None), ("w8_rows", qsets, "rows")]
        if T >= 256:
            cases += [("w8_tall", qsets, "tall"), ("w8_tall_native", qsets, "tall_w8")]
        graphs, outs = {}, {}
        for name, ws, impl in cases:
            for w1, w2 in ws:
                ops.fused_moe(x, w1, w2, logits, k, cfg.norm_topk_prob, out=out, impl=impl)
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for i in range(replays):
                    ops.fused_moe(x, *ws[i % len(ws)], logits, k, cfg.norm_topk_prob, out=out, impl=impl)
            graphs[name].replay()
            outs[name] = out.clone()
        samples = {name: [] for name in graphs}
        for _ in range(args.rounds):  # in turn: every round sees the box in the same state for all three
            for name, graph in graphs.items():
                samples[name].append(timed_us(graph.replay, 1, replays))
        us = {name: statistics.median(v) for name, v in samples.items()}
        _, ids = ops.moe_route(logits, k, cfg.norm_topk_prob)
        touched = int(ids.unique().numel())
        w8_bytes = touched * (3 * I * H + 4 * 3 * I * H // (128 * 128)) + 2 * T * H * 2
        ref = outs["bf16"].float()
        native = dict(tall_native_equals_rows=bool(torch.equal(outs["w8_tall_native"], outs["w8_rows"])),
                      w8_tall_native_over_rows=round(us["w8_tall_native"] / us["w8_rows"], 3),
                      w8_tall_native_over_bf16=round(us["w8_tall_native"] / us["bf16"], 3)) if "w8_tall_native" in us else {}
        rows.append(dict(T=T, experts_touched=touched, **{f"{n}_us": round(v, 2) for n, v in us.items()},
                         w8_rows_over_bf16=round(us["w8_rows"] / us["bf16"], 3), **native, w8_algorithmic_bytes=w8_bytes,
                         w8_rows_fraction_of_8TBps=round(w8_bytes / (us["w8_rows"] * 1e-6) / PEAK_BYTES_PER_S, 4),
                         bf16_fraction_of_8TBps=round((touched * 3 * I * H * 2 + 2 * T * H * 2) / (us["bf16"] * 1e-6) / PEAK_BYTES_PER_S, 4),
                         max_rel_diff_vs_bf16=round((outs["w8_rows"].float() - ref).abs().max().item() / ref.abs().max().item(), 5)))
        print(json.dumps(rows[-1]), flush=True)
        del graphs
    result = dict(model=cfg.name, hidden=H, moe_intermediate=I, experts=E, topk=k, device=torch.cuda.get_device_name(0),
                  method=f"{args.replays} calls per captured graph (4 at T > 256) over {args.layers} weight sets; the bf16, FP8 rows, "
                         f"FP8 dequant + tall and FP8 native tall graphs replayed in turn, median of {args.rounds} rounds", rows=rows)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "moe_bench.json"))
    ap.add_argument("--tokens", default="1,16,64,256,512,1024,2048,4096,8192")
    ap.add_argument("--impl", default="both", choices=["both", "rows", "tall"])
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--w8", action="store_true", help="FP8 experts against bf16 (see the module docstring)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "moe_bench needs the GPU"
    dev = torch.device("cuda:0")
    if args.w8:
        return w8_main(args, dev)
    cfg = PRESETS["qwen3-30b-a3b"]
    H, I, E, k = cfg.hidden_size, cfg.moe_intermediate_size, cfg.num_experts, cfg.num_experts_per_tok
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, std):
        return (torch.randn(shape, generator=g, device=dev) * std).bfloat16()

    sets = [(rnd(E, 2 * I, H, std=H ** -0.5), rnd(E, H, I, std=I ** -0.5)) for _ in range(args.layers)]
    rows = []
    for T in [int(t) for t in args.tokens.split(",")]:
        x, logits, out = rnd(T, H, std=1.0), rnd(T, E, std=1.0), torch.empty((T, H), dtype=torch.bfloat16, device=dev)
        replays = args.replays if T <= 256 else 4
        auto = "tall" if T * k >= ops.MOE_TALL_MIN_PAIRS_PER_EXPERT * E else "rows"
        impls = [i for i in ("rows", "tall") if args.impl in (i, "both") and (i == "rows" or T >= 256 or args.impl == "tall")]
        us, outs = {}, {}
        for impl in impls:
            for w1, w2 in sets:  # warm-up: every shape and weight set of the timed window
                ops.fused_moe(x, w1, w2, logits, k, cfg.norm_topk_prob, out=out, impl=impl)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for i in range(replays):
                    ops.fused_moe(x, *sets[i % len(sets)], logits, k, cfg.norm_topk_prob, out=out, impl=impl)
            graph.replay()
            us[impl] = timed_us(graph.replay, args.rounds, replays)
            outs[impl] = out.clone()
            del graph
        hip_us, hip_out = us.get(auto, us[impls[0]]), outs.get(auto, outs[impls[0]])

        weights, ids = ops.moe_route(logits, k, cfg.norm_topk_prob)
        groups, state = expert_groups(weights, ids), {"i": 0}

        def loop():
            state["i"] += 1
            torch_loop(x, *sets[state["i"] % len(sets)], groups, out)

        loop()
        torch_us = timed_us(loop, args.rounds, 1)
        torch_loop(x, *sets[(replays - 1) % len(sets)], groups, out)
        diff = (hip_out.float() - out.float()).abs().max().item() / out.float().abs().max().item()
        touched = int(ids.unique().numel())
        nbytes = touched * 3 * I * H * 2 + 2 * T * H * 2
        flops = 6 * T * k * I * H
        both = dict(tall_over_rows=round(us["rows"] / us["tall"], 3), tall_equals_rows=bool(torch.equal(outs["rows"], outs["tall"])),
                    tall_fraction_of_bf16_peak=round(flops / (us["tall"] * 1e-6) / PEAK_BF16_FLOPS, 4)) if len(us) == 2 else {}
        rows.append(dict(T=T, experts_touched=touched, auto_impl=auto, **{f"{i}_us": round(v, 2) for i, v in us.items()}, **both,
                         hip_us=round(hip_us, 2), torch_loop_us=round(torch_us, 2),
                         speedup=round(torch_us / hip_us, 2), algorithmic_bytes=nbytes,
                         hip_bytes_per_s=round(nbytes / (hip_us * 1e-6)), torch_loop_bytes_per_s=round(nbytes / (torch_us * 1e-6)),
                         hip_fraction_of_8TBps=round(nbytes / (hip_us * 1e-6) / PEAK_BYTES_PER_S, 4),
                         torch_loop_fraction_of_8TBps=round(nbytes / (torch_us * 1e-6) / PEAK_BYTES_PER_S, 4),
                         max_rel_diff_vs_torch_loop=round(diff, 5)))
        print(json.dumps(rows[-1]), flush=True)
    result = dict(model=cfg.name, hidden=H, moe_intermediate=I, experts=E, topk=k, device=torch.cuda.get_device_name(0),
                  method=f"hip: {args.replays} calls per captured graph (4 at T > 256) over {args.layers} weight sets, median of "
                         f"{args.rounds} replays; torch loop: eager launches without host syncs (per-expert row lists "
                         f"made beforehand), median of {args.rounds} passes", rows=rows)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
