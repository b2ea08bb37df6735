"""The W8A16 kernels (block-scaled e4m3 weights) against today's ops.linear on bf16 weights, at the four Qwen3-14B
projection shapes and M in {1, 8, 16, 32, 64, 128, 256, 512, 2048}.  Columns: `bf16`; `w8` = the route before the tall-tile
kernel existed (msgl_w8_gemm_nt up to 256 rows, msgl_w8_dequant + the 16-bit ops.linear above); `tall` =
msgl_w8_tall_gemm_nt (csrc/gemm_w8_tall.hip) with ops.w8_tall_plan.

    python tools/w8_bench.py [--out profiles/w8_bench.json] [--layers 6] [--replays 24] [--rounds 9]
    python tools/w8_bench.py --a8 [--out profiles/w8a8_bench.json] [--batches 64,128,256,512,2048]

`--a8`: the W8A8 route (csrc/gemm_w8a8.hip) instead: columns `bf16`; `today` = what ops.linear does for an Fp8Weight without
act_quant at that batch; `a8` = ops.w8a8_linear, the quantiser and the FP8-MFMA GEMM together (the model pays for both).

Same process, same box, alternating: per (shape, M) the bf16 side first runs the project's plan search for the shape
(model.tune_gemms' search: library solutions and the hand-written 16-bit kernels), then both sides are captured as
`--replays` calls per graph rotating over `--layers` weight sets (so weights come from HBM, not the Infinity Cache), and
the three graphs are replayed in turn `--rounds` times; medians of the per-call time.  Algorithmic bytes = the weight (and
scale) bytes plus x in and out.  No GPU: fails, nothing is estimated."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mini_sglang_amd import gemm_plan, ops  # noqa: E402
from mini_sglang_amd.model import PRESETS  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def replay_us(graph, per_call: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / per_call


def capture(fn, weights, replays: int):
    for w in weights:  # warm-up: every weight set of the timed window
        fn(w)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(replays):
            fn(weights[i % len(weights)])
    graph.replay()
    torch.cuda.synchronize()
    return graph


def a8_row(args, name, M, N, K, x, out, bf16, fp8, rep) -> dict:
    graphs = {"bf16": capture(lambda w: ops.linear(x, w, out=out), bf16, args.replays),
              "today": capture(lambda w: ops.linear(x, w, out=out), fp8, args.replays),
              "a8": capture(lambda w: ops.w8a8_linear(x, w, out=out), fp8, args.replays)}
    samples = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k, gr in graphs.items():
            samples[k].append(replay_us(gr, args.replays))
    us = {k: statistics.median(v) for k, v in samples.items()}
    ref = x.float() @ fp8[(args.replays - 1) % args.layers].dequantize().t()
    rel = ((out.float() - ref).abs().max() / ref.abs().max()).item()  # `out` holds the a8 graph's last call
    return dict(name=name, M=M, N=N, K=K, bf16_us=round(us["bf16"], 2), today_us=round(us["today"], 2), a8_us=round(us["a8"], 2),
                a8_over_today=round(us["a8"] / us["today"], 3), a8_over_bf16=round(us["a8"] / us["bf16"], 3),
                a8_tflops=round(2.0 * M * N * K / (us["a8"] * 1e-6) / 1e12, 1),
                today_route="w8_gemm" if M < ops.W8_TALL_MIN_M else "w8_tall" if M <= ops.W8_TALL_MAX_M else "dequant + linear",
                a8_plan=list(ops.w8a8_plan(M, N, K)), bf16_kernel=rep["kernel"][:120],
                spread_us={k: [round(min(v), 2), round(max(v), 2)] for k, v in samples.items()},
                a8_max_rel_err_vs_unquantised_fp32=round(rel, 5))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "w8_bench.json"))
    ap.add_argument("--batches", default="1,8,16,32,64,128,256,512,2048")
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--replays", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--a8", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "w8_bench needs the GPU"
    dev = torch.device("cuda:0")
    cfg = PRESETS["qwen3-14b"]
    H, D, I = cfg.hidden_size, cfg.head_dim, cfg.intermediate_size
    qd, kvd = cfg.num_qo_heads * D, cfg.num_kv_heads * D
    shapes = [("qkv", qd + 2 * kvd, H), ("o", H, qd), ("gate_up", 2 * I, H), ("down", H, I)]
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for name, N, K in shapes:
        bf16 = [(torch.randn((N, K), generator=g, device=dev) * K ** -0.5).bfloat16() for _ in range(args.layers)]
        fp8 = [ops.quantize_fp8_block128(w) for w in bf16]
        for M in [int(m) for m in args.batches.split(",")]:
            x = torch.randn((M, K), generator=g, device=dev).bfloat16()
            out = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
            rep = gemm_plan.tune_projection_gemms([(name, bf16, K)], [M], "heuristic", torch.bfloat16, dev)[0]
            if args.a8:
                rows.append(a8_row(args, name, M, N, K, x, out, bf16, fp8, rep))
                print(json.dumps(rows[-1]), flush=True)
                continue
            scratch = ops.w8_reserve(dev, N * K)[: N * K].view(N, K)
            old = (lambda w: ops.w8_gemm(x, w, out=out)) if M <= ops.W8_MAX_M else (
                lambda w: ops.linear(x, ops.w8_dequant(w, scratch), out=out))
            graphs = {"bf16": capture(lambda w: ops.linear(x, w, out=out), bf16, args.replays),
                      "w8": capture(old, fp8, args.replays),
                      "tall": capture(lambda w: ops.w8_tall_gemm(x, w, out=out), fp8, args.replays)}
            samples = {k: [] for k in graphs}
            for _ in range(args.rounds):
                for k, gr in graphs.items():
                    samples[k].append(replay_us(gr, args.replays))
            us = {k: statistics.median(v) for k, v in samples.items()}
            last = (args.replays - 1) % args.layers
            ref = x.float() @ fp8[last].dequantize().t()
            rel = ((out.float() - ref).abs().max() / ref.abs().max()).item()  # `out` holds the tall graph's last call
            nbytes = {"bf16": 2 * N * K, "w8": fp8[0].nbytes()}
            io = 2 * M * (N + K)
            rows.append(dict(name=name, M=M, N=N, K=K, bf16_us=round(us["bf16"], 2), w8_us=round(us["w8"], 2),
                             tall_us=round(us["tall"], 2), w8_speedup=round(us["bf16"] / us["w8"], 3),
                             tall_speedup=round(us["bf16"] / us["tall"], 3), tall_over_w8=round(us["tall"] / us["w8"], 3),
                             bf16_kernel=rep["kernel"][:120],
                             w8_plan=list(ops.w8_plan(M, N, K)) if M <= ops.W8_MAX_M else "dequant + linear",
                             tall_plan=list(ops.w8_tall_plan(M, N, K)),
                             bf16_bytes_per_s=round((nbytes["bf16"] + io) / (us["bf16"] * 1e-6)),
                             w8_bytes_per_s=round((nbytes["w8"] + io) / (us["w8"] * 1e-6)),
                             w8_fraction_of_8TBps=round((nbytes["w8"] + io) / (us["w8"] * 1e-6) / PEAK_BYTES_PER_S, 4),
                             w8_spread_us=[round(min(samples["w8"]), 2), round(max(samples["w8"]), 2)],
                             tall_spread_us=[round(min(samples["tall"]), 2), round(max(samples["tall"]), 2)],
                             bf16_spread_us=[round(min(samples["bf16"]), 2), round(max(samples["bf16"]), 2)],
                             tall_max_rel_err_vs_fp32=round(rel, 5)))
            print(json.dumps(rows[-1]), flush=True)
            del graphs
        del bf16, fp8
    result = dict(model=cfg.name, device=torch.cuda.get_device_name(0), command="python tools/w8_bench.py" + " --a8" * args.a8,
                  method=f"{args.replays} calls per captured graph over {args.layers} weight sets, the "
                         f"{'bf16, today and a8' if args.a8 else 'bf16, w8 and tall'} graphs "
                         f"replayed in turn, median of {args.rounds} replays each; bf16 = ops.linear after the project's plan "
                         f"search for the shape", rows=rows)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
