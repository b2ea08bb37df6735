"""Records the projection-GEMM kernel choice of bench.py's decode step as data -> bench_gemm_plans.json.

    python tools/bench_plans.py [--model qwen3-14b] [--batch 256] [--page-size 256] [--out bench_gemm_plans.json]

The engine's kernel search is timed (gemm_plan.tune_projection_gemms + the re-ranking inside the captured step), so two
processes may settle on different kernels where two candidates are within noise -- a different split of K, a reordered
sum, other last bits.  A plain `bench.py` run therefore installs the plans recorded here (ops.import_gemm_plans) instead
of searching: the same kernels every run, the same outputs for the same arguments.  Re-run this after a change to the
projection kernels or to the library, look at what it picked (`kernels`), and commit the file.  One entry per
"<model> tp1 B<batch>"; the other entries of the file are kept.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="qwen3-14b")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--page-size", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "bench_gemm_plans.json"))
    args = ap.parse_args()

    from mini_sglang_amd import ops
    from mini_sglang_amd.engine import Engine, EngineConfig
    from mini_sglang_amd.model import PRESETS

    device = torch.device("cuda:0")
    B = args.batch
    # bench.py's engine: one graph at the full batch, every library solution searched, finalists re-ranked in the graph
    engine = Engine(EngineConfig(model=PRESETS[args.model], max_running_req=B, cuda_graph_bs=[B], page_size=args.page_size,
                                 max_seq_len_override=4096, memory_ratio=0.9, gemm_tune="full"), device)
    code = ops._dt(torch.empty(0, dtype=torch.bfloat16))
    report = [r for r in engine.gemm_report if r["M"] == B]
    # the library's solution only where the library's kernel is the one that runs (a hand-written plan takes precedence);
    # out leading dimension N, and N / 2 for a projection whose launch ends in SiLU.mul
    to_library = {r["name"] for r in engine.refine_report if r["chosen"].startswith("library")}
    shapes = [(B, r["N"], r["K"], r["K"], r["K"], ldo, code) for r in report
              if not r.get("skinny_used") or r["name"] in to_library for ldo in (r["N"], r["N"] // 2)]
    entry = dict(ops.export_gemm_plans(shapes),
                 kernels={r["name"]: f"{r['kernel'][:90]} ({r['best_us']:.1f} us back to back)" for r in report},
                 refined_in_graph={r["name"]: r["chosen"] for r in engine.refine_report},
                 device=torch.cuda.get_device_name(0))
    engine.shutdown()
    out = Path(args.out)
    plans = json.loads(out.read_text()) if out.exists() else {}
    plans[f"{args.model} tp1 B{B}"] = entry
    out.write_text(json.dumps(plans, indent=1, sort_keys=True) + "\n")
    print(json.dumps(entry["kernels"], indent=1))


if __name__ == "__main__":
    main()
