"""head_dim 64 attention kernels (csrc/attn_d64.hip) beside the head_dim 128 defaults.

    python tools/attn_d64_bench.py [--out profiles/attn_d64_bench.json]

Decode: 256 requests, lengths uniform in [465, 1393] (mean ~929), page 256, 32 q / 8 kv heads at head_dim 64; the head_dim
128 default kernel on the same batch at HALF the lengths = the same K/V bytes.  Achieved bytes/s = K and V rows of every
token of every kv head (q, out and the partial sums are not counted) over the time of one msgl_attn_decode (partial + merge).
Prefill: one 2048-token chunk without cache hit, 32 / 8 heads at head_dim 64 beside 16 / 8 at head_dim 128 (the same
4 hq D S (S + 1) / 2 flops).  Method: `--calls` launches per captured graph rotating over `--pools` K/V pools (a pool is
larger than the Infinity Cache at the decode shape), device events around a replay, median of `--rounds`.  Outputs are checked
against oracle/ref_ops on a few requests before anything is timed.  No GPU: fails, nothing is estimated."""
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
from oracle import ref_ops  # noqa: E402


def timed_us(graph, rounds: int, per_call: int) -> float:
    samples = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b) * 1e3 / per_call)
    return statistics.median(samples)


def pools(n, slots, hkv, D, dev, g):
    return [(torch.randn((slots, hkv, D), generator=g, device=dev).bfloat16(),
             torch.randn((slots, hkv, D), generator=g, device=dev).bfloat16()) for _ in range(n)]


def paged_table(lens, page, dev, g):
    """Page-aligned allocation over permuted pages; returns (table [B, max_seq], slots used)."""
    pages_per = [(n + page - 1) // page for n in lens]
    perm = torch.randperm(sum(pages_per), generator=g, device=dev).to(torch.int32)
    table = torch.zeros((len(lens), max(pages_per) * page), dtype=torch.int32, device=dev)
    at = 0
    for b, npg in enumerate(pages_per):
        table[b, : npg * page] = (perm[at: at + npg, None] * page + torch.arange(page, dtype=torch.int32, device=dev)).flatten()
        at += npg
    return table, sum(pages_per) * page


def check(out, q, k, v, table, lens, pick):
    """Largest absolute error of the picked decode requests against the fp64 oracle."""
    ref = ref_ops.paged_attention_ref(q[pick].cpu(), k.cpu(), v.cpu(), table.cpu(), pick, [lens[b] for b in pick],
                                      [1] * len(pick), q.shape[-1] ** -0.5, double=True)
    return (out[pick].cpu().double() - ref).abs().max().item()


def decode_case(D, hq, hkv, lens, args, dev, g):
    B, page, cap = len(lens), 256, 4 * len(lens)
    table, slots = paged_table(lens, page, dev, g)
    kv = pools(args.pools, slots, hkv, D, dev, g)
    q = torch.randn((B, hq, D), generator=g, device=dev).bfloat16()
    out = torch.empty_like(q)
    seq = torch.tensor(lens, dtype=torch.int32, device=dev)
    plan = torch.zeros(ops.attn_decode_plan_words(B, cap), dtype=torch.int32, device=dev)
    ws = torch.empty(ops.attn_decode_workspace_bytes(cap, hq, D), dtype=torch.uint8, device=dev)
    ops.attn_decode_plan(plan, seq, B, B, cap, hq, hkv)

    def call(i):
        k, v = kv[i % len(kv)]
        ops.attn_decode(out, q, k, v, table, None, seq, plan, ws, B, B, cap, D ** -0.5, slot_run=page)

    for i in range(len(kv)):
        call(i)
    torch.cuda.synchronize()
    err = check(out, q, *kv[-1], table, lens, [0, 1, B - 1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(args.calls):
            call(i)
    graph.replay()
    us = timed_us(graph, args.rounds, args.calls)
    nbytes = 2 * sum(lens) * hkv * D * 2
    return dict(phase="decode", head_dim=D, q_heads=hq, kv_heads=hkv, requests=B, mean_context=round(sum(lens) / B, 1),
                page=page, us=round(us, 2), kv_bytes=nbytes, tbytes_per_s=round(nbytes / us * 1e-6, 3),
                max_abs_err_vs_fp64_oracle=err)


def prefill_case(D, hq, hkv, S, args, dev, g):
    table, slots = paged_table([S], 16, dev, g)
    kv = pools(2, slots, hkv, D, dev, g)
    q = torch.randn((S, hq, D), generator=g, device=dev).bfloat16()
    out = torch.empty_like(q)
    qt = ops.prefill_q_tile()
    tiles = (S + qt - 1) // qt
    cu_q = torch.tensor([0, S], dtype=torch.int32, device=dev)
    tile_cu = torch.tensor([0, tiles], dtype=torch.int32, device=dev)
    seq = torch.tensor([S], dtype=torch.int32, device=dev)
    order = torch.arange(tiles - 1, -1, -1, dtype=torch.int32, device=dev)  # heaviest q tiles first

    def call(i):
        k, v = kv[i % 2]
        ops.attn_prefill(out, q, k, v, table, None, seq, cu_q, tile_cu, 1, tiles, D ** -0.5, tile_order=order)

    call(0), call(1)
    torch.cuda.synchronize()
    ref = ref_ops.paged_attention_ref(q[-64:].cpu(), kv[1][0].cpu(), kv[1][1].cpu(), table.cpu(), [0], [S], [64], D ** -0.5,
                                      double=True)
    err = (out[-64:].cpu().double() - ref).abs().max().item()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(args.calls):
            call(i)
    graph.replay()
    us = timed_us(graph, args.rounds, args.calls)
    flops = 4 * hq * D * S * (S + 1) // 2
    return dict(phase="prefill", head_dim=D, q_heads=hq, kv_heads=hkv, chunk=S, us=round(us, 2), flops=flops,
                tflops_per_s=round(flops / us * 1e-6, 2), max_abs_err_vs_fp64_oracle=err)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attn_d64_bench.json"))
    ap.add_argument("--pools", type=int, default=2)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attn_d64_bench needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lens = torch.randint(465, 1394, (256,), generator=g, device=dev).tolist()
    rows = [decode_case(64, 32, 8, lens, args, dev, g), decode_case(128, 32, 8, [(n + 1) // 2 for n in lens], args, dev, g),
            prefill_case(64, 32, 8, 2048, args, dev, g), prefill_case(128, 16, 8, 2048, args, dev, g)]
    for r in rows:
        print(json.dumps(r), flush=True)
    result = dict(device=torch.cuda.get_device_name(0), command="python tools/attn_d64_bench.py",
                  method=f"{args.calls} calls per captured graph over {args.pools} K/V pools, device events around a replay, "
                         f"median of {args.rounds}; clocks and power state as the machine had them (not set by the tool)",
                  rows=rows)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
