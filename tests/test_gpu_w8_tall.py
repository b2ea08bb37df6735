"""Tall-tile W8A16 GEMM (csrc/gemm_w8_tall.hip): the product against fp64 for every M class and knob set, strided views,
the routing of ops.linear by batch, graph replay of the k-sliced path, argument refusals.

Inputs, reference and tolerance are those of tests/test_gpu_w8.py: adversarial e4m3 bytes, scales jumping 2^+-3 between
blocks, x @ dequantised weight in fp64, the project's GEMM rule 2^-7 * max|ref|."""
import ctypes

import pytest
import torch

from mini_sglang_amd import ops
from test_gpu_w8 import _check, _weight, _x

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[(128, 128), (384, 640), (256, 2048)], ids=lambda p: "%dx%d" % p)
def weight(request, dev):
    N, K = request.param
    return _weight(dev, N, K, seed=N + K)


@pytest.mark.parametrize("M", [1, 33, 128, 129, 257, 300])
def test_w8_tall_gemm_vs_fp64(dev, weight, M):
    w, wd = weight
    K = w.shape[1]
    x = _x(dev, M, K, seed=M)
    ref = x.double().cpu() @ wd.t()
    out = ops.w8_tall_gemm(x, w)
    _check(out, ref)
    assert torch.equal(out, ops.w8_tall_gemm(x, w))  # same bits on every launch
    knobs = [(128, 1), (256, 1)] + ([(128, 2)] if K >= 256 else []) + ([(128, 5)] if K == 640 else [])
    for tm, k_slices in knobs:  # the knobs only reorder fp32 sums
        _check(ops.w8_tall_gemm(x, w, tm=tm, k_slices=k_slices), ref)


@pytest.mark.parametrize("k_slices", [1, 2])
def test_w8_tall_gemm_strided_views_keep_their_neighbours(dev, k_slices):
    w, wd = _weight(dev, 384, 640, seed=9)
    xs = torch.full((136, 640 + 64), 7.0, dtype=torch.bfloat16, device=dev)
    xs[:130, :640] = _x(dev, 130, 640, seed=2)
    big = torch.full((136, 384 + 128), -3.0, dtype=torch.bfloat16, device=dev)
    out = ops.w8_tall_gemm(xs[:130, :640], w, out=big[:130, :384], k_slices=k_slices)
    _check(out, xs[:130, :640].double().cpu() @ wd.t())
    assert bool((big[130:] == -3.0).all()) and bool((big[:, 384:] == -3.0).all())


def test_linear_routes_fp8_weights_by_batch(dev):
    w, wd = _weight(dev, 384, 640, seed=6)
    x = _x(dev, 300, 640, seed=7)
    lo, hi = x[: ops.W8_TALL_MIN_M - 1], x[: ops.W8_TALL_MIN_M]
    assert torch.equal(ops.linear(hi, w), ops.w8_tall_gemm(hi, w))
    assert torch.equal(ops.linear(lo, w), ops.w8_gemm(lo, w))
    top = x[: min(300, ops.W8_TALL_MAX_M)]  # the largest routed batch
    scratch = ops.w8_reserve(dev, 384 * 640)
    scratch.fill_(-3.0)
    _check(ops.linear(top, w), top.double().cpu() @ wd.t())
    assert bool((scratch == -3.0).all())  # served from the fp8 bytes: nothing was dequantised


def test_w8_tall_gemm_graph_replay_equals_eager(dev):
    w, _ = _weight(dev, 256, 2048, seed=4)
    x = _x(dev, 130, 2048, seed=5)
    assert ops.w8_tall_plan(130, 256, 2048)[1] > 1  # the k-sliced path: slabs + the reduce launch
    eager = ops.w8_tall_gemm(x, w)
    out = torch.empty_like(eager)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.w8_tall_gemm(x, w, out=out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ops.w8_tall_gemm(x, w, out=out)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("bad", [dict(dtype=1), dict(N=192), dict(K=192), dict(tm=64), dict(slices=0), dict(slices=3),
                                 dict(slices=2, ws_bytes=1024), dict(slices=2, wo=8), dict(ldx=260), dict(ldq=264),
                                 dict(ldo=130), dict(xo=8), dict(qo=8)], ids=lambda b: "-".join(b))
def test_w8_tall_entry_point_refuses_what_it_cannot_do(dev, bad):
    from mini_sglang_amd import _lib

    w, _ = _weight(dev, 128, 256, seed=8)
    x = _x(dev, 4, 256, seed=8)
    out = torch.full((4, 128), 5.0, dtype=torch.bfloat16, device=dev)
    ws, p = ops.gemm_workspace(dev), ctypes.c_void_p

    def call(M=4, N=128, K=256, ldx=256, ldq=256, ldo=128, dtype=_lib.BF16, tm=128, slices=1, ws_bytes=1 << 20, xo=0, qo=0, wo=0):
        return _lib.lib().msgl_w8_tall_gemm_nt(p(out.data_ptr()), p(x.data_ptr() + xo), p(w.q.data_ptr() + qo),
                                               p(w.scales.data_ptr()), M, N, K, ldx, ldq, ldo, dtype, tm, slices,
                                               p(ws.data_ptr() + wo), ws_bytes, None)

    assert call(**bad) == -1
    assert _lib.lib().msgl_last_error()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())  # nothing was launched
