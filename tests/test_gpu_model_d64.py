"""End to end at head_dim 64: the `tiny-d64` preset (Llama-shaped, 8 q / 2 kv heads of 64) through the engine, prefill and
graph-replayed decode on the csrc/attn_d64.hip kernels, teacher-forced against the CPU oracle exactly as
test_gpu_model.py does for the head_dim 128 presets (its checks are imported, not copied)."""
import pytest

import test_gpu_model as tm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("page_size", [1, 16])
def test_tiny_d64_teacher_forced_parity_vs_cpu_oracle(dev, page_size):
    """Per-forward logits vs oracle/ref_model.forward bounded by the bf16 floors of the same run (oracle/torch_bf16.py on
    the GPU, its fp32-accumulating form on the CPU, parity_stats.assert_not_above_bf16_floor); KV pool vs the oracle's."""
    tm.test_teacher_forced_parity_vs_cpu_oracle(dev, "tiny-d64", page_size)


@pytest.mark.parametrize("page_size", [1, 16])
def test_tiny_d64_graph_replay_matches_eager(dev, page_size):
    ps = tm.prompts(5)
    ids = []
    for graphs in (True, False):
        eng = tm.make_engine(dev, "tiny-d64", graphs=graphs, page_size=page_size)
        ids.append(tm.run(eng, ps, 6)[0])
        eng.shutdown()
    assert ids[0] == ids[1] and all(len(i) == 6 for i in ids[0])
