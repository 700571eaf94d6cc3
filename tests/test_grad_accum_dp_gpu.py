"""Gradient accumulation under data parallelism: two gloo ranks on cuda:0 (tests/workers/accum_rank.py, launched as
tests/test_dp_gpu.py launches its workers: one fresh child per rank, ports of their own), each running K = 2 micro-batches of 1
impression per window with the bucketed all-reduce on the backward's hook.  The workers themselves assert that no collective is
pending inside a window and every bucket's is after its last backward (DistributedDataParallel's no_sync()).

Across ranks everything is bit-identical.  Against ONE rank at 4 impressions without accumulation (tests/workers/dp_rank.py, the
same weights and impressions) the averaged gradient and the parameters are held to tests/test_dp_gpu.py's bounds: it is the same
comparison with four summands instead of two."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_dp_gpu import _launch as launch_plain          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "workers", "accum_rank.py")


def _launch(tmp_path, world, dtype, B, windows, K, tag, port):
    out = str(tmp_path / (tag + "_rank%d.npz"))
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, WORKER, out, dtype, str(B), str(windows), str(K)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=900)[0] for p in procs]
    for p, lg in zip(procs, logs):
        assert p.returncode == 0, lg[-3000:]
    return [np.load(out % r) for r in range(world)]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_two_ranks_of_two_micro_batches_equal_one_rank_with_the_whole_batch(tmp_path, dtype):
    B, steps, K, lr = 4, 2, 2, 1e-4
    two = _launch(tmp_path, 2, dtype, B, steps, K, "a2", 29631 if dtype == "fp16" else 29633)
    one = launch_plain(tmp_path, 1, dtype, B, steps, "w1", 29632 if dtype == "fp16" else 29634)[0]
    # (1) both ranks hold the same summed gradients (both windows) and bit-identical parameters
    assert np.array_equal(two[0]["grads"], two[1]["grads"])
    assert np.array_equal(two[0]["params"], two[1]["params"])
    assert np.isfinite(two[0]["grads"]).all() and np.abs(two[0]["grads"]).max() > 0
    # (2) first window: the mean of the four one-impression gradients == the gradient of the 4-impression batch
    g2, g1 = two[0]["grads"][0].astype(np.float64), one["grads"][0].astype(np.float64)
    cut = int(one["head0"])
    for name, sl in (("encoder + pooling", slice(0, cut)), ("heads", slice(cut, None))):
        rel = np.linalg.norm(g2[sl] - g1[sl]) / np.linalg.norm(g1[sl])
        print("%s %s: rel. L2 difference of the averaged gradient %.2e" % (dtype, name, rel))
        assert rel < (1e-3 if dtype == "fp16" else 8e-3), (name, rel)
    # (3) parameters after two updates
    dp = np.abs(two[0]["params"].astype(np.float64) - one["params"].astype(np.float64))
    print("%s: |param diff| mean %.2e max %.2e (lr %.0e)" % (dtype, dp.mean(), dp.max(), lr))
    assert dp.mean() < 0.02 * lr and dp.max() <= 2.05 * lr * steps
