"""bench.py's command line on the GPU: a plain run prints the headline line only and --dump-outputs
writes what the last timed step computed (one small run, shared by the tests)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

H, W, ITERS, STEPS = 128, 192, 4, 2
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "lookup_b1", "lookup_b8", "iteration", "update_gemm", "dominant_kernel",
             "drop_in_forward", "fp32_exact", "cpu_baseline"}


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RAFT_BENCH_REHEARSE_1GPU"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-u", os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--height", str(H), "--width", str(W), "--iters", str(ITERS),
                        "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0]), d


def test_plain_run_prints_headline_only(plain_run):
    out, _ = plain_run
    assert HEADLINE <= set(out) and not FULL_ONLY & set(out)
    assert out["steps"] == STEPS and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(1e3 / out["ms_per_step"], rel=1e-2)


def test_dump_outputs_are_the_last_steps_flow(plain_run):
    """The dumped arrays equal RAFT.forward() on the pool pair of the last timed step (pair
    (STEPS - 1) % 4, seed 1 + k, as bench.py builds its pool): same kernels, same inputs."""
    import argparse
    from raft_optical_flow_amd import RAFT, InputPadder
    from raft_optical_flow_amd.init import seeded_images, seeded_state_dict
    _, d = plain_run
    low, up = np.load(d / "flow_low.npy"), np.load(d / "flow_up.npy")
    assert low.dtype == np.float32 and low.shape == (1, 2, H // 8, W // 8)
    assert up.dtype == np.float32 and up.shape == (1, 2, H, W)
    m = RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False))
    m.load_state_dict(seeded_state_dict(m, 0))
    m.cuda().eval()
    i1, i2 = seeded_images(1, H, W, seed=1 + (STEPS - 1) % 4)
    i1, i2 = InputPadder(i1.shape).pad(i1.cuda(), i2.cuda())
    with torch.no_grad():
        rlow, rup = m(i1, i2, iters=ITERS, test_mode=True)
    assert np.array_equal(low, rlow.cpu().numpy()) and np.array_equal(up, rup.cpu().numpy())
