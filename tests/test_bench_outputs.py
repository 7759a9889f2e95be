"""bench.py --dump-outputs and the plain / --full split.

* dump_outputs writes float32 / float64 .npy files and cuts an array above its
  share of the 64 MB to a sample that is the same from call to call (CPU).
* On the GPU two plain runs with the same arguments dump bit-identical
  outputs, time exactly --steps steps and leave the --full blocks out of the
  result line.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_formats_and_fixed_sample(tmp_path):
    rng = np.random.default_rng(3)
    big = rng.standard_normal(6_000_000, dtype=np.float32)       # 24 MB > its 21.3 MB share
    arrays = {"draws": rng.standard_normal((5, 7)).astype(np.float32),
              "count": np.arange(5, dtype=np.int32),
              "big": big}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arrays, rank=0, world=1)
    bench.dump_outputs(str(b), arrays, rank=1, world=1)
    assert sorted(os.listdir(a)) == ["big.npy", "count.npy", "draws.npy"]
    assert sorted(os.listdir(b)) == ["big_rank1.npy", "count_rank1.npy", "draws_rank1.npy"]
    draws, count, cut = (np.load(a / f"{n}.npy") for n in ("draws", "count", "big"))
    assert draws.dtype == np.float32 and np.array_equal(draws, arrays["draws"])
    assert count.dtype == np.float64 and np.array_equal(count, np.arange(5.0))
    share = bench.DUMP_BYTES // 3
    assert cut.dtype == np.float32 and cut.nbytes <= share and cut.size == share // 4
    assert np.isin(cut, big).all()
    assert np.array_equal(cut, np.load(b / "big_rank1.npy"))
    total = sum(os.path.getsize(a / f) for f in os.listdir(a))
    assert total <= bench.DUMP_BYTES


def _bench(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args,
                       capture_output=True, text=True, timeout=170, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_runs_dump_identical_outputs(gpu, tmp_path):
    args = ["--gpus", "1", "--steps", "7", "--warmup", "3", "--shape", "small", "--chains", "32",
            "--clock-warm-ms", "0"]
    outs = []
    for name in ("a", "b"):
        d = tmp_path / name
        line = _bench(args + ["--dump-outputs", str(d)])
        assert line["steps"] == 7 and line["ms_per_step"] > 0 and line["full"] is False
        assert line["value"] == pytest.approx(32 * 20 * 7 / (line["ms_per_step"] * 7 / 1e3),
                                              rel=1e-6)
        for k in ("cpu_baseline", "ess_per_sec", "ess_timed", "ess_converged"):
            assert k not in line
        outs.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = outs
    assert sorted(a) == ["logp.npy", "n_accept.npy", "samples_last_step.npy", "step_size.npy"]
    assert a["samples_last_step.npy"].shape == (32, 10)       # small: 7 groups + mu, tau, sigma
    assert a["samples_last_step.npy"].dtype == np.float32
    assert np.isfinite(a["samples_last_step.npy"]).all()
    for f in a:
        assert a[f].dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a[f], b[f])
