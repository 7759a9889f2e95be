"""The multi-rank product path on one GPU: two ranks share the
box's GPU over the gloo backend (a rehearsal of the RCCL path the driver runs
on 8 GPUs: same sharding, same chain-offset RNG contract, same collectives on
host copies).

* Two spawned ranks run the product sampler (HIP kernels) on their shards of
  the chains; the samples gathered to rank 0 are bit-identical to one process
  running every chain (draws are keyed by the global chain id), for HMC on the
  lane-resident kernel and for NUTS.
* bench.py under torchrun with two and eight ranks prints one line whose value
  aggregates every rank (64 chains each), with the diagnostics' all-reduce and the
  sample gather exercised (the small hierarchical shape: one slice, so the two
  processes' kernels need no cross-workgroup co-residency on the shared GPU).
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import workloads as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(algo, C, offset):
    import mlx_mcmc_amd as m

    lp, init = W.hierarchical(W.ns_product(), *W.SHAPES["small"])
    kw = dict(num_samples=40, num_warmup=40, key=m.random.key(6), num_chains=C,
              chain_offset=offset, progress=False, keep_on_device=True, return_info=True)
    if algo == "hmc":
        _, _, info = m.hmc(lp, init, step_size=0.01, num_leapfrog_steps=10, **kw)
    else:
        _, _, info = m.nuts(lp, init, step_size=0.05, **kw)
    return info.device_samples.contiguous()


def _worker(rank, world, port, algo, C, q):
    import torch
    import torch.distributed as dist

    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import __graft_entry__ as ge

    ge._ensure_pkg()
    from mlx_mcmc_amd.distributed import gather_to_root, shard

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        off, cnt = shard(C, world, rank)
        mine = _run(algo, cnt, off)
        allc = gather_to_root(mine)
        if rank == 0:
            q.put(allc.cpu().numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("algo", ["hmc", "nuts"])
def test_two_ranks_on_one_gpu_match_one_process(gpu, algo):
    C, world = 12, 2
    ref = _run(algo, C, 0).cpu().numpy()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, algo, C, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("world,workload", [(2, "hmc"), (8, "hmc"), (2, "nuts")])
def test_bench_ranks_gloo(gpu, world, workload):
    """world 8: the rank arithmetic of BASELINE configs[3] (8 ranks, chains
    sharded per rank) on one shared GPU, 64 chains per rank; nuts: the
    configs[4] line's multi-rank path (leaves summed over ranks)."""
    env = dict(os.environ, MC_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "20", "--warmup", "5",
           "--chains", "64", "--full", "--no-cpu-baseline", "--clock-warm-ms", "0"]
    cmd += ["--workload", "nuts"] if workload == "nuts" else [
        "--shape", "small", "--gather", "--ess-draws", "400", "--ess-warmup", "100"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=170, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    C = 64 * world
    assert out["n_gpus"] == world and out["config"]["total_chains"] == C
    assert out["value"] > 0
    if workload == "nuts":
        # leaves of every rank's chains over the max-over-ranks time
        assert out["value"] == pytest.approx(out["leaves"] / (out["ms_per_step"] * 20 / 1e3),
                                             rel=1e-6)
        assert out["leaves"] >= C * 20
    else:
        assert "gather_ms" in out
        assert out["value"] == pytest.approx(C * 20 * 20 / (out["ms_per_step"] * 20 / 1e3),
                                             rel=1e-6)


def _bench_line(world, chains, extra):
    env = dict(os.environ, MC_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--chains", str(chains),
           "--full", "--no-cpu-baseline", "--clock-warm-ms", "0"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=170, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_ess_two_ranks_equal_one_rank(gpu):
    """The ESS/s half of the metric on the multi-rank line (VERDICT r3
    "Next round" 3): two ranks of 32 chains each report the converged-ESS
    block (ESS summed over every rank's chains, split R-hat over all of them,
    all-reduced moment blocks) and the timed-draw block equal to one rank
    running the same 64 global chains, up to the f64 summation order."""
    extra = ["--shape", "small", "--steps", "150", "--warmup", "20",
             "--ess-draws", "400", "--ess-warmup", "100"]
    two = _bench_line(2, 32, extra)
    one = _bench_line(1, 64, extra)
    for out in (one, two):
        assert out["config"]["total_chains"] == 64
        assert "ess_converged" in out and "ess_timed" in out
    a, b = one["ess_converged"], two["ess_converged"]
    assert a["chains"] == b["chains"] == 64
    assert a["accept_rate"] == pytest.approx(b["accept_rate"], rel=1e-12)
    for k in ("max", "median", "mean"):
        if k in a["rhat"]:
            assert a["rhat"][k] == pytest.approx(b["rhat"][k], rel=1e-9), k
    assert (a["ess_per_sec"] is None) == (b["ess_per_sec"] is None)
    if a["ess_per_sec"] is not None:
        for k in ("min", "median", "total"):
            assert a["ess_sum"][k] == pytest.approx(b["ess_sum"][k], rel=1e-9), k
        assert b["ess_per_sec"]["min"] > 0
    ta, tb = one["ess_timed"], two["ess_timed"]
    assert ta["chains_used"] == tb["chains_used"]
    assert ta["frozen_chains"] == tb["frozen_chains"]
    if "rhat" in ta:
        assert ta["rhat"]["max"] == pytest.approx(tb["rhat"]["max"], rel=1e-9)
    assert (one["ess_per_sec"] is None) == (two["ess_per_sec"] is None)
    print("ESS converged (1 rank / 2 ranks):", a.get("ess_sum"), b.get("ess_sum"))


def test_bench_spawns_ranks_itself(gpu):
    """The driver's command shape without a launcher (VERDICT r5 "Next round"
    1): `bench.py --gpus 2` spawns its two ranks itself (here sharing the one
    GPU over gloo) and prints one line whose value sums both ranks' chains;
    the large program at 64 chains per rank, as test_bench_large_two_ranks_gloo."""
    env = dict(os.environ, MC_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20",
           "--warmup", "5", "--chains", "64", "--full", "--no-cpu-baseline",
           "--clock-warm-ms", "0",
           "--ess-draws", "200", "--ess-warmup", "50"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=170, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["total_chains"] == 128
    assert out["value"] == pytest.approx(128 * 20 * 20 / (out["ms_per_step"] * 20 / 1e3),
                                         rel=1e-6)
    assert out["ess_converged"]["chains"] == 128
    print("bench.py --gpus 2 (spawned ranks, one GPU):", out["value"] / 1e6, "M steps/s")


def _run_large(C, offset):
    import mlx_mcmc_amd as m

    lp, init = W.hierarchical(W.ns_product(), *W.SHAPES["large"])
    _, _, info = m.hmc(lp, init, num_samples=6, num_warmup=6, step_size=2e-3,
                       num_leapfrog_steps=20, key=m.random.key(0), num_chains=C,
                       chain_offset=offset, progress=False, keep_on_device=True,
                       return_info=True)
    assert info.extra["kernel"] == "lanes"
    return info.device_samples.cpu().numpy(), info.step_size


@pytest.mark.parametrize("rank", [1, 7])
def test_large_shape_rank_shard_bit_identical(gpu, rank):
    """BASELINE configs[3]'s per-rank work (VERDICT r2 "Next round" 6): rank
    r's 256 chains of the 1000-parameter model at chain_offset = 256 r, on
    the bench kernel, give draws bit-identical to the same global chains
    inside a larger 512-chain run (two launches of 256 chains on this GPU)."""
    off = 256 * rank
    mine, eps_mine = _run_large(256, off)
    big, eps_big = _run_large(512, off - 256)
    np.testing.assert_array_equal(mine, big[256:])
    np.testing.assert_array_equal(eps_mine, eps_big[256:])


def test_bench_large_two_ranks_gloo(gpu):
    """Two ranks of the large, sliced program share the one GPU: each launch
    needs its 4 chain blocks x 16 slices co-resident, 64 of the 256 CUs, so
    both grids fit side by side and the run must complete with one aggregate
    line (samples gathered, ESS over both ranks' chains).  An exchange
    timeout here is a failure."""
    out = _bench_line(2, 64, ["--steps", "20", "--warmup", "5", "--shape", "large",
                              "--gather", "--ess-draws", "200", "--ess-warmup", "50"])
    assert out["n_gpus"] == 2 and out["config"]["total_chains"] == 128
    assert "gather_ms" in out and out["value"] > 0
    assert out["ess_converged"]["chains"] == 128
    print("two ranks on one GPU:", out["value"] / 1e6, "M steps/s")
