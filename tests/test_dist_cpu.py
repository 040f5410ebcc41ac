"""Distributed tier logic on CPU: gloo backend, world_size 2 (no GPU needed).
Verifies the redundant-BFS + round-robin-slice partition and the end-of-search
collectives reproduce sequential counts exactly."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


import pytest


def run_torchrun(cmd, env, tries=4):
    """torchrun --standalone can transiently fail its rendezvous bind when
    other tests' agents are tearing down; retry with a pause before
    declaring failure."""
    import time

    for attempt in range(tries):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env,
                           cwd=os.path.dirname(HERE))
        if r.returncode == 0:
            return r
        time.sleep(2 * (attempt + 1))
    return r


@pytest.mark.parametrize("world", [2, 3])
def test_dist_gloo(world):
    # world 3: uneven dynamic-queue claims (12 sub-slices over 3 ranks) and a
    # remainder-bearing round-robin partition
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    # CPU tensors need gloo; on a machine WITH a GPU init_dist would pick nccl
    env["GATS_DIST_BACKEND"] = "gloo"
    cmd = [
        sys.executable, "-m", "torch.distributed.run",
        "--nnodes=1", f"--nproc-per-node={world}",
        "--standalone", "--local-addr", "127.0.0.1",
        os.path.join(HERE, "helpers", "dist_check.py"),
    ]
    r = run_torchrun(cmd, env)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    assert "DIST_CHECK_OK" in r.stdout


@pytest.mark.parametrize("world", [2, 3])
def test_live_steal_gloo(world):
    # engine-pausing inter-rank stealing with a skewed partition: counts
    # exact, and at least one steal actually happened
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    # CPU tensors need gloo; on a machine WITH a GPU init_dist would pick nccl
    env["GATS_DIST_BACKEND"] = "gloo"
    cmd = [
        sys.executable, "-m", "torch.distributed.run",
        "--nnodes=1", f"--nproc-per-node={world}",
        "--standalone", "--local-addr", "127.0.0.1",
        os.path.join(HERE, "helpers", "dist_live_check.py"),
    ]
    r = run_torchrun(cmd, env)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    assert "LIVE_STEAL_OK" in r.stdout


def test_cli_dist_tier_cpu():
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env["GATS_DIST_ENGINE"] = "cpu"
    env["GATS_DIST_BACKEND"] = "gloo"
    cmd = [
        sys.executable, "-m", "torch.distributed.run",
        "--nnodes=1", "--nproc-per-node=2",
        "--standalone", "--local-addr", "127.0.0.1",
        os.path.join(HERE, "helpers", "cli_dist_check.py"),
    ]
    r = run_torchrun(cmd, env)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    out = f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    assert "CLI_DIST_OK" in r.stdout, out
    assert "Size of the explored tree: 35538" in r.stdout, out   # N=10 exact
    assert "Size of the explored tree: 2573652" in r.stdout, out  # ta014 lb1_d ub1
    assert "Optimal makespan: 1377 (not improved)" in r.stdout, out
