"""The driver launches `bench.py` via torchrun at round end; this covers that
exact invocation on CPU (GATS_BENCH_CPU=1 + gloo) so the rendezvous, dynamic
slicing, MAX-over-ranks reduction and the one-line JSON contract are CI-tested
without a GPU."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def run_bench(nproc, extra):
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env["GATS_BENCH_CPU"] = "1"
    env["GATS_DIST_BACKEND"] = "gloo"
    cmd = [sys.executable, "-m", "torch.distributed.run",
           "--nnodes=1", f"--nproc-per-node={nproc}",
           "--standalone", "--local-addr", "127.0.0.1",
           os.path.join(ROOT, "bench.py"), "--gpus", str(nproc)] + extra
    import time
    for attempt in range(4):  # --standalone rendezvous can transiently fail
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env,
                           cwd=ROOT)
        if r.returncode == 0:
            break
        time.sleep(2 * (attempt + 1))
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # exactly ONE JSON line, from rank 0
    return json.loads(lines[0])


def run_bench_plain(extra):
    """bench.py as a plain single process (no torchrun), CPU evaluator."""
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env["GATS_BENCH_CPU"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra,
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def load_dump(path):
    import numpy as np

    out = {}
    for f in sorted(os.listdir(path)):
        assert f.endswith(".npy"), f
        a = np.load(os.path.join(path, f))
        assert a.dtype == np.float64 and a.shape == (1,), (f, a.dtype, a.shape)
        out[f[:-4]] = float(a[0])
    return out


def test_bench_dump_outputs_nqueens(tmp_path):
    # --dump-outputs writes what the last timed step returned; --full is
    # accepted and leaves the result line's contract untouched
    d = tmp_path / "dump"
    out = run_bench_plain(["--steps", "2", "--warmup", "1", "--problem", "nqueens",
                           "--N", "10", "--full", "--dump-outputs", str(d)])
    assert out["steps"] == 2
    assert out["metric"] == "Mnodes_per_sec"
    assert out["dtype"] == "int32"
    assert out["ms_per_step"] > 0
    assert load_dump(d) == {"tree": 35538.0, "sol": 724.0}


def test_bench_dump_outputs_headline(tmp_path):
    # headline step: both searches' counts and the proven PFSP optimum
    # (small stand-ins: N=10 + ta002 lb2, frozen in test_pfsp_seq.py)
    d = tmp_path / "dump"
    run_bench_plain(["--steps", "1", "--warmup", "0", "--N", "10",
                     "--inst", "2", "--lb", "lb2", "--dump-outputs", str(d)])
    assert load_dump(d) == {"nqueens_tree": 35538.0, "nqueens_sol": 724.0,
                            "pfsp_tree": 7.0, "pfsp_sol": 0.0, "pfsp_optimum": 1359.0}


@pytest.mark.gpu
def test_bench_dump_outputs_gpu(gpu, tmp_path):
    # the real timed path (devpool N-Queens + device-rooted PFSP): dumped
    # counts equal the sequential oracle's (test_nqueens_seq.py N=12,
    # test_pfsp_seq.py ta014 lb2)
    d = tmp_path / "dump"
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "GATS_BENCH_CPU"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "2", "--warmup", "1", "--N", "12", "--inst", "14",
                        "--lb", "lb2", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert out["explored_tree_per_step"] == 856188 + 144639
    assert load_dump(d) == {"nqueens_tree": 856188.0, "nqueens_sol": 14200.0,
                            "pfsp_tree": 144639.0, "pfsp_sol": 0.0,
                            "pfsp_optimum": 1377.0}


def test_bench_json_contract_world2():
    out = run_bench(2, ["--steps", "2", "--warmup", "1", "--N", "10",
                        "--problem", "nqueens"])
    assert out["metric"] == "Mnodes_per_sec"
    assert out["n_gpus"] == 2
    assert out["steps"] == 2
    assert out["warmup"] == 1
    assert out["unit"] == "Mnodes/s"
    assert out["higher_is_better"] is True
    assert out["scaling"] == "strong"
    assert out["value"] > 0
    assert out["ms_per_step"] > 0
    assert out["config"]["model"] == "nqueens-N10"
    # N=10 full tree: counts must equal the sequential search exactly
    assert out["explored_tree_per_step"] == 35538


def test_bench_json_contract_world1_pfsp():
    out = run_bench(1, ["--steps", "1", "--warmup", "0", "--problem", "pfsp",
                        "--inst", "14", "--lb", "lb1_d"])
    assert out["n_gpus"] == 1
    assert out["config"]["model"] == "pfsp-ta014-lb1_d"
    assert out["explored_tree_per_step"] == 2573652


def test_bench_world8_dry_run():
    # the driver's SCALE run launches bench.py at --nproc-per-node 8; dry-run
    # that exact world size on CPU so the rendezvous, 8-way slicing and
    # reductions cannot fail on plumbing when a real 8-GPU node appears
    out = run_bench(8, ["--steps", "1", "--warmup", "0", "--N", "11",
                        "--inst", "14", "--lb", "lb1_d"])
    assert out["n_gpus"] == 8
    assert out["config"]["nqueens_tree_per_step"] == 166925
    assert out["config"]["pfsp_tree_per_step"] == 2573652


def test_bench_headline_combines_both_configs():
    # default --problem headline runs BOTH BASELINE.json configs per step
    # (small stand-ins here: N=10 + ta014 lb1_d)
    out = run_bench(1, ["--steps", "1", "--warmup", "0", "--N", "10",
                        "--inst", "14", "--lb", "lb1_d"])
    assert out["config"]["model"] == "nqueens-N10+pfsp-ta014-lb1_d"
    assert out["config"]["nqueens_tree_per_step"] == 35538
    assert out["config"]["pfsp_tree_per_step"] == 2573652
    assert out["explored_tree_per_step"] == 35538 + 2573652
