"""HIP kernel numerics vs the CPU oracle (the reference's C bound library is
the oracle's oracle — c_bound_simple.c / c_bound_johnson.c; our CPU versions
replicate it and feed the golden-count tests)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_step_oracle as orc  # noqa: E402
import py_bounds  # noqa: E402

pytestmark = pytest.mark.gpu


def frontier(core, N=12, target=2000):
    nodes, _, _ = core.nq_bfs_frontier(N, 1, target)
    return nodes


def test_nq_labels_match_cpu(gpu):
    for N in (8, 12, 17):
        nodes, _, _ = gpu.nq_bfs_frontier(N, 1, 3000)
        cpu = gpu.nq_cpu_labels(N, 1, nodes)
        dev = gpu.nq_gpu_labels(N, 1, nodes)
        assert cpu == dev


@pytest.mark.parametrize("inst", [2, 14, 21])  # 20x5, 20x10, 20x20
@pytest.mark.parametrize("lb", ["lb1", "lb1_d"])
def test_pfsp_bounds_match_cpu(gpu, inst, lb):
    nodes, _, _, best = gpu.pfsp_bfs_frontier(inst, lb, 1, 2000)
    cpu = gpu.pfsp_cpu_bounds(inst, lb, nodes, best)
    dev = gpu.pfsp_gpu_bounds(inst, lb, nodes, best)
    assert cpu == dev


@pytest.mark.parametrize("inst", [2, 14, 21])
def test_pfsp_lb2_bounds_match_cpu(gpu, inst):
    # lb2's early exit depends on `best`: compare with the same incumbent.
    nodes, _, _, best = gpu.pfsp_bfs_frontier(inst, "lb2", 1, 2000)
    cpu = gpu.pfsp_cpu_bounds(inst, "lb2", nodes, best)
    dev = gpu.pfsp_gpu_bounds(inst, "lb2", nodes, best)
    assert cpu == dev


# ---------------------------------------------------------------------------
# Deep nodes. BFS frontiers of ~2000 nodes stop at depth 2-4, so the tests
# above never reach lb1_child_bound's i == k skip late in the permutation,
# lb1d_setup with a long prefix and a nearly empty remainder, lb2's scheduled
# mask with 15+ bits, or nq_safe over a long prefix. The eval kernels are pure
# functions of the node, so seeded random nodes (random permutation, any
# depth) reach every level cheaply.
# ---------------------------------------------------------------------------
DEEP_SIZES = [1, 13, 64, 257]
HUGE = 10 ** 9


def _every_depth(make, rng, n, max_depth):
    """n random nodes; once n allows it, every depth 0..max_depth occurs."""
    if n <= max_depth:
        return make(rng, n)
    return b"".join(make(rng, 1, min_depth=i % (max_depth + 1), max_depth=i % (max_depth + 1))
                    for i in range(n))


@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("N", [4, 5, 19, 20])
def test_nq_labels_deep_random_nodes(gpu, N, g):
    rng = orc.rng(300 + N)
    for n in DEEP_SIZES:
        nodes = _every_depth(lambda r, c, **kw: orc.random_nq_nodes(r, c, N, **kw), rng, n, N)
        assert len(nodes) == n * 24
        assert gpu.nq_gpu_labels(N, g, nodes) == gpu.nq_cpu_labels(N, g, nodes), (N, g, n)


@pytest.mark.parametrize("inst", [2, 14, 21])
@pytest.mark.parametrize("lb", ["lb1", "lb1_d", "lb2"])
def test_pfsp_bounds_deep_random_nodes(gpu, inst, lb):
    # lb2's per-pair early exit: never exits (huge incumbent), exits in the
    # middle (optimum), exits at the first pair (1); same `best` on both sides
    opt = gpu.taillard_best_ub(inst)
    bests = (HUGE, opt, 1) if lb == "lb2" else (opt,)
    rng = orc.rng(inst * 10 + len(lb))
    for n in DEEP_SIZES:
        nodes = _every_depth(orc.random_pfsp_nodes, rng, n, 19)
        for best in bests:
            cpu = gpu.pfsp_cpu_bounds(inst, lb, nodes, best)
            dev = gpu.pfsp_gpu_bounds(inst, lb, nodes, best)
            assert cpu == dev, (inst, lb, n, best)


@pytest.mark.parametrize("inst,lb", [(14, "lb1"), (21, "lb1_d"), (2, "lb2")])
def test_deep_bounds_three_leg_chain(gpu, inst, lb):
    # HIP == C++ oracle == pure Python on ~40 deep nodes (depth 10..19)
    jobs, machines = gpu.taillard_nb_jobs(inst), gpu.taillard_nb_machines(inst)
    ptm = gpu.taillard_processing_times(inst)
    mt = py_bounds.py_min_tails(ptm, jobs, machines)
    nodes = orc.random_pfsp_nodes(orc.rng(40 + inst), 40, min_depth=10)
    for best in ((HUGE, gpu.taillard_best_ub(inst)) if lb == "lb2" else (HUGE,)):
        cpu = gpu.pfsp_cpu_bounds(inst, lb, nodes, best)
        dev = gpu.pfsp_gpu_bounds(inst, lb, nodes, best)
        for idx, (depth, limit1, prmu) in enumerate(py_bounds.nodes_of(nodes)):
            for k in range(limit1 + 1, jobs):
                child = prmu[:]
                child[depth], child[k] = child[k], child[depth]
                if lb == "lb1":
                    expect = py_bounds.py_lb1_bound(ptm, jobs, machines, child, limit1 + 1, mt)
                elif lb == "lb1_d":
                    expect = py_bounds.py_lb1d_child_bound(ptm, jobs, machines, prmu, limit1,
                                                           mt, prmu[k])
                else:
                    expect = py_bounds.py_lb2_bound(ptm, jobs, machines, child, limit1 + 1,
                                                    mt, best)
                assert cpu[idx * jobs + k] == expect, (idx, k, best)
                assert dev[idx * jobs + k] == expect, (idx, k, best)
