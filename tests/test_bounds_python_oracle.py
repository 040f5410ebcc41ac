"""Third-party check of the C++ bound oracle: an independent pure-Python
implementation of lb1/lb2 (written directly from the math in
c_bound_simple.c / c_bound_johnson.c) must agree with gats_amd._core on
random frontier nodes. The HIP kernels are in turn compared bit-for-bit
against the C++ oracle (tests/test_gpu_kernels.py), closing the chain."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from py_bounds import (nodes_of, py_lb1_bound, py_lb1d_child_bound,  # noqa: E402
                       py_lb2_bound, py_min_tails)


def test_lb1_vs_python(core):
    inst = 14
    jobs, machines = core.taillard_nb_jobs(inst), core.taillard_nb_machines(inst)
    ptm = core.taillard_processing_times(inst)
    mt = py_min_tails(ptm, jobs, machines)
    nodes, _, _, best = core.pfsp_bfs_frontier(inst, "lb1", 1, 512)
    cpp = core.pfsp_cpu_bounds(inst, "lb1", nodes, best)
    for idx, (depth, limit1, prmu) in enumerate(nodes_of(nodes)):
        for k in range(limit1 + 1, jobs):
            child = prmu[:]
            child[depth], child[k] = child[k], child[depth]
            expect = py_lb1_bound(ptm, jobs, machines, child, limit1 + 1, mt)
            assert cpp[idx * jobs + k] == expect, (idx, k)


def test_lb2_vs_python(core):
    inst = 2  # 20x5: 10 machine pairs, fast in pure python
    jobs, machines = core.taillard_nb_jobs(inst), core.taillard_nb_machines(inst)
    ptm = core.taillard_processing_times(inst)
    mt = py_min_tails(ptm, jobs, machines)
    nodes, _, _, best = core.pfsp_bfs_frontier(inst, "lb2", 1, 128)
    cpp = core.pfsp_cpu_bounds(inst, "lb2", nodes, best)
    rng = random.Random(7)
    all_nodes = list(nodes_of(nodes))
    for idx in rng.sample(range(len(all_nodes)), min(40, len(all_nodes))):
        depth, limit1, prmu = all_nodes[idx]
        for k in range(limit1 + 1, jobs):
            child = prmu[:]
            child[depth], child[k] = child[k], child[depth]
            expect = py_lb2_bound(ptm, jobs, machines, child, limit1 + 1, mt, best)
            assert cpp[idx * jobs + k] == expect, (idx, k)


def test_lb1d_vs_python(core):
    for inst in (2, 14):
        jobs, machines = core.taillard_nb_jobs(inst), core.taillard_nb_machines(inst)
        ptm = core.taillard_processing_times(inst)
        mt = py_min_tails(ptm, jobs, machines)
        nodes, _, _, best = core.pfsp_bfs_frontier(inst, "lb1_d", 1, 256)
        cpp = core.pfsp_cpu_bounds(inst, "lb1_d", nodes, best)
        for idx, (depth, limit1, prmu) in enumerate(nodes_of(nodes)):
            for k in range(limit1 + 1, jobs):
                expect = py_lb1d_child_bound(ptm, jobs, machines, prmu, limit1, mt,
                                             prmu[k])
                assert cpp[idx * jobs + k] == expect, (inst, idx, k)
