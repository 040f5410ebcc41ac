"""k_nq_x with split finisher jobs (split 1 and 2), one iteration at a time.

Every case runs ONE devpool iteration through nq_devpool_step at split 1 and 2,
twice each: the two runs must be byte-identical (which lane walks which sub-job
varies from run to run, the outputs are sums) and must equal the pure-CPU step
oracle (helpers/devpool_step_oracle.py), which knows nothing of jobs or queues.
The pools give a block's sub-job queue the shapes the kernel treats
differently: no job, one job of one sub-job, sub-job totals around the 256
lanes (one lane refills) and around the queue's capacity (a second round), the
1024-job block (many rounds), jobs of every height, and the tile's slot edges.
`split_shape` (helpers/nq_finish_cases.py) recomputes on the CPU, with
nq_finish_block_cpu over the job states of each block, how many jobs, sub-jobs
and rounds the block has, so each test first proves that its pool has the shape
it names.
"""
import os
import sys
from collections import Counter

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_step_oracle as orc  # noqa: E402
from nq_finish_cases import (block_jobs, leaf, one_job_node, pool_with_subjobs,  # noqa: E402
                             root, run_nq, split_shape)

pytestmark = pytest.mark.gpu

SPLITS = (1, 2)


@pytest.mark.parametrize("split", SPLITS)
def test_no_job(gpu, split):
    N = 9
    pool = orc.random_nq_nodes(orc.rng(901), 100, N, N - 1, N)  # bottom-row children, leaves
    assert split_shape(gpu, pool, N, split) == [(0, 0, 0)]
    run_nq(gpu, pool, N, split=split, what="no job")
    pool = root(20) * 40  # pushed children only
    assert split_shape(gpu, pool, 20, split) == [(0, 0, 0)]
    run_nq(gpu, pool, 20, split=split, what="no job, pushes")


@pytest.mark.parametrize("split", SPLITS)
def test_one_job_one_subjob(gpu, split):
    N = 9
    pool = leaf(N) * 60 + one_job_node(gpu, orc.rng(902), N) + leaf(N) * 40
    assert split_shape(gpu, pool, N, split) == [(1, 1, 1)]
    exp, _ = run_nq(gpu, pool, N, split=split, what="one job")
    assert exp.ctl["size"] == 0


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("subjobs", [255, 256, 257])
def test_subjobs_around_the_lane_count(gpu, split, subjobs):
    """At 257 exactly one lane draws a second sub-job."""
    pool = pool_with_subjobs(gpu, split, subjobs)
    ((_, entries, rounds),) = split_shape(gpu, pool, 9, split)
    assert entries == subjobs and rounds == 1
    run_nq(gpu, pool, 9, split=split, what=("subjobs", subjobs))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("over", [-1, 0, 1])
def test_subjobs_around_the_queue_capacity(gpu, split, over):
    """QCAP - 1 and QCAP fill one round, QCAP + 1 needs a second one."""
    pool = pool_with_subjobs(gpu, split, gpu.NQ_SPLIT_QCAP + over)
    ((_, entries, rounds),) = split_shape(gpu, pool, 9, split)
    assert entries == gpu.NQ_SPLIT_QCAP + over and rounds == (2 if over > 0 else 1)
    run_nq(gpu, pool, 9, split=split, what=("qcap", over))


@pytest.mark.parametrize("split", SPLITS)
def test_full_job_queue_many_rounds(gpu, split):
    """114 depth-0 parents of N = 9: all 1024 slots of block 0 are jobs of 8
    rows; their sub-jobs need several rounds. Block 1 holds the last two."""
    N = 9
    pool = root(N) * 114
    (j0, e0, r0), (j1, _, r1) = split_shape(gpu, pool, N, split)
    assert (j0, j1, r1) == (1024, 2, 1)
    assert e0 > 2 * gpu.NQ_SPLIT_QCAP and r0 >= 3
    _, (out, ctl) = run_nq(gpu, pool, N, split=split, what="full queue")
    assert out == b"" and ctl["sol"] == 114 * 352


@pytest.mark.parametrize("split", SPLITS)
def test_mixed_block(gpu, split):
    """Jobs of every height 1..8 (so every clamp of the split depth) next to
    pushed children, bottom-row children and leaf parents."""
    N = 13
    pool = orc.random_nq_nodes(orc.rng(13008), 78, N)  # 1014 slots: one block
    (jobs,) = block_jobs(gpu, pool, N, 8)
    assert {N - j[3] for j in jobs} == set(range(1, 9))
    depths = Counter(pool[i] for i in range(0, len(pool), 24))
    assert depths[N] > 0 and depths[N - 1] > 0 and min(depths) < N - 9
    ((_, entries, _),) = split_shape(gpu, pool, N, split)
    assert entries > len(jobs)
    exp, _ = run_nq(gpu, pool, N, split=split, what="mixed")
    assert exp.children  # some children were pushed
    run_nq(gpu, pool, N, split=split, finish=5, what="mixed")  # the taller jobs are pushed


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("N,n", [(11, 93), (8, 128), (5, 205)])
def test_child_slot_edges(gpu, split, N, n):
    """n * N = 1023 / 1024 / 1025 child slots."""
    assert n * N == {11: 1023, 8: 1024, 5: 1025}[N]
    pool = orc.random_nq_nodes(orc.rng(7000 + N), n, N)
    assert sum(s[1] for s in split_shape(gpu, pool, N, split)) > 0
    for finish in (2, 8):
        run_nq(gpu, pool, N, split=split, finish=finish, what="slot edge")


@pytest.mark.parametrize("split", SPLITS)
def test_several_blocks_and_depths(gpu, split):
    N = 13
    pool = orc.random_nq_nodes(orc.rng(5113), 300, N)  # 4 blocks, parents straddle them
    assert len(split_shape(gpu, pool, N, split)) == 4
    for finish in (1, 2, 5, 8):
        run_nq(gpu, pool, N, split=split, finish=finish)


@pytest.mark.parametrize("split", SPLITS)
def test_g2_counts_like_g1(gpu, split):
    N = 13
    pool = orc.random_nq_nodes(orc.rng(13002), 300, N)
    _, (out1, ctl1) = run_nq(gpu, pool, N, split=split, g=1)
    _, (out2, ctl2) = run_nq(gpu, pool, N, split=split, g=2)
    assert ctl1 == ctl2
    assert Counter(out1[i:i + 21] for i in range(0, len(out1), 24)) == \
        Counter(out2[i:i + 21] for i in range(0, len(out2), 24))


@pytest.mark.parametrize("split", SPLITS)
def test_chain_of_four(gpu, split):
    N, finish = 12, 8
    pool = orc.random_nq_nodes(orc.rng(12004), 200, N, 0, 5)
    windows = [64, 64, 64, 64]
    capacity = 200 * 21 + 64
    a = gpu.nq_devpool_chain(pool, N, windows, 1, finish, 1, capacity, "auto", 0, split)
    b = gpu.nq_devpool_chain(pool, N, windows, 1, finish, 1, capacity, "auto", 0, split)
    assert a == b, "two runs differ"

    def step(p, M, tree, sol, iters, best):
        return orc.nq_step(gpu, p, N, 1, finish, 1, M, tree, sol, iters)

    exps = orc.check_chain(gpu, pool, a, windows, step, capacity=capacity, what="chain")
    assert all(e is not None for e in exps)
    assert a[-1][1]["size"] > 0 and a[-1][1]["sol"] > 0


@pytest.mark.parametrize("split", (0,) + SPLITS)
@pytest.mark.parametrize("N,tree,sol", [(12, 856188, 14200), (14, 27358552, 365596)])
def test_whole_search(gpu, split, N, tree, sol):
    """From the root to the empty pool, one whole-pool iteration after the
    other, against the frozen sequential counts (tests/test_nqueens_seq.py;
    N = 14 is nqueens_seq(14)'s count, its solutions the published value)."""
    pool, got_tree, got_sol, iters = root(N), 0, 0, 0
    while pool:
        pool, ctl = gpu.nq_devpool_step(pool, N, 1, 8, 1, None, None, "auto", 0, split)
        assert ctl["overflow"] == 0
        got_tree += ctl["tree"]
        got_sol += ctl["sol"]
        iters += 1
    assert iters == N - 8
    assert (got_tree, got_sol) == (tree, sol)


def test_split_is_validated(gpu):
    with pytest.raises(ValueError):
        gpu.nq_devpool_step(root(9), 9, 1, 8, 1, None, None, "auto", 0, 3)
