"""k_nq_x's batched, wave-uniform refill (split 1 and 2), one iteration at a time.

Every case runs ONE devpool iteration through nq_devpool_step(..., split,
refill) at refill 1 (a wave fetches as soon as one lane is idle), 16 and 64
(only the all-idle rule is left), twice each: the two runs must be
byte-identical and must equal the pure-CPU step oracle
(helpers/devpool_step_oracle.py), which knows nothing of jobs, queues or waves.
The pools are those of tests/test_gpu_nq_split_finisher.py
(helpers/nq_finish_cases.py), and
`split_shape` proves with nq_finish_block_cpu, on the CPU, that each pool gives the
block's queue the shape the test names: totals around the threshold, a wave,
the block's 256 lanes and the queue's capacity (a second round, where a
drained wave must fetch again).
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
REFILLS = (1, 16, 64)


def cases(f):
    f = pytest.mark.parametrize("split", SPLITS)(f)
    return pytest.mark.parametrize("refill", REFILLS)(f)


@cases
def test_no_job(gpu, split, refill):
    N = 9
    pool = orc.random_nq_nodes(orc.rng(901), 100, N, N - 1, N)  # bottom-row children, leaves
    assert split_shape(gpu, pool, N, split) == [(0, 0, 0)]
    run_nq(gpu, pool, N, split=split, refill=refill, what="no job")
    pool = root(20) * 40  # pushed children only
    assert split_shape(gpu, pool, 20, split) == [(0, 0, 0)]
    run_nq(gpu, pool, 20, split=split, refill=refill, what="no job, pushes")


@cases
def test_one_job_one_subjob(gpu, split, refill):
    N = 9
    pool = leaf(N) * 60 + one_job_node(gpu, orc.rng(902), N) + leaf(N) * 40
    assert split_shape(gpu, pool, N, split) == [(1, 1, 1)]
    exp, _ = run_nq(gpu, pool, N, split=split, refill=refill, what="one job")
    assert exp.ctl["size"] == 0


@cases
@pytest.mark.parametrize("subjobs", [15, 16, 17, 63, 64, 65, 255, 256, 257])
def test_subjobs_around_threshold_wave_and_block(gpu, split, refill, subjobs):
    """15 / 16 / 17: below, at and above the middle threshold (at refill 16 the
    15 start by the all-idle rule alone); 63 / 64 / 65: one wave's lanes;
    255 / 256 / 257: the block's, at 257 one lane draws a second sub-job."""
    pool = pool_with_subjobs(gpu, split, subjobs)
    ((_, entries, rounds),) = split_shape(gpu, pool, 9, split)
    assert entries == subjobs and rounds == 1
    run_nq(gpu, pool, 9, split=split, refill=refill, what=("subjobs", subjobs))


@cases
@pytest.mark.parametrize("over", [-1, 0, 1])
def test_subjobs_around_the_queue_capacity(gpu, split, refill, over):
    """QCAP - 1 and QCAP fill one round, QCAP + 1 needs a second one, in which
    the waves that drained in the first must fetch again."""
    pool = pool_with_subjobs(gpu, split, gpu.NQ_SPLIT_QCAP + over)
    ((_, entries, rounds),) = split_shape(gpu, pool, 9, split)
    assert entries == gpu.NQ_SPLIT_QCAP + over and rounds == (2 if over > 0 else 1)
    run_nq(gpu, pool, 9, split=split, refill=refill, what=("qcap", over))


@cases
def test_full_job_queue_many_rounds(gpu, split, refill):
    """114 depth-0 parents of N = 9: all 1024 slots of block 0 are jobs of 8
    rows; their sub-jobs need several rounds. Block 1 holds the last two."""
    N = 9
    pool = root(N) * 114
    (j0, e0, r0), (j1, _, r1) = split_shape(gpu, pool, N, split)
    assert (j0, j1, r1) == (1024, 2, 1)
    assert e0 > 2 * gpu.NQ_SPLIT_QCAP and r0 >= 3
    _, (out, ctl) = run_nq(gpu, pool, N, split=split, refill=refill, what="full queue")
    assert out == b"" and ctl["sol"] == 114 * 352


@cases
@pytest.mark.parametrize("N,n", [(11, 93), (8, 128), (5, 205)])
def test_child_slot_edges(gpu, split, refill, N, n):
    """n * N = 1023 / 1024 / 1025 child slots."""
    assert n * N == {11: 1023, 8: 1024, 5: 1025}[N]
    pool = orc.random_nq_nodes(orc.rng(7000 + N), n, N)
    assert sum(s[1] for s in split_shape(gpu, pool, N, split)) > 0
    for finish in (2, 8):
        run_nq(gpu, pool, N, split=split, refill=refill, finish=finish, what="slot edge")


@cases
def test_mixed_block_every_height(gpu, split, refill):
    N = 13
    pool = orc.random_nq_nodes(orc.rng(13008), 78, N)  # 1014 slots: one block
    (jobs,) = block_jobs(gpu, pool, N, 8)
    assert {N - j[3] for j in jobs} == set(range(1, 9))
    exp, _ = run_nq(gpu, pool, N, split=split, refill=refill, what="mixed")
    assert exp.children  # some children were pushed


@cases
def test_g2_counts_like_g1(gpu, split, refill):
    N = 13
    pool = orc.random_nq_nodes(orc.rng(13002), 300, N)
    _, (out1, ctl1) = run_nq(gpu, pool, N, split=split, refill=refill, g=1)
    _, (out2, ctl2) = run_nq(gpu, pool, N, split=split, refill=refill, g=2)
    assert ctl1 == ctl2
    assert Counter(out1[i:i + 21] for i in range(0, len(out1), 24)) == \
        Counter(out2[i:i + 21] for i in range(0, len(out2), 24))


@cases
def test_chain_of_four(gpu, split, refill):
    N, finish = 12, 8
    pool = orc.random_nq_nodes(orc.rng(12004), 200, N, 0, 5)
    windows = [64, 64, 64, 64]
    capacity = 200 * 21 + 64
    a = gpu.nq_devpool_chain(pool, N, windows, 1, finish, 1, capacity, "auto", 0, split, refill)
    b = gpu.nq_devpool_chain(pool, N, windows, 1, finish, 1, capacity, "auto", 0, split, refill)
    assert a == b, "two runs differ"

    def step(p, M, tree, sol, iters, best):
        return orc.nq_step(gpu, p, N, 1, finish, 1, M, tree, sol, iters)

    exps = orc.check_chain(gpu, pool, a, windows, step, capacity=capacity, what="chain")
    assert all(e is not None for e in exps)
    assert a[-1][1]["size"] > 0 and a[-1][1]["sol"] > 0


@cases
@pytest.mark.parametrize("N,tree,sol", [(12, 856188, 14200), (14, 27358552, 365596)])
def test_whole_search(gpu, split, refill, N, tree, sol):
    """From the root to the empty pool, one whole-pool iteration after the
    other, against the frozen sequential counts (tests/test_nqueens_seq.py)."""
    pool, got_tree, got_sol, iters = root(N), 0, 0, 0
    while pool:
        pool, ctl = gpu.nq_devpool_step(pool, N, 1, 8, 1, None, None, "auto", 0, split, refill)
        assert ctl["overflow"] == 0
        got_tree += ctl["tree"]
        got_sol += ctl["sol"]
        iters += 1
    assert iters == N - 8
    assert (got_tree, got_sol) == (tree, sol)


def test_default_refill_is_the_engines(gpu):
    """refill = -1 (and the older positional call without it) take the engine's
    default: the same bytes as naming it."""
    N = 13
    pool = orc.random_nq_nodes(orc.rng(13002), 300, N)
    want = gpu.nq_devpool_step(pool, N, 1, 8, 1, None, None, "auto", 0, 2, gpu.nq_refill_default())
    assert gpu.nq_devpool_step(pool, N, 1, 8, 1, None, None, "auto", 0, 2) == want
    assert gpu.nq_devpool_step(pool, N, 1, 8, 1, None, None, "auto", 0, 2, -1) == want


def test_refill_is_validated(gpu):
    for refill in (0, 65):
        with pytest.raises(ValueError):
            gpu.nq_devpool_step(root(9), 9, 1, 8, 1, None, None, "auto", 0, 2, refill)
        with pytest.raises(ValueError):
            gpu.nq_devpool_chain(root(9), 9, [1], 1, 8, 1, None, "auto", 0, 2, refill)
