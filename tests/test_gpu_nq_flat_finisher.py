"""k_nq_x's block-local job queue and flat finisher loop, one iteration at a time.

Every case runs ONE devpool iteration through nq_devpool_step and compares all
it writes with the pure-CPU oracle (helpers/devpool_step_oracle.py); every
configuration runs twice and must be byte-identical. The pools are built so
that a block's job queue takes the shapes the kernel treats differently: no
job, one job, a queue one short of / equal to / one above the 256 lanes (one
lane refills), the full 1024-entry queue, jobs of every subtree height next to
pushed children, bottom-row children and leaf parents, and child-slot counts
around the 1024-slot tile. `classify` recomputes on the CPU which child slot
becomes what, so each test first proves that its pool has the shape it names.
"""
import os
import sys
from collections import Counter

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_step_oracle as orc  # noqa: E402
from nq_finish_cases import TILE, leaf, one_job_node, root, run_nq  # noqa: E402

pytestmark = pytest.mark.gpu


def classify(core, pool, N, finish):
    """Per block, what each child slot of the popped pool becomes:
    Counter of 'leaf' (slot 0 of a depth-N parent), 'rem0' (safe bottom-row
    child), 'push' (safe child with rem > finish) and ('job', rem)."""
    n = len(pool) // 24
    labels = core.nq_cpu_labels(N, 1, pool)
    blocks = [Counter() for _ in range((n * N + TILE - 1) // TILE)]
    for t in range(n * N):
        pid, k = divmod(t, N)
        depth = pool[pid * 24]
        blk = blocks[t // TILE]
        if depth == N:
            blk["leaf"] += k == 0
        elif k >= depth and labels[t] == 1:
            rem = N - depth - 1
            if rem == 0:
                blk["rem0"] += 1
            elif rem <= finish:
                blk[("job", rem)] += 1
            else:
                blk["push"] += 1
    return blocks


def njobs(blk):
    return sum(v for key, v in blk.items() if isinstance(key, tuple))


@pytest.mark.parametrize("N", [5, 9, 13, 20])
def test_finish_depths_on_random_pools(gpu, N):
    # 300 nodes: several blocks for N >= 5, parents straddling block borders
    pool = orc.random_nq_nodes(orc.rng(5100 + N), 300, N)
    for finish in (0, 1, 2, 5, 8):
        run_nq(gpu, pool, N, finish=finish)


def test_mixed_block(gpu):
    """One block whose queue holds jobs of every height 1..8 together with
    pushed children, bottom-row children and leaf parents."""
    N, finish = 13, 8
    pool = orc.random_nq_nodes(orc.rng(13008), 78, N)  # 1014 slots: one block
    (blk,) = classify(gpu, pool, N, finish)
    assert {key[1] for key in blk if isinstance(key, tuple)} == set(range(1, 9)), blk
    assert blk["push"] > 0 and blk["rem0"] > 0 and blk["leaf"] > 0, blk
    run_nq(gpu, pool, N, finish=finish, what="mixed")
    # a shallower limit turns the taller jobs into pushed children
    run_nq(gpu, pool, N, finish=5, what="mixed")


def test_no_job(gpu):
    N = 9
    # bottom-row children and leaf parents only
    pool = orc.random_nq_nodes(orc.rng(901), 100, N, N - 1, N)
    (blk,) = classify(gpu, pool, N, 8)
    assert njobs(blk) == 0 and blk["rem0"] > 0 and blk["leaf"] > 0, blk
    run_nq(gpu, pool, N, what="no job")
    # pushed children only
    pool = root(20) * 40
    (blk,) = classify(gpu, pool, 20, 8)
    assert njobs(blk) == 0 and blk["push"] == 800, blk
    run_nq(gpu, pool, 20, what="no job, pushes")


def test_one_job(gpu):
    N = 9
    rng = orc.rng(902)
    pool = leaf(N) * 60 + one_job_node(gpu, rng, N) + leaf(N) * 40
    (blk,) = classify(gpu, pool, N, 8)
    assert njobs(blk) == 1, blk
    exp, _ = run_nq(gpu, pool, N, what="one job")
    assert exp.ctl["size"] == 0


@pytest.mark.parametrize("jobs", [255, 256, 257])
def test_queue_around_the_lane_count(gpu, jobs):
    """28 depth-0 parents of N = 9 give 252 eight-row jobs; single-job nodes
    fill up to the target. At 257 exactly one lane takes a second job."""
    N = 9
    rng = orc.rng(903)
    pool = root(N) * 28 + b"".join(one_job_node(gpu, rng, N) for _ in range(jobs - 252))
    (blk,) = classify(gpu, pool, N, 8)
    assert njobs(blk) == jobs, blk
    run_nq(gpu, pool, N, what=("jobs", jobs))


def test_full_queue(gpu):
    """114 depth-0 parents of N = 9, finish 8: all 1024 slots of block 0 are
    jobs, block 1 holds the last two."""
    N = 9
    pool = root(N) * 114
    blocks = classify(gpu, pool, N, 8)
    assert [njobs(b) for b in blocks] == [1024, 2], blocks
    exp, (out, ctl) = run_nq(gpu, pool, N, what="full queue")
    assert out == b"" and ctl["sol"] == 114 * 352


@pytest.mark.parametrize("N,n", [(11, 93), (8, 128), (5, 205)])
def test_child_slot_edges(gpu, N, n):
    """n * N = 1023 / 1024 / 1025 child slots."""
    assert n * N == {11: 1023, 8: 1024, 5: 1025}[N]
    pool = orc.random_nq_nodes(orc.rng(7000 + N), n, N)
    for finish in (2, 8):
        run_nq(gpu, pool, N, finish=finish, what="slot edge")


def test_last_block_one_slot_wide(gpu):
    """1025 slots: block 1 owns one slot, and that slot is a job."""
    N, n = 5, 205
    rng = orc.rng(7105)
    head = orc.random_nq_nodes(rng, n - 1, N)
    while True:
        pool = head + orc.random_nq_nodes(rng, 1, N, 0, N - 2)
        blocks = classify(gpu, pool, N, 8)
        if njobs(blocks[1]) == 1:
            break
    assert len(blocks) == 2 and sum(blocks[1].values()) == 1
    run_nq(gpu, pool, N, what="one-slot block")


def test_g2_counts_like_g1(gpu):
    N = 13
    pool = orc.random_nq_nodes(orc.rng(13002), 300, N)
    _, (out1, ctl1) = run_nq(gpu, pool, N, g=1)
    _, (out2, ctl2) = run_nq(gpu, pool, N, g=2)
    assert ctl1 == ctl2
    assert Counter(out1[i:i + 21] for i in range(0, len(out1), 24)) == \
        Counter(out2[i:i + 21] for i in range(0, len(out2), 24))


@pytest.mark.parametrize("m,M", [(1, 100), (300, 79), (250, 1), (301, 300)])
def test_pop_window_takes_the_tail_only(gpu, m, M):
    N, n = 13, 300
    pool = orc.random_nq_nodes(orc.rng(13003), n, N)
    exp, (out, ctl) = run_nq(gpu, pool, N, m=m, M=M)
    c = 0 if n < m else min(n, M)
    assert ctl["chunk"] == c
    assert out[:(n - c) * 24] == pool[:(n - c) * 24]


def test_chain_of_four(gpu):
    N, finish = 12, 8
    pool = orc.random_nq_nodes(orc.rng(12004), 200, N, 0, 5)
    windows = [64, 64, 64, 64]
    capacity = 200 * 21 + 64
    a = gpu.nq_devpool_chain(pool, N, windows, 1, finish, 1, capacity, "auto")
    b = gpu.nq_devpool_chain(pool, N, windows, 1, finish, 1, capacity, "auto")
    assert a == b, "two runs differ"

    def step(p, M, tree, sol, iters, best):
        return orc.nq_step(gpu, p, N, 1, finish, 1, M, tree, sol, iters)

    exps = orc.check_chain(gpu, pool, a, windows, step, capacity=capacity, what="chain")
    assert all(e is not None for e in exps)
    # the chain both pushed children and finished subtrees
    assert a[-1][1]["size"] > 0 and a[-1][1]["sol"] > 0
