"""k_nq_x with split finisher jobs (SPLIT 1 and 2), one iteration at a time.

Every case runs ONE devpool iteration through nq_devpool_step at split 1 and 2,
twice each: the two runs must be byte-identical (which lane walks which sub-job
varies from run to run, the outputs are sums) and must equal the pure-CPU step
oracle (helpers/devpool_step_oracle.py), which knows nothing of jobs or queues.
The pools give a block's sub-job queue the shapes the kernel treats
differently: no job, one job of one sub-job, sub-job totals around the 256
lanes (one lane refills) and around the queue's capacity (a second round), the
1024-job block (many rounds), jobs of every height, and the tile's slot edges.
`shape` recomputes on the CPU, with nq_finish_block_cpu over the job states
of each block, how many jobs, sub-jobs and rounds the block has, so each test
first proves that its pool has the shape it names.
"""
import os
import sys
from collections import Counter

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_step_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 1024  # child slots per block
SPLITS = (1, 2)

_oracle_cache = {}


def run_nq(gpu, pool, N, split, g=1, finish=8, m=1, M=None, what=""):
    key = (pool, N, finish, m, M)  # the oracle's counts depend on neither g nor split
    if key not in _oracle_cache:
        _oracle_cache[key] = orc.nq_step(gpu, pool, N, 1, finish, m, M)
    exp = _oracle_cache[key]
    a = gpu.nq_devpool_step(pool, N, g, finish, m, M, None, "auto", 0, split)
    b = gpu.nq_devpool_step(pool, N, g, finish, m, M, None, "auto", 0, split)
    what = ("nq", what, "N", N, "n", len(pool) // 24, "g", g, "finish", finish, "split", split)
    assert a == b, (what, "two runs differ")
    orc.check_step(exp, a[0], a[1], what)
    return exp, a


def block_jobs(core, pool, N, finish):
    """Per block, the finisher jobs in queue (= slot) order, as the states
    (cols, d1, d2, row) below the safe child."""
    n = len(pool) // 24
    labels = core.nq_cpu_labels(N, 1, pool)
    msk = (1 << N) - 1
    blocks = [[] for _ in range((n * N + TILE - 1) // TILE)]
    for t in range(n * N):
        pid, k = divmod(t, N)
        node = pool[pid * 24:(pid + 1) * 24]
        depth = node[0]
        if depth >= N or k < depth or labels[t] != 1 or not 0 < N - depth - 1 <= finish:
            continue
        cols = d1 = d2 = 0
        for col in list(node[1:1 + depth]) + [node[1 + k]]:
            cols |= 1 << col
            d1 = ((d1 | 1 << col) << 1) & msk
            d2 = (d2 | 1 << col) >> 1
        blocks[t // TILE].append((cols, d1, d2, depth + 1))
    return blocks


def shape(core, pool, N, split, finish=8):
    """Per block: (jobs, sub-jobs, rounds) at the kernel's queue capacity."""
    out = []
    for jobs in block_jobs(core, pool, N, finish):
        _, _, entries, rounds = core.nq_finish_block_cpu(jobs, N, 1, split, core.NQ_SPLIT_QCAP)
        out.append((len(jobs), entries, rounds))
    return out


def one_job_node(core, rng, N):
    """A depth N-2 node of which exactly one child is safe: one job with one
    row left, which is never split (one sub-job)."""
    while True:
        node = orc.random_nq_nodes(rng, 1, N, N - 2, N - 2)
        lab = core.nq_cpu_labels(N, 1, node)
        if sum(lab[k] == 1 for k in range(N - 2, N)) == 1:
            return node


def root(N):
    return orc.nq_node(0, list(range(N)))


def leaf(N):
    return orc.nq_node(N, list(range(N)))


def pool_with_subjobs(core, split, target):
    """One block of N = 9 nodes whose jobs split into exactly `target`
    sub-jobs: depth-0 parents (56 / 234 sub-jobs at split 1 / 2), depth-1
    parents and single-sub-job nodes, largest first."""
    N = 9
    rng = orc.rng(9000 + target)
    menu = [root(N)] + [orc.nq_node(1, [c] + [x for x in range(N) if x != c]) for c in (0, 4)]
    menu = sorted(((shape(core, node, N, split)[0][1], node) for node in menu), reverse=True)
    pool, left = b"", target
    for entries, node in menu:
        pool += node * (left // entries)
        left %= entries
    pool += b"".join(one_job_node(core, rng, N) for _ in range(left))
    assert len(pool) // 24 * N <= TILE
    return pool


@pytest.mark.parametrize("split", SPLITS)
def test_no_job(gpu, split):
    N = 9
    pool = orc.random_nq_nodes(orc.rng(901), 100, N, N - 1, N)  # bottom-row children, leaves
    assert shape(gpu, pool, N, split) == [(0, 0, 0)]
    run_nq(gpu, pool, N, split, what="no job")
    pool = root(20) * 40  # pushed children only
    assert shape(gpu, pool, 20, split) == [(0, 0, 0)]
    run_nq(gpu, pool, 20, split, what="no job, pushes")


@pytest.mark.parametrize("split", SPLITS)
def test_one_job_one_subjob(gpu, split):
    N = 9
    pool = leaf(N) * 60 + one_job_node(gpu, orc.rng(902), N) + leaf(N) * 40
    assert shape(gpu, pool, N, split) == [(1, 1, 1)]
    exp, _ = run_nq(gpu, pool, N, split, what="one job")
    assert exp.ctl["size"] == 0


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("subjobs", [255, 256, 257])
def test_subjobs_around_the_lane_count(gpu, split, subjobs):
    """At 257 exactly one lane draws a second sub-job."""
    pool = pool_with_subjobs(gpu, split, subjobs)
    ((_, entries, rounds),) = shape(gpu, pool, 9, split)
    assert entries == subjobs and rounds == 1
    run_nq(gpu, pool, 9, split, what=("subjobs", subjobs))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("over", [-1, 0, 1])
def test_subjobs_around_the_queue_capacity(gpu, split, over):
    """QCAP - 1 and QCAP fill one round, QCAP + 1 needs a second one."""
    pool = pool_with_subjobs(gpu, split, gpu.NQ_SPLIT_QCAP + over)
    ((_, entries, rounds),) = shape(gpu, pool, 9, split)
    assert entries == gpu.NQ_SPLIT_QCAP + over and rounds == (2 if over > 0 else 1)
    run_nq(gpu, pool, 9, split, what=("qcap", over))


@pytest.mark.parametrize("split", SPLITS)
def test_full_job_queue_many_rounds(gpu, split):
    """114 depth-0 parents of N = 9: all 1024 slots of block 0 are jobs of 8
    rows; their sub-jobs need several rounds. Block 1 holds the last two."""
    N = 9
    pool = root(N) * 114
    (j0, e0, r0), (j1, _, r1) = shape(gpu, pool, N, split)
    assert (j0, j1, r1) == (1024, 2, 1)
    assert e0 > 2 * gpu.NQ_SPLIT_QCAP and r0 >= 3
    _, (out, ctl) = run_nq(gpu, pool, N, split, what="full queue")
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
    ((_, entries, _),) = shape(gpu, pool, N, split)
    assert entries > len(jobs)
    exp, _ = run_nq(gpu, pool, N, split, what="mixed")
    assert exp.children  # some children were pushed
    run_nq(gpu, pool, N, split, finish=5, what="mixed")  # the taller jobs are pushed


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("N,n", [(11, 93), (8, 128), (5, 205)])
def test_child_slot_edges(gpu, split, N, n):
    """n * N = 1023 / 1024 / 1025 child slots."""
    assert n * N == {11: 1023, 8: 1024, 5: 1025}[N]
    pool = orc.random_nq_nodes(orc.rng(7000 + N), n, N)
    assert sum(s[1] for s in shape(gpu, pool, N, split)) > 0
    for finish in (2, 8):
        run_nq(gpu, pool, N, split, finish=finish, what="slot edge")


@pytest.mark.parametrize("split", SPLITS)
def test_several_blocks_and_depths(gpu, split):
    N = 13
    pool = orc.random_nq_nodes(orc.rng(5113), 300, N)  # 4 blocks, parents straddle them
    assert len(shape(gpu, pool, N, split)) == 4
    for finish in (1, 2, 5, 8):
        run_nq(gpu, pool, N, split, finish=finish)


@pytest.mark.parametrize("split", SPLITS)
def test_g2_counts_like_g1(gpu, split):
    N = 13
    pool = orc.random_nq_nodes(orc.rng(13002), 300, N)
    _, (out1, ctl1) = run_nq(gpu, pool, N, split, g=1)
    _, (out2, ctl2) = run_nq(gpu, pool, N, split, g=2)
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
