"""k_nq_x's batched, wave-uniform refill (SPLIT 1 and 2), one iteration at a time.

Every case runs ONE devpool iteration through nq_devpool_step(..., split,
refill) at refill 1 (a wave fetches as soon as one lane is idle), 16 and 64
(only the all-idle rule is left), twice each: the two runs must be
byte-identical and must equal the pure-CPU step oracle
(helpers/devpool_step_oracle.py), which knows nothing of jobs, queues or waves.
The pools are built as tests/test_gpu_nq_split_finisher.py builds them, and
`shape` proves with nq_finish_block_cpu, on the CPU, that each pool gives the
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

pytestmark = pytest.mark.gpu

TILE = 1024  # child slots per block
SPLITS = (1, 2)
REFILLS = (1, 16, 64)

_oracle_cache = {}


def cases(f):
    f = pytest.mark.parametrize("split", SPLITS)(f)
    return pytest.mark.parametrize("refill", REFILLS)(f)


def run_nq(gpu, pool, N, split, refill, g=1, finish=8, m=1, M=None, what=""):
    key = (pool, N, finish, m, M)  # the oracle's counts depend on none of g, split, refill
    if key not in _oracle_cache:
        _oracle_cache[key] = orc.nq_step(gpu, pool, N, 1, finish, m, M)
    exp = _oracle_cache[key]
    a = gpu.nq_devpool_step(pool, N, g, finish, m, M, None, "auto", 0, split, refill)
    b = gpu.nq_devpool_step(pool, N, g, finish, m, M, None, "auto", 0, split, refill)
    what = ("nq", what, "N", N, "n", len(pool) // 24, "g", g, "finish", finish, "split", split,
            "refill", refill)
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


_shape_cache = {}


def shape(core, pool, N, split, finish=8):
    """Per block: (jobs, sub-jobs, rounds) at the kernel's queue capacity."""
    key = (pool, N, split, finish)
    if key not in _shape_cache:
        out = []
        for jobs in block_jobs(core, pool, N, finish):
            _, _, entries, rounds = core.nq_finish_block_cpu(jobs, N, 1, split,
                                                             core.NQ_SPLIT_QCAP)
            out.append((len(jobs), entries, rounds))
        _shape_cache[key] = out
    return _shape_cache[key]


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


_pools = {}


def pool_with_subjobs(core, split, target):
    """One block of N = 9 nodes whose jobs split into exactly `target`
    sub-jobs: depth-0 parents, depth-1 parents and single-sub-job nodes,
    largest first."""
    if (split, target) in _pools:
        return _pools[split, target]
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
    _pools[split, target] = pool
    return pool


@cases
def test_no_job(gpu, split, refill):
    N = 9
    pool = orc.random_nq_nodes(orc.rng(901), 100, N, N - 1, N)  # bottom-row children, leaves
    assert shape(gpu, pool, N, split) == [(0, 0, 0)]
    run_nq(gpu, pool, N, split, refill, what="no job")
    pool = root(20) * 40  # pushed children only
    assert shape(gpu, pool, 20, split) == [(0, 0, 0)]
    run_nq(gpu, pool, 20, split, refill, what="no job, pushes")


@cases
def test_one_job_one_subjob(gpu, split, refill):
    N = 9
    pool = leaf(N) * 60 + one_job_node(gpu, orc.rng(902), N) + leaf(N) * 40
    assert shape(gpu, pool, N, split) == [(1, 1, 1)]
    exp, _ = run_nq(gpu, pool, N, split, refill, what="one job")
    assert exp.ctl["size"] == 0


@cases
@pytest.mark.parametrize("subjobs", [15, 16, 17, 63, 64, 65, 255, 256, 257])
def test_subjobs_around_threshold_wave_and_block(gpu, split, refill, subjobs):
    """15 / 16 / 17: below, at and above the middle threshold (at refill 16 the
    15 start by the all-idle rule alone); 63 / 64 / 65: one wave's lanes;
    255 / 256 / 257: the block's, at 257 one lane draws a second sub-job."""
    pool = pool_with_subjobs(gpu, split, subjobs)
    ((_, entries, rounds),) = shape(gpu, pool, 9, split)
    assert entries == subjobs and rounds == 1
    run_nq(gpu, pool, 9, split, refill, what=("subjobs", subjobs))


@cases
@pytest.mark.parametrize("over", [-1, 0, 1])
def test_subjobs_around_the_queue_capacity(gpu, split, refill, over):
    """QCAP - 1 and QCAP fill one round, QCAP + 1 needs a second one, in which
    the waves that drained in the first must fetch again."""
    pool = pool_with_subjobs(gpu, split, gpu.NQ_SPLIT_QCAP + over)
    ((_, entries, rounds),) = shape(gpu, pool, 9, split)
    assert entries == gpu.NQ_SPLIT_QCAP + over and rounds == (2 if over > 0 else 1)
    run_nq(gpu, pool, 9, split, refill, what=("qcap", over))


@cases
def test_full_job_queue_many_rounds(gpu, split, refill):
    """114 depth-0 parents of N = 9: all 1024 slots of block 0 are jobs of 8
    rows; their sub-jobs need several rounds. Block 1 holds the last two."""
    N = 9
    pool = root(N) * 114
    (j0, e0, r0), (j1, _, r1) = shape(gpu, pool, N, split)
    assert (j0, j1, r1) == (1024, 2, 1)
    assert e0 > 2 * gpu.NQ_SPLIT_QCAP and r0 >= 3
    _, (out, ctl) = run_nq(gpu, pool, N, split, refill, what="full queue")
    assert out == b"" and ctl["sol"] == 114 * 352


@cases
@pytest.mark.parametrize("N,n", [(11, 93), (8, 128), (5, 205)])
def test_child_slot_edges(gpu, split, refill, N, n):
    """n * N = 1023 / 1024 / 1025 child slots."""
    assert n * N == {11: 1023, 8: 1024, 5: 1025}[N]
    pool = orc.random_nq_nodes(orc.rng(7000 + N), n, N)
    assert sum(s[1] for s in shape(gpu, pool, N, split)) > 0
    for finish in (2, 8):
        run_nq(gpu, pool, N, split, refill, finish=finish, what="slot edge")


@cases
def test_mixed_block_every_height(gpu, split, refill):
    N = 13
    pool = orc.random_nq_nodes(orc.rng(13008), 78, N)  # 1014 slots: one block
    (jobs,) = block_jobs(gpu, pool, N, 8)
    assert {N - j[3] for j in jobs} == set(range(1, 9))
    exp, _ = run_nq(gpu, pool, N, split, refill, what="mixed")
    assert exp.children  # some children were pushed


@cases
def test_g2_counts_like_g1(gpu, split, refill):
    N = 13
    pool = orc.random_nq_nodes(orc.rng(13002), 300, N)
    _, (out1, ctl1) = run_nq(gpu, pool, N, split, refill, g=1)
    _, (out2, ctl2) = run_nq(gpu, pool, N, split, refill, g=2)
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
