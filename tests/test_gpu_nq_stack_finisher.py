"""k_nq_x with the wave-stack finisher (stack = 1), one iteration at a time.

Every case runs ONE devpool iteration through nq_devpool_step(..., stack=1)
twice: the two runs must be byte-identical (which lane takes which row varies
from run to run, the outputs are sums) and must equal the pure-CPU step oracle
(helpers/devpool_step_oracle.py), which knows nothing of jobs or stacks.
`shape` first plays each block on the CPU twin (nq_finish_stack_cpu, the
kernel's own functions), so a case that names a fallback, or none, or a stack
height, proves it before the kernel runs. The twin's waves take turns; the
kernel's run freely, so its heights can differ, but a `stack_cap` of 0 forces
the fallback for every push and the capacity bounds every height whatever the
order. No case needs a fault or a hang to fail: wrong counts fail the compare.
"""
import functools
import os
import sys
from collections import Counter

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_step_oracle as orc  # noqa: E402
import nq_finish_cases  # noqa: E402
from nq_finish_cases import block_jobs, leaf, one_job_node, root  # noqa: E402

pytestmark = pytest.mark.gpu

run_nq = functools.partial(nq_finish_cases.run_nq, stack=1)


def shape(core, pool, N, finish=8, refill=None, cap=None):
    """Per block on the CPU twin: (jobs, highest stack of a wave, fallback walks)."""
    refill = core.nq_refill_default() if refill is None else refill
    cap = core.NQ_STACK_CAP if cap is None else cap
    out = []
    for jobs in block_jobs(core, pool, N, finish):
        _, _, _, peak, fb = core.nq_finish_stack_cpu(jobs, N, 1, refill, 4, 64, cap)
        assert max(peak) <= cap
        out.append((len(jobs), max(peak), fb))
    return out


def test_no_job(gpu):
    N = 9
    pool = orc.random_nq_nodes(orc.rng(901), 100, N, N - 1, N)  # bottom-row children, leaves
    assert shape(gpu, pool, N) == [(0, 0, 0)]
    run_nq(gpu, pool, N, what="no job")
    pool = root(20) * 40  # pushed children only
    assert shape(gpu, pool, 20) == [(0, 0, 0)]
    run_nq(gpu, pool, 20, what="no job, pushes")


def test_one_job(gpu):
    N = 9
    pool = leaf(N) * 60 + one_job_node(gpu, orc.rng(902), N) + leaf(N) * 40
    assert shape(gpu, pool, N) == [(1, 0, 0)]  # one row left: nothing is ever pushed
    exp, _ = run_nq(gpu, pool, N, what="one job")
    assert exp.ctl["size"] == 0
    pool = leaf(N) * 10 + orc.nq_node(1, [4] + [x for x in range(N) if x != 4])
    ((jobs, peak, fb),) = shape(gpu, pool, N)
    assert jobs > 1 and peak > 0 and fb == 0  # tall jobs: the stack is used
    run_nq(gpu, pool, N, what="few tall jobs")


def test_full_job_queue(gpu):
    """114 depth-0 parents of N = 9: all 1024 slots of block 0 are jobs of 8
    rows. Block 1 holds the last two."""
    N = 9
    pool = root(N) * 114
    (j0, peak0, _), (j1, _, fb1) = shape(gpu, pool, N)
    assert (j0, j1, fb1) == (1024, 2, 0) and peak0 > 64
    _, (out, ctl) = run_nq(gpu, pool, N, what="full queue")
    assert out == b"" and ctl["sol"] == 114 * 352


def test_mixed_block(gpu):
    """Jobs of every height 1..8 next to pushed children, bottom-row children
    and leaf parents."""
    N = 13
    pool = orc.random_nq_nodes(orc.rng(13008), 78, N)  # 1014 slots: one block
    (jobs,) = block_jobs(gpu, pool, N, 8)
    assert {N - j[3] for j in jobs} == set(range(1, 9))
    depths = Counter(pool[i] for i in range(0, len(pool), 24))
    assert depths[N] > 0 and depths[N - 1] > 0 and min(depths) < N - 9
    ((_, peak, fb),) = shape(gpu, pool, N)
    assert peak > 0 and fb == 0
    exp, _ = run_nq(gpu, pool, N, what="mixed")
    assert exp.children  # some children were pushed
    run_nq(gpu, pool, N, finish=5, what="mixed")  # the taller jobs are pushed


@pytest.mark.parametrize("N,n", [(11, 93), (8, 128), (5, 205)])
def test_child_slot_edges(gpu, N, n):
    """n * N = 1023 / 1024 / 1025 child slots."""
    assert n * N == {11: 1023, 8: 1024, 5: 1025}[N]
    pool = orc.random_nq_nodes(orc.rng(7000 + N), n, N)
    assert sum(s[0] for s in shape(gpu, pool, N)) > 0
    for finish in (2, 8):
        run_nq(gpu, pool, N, finish=finish, what="slot edge")


def test_g2_counts_like_g1(gpu):
    N = 13
    pool = orc.random_nq_nodes(orc.rng(13002), 300, N)
    assert all(peak > 0 for _, peak, _ in shape(gpu, pool, N))  # every block uses its stacks
    _, (out1, ctl1) = run_nq(gpu, pool, N, g=1)
    _, (out2, ctl2) = run_nq(gpu, pool, N, g=2)
    assert ctl1 == ctl2
    assert Counter(out1[i:i + 21] for i in range(0, len(out1), 24)) == \
        Counter(out2[i:i + 21] for i in range(0, len(out2), 24))


@pytest.mark.parametrize("refill", [1, 16, 64])
def test_refill_thresholds(gpu, refill):
    N = 13
    pool = orc.random_nq_nodes(orc.rng(5113), 300, N)  # 4 blocks, parents straddle them
    shapes = shape(gpu, pool, N, refill=refill)  # asserts peak <= cap; some blocks fall back
    assert len(shapes) == 4 and all(peak > 0 for _, peak, _ in shapes)
    run_nq(gpu, pool, N, refill=refill, what="refill")


@pytest.mark.parametrize("stack_cap", [0, 64, 100])
def test_stack_cap_forces_the_fallback(gpu, stack_cap):
    """stack_cap 0: no push is ever allowed, every child is walked. 64: pushes
    only onto an empty stack. 100: onto a stack of at most 36. The full block
    of 8-row jobs pushes far more than that, so all three fall back."""
    N = 9
    pool = root(N) * 114
    (_, peak, fb), _ = shape(gpu, pool, N, cap=stack_cap)
    assert fb > 0 and peak <= stack_cap
    if stack_cap == 0:
        assert peak == 0
    else:
        assert peak > 0  # mixed: some children were pushed, others walked
    _, (out, ctl) = run_nq(gpu, pool, N, stack_cap=stack_cap, what="fallback")
    assert out == b"" and ctl["sol"] == 114 * 352
    pool = orc.random_nq_nodes(orc.rng(13008), 78, 13)
    run_nq(gpu, pool, 13, stack_cap=stack_cap, what="fallback, mixed")


def test_chain_of_four(gpu):
    N, finish = 12, 8
    pool = orc.random_nq_nodes(orc.rng(12004), 200, N, 0, 5)
    windows = [64, 64, 64, 64]
    capacity = 200 * 21 + 64
    # the first window pops the last 64 parents: one block with jobs, stacks in use, no fallback
    ((jobs, peak, fb),) = shape(gpu, pool[-64 * 24:], N)
    assert jobs > 0 and peak > 0 and fb == 0
    a = gpu.nq_devpool_chain(pool, N, windows, 1, finish, 1, capacity, "auto", 0, -1, -1, 1)
    b = gpu.nq_devpool_chain(pool, N, windows, 1, finish, 1, capacity, "auto", 0, -1, -1, 1)
    assert a == b, "two runs differ"

    def step(p, M, tree, sol, iters, best):
        return orc.nq_step(gpu, p, N, 1, finish, 1, M, tree, sol, iters)

    exps = orc.check_chain(gpu, pool, a, windows, step, capacity=capacity, what="chain")
    assert all(e is not None for e in exps)
    assert a[-1][1]["size"] > 0 and a[-1][1]["sol"] > 0


@pytest.mark.parametrize("N,tree,sol", [(12, 856188, 14200), (14, 27358552, 365596)])
def test_whole_search(gpu, N, tree, sol):
    """From the root to the empty pool, one whole-pool iteration after the
    other, against the frozen sequential counts (tests/test_nqueens_seq.py)."""
    pool, got_tree, got_sol, iters = root(N), 0, 0, 0
    while pool:
        pool, ctl = gpu.nq_devpool_step(pool, N, 1, 8, 1, None, None, "auto", 0, -1, -1, 1)
        assert ctl["overflow"] == 0
        got_tree += ctl["tree"]
        got_sol += ctl["sol"]
        iters += 1
    assert iters == N - 8
    assert (got_tree, got_sol) == (tree, sol)


def test_stack_arguments_are_validated(gpu):
    with pytest.raises(ValueError):
        gpu.nq_devpool_step(root(9), 9, 1, 8, 1, None, None, "auto", 0, -1, -1, 2)
    with pytest.raises(ValueError):  # an explicit split keeps the split kernels
        gpu.nq_devpool_step(root(9), 9, 1, 8, 1, None, None, "auto", 0, 2, -1, 1)
    with pytest.raises(ValueError):
        gpu.nq_devpool_step(root(9), 9, 1, 8, 1, None, None, "auto", 0, -1, -1, 1,
                            gpu.NQ_STACK_CAP + 1)
