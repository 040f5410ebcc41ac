"""The devpool kernels launched the way the ENGINES launch them.

test_gpu_devpool_step.py pins expand -> presum -> gather2 for one iteration
whose grid is clamped to the pool and whose buffers are fresh. The engine
threads differ in four ways, all covered here through nq_devpool_chain /
pfsp_devpool_chain (k eager iterations on one stream through
the problem descriptor's enqueue(), no host synchronisation in between, a snapshot of the control
block and the pool after each):

  * grids far wider than the chunk (most expand blocks start past its end,
    k_presum sums all-zero groups, k_gather2's last block sits far behind the
    last block that holds children), with the engines' own per-iteration
    presum rule ("auto" goes through the shared policy helper);
  * count / sol / extra / group-sum / child buffers allocated once for the
    largest window and reused, so a small grid follows a large one over stale
    counts and stale child slabs, and the reverse;
  * both control-block parities back to back: tree, sol, iters and best are
    carried forward, idle iterations (pool below m) change nothing, overflow
    stays set in both blocks;
  * the device-built frontiers, whose CONTENT the dist tier slices by index.

Every transition is compared exactly with the CPU oracle applied to the
previous GPU snapshot (orc.check_chain; proved to bite on the CPU in
test_devpool_step_oracle.py): the un-popped prefix byte for byte, the children
as a multiset, every control-block field. Every chain runs twice and must be
byte-identical. There is no tolerance anywhere.

Input rule for PFSP chains: ctl->best is lowered by atomicMin INSIDE an
iteration, so pruning is deterministic only if no popped chunk mixes leaf
parents (depth 19) with a best above the optimum. Every PFSP chain here uses
one of: best = optimum (no leaf of a ub=1 tree lies below it, nothing moves);
a huge best with input depth <= 19 - k, so that k iterations never pop a
depth-19 parent; or the pure-leaf chunk of orc.incumbent_pool, whose first
iteration pushes nothing and only lowers best."""
import os
import sys
from collections import Counter

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_step_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

HUGE = 10 ** 9
INSTS = [2, 14, 21]  # 20x5, 20x10, 20x20
# (lb, geom): every PFSP expand kernel; both lb2 geometries on every machine count
KERNELS = [("lb1", -1), ("lb1_d", -1), ("lb2", 3), ("lb2", 2)]
KERNEL_IDS = ["lb1", "lb1_d", "lb2-lane", "lb2-wave"]
# one kernel per geometry family: thread-per-child, thread-per-parent, per-wave
FAMILIES = [("lb1", -1), ("lb1_d", -1), ("lb2", 2)]
FAMILY_IDS = ["lb1", "lb1_d", "lb2-wave"]
WIDE = 60000  # 1172 thread-per-child blocks / 18752 wave counts at 20 children per node

_oracle_cache = {}


def nq_stepfn(core, N, g, finish, m):
    def step(pool, M, tree, sol, iters, best):
        key = ("nq", N, g, finish, m, pool, M, tree, sol, iters)
        if key not in _oracle_cache:
            _oracle_cache[key] = orc.nq_step(core, pool, N, g, finish, m, M, tree, sol, iters)
        return _oracle_cache[key]
    return step


def pfsp_stepfn(core, inst, lb, m):
    def step(pool, M, tree, sol, iters, best):
        key = ("pfsp", inst, lb, m, pool, M, tree, sol, iters, best)
        if key not in _oracle_cache:
            _oracle_cache[key] = orc.pfsp_step(core, pool, inst, lb, best, m, M, tree, sol,
                                               iters)
        return _oracle_cache[key]
    return step


def default_capacity(pool):
    return (len(pool) // 24) * 21 + 64  # the bindings' default, made explicit


def run_nq(gpu, pool, N, windows, g=1, finish=8, m=1, capacity=None, presum="auto", what=""):
    capacity = default_capacity(pool) if capacity is None else capacity
    a = gpu.nq_devpool_chain(pool, N, windows, g, finish, m, capacity, presum)
    b = gpu.nq_devpool_chain(pool, N, windows, g, finish, m, capacity, presum)
    what = ("nq", what, "N", N, "n", len(pool) // 24, "g", g, "finish", finish, "m", m,
            "windows", windows, "capacity", capacity, presum)
    assert a == b, (what, "two runs differ")
    exps = orc.check_chain(gpu, pool, a, windows, nq_stepfn(gpu, N, g, finish, m),
                           capacity=capacity, what=what)
    return exps, a


def run_pfsp(gpu, pool, inst, lb, best, windows, m=1, capacity=None, geom=-1, presum="auto",
             what=""):
    capacity = default_capacity(pool) if capacity is None else capacity
    a = gpu.pfsp_devpool_chain(pool, inst, lb, best, windows, m, capacity, geom, presum)
    b = gpu.pfsp_devpool_chain(pool, inst, lb, best, windows, m, capacity, geom, presum)
    what = ("pfsp", what, "inst", inst, lb, "geom", geom, "n", len(pool) // 24, "best", best,
            "m", m, "windows", windows, "capacity", capacity, presum)
    assert a == b, (what, "two runs differ")
    exps = orc.check_chain(gpu, pool, a, windows, pfsp_stepfn(gpu, inst, lb, m), best=best,
                           capacity=capacity, what=what)
    return exps, a


def wide_cases(n):
    """(window, presum) pairs of the one-iteration wide-grid cases."""
    return [(n + 1, "auto"), (20 * n, "auto"), (WIDE, "auto"), (WIDE, "on"), (WIDE, "off")]


def assert_idle(pool_in, ctl_in, snap, what):
    """An iteration over a pool below m: chunk 0 and nothing else moves."""
    pool_out, ctl = snap
    assert pool_out == pool_in, (what, "pool changed by an idle iteration")
    assert ctl == dict(ctl_in, chunk=0), (what, ctl, ctl_in)


# ---------------------------------------------------------------------------
# a. one iteration, grid much wider than the chunk
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("N", [5, 12, 20])
def test_nq_wide_grid(gpu, N, g):
    # the engines' presum rule switches on at N = 20 only (1172 > 1024 blocks)
    assert (gpu.devpool_grid(WIDE, N, 1) > 1024) == (N == 20)
    rng = orc.rng(2000 + N)
    for n in (1, 52, 257):
        pool = orc.random_nq_nodes(rng, n, N)
        for finish in (-1, 8):
            for W, presum in wide_cases(n):
                exps, snaps = run_nq(gpu, pool, N, [W], g=g, finish=finish, presum=presum)
                assert snaps[0][1]["chunk"] == n  # the oracle pops all n
            # pool below m under the wide grid: nothing may change
            _, snaps = run_nq(gpu, pool, N, [WIDE], g=g, finish=finish, m=n + 1)
            assert_idle(pool, dict(size=n, chunk=0, tree=0, sol=0, iters=0, best=0, overflow=0),
                        snaps[0], ("nq idle", N, n))


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("inst", INSTS)
def test_pfsp_wide_grid(gpu, inst, kernel):
    lb, geom = kernel
    opt = gpu.taillard_best_ub(inst)
    rng = orc.rng(inst * 1000 + 7)
    for n in (1, 52, 257):
        # k = 1: depth <= 18 under a huge incumbent (see the module docstring)
        pools = [(opt, orc.random_pfsp_nodes(rng, n)),
                 (HUGE, orc.random_pfsp_nodes(rng, n, max_depth=18))]
        for best, pool in pools:
            for W, presum in wide_cases(n):
                exps, snaps = run_pfsp(gpu, pool, inst, lb, best, [W], geom=geom, presum=presum)
                assert snaps[0][1]["chunk"] == n
            _, snaps = run_pfsp(gpu, pool, inst, lb, best, [WIDE], m=n + 1, geom=geom)
            assert_idle(pool, dict(size=n, chunk=0, tree=0, sol=0, iters=0, best=best,
                                   overflow=0), snaps[0], ("pfsp idle", inst, lb, n))


# ---------------------------------------------------------------------------
# b. growth chains with the loop driver's windows
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("finish", [-1, 8])
@pytest.mark.parametrize("k", [4, 5])  # the live block ends on parity 0 and on parity 1
def test_nq_growth_chain(gpu, k, finish):
    N = 12
    pool = orc.random_nq_nodes(orc.rng(40), 40, N, max_depth=3)
    windows = orc.loop_windows(40, N, 1000, k)
    assert windows == [40, 480, 1000, 1000, 1000][:k]
    exps, snaps = run_nq(gpu, pool, N, windows, finish=finish, capacity=1 << 15)
    sizes = [c["size"] for _, c in snaps]
    assert [c["iters"] for _, c in snaps] == list(range(1, k + 1))
    if finish == -1:  # every safe child is pushed: the pool outgrows the window
        assert sizes[-1] > 1000
        assert all(e.prefix for e in exps[3:])
    assert all(c["tree"] > p["tree"] for (_, p), (_, c) in zip(snaps, snaps[1:]))


def test_nq_growth_chain_n20(gpu):
    N = 20
    pool = orc.random_nq_nodes(orc.rng(13), 13, N, max_depth=2)
    windows = orc.loop_windows(13, N, 300, 5)
    assert windows == [13, 260, 300, 300, 300]
    for g in (1, 3):
        exps, snaps = run_nq(gpu, pool, N, windows, g=g, capacity=1 << 16)
        assert snaps[-1][1]["iters"] == 5 and snaps[-1][1]["size"] > 300


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("inst", [14, 21])
def test_pfsp_growth_chain_from_root(gpu, inst, kernel):
    lb, geom = kernel
    opt = gpu.taillard_best_ub(inst)
    windows = orc.loop_windows(1, 20, 400, 6)
    assert windows == [1, 20, 400, 400, 400, 400]
    exps, snaps = run_pfsp(gpu, orc.pfsp_node(0, range(20)), inst, lb, opt, windows, geom=geom,
                           capacity=1 << 15)
    assert [c["iters"] for _, c in snaps] == [1, 2, 3, 4, 5, 6]
    assert all(c["best"] == opt and c["sol"] == 0 for _, c in snaps)
    assert snaps[-1][1]["tree"] > snaps[2][1]["tree"] > 20


# ---------------------------------------------------------------------------
# c. large and small grids alternating over the same buffers
# ---------------------------------------------------------------------------

ALTERNATING = [WIDE, 7, WIDE, 1, 300]


@pytest.mark.parametrize("g", [1, 3])
def test_nq_alternating_grids(gpu, g):
    N = 12
    pool = orc.random_nq_nodes(orc.rng(300), 300, N)
    for finish in (-1, 8):
        for presum in ("auto", "on", "off"):
            exps, snaps = run_nq(gpu, pool, N, ALTERNATING, g=g, finish=finish, presum=presum,
                                 capacity=1 << 16)
            assert [c["chunk"] for _, c in snaps][1::2] == [7, 1]
            assert snaps[0][1]["chunk"] == 300


@pytest.mark.parametrize("kernel", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("inst", INSTS)
def test_pfsp_alternating_grids(gpu, inst, kernel):
    lb, geom = kernel
    opt = gpu.taillard_best_ub(inst)
    pool = orc.random_pfsp_nodes(orc.rng(inst + 300), 300)
    for presum in ("auto", "on", "off"):
        exps, snaps = run_pfsp(gpu, pool, inst, lb, opt, ALTERNATING, geom=geom, presum=presum,
                               capacity=1 << 16)
        assert snaps[0][1]["chunk"] == 300
        assert all(c["best"] == opt for _, c in snaps)


# ---------------------------------------------------------------------------
# d. draining and idling
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("W", [100, 50000])
def test_nq_drain_then_idle(gpu, W):
    # N = 8, finish = 8: the finisher swallows every child, the pool only shrinks
    N, n, m = 8, 310, 25
    pool = orc.random_nq_nodes(orc.rng(310), n, N, max_depth=7)
    exps, snaps = run_nq(gpu, pool, N, [W] * 6, finish=8, m=m)
    sizes = [c["size"] for _, c in snaps]
    live = 3 if W == 100 else 1
    assert sizes == ([210, 110, 10, 10, 10, 10] if W == 100 else [0] * 6)
    assert [c["iters"] for _, c in snaps] == list(range(1, live + 1)) + [live] * (6 - live)
    assert [c["chunk"] for _, c in snaps] == [min(W, n)] * live + [0] * (6 - live)
    for i in range(live, 6):
        assert_idle(snaps[live - 1][0], snaps[live - 1][1], snaps[i], ("drain", W, i))
    if W == 100:
        assert snaps[5][0] == pool[:10 * 24]  # the 10 leftover nodes, untouched


@pytest.mark.parametrize("kernel", FAMILIES, ids=FAMILY_IDS)
def test_pfsp_idle_keeps_best(gpu, kernel):
    # the idle path also carries best through both blocks
    lb, geom = kernel
    inst = 14
    opt = gpu.taillard_best_ub(inst)
    pool = orc.random_pfsp_nodes(orc.rng(77), 24)
    for W in (24, WIDE):
        _, snaps = run_pfsp(gpu, pool, inst, lb, opt, [W] * 3, m=25, geom=geom)
        ctl0 = dict(size=24, chunk=0, tree=0, sol=0, iters=0, best=opt, overflow=0)
        for i in range(3):
            assert_idle(pool, ctl0, snaps[i], ("pfsp idle chain", lb, W, i))


# ---------------------------------------------------------------------------
# e. incumbent carried forward
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("inst", INSTS)
def test_pfsp_incumbent_carried_forward(gpu, inst, kernel):
    lb, geom = kernel
    opt = gpu.taillard_best_ub(inst)
    best0 = opt + 200
    pool = orc.incumbent_pool(inst)
    exps, snaps = run_pfsp(gpu, pool, inst, lb, best0, [64, 64], geom=geom)
    (_, c0), (_, c1) = snaps
    assert (c0["size"], c0["sol"], c0["tree"]) == (300, 64, 0)
    assert c1["best"] == c0["best"] < best0
    assert c0["best"] == {2: 1366, 14: 1398, 21: 2388}[inst]
    # a stale incumbent cannot pass: it keeps strictly more children
    stale = orc.pfsp_step(gpu, snaps[0][0], inst, lb, best0, 1, 64)
    assert len(stale.children) > len(exps[1].children)


# ---------------------------------------------------------------------------
# f. sticky overflow
# ---------------------------------------------------------------------------

def test_nq_overflow_is_sticky(gpu):
    N, n, M = 12, 100, 60  # test_nq_overflow_flag's input
    pool = orc.random_nq_nodes(orc.rng(8), n, N, max_depth=2)
    for g in (1, 3):
        exps, snaps = run_nq(gpu, pool, N, [M] * 3, g=g, finish=-1, capacity=n)
        assert len(exps[0].children) > M
        assert [c["overflow"] for _, c in snaps] == [1, 1, 1]  # so in both blocks
        assert all(p == pool[:(n - M) * 24] for p, _ in snaps)
    # a wide grid over the flagged block
    exps, snaps = run_nq(gpu, pool, N, [M, WIDE, 7], finish=-1, capacity=n)
    assert [c["overflow"] for _, c in snaps] == [1, 1, 1]
    # exact fit is no overflow, and the chain goes on
    fit = n - M + len(exps[0].children)
    exps, snaps = run_nq(gpu, pool, N, [M, 1], finish=-1, capacity=fit + 12)
    assert [c["overflow"] for _, c in snaps] == [0, 0]


@pytest.mark.parametrize("kernel", [("lb1", -1), ("lb2", 2)], ids=["lb1", "lb2-wave"])
def test_pfsp_overflow_is_sticky(gpu, kernel):
    lb, geom = kernel
    inst, n, M = 2, 100, 60  # test_pfsp_overflow_flag's input
    pool = orc.random_pfsp_nodes(orc.rng(9), n, max_depth=10)
    exps, snaps = run_pfsp(gpu, pool, inst, lb, HUGE, [M] * 3, geom=geom, capacity=n)
    assert len(exps[0].children) > M
    assert [c["overflow"] for _, c in snaps] == [1, 1, 1]
    assert all(p == pool[:(n - M) * 24] for p, _ in snaps)
    assert all(c["best"] == HUGE for _, c in snaps)


# ---------------------------------------------------------------------------
# g. the device-built frontiers vs the level-synchronous oracle
# ---------------------------------------------------------------------------

def bfs_levels(step, root, target, best=0):
    """Iterate the oracle from the root with m = 1, M = target (every level
    pops the whole pool) up to the first level that reaches the target or
    dies out. Returns (pool, ctl, sizes)."""
    pool, ctl, sizes = root, dict(tree=0, sol=0, iters=0, best=best, size=1), []
    while 0 < len(pool) // 24 < target:
        s = step(pool, target, ctl["tree"], ctl["sol"], ctl["iters"], ctl["best"])
        assert s.prefix == b""
        pool, ctl = s.pool(), s.ctl
        sizes.append(ctl["size"])
    return pool, ctl, sizes


def keys(buf, key):
    return Counter(buf[i:i + key] for i in range(0, len(buf), 24))


@pytest.mark.parametrize("N,target,sizes", [(13, 4096, [13, 132, 1030, 6404]),
                                            (12, 300, [12, 110, 756])])
def test_nq_gpu_frontier_content(gpu, monkeypatch, N, target, sizes):
    monkeypatch.delenv("GATS_NQ_FINISH", raising=False)
    pool, ctl, got_sizes = bfs_levels(nq_stepfn(gpu, N, 1, 8, 1), orc.nq_node(0, range(20)),
                                      target)
    assert got_sizes == sizes
    a = gpu.nq_gpu_frontier(N, 1, target)
    assert a == gpu.nq_gpu_frontier(N, 1, target)
    nodes, tree, sol = a
    assert (tree, sol) == (ctl["tree"], ctl["sol"])
    assert len(nodes) == sizes[-1] * 24
    assert keys(nodes, orc.NQ_KEY) == keys(pool, orc.NQ_KEY)


def test_nq_gpu_frontier_exhausts(gpu, monkeypatch):
    monkeypatch.delenv("GATS_NQ_FINISH", raising=False)
    pool, ctl, _ = bfs_levels(nq_stepfn(gpu, 8, 1, 8, 1), orc.nq_node(0, range(20)), 1 << 20)
    assert (pool, ctl["tree"], ctl["sol"]) == (b"", 2056, 92)
    assert gpu.nq_gpu_frontier(8, 1, 1 << 20) == (b"", 2056, 92)


@pytest.mark.parametrize("inst,lb,target", [(14, "lb1", 2048), (14, "lb1_d", 2048),
                                            (14, "lb2", 2048), (21, "lb2", 300),
                                            (2, "lb2", 300)])
def test_pfsp_gpu_frontier_content(gpu, inst, lb, target):
    opt = gpu.taillard_best_ub(inst)
    pool, ctl, sizes = bfs_levels(pfsp_stepfn(gpu, inst, lb, 1), orc.pfsp_node(0, range(20)),
                                  target, best=opt)
    a = gpu.pfsp_gpu_frontier(inst, lb, 1, target)
    assert a == gpu.pfsp_gpu_frontier(inst, lb, 1, target)
    nodes, tree, sol, best = a
    assert (tree, sol, best) == (ctl["tree"], ctl["sol"], ctl["best"])
    assert best == opt
    assert keys(nodes, orc.PFSP_KEY) == keys(pool, orc.PFSP_KEY)
    if inst == 2:  # exhausts below the target
        assert (nodes, tree) == (b"", 7)
    else:
        assert len(nodes) // 24 == sizes[-1] >= target
