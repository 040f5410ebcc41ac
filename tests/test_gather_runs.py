"""k_gather2 by runs of count entries: the shapes a run-per-block gather can get wrong.

A gather block owns a run of R consecutive count entries (R a power of two
that divides the 256-entry presum group), returns at once when its run holds
no children, derives one pool offset per run and copies the run's non-empty
slabs; only the last block writes the control block. Every case below goes
through the existing step / chain entry points and is compared with the
pure-CPU oracle (helpers/devpool_step_oracle.py): the un-popped prefix byte
for byte, the children as a multiset, the control block field by field. The
shapes hold for every R in 4..32 (GATS_GATHER_R selects another R than the
default for a whole process):

  1. G = 313 count entries (prime: the last run is partial for any R > 1) over
     two presum groups, with and without group sums;
  2. runs that are empty while the prefix behind them is not: children only in
     entries 0, 255, 256, 100 and G - 1; an empty LAST run, which still owns
     the control block; a pool that pushes nothing at all;
  3. full slabs: every count equals the stride (1024, and 5120 for lb1_d);
  4. the per-wave geometry: stride 64, G = 1252 (four groups and a partial one);
  5. capacity exactly reached / missed by one node, through the chain;
  6. a narrow window after a wide one: stale counts beyond Gi must not be read.

Nothing here is timing- or tolerance-dependent.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_step_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

HUGE = 10 ** 9
NODE = orc.NODE
N = 16
TILE = 1024       # child slots per count entry, thread-per-child geometry
PER_ENTRY = TILE // N  # 64 parents per count entry at N = 16
N1 = 20000        # shape 1: ceil(20000 * 16 / 1024) = 313 count entries

_cache = {}


def shape1_pool():
    if "pool1" not in _cache:
        _cache["pool1"] = orc.random_nq_nodes(orc.rng(313), N1, N)
    return _cache["pool1"]


def shape1_step(core):
    """Oracle of shape 1 (one step, M = size), computed once."""
    if "exp1" not in _cache:
        _cache["exp1"] = orc.nq_step(core, shape1_pool(), N, 1, 3, 1, N1)
    return _cache["exp1"]


def nq_stepfn(core, finish):
    def step(pool, M, tree, sol, iters, best):
        key = ("nq", finish, pool, M, tree, sol, iters)
        if key not in _cache:
            _cache[key] = orc.nq_step(core, pool, N, 1, finish, 1, M, tree, sol, iters)
        return _cache[key]
    return step


# ---------------------------------------------------------------------------
# 1. tail run and two groups
# ---------------------------------------------------------------------------

def test_nq_tail_run_two_groups(gpu):
    pool = shape1_pool()
    assert gpu.devpool_grid(N1, N, 1) == 313
    exp = shape1_step(gpu)
    assert len(exp.children) > 0
    outs = {}
    for presum in ("on", "off", "auto"):
        a = gpu.nq_devpool_step(pool, N, 1, 3, 1, N1, None, presum)
        b = gpu.nq_devpool_step(pool, N, 1, 3, 1, N1, None, presum)
        assert a == b, (presum, "two runs differ")
        orc.check_step(exp, a[0], a[1], ("shape 1", presum))
        outs[presum] = a
    assert outs["on"] == outs["off"] == outs["auto"], "pool bytes depend on the prefix path"


# ---------------------------------------------------------------------------
# 2. empty runs with a non-zero prefix behind them
# ---------------------------------------------------------------------------

def pushing_parent(core, rng):
    """A depth-2 parent with at least one safe child (pushed at finish = 8)."""
    while True:
        node = orc.random_nq_nodes(rng, 1, N, 2, 2)
        if orc.nq_step(core, node, N, 1, 8).children:
            return node


def sparse_pool(core, entries):
    """N1 depth-7 parents (children are all finished in-kernel at finish = 8)
    with one pushing depth-2 parent planted in each count entry of `entries`."""
    rng = orc.rng(77)
    pool = bytearray(orc.random_nq_nodes(rng, N1, N, 7, 7))
    for k, e in enumerate(entries):
        pid = min(e * PER_ENTRY + 7 * k % PER_ENTRY, N1 - 1)
        assert pid // PER_ENTRY == e
        pool[pid * NODE:(pid + 1) * NODE] = pushing_parent(core, rng)
    return bytes(pool)


@pytest.mark.parametrize("entries", [(0, 255, 256, 100, 312), (0, 255, 256, 100), ()],
                         ids=["last-entry-full", "last-run-empty", "nothing-pushed"])
def test_nq_empty_runs(gpu, entries):
    pool = sparse_pool(gpu, entries)
    exp = orc.nq_step(gpu, pool, N, 1, 8, 1, N1)
    # the pool has the shape it names: only the planted parents push
    planted = sum(len(orc.nq_step(gpu, pool[p * NODE:(p + 1) * NODE], N, 1, 8).children)
                  for p in range(N1) if pool[p * NODE] == 2)
    assert len(exp.children) == planted and (planted > 0) == bool(entries)
    assert exp.ctl["tree"] > planted and exp.ctl["size"] == planted
    for presum in ("auto", "off"):
        a = gpu.nq_devpool_step(pool, N, 1, 8, 1, N1, None, presum)
        b = gpu.nq_devpool_step(pool, N, 1, 8, 1, N1, None, presum)
        assert a == b, (entries, presum, "two runs differ")
        orc.check_step(exp, a[0], a[1], ("sparse", entries, presum))


# ---------------------------------------------------------------------------
# 3. full slabs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("lb,presum,G", [("lb1", "auto", 274), ("lb1_d", "on", 55),
                                         ("lb1_d", "off", 55)])
def test_pfsp_full_slabs(gpu, lb, presum, G):
    n = 14000
    pool = orc.pfsp_node(0, list(range(20))) * n
    geom = 1 if lb == "lb1" else 0
    assert gpu.devpool_grid(n, 20, geom) == G
    key = ("full", lb)
    if key not in _cache:
        _cache[key] = orc.pfsp_step(gpu, pool, 14, lb, HUGE, 1, n)
    exp = _cache[key]
    assert len(exp.children) == 20 * n  # every slot survives: counts equal the stride
    a = gpu.pfsp_devpool_step(pool, 14, lb, HUGE, 1, n, None, -1, presum)
    b = gpu.pfsp_devpool_step(pool, 14, lb, HUGE, 1, n, None, -1, presum)
    assert a == b, (lb, presum, "two runs differ")
    orc.check_step(exp, a[0], a[1], ("full slabs", lb, presum))


# ---------------------------------------------------------------------------
# 4. per-wave geometry
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("presum", ["on", "auto"])
def test_pfsp_per_wave_geometry(gpu, presum):
    n = 4000
    assert gpu.devpool_grid(n, 20, 2) == 1252 and gpu.devpool_stride(2) == 64
    best = gpu.taillard_best_ub(14)  # the optimum: no leaf lowers it, pruning is deterministic
    if "wave" not in _cache:
        pool = orc.random_pfsp_nodes(orc.rng(1252), n)
        _cache["wave"] = (pool, orc.pfsp_step(gpu, pool, 14, "lb2", best, 1, n))
    pool, exp = _cache["wave"]
    assert len(exp.children) > 0
    a = gpu.pfsp_devpool_step(pool, 14, "lb2", best, 1, n, None, 2, presum)
    b = gpu.pfsp_devpool_step(pool, 14, "lb2", best, 1, n, None, 2, presum)
    assert a == b, (presum, "two runs differ")
    orc.check_step(exp, a[0], a[1], ("per-wave", presum))


# ---------------------------------------------------------------------------
# 5. capacity edge
# ---------------------------------------------------------------------------

def test_nq_capacity_edge(gpu):
    pool = shape1_pool()
    size1 = shape1_step(gpu).ctl["size"]
    assert size1 > N1 // 2
    step = nq_stepfn(gpu, 3)

    snaps = gpu.nq_devpool_chain(pool, N, [N1], 1, 3, 1, size1, "auto")
    assert snaps[0][1]["overflow"] == 0
    orc.check_chain(gpu, pool, snaps, [N1], step, capacity=size1, what="capacity == next size")

    windows = [N1, N1]
    snaps = gpu.nq_devpool_chain(pool, N, windows, 1, 3, 1, size1 - 1, "auto")
    assert [s[1]["overflow"] for s in snaps] == [1, 1]
    for out, _ in snaps:  # base = 0: everything was popped, nothing of the prefix is left
        assert out == b""
    orc.check_chain(gpu, pool, snaps, windows, step, capacity=size1 - 1,
                    what="capacity == next size - 1")


def test_nq_capacity_edge_keeps_prefix(gpu):
    """The same edge with an un-popped prefix below the chunk: it must survive."""
    pool = shape1_pool()
    M = N1 - 3000
    exp = nq_stepfn(gpu, 3)(pool, M, 0, 0, 0, 0)
    size1 = exp.ctl["size"]
    for cap, over in ((size1, 0), (size1 - 1, 1)):
        windows = [M] if not over else [M, M]
        snaps = gpu.nq_devpool_chain(pool, N, windows, 1, 3, 1, cap, "auto")
        assert [s[1]["overflow"] for s in snaps] == [over] * len(windows)
        if over:
            for out, _ in snaps:
                assert out == pool[:3000 * NODE]
        orc.check_chain(gpu, pool, snaps, windows, nq_stepfn(gpu, 3), capacity=cap,
                        what=("prefix kept", cap))


# ---------------------------------------------------------------------------
# 6. narrow window after a wide one
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("presum", ["auto", "on"])
def test_nq_narrow_after_wide(gpu, presum):
    pool = shape1_pool()
    windows = [N1, 300, 5000, N1]
    assert gpu.devpool_grid(300, N, 1) == 5 and gpu.devpool_grid(5000, N, 1) == 79
    a = gpu.nq_devpool_chain(pool, N, windows, 1, 3, 1, None, presum)
    b = gpu.nq_devpool_chain(pool, N, windows, 1, 3, 1, None, presum)
    assert a == b, (presum, "two runs differ")
    exps = orc.check_chain(gpu, pool, a, windows, nq_stepfn(gpu, 3), what=("narrow", presum))
    assert all(e is not None and e.ctl["overflow"] == 0 for e in exps)
    assert all(len(e.children) > 0 for e in exps)
