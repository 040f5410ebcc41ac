"""The single-iteration devpool oracle (helpers/devpool_step_oracle.py) proved
on the CPU: iterated from the root to exhaustion it must reproduce the frozen
sequential counts for every finisher setting and chunk window. Also the
host-side input validation of nq_devpool_step / pfsp_devpool_step, which runs
before the first HIP call and therefore needs no GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_step_oracle as orc  # noqa: E402

NQ_ROOT = orc.nq_node(0, range(20))
PFSP_ROOT = orc.pfsp_node(0, range(20))


@pytest.mark.parametrize("M", [7, 50000])
@pytest.mark.parametrize("finish", [-1, 0, 3, 8])
@pytest.mark.parametrize("N", [8, 10])
def test_nq_oracle_exhaustion_equals_seq(core, N, finish, M):
    seq = core.nqueens_seq(N, 1)
    pool, tree, sol, iters = NQ_ROOT, 0, 0, 0
    while pool:
        s = orc.nq_step(core, pool, N, 1, finish, 1, M, tree, sol, iters)
        assert s.ctl["iters"] == iters + 1 and s.ctl["chunk"] == min(len(pool) // 24, M)
        pool, tree, sol, iters = s.pool(), s.ctl["tree"], s.ctl["sol"], s.ctl["iters"]
    assert (tree, sol) == (seq["tree"], seq["sol"])


# the smallest ub=1 trees frozen in tests/test_pfsp_seq.py, one per bound
@pytest.mark.parametrize("M", [7, 50000])
@pytest.mark.parametrize("inst,lb,tree,sol", [(2, "lb1", 30, 0), (2, "lb1_d", 30, 0),
                                              (2, "lb2", 7, 0)])
def test_pfsp_oracle_exhaustion_equals_seq(core, inst, lb, tree, sol, M):
    best = core.taillard_best_ub(inst)
    pool, t, s_, iters = PFSP_ROOT, 0, 0, 0
    while pool:
        s = orc.pfsp_step(core, pool, inst, lb, best, 1, M, t, s_, iters)
        pool, t, s_, iters, best = s.pool(), s.ctl["tree"], s.ctl["sol"], s.ctl["iters"], \
            s.ctl["best"]
    assert (t, s_) == (tree, sol)
    assert best == core.taillard_best_ub(inst)
    r = core.pfsp_seq(inst, lb, 1)
    assert (t, s_) == (r["tree"], r["sol"])


def test_oracle_pop_rule():
    assert orc.pop_rule(10, 11, 10) == (0, 10)  # size < m: nothing popped
    assert orc.pop_rule(10, 10, 10) == (10, 0)
    assert orc.pop_rule(10, 1, 7) == (7, 3)
    assert orc.pop_rule(0, 1, 5) == (0, 0)


# ---- input validation (host side, before anything is launched) ----

def _nq(depth, board):
    return orc.nq_node(depth, board)


def _pf(depth, prmu, limit1=None):
    b = bytearray(orc.pfsp_node(depth & 0xFF, prmu))
    if limit1 is not None:
        b[1] = limit1 & 0xFF
    return bytes(b)


NQ_OK = _nq(2, [1, 3, 0, 2, 4, 5])
PF_OK = _pf(3, list(range(20)))


@pytest.mark.parametrize("kwargs", [
    dict(nodes=NQ_OK[:23]),                       # length not a multiple of 24
    dict(N=3), dict(N=21), dict(N=0),             # N outside 4..20
    dict(nodes=_nq(7, range(6))),                 # depth > N
    dict(nodes=_nq(2, [1, 1, 0, 2, 4, 5])),       # duplicate entry
    dict(nodes=_nq(2, [1, 3, 0, 2, 4, 6])),       # entry >= N
    dict(nodes=NQ_OK + _nq(255, range(6))),       # second node bad
    dict(m=0), dict(m=-1), dict(M=0), dict(M=-5),
    dict(M=(1 << 31) // 6 + 1),                   # M * branching > 2^31
    dict(nodes=NQ_OK * 3, capacity=2),            # capacity < len(nodes)
    dict(finish=-2), dict(finish=9),
    dict(g=0),
    dict(presum="maybe"), dict(presum=""),
])
def test_nq_step_rejects_malformed_input(core, kwargs):
    args = dict(nodes=NQ_OK, N=6)
    args.update(kwargs)
    with pytest.raises(ValueError):
        core.nq_devpool_step(**args)


@pytest.mark.parametrize("kwargs", [
    dict(nodes=PF_OK + b"\0"),                                # length
    dict(nodes=_pf(3, [0] + list(range(19)))),                # duplicate job
    dict(nodes=_pf(3, list(range(19)) + [20])),               # job >= jobs
    dict(nodes=_pf(20, list(range(20)))),                     # depth > jobs - 1
    dict(nodes=_pf(-1, list(range(20)), limit1=-2)),          # depth < 0
    dict(nodes=_pf(3, list(range(20)), limit1=3)),            # limit1 != depth - 1
    dict(nodes=_pf(3, list(range(20)), limit1=-1)),
    dict(nodes=PF_OK + _pf(5, list(range(20)), limit1=0)),    # second node bad
    dict(m=0), dict(M=0), dict(M=(1 << 31) // 20 + 1),
    dict(nodes=PF_OK * 2, capacity=1),
    dict(geom=0), dict(geom=1), dict(geom=4),
    dict(lb="lb1", geom=2), dict(lb="lb1_d", geom=3),         # geom 2/3 are lb2 only
    dict(lb="bogus"),
    dict(presum="yes"),
    dict(inst=31), dict(inst=0),                              # 50 jobs / no such instance
])
def test_pfsp_step_rejects_malformed_input(core, kwargs):
    args = dict(nodes=PF_OK, inst=2, lb="lb2", best=1359)
    args.update(kwargs)
    with pytest.raises(ValueError):
        core.pfsp_devpool_step(**args)


# ---- chains: loop_windows, and check_chain must bite ----

def test_loop_windows():
    assert orc.loop_windows(40, 12, 1000, 4) == [40, 480, 1000, 1000]
    assert orc.loop_windows(1, 20, 400, 6) == [1, 20, 400, 400, 400, 400]
    assert orc.loop_windows(13, 20, 300, 5) == [13, 260, 300, 300, 300]
    assert orc.loop_windows(5, 4, 80, 3) == [5, 20, 80]      # cap reached exactly
    assert orc.loop_windows(5, 4, 79, 3) == [5, 20, 79]      # one below
    assert orc.loop_windows(500, 12, 100, 2) == [100, 100]   # pool above the cap
    assert orc.loop_windows(0, 12, 100, 2) == [1, 12]        # empty pool: window >= 1
    assert orc.loop_windows(7, 1, 100, 3) == [7, 7, 7]
    assert orc.loop_windows(3, 20, 1 << 19, 1) == [3]


def _nq_chain(core):
    N, windows = 8, [20, 5, 100, 100]
    pool0 = orc.random_nq_nodes(orc.rng(123), 30, N, max_depth=3)

    def step(pool, M, tree, sol, iters, best):
        return orc.nq_step(core, pool, N, 1, 2, 1, M, tree, sol, iters)
    return pool0, windows, step


def _copy(snaps):
    return [(p, dict(c)) for p, c in snaps]


def test_check_chain_accepts_the_oracle_chain(core):
    pool0, windows, step = _nq_chain(core)
    snaps = orc.oracle_chain(pool0, windows, step)
    sizes = [c["size"] for _, c in snaps]
    # the chain exercises a live prefix, growth and carried counters
    assert sizes[0] > 10 and len(set(sizes)) == len(sizes)
    assert [c["iters"] for _, c in snaps] == [1, 2, 3, 4]
    exps = orc.check_chain(core, pool0, snaps, windows, step)
    assert all(e.prefix for e in exps[:2]) and all(e.children for e in exps)
    # children in any order inside the pushed range are the same chain
    p, c = snaps[1]
    nb = len(exps[1].prefix)
    kids = [p[i:i + 24] for i in range(nb, len(p), 24)]
    snaps[1] = (p[:nb] + b"".join(reversed(kids)), c)
    orc.check_chain(core, pool0, snaps[:2], windows[:2], step)


@pytest.mark.parametrize("where", [0, 1, 2, 3])
@pytest.mark.parametrize("what", ["dropped_child", "duplicated_child", "prefix_byte", "iters",
                                  "tree", "sol", "chunk"])
def test_check_chain_raises_on_one_corruption(core, what, where):
    pool0, windows, step = _nq_chain(core)
    good = orc.oracle_chain(pool0, windows, step)
    exps = orc.check_chain(core, pool0, good, windows, step)
    snaps = _copy(good)
    p, c = snaps[where]
    nb = len(exps[where].prefix)
    if what == "dropped_child":  # the last child is missing and size says so
        p, c["size"] = p[:-24], c["size"] - 1
    elif what == "duplicated_child":  # size right, one child replaced by its neighbour
        assert p[-24:] != p[-48:-24]
        p = p[:-24] + p[-48:-24]
    elif what == "prefix_byte":
        assert nb >= 24  # every window of this chain leaves a live prefix
        b = bytearray(p)
        b[nb - 24 + 5] ^= 1  # last un-popped node, one board byte
        p = bytes(b)
    else:
        c[what] += 1
    snaps[where] = (p, c)
    with pytest.raises(AssertionError):
        orc.check_chain(core, pool0, snaps, windows, step)


@pytest.mark.parametrize("inst,lb", [(2, "lb1"), (14, "lb1"), (21, "lb1"), (14, "lb2")])
def test_check_chain_raises_on_stale_best(core, inst, lb):
    opt = core.taillard_best_ub(inst)
    best0, windows = opt + 200, [64, 64]
    pool0 = orc.incumbent_pool(inst)

    def step(pool, M, tree, sol, iters, best):
        return orc.pfsp_step(core, pool, inst, lb, best, 1, M, tree, sol, iters)
    good = orc.oracle_chain(pool0, windows, step, best=best0)
    assert good[0][1]["best"] == good[1][1]["best"] < best0
    assert good[0][1]["best"] == {2: 1366, 14: 1398, 21: 2388}[inst]
    assert (good[0][1]["size"], good[0][1]["sol"], good[0][1]["tree"]) == (300, 64, 0)
    orc.check_chain(core, pool0, good, windows, step, best=best0)
    # iteration 2 pruned with the incumbent it started from instead of the
    # one iteration 1 found: more children survive, the chain must not pass
    stale = orc.pfsp_step(core, good[0][0], inst, lb, best0, 1, 64, 0, 64, 1)
    assert len(stale.children) > good[1][1]["size"] - 236
    snaps = [good[0], (stale.pool(), dict(stale.ctl, best=good[0][1]["best"]))]
    with pytest.raises(AssertionError):
        orc.check_chain(core, pool0, snaps, windows, step, best=best0)
    # the counters right but best itself not carried into the next block
    snaps = _copy(good)
    snaps[1][1]["best"] = best0
    with pytest.raises(AssertionError):
        orc.check_chain(core, pool0, snaps, windows, step, best=best0)
    snaps = _copy(good)
    snaps[0][1]["best"] = best0
    with pytest.raises(AssertionError):
        orc.check_chain(core, pool0, snaps, windows, step, best=best0)


def test_check_chain_overflow_is_sticky(core):
    N, n, M = 12, 100, 60
    pool0 = orc.random_nq_nodes(orc.rng(8), n, N, max_depth=2)

    def step(pool, M_, tree, sol, iters, best):
        return orc.nq_step(core, pool, N, 1, -1, 1, M_, tree, sol, iters)
    windows = [M, M, M]
    good = orc.oracle_chain(pool0, windows, step, capacity=n)
    assert [c["overflow"] for _, c in good] == [1, 1, 1]
    assert all(p == pool0[:(n - M) * 24] for p, _ in good)
    orc.check_chain(core, pool0, good, windows, step, capacity=n)
    for where in (1, 2):  # flag cleared in a later snapshot
        snaps = _copy(good)
        snaps[where][1]["overflow"] = 0
        with pytest.raises(AssertionError):
            orc.check_chain(core, pool0, snaps, windows, step, capacity=n)
        with pytest.raises(AssertionError):  # also without the capacity hint
            orc.check_chain(core, pool0, snaps, windows, step)
    for where in (0, 1, 2):  # prefix touched after the overflow
        snaps = _copy(good)
        b = bytearray(snaps[where][0])
        b[-1 - 3] ^= 1
        snaps[where] = (bytes(b), snaps[where][1])
        with pytest.raises(AssertionError):
            orc.check_chain(core, pool0, snaps, windows, step, capacity=n)
    # a flag that is set although the children fit
    fits = orc.oracle_chain(pool0, windows[:1], step)
    fits[0][1]["overflow"] = 1
    with pytest.raises(AssertionError):
        orc.check_chain(core, pool0, fits, windows[:1], step, capacity=1 << 20)
    # a flag that is missing although they do not
    with pytest.raises(AssertionError):
        orc.check_chain(core, pool0, orc.oracle_chain(pool0, windows[:1], step), windows[:1],
                        step, capacity=n)


# ---- chain entry points: host validation before the first HIP call ----

@pytest.mark.parametrize("kwargs", [
    dict(nodes=NQ_OK[:23]),
    dict(N=3), dict(N=21), dict(N=0),
    dict(nodes=_nq(7, range(6))),
    dict(nodes=_nq(2, [1, 1, 0, 2, 4, 5])),
    dict(nodes=_nq(2, [1, 3, 0, 2, 4, 6])),
    dict(nodes=NQ_OK + _nq(255, range(6))),
    dict(m=0), dict(m=-1),
    dict(windows=[]), dict(windows=[5] * 17),              # 1 <= k <= 16
    dict(windows=[0]), dict(windows=[-5]), dict(windows=[5, 0, 5]),
    dict(windows=[(1 << 31) // 6 + 1]),                    # window * branching > 2^31
    dict(windows=[5, (1 << 31) // 6 + 1]),
    dict(nodes=NQ_OK * 3, capacity=2),                     # capacity < len(nodes)
    dict(capacity=(1 << 22) // 3 + 1),                     # capacity * (k + 1) > 2^22
    dict(capacity=(1 << 22) // 17 + 1, windows=[5] * 16),
    dict(capacity=-1),
    dict(finish=-2), dict(finish=9),
    dict(g=0),
    dict(presum="maybe"), dict(presum=""),
])
def test_nq_chain_rejects_malformed_input(core, kwargs):
    args = dict(nodes=NQ_OK, N=6, windows=[5, 7])
    args.update(kwargs)
    with pytest.raises(ValueError):
        core.nq_devpool_chain(**args)


@pytest.mark.parametrize("kwargs", [
    dict(nodes=PF_OK + b"\0"),
    dict(nodes=_pf(3, [0] + list(range(19)))),
    dict(nodes=_pf(3, list(range(19)) + [20])),
    dict(nodes=_pf(20, list(range(20)))),
    dict(nodes=_pf(-1, list(range(20)), limit1=-2)),
    dict(nodes=_pf(3, list(range(20)), limit1=3)),
    dict(nodes=_pf(3, list(range(20)), limit1=-1)),
    dict(nodes=PF_OK + _pf(5, list(range(20)), limit1=0)),
    dict(m=0), dict(m=-1),
    dict(windows=[]), dict(windows=[5] * 17),
    dict(windows=[0]), dict(windows=[-5]), dict(windows=[5, 0, 5]),
    dict(windows=[(1 << 31) // 20 + 1]),
    dict(windows=[5, (1 << 31) // 20 + 1]),
    dict(nodes=PF_OK * 2, capacity=1),
    dict(capacity=(1 << 22) // 3 + 1),
    dict(capacity=(1 << 22) // 17 + 1, windows=[5] * 16),
    dict(capacity=-1),
    dict(geom=0), dict(geom=1), dict(geom=4),
    dict(lb="lb1", geom=2), dict(lb="lb1_d", geom=3),
    dict(lb="bogus"),
    dict(presum="yes"),
    dict(inst=31), dict(inst=0),
])
def test_pfsp_chain_rejects_malformed_input(core, kwargs):
    args = dict(nodes=PF_OK, inst=2, lb="lb2", best=1359, windows=[5, 7])
    args.update(kwargs)
    with pytest.raises(ValueError):
        core.pfsp_devpool_chain(**args)
