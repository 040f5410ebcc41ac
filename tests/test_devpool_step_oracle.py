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
