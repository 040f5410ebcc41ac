"""The devpool LOOP DRIVER, batch by batch.

The step and chain tests pin the kernels; the engine tests compare whole
searches with the sequential totals. In between sits the driver:
run_devpool_loop plus run_pool / spill / drain_spilled / the leftover copy of
the slice thread. It decides how many blind iterations to launch, which of the
two control blocks is live, when a captured graph is replayed, when half the
pool goes to the host and what is re-run afterwards.

nq_devpool_loop / pfsp_devpool_loop run ONE slice through the real slice
thread with the chunk cap, capacity and graph switch given as arguments and
return the driver's trace. Every test asserts

  1. every decision rule (orc.check_trace) and conservation at EVERY readback
     (orc.check_conservation: counted + a CPU search of the snapshot, of the
     spilled stack and of the leftovers == the input pool's CPU total; every
     spill moved exactly the back half of the previous snapshot), and the
     final totals + a CPU finish of the leftovers (orc.check_final);
  2. that the trace shows the path the test is named after (Case.need).

The inputs live in helpers/devpool_loop_oracle.py (CASES);
tests/test_devpool_loop_oracle.py proves on the CPU model that each reaches
its path with a factor 2 of slack, and that the checkers bite.

Not reachable, by the driver's own arithmetic: a graph replay BEFORE the first
spill of the same run. A replay needs room for 16 worst-case iterations
(16 * chunk * per nodes), a spill room for less than one, so the pool would
have to grow by 15 * chunk * per between them. A depth-first pool exceeds its
un-popped base by at most chunk * sum over levels of (children - 1), which is
below 10 * chunk * per for every problem here (PFSP: 190 < 300). The reverse
order is reachable and tested: spill_then_graph_nq spills first and replays a
graph in the run that drains the spilled half."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_loop_oracle as orc  # noqa: E402
import devpool_step_oracle as step  # noqa: E402

pytestmark = pytest.mark.gpu

_cache = {}


def prepared(gpu, name):
    """(case, pool, bfs tree, bfs sol, seq cache): computed once per case and
    never modified."""
    if name not in _cache:
        c = orc.CASES[name]
        pool, t0, s0 = orc.case_pool(gpu, c)
        _cache[name] = (c, pool, t0, s0, orc.case_seq(gpu, c))
    return _cache[name]


def run(gpu, name, graph=None):
    c, pool, _, _, _ = prepared(gpu, name)
    graph = c.graph if graph is None else graph
    if c.problem == "nq":
        return gpu.nq_devpool_loop(pool, c.N, 1, c.finish, c.m, c.chunk, c.capacity, graph,
                                   c.max_batches)
    best = gpu.taillard_best_ub(c.inst)
    lower = None if c.lower_at is None else (c.lower_at, best)
    return gpu.pfsp_devpool_loop(pool, c.inst, c.lb, best + c.best_delta, c.m, c.chunk,
                                 c.capacity, graph, c.max_batches, c.br, lower)


def run_and_check(gpu, name, graph=None, need=None):
    c, pool, t0, s0, seq = prepared(gpu, name)
    out = run(gpu, name, graph)
    cfg = c.cfg(graph)
    n = orc.case_counts(out)
    print(name, "graph" if cfg.graph else "eager", n)
    orc.check_trace(out, cfg, len(pool) // orc.NODE)
    total = orc.check_conservation(out, pool, seq, cfg)
    orc.check_final(out, seq, total)
    if c.whole_tree is not None:  # the frozen sequential counts
        assert (t0 + total[0], s0 + total[1]) == c.whole_tree
    if c.problem == "pfsp":
        assert out["best"] == gpu.taillard_best_ub(c.inst)
    orc.check_need(n, c.need if need is None else need)
    return out, n


# ---- a. eager growth from a few nodes ----

@pytest.mark.parametrize("name", ["grow_nq", "grow_lb1"])
def test_eager_growth_from_a_few_nodes(gpu, name):
    out, n = run_and_check(gpu, name)
    c = orc.CASES[name]
    assert len(out["leftover"]) // orc.NODE < c.m
    assert n["replays"] == 0 and n["spills"] == 0 and n["runs"] == 1


# ---- b / f. graph replay ----

@pytest.mark.parametrize("name", ["graph_nq", "graph_lb12"])
def test_graph_replay(gpu, name):
    a, na = run_and_check(gpu, name)
    b, nb = run_and_check(gpu, name)
    # the totals of a bounded run depend on nothing but the input
    assert [a[f] for f in ("tree", "sol", "best", "iters")] == \
        [b[f] for f in ("tree", "sol", "best", "iters")]
    assert sorted(a["leftover"][i:i + 24] for i in range(0, len(a["leftover"]), 24)) == \
        sorted(b["leftover"][i:i + 24] for i in range(0, len(b["leftover"]), 24))
    assert na == nb
    # the same input without the graph: same rules, same conservation, no replay
    e, ne = run_and_check(gpu, name, graph=False, need={})
    assert ne["replays"] == 0 and ne["captures"] == 0


# ---- c. both parities ----

def test_batches_entered_on_parity_1(gpu):
    out, n = run_and_check(gpu, "parity_nq")
    # graph=True and full batches after the fourth, but all on control block 1
    assert n["replays"] == 0 and n["odd_b"] >= 1


# ---- d. spill ----

@pytest.mark.parametrize("name", ["spill_nq", "spill_lb1"])
def test_spill_and_drain(gpu, name):
    out, n = run_and_check(gpu, name)
    assert n["runs"] >= 2 and n["replays"] == 0


def test_spill_then_graph_in_the_drained_run(gpu):
    out, n = run_and_check(gpu, "spill_then_graph_nq")
    runs = orc.runs_of(out["trace"])
    assert runs[0][1][0]["b"] == 1 and runs[0][1][1]["kind"] == "spill"
    assert n["spills"] >= 1 and n["full_on_parity1"] >= 1


# ---- e. incumbent adoption ----

def test_incumbent_adopted_mid_loop(gpu):
    name = "adopt_lb1_d"
    c, pool, _, _, seq = prepared(gpu, name)
    opt = gpu.taillard_best_ub(c.inst)
    out = run(gpu, name)
    n = orc.case_counts(out)
    print(name, n)
    bs = orc.batches_of(out["trace"])
    k = c.lower_at
    assert len(bs) > k + 1
    # nothing on the device lowers the incumbent to the optimum before the host does
    assert all(r["ctl"]["best"] > opt for r in bs[:k + 1]), [r["ctl"]["best"] for r in bs[:k + 2]]
    assert all(r["ctl"]["best"] == opt for r in bs[k + 1:])
    assert out["best"] == opt
    orc.check_trace(out, c.cfg(), len(pool) // orc.NODE)
    # from readback k on every iteration prunes with the optimum
    total = orc.check_conservation(out, pool, seq, c.cfg(), from_batch=k)
    orc.check_final(out, seq, total)
    orc.check_need(n, c.need)
    # a stale incumbent keeps strictly more: the looser search of the same pool
    loose = gpu.pfsp_seq_from_pool(pool, c.inst, c.lb, 1, opt + c.best_delta)
    tight = gpu.pfsp_seq_from_pool(pool, c.inst, c.lb, 1, opt)
    lt, _ = seq(out["leftover"])
    assert tight["tree"] < out["tree"] + lt < loose["tree"]


# ---- g. a real overflow is the handled exit ----

def test_overflow_raises(gpu):
    # test_nq_overflow_flag's input: the first iteration's children do not fit,
    # and the first turn never spills
    N, n, M = 12, 100, 60
    pool = step.random_nq_nodes(step.rng(8), n, N, max_depth=2)
    exp = step.nq_step(gpu, pool, N, 1, -1, 1, M)
    assert exp.ctl["size"] > n
    with pytest.raises(RuntimeError, match="device pool overflow"):
        gpu.nq_devpool_loop(pool, N, 1, -1, 1, M, n, True, 4)
    # the next call starts clean
    out = gpu.nq_devpool_loop(pool, N, 1, -1, 1, M, 1 << 12, True, 1)
    assert out["trace"][1]["ctl"]["overflow"] == 0
