"""Half-pool DONATION between the slice threads of one device, step by step.

Every default devpool search balances its slice threads through SliceShare
(src/slice_share.hpp): a drained thread waits, a running thread carves the back
half of its live device pool at a readback, publishes it with its incumbent and
blocks until the thief's device-to-device copy acks. The engine tests see that
only through whole-search totals, and only if a donation happens to fire.

nq_devpool_share / pfsp_devpool_share run 2..4 real slice threads over ONE
SliceShare, one shared incumbent and one slice holding all the nodes, and
return one trace per thread; `donate_floor` and `await_idle_ms` make a
donation certain in a search of a few milliseconds (thread 0 runs the slice;
at a readback at or above the floor it waits, bounded, until every other
thread is waiting or running). The protocol itself, with its withdraw and
deadline paths, is pinned on the CPU (tests/test_slice_share.py).

Which readback donates, and to whom, is a race: orc.check_share holds for every
outcome and is symmetric in the threads. It asserts, per thread, every loop
rule and conservation at every readback (donated nodes count as still to do,
taken nodes as the job's own pool), per DONATE the floor, the bytes moved (the
back half of the snapshot before), the sizes, the kept front in the next
batch and the offered incumbent, per taken DONATE exactly one TAKE in another
thread with the same bytes and incumbent and a run starting at or below it, and
at the end device totals + a CPU search of all leftovers == the CPU total.
Every case runs twice: the traces may differ, the checks and totals may not.
Where a case claims a donation it asserts a taken DONATE in the traces.

The inputs are orc.SHARE_CASES; tests/test_devpool_loop_oracle.py proves on
the CPU that each pool reaches its floor with a factor 2 of slack (or exactly,
at the real floor's edge), and that check_share bites."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_loop_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

NODE = orc.NODE
_cache = {}


def prepared(gpu, name):
    """(case, pool, bfs tree, bfs sol, seq cache): computed once per case and
    never modified."""
    if name not in _cache:
        c = orc.SHARE_CASES[name]
        pool, t0, s0 = orc.share_case_pool(gpu, c)
        _cache[name] = (c, pool, t0, s0, orc.case_seq(gpu, c) if c.fixed_best else None)
    return _cache[name]


def run_twice(gpu, name):
    c, pool, t0, s0, seq = prepared(gpu, name)
    res = []
    for rep in range(2):
        outs = orc.run_share_case(gpu, c, pool)
        assert len(outs) == c.threads
        n = orc.share_counts(outs)
        print(name, "run", rep, n, [(o["tree"], o["sol"], o["best"]) for o in outs])
        total = orc.check_share(outs, pool, seq, c.cfg())
        if c.whole_tree is not None:  # the frozen sequential counts
            assert (t0 + total[0], s0 + total[1]) == c.whole_tree
        orc.check_need({k: v for k, v in n.items()}, {k: v for k, v in c.need.items()
                                                      if k != "at_floor"})
        if c.need.get("taken"):
            assert n["taken"] >= 1 and n["withdrawn"] == 0
        res.append((outs, n, total))
    assert res[0][2] == res[1][2]
    return res


# ---- N-Queens, small floor ----

@pytest.mark.parametrize("finish", [-1, 3, 8])
@pytest.mark.parametrize("pool", ["mixed", "root"])
def test_nq_small_floor(gpu, pool, finish):
    run_twice(gpu, "%s_nq_f%d" % (pool, finish))


# ---- three threads: successive donations, a thief that donates itself ----

def test_three_threads(gpu):
    for outs, n, _ in run_twice(gpu, "three_nq"):
        # both other threads were served, and a taken half was split again
        assert n["thieves"] >= 2 and n["chains"] >= 1, n


# ---- the real floor ----

def test_real_floor_edge_donates_exactly_once(gpu):
    c = orc.SHARE_CASES["edge_nq"]
    for outs, n, _ in run_twice(gpu, "edge_nq"):
        assert n["taken"] == 1 and n["takes"] == 1, n
        (d,) = orc.donations_of(outs)
        assert d["size_before"] == orc.REAL_FLOOR and d["size_after"] == orc.REAL_FLOOR // 2
        assert len(d["moved"]) == (orc.REAL_FLOOR // 2) * NODE
        # the first readback, after b = 16 iterations of 64 leaf parents each
        owner = next(o for o in outs if o["trace"] and o["trace"][0]["kind"] == "run")
        assert owner["trace"][1]["b"] == orc.BATCH
        assert owner["trace"][1]["ctl"]["size"] == orc.REAL_FLOOR and owner["trace"][2] is d
        assert c.floor == 0


def test_one_node_below_the_real_floor_never_donates(gpu):
    for outs, n, _ in run_twice(gpu, "below_edge_nq"):
        assert n["taken"] == n["withdrawn"] == n["takes"] == 0 and n["idle_threads"] == 1, n
        owner = next(o for o in outs if o["trace"])
        assert owner["trace"][1]["ctl"]["size"] == orc.REAL_FLOOR - 1


def test_real_floor_with_work_in_the_donated_half(gpu):
    for outs, n, _ in run_twice(gpu, "deep_nq"):
        assert all(o["tree"] > 0 for o in outs), "both threads count some of it"


def test_two_m_branch_of_the_floor(gpu):
    c = orc.SHARE_CASES["two_m_nq"]
    for outs, n, _ in run_twice(gpu, "two_m_nq"):
        assert n["taken"] == 1, n
        (d,) = orc.donations_of(outs)
        assert d["size_before"] == 2 * c.m and d["size_after"] == c.m
    # one node fewer: above 65536, below 2m
    for outs, n, _ in run_twice(gpu, "below_two_m_nq"):
        assert n["taken"] == n["withdrawn"] == 0, n
        owner = next(o for o in outs if o["trace"])
        assert orc.REAL_FLOOR <= owner["trace"][1]["ctl"]["size"] == 2 * c.m - 1


# ---- a donation next to spills ----

def test_donation_next_to_a_spill(gpu):
    for outs, n, _ in run_twice(gpu, "spill_nq"):
        before = after = 0
        for o in outs:
            kinds = [(r["kind"], r.get("taken")) for r in o["trace"]]
            dons = [i for i, k in enumerate(kinds) if k == ("donate", True)]
            spills = [i for i, k in enumerate(kinds) if k[0] == "spill"]
            before += any(s < d for s in spills for d in dons)
            after += any(s > d for s in spills for d in dons)
        print("threads with a spill before / after a donation:", before, after)
        # after: arithmetic (the kept front of the first readback's pool leaves
        # room for less than one worst-case iteration)
        assert after >= 1 and before >= 1, (before, after, n)


# ---- PFSP ----

def test_pfsp_lb1_d_counts_with_the_incumbent_at_the_optimum(gpu):
    opt = gpu.taillard_best_ub(14)
    for outs, n, _ in run_twice(gpu, "lb1_d"):
        assert all(o["best"] == opt for o in outs)


def test_pfsp_lb1_d_incumbent_travels_with_the_donation(gpu):
    c = orc.SHARE_CASES["lb1_d_open"]
    opt = gpu.taillard_best_ub(c.inst)
    for outs, n, _ in run_twice(gpu, "lb1_d_open"):
        # the donor had found a better incumbent than it started from
        for d in orc.donations_of(outs, True):
            assert opt <= d["best"] < opt + c.best_delta, d["best"]
        for o in outs:
            for take, recs in orc.jobs_of(o["trace"]):
                if take is not None:
                    assert recs[0]["best"] <= take["best"] < opt + c.best_delta
        assert min(o["best"] for o in outs) == opt


def test_pfsp_lb2_four_threads(gpu):
    opt = gpu.taillard_best_ub(14)
    for outs, n, _ in run_twice(gpu, "lb2_four"):
        assert all(o["best"] == opt for o in outs)


# ---- no donation wanted ----

def test_pool_below_the_floor_never_donates(gpu):
    for outs, n, _ in run_twice(gpu, "small_nq"):
        assert n["taken"] == n["withdrawn"] == n["takes"] == 0 and n["idle_threads"] == 1, n


def test_one_batch_then_leftovers(gpu):
    c = orc.SHARE_CASES["one_batch_nq"]
    for outs, n, _ in run_twice(gpu, "one_batch_nq"):
        assert n["taken"] == n["takes"] == 0 and n["batches"] == 1 and n["idle_threads"] == 1, n
        assert sum(len(o["leftover"]) for o in outs) // NODE >= c.m
