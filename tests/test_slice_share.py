"""Half-pool donation between slice threads: the protocol alone, on the CPU.

src/slice_share.hpp holds SliceShare, the donation floor, donate_if_wanted,
wait_for_work / ack_taken and RunnerScope with no HIP in them; the engines'
slice thread supplies the two device actions ("set the live size to x and
wait", the thief's copy). share_selftest runs the same functions on plain
threads over a fake pool (src/share_selftest.hpp; every wait there is bounded)
and reports, per donation check, the outcome, every set-size call and the
donor's size afterwards, and per claim what the thief received as
(thief, offset of src in the pool, n, best). Nothing here needs a GPU."""
import pytest

FLOOR = 1 << 16


# ---- the floor ----

@pytest.mark.parametrize("m, floor", [(1, 65536), (32767, 65536), (32768, 65536), (32769, 65538)])
def test_donation_floor(core, m, floor):
    assert core.donation_floor(m) == floor == max(2 * m, 1 << 16)


# ---- no offer: the set-size callable is never called ----

@pytest.mark.parametrize("kwargs", [
    dict(size=FLOOR - 1),              # one node below the floor
    dict(size=FLOOR, thieves=0),       # nobody waits (idle == 0)
    dict(size=FLOOR, pending=True),    # another offer is open
    dict(size=FLOOR, overflow=True),   # a torn iteration
    dict(size=99, floor=100),
])
def test_no_offer(core, kwargs):
    args = dict(scenario="basic", floor=FLOOR, thieves=1, best=77)
    args.update(kwargs)
    r = core.share_selftest(**args)
    assert r["idle_reached"]
    (o,) = r["offers"]
    assert o["outcome"] == "none" and o["set_calls"] == [] and o["size_after"] == args["size"]
    assert r["takes"] == []
    assert r["returned_false"] == args["thieves"]   # the waiter left once the runner was gone
    assert o["idle_after"] == args["thieves"]       # and was still waiting until then


# ---- one donor, one thief ----

@pytest.mark.parametrize("size, floor", [(FLOOR, FLOOR), (FLOOR + 1, FLOOR), (65538, 65538),
                                         (65539, 65538), (100, 100), (101, 2), (3, 2), (2, 2)])
def test_one_donor_one_thief(core, size, floor):
    r = core.share_selftest("basic", size=size, floor=floor, thieves=1, best=1234)
    half = size // 2
    (o,) = r["offers"]
    assert o["outcome"] == "taken"
    assert o["set_calls"] == [size - half]          # once, with the kept front
    assert o["size_after"] == size - half
    assert r["takes"] == [(0, size - half, half, 1234)]   # src = pool + (size - size / 2)
    assert r["returned_false"] == 1                 # the thief came back and found no runner


# ---- two thieves, one offer ----

def test_two_thieves_one_offer_then_a_second(core):
    size = 1001
    r = core.share_selftest("basic", size=size, floor=100, thieves=2, offers=2, best=5,
                            one_each=True)
    assert r["idle_reached"]
    o1, o2 = r["offers"]
    keep1 = size - size // 2
    keep2 = keep1 - keep1 // 2
    assert o1["outcome"] == o2["outcome"] == "taken"
    assert o1["set_calls"] == [keep1] and o2["set_calls"] == [keep2]
    assert o1["idle_after"] == 1                    # exactly one claimed, the other still waits
    t1, t2 = r["takes"]
    assert t1[1:] == (keep1, size // 2, 5) and t2[1:] == (keep2, keep1 // 2, 5)
    assert {t1[0], t2[0]} == {0, 1}                 # the second offer served the other thief
    assert o2["idle_after"] == 0 and r["returned_false"] == 0


def test_offers_in_a_row_never_overlap(core):
    # one thief that keeps coming back: every node is offered at most once
    size = 4097
    r = core.share_selftest("basic", size=size, floor=2, thieves=1, offers=12, best=1)
    seen, top = [], size
    for o, t in zip(r["offers"], r["takes"]):
        assert o["outcome"] == "taken"
        assert t[1] + t[2] == top and t[1] == o["size_after"]
        seen.append(range(t[1], t[1] + t[2]))
        top = t[1]
    assert len(r["takes"]) == 12 and top == 2       # 4097 -> 2049 -> ... -> 3 -> 2
    assert sum(len(s) for s in seen) == size - r["offers"][-1]["size_after"]


# ---- two donors, one open offer ----

def test_second_donor_returns_while_an_offer_is_open(core):
    r = core.share_selftest("two_donors", size=1000, size_b=2001, floor=100)
    assert r["idle_reached"]
    b1, a, b2 = r["offers"]
    # B's check while A's offer is claimed but not acked, with a thief waiting
    assert b1["outcome"] == "none" and b1["set_calls"] == [] and b1["size_after"] == 2001
    assert b1["idle_after"] == 1
    assert a["outcome"] == "taken" and a["set_calls"] == [500] and a["size_after"] == 500
    assert b2["outcome"] == "taken" and b2["set_calls"] == [1001] and b2["size_after"] == 1001
    assert sorted(r["takes"]) == [(0, 500, 500, 7), (1, 1001, 1000, 9)]


# ---- withdraw ----

@pytest.mark.parametrize("size", [1000, 1001])
def test_unclaimed_offer_is_withdrawn_and_the_size_restored(core, size):
    r = core.share_selftest("withdraw", size=size, floor=100)
    assert r["idle_reached"]
    (o,) = r["offers"]
    assert o["outcome"] == "withdrawn"
    assert o["set_calls"] == [size - size // 2, size]   # shrunk, then restored
    assert o["size_after"] == size
    assert r["takes"] == []


# ---- deadline ----

@pytest.mark.parametrize("size", [1000, 1001])
def test_a_thief_that_never_acks_costs_the_nodes_not_a_double_count(core, size):
    r = core.share_selftest("deadline", size=size, floor=100, deadline_ms=40)
    (o,) = r["offers"]
    assert o["outcome"] == "abandoned"
    assert o["set_calls"] == [size - size // 2]     # no restore
    assert o["size_after"] == size - size // 2
    assert r["takes"] == [(0, size - size // 2, size // 2, 5)]
    assert 40 <= r["ms"] < 2000


# ---- termination ----

@pytest.mark.parametrize("runners", [1, 3])
@pytest.mark.parametrize("by_exception", [False, True])
def test_waiter_leaves_after_the_last_runner(core, runners, by_exception):
    r = core.share_selftest("termination", runners=runners, by_exception=by_exception)
    # still waiting while any runner remained, gone after the last one
    assert r["idle_reached"]
    assert r["returned_false"] == 1 and r["takes"] == [] and r["offers"] == []


def test_selftest_rejects_unknown_scenarios(core):
    with pytest.raises(ValueError):
        core.share_selftest("bogus")
    with pytest.raises(ValueError):
        core.share_selftest("basic", size=1 << 25)
