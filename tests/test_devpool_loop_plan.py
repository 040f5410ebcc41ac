"""The loop driver's planner (src/devpool_loop_plan.hpp) against the rules as
helpers/devpool_loop_oracle.py states them, on the CPU.

run_devpool_loop takes its batch length, its spills and its graph captures and
replays from plan_batch / plan_graph; _core exposes both read-only. The oracle
keeps its own constants and batch_len: it is the independent statement of the
rule, so far compared with the driver only through GPU traces. The grid
brackets every threshold of the rule: the small-pool size, 4m, and the
capacity at which room // growth is 0, 1, 15, 16 and 17."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_loop_oracle as orc  # noqa: E402

BMAX = (0, 1, 15, 16, 17)


def grid(per, m, chunk):
    """(capacity, size) pairs: room // growth takes every value of BMAX at
    every base size, at both ends of the capacity range that gives it."""
    growth = chunk * per
    base = (0, 1, 4095, 4096, 4 * m - 1, 4 * m)
    near = sorted({s + d for s in base for d in (-1, 0, 1) if s + d >= 0})
    for s, k, e in itertools.product(base, BMAX, (0, growth - 1)):
        capacity = s + k * growth + e
        if capacity == 0:  # "no capacity": not the oracle's domain, see below
            continue
        sizes = set(near) | {capacity - 1, capacity}
        for size in sorted(x for x in sizes if 0 <= x <= capacity):
            yield capacity, size


def plan(core, cfg, size, batches, stop_size=0, can_spill=True, growth=None, capacity=None):
    return core.devpool_plan_batch(
        m=cfg.m, per=cfg.per, growth=cfg.growth if growth is None else growth,
        capacity=cfg.capacity if capacity is None else capacity, stop_size=stop_size,
        size=size, batches=batches, can_spill=can_spill)


def test_constants(core):
    assert core.LOOP_BATCH == orc.BATCH == 16
    assert core.LOOP_EAGER_BATCHES == orc.EAGER_BATCHES == 4
    assert core.LOOP_SMALL_POOL == orc.SMALL_POOL == 4096


@pytest.mark.parametrize("per", [1, 8, 20])
@pytest.mark.parametrize("m", [1, 25, 40000])
@pytest.mark.parametrize("chunk", [1, 64, 256])
def test_batch_plan(core, per, m, chunk):
    seen_bmax, seen = set(), set()
    for capacity, size in grid(per, m, chunk):
        cfg = orc.Cfg(m=m, chunk=chunk, per=per, capacity=capacity)
        bmax = (capacity - size) // cfg.growth
        seen_bmax.add(bmax)
        for batches in (0, 1, 4):
            w = (per, m, chunk, capacity, size, batches)
            want = orc.batch_len(cfg, size, batches)
            seen.add(want)
            # the oracle's domain: a spill hook, growth > 0
            assert plan(core, cfg, size, batches) == want, w
            # no spill hook never plans a spill: one iteration instead
            assert plan(core, cfg, size, batches, can_spill=False) == (
                1 if want == "spill" else want), w
            # the frontier builder runs one iteration per batch; the capacity
            # rule cannot cut 1 further, it can only spill
            assert plan(core, cfg, size, batches, stop_size=size + 1) == (
                "spill" if want == "spill" else 1), w
            assert plan(core, cfg, size, batches, stop_size=1, can_spill=False) == 1, w
            # growth == 0 or capacity == 0: no capacity rule
            free = 2 if per > 1 and size < orc.SMALL_POOL else orc.BATCH
            assert plan(core, cfg, size, batches, growth=0) == free, w
            assert plan(core, cfg, size, batches, capacity=0) == free, w
    # the grid reached what it was built for
    assert set(BMAX) <= seen_bmax
    assert {"spill", 1, 15, 16} <= seen
    assert per == 1 or 2 in seen


def test_graph_plan(core):
    for allowed, batches, have_exec, b, par in itertools.product(
            (False, True), range(6), (False, True), (1, 2, 15, 16), (0, 1)):
        w = (allowed, batches, have_exec, b, par)
        cfg = orc.Cfg(m=1, chunk=1, per=1, capacity=1, graph=allowed)
        cond = bool(cfg.graph and batches >= orc.EAGER_BATCHES and b == orc.BATCH and par == 0)
        got = core.devpool_plan_graph(allowed=allowed, batches=batches, have_exec=have_exec,
                                      b=b, par=par)
        # capture: the oracle's condition, and no exec yet
        assert (got == "capture") == (cond and not have_exec), w
        # replay: an exec exists, a full batch, entered on parity 0
        assert (got == "replay") == (have_exec and b == orc.BATCH and par == 0), w
        assert got in ("eager", "capture", "replay"), w
        # an exec exists only where a capture was planned before: there the
        # batch goes through the graph iff the oracle's condition holds
        if not have_exec or (allowed and batches >= orc.EAGER_BATCHES):
            assert (got != "eager") == cond, w
