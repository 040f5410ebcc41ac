"""The wave-stack finisher on the CPU.

nq_finish_stack_cpu steps waves x lanes rows in lockstep with the kernel's own
functions (the row step, the wave rule and the overflow fallback of
src/nq_finish.hpp); the waves take turns on one job counter. Whatever the
threshold, the wave shape and the stack capacity, it must count what
nq_finish_count_cpu (one flat walk per job) counts over the same jobs. The
function itself throws when its loop passes the bound of nq_stack_act's
termination argument, so a rule that spins fails here, not on a GPU.

A lane may push only while sp + lanes <= cap. So with 64 lanes a cap below 64
makes every push fall back, cap = 64 lets a wave push onto an empty stack only
(one iteration's pushes, then it falls back until the stack is empty again),
and cap = 65..130 mixes the two further. The peak height is at most cap, always.
"""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from nq_finish_cases import jobs_n13, random_job  # noqa: E402

_count = {}


def expected(core, jobs, N):
    tree = sol = 0
    for j in jobs:
        if (j, N) not in _count:
            _count[(j, N)] = core.nq_finish_count_cpu(*j, N)
        t, s = _count[(j, N)]
        tree += t
        sol += s
    return tree, sol


def check(core, jobs, N, g=1, refill=24, waves=4, lanes=64, cap=None):
    cap = core.NQ_STACK_CAP if cap is None else cap
    tree, sol, iters, peak, fb = core.nq_finish_stack_cpu(jobs, N, g, refill, waves, lanes, cap)
    what = (N, g, refill, waves, lanes, cap)
    assert (tree, sol) == expected(core, jobs, N), what
    assert len(iters) == len(peak) == waves
    assert max(peak) <= cap, what
    return iters, peak, fb


def tall_jobs(n=200, N=13, seed=77):
    rng = random.Random(seed)
    return [random_job(rng, N, 8) for _ in range(n)]


def test_no_job_and_one_job(core):
    iters, peak, fb = check(core, [], 9)
    assert peak == [0, 0, 0, 0] and fb == 0
    assert all(i <= 1 for i in iters)  # every wave draws past the empty queue and leaves
    iters, peak, fb = check(core, [(0, 0, 0, 0)], 8)  # the whole N = 8 board
    assert fb == 0 and max(peak) > 0
    assert core.nq_finish_stack_cpu([(0, 0, 0, 0)], 8)[:2] == (2056, 92)


def test_root_without_and_with_one_candidate(core):
    N = 9
    full = (1 << N) - 1
    none = (full, 0, 0, 4)  # every column attacked: the root has no candidate
    assert core.nq_finish_count_cpu(*none, N) == (0, 0)
    _, peak, fb = check(core, [none], N)
    assert peak == [0, 0, 0, 0] and fb == 0
    one = (full ^ 1 << 3, 0, 0, 4)  # only column 3 free
    assert core.nq_finish_count_cpu(*one, N)[0] >= 1
    check(core, [one], N)
    check(core, [none, one, none, one] * 5, N)
    bottom = (full ^ 0b101, 0, 0, N - 1)  # root in the bottom row: two solutions
    assert core.nq_finish_count_cpu(*bottom, N) == (2, 2)
    check(core, [bottom], N)


@pytest.mark.parametrize("rows", range(1, 9))
def test_every_job_height(core, rows):
    rng = random.Random(100 + rows)
    for N in (rows, 9, 13):
        if N < rows or N < 4:
            continue
        jobs = [random_job(rng, N, rows) for _ in range(40)]
        _, peak, _ = check(core, jobs, N)
        if rows <= 2:
            assert max(peak) == 0  # no child has an inner row below it


@pytest.mark.parametrize("g", [1, 2])
def test_n20_masks(core, g):
    rng = random.Random(2000)
    jobs = [random_job(rng, 20, rows) for rows in (8, 7, 5, 3, 1) for _ in range(6)]
    assert any(j[0] >> 19 for j in jobs)  # the top column is in use
    check(core, jobs, 20, g=g)


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("refill", [1, 16, 64])
def test_thresholds(core, g, refill):
    check(core, jobs_n13(), 13, g=g, refill=refill)


@pytest.mark.parametrize("waves,lanes,refill", [(1, 64, 16), (4, 64, 16), (1, 4, 1), (1, 4, 4),
                                               (1, 4, 16), (3, 7, 2)])
def test_wave_shapes(core, waves, lanes, refill):
    """refill above the lane count acts as the all-idle rule."""
    check(core, jobs_n13(), 13, refill=refill, waves=waves, lanes=lanes)
    check(core, jobs_n13()[:3], 13, refill=refill, waves=waves, lanes=lanes)  # jobs < lanes


def test_large_cap_never_falls_back(core):
    jobs = tall_jobs()
    _, peak, fb = check(core, jobs, 13, cap=1 << 16)
    assert fb == 0 and max(peak) > 130  # the caps below are real limits for these jobs


@pytest.mark.parametrize("cap", [0, 63])
def test_cap_below_the_lane_count_walks_every_child(core, cap):
    jobs = tall_jobs()
    _, peak, fb = check(core, jobs, 13, cap=cap)
    assert fb > 0 and max(peak) == 0


@pytest.mark.parametrize("refill", [1, 16, 64])
@pytest.mark.parametrize("cap", [64, 65, 66, 100, 127, 128, 129, 130])
def test_small_caps_mix_pushes_and_walks(core, cap, refill):
    jobs = tall_jobs()
    _, peak, fb = check(core, jobs, 13, cap=cap, refill=refill)
    assert fb > 0 and 0 < max(peak) <= cap
    _, peak, fb = check(core, jobs_n13(), 13, cap=cap, refill=refill, waves=2)
    assert fb > 0 and 0 < max(peak) <= cap


def test_cap_with_few_lanes(core):
    """4 lanes push while sp + 4 <= cap."""
    jobs = tall_jobs(20)
    _, peak, fb = check(core, jobs, 13, cap=8, lanes=4, waves=1, refill=1)
    assert fb > 0 and 0 < max(peak) <= 8
    _, peak, fb = check(core, jobs, 13, cap=3, lanes=4, waves=1, refill=1)
    assert fb > 0 and max(peak) == 0


def test_kernel_shape_never_passes_its_capacity(core):
    rng = random.Random(1717)
    for _ in range(6):
        jobs = [random_job(rng, 17, 8) for _ in range(rng.randint(200, 280))]
        check(core, jobs, 17)


def test_entry_codec_whole_domain(core):
    """Every field at its extremes and single bits, alone and together, plus
    random words: pack / unpack are inverse and the fields do not overlap."""
    top = (1 << 20) - 1
    vals = [0, top] + [1 << b for b in range(20)]
    for h in range(16):
        for v in vals:
            for c, d1, d2 in ((v, 0, 0), (0, v, 0), (0, 0, v), (v, v, v), (v, top ^ v, v)):
                w = core.nq_entry_pack(c, d1, d2, h)
                assert w < 1 << 64
                assert core.nq_entry_unpack(w) == (c, d1, d2, h)
                assert w == c | d1 << 20 | d2 << 40 | h << 60
    rng = random.Random(64)
    for _ in range(2000):
        c, d1, d2, h = (rng.randrange(1 << 20) for _ in range(3)), 0, 0, rng.randrange(16)
        c, d1, d2 = list(c)
        assert core.nq_entry_unpack(core.nq_entry_pack(c, d1, d2, h)) == (c, d1, d2, h)
    assert core.nq_entry_pack(1, 2, 3, 0) == core.nq_pmask_pack(1, 2, 3)


def test_arguments_are_validated(core):
    job = [(0, 0, 0, 1)]
    for kw in ({"refill": 0}, {"refill": 65}, {"waves": 0}, {"lanes": 65}, {"cap": -1}, {"g": 0}):
        with pytest.raises(ValueError):
            core.nq_finish_stack_cpu(job, 9, **kw)
    with pytest.raises(ValueError):
        core.nq_finish_stack_cpu([(0, 0, 0, 0)], 9)  # nine empty rows
    with pytest.raises(ValueError):
        core.nq_finish_stack_cpu([(1 << 9, 0, 0, 1)], 9)


def test_stack_default(core):
    assert core.nq_stack_default() in (0, 1)
    assert core.NQ_STACK_CAP >= 64
