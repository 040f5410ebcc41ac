"""The split finisher's batched, wave-uniform refill on the CPU.

nq_finish_wave_cpu steps waves x lanes flat walks in lockstep and lets every
wave decide with the kernel's own rule (nq_refill_now and friends in
src/nq_finish.hpp) when its idle lanes fetch; the waves take turns on one
queue head. Whatever the threshold, it must report what nq_finish_block_cpu
(one lane, one entry after the other) reports over the same jobs: tree, sol,
entries and rounds. The function itself throws when its loop passes the bound
"walk lengths + refills", so a rule that spins fails here, not on a GPU.

A `refill` above the wave's lane count is REJECTED (ValueError), not clamped.

The packed parent masks (nq_pmask_pack / nq_pmask_unpack) and the job
reference that carries the child's column (nq_job_ref / nq_job_state) are
checked against masks stepped in Python and nq_finish_count_cpu, N = 4..20.
"""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from nq_finish_cases import fanout, free_mask, jobs_n13, random_job, step  # noqa: E402

SPLITS = (1, 2)
GS = (1, 2)
REFILLS = (1, 2, 16, 63, 64)

_block = {}


def block(core, jobs, N, g, split, qcap):
    key = (tuple(jobs), N, g, split, qcap)
    if key not in _block:
        _block[key] = core.nq_finish_block_cpu(jobs, N, g, split, qcap)
    return _block[key]


def check(core, jobs, N, split, g, refill, qcap=None, lanes=64, waves=4):
    qcap = core.NQ_SPLIT_QCAP if qcap is None else qcap
    got = core.nq_finish_wave_cpu(jobs, N, g, split, qcap, refill, lanes, waves)
    what = (N, split, g, refill, qcap, lanes, waves)
    assert got[:4] == block(core, jobs, N, g, split, qcap), what
    tree, sol, entries, rounds, refills, steps = got
    # every round ends with one draining refill per wave at least; a refill
    # that does not drain hands out one entry or more
    assert waves * rounds <= refills <= entries + waves * rounds, what
    return got


def single(rng, N):
    """A job whose root is the bottom row: never split, one sub-job."""
    return random_job(rng, N, 1)


def jobs_with_entries(N, split, target, seed):
    """Jobs, in a fixed random order, whose sub-jobs number exactly `target`:
    random jobs of 2..8 rows while they fit, single-entry jobs for the rest."""
    rng = random.Random(seed)
    jobs, left = [], target
    for _ in range(200):
        j = random_job(rng, N, rng.randint(2, 8))
        n = fanout(j, N, split)
        if 0 < n <= left:
            jobs.append(j)
            left -= n
    jobs += [single(rng, N) for _ in range(left)]
    assert sum(fanout(j, N, split) for j in jobs) == target and len(jobs) <= 1024
    return jobs


def all_cases(f):
    f = pytest.mark.parametrize("split", SPLITS)(f)
    f = pytest.mark.parametrize("g", GS)(f)
    return pytest.mark.parametrize("refill", REFILLS)(f)


@all_cases
def test_no_job(core, split, g, refill):
    assert core.nq_finish_wave_cpu([], 13, g, split, 64, refill) == (0, 0, 0, 0, 0, 0)
    # jobs without a candidate: no entry, but a round that every wave must leave
    rng = random.Random(77)
    none = []
    while len(none) < 5:
        j = random_job(rng, 13, rng.randint(2, 8))
        if free_mask(*j[:3], 13) == 0:
            none.append(j)
    got = check(core, none, 13, split, g, refill)
    assert got[2:5] == (0, 1, 4)


@all_cases
def test_one_job_one_subjob(core, split, g, refill):
    got = check(core, [single(random.Random(5), 13)], 13, split, g, refill)
    assert got[2:4] == (1, 1)


@all_cases
def test_fewer_entries_than_the_threshold(core, split, g, refill):
    """Only the all-idle rule can start them (refill >= 2)."""
    n = max(1, refill // 2)
    got = check(core, jobs_with_entries(13, split, n, 40 + refill), 13, split, g, refill)
    assert got[2] == n
    check(core, jobs_with_entries(13, split, n, 40 + refill), 13, split, g, refill, waves=1)


@all_cases
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_entries_around_the_threshold(core, split, g, refill, delta):
    n = refill + delta  # 0 at refill 1: no job at all
    got = check(core, jobs_with_entries(13, split, n, 100 + n), 13, split, g, refill)
    assert got[2] == n


@all_cases
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_entries_around_a_wave_and_the_block(core, split, g, refill, n):
    got = check(core, jobs_with_entries(13, split, n, 200 + n), 13, split, g, refill)
    assert got[2:4] == (n, 1)


@all_cases
def test_rounds_rearm_drained(core, split, g, refill):
    """A small queue forces several rounds: a wave drained in one round must
    fetch again in the next."""
    jobs = jobs_n13()
    worst = max(fanout(j, 13, split) for j in jobs)
    got = check(core, jobs, 13, split, g, refill, qcap=max(64, worst))
    assert got[3] >= 2
    check(core, jobs, 13, split, g, refill, qcap=worst)


@all_cases
def test_every_height(core, split, g, refill):
    jobs = jobs_n13()
    random.Random(1301).shuffle(jobs)
    assert {13 - j[3] for j in jobs} == set(range(1, 9))
    check(core, jobs, 13, split, g, refill)


@all_cases
def test_n20_masks(core, split, g, refill):
    rng = random.Random(2000)
    jobs = [random_job(rng, 20, rows) for rows in (8, 8, 7, 7, 6, 5, 3, 1)]
    jobs.append((0xFFF, 0x80001, 0x10, 12))
    jobs.append((0xFFF << 8, 0x1, 0x80000, 12))
    check(core, jobs, 20, split, g, refill)


@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("split", SPLITS)
def test_four_lanes_one_wave(core, split, g):
    jobs = jobs_n13()[:40]
    for refill in (1, 2, 3, 4):
        check(core, jobs, 13, split, g, refill, lanes=4, waves=1)
        check(core, jobs, 13, split, g, refill, qcap=64, lanes=4, waves=1)
    for refill in (5, 16, 64):
        with pytest.raises(ValueError, match="refill"):
            core.nq_finish_wave_cpu(jobs, 13, g, split, core.NQ_SPLIT_QCAP, refill, 4, 1)


def dense_block():
    """What a dense N = 13 block holds: jobs of 8 rows."""
    rng = random.Random(1313)
    return [random_job(rng, 13, 8) for _ in range(400)]


@pytest.mark.parametrize("split", SPLITS)
def test_batching_saves_refills(core, split):
    jobs = dense_block()
    r1 = check(core, jobs, 13, split, 1, 1)
    r16 = check(core, jobs, 13, split, 1, 16)
    assert r1[2] > 4 * 256  # several sub-jobs per lane
    assert r16[4] < r1[4], (r16[4], r1[4])


def test_rejects_bad_arguments(core):
    job = [(0, 0, 0, 5)]
    for args in ((job, 13, 1, 0, 64, 1), (job, 13, 1, 3, 64, 1), (job, 13, 0, 1, 64, 1),
                 (job, 13, 1, 1, 0, 1), (job, 13, 1, 1, 64, 0), (job, 13, 1, 1, 64, 65),
                 (job, 13, 1, 1, 64, 1, 0, 1), (job, 13, 1, 1, 64, 1, 65, 1),
                 (job, 13, 1, 1, 64, 1, 64, 0), (job, 14, 1, 1, 64, 1),
                 (job * 1025, 13, 1, 1, 64, 1)):
        with pytest.raises(ValueError):
            core.nq_finish_wave_cpu(*args)
    jobs = jobs_n13()
    worst = max(fanout(j, 13, 2) for j in jobs)
    with pytest.raises(ValueError, match="sub-jobs of job"):
        core.nq_finish_wave_cpu(jobs, 13, 1, 2, worst - 1, 1)


def test_refill_default(core):
    assert 1 <= core.nq_refill_default() <= 64
    assert 1 <= core.NQ_REFILL_DEFAULT <= 64


# ---------------------------------------------------------------------------
# packed parent masks, column-carrying job reference
# ---------------------------------------------------------------------------

def test_pmask_round_trip(core):
    rng = random.Random(20)
    top = (1 << 20) - 1
    cases = [(0, 0, 0), (top, top, top), (top, 0, 0), (0, top, 0), (0, 0, top), (1, 1 << 19, 1)]
    cases += [tuple(rng.randrange(1 << 20) for _ in range(3)) for _ in range(200)]
    seen = set()
    for c, d1, d2 in cases:
        w = core.nq_pmask_pack(c, d1, d2)
        assert w == c | d1 << 20 | d2 << 40 and w < 1 << 60
        assert core.nq_pmask_unpack(w) == (c, d1, d2)
        seen.add(w)
    assert len(seen) == len(set(cases))


@pytest.mark.parametrize("N", range(4, 21))
def test_job_state_from_packed_masks(core, N):
    """Parents of every depth that leaves a job of 1..8 rows: the job below
    each free child column, rebuilt from the packed word and the reference,
    is the state stepped here, and counts what the plain state counts."""
    rng = random.Random(400 + N)
    for depth in range(max(0, N - 9), N - 1):
        for _ in range(3):
            cols, d1, d2, row = random_job(rng, N, N - depth)  # the parent: first empty row == depth
            assert row == depth == bin(cols).count("1")
            word = core.nq_pmask_pack(cols, d1, d2)
            tree = sol = 0
            for col in range(N):
                if not free_mask(cols, d1, d2, N) >> col & 1:
                    continue
                parent = rng.randrange(258)
                ref = core.nq_job_ref(parent, col)
                assert ref == parent * 32 + col and ref < 1 << 14
                want = step(cols, d1, d2, 1 << col, N) + (depth + 1,)
                got = core.nq_job_state(word, ref, N)
                assert got == want, (N, depth, col)
                t, s = core.nq_finish_count_cpu(*got, N)
                tree += 1 + t
                sol += s
                # the reference survives the sub-job entry's 14-bit field
                e = core.nq_sub_encode(ref, 2, 19, 3)
                assert core.nq_sub_decode(e)[0] == ref
            # the children's jobs add up to the walk below the parent
            assert (tree, sol) == core.nq_finish_count_cpu(cols, d1, d2, depth, N)
