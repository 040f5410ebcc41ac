"""The split finisher's queue logic on the CPU.

nq_finish_block_cpu pushes a list of finisher jobs through the functions
k_nq_x's split drain runs (src/nq_finish.hpp): the split pass that counts and
ranks the sub-jobs, the rounds cut, the entry codec, the sub-job load and the
flat loop, one after the other. Whatever the split depth and the queue
capacity, it must count what nq_finish_count_cpu counts over the same jobs;
the number of queue entries and of rounds is recomputed here from the masks.

A qcap below one job's fan-out is REJECTED (ValueError naming the job): the
kernel's QCAP is at least the largest fan-out (56) by a static_assert, so the
case cannot arise there.
"""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from nq_finish_cases import fanout, free_mask, jobs_n13, random_job  # noqa: E402

SPLITS = (0, 1, 2)


def rounds_of(counts, qcap):
    """Greedy: the longest run of jobs, in order, that fits qcap."""
    rounds, fill = 0, None
    for n in counts:
        if fill is None or fill + n > qcap:
            rounds += 1
            fill = 0
        fill += n
    return rounds


_want = {}


def want(core, jobs, N):
    key = (tuple(jobs), N)
    if key not in _want:
        tree = sol = 0
        for cols, d1, d2, row in jobs:
            t, s = core.nq_finish_count_cpu(cols, d1, d2, row, N)
            tree += t
            sol += s
        _want[key] = (tree, sol)
    return _want[key]


def check(core, jobs, N, split, qcap, g=1):
    counts = [fanout(j, N, split) for j in jobs]
    got = core.nq_finish_block_cpu(jobs, N, g, split, qcap)
    assert got[:2] == want(core, jobs, N), (N, split, qcap, g)
    assert got[2] == sum(counts), (N, split, qcap, g)
    assert got[3] == rounds_of(counts, qcap), (N, split, qcap, g)
    return counts


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("split", SPLITS)
def test_every_height(core, split, g):
    jobs = jobs_n13()
    rng = random.Random(1301)
    rng.shuffle(jobs)
    assert {13 - j[3] for j in jobs} == set(range(1, 9))
    check(core, jobs, 13, split, core.NQ_SPLIT_QCAP, g)
    check(core, jobs, 13, split, 64, g)  # many rounds


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("split", SPLITS)
def test_roots_with_no_and_one_candidate(core, split, g):
    rng = random.Random(1302)
    none, one = [], []
    while len(none) < 8 or len(one) < 8:
        j = random_job(rng, 13, rng.randint(2, 8))
        n = bin(free_mask(*j[:3], 13)).count("1")
        if n == 0 and len(none) < 8:
            none.append(j)
        if n == 1 and len(one) < 8:
            one.append(j)
    check(core, none, 13, split, core.NQ_SPLIT_QCAP, g)
    check(core, one, 13, split, core.NQ_SPLIT_QCAP, g)
    counts = check(core, none + one + jobs_n13()[:20], 13, split, core.NQ_SPLIT_QCAP, g)
    if split:
        assert counts[:8] == [0] * 8  # a job without candidates has no sub-job


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("split", SPLITS)
def test_split_depth_clamps(core, split, g):
    rng = random.Random(1303)
    for rows in (1, 2):
        jobs = [random_job(rng, 10, rows) for _ in range(40)]
        counts = check(core, jobs, 10, split, core.NQ_SPLIT_QCAP, g)
        if rows == 1 or split == 0:
            assert counts == [1] * 40  # never split: the root is the bottom row
        else:  # one level at either split depth
            assert counts == [bin(free_mask(*j[:3], 10)).count("1") for j in jobs]
    assert any(c > 0 for c in counts)


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("split", SPLITS)
def test_n20_guard_bits(core, split, g):
    rng = random.Random(2000)
    jobs = [random_job(rng, 20, rows) for rows in (8, 8, 8, 7, 7, 6, 5, 3)]
    jobs.append((0xFFF, 0x80001, 0x10, 12))
    jobs.append((0xFFF << 8, 0x1, 0x80000, 12))
    check(core, jobs, 20, split, core.NQ_SPLIT_QCAP, g)


@pytest.mark.parametrize("split", [1, 2])
def test_qcap_around_a_run(core, split):
    jobs = jobs_n13()
    counts = [fanout(j, 13, split) for j in jobs]
    total = sum(counts)
    assert total > max(counts) + 1
    for qcap, rounds in ((total - 1, 2), (total, 1), (total + 1, 1)):
        assert rounds_of(counts, qcap) == rounds
        check(core, jobs, 13, split, qcap)
    # a cut inside the list: the first round ends exactly at job 40
    head = sum(counts[:40])
    assert counts[40] > 0
    for qcap in (head - 1, head, head + 1):
        if qcap >= max(counts):
            check(core, jobs, 13, split, qcap)
    check(core, jobs, 13, split, max(counts))  # the smallest legal queue


@pytest.mark.parametrize("split", [1, 2])
def test_qcap_below_one_fanout_is_rejected(core, split):
    jobs = jobs_n13()
    worst = max(fanout(j, 13, split) for j in jobs)
    assert worst > 1
    with pytest.raises(ValueError, match="sub-jobs of job"):
        core.nq_finish_block_cpu(jobs, 13, 1, split, worst - 1)
    check(core, jobs, 13, split, worst)


def test_rejects_bad_arguments(core):
    job = [(0, 0, 0, 5)]
    for args in ((job, 13, 1, 3, 64), (job, 13, 1, -1, 64), (job, 13, 0, 1, 64),
                 (job, 13, 1, 1, 0), (job, 14, 1, 1, 64), ([(1 << 13, 0, 0, 5)], 13, 1, 1, 64),
                 (job * 1025, 13, 1, 1, 64)):
        with pytest.raises(ValueError):
            core.nq_finish_block_cpu(*args)
    assert core.nq_finish_block_cpu([], 13, 1, 2, 64) == (0, 0, 0, 0)


def test_whole_board_as_one_job(core):
    for split in SPLITS:
        tree, sol, entries, rounds = core.nq_finish_block_cpu([(0, 0, 0, 0)], 8, 1, split, 64)
        assert (tree, sol) == core.nq_finish_count_cpu(0, 0, 0, 0, 8) and sol == 92
        assert entries == {0: 1, 1: 8, 2: 42}[split] and rounds == 1


def test_codec_round_trip(core):
    """Whole domain: 2 + 14 + 5 + 5 bits; distinct inputs give distinct entries."""
    for ncols in range(3):
        for ref in list(range(0, 1 << 14, 97)) + [(1 << 14) - 1]:
            for c1 in range(32):
                for c2 in range(32):
                    e = core.nq_sub_encode(ref, ncols, c1, c2)
                    assert e == ncols << 24 | ref << 10 | c1 << 5 | c2
                    assert core.nq_sub_decode(e) == (ref, ncols, c1, c2)
    for ref in range(1 << 14):
        e = core.nq_sub_encode(ref, 2, 19, 0)
        assert core.nq_sub_decode(e) == (ref, 2, 19, 0)


def test_constants(core):
    assert core.NQ_SPLIT_QCAP >= 56 and core.NQ_SPLIT_MAX == 2
    assert core.nq_split_default() in (0, 1, 2)
