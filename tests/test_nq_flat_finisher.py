"""The flat (single-loop, stackless) N-Queens finisher on the CPU.

nq_finish_count_cpu runs the very loop k_nq_x's phase C runs (src/nq_finish.hpp)
over one job; it must count what a plain recursive placement counts: every
safe node below the job's state (tree) and every full board (sol).
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from nq_finish_cases import masks  # noqa: E402

SOLUTIONS = {4: 2, 5: 10, 6: 4, 7: 40, 8: 92, 9: 352, 10: 724, 11: 2680}


_walks = {}


def ref_walk(N):
    """ONE plain recursion over (row, col) placements of the whole N-board,
    shared by every test of that N: {queens placed so far (tuple of (row,
    col)): (nodes, solutions) below that board}, recorded for every board of
    at most 2 and of at least N-3 rows. Attacks are looked up in sets of
    column / diagonal numbers, not in masks."""
    if N in _walks:
        return _walks[N]
    used_c, used_s, used_d, queens, out = set(), set(), set(), [], {}

    def rec(r):
        tree = sol = 0
        for c in range(N):
            if c in used_c or r + c in used_s or r - c in used_d:
                continue
            tree += 1
            if r + 1 == N:
                sol += 1
                continue
            used_c.add(c), used_s.add(r + c), used_d.add(r - c), queens.append((r, c))
            t, s = rec(r + 1)
            used_c.discard(c), used_s.discard(r + c), used_d.discard(r - c), queens.pop()
            tree += t
            sol += s
        if r <= 2 or r >= N - 3:
            out[tuple(queens)] = (tree, sol)
        return tree, sol

    rec(0)
    _walks[N] = out
    return out


def ref_count(N, row, queens):
    assert len(queens) == row
    return ref_walk(N)[tuple(queens)]


def boards_at(N, depth):
    """Every safe placement of rows 0..depth-1 (depth <= 2 or >= N-3)."""
    return sorted(q for q in ref_walk(N) if len(q) == depth)


@pytest.mark.parametrize("N", range(4, 12))
def test_from_the_root(core, N):
    tree, sol = core.nq_finish_count_cpu(0, 0, 0, 0, N)
    assert sol == SOLUTIONS[N]
    assert (tree, sol) == ref_count(N, 0, ())


@pytest.mark.parametrize("N", range(8, 13))
@pytest.mark.parametrize("where", ["depth2", "depthN-3"])
def test_from_every_node_of_a_level(core, N, where):
    depth = 2 if where == "depth2" else N - 3
    boards = boards_at(N, depth)
    assert boards
    empty = 0
    for q in boards:
        cols, d1, d2 = masks(N, depth, q)
        want = ref_count(N, depth, q)
        assert core.nq_finish_count_cpu(cols, d1, d2, depth, N) == want, (N, q)
        empty += want == (0, 0)
    if where == "depthN-3":
        assert empty > 0  # jobs with no free square at all are among them


@pytest.mark.parametrize("N", [8, 10, 12])
def test_one_and_two_rows_left(core, N):
    """The popcount path (one row above the bottom, and the bottom row itself
    as a job's root), incl. states with no free square."""
    for depth in (N - 2, N - 1):
        seen_empty = seen_full = False
        for q in boards_at(N, depth)[:400]:
            cols, d1, d2 = masks(N, depth, q)
            want = ref_count(N, depth, q)
            assert core.nq_finish_count_cpu(cols, d1, d2, depth, N) == want, (N, q)
            seen_empty |= want[0] == 0
            seen_full |= want[1] > 0
        assert seen_empty and seen_full


def test_unreachable_state_counts_like_the_masks_say(core):
    """The kernel is a pure function of the masks (random test pools hold
    boards whose queens already attack each other): compare with a recursion
    over the same masks."""
    def rec(cols, d1, d2, row, N):
        msk = (1 << N) - 1
        free = ~(cols | d1 | d2) & msk
        tree = sol = 0
        while free:
            bit = free & -free
            free ^= bit
            tree += 1
            if row + 1 == N:
                sol += 1
            else:
                t, s = rec(cols | bit, ((d1 | bit) << 1) & msk, (d2 | bit) >> 1, row + 1, N)
                tree += t
                sol += s
        return tree, sol

    for N, row, cols, d1, d2 in [(9, 1, 0b1, 0b111000000, 0b101), (13, 5, 0b11111, 0, 0x1FFF),
                                 (20, 12, 0xFFF, 0x80001, 0x10), (20, 19, 0x7FFFF, 0, 0),
                                 (12, 4, 0xF, 0xFFF, 0xFFF), (11, 0, 0, 0x400, 0x1)]:
        assert core.nq_finish_count_cpu(cols, d1, d2, row, N) == rec(cols, d1, d2, row, N)


def test_rejects_jobs_it_cannot_hold(core):
    with pytest.raises(ValueError):
        core.nq_finish_count_cpu(0, 0, 0, 0, 13)  # 13 rows > 12
    with pytest.raises(ValueError):
        core.nq_finish_count_cpu(0, 0, 0, 8, 8)   # no empty row
    with pytest.raises(ValueError):
        core.nq_finish_count_cpu(1 << 8, 0, 0, 0, 8)
