"""The devpool expand / presum / gather2 kernels one iteration at a time.

Every case uploads a chosen pool, runs exactly ONE iteration through
nq_devpool_step / pfsp_devpool_step (the engines' own launch helper) and
compares EVERYTHING that iteration writes — the un-popped prefix, the emitted
children (as a multiset of node bytes) and every control-block field — with
the pure-CPU oracle in helpers/devpool_step_oracle.py (itself proved against
the sequential counts in test_devpool_step_oracle.py). Nothing is compared
with another GPU result; every configuration also runs twice and must be
byte-identical. Inputs are CPU BFS frontiers and seeded random nodes
(random permutation, uniformly random depth): the kernels are pure functions
of the node, so unreachable nodes are legitimate and the only cheap way to
reach deep levels."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_step_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

HUGE = 10 ** 9  # incumbent no bound ever reaches
INSTS = [2, 14, 21]  # 20x5, 20x10, 20x20
# (lb, geom): every PFSP expand kernel; both lb2 geometries on every machine count
KERNELS = [("lb1", -1), ("lb1_d", -1), ("lb2", 3), ("lb2", 2)]
KERNEL_IDS = ["lb1", "lb1_d", "lb2-lane", "lb2-wave"]
GOOD_PERM = orc.GOOD_PERM

_oracle_cache = {}


def nq_expect(core, pool, N, g, finish, m, M):
    key = ("nq", pool, N, g, finish, m, M)
    if key not in _oracle_cache:
        _oracle_cache[key] = orc.nq_step(core, pool, N, g, finish, m, M)
    return _oracle_cache[key]


def pfsp_expect(core, pool, inst, lb, best, m, M):
    key = ("pfsp", pool, inst, lb, best, m, M)
    if key not in _oracle_cache:
        _oracle_cache[key] = orc.pfsp_step(core, pool, inst, lb, best, m, M)
    return _oracle_cache[key]


def run_nq(gpu, pool, N, g=1, finish=8, m=1, M=None, presum="auto", what=""):
    exp = nq_expect(gpu, pool, N, g, finish, m, M)
    a = gpu.nq_devpool_step(pool, N, g, finish, m, M, None, presum)
    b = gpu.nq_devpool_step(pool, N, g, finish, m, M, None, presum)
    what = ("nq", what, "N", N, "n", len(pool) // 24, "g", g, "finish", finish, "m", m, "M", M,
            presum)
    assert a == b, (what, "two runs differ")
    orc.check_step(exp, a[0], a[1], what)
    return exp, a


def run_pfsp(gpu, pool, inst, lb, best, m=1, M=None, geom=-1, presum="auto", what=""):
    exp = pfsp_expect(gpu, pool, inst, lb, best, m, M)
    a = gpu.pfsp_devpool_step(pool, inst, lb, best, m, M, None, geom, presum)
    b = gpu.pfsp_devpool_step(pool, inst, lb, best, m, M, None, geom, presum)
    what = ("pfsp", what, "inst", inst, lb, "geom", geom, "n", len(pool) // 24, "best", best,
            "m", m, "M", M, presum)
    assert a == b, (what, "two runs differ")
    orc.check_step(exp, a[0], a[1], what)
    return exp, a


def pop_windows(n):
    return [(1, n), (1, 7), (n, n), (n + 1, n), (1, n - 1)]


# ---------------------------------------------------------------------------
# N-Queens (k_nq_x + k_presum + k_gather2<NQNode>)
# ---------------------------------------------------------------------------

NQ_SIZES = [1, 2, 51, 52, 256, 257, 1000]


@pytest.mark.parametrize("N", [4, 5, 12, 20])
def test_nq_shapes(gpu, N):
    # n*N below / on / just above the 1024-child tile and the 256-slot
    # sub-tile; N=12 puts 85 1/3 parents in a tile, so parents straddle tile
    # boundaries. finish=-1 pushes every safe child (maximal emission and
    # compaction traffic), finish=8 is the engines' default.
    rng = orc.rng(1000 + N)
    for n in NQ_SIZES:
        pool = orc.random_nq_nodes(rng, n, N)
        for finish in (-1, 8):
            run_nq(gpu, pool, N, finish=finish)


@pytest.mark.parametrize("N", [12, 17])
def test_nq_bfs_frontier(gpu, N):
    pool, _, _ = gpu.nq_bfs_frontier(N, 1, 2000)
    for finish in (-1, 8):
        run_nq(gpu, pool, N, finish=finish, what="bfs")
        run_nq(gpu, pool, N, finish=finish, M=777, what="bfs")


@pytest.mark.parametrize("n", [52, 257])
def test_nq_pop_rule(gpu, n):
    N = 12
    pool = orc.random_nq_nodes(orc.rng(77 + n), n, N)
    for m, M in pop_windows(n):
        for finish in (-1, 8):
            exp, (out, ctl) = run_nq(gpu, pool, N, finish=finish, m=m, M=M)
            c = 0 if n < m else min(n, M)
            assert ctl["chunk"] == c
            if m == n + 1:  # below the window: nothing happens, iters untouched
                assert out == pool
                assert (ctl["size"], ctl["iters"], ctl["tree"], ctl["sol"]) == (n, 0, 0, 0)
            else:
                assert ctl["iters"] == 1


def test_nq_empty_pool(gpu):
    exp, (out, ctl) = run_nq(gpu, b"", 8)
    assert out == b""
    assert ctl == dict(size=0, chunk=0, tree=0, sol=0, iters=0, best=0, overflow=0)


@pytest.mark.parametrize("N", [8, 11])
def test_nq_finisher(gpu, N):
    # random depths 0..N include depth == N leaf parents and rem == 0 children
    pool = orc.random_nq_nodes(orc.rng(4242 + N), 300, N)
    for finish in (-1, 0, 1, 4, 8):
        run_nq(gpu, pool, N, finish=finish)
        run_nq(gpu, pool, N, finish=finish, M=129)
    # hand-made leaf parents only (finish=-1: no finisher involved at all)
    leaves = orc.random_nq_nodes(orc.rng(5), 60, N, min_depth=N)
    exp, (out, ctl) = run_nq(gpu, leaves, N, finish=-1)
    assert (ctl["size"], ctl["sol"], ctl["tree"]) == (0, 60, 0)
    # leaf parents in the popped tail behind a live prefix
    exp, (out, ctl) = run_nq(gpu, pool + leaves, N, finish=-1, M=60)
    assert (ctl["size"], ctl["sol"], ctl["tree"]) == (300, 60, 0)


def test_nq_finisher_swallows_every_child(gpu):
    # N=8, finish=8: rem <= 7 for every child, so nothing is pushed
    N = 8
    pool = orc.random_nq_nodes(orc.rng(31), 300, N, max_depth=N - 1)
    exp, (out, ctl) = run_nq(gpu, pool, N, finish=8, M=200)
    assert exp.children == [] and ctl["size"] == 100 and ctl["tree"] > 0


def test_nq_finisher_swallows_nothing(gpu):
    # N=20, depth <= 8: rem >= 11 > finish, every safe child is pushed
    N = 20
    pool = orc.random_nq_nodes(orc.rng(32), 300, N, max_depth=8)
    exp, (out, ctl) = run_nq(gpu, pool, N, finish=8)
    assert ctl["tree"] == len(exp.children) > 300 and ctl["sol"] == 0


@pytest.mark.parametrize("N", [5, 12])
def test_nq_g_mask_path(gpu, N):
    # g > 1 takes k_nq_x<false> / nq_free_g; results are g-invariant
    pool = orc.random_nq_nodes(orc.rng(90 + N), 257, N)
    for finish in (-1, 4, 8):
        _, a1 = run_nq(gpu, pool, N, g=1, finish=finish)
        _, a3 = run_nq(gpu, pool, N, g=3, finish=finish)
        assert a1 == a3


def test_nq_prefix_paths_small_grid(gpu):
    # both prefix paths of k_gather2 at a small grid (12 and 6 blocks)
    for N, n in ((12, 1000), (20, 257)):
        pool = orc.random_nq_nodes(orc.rng(600 + N), n, N)
        for presum in ("off", "on", "auto"):
            for finish in (-1, 8):
                run_nq(gpu, pool, N, finish=finish, presum=presum)


def test_nq_presum_whole_groups(gpu):
    # 13200 * 20 children = 258 expand blocks: with presum="on" gather blocks
    # 256 and 257 take one whole group sum (gfull >= 1) plus a partial walk.
    # depth <= 8 with finish=8 finishes nothing, so no subtree counts needed.
    N = 20
    pool = orc.random_nq_nodes(orc.rng(13200), 13200, N, max_depth=8)
    assert gpu.devpool_grid(13200, N, 1) > 256
    for presum in ("on", "off", "auto"):
        exp, _ = run_nq(gpu, pool, N, finish=8, presum=presum)
    assert exp.ctl["tree"] == len(exp.children)


def test_nq_overflow_flag(gpu):
    # flag test: base + #pushed > capacity >= n. The kernel guards its pool
    # writes by capacity, so every access stays in bounds.
    N, n, M = 12, 100, 60
    pool = orc.random_nq_nodes(orc.rng(8), n, N, max_depth=2)
    exp = orc.nq_step(gpu, pool, N, 1, -1, 1, M)
    pushed = len(exp.children)
    assert pushed > M
    for capacity in (n, n - M + pushed - 1):
        assert n <= capacity < n - M + pushed
        out, ctl = gpu.nq_devpool_step(pool, N, 1, -1, 1, M, capacity, "auto")
        orc.check_overflow(exp, pool, out, ctl, ("nq overflow", capacity))
    # exact fit is not an overflow
    out, ctl = gpu.nq_devpool_step(pool, N, 1, -1, 1, M, n - M + pushed, "auto")
    orc.check_step(exp, out, ctl, "nq exact-fit capacity")


# ---------------------------------------------------------------------------
# PFSP (k_pfsp_x<MM,1>, k_pfsp_x<MM,2>, k_pfsp_x_lb1d, k_pfsp_x_lb2w, presum, gather2)
# ---------------------------------------------------------------------------

PFSP_SIZES = [1, 12, 13, 51, 52, 256, 257, 1000]


def pfsp_pools(inst, n):
    """(best, pool) pairs. Mixed-depth chunks (depth 0..19, leaves included)
    keep best0 = optimum: no leaf of a ub=1 tree lies below the optimum, so no
    atomicMin can lower ctl->best mid-kernel and pruning stays deterministic.
    With a huge incumbent (nothing pruned, every non-leaf child pushed) the
    chunk holds no depth-19 parent for the same reason."""
    rng = orc.rng(inst * 100000 + n)
    return [("optimum", orc.random_pfsp_nodes(rng, n)),
            (HUGE, orc.random_pfsp_nodes(rng, n, max_depth=18))]


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("inst", INSTS)
def test_pfsp_shapes(gpu, inst, kernel):
    # 13 parents = 260 slots: the wave kernel's second block holds 4 valid
    # slots and 252 invalid ones; 51/52 straddle the 1024 tile; 256/257 the
    # lb1_d block; 1000 parents give the wave kernel ~316 count entries
    lb, geom = kernel
    opt = gpu.taillard_best_ub(inst)
    for n in PFSP_SIZES:
        for best, pool in pfsp_pools(inst, n):
            best = opt if best == "optimum" else best
            run_pfsp(gpu, pool, inst, lb, best, geom=geom)


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("inst", INSTS)
def test_pfsp_bfs_frontier(gpu, inst, kernel):
    lb, geom = kernel
    pool, _, _, best = gpu.pfsp_bfs_frontier(inst, lb, 1, 1000)
    run_pfsp(gpu, pool, inst, lb, best, geom=geom, what="bfs")
    run_pfsp(gpu, pool, inst, lb, best, geom=geom, M=333, what="bfs")


@pytest.mark.parametrize("geom", [3, 2])
@pytest.mark.parametrize("inst", INSTS)
def test_pfsp_lb2_incumbent_regimes(gpu, inst, geom):
    # huge: no early exit, all rounds of the wave kernel incl. the global-memory
    # pair rows >= 64 at 20 machines; optimum: exits in the middle; 1: every
    # child exits at the first pair / round and nothing is pushed
    opt = gpu.taillard_best_ub(inst)
    for n in (257, 1000):
        rng = orc.rng(inst * 7 + n)
        mixed = orc.random_pfsp_nodes(rng, n)
        inner = orc.random_pfsp_nodes(rng, n, max_depth=18)
        presums = ("on", "off") if n == 1000 else ("auto",)
        for presum in presums:
            exp, _ = run_pfsp(gpu, inner, inst, "lb2", HUGE, geom=geom, presum=presum)
            assert exp.ctl["tree"] == len(exp.children) > n
            run_pfsp(gpu, mixed, inst, "lb2", opt, geom=geom, presum=presum)
            exp, (out, ctl) = run_pfsp(gpu, mixed, inst, "lb2", 1, geom=geom, M=n - 57,
                                       presum=presum)
            assert exp.children == [] and ctl["size"] == 57 and ctl["best"] == 1


@pytest.mark.parametrize("inst", INSTS)
def test_pfsp_geom_auto_equals_forced_choice(gpu, inst):
    forced = gpu.devpool_lbk_geom(2, gpu.taillard_nb_machines(inst))
    assert forced in (2, 3)
    pool = orc.random_pfsp_nodes(orc.rng(inst + 50), 257, max_depth=18)
    _, auto = run_pfsp(gpu, pool, inst, "lb2", HUGE, geom=-1)
    _, pinned = run_pfsp(gpu, pool, inst, "lb2", HUGE, geom=forced)
    assert auto == pinned


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("inst", INSTS)
def test_pfsp_all_leaf_chunk(gpu, inst, kernel):
    # a popped chunk of depth-19 parents only: every child is a leaf, nothing
    # is pushed, sol counts every child and best = min(best0, min lb).
    # best0 = optimum: strict '<' means no update; optimum + 200: an update.
    lb, geom = kernel
    opt = gpu.taillard_best_ub(inst)
    rng = orc.rng(inst + 19)
    prefix = orc.random_pfsp_nodes(rng, 300)
    leaves = orc.random_pfsp_nodes(rng, 63, min_depth=19) + orc.pfsp_node(19, GOOD_PERM[inst])
    pool = prefix + leaves[:30 * 24] + leaves[63 * 24:] + leaves[30 * 24:63 * 24]
    for best0 in (opt, opt + 200):
        exp, (out, ctl) = run_pfsp(gpu, pool, inst, lb, best0, geom=geom, M=64)
        assert (ctl["size"], ctl["sol"], ctl["tree"]) == (300, 64, 0)
        if best0 == opt:
            assert ctl["best"] == opt
        else:
            assert opt <= ctl["best"] < best0


# one kernel per geometry family: thread-per-child, thread-per-parent, per-wave
@pytest.mark.parametrize("kernel", [("lb1", -1), ("lb1_d", -1), ("lb2", 2)],
                         ids=["lb1", "lb1_d", "lb2-wave"])
@pytest.mark.parametrize("n", [52, 257])
def test_pfsp_pop_rule(gpu, n, kernel):
    lb, geom = kernel
    inst = 14
    opt = gpu.taillard_best_ub(inst)
    for best, pool in pfsp_pools(inst, n):
        best = opt if best == "optimum" else best
        for m, M in pop_windows(n):
            exp, (out, ctl) = run_pfsp(gpu, pool, inst, lb, best, m=m, M=M, geom=geom)
            assert ctl["chunk"] == (0 if n < m else min(n, M))
            if m == n + 1:
                assert out == pool
                assert (ctl["size"], ctl["iters"], ctl["tree"], ctl["sol"]) == (n, 0, 0, 0)
            else:
                assert ctl["iters"] == 1


def test_pfsp_empty_pool(gpu):
    for lb, geom in KERNELS:
        exp, (out, ctl) = run_pfsp(gpu, b"", 14, lb, 1377, geom=geom)
        assert out == b""
        assert ctl == dict(size=0, chunk=0, tree=0, sol=0, iters=0, best=1377, overflow=0)


@pytest.mark.parametrize("kernel", [("lb1", -1), ("lb2", 2)], ids=["lb1", "lb2-wave"])
def test_pfsp_overflow_flag(gpu, kernel):
    # flag test (see test_nq_overflow_flag): base + #pushed > capacity >= n
    lb, geom = kernel
    inst, n, M = 2, 100, 60
    pool = orc.random_pfsp_nodes(orc.rng(9), n, max_depth=10)
    exp = orc.pfsp_step(gpu, pool, inst, lb, HUGE, 1, M)
    pushed = len(exp.children)
    assert pushed > M
    for capacity in (n, n - M + pushed - 1):
        assert n <= capacity < n - M + pushed
        out, ctl = gpu.pfsp_devpool_step(pool, inst, lb, HUGE, 1, M, capacity, geom, "auto")
        orc.check_overflow(exp, pool, out, ctl, ("pfsp overflow", lb, capacity))
    out, ctl = gpu.pfsp_devpool_step(pool, inst, lb, HUGE, 1, M, n - M + pushed, geom, "auto")
    orc.check_step(exp, out, ctl, "pfsp exact-fit capacity")
