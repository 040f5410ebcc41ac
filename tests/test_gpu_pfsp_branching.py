"""Backward / alternating / dynamic (MinBranch) branching on the GPU: the
both-directions lb1_d eval kernel, ONE iteration of the both-directions expand
kernel against the pure-Python one-step oracle (tests/helpers/bi_oracle.py),
and the engines against the frozen sequential counts."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bi_oracle as bo  # noqa: E402

pytestmark = pytest.mark.gpu

NODE = bo.NODE
INSTS = (2, 14, 21)  # 5, 10 and 20 machines: the three kernel instantiations
SIZES = (1, 255, 256, 257, 1000)  # one thread, one block, either side of a block edge
RULES = ("bwd", "alt", "minbranch")
# index (in the instance's 1000-node pool) of the parent the `mid` incumbent is
# taken from; chosen on the CPU so that at `mid` the pool (and its 257-node
# prefix) holds parents MinBranch decides by count each way, by the sum
# tie-break each way, and with an exact non-trivial cntF == cntB tie
HAND_PICKED = {2: 12, 14: 13, 21: 14}


@pytest.fixture(scope="module")
def tables(core):
    return {inst: bo.Tables(core, inst) for inst in INSTS}


@pytest.fixture(scope="module")
def pools():
    # one 1000-node pool per instance; the smaller pools are its prefixes, so the
    # oracle's (memoized) child bounds are computed once
    return {inst: bo.random_nodes(bo.rng(4200 + inst), 1000, force=bo.edge_cases())
            for inst in INSTS}


@pytest.fixture(scope="module")
def expected_bounds(tables, pools):
    return {inst: bo.bounds_arrays(tables[inst], pools[inst]) for inst in INSTS}


def mid_best(T, pool):  # pool: the instance's whole 1000-node pool
    """An incumbent strictly between the two directions' bounds of the
    hand-picked parent: above every bound of its tighter direction's best child
    and below the other direction's, so the directions' survivor counts differ."""
    h = HAND_PICKED[T.inst]
    f, b = bo.children_bounds(T, pool[h * NODE:(h + 1) * NODE])
    lo, hi = sorted((min(f.values()), min(b.values())))
    assert hi - lo >= 2, (lo, hi)
    return (lo + hi + 1) // 2


def decision_kinds(T, pool, best):
    """How MinBranch decides each parent of the pool: by count or by the sum
    tie-break, and which way."""
    kinds = {"count-back": 0, "count-front": 0, "tie-back": 0, "tie-front": 0,
             "nonzero-tie": 0}
    for i in range(0, len(pool), NODE):
        f, b = bo.children_bounds(T, pool[i:i + NODE])
        cntF, cntB, sumF, sumB = bo.stats(f, b, best)
        if cntF != cntB:
            kinds["count-back" if cntB < cntF else "count-front"] += 1
        else:
            kinds["tie-back" if sumB > sumF else "tie-front"] += 1
            kinds["nonzero-tie"] += cntF > 0 and cntF < len(f)
    return kinds


# ---------------------------------------------------------------------------
# bounds kernel
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("inst", INSTS)
def test_bounds_bi_gpu_vs_cpu_vs_python(gpu, pools, expected_bounds, inst, n):
    pool = pools[inst][:n * NODE]
    g_begin, g_end = gpu.pfsp_gpu_bounds_bi(inst, pool)
    c_begin, c_end = gpu.pfsp_cpu_bounds_bi(inst, pool)
    e_begin, e_end = expected_bounds[inst]
    assert list(c_begin) == e_begin[:n * 20] and list(c_end) == e_end[:n * 20]
    assert list(g_begin) == e_begin[:n * 20]
    assert list(g_end) == e_end[:n * 20]


# ---------------------------------------------------------------------------
# one expand iteration
# ---------------------------------------------------------------------------

def run_step(gpu, T, pool, rule, best, what, m=1, M=None):
    exp = bo.step(T, pool, rule, best, m=m, M=M)
    out = [gpu.pfsp_devpool_step(pool, T.inst, "lb1_d", best, m=m, M=M, br=rule)
           for _ in range(2)]
    bo.check_step(exp, out[0][0], out[0][1], what)
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1], (what, "runs differ")
    return exp


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("inst", INSTS)
def test_step_random_pools(gpu, tables, pools, inst, rule):
    T = tables[inst]
    opt = gpu.taillard_best_ub(inst)
    mid = mid_best(T, pools[inst])
    for n in (257, 1000):  # every way of deciding occurs at `mid`
        kinds = decision_kinds(T, pools[inst][:n * NODE], mid)
        assert all(kinds.values()), (n, kinds)
    for n in SIZES:
        pool = pools[inst][:n * NODE]
        for best in (bo.HUGE, opt, mid):
            exp = run_step(gpu, T, pool, rule, best, (inst, rule, n, best))
            if best == bo.HUGE:  # every child kept
                assert exp.ctl["tree"] == sum(20 - pool[i] for i in range(0, len(pool), NODE)
                                              if pool[i] < 19)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("inst", INSTS)
def test_step_shallow_parents_fill_the_slabs(gpu, tables, inst, rule):
    # 257 parents of depth <= 2 with every child kept: block 0 emits 256 * 18+
    # children (its BLOCK * MAX_JOBS slab nearly full), block 1 the last parent's
    T = tables[inst]
    pool = bo.random_nodes(bo.rng(77 + inst), 257, max_depth=2)
    exp = run_step(gpu, T, pool, rule, bo.HUGE, (inst, rule, "shallow"))
    assert exp.ctl["tree"] >= 257 * 18 > 4608


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("inst", INSTS)
def test_step_bfs_frontier(gpu, tables, inst, rule):
    T = tables[inst]
    opt = gpu.taillard_best_ub(inst)
    # ta002's whole minbranch tree has 30 nodes: its widest frontier is 8 nodes
    target = 8 if (inst, rule) == (2, "minbranch") else 300
    pool = gpu.pfsp_bfs_frontier(inst, "lb1_d", 1, target, br=rule)[0]
    assert len(pool) >= target * NODE
    for best in (bo.HUGE, opt, opt + 40):
        run_step(gpu, T, pool, rule, best, (inst, rule, "frontier", best))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("inst", INSTS)
def test_step_pop_windows(gpu, tables, pools, inst, rule):
    T = tables[inst]
    n = 257
    pool = pools[inst][:n * NODE]
    mid = mid_best(T, pools[inst])
    for m, M in ((1, 7), (n, n), (n + 1, n)):
        exp = run_step(gpu, T, pool, rule, mid, (inst, rule, "window", m, M), m=m, M=M)
        assert exp.ctl["chunk"] == (0 if m > n else min(n, M))


# ---------------------------------------------------------------------------
# engines
# ---------------------------------------------------------------------------

MINBRANCH = {5: (11835, 266), 14: (19300, 16), 17: (34511286, 28316), 30: (2415778, 32)}


def counts(r):
    return r["tree"], r["sol"]


@pytest.mark.parametrize("inst", sorted(MINBRANCH))
@pytest.mark.parametrize("engine", ["devpool", "hostpool", "rooted"])
def test_engines_minbranch(gpu, inst, engine):
    if engine == "rooted":
        r = gpu.pfsp_gpu_rooted(inst, "lb1_d", 1, br="minbranch")
    else:
        r = gpu.pfsp_gpu(inst, "lb1_d", 1, mode=engine, br="minbranch")
    print(inst, engine, r["tree"], r["sol"], r["optimum"], r["time"])
    assert counts(r) == MINBRANCH[inst]
    assert r["optimum"] == gpu.taillard_best_ub(inst)


@pytest.mark.parametrize("engine", ["devpool", "hostpool", "rooted"])
@pytest.mark.parametrize("inst,br,want", [(14, "alt", (66801, 32)), (5, "bwd", (12288, 0))])
def test_engines_static_rules(gpu, inst, br, want, engine):
    if engine == "rooted":
        r = gpu.pfsp_gpu_rooted(inst, "lb1_d", 1, br=br)
    else:
        r = gpu.pfsp_gpu(inst, "lb1_d", 1, mode=engine, br=br)
    assert counts(r) == want
    assert r["optimum"] == gpu.taillard_best_ub(inst)


@pytest.mark.parametrize("engine", ["devpool", "hostpool", "rooted"])
@pytest.mark.parametrize("inst", [1, 14])
def test_engines_from_scratch(gpu, inst, engine):
    if engine == "rooted":
        r = gpu.pfsp_gpu_rooted(inst, "lb1_d", 0, br="minbranch")
    else:
        r = gpu.pfsp_gpu(inst, "lb1_d", 0, mode=engine, br="minbranch")
    assert r["optimum"] == gpu.taillard_best_ub(inst)


@pytest.mark.parametrize("engine", ["devpool", "hostpool", "rooted"])
def test_engines_small_chunks(gpu, engine):
    # M = 64 is honoured by hostpool only: in devpool mode --M is a floor under
    # the 2^19 chunk, so these runs use wide chunks, finish in a handful of
    # batches and replay no graph (test_gpu_devpool_loop.py does)
    if engine == "rooted":
        r = gpu.pfsp_gpu_rooted(14, "lb1_d", 1, M=64, br="minbranch")
    else:
        r = gpu.pfsp_gpu(14, "lb1_d", 1, m=25, M=64, mode=engine, br="minbranch")
    assert counts(r) == MINBRANCH[14]


def test_chain_matches_the_oracle(gpu, tables):
    # four iterations back to back on one set of buffers, as an engine thread
    # launches them; every transition against the one-step oracle
    T = tables[14]
    opt = gpu.taillard_best_ub(14)
    pool0 = gpu.pfsp_bfs_frontier(14, "lb1_d", 1, 64, br="minbranch")[0]
    windows = [64, 64, 8, 1024]
    snaps = gpu.pfsp_devpool_chain(pool0, 14, "lb1_d", opt, windows, capacity=16384,
                                   br="minbranch")
    pool, ctl = pool0, dict(tree=0, sol=0, iters=0, best=opt)
    for (pool_out, ctl_out), M in zip(snaps, windows):
        exp = bo.step(T, pool, "minbranch", ctl["best"], M=M, tree=ctl["tree"],
                      sol=ctl["sol"], iters=ctl["iters"])
        bo.check_step(exp, pool_out, ctl_out, ("chain", M))
        pool, ctl = pool_out, ctl_out


@pytest.mark.parametrize("mode", ["devpool", "hostpool"])
def test_from_pool_completes_a_minbranch_frontier(gpu, mode):
    for inst in (14, 5):
        pool, t1, s1, best = gpu.pfsp_bfs_frontier(inst, "lb1_d", 1, 500, br="minbranch")
        r = gpu.pfsp_gpu_from_pool(pool, inst, "lb1_d", 1, best, mode=mode, br="minbranch")
        assert (t1 + r["tree"], s1 + r["sol"]) == MINBRANCH[inst]


def test_gpu_frontier_completes_to_the_seq_total(gpu):
    pool, t1, s1, best = gpu.pfsp_gpu_frontier(14, "lb1_d", 1, 400, br="minbranch")
    assert len(pool) >= NODE
    r = gpu.pfsp_seq_from_pool(pool, 14, "lb1_d", 1, best, br="minbranch")
    assert (t1 + r["tree"], s1 + r["sol"]) == MINBRANCH[14]


def test_unsupported_bound_raises(gpu):
    with pytest.raises(ValueError, match="lb2"):
        gpu.pfsp_gpu(14, lb="lb2", br="alt")
