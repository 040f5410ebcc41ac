"""The two-stage bound lb12 on the GPU: the eval kernel against the
pure-Python oracle (tests/helpers/lb12_oracle.py) and the C++ host rule, ONE
iteration of the expand kernel against the one-step oracle (run twice: the
pool and the control block must be byte-identical), a chain of iterations, and
the engines against the sequential counts.

The Python lb2 is the slow part, so pools of up to 257 nodes are checked
against it and the 1000-node pools against pfsp_cpu_bounds_lb12, which
tests/test_pfsp_lb12.py pins to the same oracle."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bi_oracle as bo  # noqa: E402
import lb12_oracle as lo  # noqa: E402

pytestmark = pytest.mark.gpu

NODE = bo.NODE
INSTS = (2, 14, 21)  # 10, 45 and 190 machine pairs: one partial round of the
#                      wave sweep, one partial round, three rounds (62 lanes in the last)
SIZES = (1, 255, 256, 257, 1000)
RULES = bo.RULES
PY_MAX = 257  # largest pool checked against the Python lb2


@pytest.fixture(scope="module")
def tables(core):
    return {inst: bo.Tables(core, inst) for inst in INSTS}


def fwd_nodes(rng, n, max_depth=19, force=()):
    """Random nodes with nothing fixed at the back (what the step entry point
    accepts under fwd); `force` lists the depths of the first nodes."""
    out = []
    for i in range(n):
        prmu = list(range(20))
        rng.shuffle(prmu)
        depth = force[i] if i < len(force) else rng.randint(0, max_depth)
        out.append(bo.make_node(depth - 1, 0, prmu))
    return b"".join(out)


@pytest.fixture(scope="module")
def pools():
    # per instance one 1000-node pool with random (limit1, nback), starting with
    # the edge cases, and one with nback == 0; smaller pools are their prefixes
    out = {}
    for inst in INSTS:
        out[inst, "bi"] = bo.random_nodes(bo.rng(5200 + inst), 1000, force=bo.edge_cases())
        out[inst, "fwd"] = fwd_nodes(bo.rng(6200 + inst), 1000, force=(0, 19, 18, 1))
    return out


def pool_of(pools, inst, rule, n):
    return pools[inst, "fwd" if rule == "fwd" else "bi"][:n * NODE]


def mid_best(T, pool):
    """The median lb1_d child bound of the pool's first 257 nodes: the filter
    prunes about half of the children, lb2 sees the rest."""
    vals = []
    for i in range(0, PY_MAX * NODE, NODE):
        f, b = bo.children_bounds(T, pool[i:i + NODE])
        vals += list(f.values()) + list(b.values())
    return sorted(vals)[len(vals) // 2]


def incumbents(gpu, T, pool):
    return (bo.HUGE, gpu.taillard_best_ub(T.inst), mid_best(T, pool))


_expected = {}


def expected_arrays(gpu, T, pool, rule, best):
    """(dir, values, is_lb2) of a pool in check_bounds' terms: Python up to
    PY_MAX nodes, the host rule's arrays beyond."""
    key = (T.inst, rule, best, pool)
    if key not in _expected:
        n = len(pool) // NODE
        if n <= PY_MAX:
            _expected[key] = lo.bounds_arrays(T, pool, rule, best)
        else:
            d, v = gpu.pfsp_cpu_bounds_lb12(T.inst, pool, best, rule)
            head = lo.bounds_arrays(T, pool[:PY_MAX * NODE], rule, best)
            assert list(d[:PY_MAX]) == head[0]
            # beyond the Python prefix a host value above best may be an early
            # exit's: the kernel's must be above best too, all others are exact
            kinds = head[2] + [x > best for x in v[PY_MAX * T.jobs:]]
            _expected[key] = (list(d), list(v), kinds)
    return _expected[key]


check_values = lo.check_bounds


# ---------------------------------------------------------------------------
# eval kernel
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("inst", INSTS)
def test_eval_kernel(gpu, tables, pools, inst, rule):
    T = tables[inst]
    big = pools[inst, "bi"]
    for best in incumbents(gpu, T, big):
        for n in SIZES:
            pool = big[:n * NODE]
            exp = expected_arrays(gpu, T, big[:(PY_MAX if n <= PY_MAX else n) * NODE], rule, best)
            exp = tuple(a[:n * (1 if j == 0 else T.jobs)] for j, a in enumerate(exp))
            d, v = gpu.pfsp_gpu_bounds_lb12(inst, pool, best, rule)
            check_values(exp, (list(d), v), best, (inst, rule, n, best))
            if best == bo.HUGE and n <= PY_MAX:  # no early exit: every value exact
                assert list(v) == exp[1]


def test_eval_edge_nodes(gpu, tables):
    # nothing fixed at the front with jobs at the back under a FRONT direction
    # (the child's front starts from zeros, not from min_heads), nothing at the
    # back under bwd (the child's back starts from zeros, not from min_tails)
    force = bo.edge_cases() + [(-1, 2), (-1, 4), (-1, 6), (3, 0), (0, 0)]
    pool = bo.random_nodes(bo.rng(31), len(force), force=force)
    for inst in INSTS:
        T = tables[inst]
        for rule in RULES:
            for best in (bo.HUGE, gpu.taillard_best_ub(inst) + 200):
                exp = lo.bounds_arrays(T, pool, rule, best)
                d, v = gpu.pfsp_gpu_bounds_lb12(inst, pool, best, rule)
                check_values(exp, (list(d), v), best, (inst, rule, best))
                if best != bo.HUGE:
                    continue
                shapes = [bo.parse(pool[i:i + NODE]) for i in range(0, len(pool), NODE)]
                if rule in ("fwd", "alt"):
                    assert any(l1 == -1 and nb > 0 and d[i] == 0 and any(exp[2][i * 20:i * 20 + 20])
                               for i, (_, l1, _, nb) in enumerate(shapes)), rule
                if rule == "bwd":
                    assert any(nb == 0 and d[i] == 1 and any(exp[2][i * 20:i * 20 + 20])
                               for i, (_, _, _, nb) in enumerate(shapes))


# ---------------------------------------------------------------------------
# one expand iteration
# ---------------------------------------------------------------------------

def oracle_step(gpu, T, pool, rule, best, m=1, M=None):
    if len(pool) // NODE <= PY_MAX:
        return lo.step(T, pool, rule, best, m=m, M=M)
    d, v, _ = expected_arrays(gpu, T, pool, rule, best)
    return lo.step_from_arrays(T, pool, d, v, best, m=m, M=M)


def run_step(gpu, T, pool, rule, best, what, m=1, M=None, exp=None):
    if exp is None:
        exp = oracle_step(gpu, T, pool, rule, best, m=m, M=M)
    out = [gpu.pfsp_devpool_step(pool, T.inst, "lb12", best, m=m, M=M, br=rule)
           for _ in range(2)]
    lo.check_step(exp, out[0][0], out[0][1], what)
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1], (what, "runs differ")
    return exp


def survivors_per_block(T, pool, rule, best):
    """lb1_d survivors (= lb2 evaluations) per 256-parent block."""
    kinds = lo.bounds_arrays(T, pool, rule, best)[2]
    per = 256 * T.jobs
    return [sum(kinds[i:i + per]) for i in range(0, len(kinds), per)]


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("inst", INSTS)
def test_step_random_pools(gpu, tables, pools, inst, rule):
    T = tables[inst]
    bests = incumbents(gpu, T, pool_of(pools, inst, rule, 1000))
    odd = 0
    for best in bests + (0,):
        for n in SIZES:
            pool = pool_of(pools, inst, rule, n)
            exp = run_step(gpu, T, pool, rule, best, (inst, rule, n, best))
            if best == 0:  # nothing survives anywhere
                assert exp.ctl["tree"] == 0 and exp.ctl["size"] == 0
            if n == PY_MAX:
                odd += sum(q % 4 != 0 for q in survivors_per_block(T, pool, rule, best))
    assert odd > 0  # queues the four waves do not share out evenly


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("inst", INSTS)
def test_step_shallow_parents_fill_the_queue(gpu, tables, inst, rule):
    # 257 parents of depth <= 2, every child kept: block 0's survivor queue and
    # slab hold 256 * 18+ of their 256 * 20 entries, block 1 the last parent's
    T = tables[inst]
    if rule == "fwd":
        pool = fwd_nodes(bo.rng(77 + inst), 257, max_depth=2)
    else:
        pool = bo.random_nodes(bo.rng(77 + inst), 257, max_depth=2)
    # the host rule's arrays (no early exit at HUGE: exact values) keep this
    # quick; the first parents go through the Python lb2 as well
    d, v = gpu.pfsp_cpu_bounds_lb12(inst, pool, bo.HUGE, rule)
    head = lo.bounds_arrays(T, pool[:8 * NODE], rule, bo.HUGE)
    assert (list(d[:8]), list(v[:8 * 20])) == head[:2]
    exp = lo.step_from_arrays(T, pool, d, v, bo.HUGE)
    assert exp.ctl["tree"] >= 257 * 18 > 4608
    out = [gpu.pfsp_devpool_step(pool, inst, "lb12", bo.HUGE, br=rule) for _ in range(2)]
    lo.check_step(exp, out[0][0], out[0][1], (inst, rule, "shallow"))
    assert out[0] == out[1]


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("inst", INSTS)
def test_step_edge_nodes(gpu, tables, inst, rule):
    T = tables[inst]
    if rule == "fwd":
        pool = fwd_nodes(bo.rng(5), 8, force=(0, 19, 18, 1, 2))
    else:
        force = bo.edge_cases() + [(-1, 2), (-1, 4), (-1, 6), (3, 0), (0, 0)]
        pool = bo.random_nodes(bo.rng(31), len(force), force=force)
    for best in (bo.HUGE, gpu.taillard_best_ub(inst) + 200, gpu.taillard_best_ub(inst)):
        run_step(gpu, T, pool, rule, best, (inst, rule, "edge", best))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("inst", INSTS)
def test_step_pop_windows(gpu, tables, pools, inst, rule):
    T = tables[inst]
    n = 257
    pool = pool_of(pools, inst, rule, n)
    mid = mid_best(T, pool_of(pools, inst, rule, 1000))
    for m, M in ((1, 7), (n, n), (n + 1, n)):
        exp = run_step(gpu, T, pool, rule, mid, (inst, rule, "window", m, M), m=m, M=M)
        assert exp.ctl["chunk"] == (0 if m > n else min(n, M))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("inst", INSTS)
def test_step_bfs_frontier(gpu, tables, inst, rule):
    T = tables[inst]
    opt = gpu.taillard_best_ub(inst)
    # ta002's whole lb12 tree under fwd / minbranch has 7 nodes
    target = 3 if (inst, rule) in ((2, "fwd"), (2, "minbranch")) else 300
    pool = gpu.pfsp_bfs_frontier(inst, "lb12", 1, target, br=rule)[0]
    assert len(pool) >= target * NODE
    for best in (bo.HUGE, opt, opt + 40):
        exp = None
        if best == bo.HUGE and inst == 21:
            # ~300 * 17 Python sweeps of 190 pairs would take seconds: the host
            # rule's arrays (exact at HUGE, pinned by the CPU tests) stand in
            d, v = gpu.pfsp_cpu_bounds_lb12(inst, pool, best, rule)
            exp = lo.step_from_arrays(T, pool, d, v, best)
        run_step(gpu, T, pool, rule, best, (inst, rule, "frontier", best), exp=exp)


def test_chain_matches_the_oracle(gpu, tables):
    # four iterations back to back on one set of buffers, as an engine thread
    # launches them; every transition against the one-step oracle
    T = tables[14]
    opt = gpu.taillard_best_ub(14)
    pool0 = gpu.pfsp_bfs_frontier(14, "lb12", 1, 64, br="minbranch")[0]
    windows = [64, 64, 8, 1024]
    snaps = gpu.pfsp_devpool_chain(pool0, 14, "lb12", opt, windows, capacity=16384,
                                   br="minbranch")
    pool, ctl = pool0, dict(tree=0, sol=0, iters=0, best=opt)
    for (pool_out, ctl_out), M in zip(snaps, windows):
        exp = lo.step(T, pool, "minbranch", ctl["best"], M=M, tree=ctl["tree"],
                      sol=ctl["sol"], iters=ctl["iters"])
        lo.check_step(exp, pool_out, ctl_out, ("chain", M))
        pool, ctl = pool_out, ctl_out
    assert ctl["tree"] > 0


# ---------------------------------------------------------------------------
# engines
# ---------------------------------------------------------------------------

# tree / sol of the sequential lb12 search at ub = 1 (tests/test_pfsp_lb12.py;
# the ta017 / ta030 figures are the CPU prototype's)
SEQ = {
    (1, "minbranch"): (0, 0), (2, "minbranch"): (7, 0), (2, "fwd"): (7, 0),
    (2, "alt"): (25513, 0), (5, "bwd"): (250, 0), (5, "minbranch"): (4851, 0),
    (5, "alt"): (89560, 0), (14, "minbranch"): (15261, 0), (14, "alt"): (45146, 0),
    (14, "fwd"): (144639, 0), (17, "minbranch"): (6219204, 0), (17, "bwd"): (1460107, 0),
    (30, "minbranch"): (1477217, 0),
}
ENGINES = ["devpool", "hostpool", "rooted"]


def run_engine(gpu, engine, inst, ub, br, **kw):
    if engine == "rooted":
        kw.pop("m", None)
        return gpu.pfsp_gpu_rooted(inst, "lb12", ub, br=br, **kw)
    return gpu.pfsp_gpu(inst, "lb12", ub, mode=engine, br=br, **kw)


@pytest.mark.parametrize("inst,br", sorted(SEQ))
@pytest.mark.parametrize("engine", ENGINES)
def test_engines_match_seq(gpu, inst, br, engine):
    r = run_engine(gpu, engine, inst, 1, br)
    print(inst, br, engine, r["tree"], r["sol"], r["optimum"], r["time"])
    assert (r["tree"], r["sol"]) == SEQ[(inst, br)]
    assert r["optimum"] == gpu.taillard_best_ub(inst)


@pytest.mark.parametrize("engine", ENGINES)
def test_engines_small_chunks(gpu, engine):
    # M = 64 is honoured by hostpool only: in devpool mode --M is a floor under
    # the 2^19 chunk, so these runs use wide chunks, finish in a handful of
    # batches and replay no graph (test_gpu_devpool_loop.py does)
    r = run_engine(gpu, engine, 14, 1, "minbranch", m=25, M=64)
    assert (r["tree"], r["sol"]) == SEQ[(14, "minbranch")]


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("inst", [1, 14])
def test_engines_from_scratch(gpu, inst, engine):
    r = run_engine(gpu, engine, inst, 0, "minbranch")
    assert r["optimum"] == gpu.taillard_best_ub(inst)


@pytest.mark.parametrize("mode", ["devpool", "hostpool"])
def test_from_pool_completes_a_frontier(gpu, mode):
    for inst, br in ((14, "minbranch"), (5, "alt")):
        pool, t1, s1, best = gpu.pfsp_bfs_frontier(inst, "lb12", 1, 500, br=br)
        r = gpu.pfsp_gpu_from_pool(pool, inst, "lb12", 1, best, mode=mode, br=br)
        assert (t1 + r["tree"], s1 + r["sol"]) == SEQ[(inst, br)]


def test_gpu_frontier_completes_to_the_seq_total(gpu):
    for inst, br in ((14, "minbranch"), (14, "fwd")):
        pool, t1, s1, best = gpu.pfsp_gpu_frontier(inst, "lb12", 1, 400, br=br)
        assert len(pool) >= NODE
        r = gpu.pfsp_seq_from_pool(pool, inst, "lb12", 1, best, br=br)
        assert (t1 + r["tree"], s1 + r["sol"]) == SEQ[(inst, br)]
