"""The two-stage bound lb12 (lb1_d picks the direction and filters the
children, lb2 bounds the survivors), CPU side: the C++ rule against the
pure-Python oracle (tests/helpers/lb12_oracle.py), sequential counts per
branching rule, frontier / drain / threaded splits, the tiers that reject the
bound, and the CLI. No GPU needed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bi_oracle as bo  # noqa: E402
import lb12_oracle as lo  # noqa: E402

NODE = bo.NODE
INSTS = (2, 14, 21)

# tree / sol of the sequential lb12 search at ub = 1: the trees small enough
# for the Python search ...
SMALL = {
    (2, "minbranch"): (7, 0), (2, "fwd"): (7, 0), (5, "bwd"): (250, 0),
    (5, "minbranch"): (4851, 0),
    (1, "fwd"): (0, 0), (1, "bwd"): (0, 0), (1, "alt"): (0, 0), (1, "minbranch"): (0, 0),
}
# ... and the larger ones, frozen from the CPU prototype of the rule
FROZEN = {
    (2, "alt"): (25513, 0), (5, "alt"): (89560, 0), (14, "minbranch"): (15261, 0),
    (14, "alt"): (45146, 0), (14, "fwd"): (144639, 0),
}


def run_cli(args):
    import contextlib
    import io

    from gats_amd import cli

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = cli.main(args)
    return rc, buf.getvalue()


@pytest.fixture(scope="module")
def tables(core):
    return {inst: bo.Tables(core, inst) for inst in INSTS}


@pytest.fixture(scope="module")
def pools():
    return {inst: bo.random_nodes(bo.rng(1200 + inst), 64, force=bo.edge_cases())
            for inst in INSTS}


def mid_best(T, pool):
    """An incumbent inside the range of the pool's lb1_d child bounds (their
    median): some children fall to the filter, some reach lb2."""
    vals = []
    for i in range(0, len(pool), NODE):
        f, b = bo.children_bounds(T, pool[i:i + NODE])
        vals += list(f.values()) + list(b.values())
    return sorted(vals)[len(vals) // 2]


def test_child_sides_start_from_zeros_where_nothing_is_fixed(core, tables):
    # the trap: a front child of a node with limit1 == -1 has a front of ONE job
    # scheduled from zeros (not min_heads + job), its back stays the parent's
    T = tables[14]
    node = bo.make_node(-1, 3, list(range(20)))
    job = 5
    front = lo.schedule_front(T, [job])
    assert front[0] == T.p[job] and T.min_heads[0] == 0
    assert front[1] == T.p[job] + T.p[20 + job]
    want = lo.lb2_general(T, front, lo.schedule_back(T, [17, 18, 19]), {job, 17, 18, 19})
    assert lo.child_lb2(T, node, 5, False) == want
    # a back child of a node with nback == 0: back from zeros, front min_heads
    node = bo.make_node(-1, 0, list(range(20)))
    want = lo.lb2_general(T, list(T.min_heads), lo.schedule_back(T, [job]), {job})
    assert lo.child_lb2(T, node, 5, True) == want
    # forward children of a forward node: the existing forward lb2
    node = bo.make_node(2, 0, list(range(20)))
    child = bo.child_of(T, node, 7, False)
    got = core.pfsp_cpu_bounds(14, "lb2", node, bo.HUGE)
    assert lo.child_lb2(T, node, 7, False) == got[7]
    assert child[:5] == bytes([4, 3, 0, 1, 2])


@pytest.mark.parametrize("rule", bo.RULES)
@pytest.mark.parametrize("inst", INSTS)
def test_cpu_bounds_lb12_vs_python(core, tables, pools, inst, rule):
    T, pool = tables[inst], pools[inst]
    opt = core.taillard_best_ub(inst)
    for best in (bo.HUGE, opt, mid_best(T, pool)):
        exp = lo.bounds_arrays(T, pool, rule, best)
        d, b = core.pfsp_cpu_bounds_lb12(inst, pool, best, rule)
        lo.check_bounds(exp, (list(d), b), best, (inst, rule, best))
        if best == bo.HUGE:  # nothing exits early: every value exact
            assert list(b) == exp[1]
        else:  # both stages prune somewhere, and something is kept
            kinds = {(k, v < best) for v, k in zip(exp[1], exp[2]) if v >= 0}
            if best != opt:
                assert {(False, False), (True, True)} <= kinds, kinds


@pytest.mark.parametrize("inst,br", sorted(SMALL))
def test_python_search_agrees_with_seq(core, inst, br):
    T = bo.Tables(core, inst)
    opt = core.taillard_best_ub(inst)
    r = core.pfsp_seq(inst, "lb12", 1, br=br)
    assert (r["tree"], r["sol"], r["optimum"]) == SMALL[(inst, br)] + (opt,)
    assert lo.search(T, br, opt) == SMALL[(inst, br)] + (opt,)


@pytest.mark.parametrize("inst,br", sorted(FROZEN))
def test_seq_frozen_counts(core, inst, br):
    r = core.pfsp_seq(inst, "lb12", 1, br=br)
    print(inst, br, r["tree"], r["sol"], r["optimum"])
    assert (r["tree"], r["sol"]) == FROZEN[(inst, br)]
    assert r["optimum"] == core.taillard_best_ub(inst)


@pytest.mark.parametrize("inst", [1, 2, 5, 14])
def test_seq_minbranch_from_scratch_finds_the_optimum(core, inst):
    r = core.pfsp_seq(inst, "lb12", 0, br="minbranch")
    print(inst, r["tree"], r["sol"], r["optimum"])
    assert r["optimum"] == core.taillard_best_ub(inst)


def test_frontier_plus_drain_equals_seq(core):
    for inst, br in ((14, "minbranch"), (14, "alt"), (5, "bwd"), (14, "fwd")):
        want = {**SMALL, **FROZEN}[(inst, br)]
        pool, t1, s1, best = core.pfsp_bfs_frontier(inst, "lb12", 1, 64, br=br)
        r = core.pfsp_seq_from_pool(pool, inst, "lb12", 1, best, br=br)
        assert (t1 + r["tree"], s1 + r["sol"]) == want
        t2, s2, best2, rest = core.pfsp_seq_step(pool, inst, "lb12", 1, best, 1000, br=br)
        r = core.pfsp_seq_from_pool(rest, inst, "lb12", 1, best2, br=br)
        assert (t1 + t2 + r["tree"], s1 + s2 + r["sol"]) == want


def test_threaded_proof_adds_up_to_seq(core):
    from concurrent.futures import ThreadPoolExecutor

    for inst, br in ((14, "minbranch"), (14, "alt")):
        pool, tree, sol, best = core.pfsp_bfs_frontier(inst, "lb12", 1, 64, br=br)
        nodes = [pool[i:i + NODE] for i in range(0, len(pool), NODE)]
        parts = [b"".join(nodes[k::16]) for k in range(16)]
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            rs = list(ex.map(
                lambda p: core.pfsp_seq_from_pool(p, inst, "lb12", 1, best, br=br), parts))
        assert (tree + sum(r["tree"] for r in rs),
                sol + sum(r["sol"] for r in rs)) == FROZEN[(inst, br)]


def test_from_pool_rejects_back_nodes_under_fwd(core):
    pool = core.pfsp_bfs_frontier(14, "lb12", 1, 64, br="minbranch")[0]
    assert any(pool[i + 22] for i in range(0, len(pool), NODE))
    with pytest.raises(ValueError, match="nback"):
        core.pfsp_seq_from_pool(pool, 14, "lb12", 1, 0)
    with pytest.raises(ValueError, match="nback"):  # before any HIP call
        core.pfsp_gpu_from_pool(pool, 14, "lb12", 1)
    with pytest.raises(ValueError, match="nback|limit1"):  # the step's host validation
        core.pfsp_devpool_step(pool, 14, "lb12", 1377)


def test_multi_tiers_and_async_engine_reject_lb12(core):
    root = bo.make_node(-1, 0, range(20))
    with pytest.raises(ValueError, match="not yet supported"):
        core.pfsp_multigpu(14, "lb12", 1)
    with pytest.raises(ValueError, match="not yet supported"):
        core.pfsp_multigpu(14, "lb12", 1, eval="cpu")
    with pytest.raises(ValueError, match="not yet supported"):
        core.PfspAsyncEngine(14, "lb12")
    with pytest.raises(ValueError, match="not yet supported"):
        core.PfspAsyncEngine(root, 14, "lb12")
    from gats_amd import dist

    for fn in (dist.run_pfsp, dist.run_pfsp_shared_ub, dist.run_pfsp_live):
        with pytest.raises(ValueError, match="not yet supported"):
            fn(14, "lb12")


def test_bad_nodes_never_reach_the_rule(core):
    with pytest.raises(ValueError, match="exceeds jobs"):
        core.pfsp_cpu_bounds_lb12(14, bo.make_node(10, 10, range(20)), 1377, "fwd")
    bad = bytearray(bo.make_node(3, 2, range(20)))
    bad[5] = 20
    with pytest.raises(ValueError, match="prmu"):
        core.pfsp_cpu_bounds_lb12(14, bytes(bad), 1377, "fwd")
    bad = bytearray(bo.make_node(3, 2, range(20)))
    bad[0] = 7
    with pytest.raises(ValueError, match="depth"):
        core.pfsp_gpu_bounds_lb12(14, bytes(bad), 1377, "alt")  # before any HIP call
    with pytest.raises(ValueError, match="branching"):
        core.pfsp_cpu_bounds_lb12(14, bo.make_node(3, 2, range(20)), 1377, "sideways")


def test_cli_seq_run_prints_the_frozen_count(core):
    rc, out = run_cli(["pfsp", "--inst", "14", "--lb", "lb12", "--br", "minbranch",
                       "--tier", "seq"])
    assert rc == 0
    assert "Lower bound function: lb12" in out
    assert "Branching rule: minbranch" in out
    assert "Size of the explored tree: 15261" in out
    assert "Optimal makespan: 1377" in out


@pytest.mark.parametrize("tier", ["multigpu", "dist"])
def test_cli_rejects_lb12_on_the_multi_tiers(tier, capsys):
    with pytest.raises(SystemExit) as e:
        run_cli(["pfsp", "--inst", "14", "--lb", "lb12", "--tier", tier])
    assert e.value.code == 2
    assert "not yet supported" in capsys.readouterr().err
