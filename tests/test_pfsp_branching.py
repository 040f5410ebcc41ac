"""Backward / alternating / dynamic (MinBranch) branching of the PFSP search,
CPU side: the C++ both-directions lb1_d bounds against the pure-Python oracle
(tests/helpers/bi_oracle.py), frozen sequential counts per rule, the support
matrix's error cells and the CLI flag. No GPU needed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bi_oracle as bo  # noqa: E402



def run_cli(args):
    import contextlib
    import io

    from gats_amd import cli

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = cli.main(args)
    return rc, buf.getvalue()


NODE = bo.NODE

# tree / sol of the sequential lb1_d search at ub = 1, per rule
FROZEN = {
    (1, "bwd"): (6, 0), (1, "alt"): (282, 0), (1, "minbranch"): (6, 0),
    (2, "alt"): (531953, 0), (2, "minbranch"): (30, 0),
    (3, "alt"): (46, 0), (3, "minbranch"): (27, 0),
    (5, "bwd"): (12288, 0), (5, "alt"): (425839, 1125), (5, "minbranch"): (11835, 266),
    (14, "alt"): (66801, 32), (14, "minbranch"): (19300, 16),
    (16, "alt"): (6096, 0), (16, "minbranch"): (1508, 0),
    (19, "alt"): (4939, 0), (19, "minbranch"): (86, 0),
}


@pytest.fixture(scope="module")
def tables(core):
    return {inst: bo.Tables(core, inst) for inst in (2, 14, 21)}


@pytest.fixture(scope="module")
def random_pools():
    # 7 forced edge cases + random (limit1, nback) nodes, per instance
    return {inst: bo.random_nodes(bo.rng(100 + inst), 120, force=bo.edge_cases())
            for inst in (2, 14, 21)}


def test_node_sets_cover_the_edge_cases(random_pools):
    for pool in random_pools.values():
        shapes = [bo.parse(pool[i:i + NODE]) for i in range(0, len(pool), NODE)]
        assert any(l1 == -1 and nb > 0 for _, l1, _, nb in shapes)
        assert any(nb == 0 for _, l1, _, nb in shapes)
        assert any(d == 19 for d, _, _, _ in shapes)
        assert all(d == l1 + 1 + nb <= 19 for d, l1, _, nb in shapes)


@pytest.mark.parametrize("inst", [2, 14, 21])
def test_cpu_bounds_bi_vs_python(core, tables, random_pools, inst):
    pool = random_pools[inst]
    lb_begin, lb_end = core.pfsp_cpu_bounds_bi(inst, pool)
    exp_begin, exp_end = bo.bounds_arrays(tables[inst], pool)
    assert list(lb_begin) == exp_begin
    assert list(lb_end) == exp_end


@pytest.mark.parametrize("inst", [2, 14, 21])
def test_last_level_bounds_are_the_makespan(core, tables, inst):
    T = tables[inst]
    r = bo.rng(7 + inst)
    force = [(l1, 18 - l1) for l1 in range(-1, 19)]  # every split of depth 19
    pool = bo.random_nodes(r, len(force), force=force)
    lb_begin, lb_end = core.pfsp_cpu_bounds_bi(inst, pool)
    for i in range(len(force)):
        depth, limit1, prmu, nback = bo.parse(pool[i * NODE:(i + 1) * NODE])
        assert depth == 19
        k = limit1 + 1  # the one unscheduled position; prmu is the full schedule
        cmax = bo.makespan(T, prmu)
        assert lb_begin[i * 20 + k] == cmax, (i, limit1, nback)
        assert lb_end[i * 20 + k] == cmax, (i, limit1, nback)
        assert sum(1 for v in lb_begin[i * 20:(i + 1) * 20] if v != -1) == 1


@pytest.mark.parametrize("inst,br", sorted(FROZEN))
def test_seq_frozen_counts(core, inst, br):
    r = core.pfsp_seq(inst, "lb1_d", 1, br=br)
    print(inst, br, r["tree"], r["sol"], r["optimum"])
    assert (r["tree"], r["sol"]) == FROZEN[(inst, br)]
    assert r["optimum"] == core.taillard_best_ub(inst)


@pytest.mark.parametrize("inst,br", [(1, "bwd"), (1, "minbranch"), (3, "alt"),
                                     (3, "minbranch"), (19, "minbranch")])
def test_python_search_agrees_with_seq(core, inst, br):
    # the oracle's own search (small trees) reproduces the frozen counts
    T = bo.Tables(core, inst)
    tree, sol, best = bo.search(T, br, core.taillard_best_ub(inst))
    assert (tree, sol) == FROZEN[(inst, br)]
    assert best == core.taillard_best_ub(inst)


@pytest.mark.parametrize("inst", range(1, 11))
def test_seq_minbranch_from_scratch_finds_the_optimum(core, inst):
    r = core.pfsp_seq(inst, "lb1_d", 0, br="minbranch")
    print(inst, r["tree"], r["sol"], r["optimum"])
    assert r["optimum"] == core.taillard_best_ub(inst)
    assert r["tree"] <= 116807  # largest tree of the CPU prototype of the rule


def test_explicit_fwd_is_todays_tree(core):
    # frozen in tests/test_pfsp_seq.py for the call without br
    r = core.pfsp_seq(14, "lb1_d", 1, br="fwd")
    assert (r["tree"], r["sol"], r["optimum"]) == (2573652, 2648, 1377)
    r = core.pfsp_seq(2, "lb1_d", 1, br="fwd")
    assert (r["tree"], r["sol"], r["optimum"]) == (30, 0, 1359)
    for lb, ub in (("lb1", 1), ("lb2", 0)):
        a, b = core.pfsp_seq(2, lb, ub, br="fwd"), core.pfsp_seq(2, lb, ub)
        assert (a["tree"], a["sol"], a["optimum"]) == (b["tree"], b["sol"], b["optimum"])


# A static direction can be catastrophic: ta003 backward is 261,164,504 nodes
# with lb1 (the lb1_d figure too; 160 s on one core) and 15,548,594 with lb2
# (30-40 s). At ub = 1 pruning does not depend on the traversal, so the proof
# is split over host threads (the drains release the GIL) and the partial
# counts add up to the sequential tree.
TA003_BWD_TREE = {"lb1": (261164504, 5386189), "lb2": (15548594, 0)}


def threaded_proof(core, inst, lb, br, chunks=256, target=8192):
    from concurrent.futures import ThreadPoolExecutor

    pool, tree, sol, best = core.pfsp_bfs_frontier(inst, lb, 1, target, br=br)
    nodes = [pool[i:i + NODE] for i in range(0, len(pool), NODE)]
    parts = [b"".join(nodes[k::chunks]) for k in range(chunks)]
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        rs = list(ex.map(lambda p: core.pfsp_seq_from_pool(p, inst, lb, 1, best, br=br), parts))
    return (tree + sum(r["tree"] for r in rs), sol + sum(r["sol"] for r in rs),
            min([best] + [r["optimum"] for r in rs]))


@pytest.mark.parametrize("lb", ["lb1", "lb2"])
@pytest.mark.parametrize("br", ["bwd", "alt"])
@pytest.mark.parametrize("inst", [1, 3, 5])
def test_seq_static_rules_with_lb1_lb2(core, inst, br, lb):
    opt = core.taillard_best_ub(inst)
    if (inst, br) == (3, "bwd"):
        tree, sol, best = threaded_proof(core, inst, lb, br)
        print(inst, lb, br, "ub=1, threaded:", tree, sol, best)
        assert best == opt  # the whole tree holds nothing below the optimum
        assert (tree, sol) == TA003_BWD_TREE[lb]
        return
    r0 = core.pfsp_seq(inst, lb, 0, br=br)  # from scratch: reaches the optimum
    r1 = core.pfsp_seq(inst, lb, 1, br=br)  # from the optimum: proves it
    print(inst, lb, br, "ub=0:", r0["tree"], r0["sol"], "ub=1:", r1["tree"], r1["sol"])
    assert r0["optimum"] == opt
    assert r1["optimum"] == opt
    assert r1["tree"] <= r0["tree"]


def test_threaded_proof_adds_up_to_seq(core):
    # the splitting used above, checked where the sequential count is frozen
    assert threaded_proof(core, 5, "lb1", "alt", chunks=16, target=64)[:2] == (425839, 1125)
    assert threaded_proof(core, 14, "lb1_d", "minbranch", chunks=16, target=64)[:2] == (19300, 16)


def test_from_pool_rejects_back_nodes_under_fwd(core):
    pool = core.pfsp_bfs_frontier(14, "lb1_d", 1, 64, br="minbranch")[0]
    assert any(pool[i + 22] for i in range(0, len(pool), NODE))
    with pytest.raises(ValueError, match="nback"):
        core.pfsp_seq_from_pool(pool, 14, "lb1_d", 1, 0)
    with pytest.raises(ValueError, match="nback"):
        core.pfsp_seq_step(pool, 14, "lb1_d", 1, 0, 10)
    with pytest.raises(ValueError, match="nback"):  # before any HIP call
        core.pfsp_gpu_from_pool(pool, 14, "lb1_d", 1)


def test_frontier_plus_drain_equals_seq(core):
    # phase-1 BFS, bounded step and drain all pick the rule up from the instance
    for inst, br in ((14, "minbranch"), (14, "alt"), (5, "bwd")):
        pool, t1, s1, best = core.pfsp_bfs_frontier(inst, "lb1_d", 1, 64, br=br)
        t2, s2, best2, rest = core.pfsp_seq_step(pool, inst, "lb1_d", 1, best, 1000, br=br)
        r = core.pfsp_seq_from_pool(rest, inst, "lb1_d", 1, best2, br=br)
        assert (t1 + t2 + r["tree"], s1 + s2 + r["sol"]) == FROZEN[(inst, br)]


def test_unsupported_combinations_raise(core):
    root = bo.make_node(-1, 0, range(20))
    for lb in ("lb1", "lb2"):
        with pytest.raises(ValueError, match="minbranch"):
            core.pfsp_seq(2, lb, 1, br="minbranch")
        with pytest.raises(ValueError, match="minbranch"):
            core.pfsp_bfs_frontier(2, lb, 1, 8, br="minbranch")
        with pytest.raises(ValueError, match="minbranch"):
            core.pfsp_seq_step(root, 2, lb, 1, 0, 10, br="minbranch")
        with pytest.raises(ValueError, match="minbranch"):
            core.pfsp_seq_from_pool(root, 2, lb, 1, 0, br="minbranch")
        for br in ("bwd", "alt", "minbranch"):
            # every GPU-tier entry point validates before its first HIP call
            with pytest.raises(ValueError, match=lb):
                core.pfsp_gpu(2, lb, 1, br=br)
            with pytest.raises(ValueError, match=lb):
                core.pfsp_gpu(2, lb, 1, mode="hostpool", br=br)
            with pytest.raises(ValueError, match=lb):
                core.pfsp_gpu_rooted(2, lb, 1, br=br)
            with pytest.raises(ValueError, match=lb):
                core.pfsp_gpu_from_pool(root, 2, lb, 1, br=br)
            with pytest.raises(ValueError, match=lb):
                core.pfsp_gpu_frontier(2, lb, 1, 64, br=br)
            with pytest.raises(ValueError, match=lb):
                core.pfsp_devpool_step(root, 2, lb, 1278, br=br)
            with pytest.raises(ValueError, match=lb):
                core.pfsp_devpool_chain(root, 2, lb, 1278, [1], br=br)
    for br in ("bwd", "alt", "minbranch"):
        for lb in ("lb1", "lb1_d", "lb2"):
            with pytest.raises(ValueError, match="not yet"):
                core.pfsp_multigpu(2, lb, 1, br=br)
            with pytest.raises(ValueError, match="not yet"):
                core.PfspAsyncEngine(2, lb, 1, br=br)
            with pytest.raises(ValueError, match="not yet"):
                core.PfspAsyncEngine(root, 2, lb, 1, br=br)
    with pytest.raises(ValueError, match="bogus"):
        core.pfsp_seq(2, "lb1_d", 1, br="bogus")


def test_step_validation_knows_nback(core):
    back = bo.make_node(-1, 2, range(20))
    with pytest.raises(ValueError):  # forward kernels take limit2 == jobs for granted
        core.pfsp_devpool_step(back, 2, "lb1_d", 1278)
    bad = bytearray(back)
    bad[0] = 3  # depth != limit1 + 1 + nback
    with pytest.raises(ValueError, match="nback"):
        core.pfsp_devpool_step(bytes(bad), 2, "lb1_d", 1278, br="alt")
    with pytest.raises(ValueError):
        core.pfsp_cpu_bounds_bi(2, bo.make_node(10, 12, range(20))[:1] + bytes([10]) +
                                bytes(range(20)) + bytes([12, 0]))


def test_cli_minbranch(core):
    rc, out = run_cli(["pfsp", "--tier", "seq", "--br", "minbranch", "--inst", "14",
                       "--lb", "lb1_d"])
    assert rc == 0
    assert "Branching rule: minbranch" in out
    assert "Size of the explored tree: 19300" in out
    assert "Optimal makespan: 1377" in out


def test_cli_default_output_is_unchanged(core):
    # without --br the banner is today's, byte for byte: its one branching
    # line reads "fwd" (tests/test_cli.py freezes that line)
    rc, out = run_cli(["pfsp", "--tier", "seq", "--inst", "2", "--lb", "lb1_d"])
    _, out_fwd = run_cli(["pfsp", "--tier", "seq", "--inst", "2", "--lb", "lb1_d",
                          "--br", "fwd"])
    lines = [ln for ln in out.splitlines() if "Branching" in ln]
    assert lines == ["Branching rule: fwd"]
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith("Elapsed time")]
    assert strip(out) == strip(out_fwd)
    assert "Size of the explored tree: 30" in out


@pytest.mark.parametrize("tier", ["multigpu", "dist"])
def test_cli_rejects_rules_on_multi_tiers(core, tier, capsys):
    from gats_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.main(["pfsp", "--tier", tier, "--br", "alt", "--lb", "lb1_d"])
    assert e.value.code != 0
    assert "not yet supported" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["pfsp", "--tier", "seq", "--br", "minbranch", "--lb", "lb2"])
