"""The loop-driver checkers (helpers/devpool_loop_oracle.py) proved on the CPU.

  * loop_model — the driver's decision rules over the step oracle in oracle
    order — produces a trace the checkers accept, with the frozen sequential
    totals where a case runs a whole tree;
  * every input of tests/test_gpu_devpool_loop.py reaches its path on the model
    with a factor 2 of slack (the path conditions are conditions on the input,
    not measurements of a GPU run: a different child order on the GPU still
    reaches the path);
  * the checkers raise on each single corruption of a correct trace;
  * nq_devpool_loop / pfsp_devpool_loop reject malformed input on the host,
    before the first HIP call (no GPU needed);
  * the same for the share runs (several slice threads over one SliceShare,
    tests/test_gpu_devpool_share.py): every pool reaches its donation floor on
    the one-thread model with a factor 2 of slack (or, at the real floor's
    edge, by arithmetic), check_share accepts a consistent set of traces and
    raises on each single corruption, and nq_devpool_share /
    pfsp_devpool_share validate on the host."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import devpool_loop_oracle as orc  # noqa: E402
import devpool_step_oracle as step  # noqa: E402

NODE = orc.NODE
_models = {}


def model(core, name):
    """(case, pool, bfs tree, bfs sol, seq, model result): computed once, never
    modified (corruption tests work on copies)."""
    if name not in _models:
        c = orc.CASES[name]
        pool, t0, s0 = orc.case_pool(core, c)
        _models[name] = (c, pool, t0, s0, orc.case_seq(core, c), orc.case_model(core, c))
    return _models[name]


def copy_of(out):
    o = dict(out)
    o["trace"] = [dict(r, ctl=dict(r["ctl"])) if r["kind"] == "batch" else dict(r)
                  for r in out["trace"]]
    o["diag"] = dict(out["diag"])
    return o


def check(core, name, out):
    c, pool, _, _, seq, _ = model(core, name)
    orc.check_trace(out, c.cfg(), len(pool) // NODE)
    from_batch = 0 if c.lower_at is None else c.lower_at
    total = orc.check_conservation(out, pool, seq, c.cfg(), from_batch=from_batch)
    orc.check_final(out, seq, total)
    return total


# ---- the model's own trace is accepted, and every input reaches its path ----

@pytest.mark.parametrize("name", sorted(orc.CASES))
def test_model_trace_is_accepted_and_reaches_the_path(core, name):
    c, pool, t0, s0, seq, out = model(core, name)
    total = check(core, name, out)
    if c.whole_tree is not None:
        assert (t0 + total[0], s0 + total[1]) == c.whole_tree
    if c.lower_at is None:
        assert total == seq(pool)
    n = orc.case_counts(out)
    orc.check_need(n, c.need, factor=2)
    assert c.need, "every case names its path"


def test_model_paths_in_detail(core):
    n = {name: orc.case_counts(model(core, name)[5]) for name in orc.CASES}
    # a: no graph, no spill, fewer than m leftovers
    for name in ("grow_nq", "grow_lb1"):
        assert n[name]["replays"] == n[name]["spills"] == 0
        assert len(model(core, name)[5]["leftover"]) // NODE < 25
    # b / f: replays, then eager batches once the pool is below 4096
    for name in ("graph_nq", "graph_lb12"):
        assert n[name]["captures"] == 1 and n[name]["parity1"] == 0
    # c: a graph is allowed, full batches happen, none is replayed
    assert n["parity_nq"]["replays"] == 0 and n["parity_nq"]["full_on_parity1"] >= 2
    bs = orc.batches_of(model(core, "parity_nq")[5]["trace"])
    assert bs[0]["b"] == 15 and {r["parity"] for r in bs[1:]} == {0, 1}
    # d': the first run stays on control block 1 after its one-iteration batch
    # and never replays; the drained run does
    out = model(core, "spill_then_graph_nq")[5]
    runs = orc.runs_of(out["trace"])
    assert [r["kind"] for r in runs[0][1][:2]] == ["batch", "spill"] and runs[0][1][0]["b"] == 1
    assert not any(r["kind"] == "batch" and r["graph"] for r in runs[0][1])
    assert n["spill_then_graph_nq"]["replays_in_drained"] >= 6
    # e: the block of the batch after the hook carries the optimum
    c, _, _, _, _, out = model(core, "adopt_lb1_d")
    opt = core.taillard_best_ub(c.inst)
    best = [r["ctl"]["best"] for r in orc.batches_of(out["trace"])]
    assert best[:c.lower_at + 1] == [opt + c.best_delta] * (c.lower_at + 1)
    assert set(best[c.lower_at + 1:]) == {opt}


@pytest.mark.parametrize("name", ["spill_nq", "spill_lb1"])
def test_spill_cases_spill_whatever_the_child_order(core, name):
    # the arithmetic of the comment above the two cases
    c, pool, _, _, _, out = model(core, name)
    cfg, n0 = c.cfg(), len(pool) // NODE
    assert cfg.capacity - n0 < cfg.growth                      # first turn: one iteration
    s1 = n0 - c.chunk                                          # at least this many after it
    assert orc.batch_len(cfg, s1, 1) == "spill"
    assert orc.batch_len(cfg, s1 - s1 // 2, 1) == "spill"      # and again after halving
    assert orc.batch_len(cfg, cfg.capacity, 1) == "spill"      # at most this many
    stack = s1 // 2 + (s1 - s1 // 2) // 2
    assert stack >= cfg.capacity // 2 >= 4 * c.m
    assert orc.batch_len(cfg, cfg.capacity // 2, 0) == 1       # the drained run's first turn
    assert orc.batch_len(cfg, cfg.capacity // 2 - c.chunk, 1) == "spill"
    assert orc.batch_len(cfg, cfg.capacity // 2 + cfg.growth, 1) == "spill"
    # the first iteration pops the same nodes on every run: its children fit
    first = orc.batches_of(out["trace"])[0]
    assert first["b"] == 1 and first["ctl"]["size"] <= cfg.capacity


def test_model_without_graph_never_replays(core):
    c = orc.CASES["graph_nq"]
    out = orc.case_model(core, c, graph=False)
    assert orc.case_counts(out)["replays"] == 0
    pool = model(core, "graph_nq")[1]
    orc.check_trace(out, c.cfg(False), len(pool) // NODE)
    with pytest.raises(AssertionError):  # a replayed batch where none is allowed
        orc.check_trace(model(core, "graph_nq")[5], c.cfg(False), len(pool) // NODE)


def test_model_overflow_raises(core):
    N, n, M = 12, 100, 60
    pool = step.random_nq_nodes(step.rng(8), n, N, max_depth=2)
    fn = lambda p, M_, t, s, i, b: step.nq_step(core, p, N, 1, -1, 1, M_, t, s, i)  # noqa: E731
    with pytest.raises(RuntimeError, match="device pool overflow"):
        orc.loop_model(fn, pool, orc.Cfg(1, M, N, n, True, 4))


def test_batch_len_rules():
    cfg = orc.Cfg(25, 256, 12, 1 << 16)          # growth 3072
    assert orc.batch_len(cfg, 100, 0) == 2        # small pool
    assert orc.batch_len(cfg, 4095, 7) == 2
    assert orc.batch_len(cfg, 4096, 0) == 16
    assert orc.batch_len(cfg, 65536 - 16 * 3072, 3) == 16
    assert orc.batch_len(cfg, 65536 - 16 * 3072 + 1, 3) == 15    # clamped, odd
    assert orc.batch_len(cfg, 65536 - 3072, 3) == 1
    assert orc.batch_len(cfg, 65536 - 3071, 3) == "spill"
    assert orc.batch_len(cfg, 65536 - 3071, 0) == 1              # never on the first turn
    tight = orc.Cfg(25, 64, 10, 700)              # growth 640
    assert orc.batch_len(tight, 99, 5) == 1       # below 4 m: no spill, one iteration
    assert orc.batch_len(tight, 100, 5) == "spill"
    assert orc.batch_len(orc.Cfg(25, 256, 1, 1 << 16), 100, 0) == 16  # per == 1: no short rule


# ---- each single corruption is caught ----

def first_index(trace, pred):
    return next(i for i, r in enumerate(trace) if pred(r))


def test_raises_on_a_batch_larger_than_the_room(core):
    out = copy_of(model(core, "parity_nq")[5])
    i = first_index(out["trace"], lambda r: r["kind"] == "batch")
    assert out["trace"][i]["b"] == 15
    out["trace"][i]["b"] = 16
    with pytest.raises(AssertionError, match="larger than the room"):
        check(core, "parity_nq", out)


def test_raises_on_a_long_batch_over_a_small_pool(core):
    out = copy_of(model(core, "grow_lb1")[5])
    i = first_index(out["trace"], lambda r: r["kind"] == "batch")
    out["trace"][i]["b"] = 3
    with pytest.raises(AssertionError, match="small pool"):
        check(core, "grow_lb1", out)


def test_raises_on_a_graph_batch_on_parity_1(core):
    out = copy_of(model(core, "parity_nq")[5])
    bs = orc.batches_of(out["trace"])
    r = next(r for k, r in enumerate(bs) if r["b"] == 16 and r["parity"] == 1 and k >= 4)
    r["graph"] = r["captured"] = True
    with pytest.raises(AssertionError):
        check(core, "parity_nq", out)


def test_raises_on_an_early_graph_batch(core):
    out = copy_of(model(core, "graph_nq")[5])
    bs = orc.batches_of(out["trace"])
    assert bs[3]["b"] == 16 and bs[3]["parity"] == 0 and not bs[3]["graph"]
    bs[3]["graph"] = bs[3]["captured"] = True
    bs[4]["captured"] = False
    with pytest.raises(AssertionError):
        check(core, "graph_nq", out)


@pytest.mark.parametrize("name", ["spill_lb1", "parity_nq"])
def test_raises_on_a_wrong_parity(core, name):
    out = copy_of(model(core, name)[5])
    bs = orc.batches_of(out["trace"])
    bs[len(bs) // 2]["parity"] ^= 1
    with pytest.raises(AssertionError, match="entry parity"):
        check(core, name, out)


@pytest.mark.parametrize("name", ["spill_nq", "spill_lb1"])
def test_raises_on_a_spill_of_the_front_half(core, name):
    out = copy_of(model(core, name)[5])
    i = first_index(out["trace"], lambda r: r["kind"] == "spill")
    sp, prev = out["trace"][i], out["trace"][i - 1]
    half = sp["size_before"] - sp["size_after"]
    assert prev["kind"] == "batch" and sp["moved"] == prev["pool"][sp["size_after"] * NODE:]
    sp["moved"] = prev["pool"][:half * NODE]
    assert sp["moved"] != prev["pool"][sp["size_after"] * NODE:]
    with pytest.raises(AssertionError, match="back half"):
        check(core, name, out)


def test_raises_on_a_spill_that_is_not_due(core):
    out = copy_of(model(core, "spill_lb1")[5])
    c = orc.CASES["spill_lb1"]
    i = first_index(out["trace"], lambda r: r["kind"] == "spill")
    assert out["trace"][i]["size_before"] >= 4 * c.m
    roomy = orc.Cfg(c.m, c.chunk, 20, c.capacity + c.chunk * 20)  # one more iteration fits
    with pytest.raises(AssertionError):
        orc.check_trace(out, roomy, 60)


@pytest.mark.parametrize("name", ["graph_nq", "spill_lb1", "graph_lb12"])
@pytest.mark.parametrize("what", ["lost", "duplicated"])
@pytest.mark.parametrize("where", ["prefix", "tail"])
def test_raises_on_one_node_lost_or_duplicated(core, name, what, where):
    c, pool, _, _, seq, good = model(core, name)
    out = copy_of(good)
    bs = orc.batches_of(out["trace"])
    r = bs[len(bs) // 2]
    p = r["pool"]
    n = len(p) // NODE
    assert n > 4
    # a node that matters to the counts, and a neighbour that differs from it
    idx = range(n - 1) if where == "prefix" else range(n - 2, -1, -1)
    i = next(i for i in idx if seq.seq_fn(p[i * NODE:(i + 1) * NODE]) != (0, 0)
             and p[i * NODE:(i + 1) * NODE] != p[(i + 1) * NODE:(i + 2) * NODE])
    if what == "lost":  # gone from the snapshot, and the size says so
        r["pool"] = p[:i * NODE] + p[(i + 1) * NODE:]
        r["ctl"]["size"] -= 1
    else:  # size right, the node's neighbour overwritten with it
        r["pool"] = p[:(i + 1) * NODE] + p[i * NODE:(i + 1) * NODE] + p[(i + 2) * NODE:]
    with pytest.raises(AssertionError):
        orc.check_conservation(out, pool, seq, c.cfg())


@pytest.mark.parametrize("field", ["tree", "sol"])
def test_raises_on_a_stale_control_block(core, field):
    # the readback of the other parity block: the counters of one iteration ago
    c, pool, _, _, seq, good = model(core, "spill_nq")
    out = copy_of(good)
    bs = orc.batches_of(out["trace"])
    k = next(k for k in range(len(bs) // 2, len(bs))
             if bs[k]["ctl"][field] != bs[k - 1]["ctl"][field])
    bs[k]["ctl"][field] = bs[k - 1]["ctl"][field]
    with pytest.raises(AssertionError, match="conservation"):
        orc.check_conservation(out, pool, seq, c.cfg())


def test_raises_on_wrong_diag_counters(core):
    for key in ("kernel_launch", "device_to_host", "host_to_device", "gpu_iters"):
        out = copy_of(model(core, "spill_lb1")[5])
        out["diag"][key] += 1
        with pytest.raises(AssertionError):
            check(core, "spill_lb1", out)


def test_raises_on_a_dropped_drain_run(core):
    c, pool, _, _, seq, good = model(core, "spill_lb1")
    out = copy_of(good)
    runs = orc.runs_of(out["trace"])
    assert len(runs) >= 3
    last = first_index(out["trace"], lambda r: r is runs[-1][0])
    out["trace"] = out["trace"][:last]  # the last drained chunk never re-run
    with pytest.raises(AssertionError):
        orc.check_trace(out, c.cfg(), len(pool) // NODE)


def test_raises_on_an_incumbent_not_adopted(core):
    # the device went on pruning with the stale incumbent: counts too high
    c, pool, _, _, seq, _ = model(core, "adopt_lb1_d")
    opt = core.taillard_best_ub(c.inst)
    stale = orc.loop_model(orc.case_step_fn(core, c), pool, c.cfg(), opt + c.best_delta, None)
    assert stale["tree"] > model(core, "adopt_lb1_d")[5]["tree"]
    with pytest.raises(AssertionError, match="conservation"):
        orc.check_conservation(stale, pool, seq, c.cfg(), from_batch=c.lower_at)


# ---- host validation of the two entry points: before any HIP call ----

NQ_OK = step.nq_node(2, [1, 3, 0, 2, 4, 5])
PF_OK = step.pfsp_node(3, list(range(20)))


def _pf(depth, prmu, limit1=None):
    b = bytearray(step.pfsp_node(depth & 0xFF, prmu))
    if limit1 is not None:
        b[1] = limit1 & 0xFF
    return bytes(b)


@pytest.mark.parametrize("kwargs", [
    dict(nodes=b""),                                   # an empty pool
    dict(nodes=NQ_OK[:23]),                            # length not a multiple of 24
    dict(N=3), dict(N=21), dict(N=0),
    dict(nodes=step.nq_node(7, range(6))),             # depth > N
    dict(nodes=step.nq_node(2, [1, 1, 0, 2, 4, 5])),   # duplicate entry
    dict(nodes=step.nq_node(2, [1, 3, 0, 2, 4, 6])),   # entry >= N
    dict(nodes=NQ_OK + step.nq_node(255, range(6))),   # second node bad
    dict(m=0), dict(m=-1), dict(m=(1 << 30) + 1),
    dict(chunk=0), dict(chunk=-5),
    dict(chunk=65, capacity=64),                       # chunk > capacity
    dict(chunk=(1 << 31) // 6 + 1, capacity=1 << 22),  # chunk * branching > 2^31
    dict(nodes=NQ_OK * 3, capacity=2),                 # capacity < len(nodes)
    dict(capacity=0), dict(capacity=-1),
    dict(capacity=(1 << 22) + 1),                      # trace bound
    dict(max_batches=-1), dict(max_batches=4097),
    dict(finish=-2), dict(finish=9),
    dict(g=0),
])
def test_nq_loop_rejects_malformed_input(core, kwargs):
    args = dict(nodes=NQ_OK, N=6, chunk=8, capacity=64, max_batches=2)
    args.update(kwargs)
    with pytest.raises(ValueError):
        core.nq_devpool_loop(**args)


@pytest.mark.parametrize("kwargs", [
    dict(nodes=b""),
    dict(nodes=PF_OK + b"\0"),
    dict(nodes=_pf(3, [0] + list(range(19)))),                # duplicate job
    dict(nodes=_pf(3, list(range(19)) + [20])),               # job >= jobs
    dict(nodes=_pf(20, list(range(20)))),                     # depth > jobs - 1
    dict(nodes=_pf(-1, list(range(20)), limit1=-2)),          # depth < 0
    dict(nodes=_pf(3, list(range(20)), limit1=3)),            # limit1 != depth - 1
    dict(nodes=PF_OK + _pf(5, list(range(20)), limit1=0)),    # second node bad
    dict(m=0), dict(m=-1), dict(m=(1 << 30) + 1),
    dict(chunk=0), dict(chunk=65, capacity=64),
    dict(chunk=(1 << 31) // 20 + 1, capacity=1 << 22),
    dict(nodes=PF_OK * 2, capacity=1),
    dict(capacity=0), dict(capacity=(1 << 22) + 1),
    dict(max_batches=-1), dict(max_batches=4097),
    dict(best=0), dict(best=-5),
    dict(lb="bogus"),
    dict(br="sideways"),
    dict(lb="lb1", br="minbranch"), dict(lb="lb2", br="bwd"),  # no such kernel
    dict(inst=31), dict(inst=0),
    dict(lower_best_at=(-1, 1377)), dict(lower_best_at=(2, 0)), dict(lower_best_at=(2, -3)),
])
def test_pfsp_loop_rejects_malformed_input(core, kwargs):
    args = dict(nodes=PF_OK, inst=2, lb="lb1", best=1359, chunk=8, capacity=64, max_batches=2)
    args.update(kwargs)
    with pytest.raises(ValueError):
        core.pfsp_devpool_loop(**args)


def test_lb12_nodes_with_jobs_at_the_back_need_their_rule(core):
    # a minbranch node handed to a forward run is refused on the host
    pool = core.pfsp_bfs_frontier(14, "lb12", 1, 400, "minbranch")[0]
    assert any(pool[i + 22] for i in range(0, len(pool), NODE))
    with pytest.raises(ValueError):
        core.pfsp_devpool_loop(pool, 14, "lb12", 1377, capacity=4096, max_batches=1)


# ---------------------------------------------------------------------------
# share runs: helpers/devpool_loop_oracle.py's SHARE_CASES and check_share
# ---------------------------------------------------------------------------

_share = {}


def share(core, name):
    """(case, pool, bfs tree, bfs sol, seq, one-thread model): computed once."""
    if name not in _share:
        c = orc.SHARE_CASES[name]
        pool, t0, s0 = orc.share_case_pool(core, c)
        _share[name] = (c, pool, t0, s0, orc.case_seq(core, c), orc.share_case_model(core, c))
    return _share[name]


@pytest.mark.parametrize("name", sorted(orc.SHARE_CASES))
def test_share_pool_reaches_its_floor_on_the_model(core, name):
    c, pool, t0, s0, seq, out = share(core, name)
    floor = c.floor_in_force()
    n = orc.at_floor(out, floor)
    print(name, "floor", floor, "readbacks at or above it", n, "of", len(orc.batches_of(out["trace"])))
    if c.floor == 0 and c.need.get("at_floor") and c.pool[0] == "leaves":
        assert n == 1                                  # the edge: exactly one, by arithmetic
    elif c.need.get("at_floor"):
        assert n >= 2 * c.need["at_floor"], (n, c.need)
    else:
        assert n == 0, "a case without a donation must stay below the floor"
    if c.whole_tree is not None:
        assert (t0 + out["tree"], s0 + out["sol"]) == c.whole_tree
    if c.problem == "pfsp":
        assert out["best"] == core.taillard_best_ub(c.inst)


@pytest.mark.parametrize("name, floor", [("edge_nq", 1 << 16), ("below_edge_nq", 1 << 16),
                                         ("two_m_nq", 80000), ("below_two_m_nq", 80000)])
def test_real_floor_edge_by_arithmetic(core, name, floor):
    c, pool, _, _, _, out = share(core, name)
    cfg, n0 = c.cfg(), len(pool) // NODE
    assert c.floor == 0 and cfg.floor == floor == core.donation_floor(c.m)
    b = orc.batch_len(cfg, n0, 0)                      # derived, not assumed
    assert b == orc.BATCH
    # leaf parents push nothing: every iteration loses exactly `chunk` nodes
    assert all(pool[i] == c.N for i in range(0, len(pool), NODE))
    edge = name in ("edge_nq", "two_m_nq")
    first = n0 - b * c.chunk
    assert first == (floor if edge else floor - 1)
    sizes = [r["ctl"]["size"] for r in orc.batches_of(out["trace"])]
    assert sizes[0] == first and all(s < floor for s in sizes[1:])
    # after the one donation of floor // 2 nodes neither half reaches the floor again
    assert first - first // 2 < floor
    if edge:
        assert first // 2 == floor // 2
    if name.endswith("two_m_nq"):
        assert floor == 2 * c.m > (1 << 16) and first >= (1 << 16)  # the 2m branch decides


def share_traces(core, name, threads=2):
    c, pool, _, _, seq, _ = share(core, name)
    key = (name, threads)
    if key not in _share:
        best = orc.case_best(core, c)
        _share[key] = orc.share_model(orc.case_step_fn(core, c), pool, c.cfg(), best, threads)
    return c, pool, seq, _share[key]


def copies(outs):
    return [copy_of(o) for o in outs]


def find(out, kind, k=0):
    return [i for i, r in enumerate(out["trace"]) if r["kind"] == kind][k]


@pytest.mark.parametrize("name, threads", [("mixed_nq_f-1", 2), ("mixed_nq_f3", 3),
                                           ("spill_nq", 2), ("lb1_d", 2), ("lb1_d", 4),
                                           ("root_nq_f3", 2)])
def test_check_share_accepts_a_consistent_set_of_traces(core, name, threads):
    c, pool, seq, outs = share_traces(core, name, threads)
    n = orc.share_counts(outs)
    # every thread donates once while its pool reaches the floor: lb1_d's third
    # half does not, and its fourth thread stays idle
    want = 2 if (name, threads) == ("lb1_d", 4) else threads - 1
    assert n["taken"] == n["takes"] == want and n["chains"] == want - 1, n
    assert n["idle_threads"] == threads - 1 - want
    total = orc.check_share(outs, pool, seq, c.cfg())
    assert total == seq(pool)
    # symmetric in the threads
    orc.check_share(outs[::-1], pool, seq, c.cfg())
    # and without the counts
    orc.check_share(outs, pool, None, c.cfg())


SHARE_BITES = ["mixed_nq_f-1", "lb1_d"]


@pytest.mark.parametrize("name", SHARE_BITES)
@pytest.mark.parametrize("what", ["dropped", "duplicated"])
@pytest.mark.parametrize("side", ["take", "both"])
def test_share_raises_on_one_donated_node_dropped_or_duplicated(core, name, what, side):
    c, pool, seq, good = share_traces(core, name)
    outs = copies(good)
    d = outs[0]["trace"][find(outs[0], "donate")]
    t = outs[1]["trace"][find(outs[1], "take")]
    run = outs[1]["trace"][find(outs[1], "run")]
    nodes = t["nodes"]
    i = (len(nodes) // NODE) // 2
    assert nodes[i * NODE:(i + 1) * NODE] != nodes[(i + 1) * NODE:(i + 2) * NODE]
    if what == "dropped":
        nodes = nodes[:i * NODE] + nodes[(i + 1) * NODE:]
        t["size"] -= 1
        run["init_size"] -= 1
    else:
        nodes = nodes[:(i + 1) * NODE] + nodes[i * NODE:(i + 1) * NODE] + nodes[(i + 2) * NODE:]
    t["nodes"] = nodes
    if side == "both":
        d["moved"] = nodes
    with pytest.raises(AssertionError):
        orc.check_share(outs, pool, seq, c.cfg())
    with pytest.raises(AssertionError):
        orc.check_share(outs, pool, None, c.cfg())


@pytest.mark.parametrize("name", SHARE_BITES)
def test_share_raises_on_the_front_half_donated(core, name):
    c, pool, seq, good = share_traces(core, name)
    outs = copies(good)
    i = find(outs[0], "donate")
    d, prev = outs[0]["trace"][i], outs[0]["trace"][i - 1]
    half = d["size_before"] // 2
    front = prev["pool"][:half * NODE]
    assert prev["kind"] == "batch" and front != d["moved"]
    d["moved"] = front
    outs[1]["trace"][find(outs[1], "take")]["nodes"] = front
    with pytest.raises(AssertionError, match="back half"):
        orc.check_share(outs, pool, None, c.cfg())


@pytest.mark.parametrize("name", SHARE_BITES)
@pytest.mark.parametrize("off", [-1, 1])
def test_share_raises_on_size_after_off_by_one(core, name, off):
    c, pool, seq, good = share_traces(core, name)
    outs = copies(good)
    outs[0]["trace"][find(outs[0], "donate")]["size_after"] += off
    with pytest.raises(AssertionError):
        orc.check_share(outs, pool, None, c.cfg())
    # ... also when the next batch agrees with the wrong size
    outs[0]["trace"][find(outs[0], "donate") + 1]["size_before"] += off
    with pytest.raises(AssertionError):
        orc.check_share(outs, pool, None, c.cfg())


@pytest.mark.parametrize("name", SHARE_BITES)
def test_share_raises_on_a_take_with_one_byte_changed(core, name):
    c, pool, seq, good = share_traces(core, name)
    outs = copies(good)
    t = outs[1]["trace"][find(outs[1], "take")]
    b = bytearray(t["nodes"])
    b[len(b) // 2] ^= 1
    t["nodes"] = bytes(b)
    with pytest.raises(AssertionError):
        orc.check_share(outs, pool, None, c.cfg())


def test_share_raises_on_a_thief_starting_above_the_offered_incumbent(core):
    c, pool, seq, good = share_traces(core, "lb1_d")
    outs = copies(good)
    t = outs[1]["trace"][find(outs[1], "take")]
    run = outs[1]["trace"][find(outs[1], "run")]
    assert run["best"] == t["best"]
    run["best"] += 1
    with pytest.raises(AssertionError, match="starts above the offer"):
        orc.check_share(outs, pool, seq, c.cfg())
    run["best"] -= 2  # a lower shared incumbent is fine
    orc.check_share(outs, pool, None, c.cfg())


def test_share_raises_on_a_wrong_offered_incumbent(core):
    c, pool, seq, good = share_traces(core, "lb1_d")
    outs = copies(good)
    outs[0]["trace"][find(outs[0], "donate")]["best"] += 1
    outs[1]["trace"][find(outs[1], "take")]["best"] += 1
    with pytest.raises(AssertionError, match="offered incumbent"):
        orc.check_share(outs, pool, None, c.cfg())


@pytest.mark.parametrize("name", SHARE_BITES)
def test_share_raises_on_a_donation_below_the_floor(core, name):
    c, pool, seq, good = share_traces(core, name)
    d = good[0]["trace"][find(good[0], "donate")]
    cfg = c.cfg()
    cfg.floor = d["size_before"]
    orc.check_share(good, pool, None, cfg)
    cfg.floor = d["size_before"] + 1
    with pytest.raises(AssertionError, match="below the floor"):
        orc.check_share(good, pool, None, cfg)


@pytest.mark.parametrize("name", SHARE_BITES)
def test_share_raises_on_a_stale_prefix_after_a_donation(core, name):
    c, pool, seq, good = share_traces(core, name)
    i = find(good[0], "donate")
    d, nxt = good[0]["trace"][i], good[0]["trace"][i + 1]
    keep = (d["size_after"] - nxt["b"] * c.chunk) * NODE
    assert nxt["kind"] == "batch" and keep > NODE
    # one byte of the kept front changed
    outs = copies(good)
    b = bytearray(nxt["pool"])
    b[keep - NODE + 1] ^= 1
    outs[0]["trace"][i + 1]["pool"] = bytes(b)
    with pytest.raises(AssertionError, match="un-popped prefix"):
        orc.check_share(outs, pool, None, c.cfg())
    # the donor went on with the size it had before the donation
    outs = copies(good)
    outs[0]["trace"][i + 1]["size_before"] = d["size_before"]
    with pytest.raises(AssertionError):
        orc.check_share(outs, pool, None, c.cfg())


def test_share_raises_on_unmatched_takes_and_offers(core):
    c, pool, seq, good = share_traces(core, "mixed_nq_f-1")
    # a take without a donation: the donor's record gone, its sizes patched up
    outs = copies(good)
    del outs[0]["trace"][find(outs[0], "donate")]
    with pytest.raises(AssertionError):
        orc.check_share(outs, pool, None, c.cfg())
    # a taken offer nobody received
    outs = copies(good)
    outs[1] = dict(outs[1], trace=[], leftover=b"", tree=0, sol=0, iters=0,
                   diag=dict.fromkeys(outs[1]["diag"], 0))
    with pytest.raises(AssertionError, match="no other thread received"):
        orc.check_share(outs, pool, None, c.cfg())
    # the thief is the donor itself
    outs = copies(good)
    outs[0]["trace"] = outs[0]["trace"] + outs[1]["trace"]
    outs[1]["trace"] = []
    with pytest.raises(AssertionError):
        orc.check_share(outs, pool, None, c.cfg())


def test_share_withdrawn_offer_keeps_the_pool(core):
    c, pool, seq, good = share_traces(core, "mixed_nq_f-1")
    # the one-thread model with a withdrawn offer after its first readback at the floor
    one = copy_of(share(core, "mixed_nq_f-1")[5])
    i = next(i for i, r in enumerate(one["trace"])
             if r["kind"] == "batch" and r["ctl"]["size"] >= c.floor_in_force())
    r = one["trace"][i]
    size = r["ctl"]["size"]
    moved = r["pool"][(size - size // 2) * NODE:]
    one["trace"].insert(i + 1, dict(kind="donate", size_before=size, size_after=size, moved=moved,
                                    best=r["ctl"]["best"], taken=False, withdrawn=True))
    idle = dict(good[1], trace=[], leftover=b"", tree=0, sol=0, iters=0,
                diag=dict.fromkeys(good[1]["diag"], 0))
    orc.check_share([one, idle], pool, seq, c.cfg())
    assert orc.share_counts([one, idle])["withdrawn"] == 1
    # withdrawn, yet the size shrank
    bad = copy_of(one)
    bad["trace"][i + 1]["size_after"] = size - size // 2
    with pytest.raises(AssertionError):
        orc.check_share([bad, idle], pool, None, c.cfg())


def test_share_global_conservation_bites(core):
    c, pool, seq, good = share_traces(core, "mixed_nq_f-1")
    outs = copies(good)
    outs[1]["tree"] += 1
    with pytest.raises(AssertionError):
        orc.check_share(outs, pool, seq, c.cfg())


@pytest.mark.parametrize("kwargs", [
    dict(threads=1), dict(threads=5), dict(threads=0), dict(threads=-2),
    dict(donate_floor=1), dict(donate_floor=-1), dict(donate_floor=-64),
    dict(await_idle_ms=-1), dict(await_idle_ms=5001),
    dict(nodes=b""), dict(nodes=NQ_OK[:23]), dict(N=3),
    dict(nodes=step.nq_node(2, [1, 1, 0, 2, 4, 5])),
    dict(m=0), dict(chunk=0), dict(chunk=65, capacity=64),
    dict(capacity=(1 << 22) + 1),                      # the per-thread trace bound
    dict(max_batches=-1), dict(max_batches=4097), dict(finish=9),
])
def test_nq_share_rejects_malformed_input(core, kwargs):
    args = dict(nodes=NQ_OK, N=6, chunk=8, capacity=64, max_batches=2, threads=2,
                donate_floor=2, await_idle_ms=10)
    args.update(kwargs)
    with pytest.raises(ValueError):
        core.nq_devpool_share(**args)


@pytest.mark.parametrize("kwargs", [
    dict(threads=1), dict(threads=5),
    dict(donate_floor=1), dict(donate_floor=-1),
    dict(await_idle_ms=-1), dict(await_idle_ms=5001),
    dict(nodes=b""), dict(nodes=PF_OK + b"\0"),
    dict(nodes=_pf(3, [0] + list(range(19)))),
    dict(m=0), dict(chunk=0), dict(chunk=65, capacity=64),
    dict(capacity=(1 << 22) + 1),
    dict(max_batches=4097), dict(best=0), dict(lb="bogus"), dict(br="sideways"),
    dict(lb="lb2", br="bwd"), dict(inst=31),
])
def test_pfsp_share_rejects_malformed_input(core, kwargs):
    args = dict(nodes=PF_OK, inst=2, lb="lb1", best=1359, chunk=8, capacity=64, max_batches=2,
                threads=2, donate_floor=2, await_idle_ms=10)
    args.update(kwargs)
    with pytest.raises(ValueError):
        core.pfsp_devpool_share(**args)
