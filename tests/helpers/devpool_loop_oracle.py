"""CPU side of the loop-driver tests (tests/test_gpu_devpool_loop.py).

nq_devpool_loop / pfsp_devpool_loop run ONE slice through the real slice
thread (run_pool, the loop driver, the capacity spill, drain_spilled, the
leftover copy) and return the driver's trace: a list of dicts, "kind" being

  run    from_spill, init_size, leftover          one per run_pool call
  batch  b, parity, graph, captured, size_before, ctl, pool   one per readback
  spill  size_before, size_after, moved           one per spill

Child order inside the pool is not part of the kernels' contract, so no
trajectory is predicted. What is checked instead:

  * check_trace: the driver's decision rules, as properties of the trace (the
    batch length is a function of the pool size at the last readback, the
    parity of the eager iterations so far, when a graph may be replayed, when a
    spill may happen and what it moves, how runs follow each other, and the
    diag counters as sums over the trace);
  * check_conservation: at every readback, counted + still to do == the input
    pool's total, "still to do" being a CPU search of the snapshot, of the
    spilled stack and of the leftovers so far. A readback of the wrong control
    block, a pool/control mismatch, a lost or duplicated node or half-pool
    breaks it at the batch where it happens;
  * check_final: device totals + a CPU finish of the leftovers == the total.

loop_model applies the same decision rules to the step oracle iterated in
oracle order. It predicts nothing about a GPU run; it is used to choose inputs
whose path conditions (graph replays, spills, ...) hold with slack, and to
prove on the CPU that the checkers accept a correct trace and bite on a
corrupted one (tests/test_devpool_loop_oracle.py).
"""
NODE = 24
BATCH = 16          # iterations per full batch
EAGER_BATCHES = 4   # batches before a graph may be captured
SMALL_POOL = 4096   # below it batches are 2 iterations long
BLOCK = 64          # nodes per cached block of SeqCache


class Cfg:
    def __init__(self, m, chunk, per, capacity, graph=True, max_batches=0):
        self.m, self.chunk, self.per, self.capacity = m, chunk, per, capacity
        self.graph, self.max_batches = graph, max_batches
        self.growth = chunk * per  # worst-case children per iteration


def batch_len(cfg, size, batches):
    """The driver's batch length at pool size `size` after `batches` batches
    of this run, or "spill"."""
    b = BATCH
    if cfg.per > 1 and size < SMALL_POOL:
        b = 2
    room = max(cfg.capacity - size, 0)
    bmax = room // cfg.growth
    if bmax == 0 and size >= 4 * cfg.m and batches > 0:
        return "spill"
    if bmax == 0:
        return 1
    return min(b, bmax)


def runs_of(trace):
    """[(run record, [batch and spill records])]"""
    out = []
    for rec in trace:
        if rec["kind"] == "run":
            out.append((rec, []))
        else:
            assert out, "the trace must start with a run record"
            out[-1][1].append(rec)
    return out


def batches_of(trace):
    return [r for r in trace if r["kind"] == "batch"]


def spills_of(trace):
    return [r for r in trace if r["kind"] == "spill"]


def counts(trace):
    """Path counters of a trace, for path assertions and the summary."""
    bs = batches_of(trace)
    spills_in_drained = drained_leftovers = 0
    for run, recs in runs_of(trace):
        if run["from_spill"]:
            spills_in_drained += sum(r["kind"] == "spill" for r in recs)
            drained_leftovers += run["leftover"] > 0
    first_spill = next((i for i, r in enumerate(trace) if r["kind"] == "spill"), len(trace))
    return dict(batches=len(bs), replays=sum(r["graph"] for r in bs),
                captures=sum(r["captured"] for r in bs),
                parity1=sum(r["parity"] == 1 for r in bs),
                odd_b=sum(r["b"] % 2 for r in bs),
                short=sum(r["b"] == 2 and r["size_before"] < SMALL_POOL for r in bs),
                spills=len(spills_of(trace)), runs=len(runs_of(trace)),
                spills_in_drained=spills_in_drained, drained_leftovers=drained_leftovers,
                replays_before_first_spill=sum(r["kind"] == "batch" and r["graph"]
                                               for r in trace[:first_spill]))


def check_trace(out, cfg, n0):
    """The decision rules. `out` is an entry point's (or the model's) result,
    n0 the input pool's node count."""
    trace = out["trace"]
    runs = runs_of(trace)
    assert runs and not runs[0][0]["from_spill"] and runs[0][0]["init_size"] == n0, runs[0][0]
    stack = 0       # nodes on the spilled stack
    sum_b = leftover_copies = leftover_nodes = iters = 0
    for ri, (run, recs) in enumerate(runs):
        w = ("run", ri)
        if ri > 0:  # drain_spilled: the top min(stack, capacity / 2) nodes
            assert run["from_spill"], w
            assert stack > 0 and run["init_size"] == min(stack, cfg.capacity // 2), (w, run, stack)
            stack -= run["init_size"]
        size, batches, par, have_graph = run["init_size"], 0, 0, False
        prev_iters = 0
        ended = False
        assert recs and recs[-1]["kind"] == "batch", (w, "a run ends with a batch")
        for rec in recs:
            w = ("run", ri, "batch", batches, {k: v for k, v in rec.items()
                                               if k not in ("pool", "moved")})
            assert not ended, (w, "record after the loop's exit condition held")
            assert rec["size_before"] == size, (w, size)
            want = batch_len(cfg, size, batches)
            if rec["kind"] == "spill":
                # only under capacity pressure, only a pool worth halving, never first
                assert cfg.capacity - size < cfg.growth, w
                assert size >= 4 * cfg.m and batches > 0, w
                assert want == "spill", w
                half = size // 2
                assert rec["size_after"] == size - half, w
                assert len(rec["moved"]) == half * NODE, (w, len(rec["moved"]))
                stack += half
                size = rec["size_after"]
                continue
            b = rec["b"]
            assert b >= 1, w
            assert b == 1 or b * cfg.growth <= cfg.capacity - size, (w, "batch larger than the room")
            assert b <= 2 or not (size < SMALL_POOL and cfg.per > 1), (w, "long batch, small pool")
            assert want != "spill", (w, "a spill was due")
            assert b == want, (w, want)
            assert rec["parity"] == par, (w, "entry parity", par)
            if rec["graph"]:
                assert cfg.graph and b == BATCH and par == 0 and batches >= EAGER_BATCHES, w
                assert rec["captured"] == (not have_graph), w
                have_graph = True
            else:
                assert not rec["captured"], w
                # an instantiated graph is replayed whenever the batch fits it
                assert not (have_graph and b == BATCH and par == 0), (w, "eager, graph ready")
                par ^= b & 1
            ctl = rec["ctl"]
            assert ctl["overflow"] == 0, w
            assert ctl["size"] * NODE == len(rec["pool"]), (w, len(rec["pool"]))
            assert ctl["size"] <= min(cfg.capacity, size + b * cfg.growth), w
            # productive iterations: at most b more than at the previous readback
            assert prev_iters <= ctl["iters"] <= prev_iters + b, (w, prev_iters)
            prev_iters = ctl["iters"]
            batches += 1
            sum_b += b
            size = ctl["size"]
            ended = size < cfg.m or (cfg.max_batches > 0 and batches >= cfg.max_batches)
        assert ended, (("run", ri), "the loop left early", size, batches)
        assert run["leftover"] == size, (("run", ri), run, size)
        leftover_copies += size > 0
        leftover_nodes += size
        iters += recs[-1]["ctl"]["iters"]
    assert stack == 0, ("spilled nodes never re-run", stack)
    assert len(out["leftover"]) == leftover_nodes * NODE
    assert out["iters"] == iters, (out["iters"], iters)
    d = out["diag"]
    assert d["kernel_launch"] == 2 * sum_b, (d, sum_b)
    assert d["device_to_host"] == len(batches_of(trace)) + len(spills_of(trace)) + \
        leftover_copies, (d, leftover_copies)
    assert d["host_to_device"] == 3 * len(runs), d  # the pool and two control blocks
    assert d["gpu_iters"] == iters, d


class SeqCache:
    """tree / sol of a CPU search of a pool, summed over 64-node blocks that are
    cached by content: successive snapshots share their un-popped prefix."""

    def __init__(self, seq_fn):
        self.seq_fn, self.cache = seq_fn, {}

    def __call__(self, pool):
        tree = sol = 0
        for i in range(0, len(pool), BLOCK * NODE):
            blk = pool[i:i + BLOCK * NODE]
            if blk not in self.cache:
                self.cache[blk] = self.seq_fn(blk)
            t, s = self.cache[blk]
            tree, sol = tree + t, sol + s
        return tree, sol


def nq_seq_fn(core, N, g=1):
    def f(pool):
        r = core.nqueens_seq_from_pool(pool, N, g)
        return r["tree"], r["sol"]
    return f


def pfsp_seq_fn(core, inst, lb, best, br="fwd"):
    """With the incumbent fixed at `best` == the optimum no leaf lowers it, so
    the count below a node does not depend on the order of the search."""
    def f(pool):
        r = core.pfsp_seq_from_pool(pool, inst, lb, 1, best, br)
        assert r["optimum"] == best
        return r["tree"], r["sol"]
    return f


def check_conservation(out, pool0, seq, cfg, from_batch=0, total=None):
    """At every readback (from global batch index `from_batch` on; `total` is
    then taken at that batch): counted + CPU search of what is left == total.
    Also the spill check (the moved nodes are the back floor(size / 2) nodes of
    the previous snapshot, the kept prefix is what the next batch starts from)
    and, between consecutive snapshots, the un-popped prefix byte for byte: a
    node whose subtree is empty is invisible to the counts, not to this.
    Returns the total (tree, sol)."""
    if total is None and from_batch == 0:
        total = seq(pool0)
    stack = b""                 # spilled nodes not yet re-run
    done_t = done_s = 0         # finished runs' counters
    left = b""                  # finished runs' leftovers
    k = 0
    for ri, (run, recs) in enumerate(runs_of(out["trace"])):
        snap = pool0
        if ri > 0:  # the drained chunk: the top of the stack
            take = run["init_size"] * NODE
            assert 0 < take <= len(stack), (ri, take, len(stack))
            stack, snap = stack[:len(stack) - take], stack[len(stack) - take:]
        rest = None  # tree / sol of the stack and the leftovers, until they change
        for rec in recs:
            if rec["kind"] == "spill":
                rest = None
                keep = rec["size_after"] * NODE
                assert len(snap) == rec["size_before"] * NODE, (ri, k, "stale snapshot")
                assert rec["moved"] == snap[keep:], (ri, k, "the spill did not move the back half")
                snap = snap[:keep]  # the kept prefix; the next readback's conservation holds
                stack += rec["moved"]  # only if the device kept exactly this
                continue
            # b iterations pop at most b * chunk nodes below the old top
            # (children are pushed above whatever is left): the rest of the
            # previous pool is still there, byte for byte
            keep = max(len(snap) - rec["b"] * cfg.chunk * NODE, 0)
            assert rec["pool"][:keep] == snap[:keep], (ri, k, "un-popped prefix changed", keep // NODE)
            snap, ctl = rec["pool"], rec["ctl"]
            if k >= from_batch:
                pt, ps = seq(snap)
                if rest is None:
                    (st, ss), (lt, ls) = seq(stack), seq(left)
                    rest = (st + lt, ss + ls)
                got = (done_t + ctl["tree"] + pt + rest[0], done_s + ctl["sol"] + ps + rest[1])
                if total is None:
                    total = got
                assert got == total, ("conservation", "run", ri, "batch", k, got, total,
                                      dict(ctl), len(snap) // NODE, len(stack) // NODE)
            k += 1
        done_t += recs[-1]["ctl"]["tree"]
        done_s += recs[-1]["ctl"]["sol"]
        left += snap
    assert left == out["leftover"], "the leftovers are not the runs' final pools"
    assert (done_t, done_s) == (out["tree"], out["sol"]), (done_t, done_s, out["tree"], out["sol"])
    return total


def check_final(out, seq, total):
    """Device totals + a CPU finish of the leftovers == the total."""
    lt, ls = seq(out["leftover"])
    assert (out["tree"] + lt, out["sol"] + ls) == tuple(total), (out["tree"], lt, out["sol"], ls,
                                                                 total)


def check_all(out, pool0, seq, cfg, total=None):
    check_trace(out, cfg, len(pool0) // NODE)
    t = check_conservation(out, pool0, seq, cfg)
    if total is not None:
        assert t == tuple(total), (t, total)
    check_final(out, seq, t)
    return counts(out["trace"])


# ---------------------------------------------------------------------------
# the model: the decision rules over the step oracle in oracle order
# ---------------------------------------------------------------------------

def loop_model(step_fn, pool0, cfg, best=0, lower_best_at=None):
    """step_fn(pool, M, tree, sol, iters, best) -> Step (prefix, children,
    ctl) with the pop threshold m built in. Returns what the entry points
    return. Raises RuntimeError where the driver reports a pool overflow."""
    trace, leftover = [], b""
    shared = [best]
    tot = dict(tree=0, sol=0, iters=0, kernel_launch=0, d2h=0, h2d=0, k=0, best=best)
    stack = b""

    def run_pool(pool, init_best, from_spill):
        nonlocal stack, leftover
        run = dict(kind="run", from_spill=from_spill, init_size=len(pool) // NODE, leftover=0)
        trace.append(run)
        tot["h2d"] += 3
        ctl = dict(size=len(pool) // NODE, chunk=0, tree=0, sol=0, iters=0,
                   best=min(init_best, shared[0]), overflow=0)
        batches, par, have_graph = 0, 0, False
        while True:
            size = ctl["size"]
            b = batch_len(cfg, size, batches)
            if b == "spill":
                keep = size - size // 2
                moved = pool[keep * NODE:]
                pool = pool[:keep * NODE]
                stack += moved
                ctl["size"] = keep
                tot["d2h"] += 1
                trace.append(dict(kind="spill", size_before=size, size_after=keep, moved=moved))
                continue
            captured = False
            graph = cfg.graph and batches >= EAGER_BATCHES and b == BATCH and par == 0
            if graph and not have_graph:
                captured = have_graph = True
            rec = dict(kind="batch", b=b, parity=par, graph=graph, captured=captured,
                       size_before=size)
            for _ in range(b):
                s = step_fn(pool, cfg.chunk, ctl["tree"], ctl["sol"], ctl["iters"], ctl["best"])
                if s.ctl["size"] > cfg.capacity:
                    raise RuntimeError("device pool overflow")
                pool, ctl = s.prefix + b"".join(s.children), dict(s.ctl)
            if not graph:
                par ^= b & 1
            batches += 1
            tot["kernel_launch"] += 2 * b
            tot["d2h"] += 1
            rec.update(ctl=dict(ctl), pool=pool)
            trace.append(rec)
            if lower_best_at is not None and tot["k"] == lower_best_at[0]:
                shared[0] = min(shared[0], lower_best_at[1])
            tot["k"] += 1
            shared[0] = min(shared[0], ctl["best"])
            ctl["best"] = shared[0]  # adoption: written to the live block
            if ctl["size"] < cfg.m or (cfg.max_batches > 0 and batches >= cfg.max_batches):
                break
        for f in ("tree", "sol", "iters"):
            tot[f] += ctl[f]
        tot["best"] = min(tot["best"], ctl["best"])
        run["leftover"] = ctl["size"]
        if pool:
            tot["d2h"] += 1
            leftover += pool

    run_pool(pool0, best, False)
    while stack:
        take = min(len(stack) // NODE, cfg.capacity // 2) * NODE
        chunk, stack = stack[len(stack) - take:], stack[:len(stack) - take]
        run_pool(chunk, tot["best"], True)
    return dict(tree=tot["tree"], sol=tot["sol"], best=min(tot["best"], shared[0]),
                iters=tot["iters"], leftover=leftover, trace=trace,
                diag=dict(kernel_launch=tot["kernel_launch"], device_to_host=tot["d2h"],
                          host_to_device=tot["h2d"], gpu_iters=tot["iters"]))


# ---------------------------------------------------------------------------
# the inputs of tests/test_gpu_devpool_loop.py, shared with the CPU tests that
# prove (on the model) that each one reaches its path with slack
# ---------------------------------------------------------------------------

class Case:
    """problem "nq" (N, finish) or "pfsp" (inst, lb, br); pool: ("bfs", target
    [, lo, hi [, reps]]) = the CPU breadth-first frontier, optionally a slice of
    it, optionally repeated (the kernels are pure functions of a node, so a
    multiset pool is a legitimate pool); need: path counters the GPU trace must
    reach at least — the model must reach twice as much."""

    def __init__(self, problem, pool, m=25, chunk=256, capacity=1 << 16, graph=True,
                 max_batches=0, need=None, N=0, finish=8, inst=0, lb="lb1", br="fwd",
                 best_delta=0, lower_at=None, whole_tree=None):
        self.problem, self.pool, self.m, self.chunk = problem, pool, m, chunk
        self.capacity, self.graph, self.max_batches = capacity, graph, max_batches
        self.need = need or {}
        self.N, self.finish, self.inst, self.lb, self.br = N, finish, inst, lb, br
        self.best_delta, self.lower_at, self.whole_tree = best_delta, lower_at, whole_tree

    def cfg(self, graph=None):
        per = self.N if self.problem == "nq" else 20
        return Cfg(self.m, self.chunk, per, self.capacity,
                   self.graph if graph is None else graph, self.max_batches)


CASES = {
    # a. eager growth from a few nodes: b = 2 while the pool is below 4096
    "grow_nq": Case("nq", ("bfs", 25), N=10, finish=2, chunk=4096, capacity=1 << 17,
                    need=dict(short=1), whole_tree=(35538, 724)),
    "grow_lb1": Case("pfsp", ("bfs", 4096, 1000, 1040), inst=14, lb="lb1", chunk=1024,
                     capacity=1 << 16, need=dict(short=1)),
    # b. graph replay, then eager again once the pool is below 4096
    "graph_nq": Case("nq", ("bfs", 6000), N=12, finish=4, chunk=128, max_batches=24,
                     need=dict(replays=3, eager_after_graph=1)),
    # f. the same through lb12 / minbranch (nodes with jobs fixed at both ends)
    "graph_lb12": Case("pfsp", ("bfs", 400, 0, None, 12), inst=14, lb="lb12", br="minbranch",
                       chunk=128, capacity=1 << 17, max_batches=24,
                       need=dict(replays=3, eager_after_graph=1)),
    # c. room for 15 iterations at first: odd batches flip the live control
    # block, and a full batch entered on block 1 must not be replayed from a graph
    "parity_nq": Case("nq", ("bfs", 6000), N=12, finish=4, chunk=128,
                      capacity=6002 + 15 * 128 * 12 + 300, max_batches=24,
                      need=dict(parity1=1, full_on_parity1=1)),
    # d. spills, also inside runs started from a drained chunk
    # A depth-first pool exceeds its un-popped base by about one worst-case
    # iteration, and by how much depends on the child order, so a pool that has
    # to GROW into a spill reaches it on the model and not on the GPU (tried).
    # These start 100 nodes below a capacity of 900 with 640 worst-case
    # children per iteration, which makes the spills arithmetic: the first turn
    # runs one iteration (room < 640), then at least 736 nodes > 900 - 640 are
    # halved twice; the stack then holds more than 450 = capacity / 2 nodes, so
    # the first drained run starts with 450, runs one iteration and, with at
    # least 386 > 260 nodes left, spills again, whatever the nodes are.
    "spill_nq": Case("nq", ("bfs", 4096, 0, 800), N=10, finish=-1, chunk=64, capacity=900,
                     need=dict(spills=3, spills_in_drained=1, drained_leftovers=1, parity1=1)),
    "spill_lb1": Case("pfsp", ("bfs", 30000, 20000, 20800), inst=14, lb="lb1", chunk=32,
                      capacity=900,
                      need=dict(spills=3, spills_in_drained=1, drained_leftovers=1, parity1=1)),
    # d'. a spill FIRST (room for exactly one iteration, whose real children
    # then leave less), then graph replays in the halved pool and in the drained
    # run, which needs the spill to have happened
    "spill_then_graph_nq": Case("nq", ("bfs", 9500), N=12, finish=3, chunk=16,
                                capacity=9502 + 16 * 12, max_batches=12,
                                need=dict(replays=3, replays_in_drained=1)),
    # e. the incumbent lowered from outside at batch 3
    "adopt_lb1_d": Case("pfsp", ("bfs", 4096, 1040, 1100), inst=14, lb="lb1_d", chunk=32,
                        capacity=1 << 12, best_delta=60, lower_at=3, need=dict(short=5)),
}


def case_pool(core, c):
    """(pool bytes, tree, sol counted by the breadth-first phase)."""
    target = c.pool[1]
    if c.problem == "nq":
        nodes, tree, sol = core.nq_bfs_frontier(c.N, 1, target)
    else:
        nodes, tree, sol, _ = core.pfsp_bfs_frontier(c.inst, c.lb, 1, target, c.br)
    if len(c.pool) > 2:
        lo, hi = c.pool[2], c.pool[3]
        nodes = nodes[lo * NODE:(len(nodes) if hi is None else hi * NODE)]
    if len(c.pool) > 4:
        nodes = nodes * c.pool[4]
    return nodes, tree, sol


def case_best(core, c):
    return core.taillard_best_ub(c.inst) if c.problem == "pfsp" else 0


def case_seq(core, c):
    if c.problem == "nq":
        return SeqCache(nq_seq_fn(core, c.N))
    return SeqCache(pfsp_seq_fn(core, c.inst, c.lb, case_best(core, c), c.br))


class _Jobs20:
    jobs = 20


def case_step_fn(core, c):
    """The model's step function for a case (the pop threshold m built in)."""
    import bi_oracle as bo
    import devpool_step_oracle as orc
    if c.problem == "nq":
        return lambda pool, M, tree, sol, iters, best: orc.nq_step(
            core, pool, c.N, 1, c.finish, c.m, M, tree, sol, iters)
    if c.lb != "lb12":
        assert c.br == "fwd"
        return lambda pool, M, tree, sol, iters, best: orc.pfsp_step(
            core, pool, c.inst, c.lb, best, c.m, M, tree, sol, iters)

    def lb12_step(pool, M, tree, sol, iters, best):
        # the C++ host rule's (dir, bounds) arrays (pinned to the Python lb12
        # oracle by tests/test_pfsp_lb12.py) over the popped chunk only
        size = len(pool) // NODE
        n, base = orc.pop_rule(size, c.m, M)
        parents = pool[base * NODE:]
        pushed, best_out = [], best
        if n:
            dirs, vals = core.pfsp_cpu_bounds_lb12(c.inst, parents, best, c.br)
            for i in range(n):
                node = parents[i * NODE:(i + 1) * NODE]
                for k in range(20):
                    v = vals[i * 20 + k]
                    if v < 0:
                        continue
                    if node[0] + 1 == 20:
                        sol += 1
                        best_out = min(best_out, v)
                    elif v < best:
                        pushed.append(bo.child_of(_Jobs20, node, k, bool(dirs[i])))
        ctl = dict(size=base + len(pushed), chunk=n, tree=tree + len(pushed), sol=sol,
                   iters=iters + (1 if n else 0), best=best_out, overflow=0)
        return orc.Step(pool[:base * NODE], pushed, ctl, NODE)
    return lb12_step


def case_model(core, c, graph=None):
    pool, _, _ = case_pool(core, c)
    best = case_best(core, c)
    lower = None if c.lower_at is None else (c.lower_at, best)
    return loop_model(case_step_fn(core, c), pool, c.cfg(graph), best + c.best_delta, lower)


def case_counts(out):
    """counts() plus the path counters only some cases need."""
    n = counts(out["trace"])
    bs = batches_of(out["trace"])
    last_g = max((i for i, r in enumerate(bs) if r["graph"]), default=None)
    n["eager_after_graph"] = 0 if last_g is None else len(bs) - 1 - last_g
    n["full_on_parity1"] = 0
    n["replays_in_drained"] = 0
    for run, recs in runs_of(out["trace"]):
        k = 0
        for r in recs:
            if r["kind"] != "batch":
                continue
            n["full_on_parity1"] += r["b"] == BATCH and r["parity"] == 1 and k >= EAGER_BATCHES
            n["replays_in_drained"] += r["graph"] and run["from_spill"]
            k += 1
    return n


def check_need(n, need, factor=1):
    for k, v in need.items():
        assert n[k] >= factor * v, ("path not reached", k, n[k], "need", factor * v, n)
