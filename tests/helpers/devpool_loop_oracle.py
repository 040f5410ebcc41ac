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
    def __init__(self, m, chunk, per, capacity, graph=True, max_batches=0, floor=None):
        self.m, self.chunk, self.per, self.capacity = m, chunk, per, capacity
        self.graph, self.max_batches = graph, max_batches
        self.floor = floor  # share runs: the donation floor in force
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


def _trace_job(trace, cfg, n0, floor=None):
    """The decision rules over one job of a slice thread: the run that starts
    from `n0` nodes (the slice, or a donated half) and the runs that drain its
    spills. `floor`: the donation floor where "donate" records may occur.
    Returns the sums the diag counters are made of."""
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
        prev = None
        assert recs and recs[-1]["kind"] in ("batch", "donate"), (w, "a run ends with a batch")

        def ended():
            return size < cfg.m or (cfg.max_batches > 0 and batches >= cfg.max_batches)
        for rec in recs:
            w = ("run", ri, "batch", batches, {k: v for k, v in rec.items()
                                               if k not in ("pool", "moved")})
            assert rec["size_before"] == size, (w, size)
            if rec["kind"] == "donate":
                # the donation check of the readback just before, at most once
                assert floor is not None, (w, "a donation without a share")
                assert prev is not None and prev["kind"] == "batch", (w, "not after a readback")
                assert size >= floor, (w, "a donation below the floor", floor)
                assert rec["taken"] != rec["withdrawn"], (w, "neither taken nor withdrawn")
                half = size // 2
                assert len(rec["moved"]) == half * NODE, (w, len(rec["moved"]))
                assert rec["best"] == prev["ctl"]["best"], (w, "offered incumbent", prev["ctl"])
                assert rec["size_after"] == (size - half if rec["taken"] else size), w
                size = rec["size_after"]
                prev = rec
                continue
            assert not ended(), (w, "record after the loop's exit condition held")
            prev = rec
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
        assert ended(), (("run", ri), "the loop left early", size, batches)
        assert run["leftover"] == size, (("run", ri), run, size)
        leftover_copies += size > 0
        leftover_nodes += size
        iters += prev_iters
    assert stack == 0, ("spilled nodes never re-run", stack)
    return dict(sum_b=sum_b, leftover_copies=leftover_copies, leftover_nodes=leftover_nodes,
                iters=iters, runs=len(runs), batches=len(batches_of(trace)),
                spills=len(spills_of(trace)))


def _check_diag(out, sums, uploads):
    """The thread's totals and diag counters as sums over its jobs."""
    t = {k: sum(s[k] for s in sums) for k in sums[0]} if sums else dict.fromkeys(
        ("sum_b", "leftover_copies", "leftover_nodes", "iters", "runs", "batches", "spills"), 0)
    assert len(out["leftover"]) == t["leftover_nodes"] * NODE
    assert out["iters"] == t["iters"], (out["iters"], t["iters"])
    d = out["diag"]
    assert d["kernel_launch"] == 2 * t["sum_b"], (d, t)
    assert d["device_to_host"] == t["batches"] + t["spills"] + t["leftover_copies"], (d, t)
    assert d["host_to_device"] == uploads, (d, uploads)
    assert d["gpu_iters"] == t["iters"], d


def check_trace(out, cfg, n0):
    """The decision rules. `out` is an entry point's (or the model's) result,
    n0 the input pool's node count."""
    sums = _trace_job(out["trace"], cfg, n0)
    _check_diag(out, [sums], 3 * sums["runs"])  # the pool and two control blocks per run


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


def _conserve_job(trace, pool0, seq, cfg, from_batch=0, total=None):
    """check_conservation over one job (see _trace_job) that starts from
    `pool0`. A taken donation is a spill whose nodes leave the thread: they are
    counted as still to do, and the kept front is what the next batch starts
    from; after a withdrawn one the whole snapshot is. seq None: the byte
    checks alone. Returns (total, (tree, sol) counted, leftovers, donated)."""
    stack = b""                 # spilled nodes not yet re-run
    done_t = done_s = 0         # finished runs' counters
    left = b""                  # finished runs' leftovers
    gone = b""                  # donated nodes
    k = 0
    for ri, (run, recs) in enumerate(runs_of(trace)):
        snap = pool0
        if ri > 0:  # the drained chunk: the top of the stack
            take = run["init_size"] * NODE
            assert 0 < take <= len(stack), (ri, take, len(stack))
            stack, snap = stack[:len(stack) - take], stack[len(stack) - take:]
        rest = None  # tree / sol of the stack and the leftovers, until they change
        last = None
        for rec in recs:
            if rec["kind"] in ("spill", "donate"):
                what = rec["kind"]
                keep = (rec["size_before"] - rec["size_before"] // 2) * NODE
                assert len(snap) == rec["size_before"] * NODE, (ri, k, "stale snapshot")
                assert rec["moved"] == snap[keep:], (ri, k, "the %s did not move the back half" % what)
                if what == "donate" and not rec["taken"]:
                    continue  # withdrawn: the next readback must find all of snap
                rest = None
                snap = snap[:keep]  # the kept prefix; the next readback's conservation holds
                if what == "spill":
                    stack += rec["moved"]  # only if the device kept exactly this
                else:
                    gone += rec["moved"]
                continue
            # b iterations pop at most b * chunk nodes below the old top
            # (children are pushed above whatever is left): the rest of the
            # previous pool is still there, byte for byte
            keep = max(len(snap) - rec["b"] * cfg.chunk * NODE, 0)
            assert rec["pool"][:keep] == snap[:keep], (ri, k, "un-popped prefix changed", keep // NODE)
            snap, ctl = rec["pool"], rec["ctl"]
            last = ctl
            if k >= from_batch and seq is not None:
                pt, ps = seq(snap)
                if rest is None:
                    (st, ss), (lt, ls), (gt, gs) = seq(stack), seq(left), seq(gone)
                    rest = (st + lt + gt, ss + ls + gs)
                got = (done_t + ctl["tree"] + pt + rest[0], done_s + ctl["sol"] + ps + rest[1])
                if total is None:
                    total = got
                assert got == total, ("conservation", "run", ri, "batch", k, got, total,
                                      dict(ctl), len(snap) // NODE, len(stack) // NODE)
            k += 1
        done_t += last["tree"]
        done_s += last["sol"]
        left += snap
    return total, (done_t, done_s), left, gone


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
    total, done, left, _ = _conserve_job(out["trace"], pool0, seq, cfg, from_batch, total)
    assert left == out["leftover"], "the leftovers are not the runs' final pools"
    assert done == (out["tree"], out["sol"]), (done, out["tree"], out["sol"])
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
# several slice threads over one SliceShare (nq_devpool_share /
# pfsp_devpool_share): one result per thread. A thread's trace is a sequence of
# jobs: the slice (thread 0's first run and the runs draining its spills), then
# one job per "take" record. "donate" records follow the readback whose
# donation check made the offer.
# ---------------------------------------------------------------------------

def jobs_of(trace):
    """[(take record or None, [the job's run / batch / spill / donate records])]"""
    jobs = []
    for rec in trace:
        if rec["kind"] == "take":
            jobs.append((rec, []))
        else:
            if not jobs:
                jobs.append((None, []))
            jobs[-1][1].append(rec)
    return jobs


def donations_of(outs, taken=None):
    return [r for o in outs for r in o["trace"]
            if r["kind"] == "donate" and (taken is None or r["taken"] == taken)]


def takes_of(outs):
    return [r for o in outs for r in o["trace"] if r["kind"] == "take"]


def share_counts(outs):
    """Path counters of a share run."""
    chains = 0  # threads that donated from a job they had taken
    for o in outs:
        chains += any(take is not None and any(r["kind"] == "donate" and r["taken"] for r in recs)
                      for take, recs in jobs_of(o["trace"]))
    drained = 0  # taken donations made by a run that drains a spilled chunk
    for o in outs:
        for run, recs in runs_of([r for r in o["trace"] if r["kind"] != "take"]):
            drained += run["from_spill"] and sum(r["kind"] == "donate" and r["taken"] for r in recs)
    return dict(taken=len(donations_of(outs, True)), withdrawn=len(donations_of(outs, False)),
                drained_donations=drained,
                takes=len(takes_of(outs)), chains=chains,
                thieves=sum(any(r["kind"] == "take" for r in o["trace"]) for o in outs),
                spills=sum(len(spills_of(o["trace"])) for o in outs),
                batches=sum(len(batches_of(o["trace"])) for o in outs),
                idle_threads=sum(not o["trace"] for o in outs))


def check_share(outs, pool0, seq, cfg, total=None):
    """Every thread of a share run, whichever thread ran the slice and whichever
    readbacks donated. cfg.floor is the donation floor in force. seq None (an
    incumbent that moves during the run): everything but the counts. Returns
    the total (tree, sol)."""
    assert cfg.floor is not None and not cfg.graph
    owners = [i for i, o in enumerate(outs) if o["trace"] and o["trace"][0]["kind"] == "run"]
    assert len(owners) == 1, ("exactly one thread runs the slice", owners)
    if seq is not None and total is None:
        total = seq(pool0)
    for ti, o in enumerate(outs):
        sums, left, done = [], b"", (0, 0)
        jobs = jobs_of(o["trace"])
        for ji, (take, recs) in enumerate(jobs):
            w = ("thread", ti, "job", ji)
            assert (take is None) == (ti == owners[0] and ji == 0), (w, "a job without a take")
            start = pool0 if take is None else take["nodes"]
            if take is not None:
                assert len(start) == take["size"] * NODE and take["size"] > 0, w
                assert recs and recs[0]["kind"] == "run", (w, "a take is followed by its run")
                # the run adopts the received incumbent, or a lower shared one
                assert recs[0]["best"] <= take["best"], (w, "the thief starts above the offer",
                                                         recs[0]["best"], take["best"])
            try:
                sums.append(_trace_job(recs, cfg, len(start) // NODE, cfg.floor))
                # per-thread conservation: what was taken is this job's pool0,
                # what was donated counts as still to do
                _, d, l, _ = _conserve_job(recs, start, seq, cfg,
                                           total=None if seq is None else seq(start))
            except AssertionError as e:
                raise AssertionError((w,) + e.args) from None
            done = (done[0] + d[0], done[1] + d[1])
            left += l
        if not jobs:
            sums = []
        takes = sum(take is not None for take, _ in jobs)
        # a taken pool arrives by a device-to-device copy, which is not counted
        _check_diag(o, sums, 3 * sum(s["runs"] for s in sums) - takes)
        assert left == o["leftover"], (ti, "the leftovers are not the runs' final pools")
        assert done == (o["tree"], o["sol"]), (ti, done, o["tree"], o["sol"])
    # every taken offer arrives exactly once, in another thread, unchanged
    open_takes = [(ti, r) for ti, o in enumerate(outs) for r in o["trace"] if r["kind"] == "take"]
    for ti, o in enumerate(outs):
        for r in o["trace"]:
            if r["kind"] != "donate" or not r["taken"]:
                continue
            k = next((k for k, (tj, t) in enumerate(open_takes)
                      if tj != ti and t["nodes"] == r["moved"] and t["best"] == r["best"]), None)
            assert k is not None, ("a taken offer that no other thread received", ti,
                                   r["size_before"], r["best"])
            del open_takes[k]
    assert not open_takes, ("a take without a donation", [(ti, t["size"], t["best"])
                                                          for ti, t in open_takes])
    # global conservation at the end
    if seq is not None:
        lt, ls = seq(b"".join(o["leftover"] for o in outs))
        got = (sum(o["tree"] for o in outs) + lt, sum(o["sol"] for o in outs) + ls)
        assert got == tuple(total), ("global conservation", got, total)
    return total


def share_model(step_fn, pool0, cfg, best=0, threads=2):
    """A consistent set of traces, one donation per thread but the last: thread
    t runs what thread t - 1 gave it. Predicts nothing about a GPU run; it is
    what check_share is proved on."""
    outs, pool, b, take = [], pool0, best, None
    for t in range(threads):
        if pool is None:
            outs.append(dict(tree=0, sol=0, best=best, iters=0, leftover=b"", trace=[],
                             diag=dict(kernel_launch=0, device_to_host=0, host_to_device=0,
                                       gpu_iters=0)))
            continue
        o = loop_model(step_fn, pool, cfg, b, donations=1 if t < threads - 1 else 0)
        if take is not None:
            o["trace"].insert(0, take)
            o["diag"]["host_to_device"] -= 1
        outs.append(o)
        pool = None
        if o["given"]:
            pool, b = o["given"][0]
            take = dict(kind="take", size=len(pool) // NODE, best=b, nodes=pool)
    return outs


# ---------------------------------------------------------------------------
# the model: the decision rules over the step oracle in oracle order
# ---------------------------------------------------------------------------

def loop_model(step_fn, pool0, cfg, best=0, lower_best_at=None, donations=0):
    """step_fn(pool, M, tree, sol, iters, best) -> Step (prefix, children,
    ctl) with the pop threshold m built in. Returns what the entry points
    return. Raises RuntimeError where the driver reports a pool overflow.
    donations: at most this many readbacks at or above cfg.floor donate (to a
    thief that is always waiting); the result's "given" lists what left as
    (nodes, incumbent)."""
    trace, leftover, given = [], b"", []
    shared = [best]
    tot = dict(tree=0, sol=0, iters=0, kernel_launch=0, d2h=0, h2d=0, k=0, best=best)
    stack = b""

    def run_pool(pool, init_best, from_spill):
        nonlocal stack, leftover
        run = dict(kind="run", from_spill=from_spill, init_size=len(pool) // NODE, leftover=0,
                   best=min(init_best, shared[0]))
        trace.append(run)
        tot["h2d"] += 3
        ctl = dict(size=len(pool) // NODE, chunk=0, tree=0, sol=0, iters=0,
                   best=run["best"], overflow=0)
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
            if cfg.floor is not None and ctl["size"] >= cfg.floor and len(given) < donations:
                size = ctl["size"]
                keep = size - size // 2
                moved, pool = pool[keep * NODE:], pool[:keep * NODE]
                ctl["size"] = keep
                given.append((moved, ctl["best"]))
                trace.append(dict(kind="donate", size_before=size, size_after=keep, moved=moved,
                                  best=ctl["best"], taken=True, withdrawn=False))
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
                iters=tot["iters"], leftover=leftover, trace=trace, given=given,
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


# ---------------------------------------------------------------------------
# the inputs of tests/test_gpu_devpool_share.py, shared with the CPU tests that
# prove (on the one-thread model) that each pool reaches its floor with slack
# ---------------------------------------------------------------------------

REAL_FLOOR = 1 << 16


def donation_floor(m):
    return max(2 * m, REAL_FLOOR)


class ShareCase(Case):
    """A Case run by `threads` slice threads over one SliceShare. floor: the
    donate_floor argument (0 = the real floor); pools besides Case's "bfs":
    ("root",), ("random", seed, n, min_depth, max_depth) and ("leaves", n) = n
    leaf parents (depth == N: popped, nothing pushed). need: share_counts the
    GPU run must reach; the one-thread model must see at_floor (readbacks with
    the pool at or above the floor) at least twice as often as need says."""

    def __init__(self, problem, pool, threads=2, floor=0, await_ms=2000, fixed_best=True, **kw):
        kw.setdefault("graph", False)
        Case.__init__(self, problem, pool, **kw)
        self.threads, self.floor, self.await_ms, self.fixed_best = threads, floor, await_ms, fixed_best

    def floor_in_force(self):
        return self.floor if self.floor else donation_floor(self.m)

    def cfg(self, graph=None):
        c = Case.cfg(self, False)
        c.floor = self.floor_in_force()
        return c


def _nq_share(pool, finish, **kw):
    kw.setdefault("need", dict(taken=1, at_floor=1))
    return ShareCase("nq", pool, finish=finish, **kw)


SHARE_CASES = {
    # a few hundred random nodes of mixed depth, small floor; finish = 8 takes
    # nodes from depth N - 8 on in one go, so it gets a larger board and
    # shallower nodes to have a pool at all
    "mixed_nq_f-1": _nq_share(("random", 21, 300, 2, 9), -1, N=10, chunk=64, floor=128,
                              capacity=1 << 14),
    "mixed_nq_f3": _nq_share(("random", 21, 300, 2, 9), 3, N=10, chunk=64, floor=128,
                             capacity=1 << 14),
    "mixed_nq_f8": _nq_share(("random", 21, 250, 2, 3), 8, N=12, chunk=32, floor=128,
                             capacity=1 << 14),
    # the root alone: the whole tree against the frozen sequential counts
    "root_nq_f-1": _nq_share(("root",), -1, N=10, m=1, chunk=64, floor=64, capacity=1 << 14,
                             whole_tree=(35538, 724)),
    "root_nq_f3": _nq_share(("root",), 3, N=10, m=1, chunk=64, floor=64, capacity=1 << 14,
                            whole_tree=(35538, 724)),
    "root_nq_f8": _nq_share(("root",), 8, N=12, m=1, chunk=16, floor=64, capacity=1 << 14,
                            whole_tree=(856188, 14200)),
}
SHARE_CASES.update({
    # two thieves served by successive donations, one of which donates itself
    "three_nq": _nq_share(("root",), 3, N=11, m=1, chunk=128, floor=64, capacity=1 << 14, threads=3,
                          need=dict(taken=2, thieves=2, at_floor=2), whole_tree=(166925, 2680)),
    # the real floor at its edge: 65536 nodes at the first readback, by
    # arithmetic (leaf parents lose exactly `chunk` nodes per iteration)
    "edge_nq": _nq_share(("leaves", REAL_FLOOR + BATCH * 64), 8, N=10, chunk=64,
                         capacity=1 << 17, need=dict(taken=1, at_floor=1)),
    "below_edge_nq": _nq_share(("leaves", REAL_FLOOR + BATCH * 64 - 1), 8, N=10, chunk=64,
                               capacity=1 << 17, need={}),
    # the real floor with work in the donated half (depth >= N - 3)
    "deep_nq": _nq_share(("random", 22, 100000, 9, 12), 8, N=12, chunk=256, capacity=1 << 17,
                         need=dict(taken=1, at_floor=1)),
    # m > floor / 2: the 2m branch decides (81920 >= 65536 would donate)
    "two_m_nq": _nq_share(("leaves", 2 * 40000 + BATCH * 64), 8, N=10, m=40000, chunk=64,
                          capacity=1 << 17, need=dict(taken=1, at_floor=1)),
    "below_two_m_nq": _nq_share(("leaves", 2 * 40000 + BATCH * 64 - 1), 8, N=10, m=40000,
                                chunk=64, capacity=1 << 17, need={}),
    # a donation next to spills (spill_nq's capacity; the front half of its
    # pool, then 400 leaf parents). The first readback (one iteration, 64 leaf
    # parents popped: 736 nodes) donates the 368 at the back, leaf parents
    # mostly, so the thief is soon waiting again; the donor keeps 368 > 900 -
    # 640 nodes and spills next, and its drained runs start with 184 or more
    # nodes >= the floor and find the thief waiting: a thread stays a runner
    # between its run_pool calls, or that thief would have left
    "spill_nq": _nq_share(("bfs+leaves", 4096, 0, 400, 400), -1, N=10, chunk=64, capacity=900,
                          floor=64, need=dict(taken=2, spills=2, drained_donations=1, at_floor=1)),
    # lb1_d with the incumbent fixed at the optimum (order-free counts) ...
    "lb1_d": ShareCase("pfsp", ("bfs", 4096, 1040, 1100), inst=14, lb="lb1_d", chunk=32,
                       capacity=1 << 12, floor=64, need=dict(taken=1, at_floor=1)),
    # ... and starting 60 above it: the incumbent moves, the records are checked
    # (frontier node 2987 holds the optimum 1377; the tail of leaf parents
    # lowers the incumbent to 1398 in the first iteration, so the first offer
    # already carries a better value than the run started from)
    "lb1_d_open": ShareCase("pfsp", ("bfs+good", 4096, 2984, 2990), inst=14, lb="lb1_d", m=5,
                            chunk=64, capacity=1 << 13, floor=64, best_delta=60, fixed_best=False,
                            need=dict(taken=1, at_floor=1)),
    # the S = 4 configuration: lb2 on a 20x10 instance, four threads
    "lb2_four": ShareCase("pfsp", ("bfs", 4096, 1000, 1150), inst=14, lb="lb2", chunk=32,
                          capacity=1 << 13, floor=64, threads=4,
                          need=dict(taken=2, thieves=2, at_floor=2)),
    # no donation wanted: the pool stays far below the real floor
    "small_nq": _nq_share(("bfs", 25), 2, N=10, chunk=4096, capacity=1 << 17, need={},
                          whole_tree=(35538, 724)),
    # one batch, then leftovers; the thief finds no runner or nothing to take
    "one_batch_nq": _nq_share(("bfs", 6000), 4, N=12, chunk=128, max_batches=1, need={}),
})


def share_case_pool(core, c):
    """(pool bytes, tree, sol counted before the pool)."""
    import devpool_step_oracle as orc
    kind = c.pool[0]
    if kind == "bfs":
        return case_pool(core, c)
    if kind == "bfs+good":
        pool, t, s = case_pool(core, c)
        return pool + orc.random_pfsp_nodes(orc.rng(c.inst), 63, min_depth=19) + \
            orc.pfsp_node(19, orc.GOOD_PERM[c.inst]), t, s
    if kind == "root":
        return orc.nq_node(0, range(c.N)), 0, 0
    if kind == "bfs+leaves":
        pool, t, s = core.nq_bfs_frontier(c.N, 1, c.pool[1])
        pool = pool[c.pool[2] * NODE:c.pool[3] * NODE]
        return pool + orc.random_nq_nodes(orc.rng(5), c.pool[4], c.N, c.N, c.N), t, s
    if kind == "leaves":
        return orc.random_nq_nodes(orc.rng(c.pool[1]), 64, c.N, c.N, c.N) * (c.pool[1] // 64) + \
            orc.random_nq_nodes(orc.rng(7), c.pool[1] % 64, c.N, c.N, c.N), 0, 0
    _, seed, n, lo, hi = c.pool
    return orc.random_nq_nodes(orc.rng(seed), n, c.N, lo, hi), 0, 0


def share_case_model(core, c):
    """The one-thread model of the case (no donation): where the pool stands at
    each readback."""
    pool, _, _ = share_case_pool(core, c)
    best = case_best(core, c)
    return loop_model(case_step_fn(core, c), pool, c.cfg(), best + c.best_delta)


def at_floor(out, floor):
    return sum(r["ctl"]["size"] >= floor for r in batches_of(out["trace"]))


def run_share_case(core, c, pool):
    if c.problem == "nq":
        return core.nq_devpool_share(pool, c.N, 1, c.finish, c.m, c.chunk, c.capacity,
                                     c.max_batches, c.threads, c.floor, c.await_ms)
    best = case_best(core, c) + c.best_delta
    return core.pfsp_devpool_share(pool, c.inst, c.lb, best, c.m, c.chunk, c.capacity,
                                   c.max_batches, c.br, c.threads, c.floor, c.await_ms)
