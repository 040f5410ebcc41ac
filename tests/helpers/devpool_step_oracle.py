"""CPU oracle for ONE devpool iteration (expand -> presum -> gather2).

Plain Python over the CPU bindings only (nq_cpu_labels, pfsp_cpu_bounds,
nqueens_seq_from_pool): nothing here touches HIP code. Given a pool and the
iteration's knobs it predicts every observable of the step:

  * the pop rule: c = 0 if size < m else min(size, M); the parents are the
    last c nodes; base = size - c;
  * pool[0:base] byte-identical to the input;
  * pool[base:] == the pushed children as a MULTISET (emission order within a
    block is thread-major and not part of the contract), compared over the
    node's meaningful bytes (depth + board for N-Queens, depth + limit1 + prmu
    for PFSP);
  * the control block written by gather2's last block: size, chunk, tree,
    sol, iters, best, overflow.

tests/test_devpool_step_oracle.py proves the oracle itself by iterating it
from the root to exhaustion against the frozen sequential counts.
"""
import random
from collections import Counter

NODE = 24
NQ_KEY = 21    # depth + board[20]
PFSP_KEY = 22  # depth + limit1 + prmu[20]

# near-optimal permutations (insertion local search on the CPU bound; makespans
# 1366 / 1398 / 2388 vs optima 1359 / 1377 / 2297): a leaf below optimum + 200
GOOD_PERM = {
    2: [5, 6, 17, 19, 14, 16, 8, 0, 10, 4, 15, 13, 1, 12, 3, 18, 11, 7, 2, 9],
    14: [2, 11, 19, 15, 17, 9, 7, 5, 1, 6, 10, 12, 13, 0, 14, 8, 3, 16, 18, 4],
    21: [15, 9, 7, 0, 6, 14, 16, 8, 4, 5, 19, 10, 11, 12, 3, 17, 1, 13, 2, 18],
}


class Step:
    """Expected outcome of one iteration."""

    def __init__(self, prefix, children, ctl, key):
        self.prefix = prefix      # bytes: the un-popped pool prefix
        self.children = children  # list of 24-byte children pushed this iteration
        self.ctl = ctl            # dict of the expected next control block
        self.key = key            # compared bytes per node

    def pool(self):
        """The next pool in oracle order (for iterating the oracle)."""
        return self.prefix + b"".join(self.children)


def pop_rule(size, m, M):
    c = 0 if size < m else min(size, M)
    return c, size - c


def nq_node(depth, board):
    b = list(board) + list(range(len(board), 20))
    return bytes([depth] + b + [0, 0, 0])


def pfsp_node(depth, prmu):
    return bytes([depth, (depth - 1) & 0xFF] + list(prmu) + [0, 0])


def random_nq_nodes(rng, n, N, min_depth=0, max_depth=None):
    """Seeded random nodes: random permutation of 0..N-1, depth uniform over
    [min_depth, max_depth] (default: the whole legal range 0..N). The kernels
    are pure functions of the node, so unreachable nodes are legitimate."""
    max_depth = N if max_depth is None else max_depth
    out = []
    for _ in range(n):
        board = list(range(N))
        rng.shuffle(board)
        out.append(nq_node(rng.randint(min_depth, max_depth), board))
    return b"".join(out)


def random_pfsp_nodes(rng, n, jobs=20, min_depth=0, max_depth=None):
    max_depth = jobs - 1 if max_depth is None else max_depth
    out = []
    for _ in range(n):
        prmu = list(range(jobs))
        rng.shuffle(prmu)
        out.append(pfsp_node(rng.randint(min_depth, max_depth), prmu))
    return b"".join(out)


def incumbent_pool(inst):
    """300 random nodes of depth <= 18, then a tail of 64 depth-19 parents (63
    random ones and the GOOD_PERM one). With windows [64, 64] the first
    iteration pops leaf parents only and lowers best from optimum + 200 to
    GOOD_PERM's makespan; the second pops 64 inner nodes and must prune with
    the lowered value (no depth-19 parent in it: pruning is deterministic)."""
    r = rng(inst * 1000 + 19)
    return (random_pfsp_nodes(r, 300, max_depth=18) +
            random_pfsp_nodes(r, 63, min_depth=19) + pfsp_node(19, GOOD_PERM[inst]))


def nq_step(core, pool, N, g=1, finish=8, m=1, M=None, tree=0, sol=0, iters=0):
    size = len(pool) // NODE
    M = max(size, 1) if M is None else M
    c, base = pop_rule(size, m, M)
    parents = pool[base * NODE:]
    labels = core.nq_cpu_labels(N, g, parents) if c else b""
    pushed, finished = [], []
    for i in range(c):
        node = parents[i * NODE:(i + 1) * NODE]
        depth = node[0]
        if depth == N:  # leaf parent: counted once, no children
            sol += 1
            continue
        rem = N - depth - 1  # levels below a child
        for k in range(depth, N):
            if labels[i * N + k] != 1:
                continue
            child = bytearray(node)
            child[0] = depth + 1
            child[1 + depth], child[1 + k] = node[1 + k], node[1 + depth]
            (finished if rem <= finish else pushed).append(bytes(child))
    sub_tree = sub_sol = 0
    if finished:
        # subtrees of the children the in-thread finisher swallows: nodes
        # BELOW them (tree) and solutions, incl. rem == 0 children themselves
        r = core.nqueens_seq_from_pool(b"".join(finished), N, g)
        sub_tree, sub_sol = r["tree"], r["sol"]
    ctl = dict(size=base + len(pushed), chunk=c,
               tree=tree + len(pushed) + len(finished) + sub_tree,
               sol=sol + sub_sol, iters=iters + (1 if c > 0 else 0), best=0, overflow=0)
    return Step(pool[:base * NODE], pushed, ctl, NQ_KEY)


def pfsp_step(core, pool, inst, lb, best, m=1, M=None, tree=0, sol=0, iters=0):
    jobs = core.taillard_nb_jobs(inst)
    size = len(pool) // NODE
    M = max(size, 1) if M is None else M
    c, base = pop_rule(size, m, M)
    parents = pool[base * NODE:]
    bounds = core.pfsp_cpu_bounds(inst, lb, parents, best) if c else []
    pushed = []
    best_out = best
    for i in range(c):
        node = parents[i * NODE:(i + 1) * NODE]
        depth = node[0]
        limit1 = int.from_bytes(node[1:2], "little", signed=True)
        for k in range(limit1 + 1, jobs):
            b = bounds[i * jobs + k]
            if depth + 1 == jobs:  # leaf child: a solution, never pushed/counted in tree
                sol += 1
                best_out = min(best_out, b)
            elif b < best:  # snapshot incumbent, not the running minimum
                child = bytearray(node)
                child[0] = depth + 1
                child[1] = (limit1 + 1) & 0xFF
                child[2 + depth], child[2 + k] = node[2 + k], node[2 + depth]
                pushed.append(bytes(child))
                tree += 1
    ctl = dict(size=base + len(pushed), chunk=c, tree=tree, sol=sol,
               iters=iters + (1 if c > 0 else 0), best=best_out, overflow=0)
    return Step(pool[:base * NODE], pushed, ctl, PFSP_KEY)


def _keys(buf, key):
    return Counter(buf[i:i + key] for i in range(0, len(buf), NODE))


def check_step(exp, pool_out, ctl, what=""):
    """Exact comparison of a step result (pool bytes + ctl dict) with `exp`."""
    for f in ("chunk", "iters", "overflow", "size", "sol", "tree", "best"):
        assert ctl[f] == exp.ctl[f], (what, f, ctl[f], exp.ctl[f], ctl, exp.ctl)
    assert len(pool_out) == exp.ctl["size"] * NODE, (what, len(pool_out))
    nb = len(exp.prefix)
    if pool_out[:nb] != exp.prefix:
        bad = next(i for i in range(0, nb, NODE)
                   if pool_out[i:i + NODE] != exp.prefix[i:i + NODE]) // NODE
        raise AssertionError((what, "un-popped prefix changed at node", bad))
    got = _keys(pool_out[nb:], exp.key)
    want = Counter(ch[:exp.key] for ch in exp.children)
    if got != want:
        missing = list((want - got).elements())[:3]
        extra = list((got - want).elements())[:3]
        raise AssertionError((what, "children differ", "missing", [list(x) for x in missing],
                              "unexpected", [list(x) for x in extra]))


def check_overflow(exp, pool_in, pool_out, ctl, what=""):
    """Overflow contract: sticky flag set, un-popped prefix untouched. Nothing
    is claimed about the popped tail or the counters."""
    assert ctl["overflow"] == 1, (what, ctl)
    nb = len(exp.prefix)
    assert pool_out[:nb] == pool_in[:nb], (what, "un-popped prefix changed")


def loop_windows(n, per, Mc, k):
    """The loop driver's launch windows for k blind iterations after a
    readback at pool size n: bound_i = n * per^i (branching `per`), clamped to
    the chunk cap Mc and to at least one node."""
    assert k >= 1 and per >= 1 and Mc >= 1
    out, bound = [], max(n, 1)
    for _ in range(k):
        out.append(min(bound, Mc))
        bound = min(bound * per, Mc)
    return out


def oracle_chain(pool0, windows, step_fn, best=0, capacity=None):
    """The oracle iterated on its own output: the snapshots a correct chain
    would return (children in oracle order). An iteration whose next size
    exceeds `capacity` sets the sticky flag: from then on the snapshot is the
    un-popped prefix and the counters stop."""
    pool, ctl = pool0, dict(size=len(pool0) // NODE, chunk=0, tree=0, sol=0, iters=0,
                            best=best, overflow=0)
    out = []
    for M in windows:
        if not ctl["overflow"]:
            exp = step_fn(pool, M, ctl["tree"], ctl["sol"], ctl["iters"], ctl["best"])
            if capacity is not None and exp.ctl["size"] > capacity:
                pool, ctl = exp.prefix, dict(ctl, overflow=1)
            else:
                pool, ctl = exp.pool(), dict(exp.ctl)
        out.append((pool, dict(ctl)))
    return out


def check_chain(core, pool0, snapshots, windows, step_fn, best=0, capacity=None, what=""):
    """Compare a chain of snapshots [(pool bytes, ctl dict), ...] with the oracle,
    one transition at a time. The input of transition i is the previous GPU
    snapshot (pool0 with zero counters and `best` for i = 0), so every
    transition is compared directly with the CPU oracle: child order inside
    the pool is not part of the contract, and only the snapshot says which
    nodes sit in the popped tail. step_fn(pool, M, tree, sol, iters, best)
    returns the expected Step. With `capacity` given, the overflow flag must
    be set exactly when the oracle's next size exceeds it; once set it must
    stay set and the un-popped prefix must never change again. Returns the
    list of expected Steps (None for transitions after the overflow). `core`
    is the bindings module the snapshots came from; the oracle itself reaches
    the CPU bindings through step_fn."""
    assert len(snapshots) == len(windows), (what, len(snapshots), len(windows))
    pool, ctl = pool0, dict(tree=0, sol=0, iters=0, best=best, overflow=0)
    exps = []
    for i, ((pool_out, ctl_out), M) in enumerate(zip(snapshots, windows)):
        w = (what, "iteration", i, "window", M)
        if ctl["overflow"]:
            # sticky: nothing is popped or pushed any more
            check_overflow(Step(pool, [], None, None), pool, pool_out, ctl_out, w)
            assert len(pool_out) == len(pool), (w, "prefix length changed", len(pool_out))
            exps.append(None)
        else:
            exp = step_fn(pool, M, ctl["tree"], ctl["sol"], ctl["iters"], ctl["best"])
            over = ctl_out["overflow"] != 0
            if capacity is not None:
                assert over == (exp.ctl["size"] > capacity), (w, "overflow flag", ctl_out,
                                                              exp.ctl, capacity)
            if over:
                check_overflow(exp, pool, pool_out, ctl_out, w)
                assert len(pool_out) == len(exp.prefix), (w, "prefix length", len(pool_out))
            else:
                check_step(exp, pool_out, ctl_out, w)
            exps.append(exp)
        pool, ctl = pool_out, ctl_out
    return exps


def rng(seed):
    return random.Random(seed)
