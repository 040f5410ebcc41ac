"""Pure-Python oracle for backward / dynamic (MinBranch) PFSP branching.

Written from the rule text (c_bound_simple.c numerics: schedule_front /
schedule_back / sum_unscheduled / add_front_and_bound / add_back_and_bound)
and independent of the C++ and HIP code: only the Taillard matrix is taken
from the bindings. It provides

  * lb1_d child bounds in BOTH directions for one node (incl. the min_heads
    front of a node with nothing fixed at the front and the min_tails back of
    a node with nothing fixed at the back);
  * the direction decision of the rules fwd / bwd / alt / minbranch;
  * a one-step expansion of a pool (the devpool iteration's contract: pop
    rule, un-popped prefix, multiset of child nodes, tree / sol / best);
  * seeded random nodes with random (limit1, nback).

Node layout (24 bytes): depth, limit1 (signed), prmu[20], nback, pad.
limit2 = jobs - nback, depth = limit1 + 1 + nback, unscheduled positions
limit1 + 1 .. limit2 - 1.
"""
import random
from collections import Counter

NODE = 24
KEY = 23  # depth + limit1 + prmu[20] + nback
HUGE = 2 ** 31 - 1
RULES = ("fwd", "bwd", "alt", "minbranch")


class Tables:
    def __init__(self, core, inst):
        self.inst = inst
        self.jobs = core.taillard_nb_jobs(inst)
        self.machines = core.taillard_nb_machines(inst)
        self.p = list(core.taillard_processing_times(inst))  # [machine * jobs + job]
        n, m, p = self.jobs, self.machines, self.p
        # min over jobs of the work BEFORE machine k / AFTER machine k
        self.min_heads = [min(sum(p[q * n + j] for q in range(k)) for j in range(n))
                          for k in range(m)]
        self.min_tails = [min(sum(p[q * n + j] for q in range(k + 1, m)) for j in range(n))
                          for k in range(m)]
        self.cache = {}  # node key -> (lb_begin, lb_end), see children_bounds


def make_node(limit1, nback, prmu):
    depth = limit1 + 1 + nback
    return bytes([depth, limit1 & 0xFF] + list(prmu) + [nback, 0])


def parse(node):
    limit1 = node[1] - 256 if node[1] > 127 else node[1]
    return node[0], limit1, list(node[2:22]), node[22]


def makespan(T, perm):
    c = [0] * T.machines
    for job in perm:
        c[0] += T.p[job]
        for k in range(1, T.machines):
            c[k] = max(c[k - 1], c[k]) + T.p[k * T.jobs + job]
    return c[-1]


def parts(T, prmu, limit1, nback):
    n, m, p = T.jobs, T.machines, T.p
    limit2 = n - nback
    if limit1 == -1:
        front = list(T.min_heads)
    else:
        front = [0] * m
        for i in range(limit1 + 1):
            job = prmu[i]
            front[0] += p[job]
            for k in range(1, m):
                front[k] = max(front[k - 1], front[k]) + p[k * n + job]
    if nback == 0:
        back = list(T.min_tails)
    else:
        back = [0] * m
        for i in range(n - 1, limit2 - 1, -1):
            job = prmu[i]
            back[m - 1] += p[(m - 1) * n + job]
            for k in range(m - 2, -1, -1):
                back[k] = max(back[k], back[k + 1]) + p[k * n + job]
    remain = [sum(p[k * n + prmu[i]] for i in range(limit1 + 1, limit2)) for k in range(m)]
    return front, back, remain


def bound_front(T, front, back, remain, job):
    n, m, p = T.jobs, T.machines, T.p
    lb = front[0] + remain[0] + back[0]
    t = front[0] + p[job]
    for k in range(1, m):
        s = max(t, front[k])
        lb = max(lb, s + remain[k] + back[k])
        t = s + p[k * n + job]
    return lb


def bound_back(T, front, back, remain, job):
    n, m, p = T.jobs, T.machines, T.p
    lb = front[m - 1] + remain[m - 1] + back[m - 1]
    t = back[m - 1] + p[(m - 1) * n + job]
    for k in range(m - 2, -1, -1):
        s = max(t, back[k])
        lb = max(lb, s + remain[k] + front[k])
        t = s + p[k * n + job]
    return lb


def children_bounds(T, node):
    """(lb_begin, lb_end): dicts position -> bound over the unscheduled positions."""
    key = bytes(node[:KEY])
    hit = T.cache.get(key)  # bounds depend on the node alone, not on rule or incumbent
    if hit is None:
        _, limit1, prmu, nback = parse(node)
        front, back, remain = parts(T, prmu, limit1, nback)
        rng_ = range(limit1 + 1, T.jobs - nback)
        hit = ({k: bound_front(T, front, back, remain, prmu[k]) for k in rng_},
               {k: bound_back(T, front, back, remain, prmu[k]) for k in rng_})
        T.cache[key] = hit
    return hit


def bounds_arrays(T, pool):
    """The layout of pfsp_cpu_bounds_bi / pfsp_gpu_bounds_bi: two flat lists
    [n * jobs] by position, -1 outside a node's unscheduled range."""
    n = len(pool) // NODE
    b, e = [-1] * (n * T.jobs), [-1] * (n * T.jobs)
    for i in range(n):
        f, g = children_bounds(T, pool[i * NODE:(i + 1) * NODE])
        for k, v in f.items():
            b[i * T.jobs + k] = v
        for k, v in g.items():
            e[i * T.jobs + k] = v
    return b, e


def stats(lb_begin, lb_end, best):
    cntF = sum(1 for v in lb_begin.values() if v < best)
    cntB = sum(1 for v in lb_end.values() if v < best)
    return cntF, cntB, sum(lb_begin.values()), sum(lb_end.values())


def backward(rule, depth, lb_begin, lb_end, best):
    """True when the parent's children fix their job at the back."""
    if rule == "fwd":
        return False
    if rule == "bwd":
        return True
    if rule == "alt":
        return depth % 2 == 1
    assert rule == "minbranch", rule
    cntF, cntB, sumF, sumB = stats(lb_begin, lb_end, best)
    return cntB < cntF or (cntB == cntF and sumB > sumF)


def child_of(T, node, k, back):
    depth, limit1, prmu, nback = parse(node)
    pos = T.jobs - nback - 1 if back else limit1 + 1
    prmu[pos], prmu[k] = prmu[k], prmu[pos]
    return make_node(limit1 + (0 if back else 1), nback + (1 if back else 0), prmu)


def expand(T, node, rule, best):
    """Children kept (list of node bytes), solutions counted, min leaf bound."""
    depth = node[0]
    lb_begin, lb_end = children_bounds(T, node)
    back = backward(rule, depth, lb_begin, lb_end, best)
    lbs = lb_end if back else lb_begin
    kept, sol, leaf_min = [], 0, HUGE
    for k in sorted(lbs):
        if depth + 1 == T.jobs:
            sol += 1
            leaf_min = min(leaf_min, lbs[k])
        elif lbs[k] < best:
            kept.append(child_of(T, node, k, back))
    return kept, sol, leaf_min


class Step:
    def __init__(self, prefix, children, ctl):
        self.prefix, self.children, self.ctl = prefix, children, ctl


def step(T, pool, rule, best, m=1, M=None, tree=0, sol=0, iters=0):
    """One devpool iteration: c = 0 if size < m else min(size, M); the last c
    nodes are expanded against the SNAPSHOT incumbent `best`; leaves lower it."""
    size = len(pool) // NODE
    M = max(size, 1) if M is None else M
    c = 0 if size < m else min(size, M)
    base = size - c
    pushed, best_out = [], best
    for i in range(base, size):
        kept, s, leaf_min = expand(T, pool[i * NODE:(i + 1) * NODE], rule, best)
        pushed += kept
        sol += s
        best_out = min(best_out, leaf_min)
    ctl = dict(size=base + len(pushed), chunk=c, tree=tree + len(pushed), sol=sol,
               iters=iters + (1 if c else 0), best=best_out, overflow=0)
    return Step(pool[:base * NODE], pushed, ctl)


def check_step(exp, pool_out, ctl, what=""):
    for f in ("chunk", "iters", "overflow", "size", "sol", "tree", "best"):
        assert ctl[f] == exp.ctl[f], (what, f, ctl[f], exp.ctl[f])
    assert len(pool_out) == exp.ctl["size"] * NODE, (what, len(pool_out))
    nb = len(exp.prefix)
    assert pool_out[:nb] == exp.prefix, (what, "un-popped prefix changed")
    got = Counter(pool_out[i:i + KEY] for i in range(nb, len(pool_out), NODE))
    want = Counter(ch[:KEY] for ch in exp.children)
    if got != want:
        missing = [list(x) for x in list((want - got).elements())[:3]]
        extra = [list(x) for x in list((got - want).elements())[:3]]
        raise AssertionError((what, "children differ", "missing", missing, "unexpected", extra))


def search(T, rule, best, pool=None, limit=10 ** 7):
    """Depth-first search to exhaustion (small trees only): tree, sol, best."""
    stack = [make_node(-1, 0, range(T.jobs))] if pool is None else \
        [pool[i:i + NODE] for i in range(0, len(pool), NODE)]
    tree = sol = 0
    while stack:
        kept, s, leaf_min = expand(T, stack.pop(), rule, best)
        best = min(best, leaf_min)
        sol += s
        tree += len(kept)
        stack += kept
        assert tree <= limit
    return tree, sol, best


def random_nodes(rng, n, jobs=20, min_depth=0, max_depth=None, force=()):
    """n seeded random nodes: random permutation, random (limit1, nback) with
    limit1 + 1 + nback <= jobs - 1. `force` is a list of (limit1, nback) pairs
    the first nodes take (edge cases the caller wants present)."""
    max_depth = jobs - 1 if max_depth is None else max_depth
    out = []
    for i in range(n):
        prmu = list(range(jobs))
        rng.shuffle(prmu)
        if i < len(force):
            limit1, nback = force[i]
        else:
            depth = rng.randint(min_depth, max_depth)
            nback = rng.randint(0, depth)
            limit1 = depth - nback - 1
        out.append(make_node(limit1, nback, prmu))
    return b"".join(out)


# edge cases every random node set starts with: nothing at the front with jobs
# at the back (min_heads front), nothing at the back, the root, depth jobs-1
# in its three shapes
def edge_cases(jobs=20):
    return [(-1, 3), (-1, jobs - 1), (4, 0), (-1, 0), (jobs - 2, 0), (8, jobs - 10),
            (0, jobs - 2)]


def rng(seed):
    return random.Random(seed)
