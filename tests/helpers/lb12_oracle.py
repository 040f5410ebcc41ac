"""Pure-Python oracle for the two-stage PFSP bound lb12: lb1_d picks the
branching direction and filters the children, lb2 (Johnson) bounds only the
survivors.

Written from the rule text and independent of the C++ and HIP code. The lb1_d
half (child bounds in both directions, the direction decision, the node
layout, the one-step contract and its checker) comes from bi_oracle; the lb2
half is a GENERAL Johnson bound here, taking a front schedule, a back schedule
and a scheduled-job set, with no early exit, over the pair tables built the way
py_bounds.py_lb2_bound builds them.

The point the oracle exists for: lb1_d bounds a child from the PARENT's front /
back, which are min_heads / min_tails where nothing is fixed, while lb2 bounds
the CHILD: its changed side is scheduled from zeros (the child has a job
there), its unchanged side keeps min_heads / min_tails when nothing is fixed
on it.
"""
import bi_oracle as bo
import py_bounds  # noqa: F401  (the table construction below mirrors py_lb2_bound's)

NODE, KEY, HUGE, RULES = bo.NODE, bo.KEY, bo.HUGE, bo.RULES


def johnson_tables(T):
    """Per machine pair (m1 < m2), lexicographic: (m1, m2, [(job, p1, p2, lag)] in
    Johnson order): jobs with p1 + lag < p2 + lag first by ascending p1 + lag,
    the rest by descending p2 + lag (py_bounds.py_lb2_bound's sort key)."""
    if getattr(T, "johnson", None) is None:
        n, m, p = T.jobs, T.machines, T.p
        out = []
        for m1 in range(m - 1):
            for m2 in range(m1 + 1, m):
                lags = [sum(p[mm * n + j] for mm in range(m1 + 1, m2)) for j in range(n)]
                jj = []
                for j in range(n):
                    a, b = p[m1 * n + j] + lags[j], p[m2 * n + j] + lags[j]
                    jj.append((0 if a < b else 1, a if a < b else -b, j))
                jj.sort(key=lambda t: (t[0], t[1]))
                out.append((m1, m2, [(j, p[m1 * n + j], p[m2 * n + j], lags[j])
                                     for _, _, j in jj]))
        T.johnson = out
        T.lb2_cache = {}
    return T.johnson


def lb2_general(T, front, back, scheduled):
    """max over all machine pairs of the two-machine (with lags) makespan of the
    unscheduled jobs in Johnson order, started from `front`, closed by `back`."""
    lb = 0
    for m1, m2, order in johnson_tables(T):
        t0, t1 = front[m1], front[m2]
        for job, p1, p2, lag in order:
            if job in scheduled:
                continue
            t0 += p1
            t1 = max(t1, t0 + lag) + p2
        lb = max(lb, t1 + back[m2], t0 + back[m1])
    return lb


def schedule_front(T, seq):
    """Completion times of the jobs `seq` scheduled first; min_heads if none."""
    if not seq:
        return list(T.min_heads)
    n, m, p = T.jobs, T.machines, T.p
    front = [0] * m
    for job in seq:
        front[0] += p[job]
        for k in range(1, m):
            front[k] = max(front[k - 1], front[k]) + p[k * n + job]
    return front


def schedule_back(T, seq):
    """Run-out times of the jobs `seq` scheduled last (seq in permutation order:
    the LAST entry is added first); min_tails if none."""
    if not seq:
        return list(T.min_tails)
    n, m, p = T.jobs, T.machines, T.p
    back = [0] * m
    for job in reversed(seq):
        back[m - 1] += p[(m - 1) * n + job]
        for k in range(m - 2, -1, -1):
            back[k] = max(back[k], back[k + 1]) + p[k * n + job]
    return back


def child_lb2(T, node, k, back):
    """Exact lb2 of the child that fixes prmu[k] at the front / at the back: the
    bound of the CHILD node, from its own front, back and scheduled set."""
    johnson_tables(T)
    key = (bytes(node[:KEY]), k, back)
    hit = T.lb2_cache.get(key)  # depends on the node and the child alone
    if hit is None:
        _, limit1, prmu, nback = bo.parse(node)
        pre, suf = prmu[:limit1 + 1], prmu[T.jobs - nback:]
        job = prmu[k]
        if back:
            suf = [job] + suf
        else:
            pre = pre + [job]
        hit = lb2_general(T, schedule_front(T, pre), schedule_back(T, suf), set(pre) | set(suf))
        T.lb2_cache[key] = hit
    return hit


def evaluate(T, node, rule, best):
    """(back, {position: (value, is_lb2)}): the direction, and per unscheduled
    position the lb1_d value of that direction (leaf parent, or lb1_d >= best:
    no lb2 is evaluated) or the exact lb2 value of the child."""
    depth = node[0]
    lb_begin, lb_end = bo.children_bounds(T, node)
    back = bo.backward(rule, depth, lb_begin, lb_end, best)
    b1s = lb_end if back else lb_begin
    leaf = depth + 1 == T.jobs
    out = {}
    for k in sorted(b1s):
        if leaf or b1s[k] >= best:
            out[k] = (b1s[k], False)
        else:
            out[k] = (child_lb2(T, node, k, back), True)
    return back, out


def bounds_arrays(T, pool, rule, best):
    """The layout of pfsp_cpu_bounds_lb12 / pfsp_gpu_bounds_lb12: dir [n], values
    [n * jobs] (-1 outside the unscheduled range), plus is_lb2 flags [n * jobs]."""
    n = len(pool) // NODE
    dirs, vals, kinds = [0] * n, [-1] * (n * T.jobs), [False] * (n * T.jobs)
    for i in range(n):
        back, out = evaluate(T, pool[i * NODE:(i + 1) * NODE], rule, best)
        dirs[i] = 1 if back else 0
        for k, (v, is_lb2) in out.items():
            vals[i * T.jobs + k] = v
            kinds[i * T.jobs + k] = is_lb2
    return dirs, vals, kinds


def check_bounds(exp, got, best, what=""):
    """dir equal everywhere; lb1_d values equal; an lb2 value equal where the
    oracle's is <= best, and otherwise merely > best (the implementations stop
    sweeping pairs once the bound exceeds the incumbent)."""
    (e_dir, e_val, e_kind), (g_dir, g_val) = exp, got
    assert list(g_dir) == e_dir, (what, "dir")
    g_val = list(g_val)
    assert len(g_val) == len(e_val), (what, len(g_val))
    for i, (e, g, is_lb2) in enumerate(zip(e_val, g_val, e_kind)):
        if is_lb2 and e > best:
            assert g > best, (what, i, g, e, best)
        else:
            assert g == e, (what, i, g, e, is_lb2)


def expand(T, node, rule, best):
    """Children kept (list of node bytes), solutions counted, min leaf bound."""
    leaf = node[0] + 1 == T.jobs
    back, out = evaluate(T, node, rule, best)
    kept, sol, leaf_min = [], 0, HUGE
    for k in sorted(out):
        v = out[k][0]
        if leaf:
            sol += 1
            leaf_min = min(leaf_min, v)
        elif v < best:
            kept.append(bo.child_of(T, node, k, back))
    return kept, sol, leaf_min


def step(T, pool, rule, best, m=1, M=None, tree=0, sol=0, iters=0):
    """One devpool iteration (bi_oracle.step's contract) under lb12."""
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
    return bo.Step(pool[:base * NODE], pushed, ctl)


def step_from_arrays(T, pool, dirs, vals, best, m=1, M=None):
    """The same iteration from (dir, bounds) arrays in the eval layout, e.g. the
    C++ host rule's (which the CPU tests pin to this oracle): for pools too
    large to run through the Python lb2."""
    size = len(pool) // NODE
    M = max(size, 1) if M is None else M
    c = 0 if size < m else min(size, M)
    base = size - c
    pushed, sol, best_out = [], 0, best
    for i in range(base, size):
        node = pool[i * NODE:(i + 1) * NODE]
        leaf = node[0] + 1 == T.jobs
        for k in range(T.jobs):
            v = vals[i * T.jobs + k]
            if v < 0:
                continue
            if leaf:
                sol += 1
                best_out = min(best_out, v)
            elif v < best:
                pushed.append(bo.child_of(T, node, k, bool(dirs[i])))
    ctl = dict(size=base + len(pushed), chunk=c, tree=len(pushed), sol=sol,
               iters=1 if c else 0, best=best_out, overflow=0)
    return bo.Step(pool[:base * NODE], pushed, ctl)


check_step = bo.check_step


def search(T, rule, best, pool=None, limit=10 ** 6):
    """Depth-first search to exhaustion (small trees only): tree, sol, best."""
    stack = [bo.make_node(-1, 0, range(T.jobs))] if pool is None else \
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
