#!/usr/bin/env python3
"""CPU model of how k_nq_x's finisher keeps its lanes busy (no GPU needed).

Plays nq_flat_run (src/nq_finish.hpp) literally on sampled N = 17 tiles and
counts loop iterations per lane. A tile is what one block sees: sibling groups
of depth-8 parents under random depth-6 prefixes, 60 parents, all their safe
children as jobs (8 rows left each). A wave is charged 64 x the iterations of
its longest lane; lane efficiency = iterations that did work / lane slots
charged. One iteration is charged per job fetch (the iteration that loads a
job also takes its first candidate, as in the kernel).

Schedules: whole jobs or jobs split 1..3 levels into sub-jobs (the rule of
nq_split_job: min(S, rem - 1) levels), handed out by static stride
(t, t + 256, ...) or dynamically (a lane that finishes takes the next queue
entry), with an optional queue capacity drained in rounds.

What the model leaves out, and what the measurement showed it matters
(docs/DESIGN.md section 3): the instructions of the fetch path itself. A wave
executes them whenever ANY of its lanes fetches, so with five sub-jobs per
lane nearly every iteration of a wave carries a fetch for one or two lanes.

The wave-stack schedule (nq_stack_act and friends) is played as well: a lane
owns a row and takes one candidate per iteration, children with an inner row
below them go onto the wave's stack, idle lanes take entries off it or draw
jobs. Reported: wave iterations, lane efficiency, fetch passes, the longest
wave, and the peak stack height per wave, from which NQ_STACK_CAP is chosen;
with --cap the pushes stop at sp + 64 > cap as in the kernel and the children
walked instead are counted (their walk's iterations are charged to the wave).

usage: nq_lane_model.py [--tiles 24] [--seed 1] [--N 17] [--cap 312]
"""
import argparse
import heapq
import random

LANES, WAVE = 256, 64


def free_of(c, d1, d2, msk):
    return ~(c | d1 | d2) & msk


def down(c, d1, d2, bit, msk):
    return c | bit, ((d1 | bit) << 1) & msk, (d2 | bit) >> 1


def flat_iters(c, d1, d2, row, N):
    """Iterations nq_flat_run spends on the job, the loading one included."""
    msk = (1 << N) - 1
    h = N - 1 - row
    stack, cand, loaded, it = [], 0, False, 0
    while True:
        if cand == 0:
            if not stack:
                if loaded:
                    return it
                loaded = True
                cand = free_of(c, d1, d2, msk) if h else 0
            else:  # pop
                c, d1, d2, col = stack.pop()
                h += 1
                cand = free_of(c, d1, d2, msk) & (~1 << col)
        if cand:  # take
            bit = cand & -cand
            cand ^= bit
            n = down(c, d1, d2, bit, msk)
            nf = free_of(*n, msk)
            if h > 1 and nf:
                stack.append((c, d1, d2, bit.bit_length() - 1))
                c, d1, d2 = n
                h -= 1
                cand = nf
        it += 1


def split(job, N, S):
    """Sub-jobs of a job, in queue order."""
    c, d1, d2, row = job
    msk = (1 << N) - 1
    out = [job]
    for _ in range(max(0, min(S, N - row - 1))):
        nxt = []
        for (c, d1, d2, row) in out:
            f = free_of(c, d1, d2, msk)
            while f:
                bit = f & -f
                f ^= bit
                nxt.append(down(c, d1, d2, bit, msk) + (row + 1,))
        out = nxt
    return out


def sample_tile(rng, N, parents=60, prefix_depth=6, parent_depth=8):
    msk = (1 << N) - 1

    def children(node):
        c, d1, d2, row = node
        f = free_of(c, d1, d2, msk)
        while f:
            bit = f & -f
            f ^= bit
            yield down(c, d1, d2, bit, msk) + (row + 1,)

    tile = []
    while len(tile) < parents:
        node = (0, 0, 0, 0)
        while node and node[3] < prefix_depth:  # a random safe prefix
            kids = list(children(node))
            node = rng.choice(kids) if kids else None
        if node is None:
            continue
        level = [node]
        for _ in range(parent_depth - prefix_depth):
            level = [k for n in level for k in children(n)]
        tile += level
    tile = tile[:parents]
    return [k for p in tile for k in children(p)]  # the jobs: safe children


def waves_cost(finish):
    return sum(WAVE * max(finish[w:w + WAVE]) for w in range(0, LANES, WAVE))


def run_static(lengths):
    finish = [0] * LANES
    for q, n in enumerate(lengths):
        finish[q % LANES] += n
    return waves_cost(finish)


def run_dynamic(lengths):
    heap = [(0, t) for t in range(LANES)]
    finish = [0] * LANES
    for n in lengths:
        t0, t = heapq.heappop(heap)
        finish[t] = t0 + n
        heapq.heappush(heap, (finish[t], t))
    return waves_cost(finish)


def schedule(jobs, N, S, dynamic, qcap=None):
    """(work, cost, entries) of one tile."""
    groups = [[flat_iters(*sj, N) for sj in split(j, N, S)] for j in jobs]
    run = run_dynamic if dynamic else run_static
    work = sum(map(sum, groups))
    entries = sum(map(len, groups))
    if qcap is None:
        return work, run([n for g in groups for n in g]), entries
    cost, cur = 0, []
    for g in groups:  # rounds: the longest run of jobs that fits
        if cur and len(cur) + len(g) > qcap:
            cost += run(cur)
            cur = []
        cur += g
    return work, cost + run(cur), entries


def run_waves(lengths, T, nwaves=LANES // WAVE):
    """The batched refill (nq_refill_now) on one round's entries: nwaves waves
    of WAVE lockstep lanes on one queue head; a wave fetches for all of its
    idle lanes when it is not drained and T of them, or all, are idle. The
    wave that is furthest behind in time moves next. Returns (iterations,
    iterations that executed the fetch path), summed over the waves."""
    left = [[0] * WAVE for _ in range(nwaves)]  # iterations left per lane
    drained = [False] * nwaves
    clock = [(0, w) for w in range(nwaves)]
    head = iters = fetches = 0
    while clock:
        t, w = heapq.heappop(clock)
        lanes = left[w]
        idle = [i for i, r in enumerate(lanes) if r == 0]
        if not drained[w] and idle and (len(idle) >= T or len(idle) == WAVE):
            got, head = head, head + len(idle)
            drained[w] = got + len(idle) >= len(lengths)
            for k, i in enumerate(idle):
                if got + k < len(lengths):
                    lanes[i] = lengths[got + k]
            fetches += 1
        elif drained[w] and len(idle) == WAVE:
            continue  # the wave leaves
        left[w] = [r - 1 if r else 0 for r in lanes]
        iters += 1
        heapq.heappush(clock, (t + 1, w))
    return iters, fetches


def schedule_waves(jobs, N, S, T, qcap):
    """(work, iterations, fetch iterations) of one tile, in rounds of qcap."""
    groups = [[flat_iters(*sj, N) for sj in split(j, N, S)] for j in jobs]
    work = sum(map(sum, groups))
    iters = fetches = 0
    cur = []
    for g in groups + [None]:
        if g is None or (cur and len(cur) + len(g) > qcap):
            i, f = run_waves(cur, T)
            iters, fetches = iters + i, fetches + f
            cur = []
        if g:
            cur += g
    return work, iters, fetches


def run_stack(jobs, N, T, shared=True, cap=None, fair=True, nwaves=LANES // WAVE):
    """The wave-stack finisher on one tile. shared: idle lanes draw jobs from
    one counter, at most the wave's even share per refill when `fair` (the
    kernel's rule, nq_stack_draw), else one per idle lane; otherwise the jobs are dealt round-robin
    onto the waves' stacks in advance. cap None: unbounded stacks. Returns
    (takes, iterations summed over the waves, fetch passes, longest wave,
    peak stack of a wave, children walked by the fallback)."""
    msk = (1 << N) - 1
    stk = [[] for _ in range(nwaves)]
    queue = list(jobs) if shared else []
    if not shared:
        for q, (c, d1, d2, row) in enumerate(jobs):
            stk[q % nwaves].append((c, d1, d2, N - 1 - row))
    head = 0
    rows = [[None] * WAVE for _ in range(nwaves)]  # [c, d1, d2, h, cand] or None
    more = [shared] * nwaves
    its = [0] * nwaves
    takes = fetches = peak = walked = 0
    clock = [(0, w) for w in range(nwaves)]
    while clock:
        t, w = heapq.heappop(clock)
        lanes, st = rows[w], stk[w]
        idle = [i for i, r in enumerate(lanes) if r is None]
        if len(idle) == WAVE or ((st or more[w]) and len(idle) >= T):
            if len(idle) == WAVE and not st and not more[w]:
                continue  # the wave leaves
            fetches += 1
            share = max(1, -(-len(queue) // nwaves)) if fair else WAVE  # nq_stack_draw
            for i in idle:
                if st:
                    c, d1, d2, h = st.pop()
                elif more[w]:
                    if head >= len(queue) or share == 0:
                        break
                    share -= 1
                    c, d1, d2, row = queue[head]
                    head += 1
                    h = N - 1 - row
                else:
                    break
                cand = free_of(c, d1, d2, msk)
                if cand and h:
                    lanes[i] = [c, d1, d2, h, cand]
            if more[w] and head >= len(queue):
                more[w] = False
        can = cap is None or len(st) + WAVE <= cap
        extra = 0
        for i, r in enumerate(lanes):
            if r is None:
                continue
            c, d1, d2, h, cand = r
            bit = cand & -cand
            r[4] = cand ^ bit
            takes += 1
            if h > 1:
                n = down(c, d1, d2, bit, msk)
                if free_of(*n, msk):
                    if can:
                        st.append(n + (h - 1,))
                    else:  # the lane walks the child; the whole wave waits
                        walked += 1
                        extra = max(extra, flat_iters(*n, N - h, N) - 1)
            if r[4] == 0:
                lanes[i] = None
        peak = max(peak, len(st))
        its[w] += 1 + extra
        heapq.heappush(clock, (t + 1 + extra, w))
    return takes, sum(its), fetches, max(its), peak, walked


def stack_table(tiles, N, cap):
    print()
    print("wave stack, four waves; refill when >= T lanes are idle (per tile; peak over all tiles)")
    print(f"{'seeds':>8s} {'cap':>5s} {'T':>3s} {'wave iters':>10s} {'lane eff.':>9s} "
          f"{'fetches':>8s} {'longest':>8s} {'peak sp':>8s} {'walked':>7s}")
    for shared, fair in ((True, True), (True, False), (False, False)):
        for c in (None, cap):
            for T in (1, 8, 16, 24):
                tk = it = fe = lo = wk = pk = 0
                for jobs in tiles:
                    a = run_stack(jobs, N, T, shared, c, fair)
                    tk, it, fe, lo, wk = tk + a[0], it + a[1], fe + a[2], lo + a[3], wk + a[5]
                    pk = max(pk, a[4])
                n = len(tiles)
                seeds = ('share' if fair else 'queue') if shared else 'dealt'
                print(f"{seeds:>8s} {c or 'inf':>5} {T:3d} {it / n:10.0f} "
                      f"{tk / (it * WAVE):9.2f} {fe / n:8.0f} {lo / n:8.0f} {pk:8d} {wk / n:7.0f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=24)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--N", type=int, default=17)
    ap.add_argument("--cap", type=int, default=312, help="wave-stack capacity [entries]")
    a = ap.parse_args()
    rng = random.Random(a.seed)
    tiles = [sample_tile(rng, a.N) for _ in range(a.tiles)]
    rows = [("whole jobs, static stride", 0, False, None),
            ("whole jobs, dynamic", 0, True, None),
            ("split 1, static stride", 1, False, None),
            ("split 1, dynamic", 1, True, None),
            ("split 2, static stride", 2, False, None),
            ("split 2, dynamic", 2, True, None),
            ("split 2, dynamic, queue 1024", 2, True, 1024),
            ("split 2, dynamic, queue 1728", 2, True, 1728),
            ("split 2, dynamic, queue 2048", 2, True, 2048),
            ("split 3, dynamic, queue 2048", 3, True, 2048),
            ("split 3, dynamic, queue 4096", 3, True, 4096)]
    base = None
    print(f"N = {a.N}, {a.tiles} tiles, {sum(map(len, tiles)) / a.tiles:.0f} jobs per tile")
    print(f"{'schedule':34s} {'entries':>8s} {'lane eff.':>9s} {'cost vs today':>13s}")
    for name, S, dyn, qcap in rows:
        work = cost = entries = 0
        for jobs in tiles:
            w, c, e = schedule(jobs, a.N, S, dyn, qcap)
            work, cost, entries = work + w, cost + c, entries + e
        base = base or cost
        print(f"{name:34s} {entries / a.tiles:8.0f} {work / cost:9.2f} {cost / base:13.2f}")
    # Wave-level accounting of the batched refill (split 2, queue 1728): a
    # wave iteration costs 1, one that executes the fetch path costs F; summed
    # over the block's waves, per tile, in thousands of step costs.
    fs = (1.0, 1.5, 2.0)
    print()
    print("split 2, queue 1728, four waves on one queue head; refill when >= T lanes are idle")
    print(f"{'T':>4s} {'fetch iters':>11s} {'lane eff.':>9s} " +
          " ".join(f"{'cost F=' + str(f):>11s}" for f in fs) + "   (per tile)")
    for T in (1, 4, 8, 12, 16, 24, 32, 64):
        work = iters = fetches = 0
        for jobs in tiles:
            w, i, f = schedule_waves(jobs, a.N, 2, T, 1728)
            work, iters, fetches = work + w, iters + i, fetches + f
        print(f"{T:4d} {fetches / a.tiles:11.0f} {work / (iters * WAVE):9.2f} " +
              " ".join(f"{(iters + (f - 1) * fetches) / a.tiles:11.0f}" for f in fs))
    stack_table(tiles, a.N, a.cap)


if __name__ == "__main__":
    main()
