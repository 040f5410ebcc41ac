"""Shared cases of the N-Queens finisher tests (tests/test_nq_*_finisher.py,
test_nq_batched_refill.py and their test_gpu_* counterparts).

CPU side: masks stepped in Python and random job states (cols, d1, d2, row).
GPU side: pools whose blocks' job queues have a named shape, the jobs of a
pool's blocks as the CPU twins take them, and run_nq, which runs ONE devpool
iteration twice and compares it with the pure-CPU step oracle
(devpool_step_oracle.py).
"""
import random

import devpool_step_oracle as orc

TILE = 1024  # child slots per block


# ---------------------------------------------------------------------------
# masks and job states
# ---------------------------------------------------------------------------

def free_mask(cols, d1, d2, N):
    return ~(cols | d1 | d2) & ((1 << N) - 1)


def bits(f):
    while f:
        b = f & -f
        f ^= b
        yield b


def step(cols, d1, d2, b, N):
    msk = (1 << N) - 1
    return cols | b, ((d1 | b) << 1) & msk, (d2 | b) >> 1


def fanout(job, N, split):
    """Sub-jobs of one job, from the masks alone."""
    cols, d1, d2, row = job
    lv = max(0, min(split, N - row - 1))
    if lv == 0:
        return 1
    f0 = free_mask(cols, d1, d2, N)
    if lv == 1:
        return bin(f0).count("1")
    return sum(bin(free_mask(*step(cols, d1, d2, b, N), N)).count("1") for b in bits(f0))


def masks(N, row, queens):
    """(cols, d1, d2) as the kernel steps them: the squares of `row` attacked
    by column, by the diagonal moving right and by the one moving left."""
    cols = d1 = d2 = 0
    for qr, qc in queens:
        cols |= 1 << qc
        a, b = qc + (row - qr), qc - (row - qr)
        if 0 <= a < N:
            d1 |= 1 << a
        if 0 <= b < N:
            d2 |= 1 << b
    return cols, d1, d2


def random_job(rng, N, rows):
    """A state with `rows` empty rows: distinct random columns for the rows
    above (they may attack each other diagonally: the walk is a function of the
    masks)."""
    row = N - rows
    return masks(N, row, enumerate(rng.sample(range(N), row))) + (row,)


def jobs_n13():
    """96 jobs of N = 13, twelve of every height 1..8."""
    rng = random.Random(1300)
    return [random_job(rng, 13, rows) for rows in range(1, 9) for _ in range(12)]


# ---------------------------------------------------------------------------
# pools and their blocks' job queues
# ---------------------------------------------------------------------------

def root(N):
    return orc.nq_node(0, list(range(N)))


def leaf(N):
    return orc.nq_node(N, list(range(N)))


def one_job_node(core, rng, N):
    """A depth N-2 node (two candidate children, one row below them) of which
    exactly one child is safe: one job with one row left, which is never split
    (one sub-job)."""
    while True:
        node = orc.random_nq_nodes(rng, 1, N, N - 2, N - 2)
        lab = core.nq_cpu_labels(N, 1, node)
        if sum(lab[k] == 1 for k in range(N - 2, N)) == 1:
            return node


def block_jobs(core, pool, N, finish):
    """Per block, the finisher jobs in queue (= slot) order, as the states
    (cols, d1, d2, row) below the safe child."""
    n = len(pool) // 24
    labels = core.nq_cpu_labels(N, 1, pool)
    msk = (1 << N) - 1
    blocks = [[] for _ in range((n * N + TILE - 1) // TILE)]
    for t in range(n * N):
        pid, k = divmod(t, N)
        node = pool[pid * 24:(pid + 1) * 24]
        depth = node[0]
        if depth >= N or k < depth or labels[t] != 1 or not 0 < N - depth - 1 <= finish:
            continue
        cols = d1 = d2 = 0
        for col in list(node[1:1 + depth]) + [node[1 + k]]:
            cols |= 1 << col
            d1 = ((d1 | 1 << col) << 1) & msk
            d2 = (d2 | 1 << col) >> 1
        blocks[t // TILE].append((cols, d1, d2, depth + 1))
    return blocks


_split_shapes = {}


def split_shape(core, pool, N, split, finish=8):
    """Per block: (jobs, sub-jobs, rounds) at the kernel's queue capacity."""
    key = (pool, N, split, finish)
    if key not in _split_shapes:
        out = []
        for jobs in block_jobs(core, pool, N, finish):
            _, _, entries, rounds = core.nq_finish_block_cpu(jobs, N, 1, split,
                                                             core.NQ_SPLIT_QCAP)
            out.append((len(jobs), entries, rounds))
        _split_shapes[key] = out
    return _split_shapes[key]


_pools = {}


def pool_with_subjobs(core, split, target):
    """One block of N = 9 nodes whose jobs split into exactly `target`
    sub-jobs: depth-0 parents (56 / 234 sub-jobs at split 1 / 2), depth-1
    parents and single-sub-job nodes, largest first."""
    if (split, target) in _pools:
        return _pools[split, target]
    N = 9
    rng = orc.rng(9000 + target)
    menu = [root(N)] + [orc.nq_node(1, [c] + [x for x in range(N) if x != c]) for c in (0, 4)]
    menu = sorted(((split_shape(core, node, N, split)[0][1], node) for node in menu),
                  reverse=True)
    pool, left = b"", target
    for entries, node in menu:
        pool += node * (left // entries)
        left %= entries
    pool += b"".join(one_job_node(core, rng, N) for _ in range(left))
    assert len(pool) // 24 * N <= TILE
    _pools[split, target] = pool
    return pool


_oracle_cache = {}


def run_nq(gpu, pool, N, g=1, finish=8, m=1, M=None, what="", *, split=-1, refill=-1, stack=-1,
           stack_cap=-1):
    """One iteration, twice: the two runs must be byte-identical and equal the
    step oracle. Returns (expected, (pool bytes, ctl))."""
    # the oracle's counts depend on neither g nor the finisher's knobs
    key = (pool, N, finish, m, M)
    if key not in _oracle_cache:
        _oracle_cache[key] = orc.nq_step(gpu, pool, N, 1, finish, m, M)
    exp = _oracle_cache[key]
    args = (pool, N, g, finish, m, M, None, "auto", 0, split, refill, stack, stack_cap)
    a = gpu.nq_devpool_step(*args)
    b = gpu.nq_devpool_step(*args)
    what = ("nq", what, "N", N, "n", len(pool) // 24, "g", g, "finish", finish, "m", m, "M", M,
            "split", split, "refill", refill, "stack", stack, "stack_cap", stack_cap)
    assert a == b, (what, "two runs differ")
    orc.check_step(exp, a[0], a[1], what)
    return exp, a
