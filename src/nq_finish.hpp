// Flat (single-loop, stackless) bitmask DFS over the last levels of the
// N-Queens tree. Shared by the k_nq_x finisher (device) and by the CPU entry
// point nq_finish_count_cpu, so the loop that runs on the GPU is the loop the
// CPU tests walk.
//
// A job is the state below one safe child: (cols, d1, d2) are the occupied
// column / diagonal masks seen from row `row` (the first empty row), exactly
// what the recursive finisher used to receive. The walk counts every safe
// node below the job (tree) and every placement that fills row N-1 (sol).
//
// State, all in scalars (nothing is indexed at run time, so nothing spills):
//   h      rows below the current row (N - 1 - row); the bottom row is h == 0
//   cols   occupied columns
//   D1     diagonal that moves one column up per row, as seen from the current
//          row: bit c set = column c attacked. Stepped `(D1 | bit) << 1` on the
//          way down and NEVER masked, so `D1 >> 1` on the way up restores it.
//   D2     diagonal that moves one column down per row, kept G guard bits to
//          the left (column c is bit c + G): stepped `(D2 | bit << G) >> 1`,
//          so the bits that leave the board stay in the word and
//          `D2 << 1` restores it.
//          -> free squares of the current row: ~(cols | D1 | D2 >> G) & msk
//   stack  the columns chosen below the job's root, one 5-bit field per level,
//          newest lowest, under a sentinel 1 bit; stack == 1 means "at the
//          job's root", stack == 0 "no job"
//   cand   candidates of the current row that are still to be taken
// The bottom row is never descended into (its candidates are counted with one
// popcount from the row above), so a walk of LEVELS rows descends at most
// G = LEVELS - 2 times: with N <= 20 both diagonals stay below bit N + G, i.e.
// inside 32 bits up to LEVELS = 12, and the stack needs 5 G + 1 bits: 31 for
// LEVELS = 8 (u32, the kernel's instantiation), 51 for LEVELS = 12 (u64, CPU
// only).
//
// One step is "pop if the row is exhausted, then take the next candidate if
// there is one": lanes of a wave that sit at different depths, or in different
// jobs, execute the same instructions, and no shift amount depends on the
// depth. Backtracking keeps no per-level candidate set; it clears the popped
// column's three bits, re-derives the free mask of that row and drops the
// candidates up to and including that column.
#pragma once

#include <cstdint>
#include <type_traits>

#if defined(__HIPCC__)
#define NQ_HD __host__ __device__
#else
#define NQ_HD
#endif

namespace gats {

// Free-column mask evaluated g times as a LIVE dependency chain (devpool
// path's g semantics: the per-node safety evaluation is the mask combine +
// negate, so g repeats exactly that). Each repeat's asm makes `occ` opaque,
// so the OR/ANDN must really execute every round; the result is the identity
// ~occ & msk.
NQ_HD inline uint32_t nq_free_occ_g(uint32_t occ0, uint32_t msk, int g) {
  uint32_t free = 0, occ = occ0;
  for (int r = 0; r < g; r++) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(occ));
#else
    asm volatile("" : "+r"(occ));
#endif
    occ |= occ0;         // identity; non-foldable through the barrier
    free |= ~occ & msk;  // idempotent accumulate keeps every repeat live
  }
  return free;
}

inline constexpr int NQ_FLAT_LEVELS_DEV = 8;   // == the kernel's finisher depth limit
inline constexpr int NQ_FLAT_LEVELS_MAX = 12;  // widest walk the 32-bit diagonals hold

template <int LEVELS>
struct NqFlat {
  static_assert(LEVELS >= 1 && LEVELS <= NQ_FLAT_LEVELS_MAX, "diagonal masks are 32-bit");
  static constexpr int G = LEVELS >= 2 ? LEVELS - 2 : 0;
  using Stack = typename std::conditional<(5 * G + 1 <= 32), uint32_t, uint64_t>::type;
  uint32_t cols, D1, D2, cand;
  Stack stack;
  int h;
  // subtree counters; 32 bits hold them: a job with r rows left has at most r
  // free columns, so at most sum_i r!/(r-i)! nodes (109,600 for r = 8,
  // 1.3e9 for r = 12)
  uint32_t tree, sol;

  NQ_HD uint32_t occupied() const { return cols | D1 | (D2 >> G); }

  // Start the walk below (cols, d1, d2) at `row`; needs 1 <= N - row <= LEVELS.
  // G1 == false evaluates the root's free mask g times (its first evaluation).
  template <bool G1>
  NQ_HD void load(uint32_t c, uint32_t d1, uint32_t d2, int row, int N, uint32_t msk, int g) {
    h = N - 1 - row;
    cols = c;
    D1 = d1;
    D2 = d2 << G;
    stack = 1;
    const uint32_t occ = occupied();
    cand = G1 ? (~occ & msk) : nq_free_occ_g(occ, msk, g);
    if (h == 0) {  // the job's root is the bottom row: every candidate is a solution
      const uint32_t n = static_cast<uint32_t>(__builtin_popcount(cand));
      tree += n;
      sol += n;
      cand = 0;
    }
  }

  // Backtrack one level (stack > 1): re-derive the row's remaining candidates.
  NQ_HD void pop(uint32_t msk) {
    const int c = static_cast<int>(stack & 31u);
    stack >>= 5;
    const uint32_t bit = 1u << c;
    h++;
    cols ^= bit;
    D1 = (D1 >> 1) ^ bit;
    D2 = (D2 << 1) ^ (bit << G);
    cand = ~occupied() & msk & (~1u << c);
  }

  // Take the lowest candidate of the current row (cand != 0, h >= 1): count
  // it, count its children with a popcount when they are the bottom row, and
  // descend only when it has children in an inner row. (`bit` is free, so it
  // is in none of the three masks and + sets it like | would.)
  template <bool G1>
  NQ_HD void take(uint32_t msk, int g) {
    const uint32_t bit = cand & (0u - cand);
    cand ^= bit;
    tree++;
    const uint32_t nc = cols + bit;
    const uint32_t n1 = (D1 + bit) << 1;
    const uint32_t n2 = (D2 + (bit << G)) >> 1;
    const uint32_t occ = nc | n1 | (n2 >> G);
    const uint32_t nf = G1 ? (~occ & msk) : nq_free_occ_g(occ, msk, g);
    if (h == 1) {
      const uint32_t n = static_cast<uint32_t>(__builtin_popcount(nf));
      tree += n;
      sol += n;
    } else if (nf) {
      cols = nc;
      D1 = n1;
      D2 = n2;
      stack = (stack << 5) | static_cast<Stack>(__builtin_ctz(bit));
      h--;
      cand = nf;
    }
  }

  // Run the loaded walk to its end: pop / take until no candidate is left at
  // the job's root. Returns the number of steps.
  template <bool G1>
  NQ_HD uint64_t exhaust(uint32_t msk, int g) {
    uint64_t steps = 0;
    for (; cand != 0 || stack > 1; steps++) {
      if (cand == 0) pop(msk);
      if (cand) take<G1>(msk, g);
    }
    return steps;
  }
};

// Walk every job `next` hands out, one after the other, in ONE loop: when a
// subtree is exhausted the same loop iteration loads the next job.
// next(st) loads a job into st (st.load<G1>(...)) and returns true, or returns
// false when there is none left.
template <int LEVELS, bool G1, class Next>
NQ_HD inline void nq_flat_run(NqFlat<LEVELS>& st, Next&& next, uint32_t msk, int g) {
  st.cand = 0;
  st.stack = 0;
  for (;;) {
    if (st.cand == 0) {
      if (st.stack <= 1) {
        if (!next(st)) break;
      } else {
        st.pop(msk);
      }
    }
    if (st.cand) st.template take<G1>(msk, g);
  }
}

// ---------------------------------------------------------------------------
// Sub-jobs: a finisher job split below its root, so that a block's queue holds
// several short walks per lane instead of one long one (k_nq_x's split drain, and
// the CPU entry point nq_finish_block_cpu: the same functions, run in sequence).
//
// A job with `rem` rows left is split L = min(S, rem - 1) levels: the split
// pass enumerates the candidates of the job's first L rows (none of them the
// bottom row), counts them as tree nodes, and every candidate of the last
// enumerated row becomes one sub-job, the subtree below it. L == 0 keeps the
// job whole. A sub-job's root may be the bottom row; NqFlat::load counts it.
// ---------------------------------------------------------------------------

// Queue capacity: k_nq_x's LDS (10,424 B + 2,052 B of offsets + the queue) has
// to stay within 20,480 B, i.e. eight blocks per CU (a static_assert in the
// kernel, which 1996 entries, 20,464 B, are the largest multiple of four to
// pass); 2048 entries need fewer second rounds but leave seven blocks and
// measured slower (BASELINE.md "Split finisher jobs"), 1728 (the capacity
// before pmask was packed) 0.17 ms slower (BASELINE.md "Batched refill").
// -DGATS_NQ_QCAP=n builds another size.
#ifndef GATS_NQ_QCAP
#define GATS_NQ_QCAP 1996
#endif
inline constexpr int NQ_SPLIT_MAX = 2;                // deepest split
inline constexpr int NQ_SPLIT_DEFAULT = 2;            // GATS_NQ_SPLIT's default
inline constexpr int NQ_SPLIT_QCAP = GATS_NQ_QCAP;    // the kernel's sub-job queue [entries]
inline constexpr uint32_t NQ_SPLIT_FANOUT_MAX = 56;   // 8 * 7 sub-jobs of an 8-row job at S = 2
static_assert(NQ_SPLIT_QCAP >= static_cast<int>(NQ_SPLIT_FANOUT_MAX), "one job must fit the queue");

NQ_HD inline int nq_split_levels(int S, int rem) {
  const int l = rem - 1 < S ? rem - 1 : S;
  return l < 0 ? 0 : l;
}

// Queue entry: | ncols 2 | job reference 14 (local parent id * 32 + k) | c1 5 | c2 5 |
// ncols is the number of columns (0..2) that lead from the job to the sub-job.
NQ_HD inline uint32_t nq_sub_encode(uint32_t ref, uint32_t ncols, uint32_t c1, uint32_t c2) {
  return ncols << 24 | ref << 10 | c1 << 5 | c2;
}
NQ_HD inline uint32_t nq_sub_ref(uint32_t e) { return (e >> 10) & 0x3fffu; }
NQ_HD inline uint32_t nq_sub_ncols(uint32_t e) { return e >> 24; }
NQ_HD inline uint32_t nq_sub_c1(uint32_t e) { return (e >> 5) & 31u; }
NQ_HD inline uint32_t nq_sub_c2(uint32_t e) { return e & 31u; }

// The masks below a queen on `bit`, seen from the next row (NqFlat::load's form).
NQ_HD inline void nq_step_down(uint32_t& c, uint32_t& d1, uint32_t& d2, uint32_t bit,
                               uint32_t msk) {
  c |= bit;
  d1 = ((d1 | bit) << 1) & msk;
  d2 = (d2 | bit) >> 1;
}

// Split the job (c, d1, d2) L levels. Returns its number of sub-jobs and adds
// the candidates of the enumerated rows to `nodes`. With EMIT, emit(ncols, c1,
// c2) is called once per sub-job, c1-major in ascending columns: that order is
// the queue order. G1 == false evaluates every enumerated row's free mask g
// times; the counting pass does that, the writing pass (EMIT) only re-derives.
template <bool G1, bool EMIT, class Emit>
NQ_HD inline uint32_t nq_split_job(uint32_t c, uint32_t d1, uint32_t d2, int L, uint32_t msk,
                                   int g, uint32_t& nodes, Emit&& emit) {
  if (L == 0) {
    if (EMIT) emit(0u, 0u, 0u);
    return 1;
  }
  const uint32_t occ0 = c | d1 | d2;
  uint32_t f0 = G1 ? (~occ0 & msk) : nq_free_occ_g(occ0, msk, g);
  uint32_t n = static_cast<uint32_t>(__builtin_popcount(f0));
  nodes += n;
  if (L == 1) {
    if (EMIT)
      for (; f0; f0 &= f0 - 1) emit(1u, static_cast<uint32_t>(__builtin_ctz(f0)), 0u);
    return n;
  }
  n = 0;
  for (; f0; f0 &= f0 - 1) {
    uint32_t c1c = c, c1d1 = d1, c1d2 = d2;
    nq_step_down(c1c, c1d1, c1d2, f0 & (0u - f0), msk);
    const uint32_t occ1 = c1c | c1d1 | c1d2;
    uint32_t f1 = G1 ? (~occ1 & msk) : nq_free_occ_g(occ1, msk, g);
    n += static_cast<uint32_t>(__builtin_popcount(f1));
    if (EMIT) {
      const uint32_t c1 = static_cast<uint32_t>(__builtin_ctz(f0));
      for (; f1; f1 &= f1 - 1) emit(2u, c1, static_cast<uint32_t>(__builtin_ctz(f1)));
    }
  }
  nodes += n;
  return n;
}

// Start the walk of sub-job `e` of the job (c, d1, d2) whose first empty row
// is `row`: re-step the job's masks through the entry's columns, then load.
template <bool G1, int LEVELS>
NQ_HD inline void nq_sub_load(NqFlat<LEVELS>& w, uint32_t e, uint32_t c, uint32_t d1,
                              uint32_t d2, int row, int N, uint32_t msk, int g) {
  const uint32_t nc = nq_sub_ncols(e);
  if (nc >= 1) nq_step_down(c, d1, d2, 1u << nq_sub_c1(e), msk);
  if (nc >= 2) nq_step_down(c, d1, d2, 1u << nq_sub_c2(e), msk);
  w.template load<G1>(c, d1, d2, row + static_cast<int>(nc), N, msk, g);
}

// A parent's three masks in one 64-bit word (one LDS read): N <= 20, so each
// of cols / d1 / d2 is below 2^20.
inline constexpr int NQ_PMASK_BITS = 20;
NQ_HD inline uint64_t nq_pmask_pack(uint32_t cols, uint32_t d1, uint32_t d2) {
  return static_cast<uint64_t>(cols) | static_cast<uint64_t>(d1) << NQ_PMASK_BITS |
         static_cast<uint64_t>(d2) << (2 * NQ_PMASK_BITS);
}
NQ_HD inline void nq_pmask_unpack(uint64_t w, uint32_t& cols, uint32_t& d1, uint32_t& d2) {
  constexpr uint32_t m = (1u << NQ_PMASK_BITS) - 1u;
  cols = static_cast<uint32_t>(w) & m;
  d1 = static_cast<uint32_t>(w >> NQ_PMASK_BITS) & m;
  d2 = static_cast<uint32_t>(w >> (2 * NQ_PMASK_BITS)) & m;
}

// Job reference: local parent id * 32 + the child's COLUMN (not its slot), so
// the job's state comes from the parent's packed masks alone: the child's
// masks seen from the row below it, and that row. The parent's depth is
// popcount(cols): its board prefix is part of a permutation, so every placed
// queen has a column of its own.
NQ_HD inline uint32_t nq_job_ref(uint32_t parent, uint32_t col) { return parent * 32u + col; }
NQ_HD inline uint32_t nq_job_parent(uint32_t ref) { return ref >> 5; }
NQ_HD inline int nq_job_state(uint64_t pm, uint32_t ref, uint32_t msk, uint32_t& c, uint32_t& d1,
                              uint32_t& d2) {
  nq_pmask_unpack(pm, c, d1, d2);
  const int row = __builtin_popcount(c) + 1;
  nq_step_down(c, d1, d2, 1u << (ref & 31u), msk);
  return row;
}

// The drain's refill rule, per wave (k_nq_x's split drain and nq_finish_wave_cpu).
// A lane is idle when it has no walk (cand == 0 && stack <= 1). In every
// iteration the wave counts its idle lanes; it fetches, for all of them at
// once, when it is not drained and at least `T` of its `lanes` lanes are idle,
// or all of them are (so fewer than T entries still get started). A wave whose
// allotment [got, got + nidle) reaches the end of the round's queue is drained:
// it asks no more, runs its remaining walks to the end, and leaves when every
// lane is idle. Both results depend on wave-uniform values only.
//
// The loop ends: (1) a refill (nidle >= 1) hands out at least one entry or sets
// drained: unless got + nidle >= nsub, all nidle entries exist; (2) once a wave
// is drained no idle lane becomes active again, since only a refill loads a
// lane; (3) every step of an active lane advances its walk (a take consumes a
// candidate, a pop shortens the stack, and a walk is finite). A wave that is
// not drained and has no active lane refills (all-idle rule), so between two
// refills of a wave at least one lane steps; (1) bounds the refills by the
// queue's length + 1, (3) the steps.
NQ_HD inline bool nq_lane_idle(uint32_t cand, uint64_t stack) { return cand == 0 && stack <= 1; }
// The idle-lane count at which the wave acts: it refills, or leaves once it is
// drained. Below it the wave only steps (the kernel's inner loop).
NQ_HD inline uint32_t nq_refill_level(uint32_t lanes, uint32_t T, bool drained) {
  return drained || T > lanes ? lanes : T;
}
NQ_HD inline bool nq_refill_now(uint32_t nidle, uint32_t lanes, uint32_t T, bool drained) {
  return !drained && nidle != 0 && nidle >= nq_refill_level(lanes, T, false);
}
NQ_HD inline bool nq_wave_done(uint32_t nidle, uint32_t lanes, bool drained) {
  return drained && nidle >= nq_refill_level(lanes, lanes, true);
}
NQ_HD inline bool nq_refill_drains(uint32_t got, uint32_t nidle, uint32_t nsub) {
  return got + nidle >= nsub;
}
inline constexpr int NQ_REFILL_DEFAULT = 24;  // GATS_NQ_REFILL's default

// ---------------------------------------------------------------------------
// Wave-stack finisher (k_nq_x's stack drain and nq_finish_stack_cpu).
//
// A lane owns one ROW, not a walk: it takes that row's candidates one per
// iteration and never backtracks. A child that has children of its own in an
// inner row is pushed, as one 64-bit entry, onto a node stack that the lane's
// wave owns; a lane whose row is exhausted takes any entry off that stack, or
// a job off the block's job queue. So there is no pop path, no split pass and
// no sub-job queue, and inside a wave no lane waits on another lane's walk
// while the stack holds work.
//
// Stack entry: cols | d1 << 20 | d2 << 40 | h << 60 (nq_pmask_pack plus four
// bits). The masks are in nq_step_down's form: seen from the node's first
// empty row, below 2^N, N <= 20. h is the number of rows below that row; a
// pushed node has 1 <= h <= NQ_FLAT_LEVELS_DEV - 2.
// ---------------------------------------------------------------------------
inline constexpr int NQ_STACK_H_BITS = 4;
inline constexpr int NQ_STACK_H_SHIFT = 3 * NQ_PMASK_BITS;
static_assert(NQ_STACK_H_SHIFT + NQ_STACK_H_BITS <= 64, "a stack entry is one 64-bit word");
static_assert(NQ_FLAT_LEVELS_DEV - 1 < (1 << NQ_STACK_H_BITS), "h of a job's root fits the field");
NQ_HD inline uint64_t nq_entry_pack(uint32_t cols, uint32_t d1, uint32_t d2, uint32_t h) {
  return nq_pmask_pack(cols, d1, d2) | static_cast<uint64_t>(h) << NQ_STACK_H_SHIFT;
}
NQ_HD inline uint32_t nq_entry_unpack(uint64_t w, uint32_t& cols, uint32_t& d1, uint32_t& d2) {
  nq_pmask_unpack(w, cols, d1, d2);
  return static_cast<uint32_t>(w >> NQ_STACK_H_SHIFT) & ((1u << NQ_STACK_H_BITS) - 1u);
}

// Per-wave stack capacity [entries] of the kernel: four stacks of 312 entries
// are 9,984 B, which with the 10,424 B of the shared phases and the job
// counter keeps k_nq_x within 20,480 B of LDS, eight blocks per CU (a
// static_assert in the kernel). The largest peak scripts/nq_lane_model.py
// sees is recorded in docs/DESIGN.md; past the capacity the fallback below is
// exact, only slower. -DGATS_NQ_STACK_CAP=n builds another size.
#ifndef GATS_NQ_STACK_CAP
#define GATS_NQ_STACK_CAP 312
#endif
inline constexpr int NQ_STACK_CAP = GATS_NQ_STACK_CAP;
inline constexpr int NQ_STACK_DEFAULT = 1;  // GATS_NQ_STACK's default

// Lane state: a row (masks seen from it, rows below it) and its candidates
// that are still to be taken. cand == 0: the lane is idle.
struct NqRow {
  uint32_t cols, d1, d2, cand;
  uint32_t h;
  uint32_t tree, sol;  // 32 bits hold a block's whole queue (see k_nq_x)
};

// A job off the queue: its root's free mask is evaluated here for the first
// time (g times when G1 == false). A root in the bottom row is counted at once.
template <bool G1>
NQ_HD inline void nq_row_load_job(NqRow& r, uint32_t c, uint32_t d1, uint32_t d2, int row, int N,
                                  uint32_t msk, int g) {
  r.cols = c;
  r.d1 = d1;
  r.d2 = d2;
  r.h = static_cast<uint32_t>(N - 1 - row);
  const uint32_t occ = c | d1 | d2;
  r.cand = G1 ? (~occ & msk) : nq_free_occ_g(occ, msk, g);
  if (r.h == 0) {
    const uint32_t n = static_cast<uint32_t>(__builtin_popcount(r.cand));
    r.tree += n;
    r.sol += n;
    r.cand = 0;
  }
}

// An entry off the stack: its free mask was evaluated when it was pushed, so
// it is re-derived plainly. It is not empty (only such nodes are pushed).
NQ_HD inline void nq_row_load_entry(NqRow& r, uint64_t e, uint32_t msk) {
  r.h = nq_entry_unpack(e, r.cols, r.d1, r.d2);
  r.cand = ~(r.cols | r.d1 | r.d2) & msk;
}

// Row step (h >= 1 where cand != 0): take the lowest candidate and count it;
// count its children with a popcount when they are the bottom row. Returns
// true when the child (nc, n1, n2), whose row has h - 1 rows below it, has
// children in an inner row: the caller pushes it, or walks it (nq_row_walk).
// An idle lane (cand == 0) passes through unchanged and returns false, so a
// wave needs no branch around the step.
template <bool G1>
NQ_HD inline bool nq_row_step(NqRow& r, uint32_t msk, int g, uint32_t& nc, uint32_t& n1,
                              uint32_t& n2) {
  const bool active = r.cand != 0;
  const uint32_t bit = r.cand & (0u - r.cand);
  r.cand ^= bit;
  r.tree += active;
  nc = r.cols;
  n1 = r.d1;
  n2 = r.d2;
  nq_step_down(nc, n1, n2, bit, msk);
  const uint32_t occ = nc | n1 | n2;
  uint32_t nf = G1 ? (~occ & msk) : nq_free_occ_g(occ, msk, g);
  nf = active ? nf : 0u;
  const uint32_t n = r.h == 1 ? static_cast<uint32_t>(__builtin_popcount(nf)) : 0u;
  r.tree += n;
  r.sol += n;
  return r.h != 1 && nf != 0;
}

// Overflow fallback: the lane walks the child nq_row_step returned to the end
// with the flat walk (load, then pop / take), then returns to its row. The
// child was counted and its free mask evaluated by the row step, so the load
// is plain; the walk counts every node below it, as pushing it would.
template <bool G1>
NQ_HD inline void nq_row_walk(NqRow& r, uint32_t nc, uint32_t n1, uint32_t n2, int N, uint32_t msk,
                              int g) {
  NqFlat<NQ_FLAT_LEVELS_DEV> w;
  w.tree = 0;
  w.sol = 0;
  w.template load<true>(nc, n1, n2, N - static_cast<int>(r.h), N, msk, 1);
  w.template exhaust<G1>(msk, g);
  r.tree += w.tree;
  r.sol += w.sol;
}

// Wave rule. Wave-uniform state: sp, the stack's height; more, whether the
// block's job queue may still hold a job for this wave (cleared by the draw
// that reaches the queue's end). Every iteration the wave counts its idle
// lanes. It stops stepping and acts (nq_stack_act) when all of its `lanes`
// lanes are idle, or when at least T are and there is work for them (sp != 0
// or more). Acting it either leaves (nq_stack_done: all idle, stack empty,
// queue exhausted) or refills: the idle lanes take min(nidle, sp) entries off
// the top of the stack (nq_stack_take), and if idle lanes remain and `more`
// holds they draw job indices from the block's counter (nq_stack_draw: one per
// idle lane up to the wave's even share of the queue), as the split finisher's
// lanes draw sub-jobs (nq_refill_drains sets more = false).
// Pushes happen only while sp + lanes <= cap (nq_stack_can_push, checked once
// per iteration, before that iteration's at most `lanes` pushes, so sp <= cap
// always); otherwise the lane walks the child (nq_row_walk).
//
// The loop ends: (1) an iteration in which a lane is active takes one
// candidate off that lane's row, and every candidate is a tree node that is
// taken once, by one lane, from a row loaded once (a job is drawn by one lane,
// an entry is popped once), or inside a fallback walk, which is finite; so the
// iterations with an active lane number at most the nodes below the jobs.
// (2) An iteration with no active lane satisfies nq_stack_act, so it is the
// last one before the wave acts, and the wave steps at least once after each
// refill: iterations <= nodes + refills. (3) A refill takes at least one entry
// off the stack (sp != 0) or advances the job counter by at least one
// (sp == 0, so `more` holds, else the wave would have left); the entries taken
// are bounded by the pushes, i.e. by the nodes, and a wave draws past the
// queue's end at most once, so a block's refills are at most nodes + jobs +
// waves. Waves share only the job counter, so none waits for another.
NQ_HD inline bool nq_stack_act(uint32_t nidle, uint32_t lanes, uint32_t T, uint32_t sp, bool more) {
  return nidle >= lanes || ((sp != 0 || more) && nidle >= T);
}
NQ_HD inline bool nq_stack_done(uint32_t nidle, uint32_t lanes, uint32_t sp, bool more) {
  return nidle >= lanes && sp == 0 && !more;
}
NQ_HD inline uint32_t nq_stack_take(uint32_t nidle, uint32_t sp) { return nidle < sp ? nidle : sp; }
// Jobs one refill draws for `rem` idle lanes: at most the wave's even share of
// the block's queue, at least one. So the block's waves start with about the
// same number of jobs each (a wave cannot take work off another wave's stack),
// instead of the first waves to arrive taking `lanes` jobs each.
NQ_HD inline uint32_t nq_stack_draw(uint32_t rem, uint32_t njobs, uint32_t waves) {
  const uint32_t share = (njobs + waves - 1u) / waves;
  return rem < share ? rem : share != 0 ? share : 1u;
}
NQ_HD inline bool nq_stack_can_push(uint32_t sp, uint32_t lanes, uint32_t cap) {
  return sp + lanes <= cap;
}

// Rounds cut. off[0..njobs] are the jobs' exclusive sub-job offsets in queue
// order (off[njobs] = all of them). A round takes the longest run of jobs
// [jb, je) whose sub-jobs fit `qcap` entries; returns je (== jb only when job
// jb alone does not fit). Every thread of a block computes the same je.
template <class OffT>
NQ_HD inline uint32_t nq_round_end(const OffT* off, uint32_t jb, uint32_t njobs, uint32_t qcap) {
  const uint32_t lim = static_cast<uint32_t>(off[jb]) + qcap;
  if (static_cast<uint32_t>(off[njobs]) <= lim) return njobs;  // the usual case: one round
  uint32_t lo = jb, hi = njobs;  // off[lo] <= lim < off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (static_cast<uint32_t>(off[mid]) <= lim)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace gats
