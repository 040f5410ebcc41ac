// CPU twins of k_nq_x's finisher drains for one block's job queue, written
// with the kernel's own functions (nq_finish.hpp) run in sequence. Plain C++
// (no Python, no HIP), so a stand-alone program can run them under a sanitizer
// (tests/helpers/nq_split_stress.cpp, nq_stack_stress.cpp); bindings.cpp only
// turns the result structs into tuples.
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "nq_finish.hpp"

namespace gats {

// (cols, d1, d2, row) states as nq_finish_count_cpu takes them.
using NqJobs = std::vector<std::array<uint32_t, 4>>;

// What every twin asks of its block: each entry point adds only its own checks.
inline void nq_validate_jobs(const NqJobs& jobs, int N, int g) {
  if (N < 1 || N > 20) throw std::invalid_argument("N must be in 1..20");
  if (g < 1) throw std::invalid_argument("g must be >= 1");
  if (jobs.size() > 1024) throw std::invalid_argument("a block holds at most 1024 jobs");
  for (const auto& j : jobs) {
    const int rows = N - static_cast<int>(j[3]);
    if (rows < 1 || rows > NQ_FLAT_LEVELS_DEV)
      throw std::invalid_argument("every job needs 1..8 empty rows");
    if ((j[0] | j[1] | j[2]) >> N) throw std::invalid_argument("mask bits at or above column N");
  }
}

// The nodes below job j, by one flat walk: the twins' bounds and the stress
// programs' expected counts.
inline void nq_job_walk(const std::array<uint32_t, 4>& j, int N, uint64_t& tree, uint64_t& sol) {
  NqFlat<NQ_FLAT_LEVELS_DEV> w;
  w.tree = w.sol = 0;
  const uint32_t msk = (1u << N) - 1u;
  w.load<true>(j[0], j[1], j[2], static_cast<int>(j[3]), N, msk, 1);
  w.exhaust<true>(msk, 1);
  tree += w.tree;
  sol += w.sol;
}

// ---------------------------------------------------------------------------
// Split finisher (k_nq_x's split drain): count and rank the sub-jobs, cut the
// queue into rounds of at most `qcap` entries, write each round's entries and
// drain them.
// ---------------------------------------------------------------------------
struct NqSplitRun {
  uint64_t tree = 0, sol = 0;
  uint32_t entries = 0, rounds = 0;
  uint64_t refills = 0, steps = 0;  // the wave twin's; steps = the waves' loop iterations
};

template <bool G1>
struct NqSplitBlock {
  const NqJobs& jobs;
  int N, g, split;
  uint32_t qcap, msk, njobs;
  std::vector<uint32_t> off;   // the jobs' exclusive sub-job offsets, off[njobs] = all
  std::vector<uint32_t> subq;  // the current round's entries
  uint32_t nodes = 0;          // candidates of the enumerated rows

  int levels(uint32_t q) const { return nq_split_levels(split, N - static_cast<int>(jobs[q][3])); }

  // The count pass (the kernel's phase C1).
  NqSplitBlock(const NqJobs& jobs_, int N_, int g_, int split_, uint32_t qcap_)
      : jobs(jobs_), N(N_), g(g_), split(split_), qcap(qcap_), msk((1u << N_) - 1u),
        njobs(static_cast<uint32_t>(jobs_.size())), off(njobs + 1, 0), subq(qcap_) {
    for (uint32_t q = 0; q < njobs; q++) {
      const uint32_t n = nq_split_job<G1, false>(jobs[q][0], jobs[q][1], jobs[q][2], levels(q),
                                                 msk, g, nodes, [](uint32_t, uint32_t, uint32_t) {});
      if (n > qcap)
        throw std::invalid_argument("qcap " + std::to_string(qcap) + " is below the " +
                                    std::to_string(n) + " sub-jobs of job " + std::to_string(q));
      off[q + 1] = off[q] + n;
    }
  }

  // Cut the round that starts at job jb and write its entries into subq.
  // Returns its end job; nsub = its number of entries.
  uint32_t write_round(uint32_t jb, uint32_t& nsub) {
    const uint32_t je = nq_round_end(off.data(), jb, njobs, qcap);
    nsub = off[je] - off[jb];
    for (uint32_t q = jb; q < je; q++) {
      uint32_t w = off[q] - off[jb], unused = 0;
      nq_split_job<true, true>(jobs[q][0], jobs[q][1], jobs[q][2], levels(q), msk, 1, unused,
                               [&](uint32_t nc, uint32_t c1, uint32_t c2) {
                                 subq[w++] = nq_sub_encode(q, nc, c1, c2);
                               });
    }
    return je;
  }

  void load(NqFlat<NQ_FLAT_LEVELS_DEV>& w, uint32_t e) const {
    const auto& j = jobs[nq_sub_ref(e)];
    nq_sub_load<G1>(w, e, j[0], j[1], j[2], static_cast<int>(j[3]), N, msk, g);
  }
};

// One flat loop drains every round.
template <bool G1>
inline NqSplitRun nq_finish_block_run(const NqJobs& jobs, int N, int g, int split, uint32_t qcap) {
  NqSplitBlock<G1> b(jobs, N, g, split, qcap);
  NqFlat<NQ_FLAT_LEVELS_DEV> st;
  st.tree = 0;
  st.sol = 0;
  NqSplitRun out;
  for (uint32_t jb = 0, nsub; jb < b.njobs; out.rounds++) {
    jb = b.write_round(jb, nsub);
    uint32_t head = 0;
    nq_flat_run<NQ_FLAT_LEVELS_DEV, G1>(
        st,
        [&](NqFlat<NQ_FLAT_LEVELS_DEV>& w) {
          if (head >= nsub) return false;
          b.load(w, b.subq[head++]);
          return true;
        },
        b.msk, g);
  }
  out.tree = static_cast<uint64_t>(b.nodes) + st.tree;
  out.sol = st.sol;
  out.entries = b.off[b.njobs];
  return out;
}

inline NqSplitRun nq_finish_block(const NqJobs& jobs, int N, int g, int split, long long qcap) {
  nq_validate_jobs(jobs, N, g);
  if (split < 0 || split > NQ_SPLIT_MAX) throw std::invalid_argument("split must be in 0..2");
  if (qcap < 1 || qcap > (1 << 20)) throw std::invalid_argument("qcap must be in 1..2^20");
  return g == 1 ? nq_finish_block_run<true>(jobs, N, g, split, static_cast<uint32_t>(qcap))
                : nq_finish_block_run<false>(jobs, N, g, split, static_cast<uint32_t>(qcap));
}

// The drain as the kernel's waves run it: `waves` x `lanes` flat walks stepped
// in lockstep, every wave deciding with the kernel's own rule (nq_refill_now /
// nq_refill_drains / nq_wave_done) when its idle lanes fetch, the waves taking
// turns, one loop iteration each, on one queue head. Every iteration but a
// wave's last either steps an active lane or is a refill, and the lane steps of
// a round sum to the walk lengths of its sub-jobs whichever lane walks them, so
// steps <= walk lengths + refills: the loop throws when it passes that bound
// instead of spinning.
template <bool G1>
inline NqSplitRun nq_finish_wave_run(const NqJobs& jobs, int N, int g, int split, uint32_t qcap,
                                     uint32_t T, uint32_t lanes, uint32_t waves) {
  using Flat = NqFlat<NQ_FLAT_LEVELS_DEV>;
  NqSplitBlock<G1> b(jobs, N, g, split, qcap);
  const uint32_t msk = b.msk;
  auto step = [&](Flat& w) {  // the kernel's loop body below the fetch
    if (w.cand == 0 && w.stack > 1) w.pop(msk);
    if (w.cand) w.template take<G1>(msk, g);
  };
  std::vector<Flat> st(static_cast<size_t>(waves) * lanes);
  for (auto& w : st) w.tree = w.sol = 0;
  NqSplitRun out;
  for (uint32_t jb = 0, nsub; jb < b.njobs; out.rounds++) {
    jb = b.write_round(jb, nsub);
    uint64_t walk = 0;  // the round's bound: one lane walks every entry
    for (uint32_t i = 0; i < nsub; i++) {
      Flat w;
      w.tree = w.sol = 0;
      b.load(w, b.subq[i]);
      walk += w.template exhaust<G1>(msk, g);
    }
    const uint64_t steps0 = out.steps, refills0 = out.refills;
    uint32_t head = 0, running = waves;
    std::vector<char> drained(waves, 0), done(waves, 0);
    for (auto& w : st) w.cand = 0, w.stack = 0;
    while (running) {
      for (uint32_t v = 0; v < waves; v++) {
        if (done[v]) continue;
        Flat* wl = &st[static_cast<size_t>(v) * lanes];
        uint32_t nidle = 0;
        for (uint32_t l = 0; l < lanes; l++) nidle += nq_lane_idle(wl[l].cand, wl[l].stack);
        if (nq_refill_now(nidle, lanes, T, drained[v] != 0)) {
          const uint32_t got = head;
          head += nidle;
          out.refills++;
          drained[v] = nq_refill_drains(got, nidle, nsub);
          uint32_t qi = got;
          for (uint32_t l = 0; l < lanes; l++)
            if (nq_lane_idle(wl[l].cand, wl[l].stack)) {
              if (qi < nsub) b.load(wl[l], b.subq[qi]);
              qi++;
            }
        } else if (nq_wave_done(nidle, lanes, drained[v] != 0)) {
          done[v] = 1;
          running--;
          continue;
        }
        for (uint32_t l = 0; l < lanes; l++) step(wl[l]);
        out.steps++;
        if (out.steps - steps0 > walk + (out.refills - refills0))
          throw std::runtime_error("the drain passed its bound of " + std::to_string(walk) +
                                   " lane steps + " + std::to_string(out.refills - refills0) +
                                   " refills in round " + std::to_string(out.rounds));
      }
    }
  }
  out.tree = b.nodes;
  for (const auto& w : st) out.tree += w.tree, out.sol += w.sol;
  out.entries = b.off[b.njobs];
  return out;
}

inline NqSplitRun nq_finish_wave(const NqJobs& jobs, int N, int g, int split, long long qcap,
                                 int refill, int lanes, int waves) {
  nq_validate_jobs(jobs, N, g);
  if (split < 1 || split > NQ_SPLIT_MAX) throw std::invalid_argument("split must be in 1..2");
  if (qcap < 1 || qcap > (1 << 20)) throw std::invalid_argument("qcap must be in 1..2^20");
  if (lanes < 1 || lanes > 64) throw std::invalid_argument("lanes must be in 1..64");
  if (waves < 1 || waves > 16) throw std::invalid_argument("waves must be in 1..16");
  // a threshold above the wave's width is rejected, not clamped: it could only
  // ever act as the all-idle rule, which `refill == lanes` already names
  if (refill < 1 || refill > lanes) throw std::invalid_argument("refill must be in 1..lanes");
  const auto q = static_cast<uint32_t>(qcap);
  const auto T = static_cast<uint32_t>(refill);
  const auto L = static_cast<uint32_t>(lanes), W = static_cast<uint32_t>(waves);
  return g == 1 ? nq_finish_wave_run<true>(jobs, N, g, split, q, T, L, W)
                : nq_finish_wave_run<false>(jobs, N, g, split, q, T, L, W);
}

// ---------------------------------------------------------------------------
// Wave-stack finisher (k_nq_x's stack drain): `waves` x `lanes` rows stepped in
// lockstep with the kernel's own functions (nq_row_step, nq_stack_act / done /
// take / can_push, nq_row_walk), the waves taking turns, one loop iteration
// each, on one job counter.
// ---------------------------------------------------------------------------
struct NqStackRun {
  uint64_t tree = 0, sol = 0;
  std::vector<uint64_t> iters;    // loop iterations per wave
  std::vector<uint32_t> peak_sp;  // highest stack height per wave
  uint64_t fallbacks = 0;         // children walked because the stack was full
  uint64_t refills = 0;
};

// cap: entries per wave's stack. Throws when the loop passes its bound
// (nq_stack_act's argument: iterations <= nodes + refills, refills <= nodes +
// jobs + waves) instead of spinning.
template <bool G1>
inline NqStackRun nq_finish_stack_run(const NqJobs& jobs, int N, int g, uint32_t T, uint32_t waves,
                                      uint32_t lanes, uint32_t cap) {
  const uint32_t msk = (1u << N) - 1u;
  const uint32_t njobs = static_cast<uint32_t>(jobs.size());
  uint64_t nodes = 0, unused = 0;  // the bound: one flat walk over every job
  for (const auto& j : jobs) nq_job_walk(j, N, nodes, unused);
  const uint64_t bound = 2 * nodes + njobs + waves;

  NqStackRun out;
  out.iters.assign(waves, 0);
  out.peak_sp.assign(waves, 0);
  std::vector<NqRow> st(static_cast<size_t>(waves) * lanes);
  for (auto& r : st) r = NqRow{0, 0, 0, 0, 0, 0, 0};
  std::vector<std::vector<uint64_t>> stk(waves, std::vector<uint64_t>(cap));
  std::vector<uint32_t> sp(waves, 0);
  std::vector<char> more(waves, 1), done(waves, 0);
  uint32_t jhead = 0, running = waves;
  uint64_t total = 0;
  while (running) {
    for (uint32_t v = 0; v < waves; v++) {
      if (done[v]) continue;
      NqRow* wl = &st[static_cast<size_t>(v) * lanes];
      uint32_t nidle = 0;
      for (uint32_t l = 0; l < lanes; l++) nidle += wl[l].cand == 0;
      // a wave starts all idle, so its first turn acts, as the kernel's does
      if (nq_stack_act(nidle, lanes, T, sp[v], more[v] != 0)) {
        if (nq_stack_done(nidle, lanes, sp[v], more[v] != 0)) {
          done[v] = 1;
          running--;
          continue;
        }
        out.refills++;
        const uint32_t take = nq_stack_take(nidle, sp[v]);
        const uint32_t rem = nq_stack_draw(nidle - take, njobs, waves);
        uint32_t got = 0;
        const bool draw = more[v] && nidle > take;
        if (draw) {
          got = jhead;
          jhead += rem;
          more[v] = !nq_refill_drains(got, rem, njobs);
        }
        uint32_t rank = 0;
        for (uint32_t l = 0; l < lanes; l++) {
          if (wl[l].cand != 0) continue;
          if (rank < take) {
            nq_row_load_entry(wl[l], stk[v][sp[v] - 1 - rank], msk);
          } else if (draw) {
            const uint32_t qi = got + rank - take;
            if (rank - take < rem && qi < njobs) {
              const auto& j = jobs[qi];
              nq_row_load_job<G1>(wl[l], j[0], j[1], j[2], static_cast<int>(j[3]), N, msk, g);
            }
          }
          rank++;
        }
        sp[v] -= take;
      }
      const bool can = nq_stack_can_push(sp[v], lanes, cap);
      uint32_t pushed = 0;
      for (uint32_t l = 0; l < lanes; l++) {
        NqRow& r = wl[l];
        uint32_t nc, n1, n2;
        if (!nq_row_step<G1>(r, msk, g, nc, n1, n2)) continue;
        if (can) {
          stk[v].at(sp[v] + pushed++) = nq_entry_pack(nc, n1, n2, r.h - 1);
        } else {
          nq_row_walk<G1>(r, nc, n1, n2, N, msk, g);
          out.fallbacks++;
        }
      }
      sp[v] += pushed;
      if (sp[v] > out.peak_sp[v]) out.peak_sp[v] = sp[v];
      out.iters[v]++;
      if (++total > bound)
        throw std::runtime_error("the stack finisher passed its bound of " +
                                 std::to_string(bound) + " iterations");
    }
  }
  for (const auto& r : st) out.tree += r.tree, out.sol += r.sol;
  return out;
}

inline NqStackRun nq_finish_stack(const NqJobs& jobs, int N, int g, int T, int waves, int lanes,
                                  long long cap) {
  nq_validate_jobs(jobs, N, g);
  if (lanes < 1 || lanes > 64) throw std::invalid_argument("lanes must be in 1..64");
  if (waves < 1 || waves > 16) throw std::invalid_argument("waves must be in 1..16");
  if (T < 1 || T > 64) throw std::invalid_argument("T must be in 1..64");
  if (cap < 0 || cap > (1 << 20)) throw std::invalid_argument("cap must be in 0..2^20");
  const auto Tu = static_cast<uint32_t>(T), W = static_cast<uint32_t>(waves);
  const auto L = static_cast<uint32_t>(lanes), C = static_cast<uint32_t>(cap);
  return g == 1 ? nq_finish_stack_run<true>(jobs, N, g, Tu, W, L, C)
                : nq_finish_stack_run<false>(jobs, N, g, Tu, W, L, C);
}

}  // namespace gats
