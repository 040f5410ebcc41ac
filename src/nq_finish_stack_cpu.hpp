// CPU run of k_nq_x's wave-stack finisher for one block: `waves` x `lanes`
// rows stepped in lockstep with the kernel's own functions (nq_finish.hpp:
// nq_row_step, nq_stack_act / done / take / can_push, nq_row_walk), the waves
// taking turns, one loop iteration each, on one job counter. Plain C++ (no
// Python, no HIP), so a stand-alone program can run it under a sanitizer.
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "nq_finish.hpp"

namespace gats {

struct NqStackRun {
  uint64_t tree = 0, sol = 0;
  std::vector<uint64_t> iters;    // loop iterations per wave
  std::vector<uint32_t> peak_sp;  // highest stack height per wave
  uint64_t fallbacks = 0;         // children walked because the stack was full
  uint64_t refills = 0;
};

// jobs: (cols, d1, d2, row) states as nq_finish_count_cpu takes them, 1..8
// empty rows each. cap: entries per wave's stack. Throws when the loop passes
// its bound (nq_stack_act's argument: iterations <= nodes + refills, refills
// <= nodes + jobs + waves) instead of spinning.
template <bool G1>
inline NqStackRun nq_finish_stack_run(const std::vector<std::array<uint32_t, 4>>& jobs, int N,
                                      int g, uint32_t T, uint32_t waves, uint32_t lanes,
                                      uint32_t cap) {
  const uint32_t msk = (1u << N) - 1u;
  const uint32_t njobs = static_cast<uint32_t>(jobs.size());
  uint64_t nodes = 0;  // the bound: one flat walk over every job
  for (const auto& j : jobs) {
    NqFlat<NQ_FLAT_LEVELS_DEV> w;
    w.tree = w.sol = 0;
    w.template load<true>(j[0], j[1], j[2], static_cast<int>(j[3]), N, msk, 1);
    while (w.cand != 0 || w.stack > 1) {
      if (w.cand == 0) w.pop(msk);
      if (w.cand) w.template take<true>(msk, 1);
    }
    nodes += w.tree;
  }
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

inline NqStackRun nq_finish_stack(const std::vector<std::array<uint32_t, 4>>& jobs, int N, int g,
                                  int T, int waves, int lanes, long long cap) {
  if (N < 1 || N > 20) throw std::invalid_argument("N must be in 1..20");
  if (g < 1) throw std::invalid_argument("g must be >= 1");
  if (lanes < 1 || lanes > 64) throw std::invalid_argument("lanes must be in 1..64");
  if (waves < 1 || waves > 16) throw std::invalid_argument("waves must be in 1..16");
  if (T < 1 || T > 64) throw std::invalid_argument("T must be in 1..64");
  if (cap < 0 || cap > (1 << 20)) throw std::invalid_argument("cap must be in 0..2^20");
  if (jobs.size() > 1024) throw std::invalid_argument("a block holds at most 1024 jobs");
  for (const auto& j : jobs) {
    const int rows = N - static_cast<int>(j[3]);
    if (rows < 1 || rows > NQ_FLAT_LEVELS_DEV)
      throw std::invalid_argument("every job needs 1..8 empty rows");
    if ((j[0] | j[1] | j[2]) >> N) throw std::invalid_argument("mask bits at or above column N");
  }
  const auto Tu = static_cast<uint32_t>(T), W = static_cast<uint32_t>(waves);
  const auto L = static_cast<uint32_t>(lanes), C = static_cast<uint32_t>(cap);
  return g == 1 ? nq_finish_stack_run<true>(jobs, N, g, Tu, W, L, C)
                : nq_finish_stack_run<false>(jobs, N, g, Tu, W, L, C);
}

}  // namespace gats
