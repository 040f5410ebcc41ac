// Stand-alone sanitizer run of the split finisher's CPU twins
// (src/nq_finish_cpu.hpp, i.e. the functions k_nq_x's split drain runs).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Isrc tests/helpers/nq_split_stress.cpp -o nq_split_stress
//   ./nq_split_stress            # exit status 0, "OK ..." on the last line
// A few hundred random job sets (N 4..20, 1..8 empty rows, 0..300 jobs), each
// through the block twin (split 0..2) and the wave twin (split 1..2, a random
// threshold and wave shape) under a random queue capacity, the small ones that
// cut the queue into several rounds included. Every run must count what one
// flat walk per job counts; the sanitizers watch the queue indexing, the
// offsets and the 5-bit stack shifts.
#include <cstdio>

#include "nq_finish_cpu.hpp"
#include "nq_stress_jobs.hpp"

using namespace gats;

int main() {
  std::mt19937 rng(20240611);
  auto pick = [&](int lo, int hi) { return lo + static_cast<int>(rng() % (hi - lo + 1)); };
  const int qcaps[] = {56, 57, 100, NQ_SPLIT_QCAP, 4096};
  uint64_t total = 0, rounds = 0;
  for (int round = 0; round < 400; round++) {
    const int N = pick(4, 20);
    const int njobs = round % 7 == 0 ? pick(0, 2) : pick(1, N >= 16 ? 40 : 300);
    NqJobs jobs;
    for (int i = 0; i < njobs; i++) jobs.push_back(random_job(rng, N, pick(1, N < 8 ? N : 8)));
    uint64_t tree = 0, sol = 0;
    for (const auto& j : jobs) nq_job_walk(j, N, tree, sol);
    const int g = pick(1, 2);
    const int qcap = qcaps[rng() % (sizeof(qcaps) / sizeof(qcaps[0]))];
    const int bsplit = pick(0, 2), wsplit = pick(1, 2);
    const int lanes = pick(1, 64), waves = pick(1, 4), refill = pick(1, lanes);
    const NqSplitRun b = nq_finish_block(jobs, N, g, bsplit, qcap);
    const NqSplitRun w = nq_finish_wave(jobs, N, g, wsplit, qcap, refill, lanes, waves);
    if (b.tree != tree || b.sol != sol || w.tree != tree || w.sol != sol) {
      std::printf("FAIL round %d: N %d jobs %d g %d qcap %d split %d / %d refill %d lanes %d "
                  "waves %d: tree %llu / %llu / %llu sol %llu / %llu / %llu\n",
                  round, N, njobs, g, qcap, bsplit, wsplit, refill, lanes, waves,
                  static_cast<unsigned long long>(b.tree), static_cast<unsigned long long>(w.tree),
                  static_cast<unsigned long long>(tree), static_cast<unsigned long long>(b.sol),
                  static_cast<unsigned long long>(w.sol), static_cast<unsigned long long>(sol));
      return 1;
    }
    total += tree;
    rounds += b.rounds + w.rounds;
  }
  std::printf("OK 400 job sets, %llu nodes, %llu queue rounds\n",
              static_cast<unsigned long long>(total), static_cast<unsigned long long>(rounds));
  return 0;
}
