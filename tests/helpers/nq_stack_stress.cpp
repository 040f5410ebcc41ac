// Stand-alone sanitizer run of the wave-stack finisher's CPU twin
// (src/nq_finish_cpu.hpp, i.e. the functions k_nq_x's stack drain runs).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Isrc tests/helpers/nq_stack_stress.cpp -o nq_stack_stress
//   ./nq_stack_stress            # exit status 0, "OK ..." on the last line
// A few hundred random job sets (N 4..20, 1..8 empty rows, 0..300 jobs), each
// under a random threshold, wave shape and stack capacity, the small capacities
// that force the fallback included. Every run must count what one flat walk
// per job counts and keep its stacks within the capacity; the sanitizers watch
// the stack indexing, the shifts and the entry codec.
#include <cstdio>

#include "nq_finish_cpu.hpp"
#include "nq_stress_jobs.hpp"

using namespace gats;

int main() {
  std::mt19937 rng(20240117);
  auto pick = [&](int lo, int hi) { return lo + static_cast<int>(rng() % (hi - lo + 1)); };
  const int caps[] = {0, 1, 63, 64, 65, 100, 130, NQ_STACK_CAP, 4096};
  uint64_t total = 0, fallbacks = 0;
  for (int round = 0; round < 400; round++) {
    const int N = pick(4, 20);
    const int njobs = round % 7 == 0 ? pick(0, 2) : pick(1, N >= 16 ? 40 : 300);
    std::vector<std::array<uint32_t, 4>> jobs;
    for (int i = 0; i < njobs; i++) jobs.push_back(random_job(rng, N, pick(1, N < 8 ? N : 8)));
    uint64_t tree = 0, sol = 0;
    for (const auto& j : jobs) nq_job_walk(j, N, tree, sol);
    const int lanes = round % 3 == 0 ? pick(1, 64) : 64;
    const int waves = pick(1, 4), T = pick(1, 64), g = pick(1, 2);
    const int cap = caps[rng() % (sizeof(caps) / sizeof(caps[0]))];
    const NqStackRun r = nq_finish_stack(jobs, N, g, T, waves, lanes, cap);
    uint32_t peak = 0;
    for (uint32_t p : r.peak_sp) peak = p > peak ? p : peak;
    if (r.tree != tree || r.sol != sol || peak > static_cast<uint32_t>(cap)) {
      std::printf("FAIL round %d: N %d jobs %d g %d T %d waves %d lanes %d cap %d: "
                  "tree %llu / %llu sol %llu / %llu peak %u\n",
                  round, N, njobs, g, T, waves, lanes, cap,
                  static_cast<unsigned long long>(r.tree), static_cast<unsigned long long>(tree),
                  static_cast<unsigned long long>(r.sol), static_cast<unsigned long long>(sol),
                  peak);
      return 1;
    }
    total += tree;
    fallbacks += r.fallbacks;
  }
  std::printf("OK 400 job sets, %llu nodes, %llu fallback walks\n",
              static_cast<unsigned long long>(total), static_cast<unsigned long long>(fallbacks));
  return 0;
}
