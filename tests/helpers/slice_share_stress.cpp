// Stress run of the half-pool donation handshake (src/slice_share.hpp) on
// plain threads, meant for the thread sanitizer:
//
//   c++ -std=c++17 -O1 -g -fsanitize=thread -pthread -Isrc \
//       tests/helpers/slice_share_stress.cpp -o slice_share_stress
//   ./slice_share_stress            # exit status 0, "OK ..." on the last line
//
// (clang's runtime, or a gcc new enough to intercept pthread_cond_clockwait:
// gcc 11's does not see the unlock inside condition_variable::wait_for and
// reports "double lock of a mutex" and races between accesses that hold it.)
//
// Each round, 2 to 4 threads play slice threads over fake pools (one
// std::vector per thread, standing in for a thread's device pool). Thread 0
// starts with `roots` nodes; a node of generation g > 0 pushes two children
// of generation g - 1 when it is popped. After every "iteration" (a pop of up
// to `chunk` nodes from the back) the thread runs the donor side exactly as
// devpool_thread does at a readback; drained threads wait, copy the offered
// range out of the donor's pool (the donor is blocked meanwhile: that copy
// is the data race the handshake has to exclude) and ack. At the end of a
// round every node id must have been popped exactly once, by whichever
// thread. Rounds repeat until a few thousand offers were taken.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "slice_share.hpp"

using namespace gats;

namespace {

struct Node {
  int id;
  int gen;
};

struct Round {
  int threads, roots, gen, chunk;
  unsigned long long floor_sz;
  SliceShare share;
  std::atomic<int> next_id{0};
  std::atomic<int> best{1000000};
  std::atomic<long> taken{0}, offered{0};
  std::vector<std::vector<Node>> pools;
  std::vector<std::vector<int>> popped;  // ids, per thread
  size_t total = 0;

  Round(int T, int roots_, int gen_, int chunk_, unsigned long long floor_)
      : threads(T), roots(roots_), gen(gen_), chunk(chunk_), floor_sz(floor_) {
    total = static_cast<size_t>(roots) * ((size_t{2} << gen) - 1);
    pools.assign(T, std::vector<Node>(total));
    popped.resize(T);
  }

  void run(int t, unsigned long long size, int init_best) {
    std::vector<Node>& pool = pools[t];
    unsigned long long live = size;  // the "device" copy of the size
    int my_best = init_best;
    RunnerScope runner(&share);
    while (size > 0) {
      // one iteration: pop from the back, push the children above what is left
      const unsigned long long n = size < static_cast<unsigned long long>(chunk) ? size : chunk;
      std::vector<Node> parents(pool.begin() + (size - n), pool.begin() + size);
      size -= n;
      for (const Node& p : parents) {
        popped[t].push_back(p.id);
        if (p.id < my_best) my_best = p.id;
        if (p.gen > 0)
          for (int c = 0; c < 2; c++) pool[size++] = {next_id.fetch_add(1), p.gen - 1};
      }
      live = size;
      // the readback boundary
      const Donation d = donate_if_wanted(
          &share, size, my_best, false, pool.data(), floor_sz,
          [&](unsigned long long x) { live = x; }, std::chrono::seconds(10));
      if (d != Donation::NONE) offered++;
      if (d == Donation::TAKEN) taken++;
      if (live != size) {
        std::fprintf(stderr, "FAIL: live size %llu, host size %llu\n", live, size);
        std::exit(1);
      }
    }
  }

  void worker(int t) {
    if (t == 0) {
      for (int i = 0; i < roots; i++) pools[0][i] = {next_id.fetch_add(1), gen};
      run(0, roots, best.load());
    }
    StolenWork w;
    while (wait_for_work(share, w)) {
      const Node* src = static_cast<const Node*>(w.src);
      for (unsigned long long i = 0; i < w.n; i++) pools[t][i] = src[i];
      ack_taken(share);
      run(t, w.n, w.best);
    }
  }

  bool go() {
    std::vector<std::thread> ts;
    // thread 0 first, so that the others find a runner
    ts.emplace_back([this] { worker(0); });
    for (int t = 1; t < threads; t++) ts.emplace_back([this, t] { worker(t); });
    for (auto& th : ts) th.join();
    std::vector<int> seen(total, 0);
    size_t count = 0;
    for (const auto& ids : popped)
      for (int id : ids) {
        if (id < 0 || static_cast<size_t>(id) >= total) return false;
        seen[id]++;
        count++;
      }
    if (count != total || static_cast<size_t>(next_id.load()) != total) return false;
    for (int s : seen)
      if (s != 1) return false;
    return true;
  }
};

}  // namespace

int main(int argc, char** argv) {
  const long want = argc > 1 ? std::atol(argv[1]) : 3000;
  long taken = 0, offered = 0, rounds = 0;
  for (; rounds < 20000 && taken < want; rounds++) {
    const int T = 2 + static_cast<int>(rounds % 3);
    // odd and even pools, floors at and above one chunk
    Round r(T, /*roots=*/33 + static_cast<int>(rounds % 4), /*gen=*/6,
            /*chunk=*/4 + static_cast<int>(rounds % 5), /*floor=*/8 + (rounds % 7));
    if (!r.go()) {
      std::fprintf(stderr, "FAIL: round %ld: a node was lost or popped twice\n", rounds);
      return 1;
    }
    taken += r.taken.load();
    offered += r.offered.load();
  }
  if (taken < want) {
    std::fprintf(stderr, "FAIL: only %ld offers taken in %ld rounds\n", taken, rounds);
    return 1;
  }
  std::printf("OK rounds=%ld offers=%ld taken=%ld\n", rounds, offered, taken);
  return 0;
}
