#pragma once
// The devpool loop driver's decisions alone, with no HIP in them: how long the
// next batch is, when the pool spills instead, when a batch may be captured
// into a graph or replayed from one, and the chunk bound of the blind
// iterations. run_devpool_loop (devpool_driver.hpp) asks these functions and
// keeps the HIP actions; tests/test_devpool_loop_plan.py compares them on the
// CPU with the rules as tests/helpers/devpool_loop_oracle.py states them. A
// host compiler parses this header alone:
//
//   echo '#include "devpool_loop_plan.hpp"' > plan_alone.cpp
//   c++ -std=c++17 -fsyntax-only -Isrc plan_alone.cpp
#include <cstdlib>

namespace gats {

constexpr int LOOP_BATCH = 16;         // iterations per full batch
constexpr int LOOP_EAGER_BATCHES = 4;  // batches before a graph may be captured
constexpr unsigned long long LOOP_SMALL_POOL = 4096;  // below it batches are 2 long

// What the plan depends on of a loop's configuration (DevLoopCfg adds the rest).
struct DevLoopShape {
  unsigned long long m = 1;          // loop exits when size < m
  unsigned long long growth = 0;     // worst-case net pool growth per iteration
  unsigned long long capacity = 0;   // pool capacity in nodes
  unsigned long long stop_size = 0;  // frontier builder: stop once size >= this
  int per = 1;                       // max children per node (grid-bound growth)
};

// Iterations of the next batch, or 0: spill now. `size` is the pool size at the
// last readback, `batches` the batches done so far. Capacity-aware: never
// launch more iterations than worst-case growth allows; spill when even one
// iteration might not fit. Small pools use short batches so the chunk bound
// (and with it the launch grids) is re-tightened every couple of iterations.
inline int plan_batch(const DevLoopShape& c, unsigned long long size, int batches,
                      bool can_spill) {
  int b = (c.stop_size > 0) ? 1 : LOOP_BATCH;
  if (c.per > 1 && size < LOOP_SMALL_POOL && b > 2) b = 2;
  if (c.growth == 0 || c.capacity == 0) return b;
  const unsigned long long room = c.capacity > size ? c.capacity - size : 0;
  const unsigned long long bmax = room / c.growth;
  if (bmax == 0 && can_spill && size >= 4 * c.m && batches > 0) return 0;
  // worst-case doesn't fit but the actual child count usually does; run one
  // iteration — the gather kernel's exact-fit guard flags a REAL overflow,
  // which is fatal (the iteration state is torn)
  if (bmax == 0) return 1;
  return bmax < static_cast<unsigned long long>(b) ? static_cast<int>(bmax) : b;
}

// GATS_NO_GRAPH=1 falls back to eager launches (rocprofv3 crashes tracing
// hipGraph replays on ROCm 7.2; eager mode gives identical results).
// multi-slice engines pass allow_graph=false: ROCm 7.2 stream capture races
// with concurrent async work from the other slice threads no matter the
// capture mode; with >1 slice in flight the host launch latency is hidden
// by the other slices anyway
inline bool graphs_allowed(bool allow_graph, unsigned long long stop_size) {
  return allow_graph && stop_size == 0 && std::getenv("GATS_NO_GRAPH") == nullptr;
}

// How a batch of b iterations entered on parity `par` is launched. Graph
// capture is LAZY: instantiation costs a few ms, which dominates small
// searches (PFSP ta0xx finish in <10 ms), so the first LOOP_EAGER_BATCHES
// batches run eager and the graph is built only if the search is still going.
// CAPTURE means "try": the batch is replayed if an exec came of it, eager if not.
enum class GraphStep { EAGER, CAPTURE, REPLAY };
inline GraphStep plan_graph(bool allowed, int batches, bool have_exec, int b, int par) {
  if (b != LOOP_BATCH || par != 0) return GraphStep::EAGER;
  if (have_exec) return GraphStep::REPLAY;
  return allowed && batches >= LOOP_EAGER_BATCHES ? GraphStep::CAPTURE : GraphStep::EAGER;
}

// chunk BOUND handed to each launch so its grid covers only the pool that
// can possibly exist: exact at readbacks, multiplied by the branching
// factor per blind iteration. Full-size grids for tiny chunks were the
// small-search floor (an 80-node ta019 tree dispatched 15k-block lb2
// grids: 1.53 ms; the engine infra itself costs 0.025 ms).
inline unsigned long long first_chunk_bound(unsigned long long size) { return size ? size : 1; }
inline unsigned long long next_chunk_bound(unsigned long long bound, int per) {
  return bound < (1ull << 40) ? bound * (per > 1 ? per : 2) : bound;
}

}  // namespace gats
