// Public API of the single-GPU engines (implemented in engine_gpu.cpp; the
// test-only entry points at the end in engine_testing.cpp).
#pragma once
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gpu_api.hpp"
#include "nodes.hpp"
#include "search_host.hpp"

namespace gats {

int gpu_device_count();
// hipSetDevice only if this thread isn't already on `device` (the raw call
// costs ~0.8 ms on ROCm 7.2; see engine_gpu.cpp)
void set_device_cached(int device);

// Phase-2+3 engine cores (phase-1 pool supplied by the caller); used by the
// CLI engines, the distributed tier and the multi-GPU tier's devpool workers.
Result nqueens_gpu_run(Pool<NQNode>& pool, int N, int g, int m, int M, int device,
                       const std::string& mode, uint64_t tree0, uint64_t sol0,
                       double phase1_time, unsigned long long capacity);
// Extraction channel for engine-pausing inter-rank steals
// (nqueens_dist_multigpu_chpl.chpl:332-377's remote half-pool steal, as an
// explicit host protocol): the dist tier posts a request; the next readback
// of a running slice thread holding >= 2m nodes carves the BACK half of its
// device pool into `taken` and flags READY. The request LIFECYCLE is one
// atomic — IDLE -> WANTED -> CARVING -> READY -> IDLE — because a carve in
// flight must still read as "pending" to the requester: treating
// consumed-want as idle let a second request trigger a second carve that
// overwrote the first one's nodes before they were taken (nodes already off
// the donor's pool => silently lost; found via count deficit + carve log).
// `live_size` is the latest readback's pool size (victim-selection
// heuristic, approximate).
struct ExtractShare {
  static constexpr int IDLE = 0, WANTED = 1, CARVING = 2, READY = 3;
  std::atomic<int> state{IDLE};
  std::atomic<unsigned long long> live_size{0};
  std::mutex mu;  // guards taken
  std::vector<PFSPNode> taken;
};

Result pfsp_gpu_run(const PfspInstance& I, LbKind lb, Pool<PFSPNode>& pool, int m, int M,
                    int device, const std::string& mode, uint64_t tree0, uint64_t sol0,
                    int best0, double phase1_time, unsigned long long capacity,
                    std::atomic<int>* shared_best, ExtractShare* extract = nullptr);

// Multi-device devpool core: S slice threads per worker (device entry) pull
// frontier slices off ONE shared queue — an oversubscribed dynamic partition
// that load-balances across devices without pausing engines (the role of the
// reference's intra-node stealing, pfsp_multigpu_chpl.chpl:438-479) — and
// same-device threads additionally donate half-pools at readback boundaries.
// Leftover nodes (pools that drained below m) are pushed back into `pool`
// for the caller's CPU phase 3. `devices` may repeat physical devices
// (D workers on fewer GPUs). Launch/copy counters merge into `diag`.
struct DevpoolMultiOut {
  uint64_t tree = 0, sol = 0;
  int best = 0;
  std::vector<uint64_t> per_dev;  // explored tree per worker (workload shares)
};
DevpoolMultiOut nq_devpool_multi(Pool<NQNode>& pool, int N, int g, int m, int M,
                                 const std::vector<int>& devices,
                                 unsigned long long capacity, Result& diag);
DevpoolMultiOut pfsp_devpool_multi(const PfspInstance& I, Pool<PFSPNode>& pool, int lbk,
                                   int best0, int m, int M,
                                   const std::vector<int>& devices,
                                   unsigned long long capacity,
                                   std::atomic<int>* shared_best, Result& diag,
                                   ExtractShare* extract = nullptr);

// Host-side build of the packed Johnson tables: lexicographic order (per-lane
// kernels, compile-time pair map) and strength order (wave kernel; see
// PfspDevTables). Shared by the engine and multigpu table uploaders.
struct PfspPackedTables {
  std::vector<uint32_t> jp, jp_w;
  std::vector<uint8_t> p1, p2, p1_w, p2_w;
};
PfspPackedTables build_packed_johnson(const PfspInstance& I);

Result nqueens_gpu(int N, int g, int m, int M, int device, const std::string& mode,
                   unsigned long long capacity);
Result nqueens_gpu_from_pool(const std::vector<NQNode>& nodes, int N, int g, int m, int M,
                             int device, const std::string& mode,
                             unsigned long long capacity);

// br (all PFSP single-GPU entry points): branching rule "fwd" (default, the
// reference's tree), "bwd", "alt" or "minbranch" (search_host.hpp). Non-fwd
// rules run the both-directions lb1_d kernels and need lb == "lb1_d", or the
// lb12 kernels (lb == "lb12", every rule); any other combination throws
// std::invalid_argument.
Result pfsp_gpu(int inst, const std::string& lb, int ub, int m, int M, int device,
                const std::string& mode, unsigned long long capacity,
                const std::string& br = "fwd");
// Device-rooted search: the WHOLE search runs in the devpool from the root
// (no CPU phase-1 BFS, no host frontier marshaling, no CPU phase 3) — the
// devpool's m is 1 so the pool drains on device. One slice thread starts at
// the root; big searches self-parallelize because idle slice threads take
// donated half-pools once the pool crosses the donation floor (64k nodes),
// while small searches (PFSP ta0xx, few ms) never pay slicing overhead.
// Counts equal the sequential engine's at ub=1 (pruning is
// decomposition-invariant); the phase split is all-phase-2 by construction.
Result pfsp_gpu_rooted(int inst, const std::string& lb, int ub, int M, int device,
                       unsigned long long capacity, const std::string& br = "fwd");
Result nqueens_gpu_rooted(int N, int g, int M, int device, unsigned long long capacity);
Result pfsp_gpu_from_pool(const std::vector<PFSPNode>& nodes, int inst, const std::string& lb,
                          int ub, int best0, int m, int M, int device,
                          const std::string& mode, unsigned long long capacity,
                          const std::string& br = "fwd");

// engine_multi.cpp: in-process multi-GPU tier (eval = "devpool", "gpu" or
// "cpu"; capacity is the per-slice-thread device pool size in nodes, devpool
// eval only).
Result nqueens_multigpu(int N, int g, int m, int M, int D, const std::string& eval,
                        double perc = 0.5, unsigned long long capacity = 1ull << 27);
Result pfsp_multigpu(int inst, const std::string& lb, int ub, int m, int M, int D,
                     const std::string& eval, bool share_best, double perc = 0.5,
                     unsigned long long capacity = 1ull << 27,
                     const std::string& br = "fwd");  // non-fwd rules, lb12: not yet, throws

// Persistent per-rank PFSP engine: a background thread that accepts
// successive frontiers (submit), runs the devpool search on each, exposes a
// shared incumbent for mid-search RCCL UB exchange, and supports
// engine-pausing work extraction so a starving rank can steal half of a
// RUNNING rank's device pool (the reference dist tier's remote steal,
// nqueens_dist_multigpu_chpl.chpl:332-377). Device buffers come from the
// process-level cache and the thread parks between submits, so repeated
// frontier claims pay no re-arm cost.
class PfspAsyncEngine {
 public:
  // br: only "fwd" is supported yet; any other rule throws, and so does lb12
  PfspAsyncEngine(int inst, const std::string& lb, int ub, int m, int M, int device,
                  unsigned long long capacity, const std::string& br = "fwd");
  // one-shot convenience (round-1 API): submits `nodes` immediately
  PfspAsyncEngine(std::vector<PFSPNode> nodes, int inst, const std::string& lb, int ub,
                  int best0, int m, int M, int device, unsigned long long capacity,
                  const std::string& br = "fwd");
  ~PfspAsyncEngine();
  void submit(std::vector<PFSPNode> nodes, int best0);
  int best() const;
  void update_best(int b);
  bool done() const;                     // parked with nothing queued
  unsigned long long pool_size() const;  // approx live device pool + queued
  // steal protocol: request -> (engine carves at a readback, or answers
  // empty when idle) -> take. `extract_pending` = request not yet answered.
  void request_extract();
  bool extract_ready() const;
  bool extract_pending() const;
  std::vector<PFSPNode> take_extract();
  Result join();  // stop accepting work, drain, join, return accumulated

 private:
  void loop();
  void answer_want_empty();
  int inst_, ub_, m_, M_, device_;
  std::string lb_;
  unsigned long long capacity_;
  std::thread th_;
  mutable std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::pair<std::vector<PFSPNode>, int>> q_;
  bool finish_ = false;
  bool running_ = false;  // a run is executing (guarded by mu_)
  std::atomic<unsigned long long> queued_nodes_{0};
  std::atomic<int> shared_best_;
  ExtractShare ex_;
  Result result_;
  std::exception_ptr err_;
};

// Device-built phase-1 frontiers: run the devpool expand from the root with
// m=1 (each iteration pops the whole pool while it is below M — level-
// synchronous BFS) until the pool reaches `target` nodes or the search
// exhausts. Deterministic for a fixed (problem, target): every rank of the
// distributed tier builds the same frontier redundantly in ~0.1-0.5 ms where
// the CPU builder needs ~3-10 ms (pfsp_dist_multigpu_cuda.c:372-378's
// redundant-BFS trick, moved onto the GPU).
std::vector<NQNode> nq_gpu_frontier(int N, int g, size_t target, int device,
                                    uint64_t& tree, uint64_t& sol);
std::vector<PFSPNode> pfsp_gpu_frontier(const PfspInstance& I, int lbk, size_t target,
                                        int device, int best0, uint64_t& tree,
                                        uint64_t& sol, int& best_out);

// Single-iteration entry points (kernel-level tests): upload `nodes` as the
// pool, set both parity control blocks to size = nodes.size() (and `best`),
// run exactly ONE devpool iteration (expand, optional presum, gather2) with
// the engines' launch helper, and read back the next control block plus the
// first `size` pool nodes (into `nodes`). `presum` is "auto" (the engines'
// rule), "on" or "off" (groupSums pointer forced present / null). For PFSP,
// geom -1 = devpool_lbk_geom's choice, 2 / 3 force the wave-cooperative /
// per-lane lb2 kernel on any machine count. Inputs are validated on the host
// BEFORE the first HIP call (std::invalid_argument), so arbitrary bytes can
// never reach a kernel; the validate_* functions are the same checks alone.
struct DevpoolStepCtl {
  unsigned long long size, chunk, tree, sol, iters;
  int best, overflow;
};
void validate_nq_step(const std::vector<NQNode>& nodes, int N, int g, int finish,
                      unsigned long long m, unsigned long long M,
                      unsigned long long capacity, const std::string& presum);
void validate_pfsp_step(const std::vector<PFSPNode>& nodes, int inst, const std::string& lb,
                        unsigned long long m, unsigned long long M,
                        unsigned long long capacity, int geom, const std::string& presum,
                        const std::string& br = "fwd");
// The finisher knobs as a caller gives them (an NqFinishOpts that
// nq_finish_opts has not resolved yet; finish passes through):
// split: levels the finisher jobs are split (0..2), < 0 = the engine's default
// refill: idle lanes at which a wave of the split finisher refills (1..64),
// < 0 = the engine's default
// stack: 1 = the wave-stack finisher, 0 = the split one, < 0 = the engine's
// rule: the stack finisher where split < 0 too, g == 1 and nq_stack_default() is 1;
// an explicit split keeps the split kernels, and so does g > 1 (the g repeats
// are issued per wave iteration, of which the stack schedule has far fewer:
// BASELINE.md "Wave-stack finisher")
// stack_cap: the stack height per wave past which children are walked instead
// of pushed (0..NQ_STACK_CAP), < 0 = NQ_STACK_CAP
// The defaults are GATS_NQ_SPLIT / GATS_NQ_REFILL / GATS_NQ_STACK, read once.
// nq_finish_opts throws std::invalid_argument for a value outside these ranges.
int nq_split_default();
int nq_refill_default();
int nq_stack_default();
NqFinishOpts nq_finish_opts(int g, const NqFinishOpts& asked);
DevpoolStepCtl nq_devpool_step(std::vector<NQNode>& nodes, int N, int g,
                               const NqFinishOpts& finisher, unsigned long long m,
                               unsigned long long M, unsigned long long capacity,
                               const std::string& presum, int device);
DevpoolStepCtl pfsp_devpool_step(std::vector<PFSPNode>& nodes, int inst, const std::string& lb,
                                 int best, unsigned long long m, unsigned long long M,
                                 unsigned long long capacity, int geom,
                                 const std::string& presum, int device,
                                 const std::string& br = "fwd");

// Chain entry points (kernel-level tests): the step functions' arguments and
// validation, with `windows` (1..16 per-iteration launch windows) in place of
// M. The count / sol / extra / group-sum / child buffers are allocated ONCE
// for max(windows), as an engine thread sizes them for its chunk cap, and
// iteration i runs one enqueue (ctl + (i & 1) -> ctl + 1 - (i & 1)) with
// window windows[i] on one stream with no host synchronisation in between.
// After every iteration the live control block and pool[0:capacity] are
// copied device-to-device into a snapshot area; snapshot i is (the first
// `size` pool nodes, the control block) as iteration i left them. Once a
// snapshot's overflow flag is set its nodes are the un-popped prefix of the
// overflowing iteration (all that is defined from then on). presum "auto" is
// the engine threads' own per-iteration rule (the shared policy helper in
// engine_internal.hpp, with the buffers' presum sizing taken from max(windows));
// "on" / "off" force the groupSums pointer present / null every iteration.
// A window below the pool size is legal and is that iteration's pop cap.
// Everything is validated on the host before the first HIP call:
// capacity * (windows.size() + 1) <= 2^22 nodes, window * branching <= 2^31.
template <class NodeT>
struct DevpoolSnapshot {
  std::vector<NodeT> nodes;
  DevpoolStepCtl ctl;
};
std::vector<DevpoolSnapshot<NQNode>> nq_devpool_chain(
    const std::vector<NQNode>& nodes, int N, int g, const NqFinishOpts& finisher,
    unsigned long long m, const std::vector<unsigned long long>& windows,
    unsigned long long capacity, const std::string& presum, int device);
std::vector<DevpoolSnapshot<PFSPNode>> pfsp_devpool_chain(
    const std::vector<PFSPNode>& nodes, int inst, const std::string& lb, int best,
    unsigned long long m, const std::vector<unsigned long long>& windows,
    unsigned long long capacity, int geom, const std::string& presum, int device,
    const std::string& br = "fwd");

// Loop-driver entry points (driver-level tests): ONE slice goes through the
// real slice thread and loop driver (devpool_driver.hpp) —
// run_pool, the loop driver, the capacity spill, drain_spilled and the
// leftover copy — with no SliceShare, the chunk cap `chunk` taken as given
// (no --M floor, no environment variable) and graph replay allowed or not by
// `graph`. `max_batches` (0 = unlimited) ends every loop call after that many
// batches; the pool then comes back as leftovers. The driver appends to the
// trace, in order:
//   RUN    at every run_pool call: from_spill (started from a drained spill
//          chunk, not from the slice), size_before = the pool it starts with,
//          size_after = the leftover count it returned;
//   BATCH  per readback: b iterations entered on control block `parity`,
//          graph / captured = replayed / captured in this turn, size_before,
//          the control block read back, and the first ctl.size pool nodes
//          copied while the stream is idle (none once overflow is set);
//   SPILL  per spill: the sizes around it and the nodes moved to the host.
// The trace copies are not counted in the diag counters. pfsp: `best` is the
// starting incumbent; lower_at >= 0 lowers the shared incumbent to lower_to
// from the readback hook of batch lower_at (counted over the whole call), so
// that the driver's own adoption writes it to the live control block.
// Everything is validated on the host before the first HIP call (the step
// entry points' checks, capacity <= 2^22 nodes); the trace itself is capped
// at 2^22 nodes in total (std::runtime_error beyond).
//
// Share entry points (nq_devpool_share / pfsp_devpool_share): `threads` (2..4)
// real slice threads on one device over ONE SliceShare, one shared incumbent
// and one slice holding all the nodes, graph replay off as in the engines'
// multi-slice runs; one DevpoolLoopOut per thread. Thread 0 runs the slice; the
// others start once it counts as a runner and go straight to wait_for_work,
// and any of them may take and donate from then on. `donate_floor`
// (0 = donation_floor(m), else >= 2) and `await_idle_ms` (0..5000) are
// DevpoolThreadTest's knobs. Two more record kinds appear:
//   DONATE in the donor's trace, after the BATCH whose readback it follows:
//          size_before, size_after (the kept front; == size_before when the
//          offer was withdrawn), best = the offered incumbent, outcome (the
//          Donation value), and the offered nodes read from the pool's back
//          half after the carve and BEFORE the offer is published;
//   TAKE   in the thief's trace, before the RUN it starts: the received nodes
//          read from the thief's own pool after its copy, best = the received
//          incumbent.
// RUN records carry in `best` the incumbent the run's control blocks start from.
struct DevLoopRec {
  enum Kind { RUN = 0, BATCH = 1, SPILL = 2, DONATE = 3, TAKE = 4 };
  int kind = BATCH;
  int b = 0, parity = 0;
  bool graph = false, captured = false, from_spill = false;
  unsigned long long size_before = 0, size_after = 0;
  int best = 0;     // RUN / DONATE / TAKE
  int outcome = 0;  // DONATE: Donation (slice_share.hpp)
  DevpoolStepCtl ctl{};
  // BATCH: the pool; SPILL / DONATE: the moved nodes; TAKE: the received ones
  std::vector<unsigned char> nodes;
};
struct DevLoopTrace {
  std::vector<DevLoopRec> recs;
  unsigned long long traced_nodes = 0;
};
template <class NodeT>
struct DevpoolLoopOut {
  uint64_t tree = 0, sol = 0, iters = 0;
  int best = 0;
  std::vector<NodeT> leftover;
  Result diag;
  DevLoopTrace trace;
};
void validate_devpool_loop(size_t n, unsigned long long chunk, unsigned long long capacity,
                           long long max_batches);
DevpoolLoopOut<NQNode> nq_devpool_loop(const std::vector<NQNode>& nodes, int N, int g,
                                       int finish, unsigned long long m,
                                       unsigned long long chunk, unsigned long long capacity,
                                       bool graph, int max_batches, int device);
DevpoolLoopOut<PFSPNode> pfsp_devpool_loop(const std::vector<PFSPNode>& nodes, int inst,
                                           const std::string& lb, int best,
                                           unsigned long long m, unsigned long long chunk,
                                           unsigned long long capacity, bool graph,
                                           int max_batches, const std::string& br,
                                           long long lower_at, int lower_to, int device);
void validate_devpool_share(int threads, long long donate_floor, long long await_idle_ms);
std::vector<DevpoolLoopOut<NQNode>> nq_devpool_share(
    const std::vector<NQNode>& nodes, int N, int g, int finish, unsigned long long m,
    unsigned long long chunk, unsigned long long capacity, int max_batches, int threads,
    unsigned long long donate_floor, int await_idle_ms, int device);
std::vector<DevpoolLoopOut<PFSPNode>> pfsp_devpool_share(
    const std::vector<PFSPNode>& nodes, int inst, const std::string& lb, int best,
    unsigned long long m, unsigned long long chunk, unsigned long long capacity,
    int max_batches, const std::string& br, int threads, unsigned long long donate_floor,
    int await_idle_ms, int device);

std::vector<uint8_t> nq_gpu_labels(int N, int g, const std::vector<NQNode>& nodes,
                                   int device);
std::vector<int32_t> pfsp_gpu_bounds(int inst, const std::string& lb,
                                     const std::vector<PFSPNode>& nodes, int best,
                                     int device);
// lb1_d child bounds in both directions, [n * jobs] each, indexed by position
// (-1 outside a parent's unscheduled range): first = children fixed at the
// front (lb_begin), second = children fixed at the back (lb_end).
std::pair<std::vector<int32_t>, std::vector<int32_t>> pfsp_gpu_bounds_bi(
    int inst, const std::vector<PFSPNode>& nodes, int device);

// lb12 eval kernel: (dir[n], bounds[n * jobs]) in pfsp_lb12_eval's layout
// (search_host.hpp; dir 255 / bounds -1 where the kernel writes nothing).
// Nodes may have jobs fixed at the back under every rule; their structure is
// checked on the host before any HIP call (validate_lb12_nodes).
void validate_lb12_nodes(const std::vector<PFSPNode>& nodes, int jobs);
std::pair<std::vector<uint8_t>, std::vector<int32_t>> pfsp_gpu_bounds_lb12(
    int inst, const std::vector<PFSPNode>& nodes, int best, const std::string& br,
    int device);

}  // namespace gats
