// Test-only entry points of the GPU engines (declared in engine_gpu.hpp): host
// validation, single devpool iterations and iteration chains built from the
// engines' own buffer set, problem descriptors and launch policy
// (engine_internal.hpp), traced runs of the real slice thread and loop driver
// (devpool_driver.hpp), and the eval-only kernels. No engine runs through
// this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "devpool_driver.hpp"
#include "engine_gpu.hpp"
#include "engine_internal.hpp"
#include "gpu_api.hpp"
#include "nq_finish.hpp"
#include "search_host.hpp"
#include "taillard.hpp"

namespace gats {

// ---------------------------------------------------------------------------
// Single-iteration entry points: upload a chosen pool, run exactly ONE
// devpool iteration through the problem descriptor's enqueue(), read the
// pool and the next control block back. The step tests compare every byte
// and counter with a CPU oracle.
// ---------------------------------------------------------------------------

namespace {

int presum_mode(const std::string& presum) {
  if (presum == "auto") return -1;
  if (presum == "on") return 1;
  if (presum == "off") return 0;
  throw std::invalid_argument("presum must be 'auto', 'on' or 'off'");
}

void validate_step_window(size_t n, int per, unsigned long long m, unsigned long long M,
                          unsigned long long capacity) {
  if (m < 1) throw std::invalid_argument("m must be >= 1");
  if (M < 1) throw std::invalid_argument("M must be >= 1");
  if (M > (1ull << 31) / static_cast<unsigned long long>(per))
    throw std::invalid_argument("M * branching must be <= 2^31");
  if (capacity < n) throw std::invalid_argument("capacity must be >= the number of nodes");
}

DevpoolStepCtl step_ctl_of(const DevCtl& c) {
  return {c.size, c.chunk, c.tree, c.sol, c.iters, c.best, c.overflow};
}

template <class NodeT>
DevpoolStepCtl step_readback(std::vector<NodeT>& nodes, const NodeT* pool_d,
                             const DevCtl* ctl_next_d, unsigned long long capacity,
                             hipStream_t s) {
  DevCtl fin{};
  HIP_CHECK(hipMemcpyAsync(&fin, ctl_next_d, sizeof(DevCtl), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (fin.size > capacity) throw std::runtime_error("devpool step: size exceeds capacity");
  nodes.resize(fin.size);
  if (fin.size > 0) {
    HIP_CHECK(hipMemcpyAsync(nodes.data(), pool_d, fin.size * sizeof(NodeT),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  return step_ctl_of(fin);
}

}  // namespace

void validate_nq_step(const std::vector<NQNode>& nodes, int N, int g, int finish,
                      unsigned long long m, unsigned long long M,
                      unsigned long long capacity, const std::string& presum) {
  // the expand kernel stages EMIT_TILE / 4 + 2 parents per block: N >= 4
  if (N < 4 || N > MAX_JOBS) throw std::invalid_argument("N must be in 4..20");
  if (g < 1) throw std::invalid_argument("g must be >= 1");
  if (finish < -1 || finish > 8) throw std::invalid_argument("finish must be in -1..8");
  validate_step_window(nodes.size(), N, m, M, capacity);
  presum_mode(presum);
  for (size_t i = 0; i < nodes.size(); i++) {
    const NQNode& p = nodes[i];
    if (p.depth > N)
      throw std::invalid_argument("node " + std::to_string(i) + ": depth > N");
    uint32_t seen = 0;
    for (int j = 0; j < N; j++) {
      if (p.board[j] >= N || (seen >> p.board[j] & 1u))
        throw std::invalid_argument("node " + std::to_string(i) +
                                    ": board[0:N] is not a permutation of 0..N-1");
      seen |= 1u << p.board[j];
    }
  }
}

void validate_pfsp_step(const std::vector<PFSPNode>& nodes, int inst, const std::string& lb,
                        unsigned long long m, unsigned long long M,
                        unsigned long long capacity, int geom, const std::string& presum,
                        const std::string& br_str) {
  const LbKind lbk = lb_from_string(lb);
  const Branching br = branching_from_string(br_str);
  check_branching_supported(lbk, br, true);
  const int jobs = taillard_nb_jobs(inst);
  if (jobs > MAX_JOBS)
    throw std::invalid_argument("instance exceeds MAX_JOBS=20 (use ta001..ta030)");
  if (geom != -1 && geom != 2 && geom != 3)
    throw std::invalid_argument("geom must be -1, 2 or 3");
  if (geom != -1 && lbk != LbKind::LB2)
    throw std::invalid_argument("geom 2/3 select an lb2 kernel: lb must be 'lb2'");
  validate_step_window(nodes.size(), jobs, m, M, capacity);
  presum_mode(presum);
  for (size_t i = 0; i < nodes.size(); i++) {
    const PFSPNode& p = nodes[i];
    if (p.depth < 0 || p.depth > jobs - 1)
      throw std::invalid_argument("node " + std::to_string(i) + ": depth not in 0..jobs-1");
    if (br == Branching::FWD) {
      // the forward kernels take limit2 == jobs for granted
      if (p.limit1 != p.depth - 1)
        throw std::invalid_argument("node " + std::to_string(i) + ": limit1 != depth - 1");
      if (p.nback != 0)
        throw std::invalid_argument("node " + std::to_string(i) +
                                    ": nback != 0 needs a non-fwd branching rule");
    } else if (p.limit1 < -1 || p.limit1 + 1 + static_cast<int>(p.nback) != p.depth) {
      throw std::invalid_argument("node " + std::to_string(i) +
                                  ": depth != limit1 + 1 + nback");
    }
    uint32_t seen = 0;
    for (int j = 0; j < jobs; j++) {
      if (p.prmu[j] >= jobs || (seen >> p.prmu[j] & 1u))
        throw std::invalid_argument("node " + std::to_string(i) +
                                    ": prmu[0:jobs] is not a permutation of 0..jobs-1");
      seen |= 1u << p.prmu[j];
    }
  }
}

namespace {

// The geometry a PFSP step / chain call runs: devpool_lbk_geom's choice
// unless the caller forces an lb2 kernel.
PfspDevProblem pfsp_step_problem(const PfspInstance& I, const std::string& lb, int geom) {
  return {I, geom < 0 ? devpool_lbk_geom(lbk_of(lb_from_string(lb)), I.machines) : geom};
}

// Callers validate first: nothing here runs before their checks passed.
template <class Problem>
DevpoolStepCtl devpool_step(const Problem& problem, std::vector<typename Problem::Node>& nodes,
                            int best, unsigned long long m, unsigned long long M,
                            unsigned long long capacity, int pm, int device) {
  using NodeT = typename Problem::Node;
  const size_t n = nodes.size();
  // grids sized to the pool that exists, like the engine loops' chunk bound
  // (bound >= size, so min(size, Mi) == min(size, M))
  const unsigned long long Mi = std::min<unsigned long long>(M, std::max<size_t>(n, 1));
  set_device_cached(device);
  const Problem P = problem.on_device(device);
  StreamGuard stream;
  const DevpoolBufs<NodeT> bufs(capacity, Mi, P.per, P.lbg, Problem::needs_be,
                                /*group_sums=*/true);
  // auto: the slice thread's sizing rule (the frontier builder's is its
  // lbg == 2 half)
  const bool ps = pm < 0 ? devpool_presum_alloc(bufs.G, P.lbg) : pm == 1;
  DevCtl ctl{};
  ctl.size = n;
  ctl.best = best;
  if (n > 0)
    HIP_CHECK(hipMemcpyAsync(bufs.pool.p, nodes.data(), n * sizeof(NodeT),
                             hipMemcpyHostToDevice, stream.s));
  upload_ctl_pair(bufs.ctl.p, ctl, stream.s);
  (void)hipGetLastError();  // drop a stale launch error of an earlier, unchecked call
  P.enqueue(bufs, bufs.ctl.p, bufs.ctl.p + 1, m, Mi, ps, stream.s);
  HIP_CHECK(hipGetLastError());
  return step_readback(nodes, bufs.pool.p, bufs.ctl.p + 1, capacity, stream.s);
}

}  // namespace

DevpoolStepCtl nq_devpool_step(std::vector<NQNode>& nodes, int N, int g,
                               const NqFinishOpts& finisher, unsigned long long m,
                               unsigned long long M, unsigned long long capacity,
                               const std::string& presum, int device) {
  // before any HIP call
  validate_nq_step(nodes, N, g, finisher.finish, m, M, capacity, presum);
  return devpool_step(NqDevProblem(N, g, nq_finish_opts(g, finisher)), nodes,
                      /*best=*/0, m, M, capacity, presum_mode(presum), device);
}

DevpoolStepCtl pfsp_devpool_step(std::vector<PFSPNode>& nodes, int inst, const std::string& lb,
                                 int best, unsigned long long m, unsigned long long M,
                                 unsigned long long capacity, int geom,
                                 const std::string& presum, int device,
                                 const std::string& br) {
  validate_pfsp_step(nodes, inst, lb, m, M, capacity, geom, presum, br);  // before any HIP call
  const PfspInstance& I = pfsp_instance_cached(inst, 1, branching_from_string(br));
  return devpool_step(pfsp_step_problem(I, lb, geom), nodes, best, m, M, capacity,
                      presum_mode(presum), device);
}

// ---------------------------------------------------------------------------
// Chain entry points (declared in engine_gpu.hpp): k iterations back to back
// over ONE set of buffers sized for the largest window, alternating control
// blocks, no host synchronisation in between — the launch shape of the engine
// threads, minus the loop driver. A snapshot of the live control block and of
// the pool follows every iteration on the same stream.
// ---------------------------------------------------------------------------

namespace {

constexpr unsigned long long CHAIN_MAX_ITERS = 16;
constexpr unsigned long long CHAIN_MAX_NODES = 1ull << 22;  // capacity * (k + 1)

void validate_chain_windows(const std::vector<unsigned long long>& windows, int per,
                            unsigned long long capacity) {
  const unsigned long long k = windows.size();
  if (k < 1 || k > CHAIN_MAX_ITERS)
    throw std::invalid_argument("windows must hold 1..16 entries");
  for (unsigned long long w : windows) {
    if (w < 1) throw std::invalid_argument("every window must be >= 1");
    if (w > (1ull << 31) / static_cast<unsigned long long>(per))
      throw std::invalid_argument("window * branching must be <= 2^31");
  }
  if (capacity > CHAIN_MAX_NODES / (k + 1))
    throw std::invalid_argument("capacity * (len(windows) + 1) must be <= 2^22 nodes");
}

// Callers validate first: nothing here runs before their checks passed.
template <class Problem>
std::vector<DevpoolSnapshot<typename Problem::Node>> devpool_chain(
    const Problem& problem, const std::vector<typename Problem::Node>& nodes, int best,
    unsigned long long m, const std::vector<unsigned long long>& windows,
    unsigned long long capacity, int pm, int device) {
  using NodeT = typename Problem::Node;
  const unsigned long long Mc = *std::max_element(windows.begin(), windows.end());
  set_device_cached(device);
  const Problem P = problem.on_device(device);
  StreamGuard stream;
  const hipStream_t s = stream.s;
  // sized ONCE for the largest window, as a slice thread sizes them for Mc
  const bool presum_alloc = devpool_presum_alloc(devpool_grid(Mc, P.per, P.lbg), P.lbg);
  const DevpoolBufs<NodeT> bufs(capacity, Mc, P.per, P.lbg, Problem::needs_be,
                                presum_alloc || pm == 1);
  NodeT* const pool_d = bufs.pool.p;
  DevCtl* const ctl_d = bufs.ctl.p;
  const size_t n = nodes.size();
  const size_t k = windows.size();
  DevGuard<NodeT> snap_pool_d(std::max<size_t>(capacity * k, 1));
  DevGuard<DevCtl> snap_ctl_d(k);
  DevCtl ctl{};
  ctl.size = n;
  ctl.best = best;
  if (n > 0)
    HIP_CHECK(hipMemcpyAsync(pool_d, nodes.data(), n * sizeof(NodeT), hipMemcpyHostToDevice, s));
  upload_ctl_pair(ctl_d, ctl, s);
  (void)hipGetLastError();  // drop a stale launch error of an earlier, unchecked call
  for (size_t i = 0; i < k; i++) {
    DevCtl* cur = ctl_d + (i & 1);
    DevCtl* next = ctl_d + 1 - (i & 1);
    const DevIterPolicy it = devpool_iter_policy(Mc, windows[i], P.per, P.lbg, presum_alloc);
    P.enqueue(bufs, cur, next, m, it.Mi, pm < 0 ? it.ps : pm == 1, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(snap_ctl_d.p + i, next, sizeof(DevCtl), hipMemcpyDeviceToDevice, s));
    if (capacity > 0)
      HIP_CHECK(hipMemcpyAsync(snap_pool_d.p + i * capacity, pool_d, capacity * sizeof(NodeT),
                               hipMemcpyDeviceToDevice, s));
  }
  std::vector<DevCtl> fin(k);
  HIP_CHECK(hipMemcpyAsync(fin.data(), snap_ctl_d.p, k * sizeof(DevCtl), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));

  std::vector<DevpoolSnapshot<NodeT>> out(k);
  // live size entering iteration i, and the un-popped prefix once overflowed:
  // the overflowing iteration leaves [base, ..) undefined and every later
  // iteration pops nothing, so that prefix is what all later snapshots keep
  unsigned long long prev = n, ovf_base = 0;
  bool overflowed = false;
  for (size_t i = 0; i < k; i++) {
    const DevCtl& f = fin[i];
    unsigned long long keep;
    if (f.overflow) {
      if (!overflowed) {
        const unsigned long long c = prev < m ? 0 : std::min(prev, windows[i]);
        ovf_base = prev - c;
        overflowed = true;
      }
      keep = ovf_base;
    } else {
      if (f.size > capacity) throw std::runtime_error("devpool chain: size exceeds capacity");
      keep = f.size;
      prev = f.size;
    }
    if (keep > capacity) throw std::runtime_error("devpool chain: prefix exceeds capacity");
    out[i].nodes.resize(keep);
    if (keep > 0)
      HIP_CHECK(hipMemcpyAsync(out[i].nodes.data(), snap_pool_d.p + i * capacity,
                               keep * sizeof(NodeT), hipMemcpyDeviceToHost, s));
    out[i].ctl = step_ctl_of(f);
  }
  HIP_CHECK(hipStreamSynchronize(s));
  return out;
}

}  // namespace

std::vector<DevpoolSnapshot<NQNode>> nq_devpool_chain(
    const std::vector<NQNode>& nodes, int N, int g, const NqFinishOpts& finisher,
    unsigned long long m, const std::vector<unsigned long long>& windows,
    unsigned long long capacity, const std::string& presum, int device) {
  // before any HIP call
  validate_nq_step(nodes, N, g, finisher.finish, m, 1, capacity, presum);
  const NqFinishOpts opts = nq_finish_opts(g, finisher);
  validate_chain_windows(windows, N, capacity);
  return devpool_chain(NqDevProblem(N, g, opts), nodes, /*best=*/0, m, windows, capacity,
                       presum_mode(presum), device);
}

std::vector<DevpoolSnapshot<PFSPNode>> pfsp_devpool_chain(
    const std::vector<PFSPNode>& nodes, int inst, const std::string& lb, int best,
    unsigned long long m, const std::vector<unsigned long long>& windows,
    unsigned long long capacity, int geom, const std::string& presum, int device,
    const std::string& br) {
  validate_pfsp_step(nodes, inst, lb, m, 1, capacity, geom, presum, br);  // before any HIP call
  validate_chain_windows(windows, taillard_nb_jobs(inst), capacity);
  const PfspInstance& I = pfsp_instance_cached(inst, 1, branching_from_string(br));
  return devpool_chain(pfsp_step_problem(I, lb, geom), nodes, best, m, windows, capacity,
                       presum_mode(presum), device);
}

// ---------------------------------------------------------------------------
// Loop-driver test entry points (declared in engine_gpu.hpp): one slice
// through the real devpool_thread (devpool_driver.hpp), traced. Nothing else
// goes through them.
// ---------------------------------------------------------------------------

namespace {

constexpr unsigned long long LOOP_TRACE_MAX_NODES = 1ull << 22;

// The observer of the traced runs: one DevLoopRec per call, nodes copied over
// the thread's idle stream. The copies are not counted in the diag counters.
class LoopRecorder : public DevLoopObserver {
 public:
  LoopRecorder(DevLoopTrace& t, size_t node_bytes, unsigned long long capacity)
      : t_(t), node_bytes_(node_bytes), capacity_(capacity) {}

  void run_begin(bool from_spill, unsigned long long size, int best) override {
    run_ = t_.recs.size();
    DevLoopRec& rec = add(DevLoopRec::RUN, size);
    rec.from_spill = from_spill;
    rec.best = best;
  }
  void run_end(unsigned long long leftover) override { t_.recs[run_].size_after = leftover; }
  void batch(int b, int parity, bool replayed, bool captured, unsigned long long size_before,
             const DevCtl& ctl, const void* pool_d, hipStream_t s) override {
    DevLoopRec& rec = add(DevLoopRec::BATCH, size_before);
    rec.b = b;
    rec.parity = parity;
    rec.graph = replayed;
    rec.captured = captured;
    rec.ctl = step_ctl_of(ctl);
    if (ctl.overflow) return;
    if (ctl.size > capacity_) throw std::runtime_error("devpool loop: size exceeds capacity");
    trace_nodes(rec, pool_d, ctl.size, &s);
  }
  void spill(unsigned long long size_before, unsigned long long size_after, const void* moved,
             unsigned long long n) override {
    DevLoopRec& rec = add(DevLoopRec::SPILL, size_before);
    rec.size_after = size_after;
    trace_nodes(rec, moved, n, nullptr);
  }
  void donate_carve(unsigned long long size_before, unsigned long long kept, int best,
                    const void* offered_d, hipStream_t s) override {
    DevLoopRec& rec = add(DevLoopRec::DONATE, size_before);
    rec.best = best;
    trace_nodes(rec, offered_d, size_before - kept, &s);
  }
  void donate_end(Donation outcome, unsigned long long size_after) override {
    if (outcome == Donation::NONE) return;  // no carve, no record
    t_.recs.back().size_after = size_after;
    t_.recs.back().outcome = static_cast<int>(outcome);
  }
  void take(unsigned long long n, int best, const void* pool_d, hipStream_t s) override {
    DevLoopRec& rec = add(DevLoopRec::TAKE, n);
    rec.size_after = n;
    rec.best = best;
    trace_nodes(rec, pool_d, n, &s);
  }

 private:
  DevLoopRec& add(int kind, unsigned long long size_before) {
    t_.recs.emplace_back();
    t_.recs.back().kind = kind;
    t_.recs.back().size_before = size_before;
    return t_.recs.back();
  }
  // Copy `n` nodes into a record: from device memory over the (idle) stream
  // `*s`, or from host memory when `s` is null.
  void trace_nodes(DevLoopRec& rec, const void* src, unsigned long long n,
                   const hipStream_t* s) {
    t_.traced_nodes += n;
    if (t_.traced_nodes > LOOP_TRACE_MAX_NODES)
      throw std::runtime_error("devpool loop trace exceeds 2^22 nodes");
    rec.nodes.resize(n * node_bytes_);
    if (n == 0) return;
    if (!s) {
      std::memcpy(rec.nodes.data(), src, rec.nodes.size());
      return;
    }
    HIP_CHECK(hipMemcpyAsync(rec.nodes.data(), src, rec.nodes.size(), hipMemcpyDeviceToHost, *s));
    HIP_CHECK(hipStreamSynchronize(*s));
  }

  DevLoopTrace& t_;
  const size_t node_bytes_;
  const unsigned long long capacity_;
  size_t run_ = 0;  // the open RUN record
};

}  // namespace

void validate_devpool_loop(size_t n, unsigned long long chunk, unsigned long long capacity,
                           long long max_batches) {
  if (capacity < 1 || capacity > LOOP_TRACE_MAX_NODES)
    throw std::invalid_argument("capacity must be in 1..2^22 nodes");
  if (chunk > capacity) throw std::invalid_argument("chunk must be <= capacity");
  if (max_batches < 0 || max_batches > 4096)
    throw std::invalid_argument("max_batches must be in 0..4096");
  if (n == 0) throw std::invalid_argument("the pool must hold at least one node");
}

// Callers validate first: nothing here runs before their checks passed.
template <class Problem>
DevpoolLoopOut<typename Problem::Node> devpool_loop_traced(
    const Problem& problem, const std::vector<typename Problem::Node>& nodes, int best0,
    unsigned long long m, unsigned long long chunk, unsigned long long capacity, bool graph,
    int max_batches, std::atomic<int>* sb, long long lower_at, int lower_to, int device) {
  using NodeT = typename Problem::Node;
  DevpoolLoopOut<NodeT> out;
  DevpoolThreadTest test;
  test.chunk = chunk;
  test.max_batches = max_batches;
  LoopRecorder rec(out.trace, sizeof(NodeT), capacity);
  const std::vector<std::vector<NodeT>> slices{nodes};
  std::atomic<int> next_slice{0};
  long long batch = 0;
  const SliceReadbackFn<NodeT> lower = [&](const SliceReadback<NodeT>&) {
    if (sb && batch++ == lower_at) min_into(*sb, lower_to);
  };
  (void)hipGetLastError();  // drop a stale launch error of an earlier, unchecked call
  const SliceOut so =
      devpool_thread(problem, slices, next_slice, best0, static_cast<int>(m), /*M=*/0, device,
                     capacity, sb, graph, /*share=*/nullptr, out.leftover, lower, &test, &rec);
  out.tree = so.fin.tree;
  out.sol = so.fin.sol;
  out.iters = so.diag.gpu_iters;
  out.best = so.fin.best;
  if (sb) out.best = std::min(out.best, sb->load(std::memory_order_relaxed));
  out.diag = so.diag;
  return out;
}

DevpoolLoopOut<NQNode> nq_devpool_loop(const std::vector<NQNode>& nodes, int N, int g,
                                       int finish, unsigned long long m,
                                       unsigned long long chunk, unsigned long long capacity,
                                       bool graph, int max_batches, int device) {
  // before any HIP call
  validate_nq_step(nodes, N, g, finish, m, chunk, capacity, "auto");
  validate_devpool_loop(nodes.size(), chunk, capacity, max_batches);
  if (m > (1ull << 30)) throw std::invalid_argument("m must be <= 2^30");
  return devpool_loop_traced(NqDevProblem(N, g, nq_finish_opts(g, {finish})), nodes,
                             /*best0=*/0, m, chunk,
                             capacity, graph, max_batches, nullptr, -1, 0, device);
}

DevpoolLoopOut<PFSPNode> pfsp_devpool_loop(const std::vector<PFSPNode>& nodes, int inst,
                                           const std::string& lb, int best,
                                           unsigned long long m, unsigned long long chunk,
                                           unsigned long long capacity, bool graph,
                                           int max_batches, const std::string& br,
                                           long long lower_at, int lower_to, int device) {
  // before any HIP call
  validate_pfsp_step(nodes, inst, lb, m, chunk, capacity, /*geom=*/-1, "auto", br);
  validate_devpool_loop(nodes.size(), chunk, capacity, max_batches);
  if (m > (1ull << 30)) throw std::invalid_argument("m must be <= 2^30");
  if (best < 1) throw std::invalid_argument("best must be >= 1");
  if (lower_at < -1) throw std::invalid_argument("lower_best_at: batch must be >= 0");
  if (lower_at >= 0 && lower_to < 1)
    throw std::invalid_argument("lower_best_at: value must be >= 1");
  const PfspInstance& I = pfsp_instance_cached(inst, 1, branching_from_string(br));
  std::atomic<int> sb{best};
  return devpool_loop_traced(
      PfspDevProblem(I, devpool_lbk_geom(lbk_of(lb_from_string(lb)), I.machines)), nodes, best,
      m, chunk, capacity, graph, max_batches, &sb, lower_at, lower_to, device);
}

// Share entry points: `threads` slice threads, one SliceShare, one slice.

void validate_devpool_share(int threads, long long donate_floor, long long await_idle_ms) {
  if (threads < 2 || threads > 4) throw std::invalid_argument("threads must be in 2..4");
  if (donate_floor != 0 && donate_floor < 2)
    throw std::invalid_argument("donate_floor must be 0 (the real floor) or >= 2");
  if (await_idle_ms < 0 || await_idle_ms > 5000)
    throw std::invalid_argument("await_idle_ms must be in 0..5000");
}

// Callers validate first: nothing here runs before their checks passed.
template <class Problem>
std::vector<DevpoolLoopOut<typename Problem::Node>> devpool_share_traced(
    const Problem& problem, const std::vector<typename Problem::Node>& nodes, int best0,
    unsigned long long m, unsigned long long chunk, unsigned long long capacity,
    int max_batches, std::atomic<int>* sb, int threads, unsigned long long donate_floor,
    int await_idle_ms, int device) {
  using NodeT = typename Problem::Node;
  std::vector<DevpoolLoopOut<NodeT>> outs(threads);
  std::vector<DevpoolThreadTest> tests(threads);
  std::vector<LoopRecorder> recs;
  for (auto& o : outs) recs.emplace_back(o.trace, sizeof(NodeT), capacity);
  const std::vector<std::vector<NodeT>> slices{nodes};
  std::atomic<int> next_slice{0};
  SliceShare share;
  std::vector<SliceOut> sos(threads);
  std::vector<std::exception_ptr> errs(threads);
  std::atomic<bool> first_done{false};
  (void)hipGetLastError();  // drop a stale launch error of an earlier, unchecked call
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++) {
    tests[t].chunk = chunk;
    tests[t].max_batches = max_batches;
    tests[t].donate_floor = donate_floor;
    tests[t].await_idle_ms = await_idle_ms;
    tests[t].threads = threads;
    pool.emplace_back([&, t] {
      try {
        sos[t] = devpool_thread(problem, slices, next_slice, best0, static_cast<int>(m),
                                /*M=*/0, device, capacity, sb, /*allow_graph=*/false, &share,
                                outs[t].leftover, {}, &tests[t], &recs[t]);
      } catch (...) {
        errs[t] = std::current_exception();
      }
      if (t == 0) first_done.store(true);
    });
    // a thread that reaches wait_for_work before the slice's owner counts as a
    // runner leaves at once (the engines live with that); here the others
    // start only once thread 0 runs the slice, or is through with it
    if (t == 0) {
      const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(5);
      while (!first_done.load() && std::chrono::steady_clock::now() < deadline) {
        {
          std::lock_guard<std::mutex> l(share.mu);
          if (share.runners > 0) break;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
      }
    }
  }
  for (auto& th : pool) th.join();
  for (auto& e : errs)
    if (e) std::rethrow_exception(e);
  for (int t = 0; t < threads; t++) {
    DevpoolLoopOut<NodeT>& out = outs[t];
    out.tree = sos[t].fin.tree;
    out.sol = sos[t].fin.sol;
    out.iters = sos[t].diag.gpu_iters;
    out.best = sos[t].fin.best;
    out.diag = sos[t].diag;
  }
  return outs;
}

std::vector<DevpoolLoopOut<NQNode>> nq_devpool_share(
    const std::vector<NQNode>& nodes, int N, int g, int finish, unsigned long long m,
    unsigned long long chunk, unsigned long long capacity, int max_batches, int threads,
    unsigned long long donate_floor, int await_idle_ms, int device) {
  // before any HIP call
  validate_nq_step(nodes, N, g, finish, m, chunk, capacity, "auto");
  validate_devpool_loop(nodes.size(), chunk, capacity, max_batches);
  validate_devpool_share(threads, static_cast<long long>(donate_floor), await_idle_ms);
  if (m > (1ull << 30)) throw std::invalid_argument("m must be <= 2^30");
  return devpool_share_traced(NqDevProblem(N, g, nq_finish_opts(g, {finish})), nodes,
                              /*best0=*/0, m, chunk,
                              capacity, max_batches, nullptr, threads, donate_floor,
                              await_idle_ms, device);
}

std::vector<DevpoolLoopOut<PFSPNode>> pfsp_devpool_share(
    const std::vector<PFSPNode>& nodes, int inst, const std::string& lb, int best,
    unsigned long long m, unsigned long long chunk, unsigned long long capacity,
    int max_batches, const std::string& br, int threads, unsigned long long donate_floor,
    int await_idle_ms, int device) {
  // before any HIP call
  validate_pfsp_step(nodes, inst, lb, m, chunk, capacity, /*geom=*/-1, "auto", br);
  validate_devpool_loop(nodes.size(), chunk, capacity, max_batches);
  validate_devpool_share(threads, static_cast<long long>(donate_floor), await_idle_ms);
  if (m > (1ull << 30)) throw std::invalid_argument("m must be <= 2^30");
  if (best < 1) throw std::invalid_argument("best must be >= 1");
  const PfspInstance& I = pfsp_instance_cached(inst, 1, branching_from_string(br));
  std::atomic<int> sb{best};
  return devpool_share_traced(
      PfspDevProblem(I, devpool_lbk_geom(lbk_of(lb_from_string(lb)), I.machines)), nodes, best,
      m, chunk, capacity, max_batches, &sb, threads, donate_floor, await_idle_ms, device);
}

// ---------------------------------------------------------------------------
// Eval-only entry points (HIP-kernel-vs-CPU-oracle numerics tests)
// ---------------------------------------------------------------------------

std::vector<uint8_t> nq_gpu_labels(int N, int g, const std::vector<NQNode>& nodes,
                                   int device) {
  set_device_cached(device);
  const size_t n = nodes.size();
  std::vector<uint8_t> labels(n * N, 255);
  DevGuard<NQNode> parents_d(n);
  DevGuard<uint8_t> labels_d(n * N);
  HIP_CHECK(hipMemcpy(parents_d.p, nodes.data(), n * sizeof(NQNode), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(labels_d.p, 255, n * N));
  launch_nq_eval(parents_d.p, static_cast<int>(n), N, g, labels_d.p, nullptr);
  HIP_CHECK(hipMemcpy(labels.data(), labels_d.p, n * N, hipMemcpyDeviceToHost));
  return labels;
}

std::vector<int32_t> pfsp_gpu_bounds(int inst, const std::string& lb_str,
                                     const std::vector<PFSPNode>& nodes, int best,
                                     int device) {
  const LbKind lb = lb_from_string(lb_str);
  PfspInstance I = make_pfsp_instance(inst, 1);
  set_device_cached(device);
  PfspTablesGuard tables(I);
  const size_t n = nodes.size();
  std::vector<int32_t> bounds(n * I.jobs, -1);
  DevGuard<PFSPNode> parents_d(n);
  DevGuard<int32_t> bounds_d(n * I.jobs);
  HIP_CHECK(hipMemcpy(parents_d.p, nodes.data(), n * sizeof(PFSPNode), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(bounds_d.p, 255, n * I.jobs * sizeof(int32_t)));
  launch_pfsp_eval(parents_d.p, static_cast<int>(n), I.jobs, I.machines, lbk_of(lb),
                   tables.tb, best, bounds_d.p, nullptr);
  HIP_CHECK(hipMemcpy(bounds.data(), bounds_d.p, n * I.jobs * sizeof(int32_t),
                      hipMemcpyDeviceToHost));
  return bounds;
}

std::pair<std::vector<int32_t>, std::vector<int32_t>> pfsp_gpu_bounds_bi(
    int inst, const std::vector<PFSPNode>& nodes, int device) {
  PfspInstance I = make_pfsp_instance(inst, 1);
  // the kernel indexes prmu by [limit1 + 1, jobs - nback): check before any HIP call
  for (size_t i = 0; i < nodes.size(); i++) {
    const PFSPNode& p = nodes[i];
    if (p.limit1 < -1 || p.limit1 + 1 + static_cast<int>(p.nback) > I.jobs)
      throw std::invalid_argument("node " + std::to_string(i) +
                                  ": limit1 + 1 + nback exceeds jobs");
    for (int j = 0; j < I.jobs; j++)
      if (p.prmu[j] >= I.jobs)
        throw std::invalid_argument("node " + std::to_string(i) + ": prmu entry >= jobs");
  }
  set_device_cached(device);
  PfspTablesGuard tables(I);
  const size_t n = nodes.size();
  std::vector<int32_t> lb_begin(n * I.jobs, -1), lb_end(n * I.jobs, -1);
  if (n == 0) return {lb_begin, lb_end};
  DevGuard<PFSPNode> parents_d(n);
  DevGuard<int32_t> begin_d(n * I.jobs), end_d(n * I.jobs);
  HIP_CHECK(hipMemcpy(parents_d.p, nodes.data(), n * sizeof(PFSPNode), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(begin_d.p, 255, n * I.jobs * sizeof(int32_t)));
  HIP_CHECK(hipMemset(end_d.p, 255, n * I.jobs * sizeof(int32_t)));
  (void)hipGetLastError();  // drop a stale launch error of an earlier, unchecked call
  launch_pfsp_eval(parents_d.p, static_cast<int>(n), I.jobs, I.machines, 0, tables.tb, 0,
                   begin_d.p, nullptr, static_cast<int>(Branching::MINBRANCH), end_d.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(lb_begin.data(), begin_d.p, n * I.jobs * sizeof(int32_t),
                      hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(lb_end.data(), end_d.p, n * I.jobs * sizeof(int32_t),
                      hipMemcpyDeviceToHost));
  return {lb_begin, lb_end};
}

void validate_lb12_nodes(const std::vector<PFSPNode>& nodes, int jobs) {
  for (size_t i = 0; i < nodes.size(); i++) {
    const PFSPNode& p = nodes[i];
    if (p.limit1 < -1 || p.limit1 + 1 + static_cast<int>(p.nback) > jobs)
      throw std::invalid_argument("node " + std::to_string(i) +
                                  ": limit1 + 1 + nback exceeds jobs");
    if (p.depth != p.limit1 + 1 + static_cast<int>(p.nback))
      throw std::invalid_argument("node " + std::to_string(i) +
                                  ": depth != limit1 + 1 + nback");
    for (int j = 0; j < jobs; j++)
      if (p.prmu[j] >= jobs)
        throw std::invalid_argument("node " + std::to_string(i) + ": prmu entry >= jobs");
  }
}

std::pair<std::vector<uint8_t>, std::vector<int32_t>> pfsp_gpu_bounds_lb12(
    int inst, const std::vector<PFSPNode>& nodes, int best, const std::string& br_str,
    int device) {
  const Branching br = branching_from_string(br_str);
  PfspInstance I = make_pfsp_instance(inst, 1, br);
  validate_lb12_nodes(nodes, I.jobs);  // before any HIP call
  const size_t n = nodes.size();
  std::vector<uint8_t> dir(n, 255);
  std::vector<int32_t> bounds(n * I.jobs, -1);
  if (n == 0) return {dir, bounds};
  set_device_cached(device);
  PfspTablesGuard tables(I);
  DevGuard<PFSPNode> parents_d(n);
  DevGuard<uint8_t> dir_d(n);
  DevGuard<int32_t> bounds_d(n * I.jobs);
  HIP_CHECK(hipMemcpy(parents_d.p, nodes.data(), n * sizeof(PFSPNode), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(dir_d.p, 255, n));
  HIP_CHECK(hipMemset(bounds_d.p, 255, n * I.jobs * sizeof(int32_t)));
  (void)hipGetLastError();  // drop a stale launch error of an earlier, unchecked call
  launch_pfsp_eval(parents_d.p, static_cast<int>(n), I.jobs, I.machines, lbk_of(LbKind::LB12),
                   tables.tb, best, bounds_d.p, nullptr, static_cast<int>(br), nullptr,
                   dir_d.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(dir.data(), dir_d.p, n, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(bounds.data(), bounds_d.p, n * I.jobs * sizeof(int32_t),
                      hipMemcpyDeviceToHost));
  return {dir, bounds};
}
}  // namespace gats
