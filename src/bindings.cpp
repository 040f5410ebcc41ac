// pybind11 bindings for the gats_amd core (built directly with hipcc; no
// libtorch dependency — torch is only used by the Python distributed tier).
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <cstring>
#include <stdexcept>

#include "devpool_loop_plan.hpp"
#include "engine_gpu.hpp"
#include "gpu_api.hpp"
#include "nodes.hpp"
#include "nq_finish.hpp"
#include "nq_finish_cpu.hpp"
#include "pool.hpp"
#include "search_host.hpp"
#include "share_selftest.hpp"
#include "slice_share.hpp"
#include "taillard.hpp"

namespace py = pybind11;
using namespace gats;

namespace {

py::dict result_to_dict(const Result& r) {
  py::dict d;
  d["tree"] = r.tree;
  d["sol"] = r.sol;
  d["optimum"] = r.optimum;
  d["time"] = r.time;
  py::list phases;
  for (const auto& p : r.phases) {
    py::dict pd;
    pd["tree"] = p.tree;
    pd["sol"] = p.sol;
    pd["time"] = p.time;
    phases.append(pd);
  }
  d["phases"] = phases;
  py::dict diag;
  diag["kernel_launch"] = r.kernel_launch;
  diag["host_to_device"] = r.h2d;
  diag["device_to_host"] = r.d2h;
  diag["h2d_bytes"] = r.h2d_bytes;
  diag["d2h_bytes"] = r.d2h_bytes;
  diag["gpu_iters"] = r.gpu_iters;
  diag["gpu_time"] = r.gpu_time;
  d["diag"] = diag;
  if (!r.per_worker.empty()) {
    py::list w;
    for (uint64_t v : r.per_worker) w.append(v);
    d["per_worker_tree"] = w;
  }
  return d;
}

template <typename NodeT>
std::vector<NodeT> nodes_from_bytes(const py::bytes& b) {
  std::string s = b;  // copy; fine for frontier-scale data
  if (s.size() % sizeof(NodeT) != 0)
    throw std::invalid_argument("node buffer size not a multiple of 24");
  std::vector<NodeT> v(s.size() / sizeof(NodeT));
  std::memcpy(v.data(), s.data(), s.size());
  return v;
}

// CPU run of the k_nq_x finisher's loop (nq_finish.hpp) over one job: the
// nodes and solutions below the state (cols, d1, d2) whose first empty row is
// `row`. Jobs of up to 8 rows go through the kernel's own instantiation.
template <int LEVELS>
py::tuple nq_finish_count(uint32_t cols, uint32_t d1, uint32_t d2, int row, int N) {
  NqFlat<LEVELS> st;
  st.tree = 0;
  st.sol = 0;
  const uint32_t msk = (1u << N) - 1u;
  st.template load<true>(cols, d1, d2, row, N, msk, 1);
  st.template exhaust<true>(msk, 1);
  return py::make_tuple(static_cast<uint64_t>(st.tree), static_cast<uint64_t>(st.sol));
}

py::tuple nq_finish_count_cpu(uint32_t cols, uint32_t d1, uint32_t d2, int row, int N) {
  if (N < 1 || N > MAX_JOBS) throw std::invalid_argument("N must be in 1..20");
  const int rows = N - row;
  if (row < 0 || rows < 1 || rows > NQ_FLAT_LEVELS_MAX)
    throw std::invalid_argument("the job needs 1..12 empty rows");
  if ((cols | d1 | d2) >> N) throw std::invalid_argument("mask bits at or above column N");
  return rows <= NQ_FLAT_LEVELS_DEV ? nq_finish_count<NQ_FLAT_LEVELS_DEV>(cols, d1, d2, row, N)
                                    : nq_finish_count<NQ_FLAT_LEVELS_MAX>(cols, d1, d2, row, N);
}

// The CPU twins of k_nq_x's drains over one block's job queue (nq_finish_cpu.hpp).
// jobs: (cols, d1, d2, row) states as nq_finish_count_cpu takes them.
// Split finisher, one flat loop: (tree, sol, entries, rounds).
py::tuple nq_finish_block_cpu(const NqJobs& jobs, int N, int g, int split, long long qcap) {
  const NqSplitRun r = nq_finish_block(jobs, N, g, split, qcap);
  return py::make_tuple(r.tree, r.sol, r.entries, r.rounds);
}

// Split finisher as `waves` x `lanes` walks in lockstep:
// (tree, sol, entries, rounds, refills, steps).
py::tuple nq_finish_wave_cpu(const NqJobs& jobs, int N, int g, int split, long long qcap,
                             int refill, int lanes, int waves) {
  const NqSplitRun r = nq_finish_wave(jobs, N, g, split, qcap, refill, lanes, waves);
  return py::make_tuple(r.tree, r.sol, r.entries, r.rounds, r.refills, r.steps);
}

// Wave-stack finisher:
// (tree, sol, iterations per wave, peak sp per wave, fallback walks).
py::tuple nq_finish_stack_cpu(const NqJobs& jobs, int N, int g, int refill, int waves, int lanes,
                              long long cap) {
  const NqStackRun r = nq_finish_stack(jobs, N, g, refill, waves, lanes, cap);
  return py::make_tuple(r.tree, r.sol, r.iters, r.peak_sp, r.fallbacks);
}

py::tuple nq_entry_unpack_py(uint64_t w) {
  uint32_t c, d1, d2;
  const uint32_t h = nq_entry_unpack(w, c, d1, d2);
  return py::make_tuple(c, d1, d2, h);
}

// The packed parent masks and the job reference, for tests.
py::tuple nq_pmask_unpack_py(uint64_t w) {
  uint32_t c, d1, d2;
  nq_pmask_unpack(w, c, d1, d2);
  return py::make_tuple(c, d1, d2);
}

// (cols, d1, d2, row): the job below child column `ref & 31` of the parent
// whose packed masks are `w`, as nq_finish_count_cpu takes it.
py::tuple nq_job_state_py(uint64_t w, uint32_t ref, int N) {
  if (N < 1 || N > MAX_JOBS) throw std::invalid_argument("N must be in 1..20");
  uint32_t c, d1, d2;
  const int row = nq_job_state(w, ref, (1u << N) - 1u, c, d1, d2);
  return py::make_tuple(c, d1, d2, row);
}

// The sub-job queue entry codec, for tests: encode, and decode to
// (ref, ncols, c1, c2).
py::tuple nq_sub_decode_py(uint32_t e) {
  return py::make_tuple(nq_sub_ref(e), nq_sub_ncols(e), nq_sub_c1(e), nq_sub_c2(e));
}

template <typename NodeT>
py::bytes nodes_to_bytes(const NodeT* p, size_t n) {
  return py::bytes(reinterpret_cast<const char*>(p), n * sizeof(NodeT));
}

// CPU oracle twins of the GPU eval kernels (same output layout) for numerics
// tests: GPU labels/bounds must match these exactly.
py::bytes nq_cpu_labels(int N, int g, const py::bytes& pool_bytes) {
  auto nodes = nodes_from_bytes<NQNode>(pool_bytes);
  std::vector<uint8_t> labels(nodes.size() * N, 255);
  for (size_t i = 0; i < nodes.size(); i++) {
    const NQNode& p = nodes[i];
    if (p.depth >= N) continue;
    for (int k = p.depth; k < N; k++)
      labels[i * N + k] = nq_is_safe(p.board, p.depth, p.board[k], g) ? 1 : 0;
  }
  return py::bytes(reinterpret_cast<const char*>(labels.data()), labels.size());
}

std::vector<int32_t> pfsp_cpu_bounds(int inst, const std::string& lb_str,
                                     const py::bytes& pool_bytes, int best) {
  const LbKind lb = lb_from_string(lb_str);
  PfspInstance I = make_pfsp_instance(inst, 1);
  auto nodes = nodes_from_bytes<PFSPNode>(pool_bytes);
  std::vector<int32_t> bounds(nodes.size() * I.jobs, -1);
  for (size_t i = 0; i < nodes.size(); i++) {
    const PFSPNode& p = nodes[i];
    if (lb == LbKind::LB1_D) {
      int lb_begin[MAX_JOBS];
      lb1_children_bounds(I.lb1, p.prmu, p.limit1, I.jobs, lb_begin);
      for (int k = p.limit1 + 1; k < I.jobs; k++)
        bounds[i * I.jobs + k] = lb_begin[p.prmu[k]];
    } else {
      for (int k = p.limit1 + 1; k < I.jobs; k++) {
        PFSPNode child = p;
        child.depth = static_cast<int8_t>(p.depth + 1);
        child.limit1 = static_cast<int8_t>(p.limit1 + 1);
        child.prmu[p.depth] = p.prmu[k];
        child.prmu[k] = p.prmu[p.depth];
        bounds[i * I.jobs + k] =
            (lb == LbKind::LB1)
                ? lb1_bound(I.lb1, child.prmu, child.limit1, I.jobs)
                : lb2_bound(I.lb1, I.lb2, child.prmu, child.limit1, I.jobs, best);
      }
    }
  }
  return bounds;
}

// Both-directions lb1_d child bounds (same layout as pfsp_gpu_bounds_bi): by
// position, -1 outside the parent's unscheduled range.
py::tuple pfsp_cpu_bounds_bi(int inst, const py::bytes& pool_bytes) {
  PfspInstance I = make_pfsp_instance(inst, 1);
  auto nodes = nodes_from_bytes<PFSPNode>(pool_bytes);
  std::vector<int32_t> lb_begin(nodes.size() * I.jobs, -1), lb_end(nodes.size() * I.jobs, -1);
  for (size_t i = 0; i < nodes.size(); i++) {
    const PFSPNode& p = nodes[i];
    const int limit2 = I.jobs - p.nback;
    if (p.limit1 < -1 || p.limit1 + 1 > limit2)
      throw std::invalid_argument("node " + std::to_string(i) +
                                  ": limit1 + 1 + nback exceeds jobs");
    for (int j = 0; j < I.jobs; j++)
      if (p.prmu[j] >= I.jobs)
        throw std::invalid_argument("node " + std::to_string(i) + ": prmu entry >= jobs");
    int b[MAX_JOBS], e[MAX_JOBS];
    lb1_children_bounds_bi(I.lb1, p.prmu, p.limit1, limit2, b, e);
    for (int k = p.limit1 + 1; k < limit2; k++) {
      lb_begin[i * I.jobs + k] = b[p.prmu[k]];
      lb_end[i * I.jobs + k] = e[p.prmu[k]];
    }
  }
  return py::make_tuple(lb_begin, lb_end);
}

// lb12 twin of pfsp_gpu_bounds_lb12: (dir bytes, bounds) from the host rule.
py::tuple pfsp_cpu_bounds_lb12(int inst, const py::bytes& pool_bytes, int best,
                               const std::string& br_str) {
  PfspInstance I = make_pfsp_instance(inst, 1, branching_from_string(br_str));
  auto nodes = nodes_from_bytes<PFSPNode>(pool_bytes);
  validate_lb12_nodes(nodes, I.jobs);
  std::vector<uint8_t> dir(nodes.size(), 255);
  std::vector<int32_t> bounds(nodes.size() * I.jobs, -1);
  for (size_t i = 0; i < nodes.size(); i++)
    pfsp_lb12_eval(I, nodes[i], best, dir[i], bounds.data() + i * I.jobs);
  return py::make_tuple(py::bytes(reinterpret_cast<const char*>(dir.data()), dir.size()),
                        bounds);
}

py::tuple nq_bfs_frontier(int N, int g, size_t target) {
  Pool<NQNode> pool;
  pool.pushBack(nq_root());
  uint64_t tree = 0, sol = 0;
  // big frontiers (dist tier: every rank builds this redundantly) go through
  // the parallel level-synchronous builder; small ones keep the serial
  // popFront order
  if (target >= 16384)
    nq_bfs_level(N, g, target, pool, tree, sol);
  else
    nq_bfs_until(N, g, target, pool, tree, sol);
  return py::make_tuple(nodes_to_bytes(pool.data(), pool.size()), tree, sol);
}

py::tuple nq_gpu_frontier_py(int N, int g, size_t target, int device) {
  uint64_t tree = 0, sol = 0;
  std::vector<NQNode> nodes;
  {
    py::gil_scoped_release rel;
    nodes = nq_gpu_frontier(N, g, target, device, tree, sol);
  }
  return py::make_tuple(nodes_to_bytes(nodes.data(), nodes.size()), tree, sol);
}

py::tuple pfsp_gpu_frontier_py(int inst, const std::string& lb_str, int ub, size_t target,
                               int device, const std::string& br_str) {
  const LbKind lb = lb_from_string(lb_str);
  const Branching br = branching_from_string(br_str);
  check_branching_supported(lb, br, true);
  PfspInstance I = make_pfsp_instance(inst, ub, br);
  const int lbk =
      (lb == LbKind::LB1_D) ? 0 : (lb == LbKind::LB1 ? 1 : (lb == LbKind::LB12 ? 4 : 2));
  uint64_t tree = 0, sol = 0;
  int best = I.init_ub;
  std::vector<PFSPNode> nodes;
  {
    py::gil_scoped_release rel;
    nodes = pfsp_gpu_frontier(I, lbk, target, device, I.init_ub, tree, sol, best);
  }
  return py::make_tuple(nodes_to_bytes(nodes.data(), nodes.size()), tree, sol, best);
}

py::tuple pfsp_bfs_frontier(int inst, const std::string& lb_str, int ub, size_t target,
                            const std::string& br_str) {
  const LbKind lb = lb_from_string(lb_str);
  const Branching br = branching_from_string(br_str);
  check_branching_supported(lb, br, false);
  PfspInstance I = make_pfsp_instance(inst, ub, br);
  Pool<PFSPNode> pool;
  pool.pushBack(pfsp_root());
  uint64_t tree = 0, sol = 0;
  int best = I.init_ub;
  pfsp_bfs_until(I, lb, target, pool, tree, sol, best);
  return py::make_tuple(nodes_to_bytes(pool.data(), pool.size()), tree, sol, best);
}

// Sequential drain of an explicit frontier (distributed tier's CPU path and
// the phase-3 semantics oracle).
py::dict nqueens_seq_from_pool(const py::bytes& nodes, int N, int g) {
  auto v = nodes_from_bytes<NQNode>(nodes);
  Result r;
  {
    py::gil_scoped_release rel;
    Pool<NQNode> pool;
    pool.pushBackBulk(v.data(), v.size());
    const double t0 = now_sec();
    NQNode parent;
    while (pool.popBack(parent)) nq_decompose(parent, N, g, r.tree, r.sol, pool);
    r.time = now_sec() - t0;
    r.phases.push_back({r.tree, r.sol, r.time});
  }
  return result_to_dict(r);
}

py::dict pfsp_seq_from_pool(const py::bytes& nodes, int inst, const std::string& lb_str,
                            int ub, int best0, const std::string& br_str) {
  auto v = nodes_from_bytes<PFSPNode>(nodes);
  const LbKind lb = lb_from_string(lb_str);
  const Branching br = branching_from_string(br_str);
  check_branching_supported(lb, br, false);
  check_pfsp_pool(v.data(), v.size(), br);
  Result r;
  {
    py::gil_scoped_release rel;
    PfspInstance I = make_pfsp_instance(inst, ub, br);
    int best = (best0 > 0) ? best0 : I.init_ub;
    Pool<PFSPNode> pool;
    pool.pushBackBulk(v.data(), v.size());
    const double t0 = now_sec();
    PFSPNode parent;
    while (pool.popBack(parent)) pfsp_decompose(I, lb, parent, r.tree, r.sol, best, pool);
    r.time = now_sec() - t0;
    r.optimum = best;
    r.phases.push_back({r.tree, r.sol, r.time});
  }
  return result_to_dict(r);
}

// Bounded sequential step: explore up to max_nodes tree nodes of the given
// frontier, then return the remaining pool (checkpointable CPU search; the
// dist tier's CPU mock engine uses it so a stale incumbent is re-read every
// few ms instead of once per whole subtree).
py::tuple pfsp_seq_step(const py::bytes& nodes, int inst, const std::string& lb_str,
                        int ub, int best0, uint64_t max_nodes, const std::string& br_str) {
  auto v = nodes_from_bytes<PFSPNode>(nodes);
  const LbKind lb = lb_from_string(lb_str);
  const Branching br = branching_from_string(br_str);
  check_branching_supported(lb, br, false);
  check_pfsp_pool(v.data(), v.size(), br);
  uint64_t tree = 0, sol = 0;
  int best;
  Pool<PFSPNode> pool;
  {
    py::gil_scoped_release rel;
    PfspInstance I = make_pfsp_instance(inst, ub, br);
    best = (best0 > 0) ? best0 : I.init_ub;
    pool.pushBackBulk(v.data(), v.size());
    PFSPNode parent;
    while (tree < max_nodes && pool.popBack(parent))
      pfsp_decompose(I, lb, parent, tree, sol, best, pool);
  }
  return py::make_tuple(tree, sol, best, nodes_to_bytes(pool.data(), pool.size()));
}

// Single devpool iteration on a chosen pool (kernel-level tests). M defaults
// to the pool length and capacity to the frontier builders' sizing rule.
unsigned long long step_arg(const py::object& o, unsigned long long dflt, const char* name) {
  if (o.is_none()) return dflt;
  const long long v = o.cast<long long>();
  if (v < 0) throw std::invalid_argument(std::string(name) + " must be >= 0");
  return static_cast<unsigned long long>(v);
}

py::dict step_ctl_to_dict(const DevpoolStepCtl& c) {
  py::dict d;
  d["size"] = c.size;
  d["chunk"] = c.chunk;
  d["tree"] = c.tree;
  d["sol"] = c.sol;
  d["iters"] = c.iters;
  d["best"] = c.best;
  d["overflow"] = c.overflow;
  return d;
}

py::tuple nq_devpool_step_py(const py::bytes& nodes, int N, int g, int finish, long long m,
                             const py::object& M, const py::object& capacity,
                             const std::string& presum, int device, int split, int refill,
                             int stack, int stack_cap) {
  auto v = nodes_from_bytes<NQNode>(nodes);
  if (m < 0) throw std::invalid_argument("m must be >= 1");
  const unsigned long long Mv = step_arg(M, v.empty() ? 1 : v.size(), "M");
  const unsigned long long cap = step_arg(capacity, v.size() * (MAX_JOBS + 1) + 64, "capacity");
  DevpoolStepCtl c;
  {
    py::gil_scoped_release rel;
    c = nq_devpool_step(v, N, g, {finish, split, refill, stack, stack_cap},
                        static_cast<unsigned long long>(m), Mv, cap, presum, device);
  }
  return py::make_tuple(nodes_to_bytes(v.data(), v.size()), step_ctl_to_dict(c));
}

py::tuple pfsp_devpool_step_py(const py::bytes& nodes, int inst, const std::string& lb,
                               int best, long long m, const py::object& M,
                               const py::object& capacity, int geom,
                               const std::string& presum, int device,
                               const std::string& br) {
  auto v = nodes_from_bytes<PFSPNode>(nodes);
  if (m < 0) throw std::invalid_argument("m must be >= 1");
  const unsigned long long Mv = step_arg(M, v.empty() ? 1 : v.size(), "M");
  const unsigned long long cap = step_arg(capacity, v.size() * (MAX_JOBS + 1) + 64, "capacity");
  DevpoolStepCtl c;
  {
    py::gil_scoped_release rel;
    c = pfsp_devpool_step(v, inst, lb, best, static_cast<unsigned long long>(m), Mv, cap,
                          geom, presum, device, br);
  }
  return py::make_tuple(nodes_to_bytes(v.data(), v.size()), step_ctl_to_dict(c));
}

// k devpool iterations over one set of buffers (kernel-level tests): a list of
// (pool bytes, ctl dict) snapshots, one per iteration.
std::vector<unsigned long long> chain_windows(const std::vector<long long>& windows) {
  std::vector<unsigned long long> w;
  for (long long v : windows) {
    if (v < 1) throw std::invalid_argument("every window must be >= 1");
    w.push_back(static_cast<unsigned long long>(v));
  }
  return w;
}

template <class NodeT>
py::list chain_to_list(const std::vector<DevpoolSnapshot<NodeT>>& snaps) {
  py::list out;
  for (const auto& s : snaps)
    out.append(py::make_tuple(nodes_to_bytes(s.nodes.data(), s.nodes.size()),
                              step_ctl_to_dict(s.ctl)));
  return out;
}

py::list nq_devpool_chain_py(const py::bytes& nodes, int N, const std::vector<long long>& windows,
                             int g, int finish, long long m, const py::object& capacity,
                             const std::string& presum, int device, int split, int refill,
                             int stack, int stack_cap) {
  auto v = nodes_from_bytes<NQNode>(nodes);
  if (m < 0) throw std::invalid_argument("m must be >= 1");
  const auto w = chain_windows(windows);
  const unsigned long long cap = step_arg(capacity, v.size() * (MAX_JOBS + 1) + 64, "capacity");
  std::vector<DevpoolSnapshot<NQNode>> snaps;
  {
    py::gil_scoped_release rel;
    snaps = nq_devpool_chain(v, N, g, {finish, split, refill, stack, stack_cap},
                             static_cast<unsigned long long>(m), w, cap, presum, device);
  }
  return chain_to_list(snaps);
}

py::list pfsp_devpool_chain_py(const py::bytes& nodes, int inst, const std::string& lb,
                               int best, const std::vector<long long>& windows, long long m,
                               const py::object& capacity, int geom, const std::string& presum,
                               int device, const std::string& br) {
  auto v = nodes_from_bytes<PFSPNode>(nodes);
  if (m < 0) throw std::invalid_argument("m must be >= 1");
  const auto w = chain_windows(windows);
  const unsigned long long cap = step_arg(capacity, v.size() * (MAX_JOBS + 1) + 64, "capacity");
  std::vector<DevpoolSnapshot<PFSPNode>> snaps;
  {
    py::gil_scoped_release rel;
    snaps = pfsp_devpool_chain(v, inst, lb, best, static_cast<unsigned long long>(m), w, cap,
                               geom, presum, device, br);
  }
  return chain_to_list(snaps);
}

// One slice through the real slice thread and loop driver (driver-level
// tests): totals, leftovers, diag counters and the driver's trace as a list of
// dicts ("kind" is "run", "batch" or "spill"; engine_gpu.hpp has the fields).
template <class NodeT>
py::dict loop_out_to_dict(const DevpoolLoopOut<NodeT>& o) {
  py::dict d;
  d["tree"] = o.tree;
  d["sol"] = o.sol;
  d["best"] = o.best;
  d["iters"] = o.iters;
  d["leftover"] = nodes_to_bytes(o.leftover.data(), o.leftover.size());
  d["diag"] = result_to_dict(o.diag)["diag"];
  py::list trace;
  for (const DevLoopRec& r : o.trace.recs) {
    py::dict t;
    const py::bytes nodes(reinterpret_cast<const char*>(r.nodes.data()), r.nodes.size());
    if (r.kind == DevLoopRec::RUN) {
      t["kind"] = "run";
      t["from_spill"] = r.from_spill;
      t["init_size"] = r.size_before;
      t["leftover"] = r.size_after;
      t["best"] = r.best;
    } else if (r.kind == DevLoopRec::DONATE) {
      t["kind"] = "donate";
      t["size_before"] = r.size_before;
      t["size_after"] = r.size_after;
      t["best"] = r.best;
      t["taken"] = r.outcome == static_cast<int>(Donation::TAKEN);
      t["withdrawn"] = r.outcome == static_cast<int>(Donation::WITHDRAWN);
      t["moved"] = nodes;
    } else if (r.kind == DevLoopRec::TAKE) {
      t["kind"] = "take";
      t["size"] = r.size_before;
      t["best"] = r.best;
      t["nodes"] = nodes;
    } else if (r.kind == DevLoopRec::SPILL) {
      t["kind"] = "spill";
      t["size_before"] = r.size_before;
      t["size_after"] = r.size_after;
      t["moved"] = nodes;
    } else {
      t["kind"] = "batch";
      t["b"] = r.b;
      t["parity"] = r.parity;
      t["graph"] = r.graph;
      t["captured"] = r.captured;
      t["size_before"] = r.size_before;
      t["ctl"] = step_ctl_to_dict(r.ctl);
      t["pool"] = nodes;
    }
    trace.append(t);
  }
  d["trace"] = trace;
  return d;
}

unsigned long long loop_arg(long long v, const char* name) {
  if (v < 0) throw std::invalid_argument(std::string(name) + " must be >= 0");
  return static_cast<unsigned long long>(v);
}

py::dict nq_devpool_loop_py(const py::bytes& nodes, int N, int g, int finish, long long m,
                            long long chunk, long long capacity, bool graph,
                            long long max_batches, int device) {
  auto v = nodes_from_bytes<NQNode>(nodes);
  const unsigned long long mv = loop_arg(m, "m"), cv = loop_arg(chunk, "chunk"),
                           cap = loop_arg(capacity, "capacity");
  validate_devpool_loop(v.size(), cv, cap, max_batches);
  DevpoolLoopOut<NQNode> o;
  {
    py::gil_scoped_release rel;
    o = nq_devpool_loop(v, N, g, finish, mv, cv, cap, graph, static_cast<int>(max_batches),
                        device);
  }
  return loop_out_to_dict(o);
}

py::dict pfsp_devpool_loop_py(const py::bytes& nodes, int inst, const std::string& lb, int best,
                              long long m, long long chunk, long long capacity, bool graph,
                              long long max_batches, const std::string& br,
                              const py::object& lower_best_at, int device) {
  auto v = nodes_from_bytes<PFSPNode>(nodes);
  const unsigned long long mv = loop_arg(m, "m"), cv = loop_arg(chunk, "chunk"),
                           cap = loop_arg(capacity, "capacity");
  validate_devpool_loop(v.size(), cv, cap, max_batches);
  long long lower_at = -1;
  int lower_to = 0;
  if (!lower_best_at.is_none()) {
    const auto kv = lower_best_at.cast<std::pair<long long, int>>();
    if (kv.first < 0) throw std::invalid_argument("lower_best_at: batch must be >= 0");
    lower_at = kv.first;
    lower_to = kv.second;
  }
  DevpoolLoopOut<PFSPNode> o;
  {
    py::gil_scoped_release rel;
    o = pfsp_devpool_loop(v, inst, lb, best, mv, cv, cap, graph, static_cast<int>(max_batches),
                          br, lower_at, lower_to, device);
  }
  return loop_out_to_dict(o);
}

// Exercises pool push/pop/bulk semantics from C++ (unit-test helper).
py::dict pool_selftest() {
  py::dict d;
  Pool<NQNode> p;
  NQNode n = nq_root();
  for (int i = 0; i < 3000; i++) {
    n.depth = static_cast<uint8_t>(i % 20);
    p.pushBack(n);
  }
  d["size_after_push"] = p.size();
  NQNode out;
  bool ok = p.popFront(out);
  d["pop_front_ok"] = ok;
  d["front_depth"] = static_cast<int>(out.depth);
  ok = p.popBack(out);
  d["pop_back_ok"] = ok;
  d["back_depth"] = static_cast<int>(out.depth);
  std::vector<NQNode> buf(5000);
  d["bulk_below_m"] = p.popBackBulk(100000, 5000, buf.data());  // size < m -> 0
  d["bulk"] = p.popBackBulk(10, 500, buf.data());               // -> 500
  d["size_final"] = p.size();
  return d;
}

// `threads` slice threads over one SliceShare (driver-level tests): a list of
// loop_out_to_dict results, one per thread.
template <class NodeT>
py::list share_outs_to_list(const std::vector<DevpoolLoopOut<NodeT>>& outs) {
  py::list l;
  for (const auto& o : outs) l.append(loop_out_to_dict(o));
  return l;
}

py::list nq_devpool_share_py(const py::bytes& nodes, int N, int g, int finish, long long m,
                             long long chunk, long long capacity, long long max_batches,
                             int threads, long long donate_floor, long long await_idle_ms,
                             int device) {
  auto v = nodes_from_bytes<NQNode>(nodes);
  const unsigned long long mv = loop_arg(m, "m"), cv = loop_arg(chunk, "chunk"),
                           cap = loop_arg(capacity, "capacity");
  validate_devpool_loop(v.size(), cv, cap, max_batches);
  validate_devpool_share(threads, donate_floor, await_idle_ms);
  std::vector<DevpoolLoopOut<NQNode>> o;
  {
    py::gil_scoped_release rel;
    o = nq_devpool_share(v, N, g, finish, mv, cv, cap, static_cast<int>(max_batches), threads,
                         static_cast<unsigned long long>(donate_floor),
                         static_cast<int>(await_idle_ms), device);
  }
  return share_outs_to_list(o);
}

py::list pfsp_devpool_share_py(const py::bytes& nodes, int inst, const std::string& lb, int best,
                               long long m, long long chunk, long long capacity,
                               long long max_batches, const std::string& br, int threads,
                               long long donate_floor, long long await_idle_ms, int device) {
  auto v = nodes_from_bytes<PFSPNode>(nodes);
  const unsigned long long mv = loop_arg(m, "m"), cv = loop_arg(chunk, "chunk"),
                           cap = loop_arg(capacity, "capacity");
  validate_devpool_loop(v.size(), cv, cap, max_batches);
  validate_devpool_share(threads, donate_floor, await_idle_ms);
  std::vector<DevpoolLoopOut<PFSPNode>> o;
  {
    py::gil_scoped_release rel;
    o = pfsp_devpool_share(v, inst, lb, best, mv, cv, cap, static_cast<int>(max_batches), br,
                           threads, static_cast<unsigned long long>(donate_floor),
                           static_cast<int>(await_idle_ms), device);
  }
  return share_outs_to_list(o);
}

// The donation protocol (slice_share.hpp) on plain threads over a fake pool
// (unit-test helper); the scenarios are in share_selftest.hpp.
py::dict share_out_to_dict(const share_test::Out& o) {
  py::dict d;
  py::list offers, takes;
  for (const auto& f : o.offers) {
    py::dict t;
    static const char* names[] = {"none", "taken", "withdrawn", "abandoned"};
    t["outcome"] = names[f.outcome];
    t["set_calls"] = f.set_calls;
    t["size_after"] = f.size_after;
    t["idle_after"] = f.idle_after;
    offers.append(t);
  }
  for (const auto& k : o.takes) takes.append(py::make_tuple(k.thief, k.offset, k.n, k.best));
  d["offers"] = offers;
  d["takes"] = takes;
  d["returned_false"] = o.returned_false;
  d["idle_reached"] = o.idle_reached;
  d["ms"] = o.ms;
  return d;
}

py::dict share_selftest(const std::string& scenario, unsigned long long size,
                        unsigned long long floor_sz, int thieves, int offers, bool pending,
                        bool overflow, int best, bool one_each, unsigned long long size_b,
                        int deadline_ms, int runners, bool by_exception) {
  if (size > (1ull << 24) || size_b > (1ull << 24) || thieves < 0 || thieves > 8 || offers < 0 ||
      offers > 64 || runners < 1 || runners > 8 || deadline_ms < 1 || deadline_ms > 2000)
    throw std::invalid_argument("share_selftest: argument out of range");
  share_test::Out o;
  {
    py::gil_scoped_release rel;
    if (scenario == "basic")
      o = share_test::basic(size, floor_sz, thieves, offers, pending, overflow, best, one_each);
    else if (scenario == "two_donors")
      o = share_test::two_donors(size, size_b, floor_sz);
    else if (scenario == "withdraw")
      o = share_test::withdraw(size, floor_sz);
    else if (scenario == "deadline")
      o = share_test::deadline(size, floor_sz, deadline_ms);
    else if (scenario == "termination")
      o = share_test::termination(runners, by_exception);
    else
      throw std::invalid_argument("share_selftest: unknown scenario");
  }
  return share_out_to_dict(o);
}

}  // namespace

PYBIND11_MODULE(_core, mod) {
  mod.doc() = "MI355X-native tree-search core (N-Queens + PFSP B&B)";

  mod.def("taillard_nb_jobs", &taillard_nb_jobs);
  mod.def("taillard_nb_machines", &taillard_nb_machines);
  mod.def("taillard_best_ub", &taillard_best_ub);
  mod.def("taillard_processing_times", &taillard_processing_times);

  mod.def("nqueens_seq",
          [](int N, int g) {
            Result r;
            {
              py::gil_scoped_release rel;
              r = nqueens_seq(N, g);
            }
            return result_to_dict(r);
          },
          py::arg("N") = 14, py::arg("g") = 1);
  mod.def("pfsp_seq",
          [](int inst, const std::string& lb, int ub, const std::string& br) {
            Result r;
            {
              py::gil_scoped_release rel;
              r = pfsp_seq(inst, lb, ub, br);
            }
            return result_to_dict(r);
          },
          py::arg("inst") = 14, py::arg("lb") = "lb1", py::arg("ub") = 1,
          py::arg("br") = "fwd");

  mod.def("gpu_device_count", &gpu_device_count);

  mod.def("nqueens_multigpu",
          [](int N, int g, int m, int M, int D, const std::string& eval, double perc,
             unsigned long long capacity) {
            Result r;
            {
              py::gil_scoped_release rel;
              r = nqueens_multigpu(N, g, m, M, D, eval, perc, capacity);
            }
            return result_to_dict(r);
          },
          py::arg("N") = 14, py::arg("g") = 1, py::arg("m") = 25, py::arg("M") = 50000,
          py::arg("D") = 1, py::arg("eval") = "gpu", py::arg("perc") = 0.5,
          py::arg("capacity") = (1ull << 27));
  mod.def("pfsp_multigpu",
          [](int inst, const std::string& lb, int ub, int m, int M, int D,
             const std::string& eval, bool share_best, double perc,
             unsigned long long capacity, const std::string& br) {
            Result r;
            {
              py::gil_scoped_release rel;
              r = pfsp_multigpu(inst, lb, ub, m, M, D, eval, share_best, perc, capacity, br);
            }
            return result_to_dict(r);
          },
          py::arg("inst") = 14, py::arg("lb") = "lb1", py::arg("ub") = 1, py::arg("m") = 25,
          py::arg("M") = 50000, py::arg("D") = 1, py::arg("eval") = "gpu",
          py::arg("share_best") = false, py::arg("perc") = 0.5,
          py::arg("capacity") = (1ull << 27), py::arg("br") = "fwd");

  mod.def("nqueens_gpu",
          [](int N, int g, int m, int M, int device, const std::string& mode,
             unsigned long long capacity) {
            Result r;
            {
              py::gil_scoped_release rel;
              r = nqueens_gpu(N, g, m, M, device, mode, capacity);
            }
            return result_to_dict(r);
          },
          py::arg("N") = 14, py::arg("g") = 1, py::arg("m") = 25, py::arg("M") = 50000,
          py::arg("device") = 0, py::arg("mode") = "devpool",
          py::arg("capacity") = (1ull << 27));

  mod.def("pfsp_gpu",
          [](int inst, const std::string& lb, int ub, int m, int M, int device,
             const std::string& mode, unsigned long long capacity, const std::string& br) {
            Result r;
            {
              py::gil_scoped_release rel;
              r = pfsp_gpu(inst, lb, ub, m, M, device, mode, capacity, br);
            }
            return result_to_dict(r);
          },
          py::arg("inst") = 14, py::arg("lb") = "lb1", py::arg("ub") = 1, py::arg("m") = 25,
          py::arg("M") = 50000, py::arg("device") = 0, py::arg("mode") = "devpool",
          py::arg("capacity") = (1ull << 27), py::arg("br") = "fwd");

  mod.def("nqueens_gpu_rooted",
          [](int N, int g, int M, int device, unsigned long long capacity) {
            Result r;
            {
              py::gil_scoped_release rel;
              r = nqueens_gpu_rooted(N, g, M, device, capacity);
            }
            return result_to_dict(r);
          },
          py::arg("N") = 14, py::arg("g") = 1, py::arg("M") = 50000,
          py::arg("device") = 0, py::arg("capacity") = (1ull << 27));

  mod.def("pfsp_gpu_rooted",
          [](int inst, const std::string& lb, int ub, int M, int device,
             unsigned long long capacity, const std::string& br) {
            Result r;
            {
              py::gil_scoped_release rel;
              r = pfsp_gpu_rooted(inst, lb, ub, M, device, capacity, br);
            }
            return result_to_dict(r);
          },
          py::arg("inst") = 14, py::arg("lb") = "lb1", py::arg("ub") = 1,
          py::arg("M") = 50000, py::arg("device") = 0,
          py::arg("capacity") = (1ull << 27), py::arg("br") = "fwd");

  mod.def("nqueens_gpu_from_pool",
          [](const py::bytes& nodes, int N, int g, int m, int M, int device,
             const std::string& mode, unsigned long long capacity) {
            auto v = nodes_from_bytes<NQNode>(nodes);
            Result r;
            {
              py::gil_scoped_release rel;
              r = nqueens_gpu_from_pool(v, N, g, m, M, device, mode, capacity);
            }
            return result_to_dict(r);
          },
          py::arg("nodes"), py::arg("N"), py::arg("g") = 1, py::arg("m") = 25,
          py::arg("M") = 50000, py::arg("device") = 0, py::arg("mode") = "devpool",
          py::arg("capacity") = (1ull << 27));

  mod.def("pfsp_gpu_from_pool",
          [](const py::bytes& nodes, int inst, const std::string& lb, int ub, int best0,
             int m, int M, int device, const std::string& mode,
             unsigned long long capacity, const std::string& br) {
            auto v = nodes_from_bytes<PFSPNode>(nodes);
            Result r;
            {
              py::gil_scoped_release rel;
              r = pfsp_gpu_from_pool(v, inst, lb, ub, best0, m, M, device, mode, capacity,
                                     br);
            }
            return result_to_dict(r);
          },
          py::arg("nodes"), py::arg("inst"), py::arg("lb") = "lb1", py::arg("ub") = 1,
          py::arg("best0") = 0, py::arg("m") = 25, py::arg("M") = 50000,
          py::arg("device") = 0, py::arg("mode") = "devpool",
          py::arg("capacity") = (1ull << 27), py::arg("br") = "fwd");

  mod.def("pfsp_seq_step", &pfsp_seq_step, py::arg("nodes"), py::arg("inst"),
          py::arg("lb") = "lb1", py::arg("ub") = 1, py::arg("best0") = 0,
          py::arg("max_nodes") = 50000, py::arg("br") = "fwd");
  mod.def("nqueens_seq_from_pool", &nqueens_seq_from_pool, py::arg("nodes"), py::arg("N"),
          py::arg("g") = 1);
  mod.def("pfsp_seq_from_pool", &pfsp_seq_from_pool, py::arg("nodes"), py::arg("inst"),
          py::arg("lb") = "lb1", py::arg("ub") = 1, py::arg("best0") = 0,
          py::arg("br") = "fwd");

  mod.def("nq_bfs_frontier", &nq_bfs_frontier, py::arg("N"), py::arg("g") = 1,
          py::arg("target") = 1024);
  mod.def("pfsp_bfs_frontier", &pfsp_bfs_frontier, py::arg("inst"), py::arg("lb") = "lb1",
          py::arg("ub") = 1, py::arg("target") = 1024, py::arg("br") = "fwd");
  mod.def("nq_gpu_frontier", &nq_gpu_frontier_py, py::arg("N"), py::arg("g") = 1,
          py::arg("target") = 1024, py::arg("device") = 0);
  mod.def("pfsp_gpu_frontier", &pfsp_gpu_frontier_py, py::arg("inst"),
          py::arg("lb") = "lb1", py::arg("ub") = 1, py::arg("target") = 1024,
          py::arg("device") = 0, py::arg("br") = "fwd");

  mod.def("nq_cpu_labels", &nq_cpu_labels);
  mod.def("nq_finish_count_cpu", &nq_finish_count_cpu, py::arg("cols"), py::arg("d1"),
          py::arg("d2"), py::arg("row"), py::arg("N"));
  mod.def("nq_finish_block_cpu", &nq_finish_block_cpu, py::arg("jobs"), py::arg("N"),
          py::arg("g") = 1, py::arg("split") = NQ_SPLIT_DEFAULT,
          py::arg("qcap") = NQ_SPLIT_QCAP);
  mod.def("nq_sub_encode", &nq_sub_encode, py::arg("ref"), py::arg("ncols"), py::arg("c1"),
          py::arg("c2"));
  mod.def("nq_sub_decode", &nq_sub_decode_py, py::arg("entry"));
  mod.def("nq_split_default", &nq_split_default);
  mod.def("nq_finish_wave_cpu", &nq_finish_wave_cpu, py::arg("jobs"), py::arg("N"),
          py::arg("g") = 1, py::arg("split") = NQ_SPLIT_DEFAULT,
          py::arg("qcap") = NQ_SPLIT_QCAP, py::arg("refill") = NQ_REFILL_DEFAULT,
          py::arg("lanes") = 64, py::arg("waves") = 4);
  mod.def("nq_pmask_pack", &nq_pmask_pack, py::arg("cols"), py::arg("d1"), py::arg("d2"));
  mod.def("nq_pmask_unpack", &nq_pmask_unpack_py, py::arg("word"));
  mod.def("nq_job_ref", &nq_job_ref, py::arg("parent"), py::arg("col"));
  mod.def("nq_job_state", &nq_job_state_py, py::arg("word"), py::arg("ref"), py::arg("N"));
  mod.def("nq_finish_stack_cpu", &nq_finish_stack_cpu, py::arg("jobs"), py::arg("N"),
          py::arg("g") = 1, py::arg("refill") = NQ_REFILL_DEFAULT, py::arg("waves") = 4,
          py::arg("lanes") = 64, py::arg("cap") = NQ_STACK_CAP);
  mod.def("nq_entry_pack", &nq_entry_pack, py::arg("cols"), py::arg("d1"), py::arg("d2"),
          py::arg("h"));
  mod.def("nq_entry_unpack", &nq_entry_unpack_py, py::arg("word"));
  mod.def("nq_stack_default", &nq_stack_default);
  mod.attr("NQ_STACK_CAP") = NQ_STACK_CAP;
  mod.def("nq_refill_default", &nq_refill_default);
  mod.attr("NQ_REFILL_DEFAULT") = NQ_REFILL_DEFAULT;
  mod.attr("NQ_SPLIT_QCAP") = NQ_SPLIT_QCAP;
  mod.attr("NQ_SPLIT_MAX") = NQ_SPLIT_MAX;
  mod.def("pfsp_cpu_bounds", &pfsp_cpu_bounds);
  mod.def("pfsp_cpu_bounds_bi", &pfsp_cpu_bounds_bi, py::arg("inst"), py::arg("nodes"));
  mod.def("pfsp_gpu_bounds_bi",
          [](int inst, const py::bytes& nodes, int device) {
            auto v = nodes_from_bytes<PFSPNode>(nodes);
            auto r = pfsp_gpu_bounds_bi(inst, v, device);
            return py::make_tuple(r.first, r.second);
          },
          py::arg("inst"), py::arg("nodes"), py::arg("device") = 0);
  mod.def("pfsp_cpu_bounds_lb12", &pfsp_cpu_bounds_lb12, py::arg("inst"), py::arg("nodes"),
          py::arg("best"), py::arg("br"));
  mod.def("pfsp_gpu_bounds_lb12",
          [](int inst, const py::bytes& nodes, int best, const std::string& br, int device) {
            auto v = nodes_from_bytes<PFSPNode>(nodes);
            auto r = pfsp_gpu_bounds_lb12(inst, v, best, br, device);
            return py::make_tuple(
                py::bytes(reinterpret_cast<const char*>(r.first.data()), r.first.size()),
                r.second);
          },
          py::arg("inst"), py::arg("nodes"), py::arg("best"), py::arg("br"),
          py::arg("device") = 0);
  mod.def("nq_gpu_labels",
          [](int N, int g, const py::bytes& nodes, int device) {
            auto v = nodes_from_bytes<NQNode>(nodes);
            auto labels = nq_gpu_labels(N, g, v, device);
            return py::bytes(reinterpret_cast<const char*>(labels.data()), labels.size());
          },
          py::arg("N"), py::arg("g"), py::arg("nodes"), py::arg("device") = 0);
  mod.def("pfsp_gpu_bounds",
          [](int inst, const std::string& lb, const py::bytes& nodes, int best, int device) {
            auto v = nodes_from_bytes<PFSPNode>(nodes);
            return pfsp_gpu_bounds(inst, lb, v, best, device);
          },
          py::arg("inst"), py::arg("lb"), py::arg("nodes"), py::arg("best"),
          py::arg("device") = 0);

  mod.def("nq_devpool_step", &nq_devpool_step_py, py::arg("nodes"), py::arg("N"),
          py::arg("g") = 1, py::arg("finish") = 8, py::arg("m") = 1,
          py::arg("M") = py::none(), py::arg("capacity") = py::none(),
          py::arg("presum") = "auto", py::arg("device") = 0, py::arg("split") = -1,
          py::arg("refill") = -1, py::arg("stack") = -1, py::arg("stack_cap") = -1);
  mod.def("pfsp_devpool_step", &pfsp_devpool_step_py, py::arg("nodes"), py::arg("inst"),
          py::arg("lb"), py::arg("best"), py::arg("m") = 1, py::arg("M") = py::none(),
          py::arg("capacity") = py::none(), py::arg("geom") = -1,
          py::arg("presum") = "auto", py::arg("device") = 0, py::arg("br") = "fwd");
  mod.def("nq_devpool_chain", &nq_devpool_chain_py, py::arg("nodes"), py::arg("N"),
          py::arg("windows"), py::arg("g") = 1, py::arg("finish") = 8, py::arg("m") = 1,
          py::arg("capacity") = py::none(), py::arg("presum") = "auto",
          py::arg("device") = 0, py::arg("split") = -1, py::arg("refill") = -1,
          py::arg("stack") = -1, py::arg("stack_cap") = -1);
  mod.def("pfsp_devpool_chain", &pfsp_devpool_chain_py, py::arg("nodes"), py::arg("inst"),
          py::arg("lb"), py::arg("best"), py::arg("windows"), py::arg("m") = 1,
          py::arg("capacity") = py::none(), py::arg("geom") = -1,
          py::arg("presum") = "auto", py::arg("device") = 0, py::arg("br") = "fwd");
  mod.def("nq_devpool_loop", &nq_devpool_loop_py, py::arg("nodes"), py::arg("N"),
          py::arg("g") = 1, py::arg("finish") = 8, py::arg("m") = 25, py::arg("chunk") = 256,
          py::arg("capacity") = 1 << 16, py::arg("graph") = true,
          py::arg("max_batches") = 0, py::arg("device") = 0);
  mod.def("pfsp_devpool_loop", &pfsp_devpool_loop_py, py::arg("nodes"), py::arg("inst"),
          py::arg("lb"), py::arg("best"), py::arg("m") = 25, py::arg("chunk") = 256,
          py::arg("capacity") = 1 << 16, py::arg("graph") = true,
          py::arg("max_batches") = 0, py::arg("br") = "fwd",
          py::arg("lower_best_at") = py::none(), py::arg("device") = 0);

  mod.def("nq_devpool_share", &nq_devpool_share_py, py::arg("nodes"), py::arg("N"),
          py::arg("g") = 1, py::arg("finish") = 8, py::arg("m") = 25, py::arg("chunk") = 256,
          py::arg("capacity") = 1 << 16, py::arg("max_batches") = 0, py::arg("threads") = 2,
          py::arg("donate_floor") = 0, py::arg("await_idle_ms") = 0, py::arg("device") = 0);
  mod.def("pfsp_devpool_share", &pfsp_devpool_share_py, py::arg("nodes"), py::arg("inst"),
          py::arg("lb"), py::arg("best"), py::arg("m") = 25, py::arg("chunk") = 256,
          py::arg("capacity") = 1 << 16, py::arg("max_batches") = 0, py::arg("br") = "fwd",
          py::arg("threads") = 2, py::arg("donate_floor") = 0, py::arg("await_idle_ms") = 0,
          py::arg("device") = 0);

  mod.def("pool_selftest", &pool_selftest);
  // The loop driver's planner (devpool_loop_plan.hpp), read-only; no GPU needed.
  mod.attr("LOOP_BATCH") = LOOP_BATCH;
  mod.attr("LOOP_EAGER_BATCHES") = LOOP_EAGER_BATCHES;
  mod.attr("LOOP_SMALL_POOL") = LOOP_SMALL_POOL;
  mod.def(
      "devpool_plan_batch",
      [](unsigned long long m, int per, unsigned long long growth, unsigned long long capacity,
         unsigned long long stop_size, unsigned long long size, int batches,
         bool can_spill) -> py::object {
        DevLoopShape c;
        c.m = m;
        c.per = per;
        c.growth = growth;
        c.capacity = capacity;
        c.stop_size = stop_size;
        const int b = plan_batch(c, size, batches, can_spill);
        return b ? py::object(py::int_(b)) : py::object(py::str("spill"));
      },
      py::arg("m"), py::arg("per"), py::arg("growth"), py::arg("capacity"),
      py::arg("stop_size"), py::arg("size"), py::arg("batches"), py::arg("can_spill"));
  mod.def(
      "devpool_plan_graph",
      [](bool allowed, int batches, bool have_exec, int b, int par) {
        static const char* names[] = {"eager", "capture", "replay"};
        return names[static_cast<int>(plan_graph(allowed, batches, have_exec, b, par))];
      },
      py::arg("allowed"), py::arg("batches"), py::arg("have_exec"), py::arg("b"),
      py::arg("par"));
  mod.def("donation_floor", &donation_floor, py::arg("m"));
  mod.def("share_selftest", &share_selftest, py::arg("scenario"), py::arg("size") = 0,
          py::arg("floor") = 0, py::arg("thieves") = 1, py::arg("offers") = 1,
          py::arg("pending") = false, py::arg("overflow") = false, py::arg("best") = 0,
          py::arg("one_each") = false, py::arg("size_b") = 0, py::arg("deadline_ms") = 40,
          py::arg("runners") = 1, py::arg("by_exception") = false);
  // pure policy helpers (CPU-unit-testable): kernel geometry selection and
  // the devpool expansion-chunk clamp
  mod.def("devpool_lbk_geom", &devpool_lbk_geom, py::arg("lbk"), py::arg("machines"));
  mod.def("devpool_grid", &devpool_grid, py::arg("M"), py::arg("per"), py::arg("lbk"));
  mod.def("devpool_stride", &devpool_stride, py::arg("lbk"));

  py::class_<PfspAsyncEngine>(mod, "PfspAsyncEngine",
                              "Persistent per-rank PFSP devpool engine: successive "
                              "frontier submits, shared incumbent (mid-search RCCL UB "
                              "exchange), engine-pausing work extraction for inter-rank "
                              "steals")
      .def(py::init([](const py::bytes& nodes, int inst, const std::string& lb, int ub,
                       int best0, int m, int M, int device, unsigned long long capacity,
                       const std::string& br) {
             return new PfspAsyncEngine(nodes_from_bytes<PFSPNode>(nodes), inst, lb, ub,
                                        best0, m, M, device, capacity, br);
           }),
           py::arg("nodes"), py::arg("inst"), py::arg("lb") = "lb1", py::arg("ub") = 1,
           py::arg("best0") = 0, py::arg("m") = 25, py::arg("M") = 50000,
           py::arg("device") = 0, py::arg("capacity") = (1ull << 24),
           py::arg("br") = "fwd")
      .def(py::init([](int inst, const std::string& lb, int ub, int m, int M, int device,
                       unsigned long long capacity, const std::string& br) {
             return new PfspAsyncEngine(inst, lb, ub, m, M, device, capacity, br);
           }),
           py::arg("inst"), py::arg("lb") = "lb1", py::arg("ub") = 1, py::arg("m") = 25,
           py::arg("M") = 50000, py::arg("device") = 0,
           py::arg("capacity") = (1ull << 24), py::arg("br") = "fwd")
      .def("submit",
           [](PfspAsyncEngine& e, const py::bytes& nodes, int best0) {
             e.submit(nodes_from_bytes<PFSPNode>(nodes), best0);
           },
           py::arg("nodes"), py::arg("best0") = 0)
      .def("best", &PfspAsyncEngine::best)
      .def("update_best", &PfspAsyncEngine::update_best)
      .def("done", &PfspAsyncEngine::done)
      .def("pool_size", &PfspAsyncEngine::pool_size)
      .def("request_extract", &PfspAsyncEngine::request_extract)
      .def("extract_ready", &PfspAsyncEngine::extract_ready)
      .def("extract_pending", &PfspAsyncEngine::extract_pending)
      .def("take_extract",
           [](PfspAsyncEngine& e) {
             auto v = e.take_extract();
             return nodes_to_bytes(v.data(), v.size());
           })
      .def("join", [](PfspAsyncEngine& e) {
        Result r;
        {
          py::gil_scoped_release rel;
          r = e.join();
        }
        return result_to_dict(r);
      });
}
