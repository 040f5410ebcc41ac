// Single-GPU 3-phase search engines for MI355X.
//
// Phase structure parity: reference pfsp_gpu_chpl.chpl:306-431 /
// nqueens_gpu_chpl.chpl:152-248 (phase 1 CPU BFS until size >= m; phase 2
// chunked m/M offload; phase 3 CPU DFS drain).
//
// Two phase-2 modes:
//   "hostpool": the reference's architecture, done right for MI355X — pinned
//       host buffers, async prefix-only copies (the Chapel version copies the
//       full M-element arrays every iteration, SURVEY.md §8.4 — we don't),
//       one HIP stream, host-side generate_children.
//   "devpool": MI355X-native fast path — pools live in HBM3E; each offload
//       round is an expand-compact + gather kernel pair (kernels.hip), with
//       frontier slices pulled off a queue by a few worker threads on
//       concurrent streams (see devpool_slices); the host polls 48 B
//       control blocks every few iterations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine_gpu.hpp"
#include "engine_internal.hpp"
#include "gpu_api.hpp"
#include "nq_finish.hpp"
#include "search_host.hpp"
#include "slice_share.hpp"
#include "taillard.hpp"

namespace gats {

int gpu_device_count() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return 0;
  return n;
}

// hipSetDevice measured ~0.8 ms PER CALL on ROCm 7.2 even when the thread is
// already on that device (runtime-trace: 63 calls = 52 ms across 21 trivial
// searches); the engines run on pooled threads whose device rarely changes,
// so skip the call unless it would actually switch.
void set_device_cached(int device) {
  static thread_local int tl_device = -1;
  if (tl_device == device) return;
  HIP_CHECK(hipSetDevice(device));
  tl_device = device;
}

namespace {

// Process-level buffer cache: hipMalloc of the multi-GB slice pools costs
// tens of ms, which dominates repeated searches (bench steps, PFSP
// instances) once a search itself is ~100 ms. Buffers are recycled by exact
// (device, size); sizes are deterministic per engine config so the hit rate
// is ~100% after the first search. Freed only at process exit.
struct BufferCache {
  std::mutex mu;
  std::map<std::pair<int, size_t>, std::vector<void*>> dev, pinned;
};
BufferCache& buffer_cache() {
  static BufferCache c;
  return c;
}

}  // namespace

void* cached_dev_alloc(size_t bytes) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  {
    std::lock_guard<std::mutex> l(buffer_cache().mu);
    auto& v = buffer_cache().dev[{dev, bytes}];
    if (!v.empty()) {
      void* p = v.back();
      v.pop_back();
      return p;
    }
  }
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, bytes));
  return p;
}

void cached_dev_free(void* p, size_t bytes) {
  if (!p) return;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> l(buffer_cache().mu);
  buffer_cache().dev[{dev, bytes}].push_back(p);
}

void* cached_pinned_alloc(size_t bytes) {
  {
    std::lock_guard<std::mutex> l(buffer_cache().mu);
    auto& v = buffer_cache().pinned[{0, bytes}];
    if (!v.empty()) {
      void* p = v.back();
      v.pop_back();
      return p;
    }
  }
  void* p = nullptr;
  HIP_CHECK(hipHostMalloc(&p, bytes));
  return p;
}

void cached_pinned_free(void* p, size_t bytes) {
  if (!p) return;
  std::lock_guard<std::mutex> l(buffer_cache().mu);
  buffer_cache().pinned[{0, bytes}].push_back(p);
}

namespace {

template <typename T>
T* dev_alloc(size_t n) {
  return static_cast<T*>(cached_dev_alloc(n * sizeof(T)));
}

template <typename T>
T* dev_upload(const T* src, size_t n) {
  T* d = dev_alloc<T>(n);
  HIP_CHECK(hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

}  // namespace

PfspTablesGuard::PfspTablesGuard(const PfspInstance& I) {
  const int n = I.jobs, m = I.machines;
  std::vector<int16_t> p16(static_cast<size_t>(m) * n);
  for (size_t i = 0; i < p16.size(); i++) p16[i] = static_cast<int16_t>(I.lb1.p_times[i]);
  std::vector<int32_t> mt(I.lb1.min_tails.begin(), I.lb1.min_tails.end());
  const PfspPackedTables pk = build_packed_johnson(I);
  tb.p_times = keep(dev_upload(p16.data(), p16.size()), p16.size() * sizeof(p16[0]));
  tb.min_tails = keep(dev_upload(mt.data(), mt.size()), mt.size() * sizeof(mt[0]));
  tb.johnson_packed =
      keep(dev_upload(pk.jp.data(), pk.jp.size()), pk.jp.size() * sizeof(uint32_t));
  tb.pairs1 = keep(dev_upload(pk.p1.data(), pk.p1.size()), pk.p1.size());
  tb.pairs2 = keep(dev_upload(pk.p2.data(), pk.p2.size()), pk.p2.size());
  tb.johnson_packed_w =
      keep(dev_upload(pk.jp_w.data(), pk.jp_w.size()), pk.jp_w.size() * sizeof(uint32_t));
  tb.pairs1_w = keep(dev_upload(pk.p1_w.data(), pk.p1_w.size()), pk.p1_w.size());
  tb.pairs2_w = keep(dev_upload(pk.p2_w.data(), pk.p2_w.size()), pk.p2_w.size());
  std::vector<int32_t> mh(I.lb1.min_heads.begin(), I.lb1.min_heads.end());
  tb.min_heads = keep(dev_upload(mh.data(), mh.size()), mh.size() * sizeof(mh[0]));
}

PfspTablesGuard::~PfspTablesGuard() {
  for (size_t i = 0; i < allocs.size(); i++) cached_dev_free(allocs[i], alloc_bytes[i]);
}

namespace {

// Parked worker threads reused across searches (the persistent-engine thread
// component): spawning slice threads per search costs ~50-100 us each and the
// dist tier re-arms an engine per frontier claim, so threads park on a
// condvar between tasks instead of being joined. Threads are created on
// demand up to the high-water mark of concurrent tasks; the pool object is
// intentionally leaked so detached workers never touch destroyed statics at
// process exit. HIP device selection is per-thread and every engine task sets
// it on entry, so reuse across devices is safe.
class WorkerPool {
 public:
  static WorkerPool& instance() {
    static WorkerPool* p = new WorkerPool();  // leaked by design
    return *p;
  }
  void submit(std::function<void()> fn) {
    std::lock_guard<std::mutex> l(mu_);
    q_.push_back(std::move(fn));
    // avail_ counts workers inside (or re-acquiring from) cv_.wait: each will
    // take one queued task on its next lock acquisition, so spawn only when
    // the queue outgrew the parked set — never serializes two tasks onto one
    // worker
    if (q_.size() > static_cast<size_t>(avail_)) std::thread([this] { loop(); }).detach();
    cv_.notify_one();
  }

 private:
  void loop() {
    std::unique_lock<std::mutex> l(mu_);
    for (;;) {
      while (q_.empty()) {
        avail_++;
        cv_.wait(l);
        avail_--;
      }
      std::function<void()> fn = std::move(q_.front());
      q_.pop_front();
      l.unlock();
      fn();  // tasks are noexcept by contract (engine lambdas catch all)
      l.lock();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> q_;
  int avail_ = 0;
};

// Run T engine tasks on pooled threads and wait for all of them.
template <class MakeTask>
static void run_on_pool(int T, MakeTask&& make_task) {
  std::atomic<int> remaining{T};
  std::mutex done_mu;
  std::condition_variable done_cv;
  for (int t = 0; t < T; t++) {
    WorkerPool::instance().submit([t, &remaining, &done_mu, &done_cv, &make_task] {
      make_task(t);
      if (remaining.fetch_sub(1, std::memory_order_acq_rel) == 1) {
        std::lock_guard<std::mutex> l(done_mu);
        done_cv.notify_all();
      }
    });
  }
  std::unique_lock<std::mutex> l(done_mu);
  done_cv.wait(l, [&] { return remaining.load(std::memory_order_acquire) == 0; });
}

// Stream recycling is ON by default (round 2): hipStreamCreate/Destroy costs
// up to ~3 ms per stream on an otherwise-idle ROCm 7.2 device, which
// dominated small searches (ta019 lb2: 15 ms -> 1.55 ms with reuse) and cost
// the N=17 bench ~2 ms/step. Round 1 measured reuse 40% SLOWER, but that
// regression disappeared with the round-2 loop (parked worker threads +
// non-blocking streams + async slice copies). GATS_STREAM_CACHE=0 restores
// fresh streams for experiments.
struct StreamCache {
  std::mutex mu;
  std::map<int, std::vector<hipStream_t>> free_;
};
StreamCache& stream_cache() {
  static StreamCache c;
  return c;
}

}  // namespace

bool StreamGuard::caching() {
  static const char* e = std::getenv("GATS_STREAM_CACHE");
  static const bool on = (e == nullptr) || std::string(e) != "0";
  return on;
}

StreamGuard::StreamGuard() {
  (void)hipGetDevice(&dev);
  if (caching()) {
    std::lock_guard<std::mutex> l(stream_cache().mu);
    auto& v = stream_cache().free_[dev];
    if (!v.empty()) {
      s = v.back();
      v.pop_back();
      return;
    }
  }
  HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
}

StreamGuard::~StreamGuard() {
  if (caching()) {
    std::lock_guard<std::mutex> l(stream_cache().mu);
    stream_cache().free_[dev].push_back(s);
  } else {
    (void)hipStreamDestroy(s);
  }
}

// PFSP device bound tables are immutable per instance: build + upload once
// per (device, instance) and share across searches/slices (rebuilding cost a
// visible slice of few-ms searches).
const PfspDevTables& pfsp_tables_cached(const PfspInstance& I, int device) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, PfspTablesGuard*> cache;
  std::lock_guard<std::mutex> l(mu);
  auto key = std::make_pair(device, I.inst);
  auto it = cache.find(key);
  if (it == cache.end())
    it = cache.emplace(key, new PfspTablesGuard(I)).first;  // lives for the process
  return it->second->tb;
}

PfspPackedTables build_packed_johnson(const PfspInstance& I) {
  const int n = I.jobs;
  const int pairs = I.lb2.nb_pairs;
  PfspPackedTables pk;
  pk.p1.resize(pairs);
  pk.p2.resize(pairs);
  // u32 pack (lossless: job < 20, lag <= 20*99 < 2^11, ptm <= 99 < 2^8)
  pk.jp.resize(static_cast<size_t>(pairs) * n);
  for (int k = 0; k < pairs; k++) {
    const int ma0 = I.lb2.pairs1[k], ma1 = I.lb2.pairs2[k];
    pk.p1[k] = static_cast<uint8_t>(ma0);
    pk.p2[k] = static_cast<uint8_t>(ma1);
    for (int j = 0; j < n; j++) {
      const int job = I.lb2.johnson_schedules[static_cast<size_t>(k) * n + j];
      const uint32_t ptm0 = static_cast<uint32_t>(I.lb1.p_times[ma0 * n + job]);
      const uint32_t ptm1 = static_cast<uint32_t>(I.lb1.p_times[ma1 * n + job]);
      const uint32_t lag =
          static_cast<uint32_t>(I.lb2.lags[static_cast<size_t>(k) * n + job]);
      pk.jp[static_cast<size_t>(k) * n + j] =
          (static_cast<uint32_t>(job) << 27) | (lag << 16) | (ptm1 << 8) | ptm0;
    }
  }
  // wave-kernel order: widest machine span first (strongest pairs in the
  // first 64-pair round -> the collective early exit fires sooner); counts
  // are order-invariant — the bound VALUE is the max over all pairs and the
  // exit decision (partial max > best) implies the full max's decision
  std::vector<int> perm(pairs);
  for (int i = 0; i < pairs; i++) perm[i] = i;
  const char* orde = std::getenv("GATS_LB2_ORDER");
  const std::string ord = orde ? orde : "span";
  if (ord == "lagsum") {
    // tie-break proxy: pairs whose relaxation carries the most lag mass
    std::vector<long long> ls(pairs, 0);
    for (int k = 0; k < pairs; k++)
      for (int j = 0; j < n; j++)
        ls[k] += I.lb2.lags[static_cast<size_t>(k) * n + j];
    std::sort(perm.begin(), perm.end(), [&](int a, int b) {
      if (ls[a] != ls[b]) return ls[a] > ls[b];
      return a < b;
    });
  } else if (ord != "lex") {  // default: widest machine span first
    std::sort(perm.begin(), perm.end(), [&](int a, int b) {
      const int sa = I.lb2.pairs2[a] - I.lb2.pairs1[a];
      const int sb = I.lb2.pairs2[b] - I.lb2.pairs1[b];
      if (sa != sb) return sa > sb;
      return a < b;
    });
  }
  pk.p1_w.resize(pairs);
  pk.p2_w.resize(pairs);
  pk.jp_w.resize(pk.jp.size());
  for (int l = 0; l < pairs; l++) {
    const int k = perm[l];
    pk.p1_w[l] = pk.p1[k];
    pk.p2_w[l] = pk.p2[k];
    std::copy(pk.jp.begin() + static_cast<size_t>(k) * n,
              pk.jp.begin() + static_cast<size_t>(k + 1) * n,
              pk.jp_w.begin() + static_cast<size_t>(l) * n);
  }
  return pk;
}

// Shared devpool driver: capture BATCH iterations into a hipGraph once, then
// replay + poll the 48 B control block until the pool drops below m
// (graph replay ~10-16 us vs ~3.5 us host cost PER LAUNCH eager — the hot
// loop is launch-bound at chunk sizes this small).
// `shared_best` (optional): a cross-thread incumbent. Each readback publishes
// the engine's best into it (atomic min) and adopts a lower value published by
// other ranks/threads by writing ctl->best on the (synchronized) stream —
// the RCCL incumbent-UB exchange of the distributed tier plugs in here.
// enqueue_iter(parity, chunk_bound): parity alternates 0/1 per iteration —
// iteration i reads ctl[parity] and gather2 writes ctl[1-parity]; the loop
// tracks the live parity so hooks and readbacks always touch the block the
// last gather wrote. chunk_bound is an upper bound on the pool size at that
// iteration (exact at readbacks, x branching per blind iteration) so the
// callee can size its launch grids to work that can actually exist; pop
// semantics are unchanged because bound >= size implies
// min(size, min(Mc, bound)) == min(size, Mc).
// `readback_hook(host_ctl, live_ctl_d)`: called after every batch readback
// with the stream idle; may reduce host_ctl->size after carving the pool (the
// donor path of SliceShare) — it must then also write the device ctl itself.
// `spill_hook(host_ctl, live_ctl_d)`: called (stream idle) when the next
// iteration's worst-case growth no longer fits `capacity`; carves part of the
// pool to host storage and rewrites both sizes. The caller re-runs spilled
// nodes after the loop, so counts stay exact (Pool.chpl:28-31's unbounded-
// growth contract, met by spilling instead of growing).
using ReadbackHook = std::function<void(DevCtl*, DevCtl*)>;

struct DevLoopCfg {
  unsigned long long m = 1;          // loop exits when size < m
  unsigned long long init_size = 0;  // pool size at entry
  unsigned long long growth = 0;     // worst-case net pool growth per iteration
  unsigned long long capacity = 0;   // pool capacity in nodes
  unsigned long long stop_size = 0;  // frontier builder: stop once size >= this
  int kernels_per_iter = 2;
  int per = 1;                       // max children per node (grid-bound growth)
  bool allow_graph = true;
  int max_batches = 0;            // tests: end the loop after this many batches (0 = never)
  DevLoopTrace* trace = nullptr;  // tests: one record per loop turn (engine_gpu.hpp)
};

static DevpoolStepCtl step_ctl_of(const DevCtl& c) {
  return {c.size, c.chunk, c.tree, c.sol, c.iters, c.best, c.overflow};
}

constexpr unsigned long long LOOP_TRACE_MAX_NODES = 1ull << 22;

// Copy `n` nodes into a trace record: from device memory over the (idle)
// stream `s`, or from host memory when `on_device` is false.
static void trace_nodes(DevLoopTrace& t, DevLoopRec& rec, const void* src,
                        unsigned long long n, bool on_device, hipStream_t s) {
  t.traced_nodes += n;
  if (t.traced_nodes > LOOP_TRACE_MAX_NODES)
    throw std::runtime_error("devpool loop trace exceeds 2^22 nodes");
  rec.nodes.resize(n * t.node_bytes);
  if (n == 0) return;
  if (!on_device) {
    std::memcpy(rec.nodes.data(), src, rec.nodes.size());
    return;
  }
  HIP_CHECK(hipMemcpyAsync(rec.nodes.data(), src, rec.nodes.size(), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

template <class EnqueueIter>
static DevCtl run_devpool_loop(hipStream_t s, DevCtl* ctl_d, const DevLoopCfg& cfg,
                               EnqueueIter&& enqueue_iter, Result& r,
                               std::atomic<int>* shared_best = nullptr,
                               const ReadbackHook& readback_hook = {},
                               const ReadbackHook& spill_hook = {}) {
  PinnedGuard<DevCtl> ctl_h(1);
  const int BATCH = 16;
  // GATS_NO_GRAPH=1 falls back to eager launches (rocprofv3 crashes tracing
  // hipGraph replays on ROCm 7.2; eager mode gives identical results).
  // Graph capture is LAZY: instantiation costs a few ms, which dominates
  // small searches (PFSP ta0xx finish in <10 ms), so the first EAGER_BATCHES
  // batches run eager and the graph is built only if the search is still
  // going.
  // multi-slice engines pass allow_graph=false: ROCm 7.2 stream capture races
  // with concurrent async work from the other slice threads no matter the
  // capture mode; with >1 slice in flight the host launch latency is hidden
  // by the other slices anyway
  const bool graph_allowed = cfg.allow_graph && cfg.stop_size == 0 &&
                             std::getenv("GATS_NO_GRAPH") == nullptr;
  const int EAGER_BATCHES = 4;
  int batches = 0;
  int par = 0;  // parity of the NEXT iteration == index of the live ctl block
  unsigned long long last_size = cfg.init_size;
  // chunk BOUND handed to each launch so its grid covers only the pool that
  // can possibly exist: exact at readbacks, multiplied by the branching
  // factor per blind iteration. Full-size grids for tiny chunks were the
  // small-search floor (an 80-node ta019 tree dispatched 15k-block lb2
  // grids: 1.53 ms; the engine infra itself costs 0.025 ms).
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  bool overflow = false;
  *ctl_h.p = DevCtl{};
  ctl_h.p->size = cfg.init_size;
  while (true) {
    // capacity-aware batch: never launch more iterations than worst-case
    // growth allows; spill when even one iteration might not fit. Small
    // pools use short batches so the chunk bound (and with it the launch
    // grids) is re-tightened every couple of iterations.
    int b = (cfg.stop_size > 0) ? 1 : BATCH;
    if (cfg.per > 1 && last_size < 4096 && b > 2) b = 2;
    if (cfg.growth > 0 && cfg.capacity > 0) {
      const unsigned long long room =
          cfg.capacity > last_size ? cfg.capacity - last_size : 0;
      const unsigned long long bmax = room / cfg.growth;
      if (bmax == 0 && spill_hook && last_size >= 4 * cfg.m && batches > 0) {
        if (cfg.trace) {
          cfg.trace->recs.emplace_back();
          cfg.trace->recs.back().kind = DevLoopRec::SPILL;
          cfg.trace->recs.back().size_before = last_size;
        }
        spill_hook(ctl_h.p, ctl_d + par);  // fills the record's nodes
        last_size = ctl_h.p->size;
        if (cfg.trace) cfg.trace->recs.back().size_after = last_size;
        continue;
      }
      if (bmax == 0) {
        // worst-case doesn't fit but the actual child count usually does;
        // run one iteration — the gather kernel's exact-fit guard flags a
        // REAL overflow, which is fatal (the iteration state is torn)
        b = 1;
      } else if (bmax < static_cast<unsigned long long>(b)) {
        b = static_cast<int>(bmax);
      }
    }
    bool captured = false;
    const int par_in = par;
    if (graph_allowed && batches >= EAGER_BATCHES && exec == nullptr && b == BATCH &&
        par == 0) {
      // one capture at a time: concurrent captures from the slice threads
      // race inside ROCm 7.2 ("previous error during capture"); relaxed mode
      // lets the other slices keep launching meanwhile. A failed capture is
      // not fatal — the loop just stays eager.
      static std::mutex capture_mu;
      std::lock_guard<std::mutex> lock(capture_mu);
      hipError_t ce = hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed);
      if (ce == hipSuccess) {
        for (int i = 0; i < BATCH; i++) enqueue_iter(i & 1, ~0ull);
        ce = hipStreamEndCapture(s, &graph);
        if (ce == hipSuccess) {
          if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
            (void)hipGraphDestroy(graph);
            graph = nullptr;
            exec = nullptr;
          }
        } else {
          graph = nullptr;
        }
        // a successfully captured batch was not EXECUTED; replay it below or
        // re-run eagerly — either way the work happens exactly once
        if (exec == nullptr) (void)hipGetLastError();
        captured = exec != nullptr;
      } else {
        (void)hipGetLastError();
      }
    }
    const bool replay = exec != nullptr && b == BATCH && par == 0;
    if (replay) {
      HIP_CHECK(hipGraphLaunch(exec, s));  // even count: parity unchanged
    } else {
      unsigned long long bound = last_size ? last_size : 1;
      for (int i = 0; i < b; i++) {
        enqueue_iter(par, bound);
        par ^= 1;
        if (bound < (1ull << 40)) bound *= cfg.per > 1 ? cfg.per : 2;
      }
    }
    batches++;
    HIP_CHECK(
        hipMemcpyAsync(ctl_h.p, ctl_d + par, sizeof(DevCtl), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    r.kernel_launch += static_cast<uint64_t>(cfg.kernels_per_iter) * b;
    r.d2h++;
    r.d2h_bytes += sizeof(DevCtl);
    static const bool chk = std::getenv("GATS_DEVPOOL_CHECK") != nullptr;
    if (chk && cfg.growth > 0 &&
        ctl_h.p->size > last_size + static_cast<unsigned long long>(b) * cfg.growth)
      fprintf(stderr, "DEVPOOL VIOLATION: size %llu -> %llu after %d iters (growth %llu)\n",
              last_size, ctl_h.p->size, b, cfg.growth);
    if (cfg.trace) {
      DevLoopTrace& t = *cfg.trace;
      t.recs.emplace_back();
      DevLoopRec& rec = t.recs.back();
      rec.kind = DevLoopRec::BATCH;
      rec.b = b;
      rec.parity = par_in;
      rec.graph = replay;
      rec.captured = captured;
      rec.size_before = last_size;
      rec.ctl = step_ctl_of(*ctl_h.p);
      if (!ctl_h.p->overflow) {
        if (ctl_h.p->size > cfg.capacity)
          throw std::runtime_error("devpool loop: size exceeds capacity");
        trace_nodes(t, rec, t.pool_d, ctl_h.p->size, /*on_device=*/true, s);
      }
    }
    last_size = ctl_h.p->size;
    if (ctl_h.p->overflow) {
      overflow = true;
      break;
    }
    if (readback_hook) {
      readback_hook(ctl_h.p, ctl_d + par);
      last_size = ctl_h.p->size;
    }
    if (shared_best) {
      int mine = ctl_h.p->best;
      int cur = shared_best->load(std::memory_order_relaxed);
      while (mine < cur && !shared_best->compare_exchange_weak(cur, mine,
                                                               std::memory_order_relaxed)) {
      }
      cur = shared_best->load(std::memory_order_relaxed);
      if (cur < mine) {
        // adopt the lower incumbent; the stream is idle (synchronized above),
        // so no device atomicMin can race this write
        HIP_CHECK(hipMemcpyAsync(&(ctl_d + par)->best, &cur, sizeof(int),
                                 hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
      }
    }
    if (cfg.stop_size > 0 && ctl_h.p->size >= cfg.stop_size) break;
    if (ctl_h.p->size < cfg.m) break;
    if (cfg.max_batches > 0 && batches >= cfg.max_batches) break;
  }
  if (exec != nullptr) {
    (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(graph);
  }
  if (overflow)
    throw std::runtime_error(
        "device pool overflow: capacity too small for one offload iteration even after "
        "spilling; raise --capacity (or lower --M)");
  return *ctl_h.p;
}

// ---------------------------------------------------------------------------
// Multi-slice devpool: S independent device pools driven on S HIP streams by
// S host threads — ONE devpool loop is a serial expand->gather dependency
// chain, so concurrent chains hide its kernel-boundary bubbles (and, before
// the wide-chunk change, filled the otherwise half-idle chip). The frontier
// is round-robin split exactly like the multi-GPU partition
// (nqueens_multigpu_chpl.chpl:221-226), just inside one device; a drained
// thread takes donated half-pools (SliceShare below). Counts are
// slice-order independent. S default: see devpool_slices().
// ---------------------------------------------------------------------------

// Concurrent slice chains per device. Wide-chunk paths (N-Queens, lb1,
// lb1_d) fill the chip from one ~512k-node launch, so 2 chains suffice to
// hide kernel-boundary bubbles (measured N=17: S=1 89.3 ms, S=2 77.4,
// S=4 79.6, S=6 84.2). lb2 keeps the narrow --M chunk (per-wave grid), so
// its kernels are short and need 4 chains (ta005 20x5: S=2 41.4 s,
// S=4 31.5 s; ta021 20x20 is S-insensitive). lb12 (code 4) starts from the
// lb1_d choices here and in devpool_chunk_cap: its grid is per parent like
// lb1_d's, but neither choice has been measured for its kernel yet.
static int devpool_slices(int lbk = 1) {
  if (const char* e = std::getenv("GATS_SLICES")) {
    int v = atoi(e);
    return v < 1 ? 1 : v;
  }
  return (lbk == 2) ? 4 : 2;
}

// Internal per-iteration expansion width of the devpool. The reference's M
// caps how many nodes are COPIED to the GPU per offload round
// (pfsp_gpu_cuda.c:424-426); a device-resident pool has no copy window, so
// the devpool widens the chunk to ~512k nodes — one launch then fills the
// 256 CUs by itself and the iteration count drops ~10x. --M stays a lower
// bound here (and is honored exactly in hostpool mode). Clamped so one
// iteration's worst-case children still fit half the pool capacity (the
// spill path needs that), and so chunk*branching fits u32 child indexing.
static unsigned long long devpool_chunk_cap(int M, int per, unsigned long long capacity,
                                            int lbk) {
  // lb2's wave-cooperative kernel gives each CHILD a whole wave, so M=50000
  // already launches ~16k waves (chip is full); widening it just multiplies
  // the gather grid with empty slots and the worst-case growth bound
  // (measured: spill storms + 687 us gathers on ta006 at a 419k chunk)
  unsigned long long c = (lbk == 2) ? static_cast<unsigned long long>(M) : (1ull << 19);
  if (const char* e = std::getenv("GATS_DEVPOOL_CHUNK")) c = strtoull(e, nullptr, 10);
  const unsigned long long fit = capacity / (2 * static_cast<unsigned long long>(per));
  if (c > fit) c = fit;
  if (c < static_cast<unsigned long long>(M)) c = M;  // user window is the floor
  const unsigned long long lim = (1ull << 31) / per;
  if (c > lim) c = lim;
  return c;
}

struct SliceOut {
  DevCtl fin{};
  Result diag;
};

// Work-sharing between the slice threads of ONE engine: a thread whose queue
// drained waits here; a running thread donates the BACK half of its device
// pool at a readback boundary (stream synced, so the handoff region is
// quiescent until the thief's D2D copy acks). Steal-half + the >=2m donor
// threshold mirror the reference's stealing rule (Pool_par.chpl:153-165);
// all waits are bounded, and a waiter exits once no runner remains.
// SliceShare, the floor and both sides of the handshake live in
// slice_share.hpp (no HIP there); devpool_thread supplies the device actions.

// What a slice thread's readback and spill hooks see: the host copy of the
// live control block, its device address, the thread's pool and stream (idle
// at that point) and the thread's counters.
template <class NodeT>
struct SliceReadback {
  DevCtl* hc;
  DevCtl* live;
  const NodeT* pool_d;
  hipStream_t s;
  Result& r;
};
template <class NodeT>
using SliceReadbackFn = std::function<void(const SliceReadback<NodeT>&)>;

// MOVE the back half of the live pool to host memory: copy it to
// dest(half), shrink the size in both copies of the control block, wait, and
// count the transfer. `dest_mu`, when given, is held while dest() makes room
// and the copy is enqueued.
template <class NodeT, class Dest>
static void carve_back_half(const SliceReadback<NodeT>& rb, std::mutex* dest_mu, Dest&& dest) {
  const unsigned long long half = rb.hc->size / 2;
  const unsigned long long newsize = rb.hc->size - half;
  {
    std::unique_lock<std::mutex> l;
    if (dest_mu) l = std::unique_lock<std::mutex>(*dest_mu);
    HIP_CHECK(hipMemcpyAsync(dest(half), rb.pool_d + newsize, half * sizeof(NodeT),
                             hipMemcpyDeviceToHost, rb.s));
  }
  HIP_CHECK(hipMemcpyAsync(&rb.live->size, &newsize, sizeof(newsize), hipMemcpyHostToDevice,
                           rb.s));
  HIP_CHECK(hipStreamSynchronize(rb.s));
  rb.hc->size = newsize;
  rb.r.d2h++;
  rb.r.d2h_bytes += half * sizeof(NodeT);
}

// What the loop-driver test entry points add to a slice thread: the chunk cap
// taken as given, a batch limit per loop call and the trace sink (donations
// and takes are recorded in it too). With a SliceShare: `donate_floor`
// replaces donation_floor(m) (0 = the real floor), and at a readback whose
// pool is at or above the floor the thread first waits at most
// `await_idle_ms` until each of the `threads` threads of the share is either
// running or waiting for work (await_idle), so that a search of a few
// milliseconds donates for certain.
struct DevpoolThreadTest {
  unsigned long long chunk = 0;
  int max_batches = 0;
  DevLoopTrace* trace = nullptr;
  unsigned long long donate_floor = 0;
  int await_idle_ms = 0;
  int threads = 1;
};

// Queue-driven slice thread: allocates its device buffers once, then keeps
// claiming frontier slices from the shared index until none remain. Slices
// are oversubscribed (~4 per thread) so a thread whose slice finishes early
// just pulls the next one; once the queue is empty it takes donated
// half-pools of same-device threads (SliceShare). `shared_best` (optional) is
// the cross-thread incumbent handed to run_devpool_loop: without it nothing is
// published or written to the device. `on_readback` (optional) runs after
// the donation check at every readback boundary.
template <class Problem>
static SliceOut devpool_thread(const Problem& problem,
                               const std::vector<std::vector<typename Problem::Node>>& slices,
                               std::atomic<int>& next_slice, int best0, int m, int M,
                               int device, unsigned long long capacity,
                               std::atomic<int>* shared_best, bool allow_graph,
                               SliceShare* share,
                               std::vector<typename Problem::Node>& leftover,
                               const SliceReadbackFn<typename Problem::Node>& on_readback,
                               const DevpoolThreadTest* test = nullptr) {
  using NodeT = typename Problem::Node;
  set_device_cached(device);
  const Problem P = problem.on_device(device);
  StreamGuard stream;
  SliceOut out;
  out.fin.best = best0;
  Result& r = out.diag;
  const unsigned long long Mc =
      test ? test->chunk : devpool_chunk_cap(M, P.per, capacity, P.lbg);
  const bool presum = devpool_presum_alloc(devpool_grid(Mc, P.per, P.lbg), P.lbg);
  const DevpoolBufs<NodeT> bufs(capacity, Mc, P.per, P.lbg, Problem::needs_be, presum);
  DevLoopTrace* const trace = test ? test->trace : nullptr;
  if (trace) {
    trace->pool_d = bufs.pool.p;
    trace->node_bytes = sizeof(NodeT);
  }
  std::vector<NodeT> spilled;  // capacity-pressure spill, re-run after the slice

  auto iter = [&](int parity, unsigned long long bound) {
    const DevIterPolicy it = devpool_iter_policy(Mc, bound, P.per, P.lbg, presum);
    P.enqueue(bufs, bufs.ctl.p + parity, bufs.ctl.p + (1 - parity), m, it.Mi, it.ps, stream.s);
  };
  // Donor side of SliceShare: runs at readback boundaries (stream idle).
  auto donate = [&](DevCtl* hc, DevCtl* live) {
    static const bool off = std::getenv("GATS_NO_DONATE") != nullptr;  // bisect knob
    if (off || !share) return;
    const unsigned long long floor_sz =
        (test && test->donate_floor) ? test->donate_floor : donation_floor(m);
    if (test && test->await_idle_ms > 0 && !hc->overflow && hc->size >= floor_sz)
      await_idle(*share, test->threads, test->await_idle_ms);
    const unsigned long long before = hc->size;
    bool traced = false;
    // the stream is idle (caller synced), so rewriting the live size is safe
    auto set_size = [&](unsigned long long x) {
      HIP_CHECK(hipMemcpyAsync(&live->size, &x, sizeof(x), hipMemcpyHostToDevice, stream.s));
      HIP_CHECK(hipStreamSynchronize(stream.s));
      if (trace && x < before) {  // the carve: the offer is not published yet
        trace->recs.emplace_back();
        DevLoopRec& rec = trace->recs.back();
        rec.kind = DevLoopRec::DONATE;
        rec.size_before = before;
        rec.best = hc->best;
        traced = true;
        trace_nodes(*trace, rec, bufs.pool.p + x, before - x, /*on_device=*/true, stream.s);
      }
    };
    const Donation d = donate_if_wanted(share, hc->size, hc->best, hc->overflow != 0,
                                        bufs.pool.p, floor_sz, set_size);
    if (traced) {
      trace->recs.back().size_after = hc->size;
      trace->recs.back().outcome = static_cast<int>(d);
    }
  };
  ReadbackHook hook = [&](DevCtl* hc, DevCtl* live) {
    donate(hc, live);
    if (on_readback) on_readback({hc, live, bufs.pool.p, stream.s, r});
  };
  ReadbackHook spill = [&](DevCtl* hc, DevCtl* live) {
    if (hc->size / 2 == 0) return;
    const size_t before = spilled.size();
    carve_back_half<NodeT>({hc, live, bufs.pool.p, stream.s, r}, nullptr,
                           [&](unsigned long long half) {
                             spilled.resize(spilled.size() + half);
                             return spilled.data() + (spilled.size() - half);
                           });
    if (trace) {
      const unsigned long long half = spilled.size() - before;
      trace_nodes(*trace, trace->recs.back(), spilled.data() + before, half,
                  /*on_device=*/false, stream.s);
    }
  };

  DevLoopCfg cfg;
  cfg.m = m;
  cfg.capacity = capacity;
  cfg.growth = Mc * P.per;  // worst-case children/iter
  cfg.per = P.per;
  cfg.allow_graph = allow_graph;
  if (test) {
    cfg.max_batches = test->max_batches;
    cfg.trace = trace;
  }

  auto run_pool = [&](unsigned long long init_size, int init_best, bool from_spill = false) {
    size_t run_rec = 0;
    if (trace) {
      run_rec = trace->recs.size();
      trace->recs.emplace_back();
      trace->recs.back().kind = DevLoopRec::RUN;
      trace->recs.back().from_spill = from_spill;
      trace->recs.back().size_before = init_size;
    }
    DevCtl ctl{};
    ctl.size = init_size;
    // adopt the freshest incumbent before starting
    const int sb_now =
        shared_best ? shared_best->load(std::memory_order_relaxed) : init_best;
    ctl.best = sb_now < init_best ? sb_now : init_best;
    if (trace) trace->recs[run_rec].best = ctl.best;
    upload_ctl_pair(bufs.ctl.p, ctl, stream.s);
    r.h2d += 2;
    r.h2d_bytes += 2 * sizeof(DevCtl);
    cfg.init_size = init_size;
    const DevCtl fin = run_devpool_loop(stream.s, bufs.ctl.p, cfg, iter, r, shared_best,
                                        hook, spill);
    out.fin.tree += fin.tree;
    out.fin.sol += fin.sol;
    if (fin.best < out.fin.best) out.fin.best = fin.best;
    r.gpu_iters += fin.iters;
    if (trace) trace->recs[run_rec].size_after = fin.size;
    if (fin.size > 0) {
      const size_t base = leftover.size();
      leftover.resize(base + fin.size);
      HIP_CHECK(hipMemcpyAsync(leftover.data() + base, bufs.pool.p,
                               fin.size * sizeof(NodeT), hipMemcpyDeviceToHost, stream.s));
      HIP_CHECK(hipStreamSynchronize(stream.s));
      r.d2h++;
      r.d2h_bytes += fin.size * sizeof(NodeT);
    }
  };
  // re-run anything the capacity spill pushed out (it may spill again; the
  // stack shrinks by at least half the capacity per round)
  auto drain_spilled = [&]() {
    while (!spilled.empty()) {
      const size_t take = std::min<size_t>(spilled.size(), capacity / 2);
      std::vector<NodeT> chunk(spilled.end() - take, spilled.end());
      spilled.resize(spilled.size() - take);
      HIP_CHECK(hipMemcpyAsync(bufs.pool.p, chunk.data(), take * sizeof(NodeT),
                               hipMemcpyHostToDevice, stream.s));
      r.h2d++;
      r.h2d_bytes += take * sizeof(NodeT);
      run_pool(take, out.fin.best, /*from_spill=*/true);
    }
  };

  int si;
  while ((si = next_slice.fetch_add(1)) < static_cast<int>(slices.size())) {
    const std::vector<NodeT>& nodes = slices[si];
    if (nodes.empty()) continue;
    if (nodes.size() > capacity) throw std::runtime_error("devpool capacity too small");
    // per-stream async copies: synchronous hipMemcpy runs on the NULL stream
    // and would serialize every slice thread at each slice boundary
    HIP_CHECK(hipMemcpyAsync(bufs.pool.p, nodes.data(), nodes.size() * sizeof(NodeT),
                             hipMemcpyHostToDevice, stream.s));
    r.h2d++;
    r.h2d_bytes += nodes.size() * sizeof(NodeT);
    // a runner from here until the spilled stack is re-run too: with one
    // scope per run_pool call a waiter that looked between two of them saw no
    // runner and left for good while this thread still had nodes to share
    RunnerScope runner(share);
    run_pool(nodes.size(), best0);
    drain_spilled();
  }

  // queue drained: take donated halves of still-running slices until no
  // runner remains (ROADMAP item 2, landed)
  while (share) {
    StolenWork w;
    if (!wait_for_work(*share, w)) break;
    HIP_CHECK(hipMemcpyAsync(bufs.pool.p, w.src, w.n * sizeof(NodeT), hipMemcpyDeviceToDevice,
                             stream.s));
    HIP_CHECK(hipStreamSynchronize(stream.s));
    ack_taken(*share);
    if (trace) {  // what arrived, read from this thread's own pool
      trace->recs.emplace_back();
      DevLoopRec& rec = trace->recs.back();
      rec.kind = DevLoopRec::TAKE;
      rec.size_before = rec.size_after = w.n;
      rec.best = w.best;
      trace_nodes(*trace, rec, bufs.pool.p, w.n, /*on_device=*/true, stream.s);
    }
    RunnerScope runner(share);  // as above
    run_pool(w.n, w.best);
    drain_spilled();
  }
  return out;
}

static void merge_slice_diag(Result& r, const Result& d) {
  r.kernel_launch += d.kernel_launch;
  r.h2d += d.h2d;
  r.d2h += d.d2h;
  r.h2d_bytes += d.h2d_bytes;
  r.d2h_bytes += d.d2h_bytes;
  r.gpu_iters += d.gpu_iters;
}

// ---------------------------------------------------------------------------
// Multi-device devpool core (declared in engine_gpu.hpp): one shared slice
// queue across ALL workers' threads. A worker whose slices finish early just
// keeps claiming — the queue is the cross-device balancer (replacing the
// static per-worker partition the reference's own CUDA multi-GPU baseline
// uses, nqueens_multigpu_cuda.cu:268-277, which its README flags unstable).
// Donation (SliceShare) stays within a worker group: the half-pool handoff is
// a same-device D2D copy.
// ---------------------------------------------------------------------------

// S is the caller's devpool_slices() choice; `deep_levels` its threshold for
// the deep-frontier rule below. `sb` (optional) is the incumbent the slice
// threads share; `on_readback` goes to every slice thread.
template <class Problem>
static DevpoolMultiOut devpool_multi(const Problem& problem,
                                     Pool<typename Problem::Node>& pool, int S,
                                     int deep_levels, int best0, int m, int M,
                                     const std::vector<int>& devices,
                                     unsigned long long capacity, std::atomic<int>* sb,
                                     Result& r,
                                     const SliceReadbackFn<typename Problem::Node>& on_readback) {
  using NodeT = typename Problem::Node;
  const int D = static_cast<int>(devices.size());
  // a frontier of DEEP nodes explodes immediately (a 2048-node N=17 dist
  // sub-slice carries billion-node subtrees), so it deserves full slicing
  // no matter how small the pool is; only genuinely small searches (the
  // remaining levels bound the subtree) shrink S to skip slicing overhead
  int maxd = 0;
  for (size_t i = 0; i < pool.size(); i++)
    maxd = std::max(maxd, static_cast<int>(pool.data()[i].depth));
  if (problem.per - maxd < deep_levels)
    while (S > 1 && pool.size() < static_cast<size_t>(D) * S * 2048) S--;
  const int T = D * S;
  const int NS = (T == 1) ? 1 : T * 4;  // oversubscribe: ~4 queued slices/thread
  std::vector<std::vector<NodeT>> slices(NS);
  {
    const NodeT* src = pool.data();
    const size_t total = pool.size();
    for (int t = 0; t < NS; t++) slices[t].reserve(total / NS + 1);
    for (size_t i = 0; i < total; i++) slices[i % NS].push_back(src[i]);
    pool.clear();
  }
  std::atomic<int> next_slice{0};
  std::vector<SliceShare> shares(D);
  std::vector<SliceOut> outs(T);
  std::vector<std::vector<NodeT>> lefts(T);
  std::vector<std::exception_ptr> errs(T);
  const bool allow_graph = (T == 1);
  run_on_pool(T, [&](int t) {
    try {
      SliceShare* sh = (S > 1) ? &shares[t / S] : nullptr;
      outs[t] = devpool_thread(problem, slices, next_slice, best0, m, M, devices[t / S],
                               capacity, sb, allow_graph, sh, lefts[t], on_readback);
    } catch (...) {
      errs[t] = std::current_exception();
    }
  });
  for (auto& e : errs)
    if (e) std::rethrow_exception(e);
  DevpoolMultiOut o;
  o.best = best0;
  o.per_dev.assign(D, 0);
  for (int t = 0; t < T; t++) {
    o.tree += outs[t].fin.tree;
    o.sol += outs[t].fin.sol;
    if (outs[t].fin.best < o.best) o.best = outs[t].fin.best;
    o.per_dev[t / S] += outs[t].fin.tree;
    merge_slice_diag(r, outs[t].diag);
    if (!lefts[t].empty()) pool.pushBackBulk(lefts[t].data(), lefts[t].size());
  }
  if (sb) {
    const int sbv = sb->load(std::memory_order_relaxed);
    if (sbv < o.best) o.best = sbv;
  }
  return o;
}

// GATS_NQ_FINISH: depth of the in-thread bitmask subtree finisher (levels from
// the bottom), default and upper limit 8 (template recursion budget,
// NQ_FINISH_MAX).
static int nq_finish_depth() {
  int finish = 8;
  if (const char* e = std::getenv("GATS_NQ_FINISH")) finish = atoi(e);
  if (finish > 8) finish = 8;
  return finish;
}

// GATS_NQ_SPLIT: levels (0..2) k_nq_x splits every finisher job into sub-jobs
// before the lanes draw them from the block's queue; 0 is the whole-job,
// static-stride finisher. Read once.
int nq_split_default() {
  static const int split = [] {
    int v = NQ_SPLIT_DEFAULT;
    if (const char* e = std::getenv("GATS_NQ_SPLIT")) v = atoi(e);
    return v < 0 ? 0 : v > NQ_SPLIT_MAX ? NQ_SPLIT_MAX : v;
  }();
  return split;
}

DevpoolMultiOut nq_devpool_multi(Pool<NQNode>& pool, int N, int g, int m, int M,
                                 const std::vector<int>& devices,
                                 unsigned long long capacity, Result& r) {
  if (static_cast<unsigned long long>(M) * N > (1ull << 31))
    throw std::invalid_argument("devpool requires M * N <= 2^31");
  return devpool_multi(NqDevProblem(N, g, nq_finish_depth()), pool, devpool_slices(),
                       /*deep_levels=*/10, /*best0=*/0, m, M, devices, capacity, nullptr, r,
                       {});
}

static void check_devpool_branching(const PfspInstance& I, int lbk) {
  if (I.br != Branching::FWD && lbk != 0 && lbk != 4)
    throw std::invalid_argument(std::string("branching rule '") + branching_name(I.br) +
                                "' on the gpu tier needs lb1_d or lb12");
}

DevpoolMultiOut pfsp_devpool_multi(const PfspInstance& I, Pool<PFSPNode>& pool, int lbk,
                                   int best0, int m, int M,
                                   const std::vector<int>& devices,
                                   unsigned long long capacity,
                                   std::atomic<int>* shared_best, Result& r,
                                   ExtractShare* extract) {
  if (static_cast<unsigned long long>(M) * I.jobs > (1ull << 31))
    throw std::invalid_argument("devpool requires M * jobs <= 2^31");
  check_devpool_branching(I, lbk);
  const int lbg = devpool_lbk_geom(lbk, I.machines);  // 3 = per-lane lb2
  // workers share the incumbent through this atomic even when no external
  // one is plugged in (cross-worker pruning; identical counts at ub=1)
  std::atomic<int> local_best{best0};
  // engine-pausing inter-rank steal (ExtractShare): a pending request is
  // served at this (stream-idle) readback boundary by carving the back half to
  // the host; nodes MOVE, never copy, so counts stay exact. The CARVING
  // state keeps the request visibly pending until the nodes are READY to
  // take.
  SliceReadbackFn<PFSPNode> serve_extract;
  if (extract)
    serve_extract = [extract, m](const SliceReadback<PFSPNode>& rb) {
      extract->live_size.store(rb.hc->size, std::memory_order_relaxed);
      int want = ExtractShare::WANTED;
      if (extract->state.load(std::memory_order_relaxed) == want &&
          rb.hc->size >= 2 * static_cast<unsigned long long>(m) &&
          extract->state.compare_exchange_strong(want, ExtractShare::CARVING,
                                                 std::memory_order_acq_rel)) {
        const unsigned long long before = rb.hc->size;
        carve_back_half(rb, &extract->mu, [extract](unsigned long long half) {
          extract->taken.resize(half);
          return extract->taken.data();
        });
        if (std::getenv("GATS_CARVE_LOG"))
          fprintf(stderr, "CARVE pool=%p size %llu -> %llu tree=%llu iters=%llu\n",
                  (void*)rb.pool_d, before, rb.hc->size, rb.hc->tree, rb.hc->iters);
        extract->state.store(ExtractShare::READY, std::memory_order_release);
      }
    };
  // deep-frontier rule: 12+ open jobs
  return devpool_multi(PfspDevProblem(I, lbg), pool, devpool_slices(lbg),
                       /*deep_levels=*/12, best0, m, M, devices, capacity,
                       shared_best ? shared_best : &local_best, r, serve_extract);
}

// ---------------------------------------------------------------------------
// N-Queens
// ---------------------------------------------------------------------------

// Runs phases 2+3 given a phase-1 pool; shared by the CLI engine and the
// distributed tier (which builds the frontier itself and slices it).
Result nqueens_gpu_run(Pool<NQNode>& pool, int N, int g, int m, int M, int device,
                       const std::string& mode, uint64_t tree0, uint64_t sol0,
                       double phase1_time, unsigned long long capacity) {
  Result r;
  r.phases.push_back({tree0, sol0, phase1_time});
  uint64_t tree = tree0, sol = sol0;

  set_device_cached(device);
  const double t2 = now_sec();

  std::string mode_eff = mode;
  if (mode == "devpool" && N < 4) mode_eff = "hostpool";  // expand tiles assume N >= 4

  if (mode_eff == "hostpool") {
    StreamGuard stream;
    PinnedGuard<NQNode> parents(M);
    PinnedGuard<uint8_t> labels(static_cast<size_t>(M) * N);
    DevGuard<NQNode> parents_d(M);
    DevGuard<uint8_t> labels_d(static_cast<size_t>(M) * N);
    while (true) {
      const size_t n = pool.popBackBulk(m, M, parents.p);
      if (n == 0) break;
      HIP_CHECK(hipMemcpyAsync(parents_d.p, parents.p, n * sizeof(NQNode),
                               hipMemcpyHostToDevice, stream.s));
      launch_nq_eval(parents_d.p, static_cast<int>(n), N, g, labels_d.p, stream.s);
      HIP_CHECK(hipMemcpyAsync(labels.p, labels_d.p, n * N, hipMemcpyDeviceToHost, stream.s));
      HIP_CHECK(hipStreamSynchronize(stream.s));
      r.kernel_launch++;
      r.h2d++;
      r.d2h++;
      r.h2d_bytes += n * sizeof(NQNode);
      r.d2h_bytes += n * N;
      r.gpu_iters++;
      nq_generate_children(parents.p, n, N, labels.p, tree, sol, pool);
    }
  } else if (mode_eff == "devpool") {
    DevpoolMultiOut o = nq_devpool_multi(pool, N, g, m, M, {device}, capacity, r);
    tree += o.tree;
    sol += o.sol;
  } else {
    throw std::invalid_argument("mode must be hostpool or devpool");
  }

  const double t3 = now_sec();
  r.gpu_time = t3 - t2;
  r.phases.push_back({tree - tree0, sol - sol0, t3 - t2});

  // Phase 3: CPU DFS drain (nqueens_gpu_chpl.chpl:226-245).
  uint64_t tree_p2 = tree, sol_p2 = sol;
  NQNode parent;
  while (pool.popBack(parent)) nq_decompose(parent, N, g, tree, sol, pool);
  const double t4 = now_sec();
  r.phases.push_back({tree - tree_p2, sol - sol_p2, t4 - t3});

  r.tree = tree;
  r.sol = sol;
  r.time = phase1_time + (t4 - t2);
  return r;
}

Result nqueens_gpu(int N, int g, int m, int M, int device, const std::string& mode,
                   unsigned long long capacity) {
  Pool<NQNode> pool;
  pool.pushBack(nq_root());
  uint64_t tree = 0, sol = 0;
  const double t0 = now_sec();
  size_t target = static_cast<size_t>(m);
  if (mode == "devpool")  // enough frontier to split across S device slices
    target = std::max(target, static_cast<size_t>(2048) * devpool_slices());
  nq_bfs_until(N, g, target, pool, tree, sol);
  const double p1 = now_sec() - t0;
  return nqueens_gpu_run(pool, N, g, m, M, device, mode, tree, sol, p1, capacity);
}

Result nqueens_gpu_from_pool(const std::vector<NQNode>& nodes, int N, int g, int m, int M,
                             int device, const std::string& mode,
                             unsigned long long capacity) {
  Pool<NQNode> pool;
  pool.pushBackBulk(nodes.data(), nodes.size());
  return nqueens_gpu_run(pool, N, g, m, M, device, mode, 0, 0, 0.0, capacity);
}

// ---------------------------------------------------------------------------
// PFSP
// ---------------------------------------------------------------------------

Result pfsp_gpu_run(const PfspInstance& I, LbKind lb, Pool<PFSPNode>& pool, int m, int M,
                    int device, const std::string& mode, uint64_t tree0, uint64_t sol0,
                    int best0, double phase1_time, unsigned long long capacity,
                    std::atomic<int>* shared_best /*= nullptr*/,
                    ExtractShare* extract /*= nullptr*/) {
  Result r;
  r.phases.push_back({tree0, sol0, phase1_time});
  uint64_t tree = tree0, sol = sol0;
  int best = best0;
  const int jobs = I.jobs, machines = I.machines;
  const int lbk = lbk_of(lb);

  set_device_cached(device);
  const double t2 = now_sec();

  if (mode == "hostpool") {
    StreamGuard stream;
    const PfspDevTables& tb_dev = pfsp_tables_cached(I, device);
    PinnedGuard<PFSPNode> parents(M);
    PinnedGuard<int32_t> bounds(static_cast<size_t>(M) * jobs);
    DevGuard<PFSPNode> parents_d(M);
    DevGuard<int32_t> bounds_d(static_cast<size_t>(M) * jobs);
    // non-fwd branching rules: the kernel returns both directions' bounds
    // (lb_begin in bounds, lb_end in bounds2) and the host picks per parent
    // lb12: the kernel picks the direction and filters with this batch's
    // incumbent; the host applies dir / bounds with its live one
    const bool l12 = lb == LbKind::LB12;
    std::unique_ptr<PinnedGuard<uint8_t>> dirs;
    std::unique_ptr<DevGuard<uint8_t>> dirs_d;
    if (l12) {
      dirs.reset(new PinnedGuard<uint8_t>(M));
      dirs_d.reset(new DevGuard<uint8_t>(M));
    }
    const bool bi = !l12 && I.br != Branching::FWD;
    if (bi) check_branching_supported(lb, I.br, true);
    std::unique_ptr<PinnedGuard<int32_t>> bounds2;
    std::unique_ptr<DevGuard<int32_t>> bounds2_d;
    if (bi) {
      bounds2.reset(new PinnedGuard<int32_t>(static_cast<size_t>(M) * jobs));
      bounds2_d.reset(new DevGuard<int32_t>(static_cast<size_t>(M) * jobs));
    }
    while (true) {
      const size_t n = pool.popBackBulk(m, M, parents.p);
      if (n == 0) break;
      HIP_CHECK(hipMemcpyAsync(parents_d.p, parents.p, n * sizeof(PFSPNode),
                               hipMemcpyHostToDevice, stream.s));
      launch_pfsp_eval(parents_d.p, static_cast<int>(n), jobs, machines, lbk, tb_dev, best,
                       bounds_d.p, stream.s, static_cast<int>(I.br),
                       bi ? bounds2_d->p : nullptr, l12 ? dirs_d->p : nullptr);
      if (l12)
        HIP_CHECK(hipMemcpyAsync(dirs->p, dirs_d->p, n, hipMemcpyDeviceToHost, stream.s));
      HIP_CHECK(hipMemcpyAsync(bounds.p, bounds_d.p, n * jobs * sizeof(int32_t),
                               hipMemcpyDeviceToHost, stream.s));
      if (bi)
        HIP_CHECK(hipMemcpyAsync(bounds2->p, bounds2_d->p, n * jobs * sizeof(int32_t),
                                 hipMemcpyDeviceToHost, stream.s));
      HIP_CHECK(hipStreamSynchronize(stream.s));
      r.kernel_launch++;
      r.h2d++;
      r.d2h += (bi || l12) ? 2 : 1;
      r.h2d_bytes += n * sizeof(PFSPNode);
      r.d2h_bytes += (bi ? 2 : 1) * n * jobs * sizeof(int32_t) + (l12 ? n : 0);
      r.gpu_iters++;
      if (l12)
        pfsp_generate_children_lb12(I, parents.p, n, dirs->p, bounds.p, tree, sol, best, pool);
      else if (bi)
        pfsp_generate_children_bi(I, parents.p, n, bounds.p, bounds2->p, tree, sol, best,
                                  pool);
      else
        pfsp_generate_children(I, parents.p, n, bounds.p, tree, sol, best, pool);
    }
  } else if (mode == "devpool") {
    DevpoolMultiOut o = pfsp_devpool_multi(I, pool, lbk, best, m, M, {device}, capacity,
                                           shared_best, r, extract);
    tree += o.tree;
    sol += o.sol;
    if (o.best < best) best = o.best;
  } else {
    throw std::invalid_argument("mode must be hostpool or devpool");
  }

  const double t3 = now_sec();
  r.gpu_time = t3 - t2;
  r.phases.push_back({tree - tree0, sol - sol0, t3 - t2});

  uint64_t tree_p2 = tree, sol_p2 = sol;
  PFSPNode parent;
  while (pool.popBack(parent)) pfsp_decompose(I, lb, parent, tree, sol, best, pool);
  const double t4 = now_sec();
  r.phases.push_back({tree - tree_p2, sol - sol_p2, t4 - t3});

  r.tree = tree;
  r.sol = sol;
  r.optimum = best;
  r.time = phase1_time + (t4 - t2);
  return r;
}

// Host-side instance (Taillard matrix + lb1/lb2 tables incl. 190 Johnson
// sorts) cached per (inst, ub, branching rule).
const PfspInstance& pfsp_instance_cached(int inst, int ub, Branching br) {
  static std::mutex mu;
  static std::map<std::pair<std::pair<int, int>, int>, PfspInstance*> cache;
  std::lock_guard<std::mutex> l(mu);
  auto key = std::make_pair(std::make_pair(inst, ub), static_cast<int>(br));
  auto it = cache.find(key);
  if (it == cache.end())
    it = cache.emplace(key, new PfspInstance(make_pfsp_instance(inst, ub, br))).first;
  return *it->second;
}

// Parse + validate a branching rule for a GPU-tier entry point.
static Branching gpu_branching(LbKind lb, const std::string& br_str) {
  const Branching br = branching_from_string(br_str);
  check_branching_supported(lb, br, true);
  return br;
}

Result pfsp_gpu(int inst, const std::string& lb_str, int ub, int m, int M, int device,
                const std::string& mode, unsigned long long capacity,
                const std::string& br) {
  const LbKind lb = lb_from_string(lb_str);
  const PfspInstance& I = pfsp_instance_cached(inst, ub, gpu_branching(lb, br));
  Pool<PFSPNode> pool;
  pool.pushBack(pfsp_root());
  uint64_t tree = 0, sol = 0;
  int best = I.init_ub;
  const double t0 = now_sec();
  size_t target = static_cast<size_t>(m);
  if (mode == "devpool")
    target = std::max(target, static_cast<size_t>(2048) * devpool_slices());
  pfsp_bfs_until(I, lb, target, pool, tree, sol, best);
  const double p1 = now_sec() - t0;
  return pfsp_gpu_run(I, lb, pool, m, M, device, mode, tree, sol, best, p1, capacity,
                      nullptr);
}

Result pfsp_gpu_rooted(int inst, const std::string& lb_str, int ub, int M, int device,
                       unsigned long long capacity, const std::string& br) {
  const LbKind lb = lb_from_string(lb_str);
  const PfspInstance& I = pfsp_instance_cached(inst, ub, gpu_branching(lb, br));
  Result r;
  Pool<PFSPNode> pool;
  pool.pushBack(pfsp_root());
  const int lbk = lbk_of(lb);
  set_device_cached(device);
  const double t0 = now_sec();
  r.phases.push_back({0, 0, 0.0});  // no CPU phase 1
  DevpoolMultiOut o =
      pfsp_devpool_multi(I, pool, lbk, I.init_ub, /*m=*/1, M, {device}, capacity,
                         nullptr, r);
  uint64_t tree = o.tree, sol = o.sol;
  int best = o.best;
  const double t2 = now_sec();
  r.phases.push_back({tree, sol, t2 - t0});
  // leftovers can only exist if a slice aborted; drain defensively
  uint64_t tree2 = tree, sol2 = sol;
  PFSPNode parent;
  while (pool.popBack(parent)) pfsp_decompose(I, lb, parent, tree2, sol2, best, pool);
  const double t3 = now_sec();
  r.phases.push_back({tree2 - tree, sol2 - sol, t3 - t2});
  r.tree = tree2;
  r.sol = sol2;
  r.optimum = best;
  r.gpu_time = t2 - t0;
  r.time = t3 - t0;
  return r;
}

Result nqueens_gpu_rooted(int N, int g, int M, int device, unsigned long long capacity) {
  Result r;
  Pool<NQNode> pool;
  pool.pushBack(nq_root());
  set_device_cached(device);
  const double t0 = now_sec();
  r.phases.push_back({0, 0, 0.0});  // no CPU phase 1
  DevpoolMultiOut o = nq_devpool_multi(pool, N, g, /*m=*/1, M, {device}, capacity, r);
  const double t2 = now_sec();
  r.phases.push_back({o.tree, o.sol, t2 - t0});
  uint64_t tree2 = o.tree, sol2 = o.sol;
  NQNode parent;
  while (pool.popBack(parent)) nq_decompose(parent, N, g, tree2, sol2, pool);
  const double t3 = now_sec();
  r.phases.push_back({tree2 - o.tree, sol2 - o.sol, t3 - t2});
  r.tree = tree2;
  r.sol = sol2;
  r.gpu_time = t2 - t0;
  r.time = t3 - t0;
  return r;
}

Result pfsp_gpu_from_pool(const std::vector<PFSPNode>& nodes, int inst,
                          const std::string& lb_str, int ub, int best0, int m, int M,
                          int device, const std::string& mode, unsigned long long capacity,
                          const std::string& br) {
  const LbKind lb = lb_from_string(lb_str);
  const PfspInstance& I = pfsp_instance_cached(inst, ub, gpu_branching(lb, br));
  check_pfsp_pool(nodes.data(), nodes.size(), I.br);  // before any HIP call
  Pool<PFSPNode> pool;
  pool.pushBackBulk(nodes.data(), nodes.size());
  const int best = (best0 > 0) ? best0 : I.init_ub;
  return pfsp_gpu_run(I, lb, pool, m, M, device, mode, 0, 0, best, 0.0, capacity,
                      nullptr);
}

// ---------------------------------------------------------------------------
// Loop-driver test entry points (declared in engine_gpu.hpp): one slice
// through the real devpool_thread, traced. Nothing else goes through them.
// ---------------------------------------------------------------------------

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
static DevpoolLoopOut<typename Problem::Node> devpool_loop_traced(
    const Problem& problem, const std::vector<typename Problem::Node>& nodes, int best0,
    unsigned long long m, unsigned long long chunk, unsigned long long capacity, bool graph,
    int max_batches, std::atomic<int>* sb, long long lower_at, int lower_to, int device) {
  using NodeT = typename Problem::Node;
  DevpoolLoopOut<NodeT> out;
  DevpoolThreadTest test;
  test.chunk = chunk;
  test.max_batches = max_batches;
  test.trace = &out.trace;
  const std::vector<std::vector<NodeT>> slices{nodes};
  std::atomic<int> next_slice{0};
  long long batch = 0;
  const SliceReadbackFn<NodeT> lower = [&](const SliceReadback<NodeT>&) {
    if (sb && batch++ == lower_at) {
      int cur = sb->load(std::memory_order_relaxed);
      while (lower_to < cur &&
             !sb->compare_exchange_weak(cur, lower_to, std::memory_order_relaxed)) {
      }
    }
  };
  (void)hipGetLastError();  // drop a stale launch error of an earlier, unchecked call
  const SliceOut so =
      devpool_thread(problem, slices, next_slice, best0, static_cast<int>(m), /*M=*/0, device,
                     capacity, sb, graph, /*share=*/nullptr, out.leftover, lower, &test);
  out.tree = so.fin.tree;
  out.sol = so.fin.sol;
  out.iters = so.diag.gpu_iters;
  out.best = so.fin.best;
  if (sb) out.best = std::min(out.best, sb->load(std::memory_order_relaxed));
  out.diag = so.diag;
  out.trace.pool_d = nullptr;
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
  return devpool_loop_traced(NqDevProblem(N, g, finish), nodes, /*best0=*/0, m, chunk,
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
static std::vector<DevpoolLoopOut<typename Problem::Node>> devpool_share_traced(
    const Problem& problem, const std::vector<typename Problem::Node>& nodes, int best0,
    unsigned long long m, unsigned long long chunk, unsigned long long capacity,
    int max_batches, std::atomic<int>* sb, int threads, unsigned long long donate_floor,
    int await_idle_ms, int device) {
  using NodeT = typename Problem::Node;
  std::vector<DevpoolLoopOut<NodeT>> outs(threads);
  std::vector<DevpoolThreadTest> tests(threads);
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
    tests[t].trace = &outs[t].trace;
    tests[t].donate_floor = donate_floor;
    tests[t].await_idle_ms = await_idle_ms;
    tests[t].threads = threads;
    pool.emplace_back([&, t] {
      try {
        sos[t] = devpool_thread(problem, slices, next_slice, best0, static_cast<int>(m),
                                /*M=*/0, device, capacity, sb, /*allow_graph=*/false, &share,
                                outs[t].leftover, {}, &tests[t]);
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
    out.trace.pool_d = nullptr;
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
  return devpool_share_traced(NqDevProblem(N, g, finish), nodes, /*best0=*/0, m, chunk,
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
// Device-built frontiers (declared in engine_gpu.hpp)
// ---------------------------------------------------------------------------

// Expands `root` level by level until the pool holds `target` nodes; returns
// the pool and, in `fin`, the final control block.
template <class Problem>
static std::vector<typename Problem::Node> gpu_frontier(const Problem& problem,
                                                        const typename Problem::Node& root,
                                                        size_t target, int device, int best0,
                                                        DevCtl& fin) {
  using NodeT = typename Problem::Node;
  set_device_cached(device);
  const Problem P = problem.on_device(device);
  StreamGuard stream;
  Result r;
  const unsigned long long M = target;  // one level per iteration below target
  const unsigned long long capacity = target * (MAX_JOBS + 1) + 64;  // branching <= 20
  const bool presum = (P.lbg == 2);
  const DevpoolBufs<NodeT> bufs(capacity, M, P.per, P.lbg, Problem::needs_be, presum);

  DevCtl ctl{};
  ctl.size = 1;
  ctl.best = best0;
  HIP_CHECK(hipMemcpyAsync(bufs.pool.p, &root, sizeof(NodeT), hipMemcpyHostToDevice, stream.s));
  upload_ctl_pair(bufs.ctl.p, ctl, stream.s);

  auto iter = [&](int parity, unsigned long long bound) {
    const unsigned long long Mi =
        std::min<unsigned long long>(M, std::max<unsigned long long>(bound, 1));
    P.enqueue(bufs, bufs.ctl.p + parity, bufs.ctl.p + (1 - parity), 1, Mi, presum, stream.s);
  };
  DevLoopCfg cfg;
  cfg.m = 1;
  cfg.init_size = 1;
  cfg.stop_size = target;
  cfg.per = P.per;
  cfg.allow_graph = false;
  fin = run_devpool_loop(stream.s, bufs.ctl.p, cfg, iter, r);
  std::vector<NodeT> nodes(fin.size);
  if (fin.size > 0) {
    // staged through cached pinned memory: a pageable 7 MB D2H runs ~5x
    // slower and showed up as ~10 ms/step in the bench
    PinnedGuard<NodeT> stage(capacity);
    HIP_CHECK(hipMemcpyAsync(stage.p, bufs.pool.p, fin.size * sizeof(NodeT),
                             hipMemcpyDeviceToHost, stream.s));
    HIP_CHECK(hipStreamSynchronize(stream.s));
    std::memcpy(nodes.data(), stage.p, fin.size * sizeof(NodeT));
  }
  return nodes;
}

std::vector<NQNode> nq_gpu_frontier(int N, int g, size_t target, int device,
                                    uint64_t& tree, uint64_t& sol) {
  DevCtl fin;
  std::vector<NQNode> nodes = gpu_frontier(NqDevProblem(N, g, nq_finish_depth()), nq_root(),
                                           target, device, /*best0=*/0, fin);
  tree = fin.tree;
  sol = fin.sol;
  return nodes;
}

std::vector<PFSPNode> pfsp_gpu_frontier(const PfspInstance& I, int lbk, size_t target,
                                        int device, int best0, uint64_t& tree,
                                        uint64_t& sol, int& best_out) {
  check_devpool_branching(I, lbk);
  DevCtl fin;
  std::vector<PFSPNode> nodes =
      gpu_frontier(PfspDevProblem(I, devpool_lbk_geom(lbk, I.machines)), pfsp_root(), target,
                   device, best0, fin);
  tree = fin.tree;
  sol = fin.sol;
  best_out = fin.best;
  return nodes;
}

// ---------------------------------------------------------------------------
// Asynchronous PFSP engine: runs the devpool search on a background thread
// and exposes a shared incumbent, so the Python distributed tier can run a
// fixed-cadence RCCL all_reduce(min) loop exchanging upper bounds DURING the
// search (the reference only min-reduces at the end,
// pfsp_dist_multigpu_cuda.c:694 — exchanging earlier tightens pruning and is
// always sound since any incumbent >= the optimum is a valid UB).
// ---------------------------------------------------------------------------

PfspAsyncEngine::PfspAsyncEngine(int inst, const std::string& lb_str, int ub, int m,
                                 int M, int device, unsigned long long capacity,
                                 const std::string& br)
    : inst_(inst), ub_(ub), m_(m), M_(M), device_(device), lb_(lb_str),
      capacity_(capacity), shared_best_(0) {
  if (lb_str == "lb12")
    throw std::invalid_argument("bound 'lb12' is not yet supported by PfspAsyncEngine");
  if (branching_from_string(br) != Branching::FWD)
    throw std::invalid_argument("branching rule '" + br +
                                "' is not yet supported by PfspAsyncEngine (fwd only)");
  const PfspInstance& I = pfsp_instance_cached(inst, ub);
  shared_best_.store(I.init_ub);
  result_.optimum = I.init_ub;
  th_ = std::thread([this] { loop(); });
}

PfspAsyncEngine::PfspAsyncEngine(std::vector<PFSPNode> nodes, int inst,
                                 const std::string& lb_str, int ub, int best0, int m, int M,
                                 int device, unsigned long long capacity,
                                 const std::string& br)
    : PfspAsyncEngine(inst, lb_str, ub, m, M, device, capacity, br) {
  submit(std::move(nodes), best0);
}

void PfspAsyncEngine::loop() {
  try {
    const PfspInstance& I = pfsp_instance_cached(inst_, ub_);
    const LbKind lb = lb_from_string(lb_);
    while (true) {
      std::vector<PFSPNode> nodes;
      int b0 = 0;
      {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return finish_ || !q_.empty(); });
        if (q_.empty()) break;  // finish requested and drained
        nodes = std::move(q_.front().first);
        b0 = q_.front().second;
        q_.pop_front();
        running_ = true;
        queued_nodes_.fetch_sub(nodes.size(), std::memory_order_relaxed);
      }
      Pool<PFSPNode> pool;
      pool.pushBackBulk(nodes.data(), nodes.size());
      const int start = (b0 > 0) ? b0 : I.init_ub;
      update_best(start);  // non-increasing incumbent across submits
      Result r = pfsp_gpu_run(I, lb, pool, m_, M_, device_, "devpool", 0, 0,
                              shared_best_.load(std::memory_order_relaxed), 0.0,
                              capacity_, &shared_best_, &ex_);
      result_.tree += r.tree;
      result_.sol += r.sol;
      if (r.optimum > 0 &&
          (result_.optimum == 0 || r.optimum < result_.optimum))
        result_.optimum = r.optimum;
      merge_slice_diag(result_, r);
      {
        std::lock_guard<std::mutex> l(mu_);
        running_ = false;
        if (q_.empty()) {
          ex_.live_size.store(0, std::memory_order_relaxed);
          answer_want_empty();  // unanswered steal request meets an empty engine
        }
      }
    }
    answer_want_empty();  // finishing with a pending request: no rank may block
  } catch (...) {
    err_ = std::current_exception();
    {
      // drain so done() turns true and the error surfaces at join() instead
      // of wedging pollers that wait for done()
      std::lock_guard<std::mutex> l(mu_);
      for (auto& it : q_) queued_nodes_.fetch_sub(it.first.size(), std::memory_order_relaxed);
      q_.clear();
      running_ = false;
    }
    answer_want_empty();
  }
}

// WANTED -> READY with an empty grant (the "nothing to give" answer). A
// CARVING state is left alone: the carver will set READY itself.
void PfspAsyncEngine::answer_want_empty() {
  int want = ExtractShare::WANTED;
  ex_.state.compare_exchange_strong(want, ExtractShare::READY,
                                    std::memory_order_acq_rel);
}

void PfspAsyncEngine::submit(std::vector<PFSPNode> nodes, int best0) {
  std::lock_guard<std::mutex> l(mu_);
  queued_nodes_.fetch_add(nodes.size(), std::memory_order_relaxed);
  q_.emplace_back(std::move(nodes), best0);
  cv_.notify_one();
}

PfspAsyncEngine::~PfspAsyncEngine() {
  {
    std::lock_guard<std::mutex> l(mu_);
    finish_ = true;
    cv_.notify_all();
  }
  if (th_.joinable()) th_.join();
}

int PfspAsyncEngine::best() const { return shared_best_.load(std::memory_order_relaxed); }

void PfspAsyncEngine::update_best(int b) {
  int cur = shared_best_.load(std::memory_order_relaxed);
  while (b < cur &&
         !shared_best_.compare_exchange_weak(cur, b, std::memory_order_relaxed)) {
  }
}

bool PfspAsyncEngine::done() const {
  std::lock_guard<std::mutex> l(mu_);
  return !running_ && q_.empty();
}

unsigned long long PfspAsyncEngine::pool_size() const {
  std::lock_guard<std::mutex> l(mu_);
  const unsigned long long live =
      running_ ? ex_.live_size.load(std::memory_order_relaxed) : 0;
  return live + queued_nodes_.load(std::memory_order_relaxed);
}

void PfspAsyncEngine::request_extract() {
  {
    std::lock_guard<std::mutex> l(mu_);
    if (ex_.state.load(std::memory_order_acquire) != ExtractShare::IDLE)
      return;  // one outstanding request at a time
    // cheapest grant first: an un-started queued frontier moves host-to-host
    if (!q_.empty()) {
      std::vector<PFSPNode> nodes = std::move(q_.back().first);
      q_.pop_back();
      queued_nodes_.fetch_sub(nodes.size(), std::memory_order_relaxed);
      std::lock_guard<std::mutex> le(ex_.mu);
      ex_.taken = std::move(nodes);
      ex_.state.store(ExtractShare::READY, std::memory_order_release);
      return;
    }
    if (!running_) {  // nothing to give: answer immediately so no rank waits
      ex_.state.store(ExtractShare::READY, std::memory_order_release);
      return;
    }
    ex_.state.store(ExtractShare::WANTED, std::memory_order_release);
  }
  // re-check: the run may have completed between the checks
  if (done()) answer_want_empty();
}

bool PfspAsyncEngine::extract_ready() const {
  return ex_.state.load(std::memory_order_acquire) == ExtractShare::READY;
}

bool PfspAsyncEngine::extract_pending() const {
  const int s = ex_.state.load(std::memory_order_acquire);
  return s == ExtractShare::WANTED || s == ExtractShare::CARVING;
}

std::vector<PFSPNode> PfspAsyncEngine::take_extract() {
  std::vector<PFSPNode> out;
  if (ex_.state.load(std::memory_order_acquire) != ExtractShare::READY) return out;
  {
    std::lock_guard<std::mutex> l(ex_.mu);
    out.swap(ex_.taken);
  }
  ex_.state.store(ExtractShare::IDLE, std::memory_order_release);
  return out;
}

Result PfspAsyncEngine::join() {
  {
    std::lock_guard<std::mutex> l(mu_);
    finish_ = true;
    cv_.notify_all();
  }
  if (th_.joinable()) th_.join();
  if (err_) std::rethrow_exception(err_);
  return result_;
}

}  // namespace gats
