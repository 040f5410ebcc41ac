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

#include "devpool_driver.hpp"
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

// ---------------------------------------------------------------------------
// Multi-slice devpool: S independent device pools driven on S HIP streams by
// S host threads — ONE devpool loop is a serial expand->gather dependency
// chain, so concurrent chains hide its kernel-boundary bubbles (and, before
// the wide-chunk change, filled the otherwise half-idle chip). The frontier
// is round-robin split exactly like the multi-GPU partition
// (nqueens_multigpu_chpl.chpl:221-226), just inside one device; a drained
// thread takes donated half-pools (SliceShare). Counts are slice-order
// independent. S default: see devpool_slices(). The loop
// driver and the slice thread themselves are in devpool_driver.hpp.
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

// GATS_NQ_REFILL: idle lanes (1..64) at which a wave of the split finisher
// fetches sub-jobs for all of its idle lanes (nq_refill_now); 1 refills as
// soon as any lane is idle. Read once.
int nq_refill_default() {
  static const int refill = [] {
    int v = NQ_REFILL_DEFAULT;
    if (const char* e = std::getenv("GATS_NQ_REFILL")) v = atoi(e);
    return v < 1 ? 1 : v > 64 ? 64 : v;
  }();
  return refill;
}

// GATS_NQ_STACK: 1 = k_nq_x finishes subtrees from per-wave LDS node stacks
// (nq_finish.hpp) wherever the split is the default too and g == 1, 0 = the
// split finisher. Read once.
int nq_stack_default() {
  static const int stack = [] {
    int v = NQ_STACK_DEFAULT;
    if (const char* e = std::getenv("GATS_NQ_STACK")) v = atoi(e);
    return v != 0 ? 1 : 0;
  }();
  return stack;
}

NqFinishOpts nq_finish_opts(int g, const NqFinishOpts& asked) {
  if (asked.split > NQ_SPLIT_MAX) throw std::invalid_argument("split must be in 0..2, or < 0");
  if (asked.refill == 0 || asked.refill > 64)
    throw std::invalid_argument("refill must be in 1..64, or < 0");
  // stack = 1 is the finisher of the default split only; stack_cap is its knob
  if (asked.stack > 1) throw std::invalid_argument("stack must be 0 or 1, or < 0");
  if (asked.stack == 1 && asked.split >= 0)
    throw std::invalid_argument("stack = 1 takes no explicit split");
  if (asked.stack_cap > NQ_STACK_CAP)
    throw std::invalid_argument("stack_cap must be in 0.." + std::to_string(NQ_STACK_CAP) +
                                ", or < 0");
  NqFinishOpts o = asked;
  if (o.split < 0) o.split = nq_split_default();
  if (o.refill < 0) o.refill = nq_refill_default();
  o.stack = asked.stack < 0 ? (asked.split < 0 && g == 1 && nq_stack_default() == 1)
                            : asked.stack != 0;
  if (o.stack_cap < 0) o.stack_cap = NQ_STACK_CAP;
  return o;
}

// The engines' finisher: GATS_NQ_FINISH levels, every other knob its default.
static NqFinishOpts nq_engine_finisher(int g) {
  return nq_finish_opts(g, {nq_finish_depth()});
}

DevpoolMultiOut nq_devpool_multi(Pool<NQNode>& pool, int N, int g, int m, int M,
                                 const std::vector<int>& devices,
                                 unsigned long long capacity, Result& r) {
  if (static_cast<unsigned long long>(M) * N > (1ull << 31))
    throw std::invalid_argument("devpool requires M * N <= 2^31");
  return devpool_multi(NqDevProblem(N, g, nq_engine_finisher(g)), pool, devpool_slices(),
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
  std::vector<NQNode> nodes = gpu_frontier(NqDevProblem(N, g, nq_engine_finisher(g)), nq_root(),
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

void PfspAsyncEngine::update_best(int b) { min_into(shared_best_, b); }

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
