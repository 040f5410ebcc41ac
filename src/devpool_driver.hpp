// The devpool loop driver and the slice thread that runs it — what every GPU
// tier goes through. Shared by engine_gpu.cpp (the engines) and
// engine_testing.cpp (the loop-driver test entry points), header-only. The
// driver's decisions are in devpool_loop_plan.hpp, the donation protocol in
// slice_share.hpp (no HIP in either); the HIP actions are here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "devpool_loop_plan.hpp"
#include "engine_gpu.hpp"
#include "engine_internal.hpp"
#include "gpu_api.hpp"
#include "slice_share.hpp"

namespace gats {

// Tests only (null in every engine): told what the driver and the slice
// thread do, at the points the loop-driver entry points document
// (engine_gpu.hpp). `pool_d` is the thread's device pool and `s` its stream,
// idle at every call, so an observer may copy nodes over it.
struct DevLoopObserver {
  virtual ~DevLoopObserver() = default;
  // a run_pool call: the pool and incumbent it starts with; the leftovers it returned
  virtual void run_begin(bool /*from_spill*/, unsigned long long /*size*/, int /*best*/) {}
  virtual void run_end(unsigned long long /*leftover*/) {}
  // after a batch's readback, before the overflow check and the readback hook
  virtual void batch(int /*b*/, int /*parity*/, bool /*replayed*/, bool /*captured*/,
                     unsigned long long /*size_before*/, const DevCtl& /*ctl*/,
                     const void* /*pool_d*/, hipStream_t /*s*/) {}
  // `n` nodes were moved to host memory at `moved`
  virtual void spill(unsigned long long /*size_before*/, unsigned long long /*size_after*/,
                     const void* /*moved*/, unsigned long long /*n*/) {}
  // the carve (`offered_d` = pool + kept; the offer is not published yet), then its outcome
  virtual void donate_carve(unsigned long long /*size_before*/, unsigned long long /*kept*/,
                            int /*best*/, const void* /*offered_d*/, hipStream_t /*s*/) {}
  virtual void donate_end(Donation /*outcome*/, unsigned long long /*size_after*/) {}
  // after the thief's copy and ack_taken: pool_d[0:n] is what arrived
  virtual void take(unsigned long long /*n*/, int /*best*/, const void* /*pool_d*/,
                    hipStream_t /*s*/) {}
};

// Shared devpool driver: capture LOOP_BATCH iterations into a hipGraph once,
// then replay + poll the 48 B control block until the pool drops below m
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

struct DevLoopCfg : DevLoopShape {
  unsigned long long init_size = 0;  // pool size at entry
  int kernels_per_iter = 2;
  bool allow_graph = true;
  int max_batches = 0;  // tests: end the loop after this many batches (0 = never)
  DevLoopObserver* obs = nullptr;  // tests
  const void* pool_d = nullptr;    // the pool ctl_d describes: handed to obs, not used
};

// Capture one full batch on `s` and instantiate it. One capture at a time:
// concurrent captures from the slice threads race inside ROCm 7.2 ("previous
// error during capture"); relaxed mode lets the other slices keep launching
// meanwhile. A failed capture is not fatal — exec stays null, the error is
// cleared and the loop just stays eager. A successfully captured batch was
// not EXECUTED; the caller replays it or re-runs it eagerly — either way the
// work happens exactly once.
template <class EnqueueIter>
void try_capture_batch(hipStream_t s, EnqueueIter&& enqueue_iter, hipGraph_t& graph,
                       hipGraphExec_t& exec) {
  static std::mutex capture_mu;
  std::lock_guard<std::mutex> lock(capture_mu);
  if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) == hipSuccess) {
    for (int i = 0; i < LOOP_BATCH; i++) enqueue_iter(i & 1, ~0ull);
    if (hipStreamEndCapture(s, &graph) != hipSuccess) {
      graph = nullptr;
    } else if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
      (void)hipGraphDestroy(graph);
      graph = nullptr;
      exec = nullptr;
    }
  }
  if (exec == nullptr) (void)hipGetLastError();
}

// Publish `mine` into the shared incumbent and adopt a lower one into the
// live control block; the stream is idle (the caller synchronized), so no
// device atomicMin can race this write.
inline void incumbent_exchange(std::atomic<int>& shared_best, int mine, DevCtl* live,
                               hipStream_t s) {
  min_into(shared_best, mine);
  const int cur = shared_best.load(std::memory_order_relaxed);
  if (cur < mine) {
    HIP_CHECK(hipMemcpyAsync(&live->best, &cur, sizeof(int), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
}

template <class EnqueueIter>
DevCtl run_devpool_loop(hipStream_t s, DevCtl* ctl_d, const DevLoopCfg& cfg,
                        EnqueueIter&& enqueue_iter, Result& r,
                        std::atomic<int>* shared_best = nullptr,
                        const ReadbackHook& readback_hook = {},
                        const ReadbackHook& spill_hook = {}) {
  PinnedGuard<DevCtl> ctl_h(1);
  const bool graph_allowed = graphs_allowed(cfg.allow_graph, cfg.stop_size);
  int batches = 0;
  int par = 0;  // parity of the NEXT iteration == index of the live ctl block
  unsigned long long last_size = cfg.init_size;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  bool overflow = false;
  *ctl_h.p = DevCtl{};
  ctl_h.p->size = cfg.init_size;
  while (true) {
    const int b = plan_batch(cfg, last_size, batches, static_cast<bool>(spill_hook));
    if (b == 0) {
      spill_hook(ctl_h.p, ctl_d + par);
      last_size = ctl_h.p->size;
      continue;
    }
    const int par_in = par;
    GraphStep g = plan_graph(graph_allowed, batches, exec != nullptr, b, par);
    bool captured = false;
    if (g == GraphStep::CAPTURE) {
      try_capture_batch(s, enqueue_iter, graph, exec);
      captured = exec != nullptr;
      g = captured ? GraphStep::REPLAY : GraphStep::EAGER;
    }
    if (g == GraphStep::REPLAY) {
      HIP_CHECK(hipGraphLaunch(exec, s));  // even count: parity unchanged
    } else {
      unsigned long long bound = first_chunk_bound(last_size);
      for (int i = 0; i < b; i++) {
        enqueue_iter(par, bound);
        par ^= 1;
        bound = next_chunk_bound(bound, cfg.per);
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
    if (cfg.obs)
      cfg.obs->batch(b, par_in, g == GraphStep::REPLAY, captured, last_size, *ctl_h.p,
                     cfg.pool_d, s);
    last_size = ctl_h.p->size;
    if (ctl_h.p->overflow) {
      overflow = true;
      break;
    }
    if (readback_hook) {
      readback_hook(ctl_h.p, ctl_d + par);
      last_size = ctl_h.p->size;
    }
    if (shared_best) incumbent_exchange(*shared_best, ctl_h.p->best, ctl_d + par, s);
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

// Internal per-iteration expansion width of the devpool. The reference's M
// caps how many nodes are COPIED to the GPU per offload round
// (pfsp_gpu_cuda.c:424-426); a device-resident pool has no copy window, so
// the devpool widens the chunk to ~512k nodes — one launch then fills the
// 256 CUs by itself and the iteration count drops ~10x. --M stays a lower
// bound here (and is honored exactly in hostpool mode). Clamped so one
// iteration's worst-case children still fit half the pool capacity (the
// spill path needs that), and so chunk*branching fits u32 child indexing.
inline unsigned long long devpool_chunk_cap(int M, int per, unsigned long long capacity,
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
void carve_back_half(const SliceReadback<NodeT>& rb, std::mutex* dest_mu, Dest&& dest) {
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

// What the loop-driver test entry points change in a slice thread: the chunk
// cap taken as given and a batch limit per loop call. With a SliceShare:
// `donate_floor` replaces donation_floor(m) (0 = the real floor), and at a
// readback whose pool is at or above the floor the thread first waits at most
// `await_idle_ms` until each of the `threads` threads of the share is either
// running or waiting for work (await_idle), so that a search of a few
// milliseconds donates for certain.
struct DevpoolThreadTest {
  unsigned long long chunk = 0;
  int max_batches = 0;
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
SliceOut devpool_thread(const Problem& problem,
                        const std::vector<std::vector<typename Problem::Node>>& slices,
                        std::atomic<int>& next_slice, int best0, int m, int M, int device,
                        unsigned long long capacity, std::atomic<int>* shared_best,
                        bool allow_graph, SliceShare* share,
                        std::vector<typename Problem::Node>& leftover,
                        const SliceReadbackFn<typename Problem::Node>& on_readback,
                        const DevpoolThreadTest* test = nullptr,
                        DevLoopObserver* obs = nullptr) {
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
    // the stream is idle (caller synced), so rewriting the live size is safe
    auto set_size = [&](unsigned long long x) {
      HIP_CHECK(hipMemcpyAsync(&live->size, &x, sizeof(x), hipMemcpyHostToDevice, stream.s));
      HIP_CHECK(hipStreamSynchronize(stream.s));
      if (obs && x < before) obs->donate_carve(before, x, hc->best, bufs.pool.p + x, stream.s);
    };
    const Donation d = donate_if_wanted(share, hc->size, hc->best, hc->overflow != 0,
                                        bufs.pool.p, floor_sz, set_size);
    if (obs) obs->donate_end(d, hc->size);
  };
  ReadbackHook hook = [&](DevCtl* hc, DevCtl* live) {
    donate(hc, live);
    if (on_readback) on_readback({hc, live, bufs.pool.p, stream.s, r});
  };
  ReadbackHook spill = [&](DevCtl* hc, DevCtl* live) {
    if (hc->size / 2 == 0) return;
    const size_t kept = spilled.size();
    const unsigned long long before = hc->size;
    carve_back_half<NodeT>({hc, live, bufs.pool.p, stream.s, r}, nullptr,
                           [&](unsigned long long half) {
                             spilled.resize(spilled.size() + half);
                             return spilled.data() + (spilled.size() - half);
                           });
    if (obs) obs->spill(before, hc->size, spilled.data() + kept, spilled.size() - kept);
  };

  DevLoopCfg cfg;
  cfg.m = m;
  cfg.capacity = capacity;
  cfg.growth = Mc * P.per;  // worst-case children/iter
  cfg.per = P.per;
  cfg.allow_graph = allow_graph;
  if (test) cfg.max_batches = test->max_batches;
  cfg.obs = obs;
  cfg.pool_d = bufs.pool.p;

  auto run_pool = [&](unsigned long long init_size, int init_best, bool from_spill = false) {
    DevCtl ctl{};
    ctl.size = init_size;
    // adopt the freshest incumbent before starting
    const int sb_now =
        shared_best ? shared_best->load(std::memory_order_relaxed) : init_best;
    ctl.best = sb_now < init_best ? sb_now : init_best;
    if (obs) obs->run_begin(from_spill, init_size, ctl.best);
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
    if (obs) obs->run_end(fin.size);
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
    if (obs) obs->take(w.n, w.best, bufs.pool.p, stream.s);
    RunnerScope runner(share);  // as above
    run_pool(w.n, w.best);
    drain_spilled();
  }
  return out;
}

}  // namespace gats
