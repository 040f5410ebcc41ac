// Internals shared by the engine translation units (engine_gpu.cpp,
// engine_multi.cpp, engine_testing.cpp): HIP error check, cached device /
// pinned memory and streams, the PFSP table caches, min_into, and the pieces every
// devpool caller is built from — the owning buffer set, the per-problem
// descriptors and the per-iteration launch policy. Not part of the public
// API: bindings.cpp sees engine_gpu.hpp only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine_gpu.hpp"
#include "gpu_api.hpp"

namespace gats {

#define HIP_CHECK(expr)                                                              \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess)                                                            \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) +  \
                               " at " #expr);                                        \
  } while (0)

// Lower the shared incumbent `a` to `v` unless it is already that low.
inline void min_into(std::atomic<int>& a, int v) {
  int cur = a.load(std::memory_order_relaxed);
  while (v < cur && !a.compare_exchange_weak(cur, v, std::memory_order_relaxed)) {
  }
}

// Process-level buffer cache (engine_gpu.cpp): buffers are recycled by exact
// (device, bytes) and freed only at process exit.
void* cached_dev_alloc(size_t bytes);
void cached_dev_free(void* p, size_t bytes);
void* cached_pinned_alloc(size_t bytes);
void cached_pinned_free(void* p, size_t bytes);

template <typename T>
struct DevGuard {
  T* p = nullptr;
  size_t bytes = 0;
  explicit DevGuard(size_t n) : bytes(n * sizeof(T)) {
    p = static_cast<T*>(cached_dev_alloc(bytes));
  }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
  ~DevGuard() { cached_dev_free(p, bytes); }
};

template <typename T>
struct PinnedGuard {
  T* p = nullptr;
  size_t bytes = 0;
  explicit PinnedGuard(size_t n) : bytes(n * sizeof(T)) {
    p = static_cast<T*>(cached_pinned_alloc(bytes));
  }
  PinnedGuard(const PinnedGuard&) = delete;
  PinnedGuard& operator=(const PinnedGuard&) = delete;
  ~PinnedGuard() { cached_pinned_free(p, bytes); }
};

// A non-blocking stream of the current device, recycled through a
// process-level cache (engine_gpu.cpp has the measurements).
struct StreamGuard {
  hipStream_t s{};
  int dev = 0;
  static bool caching();
  StreamGuard();
  StreamGuard(const StreamGuard&) = delete;
  StreamGuard& operator=(const StreamGuard&) = delete;
  ~StreamGuard();
};

// Owns the int16/uint8-compressed PFSP bound tables on the current device.
struct PfspTablesGuard {
  PfspDevTables tb{};
  std::vector<void*> allocs;
  std::vector<size_t> alloc_bytes;
  explicit PfspTablesGuard(const PfspInstance& I);
  PfspTablesGuard(const PfspTablesGuard&) = delete;
  PfspTablesGuard& operator=(const PfspTablesGuard&) = delete;
  ~PfspTablesGuard();
  template <typename T>
  T* keep(T* p, size_t bytes) {
    allocs.push_back(p);
    alloc_bytes.push_back(bytes);
    return p;
  }
};

// PFSP device bound tables, built + uploaded once per (device, instance).
const PfspDevTables& pfsp_tables_cached(const PfspInstance& I, int device);
// Host-side instance (Taillard matrix + lb1/lb2 tables incl. 190 Johnson
// sorts) cached per (inst, ub, branching rule).
const PfspInstance& pfsp_instance_cached(int inst, int ub, Branching br = Branching::FWD);

// Kernel-side bound code: 0 = lb1_d, 1 = lb1, 2 = lb2, 4 = lb12 (3 is the
// per-lane lb2 GEOMETRY, gpu_api.hpp).
inline int lbk_of(LbKind lb) {
  switch (lb) {
    case LbKind::LB1_D:
      return 0;
    case LbKind::LB1:
      return 1;
    case LbKind::LB12:
      return 4;
    default:
      return 2;
  }
}

// Device buffers of one devpool (one slice thread, frontier builder, step or
// chain call). The grids are sized for `window` parents of up to `per`
// children each under geometry `lbg`; G is that grid's block count and
// `capacity` what gather2 checks the pool against. `with_be` adds the
// N-Queens finisher counts. `group_sums` sizes gsum for the group presum,
// (G + 255) / 256 entries; without it gsum is a 1-entry dummy and presum
// must never be requested.
template <class NodeT>
struct DevpoolBufs {
  const unsigned long long capacity;
  const int G;
  const int stride;
  DevGuard<NodeT> pool;
  DevGuard<DevCtl> ctl;  // parity-alternating control blocks
  DevGuard<NodeT> childbuf;
  DevGuard<uint32_t> bc;
  DevGuard<unsigned long long> bs;
  const std::unique_ptr<DevGuard<unsigned long long>> be_;
  DevGuard<uint32_t> gsum;

  DevpoolBufs(unsigned long long capacity_, unsigned long long window, int per, int lbg,
              bool with_be, bool group_sums)
      : capacity(capacity_),
        G(devpool_grid(window, per, lbg)),
        stride(devpool_stride(lbg)),
        pool(std::max<unsigned long long>(capacity_, 1)),
        ctl(2),
        childbuf(static_cast<size_t>(G) * stride),
        bc(G),
        bs(G),
        be_(with_be ? new DevGuard<unsigned long long>(G) : nullptr),
        gsum(group_sums ? (G + 255) / 256 : 1) {}

  unsigned long long* be() const { return be_ ? be_->p : nullptr; }
};

// Write `ctl` into both parity blocks and wait for it (callers pass a stack
// temporary). Copies enqueued on `s` before this call complete with it.
inline void upload_ctl_pair(DevCtl* ctl_d, const DevCtl& ctl, hipStream_t s) {
  HIP_CHECK(hipMemcpyAsync(ctl_d, &ctl, sizeof(DevCtl), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(ctl_d + 1, &ctl, sizeof(DevCtl), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// Problem descriptors: what the devpool callers (slice thread, multi-device
// core, frontier builder, step and chain entry points) need to know about
// the problem they run. `per` is the branching bound (N / jobs), `lbg` the
// kernel geometry code (gpu_api.hpp), `needs_be` whether gather2 takes the
// finisher counts. on_device(d) returns the descriptor with its per-device
// resources resolved; call it on the thread that runs the pool, after
// set_device_cached(d).
// enqueue() is ONE devpool iteration: expand -> (group presum) -> gather2.
// Every engine loop and the step / chain entry points enqueue exactly this
// sequence; the iteration reads `cur` and gather2's last block writes `next`.
// Mi is the chunk window the grids are sized for (callers clamp it to a bound
// on the live pool size, which leaves the pop rule min(size, M) unchanged).
struct NqDevProblem {
  using Node = NQNode;
  static constexpr bool needs_be = true;
  int per;  // N
  int lbg = 1;
  int g;
  NqFinishOpts finisher;  // resolved for this g: nq_finish_opts(g, ...)

  NqDevProblem(int N, int g_, const NqFinishOpts& finisher_)
      : per(N), g(g_), finisher(finisher_) {}
  NqDevProblem on_device(int) const { return *this; }

  void enqueue(const DevpoolBufs<NQNode>& b, DevCtl* cur, DevCtl* next, unsigned long long m,
               unsigned long long Mi, bool presum, hipStream_t s) const {
    const int Gi = devpool_grid(Mi, per, lbg);
    launch_nq_x(cur, b.pool.p, b.childbuf.p, b.bc.p, b.bs.p, b.be(), per, g, finisher, m, Mi, s);
    if (presum) launch_presum(b.bc.p, b.gsum.p, Gi, s);
    launch_gather2_nq(cur, next, b.bc.p, b.bs.p, b.be(), presum ? b.gsum.p : nullptr,
                      b.childbuf.p, b.pool.p, b.stride, Gi, m, Mi, b.capacity, s);
  }
};

struct PfspDevProblem {
  using Node = PFSPNode;
  static constexpr bool needs_be = false;
  int per;  // jobs
  int lbg;  // devpool_lbk_geom(lbk, machines), or a forced lb2 geometry
  int machines;
  int br;  // branching rule code
  const PfspInstance* inst;
  const PfspDevTables* tb = nullptr;  // per device: set by on_device()

  PfspDevProblem(const PfspInstance& I, int lbg_)
      : per(I.jobs), lbg(lbg_), machines(I.machines), br(static_cast<int>(I.br)), inst(&I) {}
  PfspDevProblem on_device(int device) const {
    PfspDevProblem p = *this;
    p.tb = &pfsp_tables_cached(*inst, device);
    return p;
  }

  void enqueue(const DevpoolBufs<PFSPNode>& b, DevCtl* cur, DevCtl* next,
               unsigned long long m, unsigned long long Mi, bool presum, hipStream_t s) const {
    const int Gi = devpool_grid(Mi, per, lbg);
    launch_pfsp_x(cur, b.pool.p, b.childbuf.p, b.bc.p, b.bs.p, per, machines, lbg, *tb, m, Mi,
                  s, br);
    if (presum) launch_presum(b.bc.p, b.gsum.p, Gi, s);
    launch_gather2_pfsp(cur, next, b.bc.p, b.bs.p, presum ? b.gsum.p : nullptr, b.childbuf.p,
                        b.pool.p, b.stride, Gi, m, Mi, b.capacity, s);
  }
};

// Per-iteration launch policy of the devpool engine threads (and of the chain
// test entry points, so that they launch what the engines launch): the grid
// window Mi covers only the chunk that can exist (bound >= pool size, so
// min(size, Mi) == min(size, Mc): the pop rule is unchanged), and the group
// presum runs only where the buffers were sized for it (presum_alloc) and the
// prefix walk is long enough to pay for the extra launch.
struct DevIterPolicy {
  unsigned long long Mi;
  bool ps;
};

// group sums keep gather's prefix walk O(G/256): always needed for lb2's
// per-wave counts, and for the thread-per-child paths once the chunk is wide
// (at the wide chunk G is ~8700 blocks and the linear walk dominated gather,
// 193 us avg at N=17). lb12 (code 4) has lb1_d's count granularity and
// starts from lb1_d's rule; unmeasured for its kernel.
inline bool devpool_presum_alloc(int G, int lbg) { return lbg == 2 || G > 1024; }

inline DevIterPolicy devpool_iter_policy(unsigned long long Mc, unsigned long long bound,
                                         int per, int lbg, bool presum_alloc) {
  const unsigned long long Mi = std::min(Mc, std::max<unsigned long long>(bound, 1));
  const bool ps = presum_alloc && (lbg == 2 || devpool_grid(Mi, per, lbg) > 256);
  return {Mi, ps};
}

}  // namespace gats
