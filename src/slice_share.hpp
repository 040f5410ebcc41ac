#pragma once
// Half-pool donation between the slice threads of one device: the protocol
// alone, with no HIP in it. A thread whose queue drained waits in
// wait_for_work; a running thread, at a readback boundary (its stream idle),
// carves the BACK half of its live device pool in donate_if_wanted, publishes
// the range and its incumbent, and blocks (bounded waits) until the thief's
// copy acks. Steal-half and the >= 2m donor threshold mirror the reference's
// stealing rule (Pool_par.chpl:153-165). The two device actions are callables
// of the caller: `set_size(x)` ("write x to the live control block's size and
// wait") here, the thief's copy between wait_for_work and ack_taken.
// tests/test_slice_share.py and tests/helpers/slice_share_stress.cpp run all
// of it on plain threads.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>

namespace gats {

// A half-pool must be a worthwhile work grant (the thief pays ~1 ms of engine
// start-up): 2m alone (the reference's steal threshold) caused donation
// thrash on large searches.
inline unsigned long long donation_floor(unsigned long long m) {
  return std::max<unsigned long long>(2 * m, 1ull << 16);
}

struct SliceShare {
  std::mutex mu;
  std::condition_variable cv;
  // threads waiting for donated work. Written under `mu`; atomic because the
  // donor's fast path reads it without the lock.
  std::atomic<int> idle{0};
  int runners = 0;  // threads currently inside a devpool loop
  bool offer_ready = false;
  bool offer_claimed = false;  // a thief took the pointer and is copying
  bool offer_taken = false;    // the thief's copy completed
  const void* offer_src = nullptr;  // device ptr to the donated node range
  unsigned long long offer_n = 0;
  int offer_best = 0;
};

enum class Donation {
  NONE = 0,       // no offer was made (set_size never called)
  TAKEN = 1,      // a thief copied the half; size is the kept front
  WITHDRAWN = 2,  // every waiter left unclaimed; size restored
  ABANDONED = 3,  // claimed, never acked before the deadline; nodes given up
};

// Donor side. `size`, `best`, `overflow` are the host copy of the live control
// block, `pool` the device pool it describes, `floor_sz` the smallest pool
// that donates. Offers pool[size - size / 2, size) when someone is waiting
// and no other offer is open; on TAKEN / ABANDONED `size` is the kept front.
template <class NodeT, class SetSize>
Donation donate_if_wanted(
    SliceShare* share, unsigned long long& size, int best, bool overflow, const NodeT* pool,
    unsigned long long floor_sz, SetSize&& set_size,
    std::chrono::milliseconds thief_deadline = std::chrono::seconds(10)) {
  if (!share || overflow) return Donation::NONE;
  if (size < floor_sz) return Donation::NONE;
  // fast path: rechecked under the lock
  if (share->idle.load(std::memory_order_relaxed) == 0) return Donation::NONE;
  std::unique_lock<std::mutex> lock(share->mu);
  if (share->idle == 0 || share->offer_ready) return Donation::NONE;
  const unsigned long long half = size / 2;
  const unsigned long long newsize = size - half;
  set_size(newsize);
  share->offer_src = pool + newsize;
  share->offer_n = half;
  share->offer_best = best;
  share->offer_ready = true;
  share->offer_claimed = false;
  share->offer_taken = false;
  share->cv.notify_all();
  const auto deadline = std::chrono::steady_clock::now() + thief_deadline;
  while (!share->offer_taken) {
    if (!share->offer_claimed && share->idle == 0) {
      // every waiter left (e.g. threw): withdraw the offer, restore the pool
      share->offer_ready = false;
      set_size(size);
      return Donation::WITHDRAWN;
    }
    if (share->offer_claimed && std::chrono::steady_clock::now() > deadline) {
      // thief died mid-copy (an exception is already propagating): give the
      // nodes up rather than double-count them
      share->offer_ready = false;
      size = newsize;
      return Donation::ABANDONED;
    }
    share->cv.wait_for(lock, std::chrono::milliseconds(20));
  }
  share->offer_ready = false;
  size = newsize;  // keep the loop's own view consistent
  return Donation::TAKEN;
}

// Thief side: returns true with (src, n, best) filled when donated work was
// claimed (caller must copy it and ack via ack_taken), false when no runner
// remains. Caller holds no lock.
struct StolenWork {
  const void* src = nullptr;
  unsigned long long n = 0;
  int best = 0;
};

inline bool wait_for_work(SliceShare& share, StolenWork& w) {
  std::unique_lock<std::mutex> lock(share.mu);
  share.idle++;
  while (true) {
    if (share.offer_ready && !share.offer_claimed) {
      w.src = share.offer_src;
      w.n = share.offer_n;
      w.best = share.offer_best;
      share.offer_claimed = true;  // ack via ack_taken after the copy
      share.idle--;
      return true;
    }
    if (share.runners == 0) {
      share.idle--;
      return false;
    }
    share.cv.wait_for(lock, std::chrono::milliseconds(20));
  }
}

inline void ack_taken(SliceShare& share) {
  std::lock_guard<std::mutex> lock(share.mu);
  share.offer_taken = true;
  share.cv.notify_all();
}

struct RunnerScope {
  SliceShare* s;
  explicit RunnerScope(SliceShare* share) : s(share) {
    if (s) {
      std::lock_guard<std::mutex> l(s->mu);
      s->runners++;
    }
  }
  RunnerScope(const RunnerScope&) = delete;
  RunnerScope& operator=(const RunnerScope&) = delete;
  ~RunnerScope() {
    if (s) {
      std::lock_guard<std::mutex> l(s->mu);
      s->runners--;
      s->cv.notify_all();
    }
  }
};

// Tests only: a runner (counted in `runners`) waits at most `ms` until every
// one of the `threads` threads is either running or waiting for work, so that
// a thread still on its way to wait_for_work is seen by the donation check
// that follows. With one runner that is idle == threads - 1. Returns whether
// the condition held.
inline bool await_idle(SliceShare& share, int threads, int ms) {
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(ms);
  std::unique_lock<std::mutex> lock(share.mu);
  while (share.idle + share.runners < threads) {
    if (std::chrono::steady_clock::now() >= deadline) return false;
    share.cv.wait_for(lock, std::chrono::milliseconds(1));
  }
  return true;
}

}  // namespace gats
