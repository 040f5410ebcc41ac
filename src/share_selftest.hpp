#pragma once
// Scenarios over slice_share.hpp on plain std::threads and a fake pool (a
// vector of ints): no GPU, every wait bounded. share_selftest() in
// bindings.cpp runs them; tests/test_slice_share.py pins what they report.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <stdexcept>
#include <thread>
#include <vector>

#include "slice_share.hpp"

namespace gats {
namespace share_test {

struct Take {
  int thief = 0;
  long long offset = 0;  // src - pool base, in nodes
  unsigned long long n = 0;
  int best = 0;
  const void* src = nullptr;
};

inline long long node_offset(const void* src, const int* base) {
  return (reinterpret_cast<std::intptr_t>(src) - reinterpret_cast<std::intptr_t>(base)) /
         static_cast<long long>(sizeof(int));
}

struct Offer {
  int outcome = 0;                            // Donation
  std::vector<unsigned long long> set_calls;  // arguments of set_size, in order
  unsigned long long size_after = 0;
  int idle_after = 0;  // share.idle when donate_if_wanted returned
};

struct Out {
  std::vector<Offer> offers;  // one per donate_if_wanted call, in call order
  std::vector<Take> takes;    // in claim order
  int returned_false = 0;     // waiters that left wait_for_work empty-handed
  bool idle_reached = true;   // every await_idle of the scenario held
  double ms = 0;
};

inline bool spin_until(const std::atomic<bool>& flag, int ms) {
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(ms);
  while (!flag.load()) {
    if (std::chrono::steady_clock::now() >= deadline) return false;
    std::this_thread::sleep_for(std::chrono::microseconds(100));
  }
  return true;
}

struct Fixture {
  SliceShare share;
  std::vector<int> pool;
  std::mutex out_mu;
  Out out;

  Offer donate(unsigned long long& size, int best, bool overflow, unsigned long long floor_sz,
               std::chrono::milliseconds deadline = std::chrono::seconds(10)) {
    Offer o;
    auto set_size = [&](unsigned long long x) { o.set_calls.push_back(x); };
    o.outcome = static_cast<int>(donate_if_wanted(&share, size, best, overflow, pool.data(),
                                                  floor_sz, set_size, deadline));
    o.size_after = size;
    {
      std::lock_guard<std::mutex> l(share.mu);
      o.idle_after = share.idle;
    }
    return o;
  }

  // A thief: claims up to `max_takes` offers (< 0: any number), acks each at
  // once unless `hold` is given (then it acks only once *hold is set, or never
  // when it is not set within 5 s), and leaves when no runner remains.
  void thief(int id, int max_takes, const std::atomic<bool>* hold = nullptr,
             bool never_ack = false) {
    for (int k = 0; max_takes < 0 || k < max_takes; k++) {
      StolenWork w;
      if (!wait_for_work(share, w)) {
        std::lock_guard<std::mutex> l(out_mu);
        out.returned_false++;
        return;
      }
      {
        std::lock_guard<std::mutex> l(out_mu);
        out.takes.push_back({id, node_offset(w.src, pool.data()), w.n, w.best, w.src});
      }
      if (never_ack) return;  // "the thief died": a thread that returns
      if (hold && !spin_until(*hold, 5000)) return;
      ack_taken(share);
    }
  }
};

// One donor (a runner), `thieves` waiting threads, `offers` donation checks in
// a row on a pool of `size` nodes. `pending`: another offer is open (and
// claimed) during the checks. Each thief takes at most one offer when
// `one_each`, so a second offer must go to another thief.
inline Out basic(unsigned long long size, unsigned long long floor_sz, int thieves, int offers,
                 bool pending, bool overflow, int best, bool one_each) {
  Fixture f;
  f.pool.assign(size + 1, 0);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> ts;
  {
    RunnerScope runner(&f.share);
    for (int i = 0; i < thieves; i++)
      ts.emplace_back([&f, i, one_each] { f.thief(i, one_each ? 1 : -1); });
    f.out.idle_reached = await_idle(f.share, 1 + thieves, 5000);
    if (pending) {
      std::lock_guard<std::mutex> l(f.share.mu);
      f.share.offer_ready = f.share.offer_claimed = true;
    }
    for (int k = 0; k < offers; k++) {
      // a thief that acked is on its way back to wait_for_work (or gone)
      const int waiting = one_each ? std::max(thieves - k, 0) : thieves;
      f.out.idle_reached = f.out.idle_reached && await_idle(f.share, 1 + waiting, 5000);
      f.out.offers.push_back(f.donate(size, best, overflow, floor_sz));
    }
    if (pending) {
      std::lock_guard<std::mutex> l(f.share.mu);
      f.share.offer_ready = f.share.offer_claimed = false;
    }
  }
  for (auto& t : ts) t.join();
  f.out.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return f.out;
}

// Two donors, two thieves. Thief 0 claims donor A's offer and holds its ack;
// thief 1 keeps waiting (idle == 1). Donor B's check in that state is
// offers[0]; then thief 0 acks, A returns (offers[1]), and B's second check
// (offers[2]) serves thief 1.
inline Out two_donors(unsigned long long size_a, unsigned long long size_b,
                      unsigned long long floor_sz) {
  Fixture f, g;  // g: donor B's pool only
  f.pool.assign(size_a + 1, 0);
  g.pool.assign(size_b + 1, 0);
  std::atomic<bool> release{false};
  Offer a, b1, b2;
  std::vector<std::thread> ts;
  {
    RunnerScope runner_a(&f.share), runner_b(&f.share);
    ts.emplace_back([&] { f.thief(0, 1, &release); });
    f.out.idle_reached = await_idle(f.share, 3, 5000);
    std::thread donor_a([&] { a = f.donate(size_a, 7, false, floor_sz); });
    // A's offer is claimed once thief 0's take is recorded
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(5);
    while (std::chrono::steady_clock::now() < deadline) {
      {
        std::lock_guard<std::mutex> l(f.out_mu);
        if (!f.out.takes.empty()) break;
      }
      std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    ts.emplace_back([&] { f.thief(1, 1); });
    f.out.idle_reached = f.out.idle_reached && await_idle(f.share, 3, 5000);
    auto donate_b = [&](int best) {
      Offer o;
      auto set_size = [&](unsigned long long x) { o.set_calls.push_back(x); };
      o.outcome = static_cast<int>(
          donate_if_wanted(&f.share, size_b, best, false, g.pool.data(), floor_sz, set_size));
      o.size_after = size_b;
      std::lock_guard<std::mutex> l(f.share.mu);
      o.idle_after = f.share.idle;
      return o;
    };
    b1 = donate_b(9);
    release.store(true);
    donor_a.join();
    b2 = donate_b(9);
  }
  for (auto& t : ts) t.join();
  f.out.offers = {b1, a, b2};
  // thief 1's take points into B's pool
  for (Take& t : f.out.takes)
    if (t.thief == 1) t.offset = node_offset(t.src, g.pool.data());
  return f.out;
}

// The only waiter gives up before claiming: a stand-in for a waiter (it counts
// itself idle as wait_for_work does, and leaves once it sees the offer without
// claiming it). wait_for_work itself claims whatever open offer it wakes up
// to, so this path needs a waiter that does not.
inline Out withdraw(unsigned long long size, unsigned long long floor_sz) {
  Fixture f;
  f.pool.assign(size + 1, 0);
  std::thread waiter;
  {
    RunnerScope runner(&f.share);
    waiter = std::thread([&] {
      std::unique_lock<std::mutex> lock(f.share.mu);
      f.share.idle++;
      const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(5);
      while (!f.share.offer_ready && std::chrono::steady_clock::now() < deadline)
        f.share.cv.wait_for(lock, std::chrono::milliseconds(1));
      f.share.idle--;
      f.share.cv.notify_all();
    });
    f.out.idle_reached = await_idle(f.share, 2, 5000);
    f.out.offers.push_back(f.donate(size, 5, false, floor_sz));
  }
  waiter.join();
  return f.out;
}

// A thief that claims and never acks; the donor gives the nodes up after
// `deadline_ms`.
inline Out deadline(unsigned long long size, unsigned long long floor_sz, int deadline_ms) {
  Fixture f;
  f.pool.assign(size + 1, 0);
  const auto t0 = std::chrono::steady_clock::now();
  std::thread t;
  {
    RunnerScope runner(&f.share);
    t = std::thread([&] { f.thief(0, 1, nullptr, /*never_ack=*/true); });
    f.out.idle_reached = await_idle(f.share, 2, 5000);
    f.out.offers.push_back(
        f.donate(size, 5, false, floor_sz, std::chrono::milliseconds(deadline_ms)));
  }
  t.join();
  f.out.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return f.out;
}

// `runners` runner threads leave one after the other (by exception when
// `by_exception`); the waiter must still be waiting while one remains and
// return false after the last. idle_reached: it was still waiting each time.
inline Out termination(int runners, bool by_exception) {
  Fixture f;
  std::vector<std::atomic<bool>> go(runners);
  for (auto& g : go) g.store(false);
  std::atomic<int> entered{0};
  std::vector<std::thread> rs;
  for (int i = 0; i < runners; i++)
    rs.emplace_back([&, i] {
      try {
        RunnerScope runner(&f.share);
        entered++;
        spin_until(go[i], 5000);
        if (by_exception) throw std::runtime_error("runner failed");
      } catch (const std::runtime_error&) {
      }
    });
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(5);
  while (entered.load() < runners && std::chrono::steady_clock::now() < deadline)
    std::this_thread::sleep_for(std::chrono::microseconds(100));
  std::thread waiter([&] { f.thief(0, -1); });
  for (int i = 0; i < runners; i++) {
    // all of runners - i runners and the waiter accounted for: still waiting
    f.out.idle_reached = f.out.idle_reached && await_idle(f.share, runners - i + 1, 5000);
    {
      std::lock_guard<std::mutex> l(f.out_mu);
      f.out.idle_reached = f.out.idle_reached && f.out.returned_false == 0;
    }
    go[i].store(true);
    rs[i].join();
  }
  waiter.join();
  return f.out;
}

}  // namespace share_test
}  // namespace gats
