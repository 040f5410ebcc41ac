#include "search_host.hpp"

#include <chrono>
#include <climits>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <vector>

#include "taillard.hpp"

namespace gats {

double now_sec() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

LbKind lb_from_string(const std::string& s) {
  if (s == "lb1") return LbKind::LB1;
  if (s == "lb1_d") return LbKind::LB1_D;
  if (s == "lb2") return LbKind::LB2;
  if (s == "lb12") return LbKind::LB12;
  throw std::invalid_argument("unsupported lower bound '" + s + "' (lb1, lb1_d, lb2, lb12)");
}

Branching branching_from_string(const std::string& s) {
  if (s == "fwd") return Branching::FWD;
  if (s == "bwd") return Branching::BWD;
  if (s == "alt") return Branching::ALT;
  if (s == "minbranch") return Branching::MINBRANCH;
  throw std::invalid_argument("unsupported branching rule '" + s +
                              "' (fwd, bwd, alt, minbranch)");
}

const char* branching_name(Branching br) {
  switch (br) {
    case Branching::BWD:
      return "bwd";
    case Branching::ALT:
      return "alt";
    case Branching::MINBRANCH:
      return "minbranch";
    default:
      return "fwd";
  }
}

void check_branching_supported(LbKind lb, Branching br, bool gpu_tier) {
  if (br == Branching::FWD || lb == LbKind::LB12) return;  // lb12: every rule, seq and gpu
  const char* lbn = lb == LbKind::LB1 ? "lb1" : (lb == LbKind::LB1_D ? "lb1_d" : "lb2");
  if (br == Branching::MINBRANCH && lb != LbKind::LB1_D)
    throw std::invalid_argument(std::string("branching rule 'minbranch' with bound '") + lbn +
                                "' is not supported: minbranch needs both directions' "
                                "bounds of every child (lb1_d only)");
  if (gpu_tier && lb != LbKind::LB1_D)
    throw std::invalid_argument(std::string("branching rule '") + branching_name(br) +
                                "' with bound '" + lbn +
                                "' is not supported on the gpu tier: the bi-directional "
                                "kernels exist for lb1_d only");
}

void check_pfsp_pool(const PFSPNode* nodes, size_t n, Branching br) {
  if (br != Branching::FWD) return;
  for (size_t i = 0; i < n; i++)
    if (nodes[i].nback != 0)
      throw std::invalid_argument("node " + std::to_string(i) +
                                  ": nback != 0 needs a non-fwd branching rule (br)");
}

// ---------------- N-Queens ----------------

bool nq_is_safe(const uint8_t* board, int depth, int row_pos, int g) {
  uint8_t safe = 1;
  for (int i = 0; i < depth; i++) {
    const int other = board[i];
    for (int r = 0; r < g; r++) {
      int rp = row_pos;
      // barrier keeps the g repeats real work (the reference's artificial-work
      // knob); without it the loop is invariant and folds to one check
      if (g > 1) asm volatile("" : "+r"(rp));
      if (other == rp - (depth - i) || other == rp + (depth - i)) safe = 0;
    }
  }
  return safe != 0;
}

void nq_decompose(const NQNode& parent, int N, int g, uint64_t& tree, uint64_t& sol,
                  Pool<NQNode>& pool) {
  const int depth = parent.depth;
  if (depth == N) {
    sol += 1;
    return;
  }
  for (int j = depth; j < N; j++) {
    if (nq_is_safe(parent.board, depth, parent.board[j], g)) {
      NQNode child = parent;
      child.depth = static_cast<uint8_t>(depth + 1);
      child.board[depth] = parent.board[j];
      child.board[j] = parent.board[depth];
      pool.pushBack(child);
      tree += 1;
    }
  }
}

static void nq_check(int N, int g) {
  if (N < 1 || N > MAX_JOBS)
    throw std::invalid_argument("N must be in 1..20 (MAX_QUEENS parity, NQueens_node.chpl:7)");
  if (g < 1) throw std::invalid_argument("g must be >= 1");
}

Result nqueens_seq(int N, int g) {
  nq_check(N, g);
  Result r;
  Pool<NQNode> pool;
  pool.pushBack(nq_root());
  const double t0 = now_sec();
  NQNode parent;
  while (pool.popBack(parent)) nq_decompose(parent, N, g, r.tree, r.sol, pool);
  r.time = now_sec() - t0;
  r.phases.push_back({r.tree, r.sol, r.time});
  return r;
}

void nq_bfs_until(int N, int g, size_t target, Pool<NQNode>& pool, uint64_t& tree,
                  uint64_t& sol) {
  nq_check(N, g);
  NQNode parent;
  while (pool.size() < target) {
    if (!pool.popFront(parent)) break;
    nq_decompose(parent, N, g, tree, sol, pool);
  }
}

void nq_bfs_level(int N, int g, size_t target, Pool<NQNode>& pool, uint64_t& tree,
                  uint64_t& sol) {
  nq_check(N, g);
  // Serial BFS with BLOCK-granular pops: take up to BLOCK nodes off the
  // front, expand them in parallel (fixed chunk boundaries, children
  // concatenated in chunk order -> identical frontier for any thread count),
  // append the children at the back. Overshoot past `target` is bounded by
  // one block's children (vs whole-level sync, which overshot 5-7x on the
  // geometric N-Queens levels).
  constexpr size_t BLOCK = 8192;
  std::vector<NQNode> deque(pool.size());
  std::memcpy(deque.data(), pool.data(), pool.size() * sizeof(NQNode));
  pool.clear();
  size_t head = 0;
  while (deque.size() - head != 0 && deque.size() - head < target) {
    const size_t n = std::min(BLOCK, deque.size() - head);
    unsigned T = std::thread::hardware_concurrency();
    if (T == 0) T = 1;
    if (T > 16) T = 16;
    if (n < 2048) T = 1;  // thread spawn not worth it on small blocks
    std::vector<std::vector<NQNode>> childv(T);
    std::vector<uint64_t> tcnt(T, 0), scnt(T, 0);
    auto work = [&](unsigned t) {
      const size_t lo = head + n * t / T, hi = head + n * (t + 1) / T;
      Pool<NQNode> local;
      for (size_t i = lo; i < hi; i++) nq_decompose(deque[i], N, g, tcnt[t], scnt[t], local);
      childv[t].assign(local.data(), local.data() + local.size());
    };
    if (T == 1) {
      work(0);
    } else {
      std::vector<std::thread> th;
      for (unsigned t = 1; t < T; t++) th.emplace_back(work, t);
      work(0);
      for (auto& x : th) x.join();
    }
    head += n;
    if (head > (1u << 20) && head > deque.size() - head) {  // compact dead front
      deque.erase(deque.begin(), deque.begin() + head);
      head = 0;
    }
    for (unsigned t = 0; t < T; t++) {
      tree += tcnt[t];
      sol += scnt[t];
      deque.insert(deque.end(), childv[t].begin(), childv[t].end());
    }
  }
  if (deque.size() - head != 0)
    pool.pushBackBulk(deque.data() + head, deque.size() - head);
}

void nq_generate_children(const NQNode* parents, size_t n, int N, const uint8_t* labels,
                          uint64_t& tree, uint64_t& sol, Pool<NQNode>& pool) {
  for (size_t i = 0; i < n; i++) {
    const NQNode& parent = parents[i];
    const int depth = parent.depth;
    if (depth == N) {
      sol += 1;
      continue;
    }
    for (int j = depth; j < N; j++) {
      if (labels[i * N + j] == 1) {
        NQNode child = parent;
        child.depth = static_cast<uint8_t>(depth + 1);
        child.board[depth] = parent.board[j];
        child.board[j] = parent.board[depth];
        pool.pushBack(child);
        tree += 1;
      }
    }
  }
}

// ---------------- PFSP ----------------

PfspInstance make_pfsp_instance(int inst, int ub, Branching br) {
  if (ub != 0 && ub != 1) throw std::invalid_argument("ub must be 0 or 1");
  PfspInstance I;
  I.inst = inst;
  I.br = br;
  I.jobs = taillard_nb_jobs(inst);
  I.machines = taillard_nb_machines(inst);
  if (I.jobs > MAX_JOBS)
    throw std::invalid_argument("instance exceeds MAX_JOBS=20 (use ta001..ta030)");
  I.init_ub = (ub == 1) ? taillard_best_ub(inst) : INT_MAX;
  I.lb1 = make_lb1_data(inst);
  I.lb2 = make_lb2_data(I.lb1);
  return I;
}

namespace {

inline PFSPNode make_child(const PFSPNode& parent, int i) {
  PFSPNode child = parent;
  child.depth = static_cast<int8_t>(parent.depth + 1);
  child.limit1 = static_cast<int8_t>(parent.limit1 + 1);
  child.prmu[parent.depth] = parent.prmu[i];
  child.prmu[i] = parent.prmu[parent.depth];
  return child;
}

// pfsp_chpl.chpl:88-113 (lb1): bound each child from scratch.
void decompose_lb1(const PfspInstance& I, const PFSPNode& parent, uint64_t& tree, uint64_t& sol,
                   int& best, Pool<PFSPNode>& pool) {
  for (int i = parent.limit1 + 1; i < I.jobs; i++) {
    PFSPNode child = make_child(parent, i);
    int lb = lb1_bound(I.lb1, child.prmu, child.limit1, I.jobs);
    if (child.depth == I.jobs) {
      sol += 1;
      if (lb < best) best = lb;
    } else if (lb < best) {
      pool.pushBack(child);
      tree += 1;
    }
  }
}

// pfsp_chpl.chpl:115-145 (lb1_d): one incremental pass bounds all children.
void decompose_lb1_d(const PfspInstance& I, const PFSPNode& parent, uint64_t& tree,
                     uint64_t& sol, int& best, Pool<PFSPNode>& pool) {
  int lb_begin[MAX_JOBS];
  lb1_children_bounds(I.lb1, parent.prmu, parent.limit1, I.jobs, lb_begin);
  for (int i = parent.limit1 + 1; i < I.jobs; i++) {
    const int job = parent.prmu[i];
    const int lb = lb_begin[job];
    if (parent.depth + 1 == I.jobs) {
      sol += 1;
      if (lb < best) best = lb;
    } else if (lb < best) {
      pool.pushBack(make_child(parent, i));
      tree += 1;
    }
  }
}

// pfsp_chpl.chpl:147-172 (lb2).
void decompose_lb2(const PfspInstance& I, const PFSPNode& parent, uint64_t& tree, uint64_t& sol,
                   int& best, Pool<PFSPNode>& pool) {
  for (int i = parent.limit1 + 1; i < I.jobs; i++) {
    PFSPNode child = make_child(parent, i);
    int lb = lb2_bound(I.lb1, I.lb2, child.prmu, child.limit1, I.jobs, best);
    if (child.depth == I.jobs) {
      sol += 1;
      if (lb < best) best = lb;
    } else if (lb < best) {
      pool.pushBack(child);
      tree += 1;
    }
  }
}

// Children of a node that may already have jobs fixed at the back: the
// forward child fixes prmu[i] at position limit1 + 1, the backward child at
// position limit2 - 1 (limit2 = jobs - nback).
inline PFSPNode make_child_front(const PFSPNode& parent, int i) {
  PFSPNode child = parent;
  const int pos = parent.limit1 + 1;
  child.depth = static_cast<int8_t>(parent.depth + 1);
  child.limit1 = static_cast<int8_t>(pos);
  child.prmu[pos] = parent.prmu[i];
  child.prmu[i] = parent.prmu[pos];
  return child;
}

inline PFSPNode make_child_back(const PFSPNode& parent, int jobs, int i) {
  PFSPNode child = parent;
  const int pos = jobs - parent.nback - 1;
  child.depth = static_cast<int8_t>(parent.depth + 1);
  child.nback = static_cast<uint8_t>(parent.nback + 1);
  child.prmu[pos] = parent.prmu[i];
  child.prmu[i] = parent.prmu[pos];
  return child;
}

// Direction of a parent's children under a static rule.
inline bool static_backward(Branching br, int depth) {
  return br == Branching::BWD || (br == Branching::ALT && (depth & 1));
}

// MinBranch over the unscheduled positions [lo, hi): lbF(k) / lbB(k) give the
// two directions' bounds of the job at position k.
template <class F, class B>
inline bool choose_minbranch(int lo, int hi, int best, F&& lbF, B&& lbB) {
  int cntF = 0, cntB = 0;
  long long sumF = 0, sumB = 0;
  for (int k = lo; k < hi; k++) {
    const int f = lbF(k), b = lbB(k);
    cntF += f < best;
    cntB += b < best;
    sumF += f;
    sumB += b;
  }
  return minbranch_backward(cntF, cntB, sumF, sumB);
}

// Backward / alternating / dynamic branching (all three bounds; minbranch
// for lb1_d only). Pruning and leaf rules are those of the forward decompose.
void decompose_bi(const PfspInstance& I, LbKind lb, const PFSPNode& parent, uint64_t& tree,
                  uint64_t& sol, int& best, Pool<PFSPNode>& pool) {
  const int jobs = I.jobs;
  const int limit1 = parent.limit1, limit2 = jobs - parent.nback;
  const bool leaf = parent.depth + 1 == jobs;
  int lb_begin[MAX_JOBS], lb_end[MAX_JOBS];
  bool back;
  if (I.br == Branching::MINBRANCH) {
    if (lb != LbKind::LB1_D) check_branching_supported(lb, I.br, false);
    lb1_children_bounds_bi(I.lb1, parent.prmu, limit1, limit2, lb_begin, lb_end);
    back = choose_minbranch(
        limit1 + 1, limit2, best, [&](int k) { return lb_begin[parent.prmu[k]]; },
        [&](int k) { return lb_end[parent.prmu[k]]; });
  } else {
    back = static_backward(I.br, parent.depth);
    if (lb == LbKind::LB1_D)
      lb1_children_bounds_bi(I.lb1, parent.prmu, limit1, limit2, back ? nullptr : lb_begin,
                             back ? lb_end : nullptr);
  }
  for (int i = limit1 + 1; i < limit2; i++) {
    const PFSPNode child = back ? make_child_back(parent, jobs, i) : make_child_front(parent, i);
    int b;
    if (lb == LbKind::LB1_D)
      b = (back ? lb_end : lb_begin)[parent.prmu[i]];
    else if (lb == LbKind::LB1)
      b = lb1_bound(I.lb1, child.prmu, child.limit1, jobs - child.nback);
    else
      b = lb2_bound(I.lb1, I.lb2, child.prmu, child.limit1, jobs - child.nback, best);
    if (leaf) {
      sol += 1;
      if (b < best) best = b;
    } else if (b < best) {
      pool.pushBack(child);
      tree += 1;
    }
  }
}

// lb12: lb1_d picks the direction and filters the children, lb2 refines the
// survivors (evaluated against the incumbent, never at leaves).
void decompose_lb12(const PfspInstance& I, const PFSPNode& parent, uint64_t& tree,
                    uint64_t& sol, int& best, Pool<PFSPNode>& pool) {
  const int jobs = I.jobs;
  uint8_t dir;
  int32_t b[MAX_JOBS];
  pfsp_lb12_eval(I, parent, best, dir, b);
  const bool leaf = parent.depth + 1 == jobs;
  for (int i = parent.limit1 + 1; i < jobs - parent.nback; i++) {
    if (leaf) {
      sol += 1;
      if (b[i] < best) best = b[i];
    } else if (b[i] < best) {
      pool.pushBack(dir ? make_child_back(parent, jobs, i) : make_child_front(parent, i));
      tree += 1;
    }
  }
}

}  // namespace

void pfsp_lb12_eval(const PfspInstance& I, const PFSPNode& parent, int best, uint8_t& dir,
                    int32_t* bounds) {
  const int jobs = I.jobs;
  const int limit1 = parent.limit1, limit2 = jobs - parent.nback;
  const bool leaf = parent.depth + 1 == jobs;
  int lb_begin[MAX_JOBS], lb_end[MAX_JOBS];
  bool back;
  if (I.br == Branching::MINBRANCH) {
    lb1_children_bounds_bi(I.lb1, parent.prmu, limit1, limit2, lb_begin, lb_end);
    back = choose_minbranch(
        limit1 + 1, limit2, best, [&](int k) { return lb_begin[parent.prmu[k]]; },
        [&](int k) { return lb_end[parent.prmu[k]]; });
  } else {
    back = static_backward(I.br, parent.depth);
    lb1_children_bounds_bi(I.lb1, parent.prmu, limit1, limit2, back ? nullptr : lb_begin,
                           back ? lb_end : nullptr);
  }
  dir = back ? 1 : 0;
  for (int i = 0; i < jobs; i++) bounds[i] = -1;
  for (int i = limit1 + 1; i < limit2; i++) {
    const int b1 = (back ? lb_end : lb_begin)[parent.prmu[i]];
    if (leaf || b1 >= best) {  // leaves keep the lb1_d rule; a filtered child costs no lb2
      bounds[i] = b1;
      continue;
    }
    const PFSPNode child = back ? make_child_back(parent, jobs, i) : make_child_front(parent, i);
    bounds[i] = lb2_bound(I.lb1, I.lb2, child.prmu, child.limit1, jobs - child.nback, best);
  }
}

void pfsp_decompose(const PfspInstance& I, LbKind lb, const PFSPNode& parent, uint64_t& tree,
                    uint64_t& sol, int& best, Pool<PFSPNode>& pool) {
  if (lb == LbKind::LB12) {
    decompose_lb12(I, parent, tree, sol, best, pool);
    return;
  }
  if (I.br != Branching::FWD) {
    decompose_bi(I, lb, parent, tree, sol, best, pool);
    return;
  }
  switch (lb) {
    case LbKind::LB1:
      decompose_lb1(I, parent, tree, sol, best, pool);
      break;
    case LbKind::LB1_D:
      decompose_lb1_d(I, parent, tree, sol, best, pool);
      break;
    case LbKind::LB2:
      decompose_lb2(I, parent, tree, sol, best, pool);
      break;
    case LbKind::LB12:
      break;  // handled above
  }
}

Result pfsp_seq(int inst, const std::string& lb_str, int ub, const std::string& br_str) {
  const LbKind lb = lb_from_string(lb_str);
  const Branching br = branching_from_string(br_str);
  check_branching_supported(lb, br, false);
  Result r;
  PfspInstance I = make_pfsp_instance(inst, ub, br);
  int best = I.init_ub;
  Pool<PFSPNode> pool;
  pool.pushBack(pfsp_root());
  const double t0 = now_sec();
  PFSPNode parent;
  while (pool.popBack(parent)) pfsp_decompose(I, lb, parent, r.tree, r.sol, best, pool);
  r.time = now_sec() - t0;
  r.optimum = best;
  r.phases.push_back({r.tree, r.sol, r.time});
  return r;
}

void pfsp_bfs_until(const PfspInstance& I, LbKind lb, size_t target, Pool<PFSPNode>& pool,
                    uint64_t& tree, uint64_t& sol, int& best) {
  PFSPNode parent;
  while (pool.size() < target) {
    if (!pool.popFront(parent)) break;
    pfsp_decompose(I, lb, parent, tree, sol, best, pool);
  }
}

void pfsp_generate_children(const PfspInstance& I, const PFSPNode* parents, size_t n,
                            const int32_t* bounds, uint64_t& tree, uint64_t& sol, int& best,
                            Pool<PFSPNode>& pool) {
  for (size_t i = 0; i < n; i++) {
    const PFSPNode& parent = parents[i];
    const int depth = parent.depth;
    for (int j = parent.limit1 + 1; j < I.jobs; j++) {
      const int lb = bounds[i * I.jobs + j];
      if (depth + 1 == I.jobs) {
        sol += 1;
        if (lb < best) best = lb;
      } else if (lb < best) {
        pool.pushBack(make_child(parent, j));
        tree += 1;
      }
    }
  }
}

void pfsp_generate_children_bi(const PfspInstance& I, const PFSPNode* parents, size_t n,
                               const int32_t* lb_begin, const int32_t* lb_end,
                               uint64_t& tree, uint64_t& sol, int& best,
                               Pool<PFSPNode>& pool) {
  const int jobs = I.jobs;
  for (size_t i = 0; i < n; i++) {
    const PFSPNode& parent = parents[i];
    const int lo = parent.limit1 + 1, hi = jobs - parent.nback;
    const int32_t* f = lb_begin + i * jobs;
    const int32_t* b = lb_end + i * jobs;
    const bool back =
        I.br == Branching::MINBRANCH
            ? choose_minbranch(
                  lo, hi, best, [&](int k) { return f[k]; }, [&](int k) { return b[k]; })
            : static_backward(I.br, parent.depth);
    const bool leaf = parent.depth + 1 == jobs;
    for (int j = lo; j < hi; j++) {
      const int lb = back ? b[j] : f[j];
      if (leaf) {
        sol += 1;
        if (lb < best) best = lb;
      } else if (lb < best) {
        pool.pushBack(back ? make_child_back(parent, jobs, j) : make_child_front(parent, j));
        tree += 1;
      }
    }
  }
}

void pfsp_generate_children_lb12(const PfspInstance& I, const PFSPNode* parents, size_t n,
                                 const uint8_t* dir, const int32_t* bounds, uint64_t& tree,
                                 uint64_t& sol, int& best, Pool<PFSPNode>& pool) {
  const int jobs = I.jobs;
  for (size_t i = 0; i < n; i++) {
    const PFSPNode& parent = parents[i];
    const bool back = dir[i] != 0;
    const bool leaf = parent.depth + 1 == jobs;
    for (int j = parent.limit1 + 1; j < jobs - parent.nback; j++) {
      const int lb = bounds[i * jobs + j];
      if (leaf) {
        sol += 1;
        if (lb < best) best = lb;
      } else if (lb < best) {
        pool.pushBack(back ? make_child_back(parent, jobs, j) : make_child_front(parent, j));
        tree += 1;
      }
    }
  }
}

}  // namespace gats
