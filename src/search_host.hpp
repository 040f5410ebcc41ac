// Host-side search engines: sequential DFS drivers + the CPU decompose
// routines shared by every tier (phase-1 BFS, phase-3 drain, generate_children).
//
// Parity: reference sequential drivers `nqueens_chpl.chpl` (decompose :70-89,
// nqueens_search :92-113) and `pfsp_chpl.chpl` (decompose_lb1 :88, lb1_d :115,
// lb2 :147, pfsp_search :191).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "bounds.hpp"
#include "nodes.hpp"
#include "pool.hpp"

namespace gats {

struct PhaseStats {
  uint64_t tree = 0, sol = 0;
  double time = 0.0;
};

struct Result {
  uint64_t tree = 0, sol = 0;
  int optimum = 0;  // PFSP only (final best makespan)
  double time = 0.0;
  std::vector<PhaseStats> phases;
  // GPU diagnostics (GpuDiagnostics parity, nqueens_gpu_chpl.chpl:278-282)
  uint64_t kernel_launch = 0, h2d = 0, d2h = 0;
  uint64_t h2d_bytes = 0, d2h_bytes = 0;
  uint64_t gpu_iters = 0;
  double gpu_time = 0.0;  // cumulative device-loop wall time
  std::vector<uint64_t> per_worker;  // multi-GPU tier: explored tree per worker
                                     // (workload-share print parity,
                                     // nqueens_multigpu_chpl.chpl:337)
};

// LB12 is the two-stage bound: lb1_d picks the branching direction and filters
// the children, lb2 (Johnson) then bounds only the survivors.
enum class LbKind { LB1, LB1_D, LB2, LB12 };
LbKind lb_from_string(const std::string& s);

// ---------------- N-Queens ----------------

// Diagonal-safety check for placing board[j] at column `depth`
// (nqueens_chpl.chpl:51-67); g repeats the check to scale artificial work.
bool nq_is_safe(const uint8_t* board, int depth, int row_pos, int g);

// Expand one parent into the pool; counts pushed children in `tree` and
// depth==N leaves in `sol` (nqueens_chpl.chpl:70-89).
void nq_decompose(const NQNode& parent, int N, int g, uint64_t& tree, uint64_t& sol,
                  Pool<NQNode>& pool);

Result nqueens_seq(int N, int g);

// Partial BFS (popFront) until pool.size >= target; phase 1 of every GPU tier
// (nqueens_gpu_chpl.chpl:169-175).
void nq_bfs_until(int N, int g, size_t target, Pool<NQNode>& pool, uint64_t& tree,
                  uint64_t& sol);

// Deterministic PARALLEL level-synchronous BFS: expands whole depth levels
// with up to 16 host threads until the frontier reaches `target` (may
// overshoot by one level) or the tree is exhausted. The frontier is identical
// for any thread count (children concatenated in parent order), so every rank
// of the distributed tier computes the same partition redundantly
// (pfsp_dist_multigpu_cuda.c:372-378's trick) without the serial-BFS cost.
void nq_bfs_level(int N, int g, size_t target, Pool<NQNode>& pool, uint64_t& tree,
                  uint64_t& sol);

// ---------------- PFSP ----------------

// Branching rule (beyond the reference, which branches forward only,
// pfsp_chpl.chpl:29-32). A node fixes jobs at the front (limit1) and at the
// back (nback) of the permutation; the rule picks, per parent, on which side
// its children fix their job:
//   FWD        always the front (the reference's tree; the default)
//   BWD        always the back
//   ALT        front when the parent's depth is even, back when odd
//   MINBRANCH  (lb1_d and lb12) the side with fewer children surviving the
//              incumbent under lb1_d; on a tie the side with the larger bound sum
enum class Branching { FWD = 0, BWD = 1, ALT = 2, MINBRANCH = 3 };
Branching branching_from_string(const std::string& s);
const char* branching_name(Branching br);
// Throws std::invalid_argument naming the combination when `lb` has no
// implementation of `br` (minbranch needs both directions' bounds of every
// child, which only lb1_d produces in one pass). gpu_tier adds the GPU tier's
// restriction: its bi-directional kernels exist for lb1_d only. lb12 has its
// own decompose rule and kernels and takes every rule on both tiers.
void check_branching_supported(LbKind lb, Branching br, bool gpu_tier);

// A pool handed in from outside (the *_from_pool entry points): under fwd the
// decompose rules and the forward kernels take limit2 == jobs for granted, so
// a node with jobs fixed at the back (e.g. a minbranch frontier passed on
// without its rule) throws std::invalid_argument instead of silently
// searching another tree.
void check_pfsp_pool(const PFSPNode* nodes, size_t n, Branching br);

// MinBranch decision from the two directions' survivor counts and bound sums:
// true = branch backward.
inline bool minbranch_backward(int cntF, int cntB, long long sumF, long long sumB) {
  return cntB < cntF || (cntB == cntF && sumB > sumF);
}

struct PfspInstance {
  int inst = 0, jobs = 0, machines = 0, init_ub = 0;
  Branching br = Branching::FWD;
  Lb1Data lb1;
  Lb2Data lb2;
};
PfspInstance make_pfsp_instance(int inst, int ub, Branching br = Branching::FWD);

void pfsp_decompose(const PfspInstance& I, LbKind lb, const PFSPNode& parent, uint64_t& tree,
                    uint64_t& sol, int& best, Pool<PFSPNode>& pool);

Result pfsp_seq(int inst, const std::string& lb, int ub, const std::string& br = "fwd");

void pfsp_bfs_until(const PfspInstance& I, LbKind lb, size_t target, Pool<PFSPNode>& pool,
                    uint64_t& tree, uint64_t& sol, int& best);

// Host-side generate_children from GPU-evaluated child bounds
// (pfsp_gpu_chpl.chpl:273-303): bounds[i*jobs + j] is the bound of parent i's
// child obtained by scheduling prmu[j] next.
void pfsp_generate_children(const PfspInstance& I, const PFSPNode* parents, size_t n,
                            const int32_t* bounds, uint64_t& tree, uint64_t& sol, int& best,
                            Pool<PFSPNode>& pool);

// Both-directions variant (hostpool, lb1_d, non-fwd rules): lb_begin / lb_end
// hold, per parent and POSITION j, the bound of the child that fixes prmu[j]
// at the front / at the back. The direction is chosen per parent on the host
// by I.br, with the same rule as the sequential decompose.
void pfsp_generate_children_bi(const PfspInstance& I, const PFSPNode* parents, size_t n,
                               const int32_t* lb_begin, const int32_t* lb_end,
                               uint64_t& tree, uint64_t& sol, int& best,
                               Pool<PFSPNode>& pool);

// lb12 for one parent (the definition the kernels are tested against): the
// direction (0 front, 1 back) chosen by I.br on the lb1_d values, and per
// POSITION -1 outside the unscheduled range, the lb1_d value of the chosen
// direction for a leaf's children and for children with lb1_d >= best, and
// otherwise lb2_bound of the child (early exit: exact when <= best).
void pfsp_lb12_eval(const PfspInstance& I, const PFSPNode& parent, int best, uint8_t& dir,
                    int32_t* bounds);

// Hostpool, lb12: dir[i] / bounds[i*jobs + j] as pfsp_lb12_eval lays them out,
// evaluated on the GPU with the batch's incumbent (>= the live one, so a
// value that pruned there prunes here too).
void pfsp_generate_children_lb12(const PfspInstance& I, const PFSPNode* parents, size_t n,
                                 const uint8_t* dir, const int32_t* bounds, uint64_t& tree,
                                 uint64_t& sol, int& best, Pool<PFSPNode>& pool);

// N-Queens variant from GPU safety labels (nqueens_gpu_chpl.chpl:126-149).
void nq_generate_children(const NQNode* parents, size_t n, int N, const uint8_t* labels,
                          uint64_t& tree, uint64_t& sol, Pool<NQNode>& pool);

double now_sec();

}  // namespace gats
