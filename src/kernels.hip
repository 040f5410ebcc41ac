// CDNA4 (gfx950) kernels for the tree-search framework.
//
// Functional parity targets (semantics, not code, from the reference):
//   - N-Queens evaluate:      baselines/nqueens/nqueens_gpu_cuda.cu:137-164
//   - PFSP lb1 / lb1_d / lb2: baselines/pfsp/lib/c_bounds_gpu.cu + evaluate.cu:25-91
//
// MI355X-first design decisions (NOT a port):
//   * 24-byte packed nodes (int8 permutations) instead of 88 B int32 nodes.
//   * Two modes:
//       "hostpool"  — reference-shaped: kernel evaluates labels/bounds, host
//                     prunes and branches (used for oracle parity tests).
//       "devpool"   — device-resident pool: two kernels per offload round
//                     (expand-compact + self-prefixing gather with parity
//                     control blocks) keep the entire hot loop on the GPU;
//                     the host only polls a 64 B control block every few
//                     iterations. No global atomics on the hot path.
//   * Bound tables staged in LDS (p_times int16; Johnson entries packed into
//     one u32 per (pair, position): job<<27|lag<<16|ptm1<<8|ptm0): ~16 KB
//     for 20x20 vs 160 KB per CU.
//   * No runtime-indexed per-thread arrays (they would spill to scratch on
//     CDNA4): machine loops are fully unrolled via a machine-count template
//     parameter; lb2's machine pairs are a compile-time lexicographic map;
//     lb1_d iterates positions instead of a job-indexed local array.
//   * Wavefront = 64 idioms throughout (__ballot is 64-bit).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <stdexcept>
#include <type_traits>

#include "gpu_api.hpp"
#include "nq_finish.hpp"

namespace gats {

#define BLOCK 256

// ---------------------------------------------------------------------------
// Shared helpers (LDS staging, child emission)
// ---------------------------------------------------------------------------

// Block-cooperative staging of the parents this block touches into LDS.
// One shared copy per parent (the reference's per-thread `var parent =
// parents_d[parentId]` would be a 96 B/thread scratch/LDS spill on CDNA4
// because board/prmu are runtime-indexed). Caller must __syncthreads() after.
// Returns this thread's local parent index, or -1 if t >= total.
template <class NodeT, int MAXN>
__device__ inline int stage_parents(const NodeT* parents, unsigned long long total,
                                    int per_parent, NodeT (&snodes)[MAXN],
                                    unsigned long long t) {
  const unsigned long long t0 = static_cast<unsigned long long>(blockIdx.x) * blockDim.x;
  if (t0 >= total) return -1;
  const unsigned int first = static_cast<unsigned int>(t0 / per_parent);
  unsigned long long tlast = t0 + blockDim.x - 1;
  if (tlast > total - 1) tlast = total - 1;
  const unsigned int last = static_cast<unsigned int>(tlast / per_parent);
  const int nblk = static_cast<int>(last - first + 1);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(parents + first);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&snodes[0]);
  const int words = nblk * static_cast<int>(sizeof(NodeT) / 4);
  for (int i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
  if (t >= total) return -1;
  return static_cast<int>(t / per_parent - first);
}

// Emit a child node straight into its pool slot: three patched qword stores
// plus two byte stores for the swapped permutation entries — avoids any
// runtime-indexed private array (scratch) for the child.
__device__ inline void emit_nq_child(NQNode* pool, unsigned long long slot,
                                     const NQNode& parent, int depth, int k) {
  const unsigned long long* s = reinterpret_cast<const unsigned long long*>(&parent);
  unsigned long long* d = reinterpret_cast<unsigned long long*>(&pool[slot]);
  // byte 0 = depth; board bytes at 1..20
  d[0] = (s[0] & ~0xFFull) | static_cast<unsigned long long>(depth + 1);
  d[1] = s[1];
  d[2] = s[2];
  uint8_t* db = reinterpret_cast<uint8_t*>(d);
  db[1 + depth] = parent.board[k];
  db[1 + k] = parent.board[depth];
}

__device__ inline void emit_pfsp_child(PFSPNode* pool, unsigned long long slot,
                                       const PFSPNode& parent, int depth, int limit1,
                                       int k) {
  const unsigned long long* s = reinterpret_cast<const unsigned long long*>(&parent);
  unsigned long long* d = reinterpret_cast<unsigned long long*>(&pool[slot]);
  // byte 0 = depth, byte 1 = limit1; prmu bytes at 2..21
  d[0] = (s[0] & ~0xFFFFull) |
         static_cast<unsigned long long>(static_cast<uint8_t>(depth + 1)) |
         (static_cast<unsigned long long>(static_cast<uint8_t>(limit1 + 1)) << 8);
  d[1] = s[1];
  d[2] = s[2];
  uint8_t* db = reinterpret_cast<uint8_t*>(d);
  db[2 + depth] = parent.prmu[k];
  db[2 + k] = parent.prmu[depth];
}

// Children of a node that may have jobs fixed at the back (nback > 0,
// backward / dynamic branching). The forward child fixes prmu[k] at position
// limit1 + 1 (== depth only while nback == 0, which is why emit_pfsp_child
// cannot be reused): bytes 0, 1 and the two swapped prmu bytes change.
__device__ inline void emit_pfsp_child_front(PFSPNode* pool, unsigned long long slot,
                                             const PFSPNode& parent, int depth, int limit1,
                                             int k) {
  const unsigned long long* s = reinterpret_cast<const unsigned long long*>(&parent);
  unsigned long long* d = reinterpret_cast<unsigned long long*>(&pool[slot]);
  d[0] = (s[0] & ~0xFFFFull) |
         static_cast<unsigned long long>(static_cast<uint8_t>(depth + 1)) |
         (static_cast<unsigned long long>(static_cast<uint8_t>(limit1 + 1)) << 8);
  d[1] = s[1];
  d[2] = s[2];
  uint8_t* db = reinterpret_cast<uint8_t*>(d);
  const int pos = limit1 + 1;
  db[2 + pos] = parent.prmu[k];
  db[2 + k] = parent.prmu[pos];
}

// The backward child fixes prmu[k] at position limit2 - 1 = jobs - nback - 1:
// byte 0 (depth), byte 22 (nback) and the two swapped prmu bytes change.
__device__ inline void emit_pfsp_child_back(PFSPNode* pool, unsigned long long slot,
                                            const PFSPNode& parent, int depth, int nback,
                                            int jobs, int k) {
  const unsigned long long* s = reinterpret_cast<const unsigned long long*>(&parent);
  unsigned long long* d = reinterpret_cast<unsigned long long*>(&pool[slot]);
  d[0] = (s[0] & ~0xFFull) | static_cast<unsigned long long>(static_cast<uint8_t>(depth + 1));
  d[1] = s[1];
  // byte 22 is bits 48..55 of the third qword
  d[2] = (s[2] & ~(0xFFull << 48)) |
         (static_cast<unsigned long long>(static_cast<uint8_t>(nback + 1)) << 48);
  uint8_t* db = reinterpret_cast<uint8_t*>(d);
  const int pos = jobs - nback - 1;
  db[2 + pos] = parent.prmu[k];
  db[2 + k] = parent.prmu[pos];
}

// ---------------------------------------------------------------------------
// N-Queens
// ---------------------------------------------------------------------------

// Diagonal safety of placing row `q` at column `depth` against columns [0,depth).
// g repeats every check (the reference's artificial-work knob,
// nqueens_gpu_cuda.cu:137-164); the empty asm is an optimization barrier so
// the repeats are real work the compiler cannot hoist out of the loop.
__device__ inline uint8_t nq_safe(const uint8_t* board, int depth, int q, int g) {
  uint8_t safe = 1;
  for (int i = 0; i < depth; i++) {
    const int o = board[i];
    for (int r = 0; r < g; r++) {
      int qq = q;
      if (g > 1) asm volatile("" : "+v"(qq));
      safe &= (o != qq - (depth - i)) & (o != qq + (depth - i));
    }
  }
  return safe;
}

// hostpool mode: one thread per (parent, k), labels out
// (reference mapping nqueens_gpu_cuda.cu:137-164).
__global__ void k_nq_eval(const NQNode* parents, int n, int N, int g, uint8_t* labels) {
  __shared__ NQNode snodes[BLOCK + 2];
  const unsigned long long t =
      static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int lp = stage_parents(parents, static_cast<unsigned long long>(n) * N, N, snodes, t);
  __syncthreads();
  if (lp < 0) return;
  const int k = static_cast<int>(t % static_cast<unsigned long long>(N));
  const NQNode& parent = snodes[lp];
  const int depth = parent.depth;
  if (k >= depth && depth < N)
    labels[t] = nq_safe(parent.board, depth, parent.board[k], g);
}

// ---------------------------------------------------------------------------
// PFSP device bound math (templated on machine count MM for full unrolling;
// every per-thread array index is compile-time so nothing spills to scratch).
// ---------------------------------------------------------------------------

template <int MM>
struct LdsLb1 {
  int16_t p[MM * MAX_JOBS];  // p_times[machine][job]
  int32_t min_tails[MM];
};

// LB2_FULL's machine-pair list is the deterministic lexicographic (i < j)
// enumeration (c_bound_johnson.c:57-70): with the pair loop fully unrolled
// these fold to compile-time constants, so the pair-indexed `front` reads
// become register accesses (the earlier design kept a 21.5 KB per-block LDS
// scratch for runtime-indexed front, capping occupancy at 3 blocks/CU).
template <int MM>
__host__ __device__ constexpr int pair_first(int l) {
  int i = 0, rem = l;
  while (rem >= MM - 1 - i) {
    rem -= MM - 1 - i;
    i++;
  }
  return i;
}
template <int MM>
__host__ __device__ constexpr int pair_second(int l) {
  return pair_first<MM>(l) + 1 + (l - (pair_first<MM>(l) * (2 * MM - pair_first<MM>(l) - 1)) / 2);
}

template <int MM>
struct LdsLb2 {
  static constexpr int PAIRS = MM * (MM - 1) / 2;
  int16_t p[MM * MAX_JOBS];
  int32_t min_tails[MM];
  uint32_t jp[PAIRS * MAX_JOBS];  // packed johnson: job<<27|lag<<16|ptm1<<8|ptm0
};

template <int MM, class LDS>
__device__ inline void stage_lb1_tables(LDS& lds, const PfspDevTables& tb, int jobs) {
  for (int i = threadIdx.x; i < MM * jobs; i += blockDim.x) lds.p[i] = tb.p_times[i];
  if (threadIdx.x < MM) lds.min_tails[threadIdx.x] = tb.min_tails[threadIdx.x];
}

template <int MM>
__device__ inline void stage_lb2_tables(LdsLb2<MM>& lds, const PfspDevTables& tb, int jobs) {
  stage_lb1_tables<MM>(lds, tb, jobs);
  constexpr int PAIRS = LdsLb2<MM>::PAIRS;
  for (int i = threadIdx.x; i < PAIRS * jobs; i += blockDim.x)
    lds.jp[i] = tb.johnson_packed[i];
}

// front <- completion times of the child prefix (parent prefix + job k placed
// at position depth); c_bound_simple.c:31-69 without materializing the swap.
// `front` may be a register array (compile-time indexed here) or LDS.
template <int MM, class LDS>
__device__ inline void child_front(const LDS& lds, const uint8_t* prmu, int depth, int job_k,
                                   int jobs, int* front, int stride) {
#pragma unroll
  for (int i = 0; i < MM; i++) front[i * stride] = 0;
  for (int i = 0; i < depth; i++) {
    const int job = prmu[i];
    front[0] += lds.p[job];
#pragma unroll
    for (int j = 1; j < MM; j++) {
      const int prev = max(front[(j - 1) * stride], front[j * stride]);
      front[j * stride] = prev + lds.p[j * jobs + job];
    }
  }
  front[0] += lds.p[job_k];
#pragma unroll
  for (int j = 1; j < MM; j++) {
    const int prev = max(front[(j - 1) * stride], front[j * stride]);
    front[j * stride] = prev + lds.p[j * jobs + job_k];
  }
}

// lb1 bound of the child that schedules prmu[k] next (c_bound_simple.c:143-158;
// limit2 == jobs, so the back schedule is the constant min_tails row,
// SURVEY.md §8.2).
template <int MM>
__device__ inline int lb1_child_bound(const LdsLb1<MM>& lds, const uint8_t* prmu, int depth,
                                      int k, int jobs) {
  int front[MM];
  child_front<MM>(lds, prmu, depth, prmu[k], jobs, front, 1);

  int remain[MM];
#pragma unroll
  for (int i = 0; i < MM; i++) remain[i] = 0;
  for (int i = depth; i < jobs; i++) {
    if (i == k) continue;  // job k moved into the prefix
    const int job = prmu[i];
#pragma unroll
    for (int j = 0; j < MM; j++) remain[j] += lds.p[j * jobs + job];
  }

  int tmp0 = front[0] + remain[0];
  int lb = tmp0 + lds.min_tails[0];
#pragma unroll
  for (int i = 1; i < MM; i++) {
    const int tmp1 = max(tmp0, front[i] + remain[i]);
    lb = max(lb, tmp1 + lds.min_tails[i]);
    tmp0 = tmp1;
  }
  return lb;
}

// lb1_d setup: parent-prefix front + remain over unscheduled jobs
// (c_bound_simple.c:52-69,109-124). Register arrays, compile-time indexed.
template <int MM>
__device__ inline void lb1d_setup(const LdsLb1<MM>& lds, const uint8_t* prmu, int limit1,
                                  int jobs, int* front, int* remain) {
#pragma unroll
  for (int i = 0; i < MM; i++) front[i] = remain[i] = 0;
  for (int i = 0; i <= limit1; i++) {
    const int job = prmu[i];
    front[0] += lds.p[job];
#pragma unroll
    for (int j = 1; j < MM; j++) front[j] = max(front[j - 1], front[j]) + lds.p[j * jobs + job];
  }
  for (int i = limit1 + 1; i < jobs; i++) {
    const int job = prmu[i];
#pragma unroll
    for (int j = 0; j < MM; j++) remain[j] += lds.p[j * jobs + job];
  }
}

// O(m) incremental child bound from the parent's front/remain
// (add_front_and_bound, c_bound_simple.c:218-244). remain still contains the
// child job itself: lb1_d is a deliberately different bound than lb1.
template <int MM>
__device__ inline int lb1d_child_bound(const LdsLb1<MM>& lds, const int* front,
                                       const int* remain, int job, int jobs) {
  int lb = front[0] + remain[0] + lds.min_tails[0];
  int tmp0 = front[0] + lds.p[job];
#pragma unroll
  for (int j = 1; j < MM; j++) {
    const int tmp1 = max(tmp0, front[j]);
    lb = max(lb, tmp1 + remain[j] + lds.min_tails[j]);
    tmp0 = tmp1 + lds.p[j * jobs + job];
  }
  return lb;
}

// ---- lb1_d in both directions (backward / dynamic branching) ----

template <int MM>
struct LdsLb1Bi {
  int16_t p[MM * MAX_JOBS];
  int32_t min_tails[MM];
  int32_t min_heads[MM];
};

template <int MM>
__device__ inline void stage_lb1bi_tables(LdsLb1Bi<MM>& lds, const PfspDevTables& tb,
                                          int jobs) {
  stage_lb1_tables<MM>(lds, tb, jobs);
  if (threadIdx.x < MM) lds.min_heads[threadIdx.x] = tb.min_heads[threadIdx.x];
}

// Parent state shared by all of its children in both directions
// (c_bound_simple.c:52-124): front = schedule_front (min_heads when nothing is
// fixed at the front), back = schedule_back (min_tails when nothing is fixed
// at the back), remain = work of the unscheduled positions [limit1+1, limit2).
// Three register arrays, every machine index compile-time.
template <int MM>
__device__ inline void lb1d_bi_setup(const LdsLb1Bi<MM>& lds, const uint8_t* prmu, int limit1,
                                     int limit2, int jobs, int* front, int* back,
                                     int* remain) {
#pragma unroll
  for (int i = 0; i < MM; i++) front[i] = back[i] = remain[i] = 0;
  if (limit1 == -1) {
#pragma unroll
    for (int i = 0; i < MM; i++) front[i] = lds.min_heads[i];
  } else {
    for (int i = 0; i <= limit1; i++) {
      const int job = prmu[i];
      front[0] += lds.p[job];
#pragma unroll
      for (int j = 1; j < MM; j++)
        front[j] = max(front[j - 1], front[j]) + lds.p[j * jobs + job];
    }
  }
  if (limit2 == jobs) {
#pragma unroll
    for (int i = 0; i < MM; i++) back[i] = lds.min_tails[i];
  } else {
    for (int k = jobs - 1; k >= limit2; k--) {
      const int job = prmu[k];
      back[MM - 1] += lds.p[(MM - 1) * jobs + job];
#pragma unroll
      for (int jj = 0; jj < MM - 1; jj++) {
        constexpr int last = MM - 2;
        const int j = last - jj;  // MM-2 .. 0, compile-time after unrolling
        back[j] = max(back[j], back[j + 1]) + lds.p[j * jobs + job];
      }
    }
  }
  for (int i = limit1 + 1; i < limit2; i++) {
    const int job = prmu[i];
#pragma unroll
    for (int j = 0; j < MM; j++) remain[j] += lds.p[j * jobs + job];
  }
}

// add_front_and_bound with a general back schedule (c_bound_simple.c:218-244).
template <int MM>
__device__ inline int lb1d_bound_front(const LdsLb1Bi<MM>& lds, const int* front,
                                       const int* back, const int* remain, int job,
                                       int jobs) {
  int lb = front[0] + remain[0] + back[0];
  int tmp0 = front[0] + lds.p[job];
#pragma unroll
  for (int j = 1; j < MM; j++) {
    const int tmp1 = max(tmp0, front[j]);
    lb = max(lb, tmp1 + remain[j] + back[j]);
    tmp0 = tmp1 + lds.p[j * jobs + job];
  }
  return lb;
}

// add_back_and_bound (c_bound_simple.c:246-275): the mirror image — machines
// in descending order, front and back swap roles.
template <int MM>
__device__ inline int lb1d_bound_back(const LdsLb1Bi<MM>& lds, const int* front,
                                      const int* back, const int* remain, int job,
                                      int jobs) {
  int lb = front[MM - 1] + remain[MM - 1] + back[MM - 1];
  int tmp0 = back[MM - 1] + lds.p[(MM - 1) * jobs + job];
#pragma unroll
  for (int jj = 0; jj < MM - 1; jj++) {
    const int j = MM - 2 - jj;  // MM-2 .. 0
    const int tmp1 = max(tmp0, back[j]);
    lb = max(lb, tmp1 + remain[j] + front[j]);
    tmp0 = tmp1 + lds.p[j * jobs + job];
  }
  return lb;
}

// lb2: Johnson two-machine relaxation over all machine pairs with early exit
// (c_bound_johnson.c:211-254). Pair order is identity (LB2_FULL). `front` is
// this thread's LDS slice (runtime-indexed by pair machine ids).
template <int MM>
__device__ inline int lb2_child_bound(const LdsLb2<MM>& lds, const uint8_t* prmu, int depth,
                                      int k, int jobs, int best) {
  int front[MM];
  const int job_k = prmu[k];
  child_front<MM>(lds, prmu, depth, job_k, jobs, front, 1);

  unsigned int scheduled = 0;
  for (int i = 0; i < depth; i++) scheduled |= 1u << prmu[i];
  scheduled |= 1u << job_k;

  constexpr int PAIRS = LdsLb2<MM>::PAIRS;
  int lb = 0;
  // fully unrolled over the compile-time pair list; two pairs in flight per
  // step (each pair's update chain is serial — interleaving two independent
  // chains hides the ds_read_b64 latency)
#pragma unroll
  for (int l = 0; l < PAIRS; l += 2) {
    const bool two = (l + 1) < PAIRS;
    const int ma0a = pair_first<MM>(l), ma1a = pair_second<MM>(l);
    const int ma0b = pair_first<MM>(two ? l + 1 : l), ma1b = pair_second<MM>(two ? l + 1 : l);
    int t0a = front[ma0a], t1a = front[ma1a];
    int t0b = front[ma0b], t1b = front[ma1b];
    const uint32_t* jpa = &lds.jp[l * jobs];
    const uint32_t* jpb = &lds.jp[(two ? l + 1 : l) * jobs];
    // jobs == MAX_JOBS for every GPU-supported instance: full unrolling
    // batches the dependent ds_read_b32s (see the wave kernel's note)
    if (jobs == MAX_JOBS) {
#pragma unroll
      for (int j = 0; j < MAX_JOBS; j++) {
        const uint32_t va = jpa[j];  // one ds_read_b32 replaces 4 scalar LDS reads
        const uint32_t vb = jpb[j];
        const int ja = static_cast<int>(va >> 27);
        const int jb = static_cast<int>(vb >> 27);
        if (!(scheduled >> ja & 1u)) {
          t0a += static_cast<int>(va & 0xffu);
          t1a = max(t1a, t0a + static_cast<int>((va >> 16) & 0x7ffu));
          t1a += static_cast<int>((va >> 8) & 0xffu);
        }
        if (!(scheduled >> jb & 1u)) {
          t0b += static_cast<int>(vb & 0xffu);
          t1b = max(t1b, t0b + static_cast<int>((vb >> 16) & 0x7ffu));
          t1b += static_cast<int>((vb >> 8) & 0xffu);
        }
      }
    } else {
      for (int j = 0; j < jobs; j++) {
        const uint32_t va = jpa[j];
        const uint32_t vb = jpb[j];
        const int ja = static_cast<int>(va >> 27);
        const int jb = static_cast<int>(vb >> 27);
        if (!(scheduled >> ja & 1u)) {
          t0a += static_cast<int>(va & 0xffu);
          t1a = max(t1a, t0a + static_cast<int>((va >> 16) & 0x7ffu));
          t1a += static_cast<int>((va >> 8) & 0xffu);
        }
        if (!(scheduled >> jb & 1u)) {
          t0b += static_cast<int>(vb & 0xffu);
          t1b = max(t1b, t0b + static_cast<int>((vb >> 16) & 0x7ffu));
          t1b += static_cast<int>((vb >> 8) & 0xffu);
        }
      }
    }
    // merge pair a, check, then pair b: keeps the returned value bit-equal to
    // the reference's per-pair early exit (c_bound_johnson.c:231-233), which
    // the hostpool-vs-CPU-oracle tests assert
    lb = max(lb, max(t1a + lds.min_tails[ma1a], t0a + lds.min_tails[ma0a]));
    if (lb > best) break;
    if (two) {
      lb = max(lb, max(t1b + lds.min_tails[ma1b], t0b + lds.min_tails[ma0b]));
      if (lb > best) break;
    }
  }
  return lb;
}

// ---------------------------------------------------------------------------
// PFSP hostpool kernels: bounds out, host prunes (oracle-comparable).
// ---------------------------------------------------------------------------

template <int MM>
__global__ void k_pfsp_eval_lb1(const PFSPNode* parents, int n, int jobs, PfspDevTables tb,
                                int32_t* bounds) {
  __shared__ LdsLb1<MM> lds;
  __shared__ PFSPNode snodes[BLOCK / 5 + 2];
  stage_lb1_tables<MM>(lds, tb, jobs);
  const unsigned long long t =
      static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int lp =
      stage_parents(parents, static_cast<unsigned long long>(n) * jobs, jobs, snodes, t);
  __syncthreads();
  if (lp < 0) return;
  const int k = static_cast<int>(t % static_cast<unsigned long long>(jobs));
  const PFSPNode& parent = snodes[lp];
  if (k >= parent.limit1 + 1)
    bounds[t] = lb1_child_bound<MM>(lds, parent.prmu, parent.depth, k, jobs);
}

// lb1_d: one thread per parent (reference evaluate.cu:51-70 mapping); bounds
// written per position, no job-indexed local array.
template <int MM>
__global__ void k_pfsp_eval_lb1d(const PFSPNode* parents, int n, int jobs, PfspDevTables tb,
                                 int32_t* bounds) {
  __shared__ LdsLb1<MM> lds;
  __shared__ PFSPNode snodes[BLOCK];
  stage_lb1_tables<MM>(lds, tb, jobs);
  const unsigned long long t =
      static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int lp = stage_parents(parents, static_cast<unsigned long long>(n), 1, snodes, t);
  __syncthreads();
  if (lp < 0) return;
  const PFSPNode& parent = snodes[lp];
  int front[MM], remain[MM];
  lb1d_setup<MM>(lds, parent.prmu, parent.limit1, jobs, front, remain);
  for (int k = parent.limit1 + 1; k < jobs; k++)
    bounds[t * jobs + k] = lb1d_child_bound<MM>(lds, front, remain, parent.prmu[k], jobs);
}

// lb1_d in both directions, one thread per parent: lb_begin / lb_end per
// unscheduled POSITION; the host chooses the direction (hostpool, non-fwd
// branching rules).
template <int MM>
__global__ void k_pfsp_eval_lb1d_bi(const PFSPNode* parents, int n, int jobs,
                                    PfspDevTables tb, int32_t* lb_begin, int32_t* lb_end) {
  __shared__ LdsLb1Bi<MM> lds;
  __shared__ PFSPNode snodes[BLOCK];
  stage_lb1bi_tables<MM>(lds, tb, jobs);
  const unsigned long long t =
      static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int lp = stage_parents(parents, static_cast<unsigned long long>(n), 1, snodes, t);
  __syncthreads();
  if (lp < 0) return;
  const PFSPNode& parent = snodes[lp];
  const int limit1 = parent.limit1, limit2 = jobs - parent.nback;
  int front[MM], back[MM], remain[MM];
  lb1d_bi_setup<MM>(lds, parent.prmu, limit1, limit2, jobs, front, back, remain);
  for (int k = limit1 + 1; k < limit2; k++) {
    const int job = parent.prmu[k];
    lb_begin[t * jobs + k] = lb1d_bound_front<MM>(lds, front, back, remain, job, jobs);
    lb_end[t * jobs + k] = lb1d_bound_back<MM>(lds, front, back, remain, job, jobs);
  }
}

template <int MM>
__global__ void k_pfsp_eval_lb2(const PFSPNode* parents, int n, int jobs, PfspDevTables tb,
                                int best, int32_t* bounds) {
  __shared__ LdsLb2<MM> lds;
  __shared__ PFSPNode snodes[BLOCK / 5 + 2];
  stage_lb2_tables<MM>(lds, tb, jobs);
  const unsigned long long t =
      static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int lp =
      stage_parents(parents, static_cast<unsigned long long>(n) * jobs, jobs, snodes, t);
  __syncthreads();
  if (lp < 0) return;
  const int k = static_cast<int>(t % static_cast<unsigned long long>(jobs));
  const PFSPNode& parent = snodes[lp];
  if (k >= parent.limit1 + 1)
    bounds[t] = lb2_child_bound<MM>(lds, parent.prmu, parent.depth, k, jobs, best);
}


// ---------------------------------------------------------------------------
// Devpool pipeline v3: three kernels per iteration, zero global atomics on
// the hot path.
//
//   K1 expand:  every block derives this iteration's chunk c = popBackBulk
//               semantics (a pure function of ctl->size), reads its parents
//               straight from the pool tail (LDS-staged), evaluates children
//               and writes the survivors COMPACTED into its private childbuf
//               region (block-local exclusive scan for ranks). Per-block
//               child/solution counts out; no control-block writes.
//   K2 scan:    single block: exclusive scan of the G per-block counts into
//               absolute pool offsets; sole writer of size/tree/sol/iters;
//               overflow guard. (Replaces the separate `begin` kernel: the
//               pop is re-derived here identically.)
//   K3 gather:  each block memcpys its children from childbuf into the pool
//               at its scan offset. Runs after K1 read the parents, so
//               overwriting the popped tail is safe.
//
// History: v1 used one atomicAdd per wave on the DevCtl line and saturated
// the L2 atomic unit (~12 ns/op on one line -> ~300 us/iter at chunk 50k,
// 163 Mnodes/s end to end on N=17); v2 (labels + count + scan + emit, 5-6
// kernels) reached 1992 Mnodes/s; v3 cuts the per-iteration kernel count to
// 3 since the hot loop is boundary/launch-bound at M = 50000.
// ---------------------------------------------------------------------------

constexpr int EMIT_TILE = 1024;  // children per block in per-child kernels (4/thread)

// stage parents covering child range [c0, c1) into LDS; returns the first pid.
template <class NodeT, int MAXN>
__device__ inline unsigned int stage_range(const NodeT* parents, unsigned long long c0,
                                           unsigned long long c1, int per,
                                           NodeT (&s)[MAXN]) {
  const unsigned int first = static_cast<unsigned int>(c0 / per);
  const unsigned int last = static_cast<unsigned int>((c1 - 1) / per);
  const int words = static_cast<int>(last - first + 1) * static_cast<int>(sizeof(NodeT) / 4);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(parents + first);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&s[0]);
  for (int i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
  return first;
}

// Exclusive scan of v over the 256-thread block; total broadcast to all lanes.
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t& total) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  __shared__ uint32_t wtot[4];
  __syncthreads();
  if (lane == 63) wtot[wid] = x;
  __syncthreads();
  uint32_t wbase = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (i < wid) wbase += wtot[i];
  total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
  return wbase + x - v;
}

// Block-wide sum of a u64 per-thread value (for subtree-finisher counters,
// which can exceed 32 bits per block).
__device__ inline unsigned long long block_reduce_u64(unsigned long long v) {
  const int wid = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  __shared__ unsigned long long wsum[4];
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wsum[wid] = v;
  __syncthreads();
  return wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

constexpr int NQ_FINISH_MAX = NQ_FLAT_LEVELS_DEV;  // deepest subtree finished in-kernel

// popBackBulk chunk, re-derived identically by every kernel of an iteration
// (pure function of ctl->size, which only K2 of the previous iteration wrote).
__device__ inline unsigned long long derive_chunk(const DevCtl* ctl, unsigned long long m,
                                                  unsigned long long M) {
  if (ctl->overflow) return 0;
  const unsigned long long size = ctl->size;
  if (size < m) return 0;
  return size < M ? size : M;
}

// K1 for N-Queens: evaluate + compact children into the block's childbuf slab.
// Children within `finish` levels of the bottom are counted in-kernel by the
// flat bitmask DFS (nq_finish.hpp) instead of being pushed: the deepest levels
// dominate the tree, so the pool machinery only carries the shallow part.
// A phase-A pass computes each PARENT's (cols, d1, d2) diagonal masks once
// (one thread per staged parent), so a child's safety test and the finisher's
// starting masks are O(1) instead of an O(depth) walk per child.
// Phase B classifies the block's 1024 child slots; the slots that start a
// subtree walk (a safe child with 0 < rem <= finish) become jobs, compacted
// in slot order into an LDS queue (wave ballots + a 16-entry count table: no
// atomics, so the order is the same in every run). Phase C drains the queue
// in ONE loop per lane (nq_flat_run), so a wave's lanes stay busy whatever
// depth or job each of them is in. The kernel is classify, drain, emit; the
// drain is one of three functions (NqDrain, chosen by launch_nq_x), each of
// which returns the lane's counts.
// flat: thread t walks jobs t, t + 256, ...
// split1 / split2: every job is first split one / two levels into sub-jobs
// (nq_finish.hpp), the sub-jobs go into a second LDS queue of NQ_SPLIT_QCAP
// entries (ranked by a block scan, filled and drained in rounds when they do
// not all fit), and a wave that has `refill` idle lanes (or only idle lanes)
// hands all of them the next unclaimed entries from an LDS counter
// (nq_refill_now): which lane walks what varies, the sums do not.
// stack: the wave-stack finisher (nq_finish.hpp). A lane owns a
// row and never backtracks; children with an inner row below them go onto the
// wave's own LDS stack of NQ_STACK_CAP entries, idle lanes take them off it or
// draw whole jobs from jobq through one LDS counter. No split pass, no sub-job
// queue, no block barrier inside the drain. stack_cap (<= NQ_STACK_CAP) is the
// height past which children are walked instead of pushed (a test knob).
enum class NqDrain { flat, split1, split2, stack };

// 16-byte aligned wherever it lands behind a drain's struct: the 16 jobcnt
// words are then read with four 128-bit LDS reads (measured: BASELINE.md
// "Finisher refactor").
struct alignas(16) NqTileLds {
  NQNode s[EMIT_TILE / 4 + 2];        // staged parents; N >= 4 (engine falls back below)
  uint64_t pmask[EMIT_TILE / 4 + 2];  // per-parent cols/d1/d2 (nq_pmask_pack)
  uint16_t jobq[EMIT_TILE];           // finisher jobs: nq_job_ref(local parent id, column)
  uint32_t jobcnt[(EMIT_TILE / BLOCK) * (BLOCK / 64)];  // jobs per (j, wave)
};
struct NqStackLds {
  uint64_t stk[BLOCK / 64][NQ_STACK_CAP];  // one node stack per wave
  uint32_t jhead;                          // next undrawn job
};
struct NqSplitLds {
  uint32_t subq[NQ_SPLIT_QCAP];    // the round's sub-jobs (nq_sub_encode)
  uint16_t joboff[EMIT_TILE + 2];  // the jobs' exclusive sub-job offsets
  uint32_t qhead;                  // next unclaimed entry
};
static_assert(MAX_JOBS <= 32 && (EMIT_TILE / 4 + 2) * 32 <= 65536, "jobq entry is 16-bit");
static_assert(EMIT_TILE * NQ_SPLIT_FANOUT_MAX < 65536, "sub-job offsets are 16-bit");
// A block's LDS. The drain's arrays come first: the stack / queue that its
// inner loop indexes sits at LDS address 0 and needs no base register.
template <NqDrain D>
struct NqLds {
  NqSplitLds drain;
  NqTileLds tile;
};
template <>
struct NqLds<NqDrain::stack> {
  NqStackLds drain;
  NqTileLds tile;
};
template <>
struct NqLds<NqDrain::flat> {
  NqTileLds tile;
};
// With block_excl_scan's and block_reduce_u64's scratch and the padding
// between the three, a block's LDS must leave eight blocks per CU.
template <NqDrain D>
constexpr size_t nq_x_lds_bytes =
    sizeof(NqLds<D>) + 4 * sizeof(uint32_t) + 4 * sizeof(unsigned long long) + 16;

// What a lane's drain counted. nodes: the candidates of the rows the split
// pass enumerated (the split drain alone).
// 32-bit per-lane counters: a block's whole queue is at most 1024 jobs of
// <= 109,600 nodes each, below 2^32, whichever lane walks what
struct NqDrained {
  uint32_t tree = 0, sol = 0;
  unsigned long long nodes = 0;
};

// job ref -> the child's masks, seen from the row below it (as phase A
// steps them); returns that row. One LDS read: the parent's packed masks.
__device__ inline int nq_tile_job(const NqTileLds& t, uint32_t e, uint32_t msk, uint32_t& jc,
                                  uint32_t& jd1, uint32_t& jd2) {
  return nq_job_state(t.pmask[nq_job_parent(e)], e, msk, jc, jd1, jd2);
}

// Phase A: one thread per staged parent computes its packed masks.
__device__ inline void nq_tile_masks(NqTileLds& t, int nblk, int N, uint32_t msk) {
  for (int pi = threadIdx.x; pi < nblk; pi += blockDim.x) {
    const NQNode& p = t.s[pi];
    uint32_t cols = 0, d1 = 0, d2 = 0;
    const int depth = p.depth;
    for (int i = 0; i < depth && i < N; i++) {
      const uint32_t b = 1u << p.board[i];
      cols |= b;
      d1 = ((d1 | b) << 1) & msk;
      d2 = (d2 | b) >> 1;
    }
    t.pmask[pi] = nq_pmask_pack(cols, d1, d2);
  }
}

// Job queue: the slots labelled 2 go into t.jobq in slot order; slot
// j * 256 + threadIdx.x ranks as (j, wave, lane). Returns the number of jobs.
// Two block barriers; the queue is complete after the second.
__device__ inline uint32_t nq_tile_rank_jobs(NqTileLds& t, const uint8_t (&lab)[EMIT_TILE / BLOCK],
                                             const uint16_t (&lpid)[EMIT_TILE / BLOCK],
                                             const uint8_t (&lcol)[EMIT_TILE / BLOCK]) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  uint32_t rank[EMIT_TILE / BLOCK];
#pragma unroll
  for (int j = 0; j < EMIT_TILE / BLOCK; j++) {
    const unsigned long long bal = __ballot(lab[j] == 2);
    rank[j] = static_cast<uint32_t>(__popcll(bal & ((1ull << lane) - 1ull)));
    if (lane == 0) t.jobcnt[j * (BLOCK / 64) + wid] = static_cast<uint32_t>(__popcll(bal));
  }
  __syncthreads();
  uint32_t njobs = 0;
#pragma unroll
  for (int i = 0; i < (EMIT_TILE / BLOCK) * (BLOCK / 64); i++) {
    if (i % (BLOCK / 64) == wid) rank[i / (BLOCK / 64)] += njobs;
    njobs += t.jobcnt[i];
  }
#pragma unroll
  for (int j = 0; j < EMIT_TILE / BLOCK; j++)
    if (lab[j] == 2) t.jobq[rank[j]] = static_cast<uint16_t>(nq_job_ref(lpid[j], lcol[j]));
  __syncthreads();
  return njobs;
}

// Flat drain: one flat loop per lane over its strided share of the queue.
template <bool G1>
__device__ inline NqDrained nq_drain_flat(const NqTileLds& t, uint32_t njobs, uint32_t msk, int N,
                                          int g) {
  NqFlat<NQ_FLAT_LEVELS_DEV> st;
  st.tree = 0;
  st.sol = 0;
  uint32_t q = threadIdx.x;
  nq_flat_run<NQ_FLAT_LEVELS_DEV, G1>(
      st,
      [&](NqFlat<NQ_FLAT_LEVELS_DEV>& w) {
        if (q >= njobs) return false;
        const uint32_t e = t.jobq[q];
        q += BLOCK;
        uint32_t jc, jd1, jd2;
        const int row = nq_tile_job(t, e, msk, jc, jd1, jd2);
        w.template load<G1>(jc, jd1, jd2, row, N, msk, g);
        return true;
      },
      msk, g);
  return {st.tree, st.sol, 0};
}

// Stack drain. One block barrier (after the job counter's reset).
template <bool G1>
__device__ inline NqDrained nq_drain_stack(const NqTileLds& t, NqStackLds& d, uint32_t njobs,
                                           uint32_t msk, int N, int g, int refill,
                                           int stack_cap) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  if (threadIdx.x == 0) d.jhead = 0;
  __syncthreads();
  uint64_t* const my = d.stk[wid];  // this wave's stack; no other wave touches it
  const unsigned long long lt = (1ull << lane) - 1ull;
  const uint32_t T = static_cast<uint32_t>(refill);
  const uint32_t cap = static_cast<uint32_t>(stack_cap);  // <= NQ_STACK_CAP (launch_nq_x)
  NqRow r = {0, 0, 0, 0, 0, 0, 0};
  uint32_t sp = 0;   // wave-uniform: ballots and the broadcast counter alone move it
  bool more = true;  // wave-uniform
  unsigned long long im = ~0ull;  // every lane starts idle, so the wave starts by acting
  uint32_t nidle = 64u;
  // Why it ends: see nq_stack_act (nq_finish.hpp). The iterations that only
  // step and push are an inner loop of their own; the fetch is behind the
  // scalar branch nq_stack_act.
  for (;;) {
    if (nq_stack_done(nidle, 64u, sp, more)) break;
    const bool idle = r.cand == 0;
    const uint32_t rank = static_cast<uint32_t>(__popcll(im & lt));
    const uint32_t take = nq_stack_take(nidle, sp);
    // rank < take <= sp: my[sp - 1 - rank] is inside [0, sp)
    if (idle && rank < take) nq_row_load_entry(r, my[sp - 1u - rank], msk);
    sp -= take;
    if (more && nidle > take) {
      const uint32_t rem = nq_stack_draw(nidle - take, njobs, BLOCK / 64);
      uint32_t got = 0;
      if (lane == 0) got = atomicAdd(&d.jhead, rem);
      got = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(got)));
      more = !nq_refill_drains(got, rem, njobs);
      const uint32_t qi = got + rank - take;
      // qi < njobs <= EMIT_TILE: inside jobq
      if (idle && rank >= take && rank - take < rem && qi < njobs) {
        uint32_t jc, jd1, jd2;
        const int row = nq_tile_job(t, t.jobq[qi], msk, jc, jd1, jd2);
        nq_row_load_job<G1>(r, jc, jd1, jd2, row, N, msk, g);
      }
    }
    do {
      uint32_t nc, n1, n2;
      const bool push = nq_row_step<G1>(r, msk, g, nc, n1, n2);  // idle lanes pass through
      if (nq_stack_can_push(sp, 64u, cap)) {  // scalar: sp + 64 <= cap <= NQ_STACK_CAP
        const unsigned long long pm = __builtin_amdgcn_ballot_w64(push);
        if (push)
          my[sp + static_cast<uint32_t>(__popcll(pm & lt))] = nq_entry_pack(nc, n1, n2, r.h - 1u);
        sp += static_cast<uint32_t>(__popcll(pm));
      } else if (push) {
        nq_row_walk<G1>(r, nc, n1, n2, N, msk, g);
      }
      im = __builtin_amdgcn_ballot_w64(r.cand == 0);
      nidle = static_cast<uint32_t>(__popcll(im));
    } while (!nq_stack_act(nidle, 64u, T, sp, more));
  }
  return {r.tree, r.sol, 0};
}

// Split drain, S levels. Its barriers (the count pass's scans, one after the
// offsets, two per round) are all at block-uniform places.
template <bool G1, int S>
__device__ inline NqDrained nq_drain_split(const NqTileLds& t, NqSplitLds& d, uint32_t njobs,
                                           uint32_t msk, int N, int g, int refill) {
  const int lane = threadIdx.x & 63;
  NqDrained out;
  // count pass: thread t counts the sub-jobs of jobs t, t + 256, ...
  // (and the nodes of the rows it enumerates); a block scan per row of 256
  // jobs turns the counts into queue offsets, in job order.
  uint32_t run = 0;
  for (uint32_t q0 = 0; q0 < njobs; q0 += BLOCK) {  // block-uniform trip count
    const uint32_t q = q0 + threadIdx.x;
    uint32_t n = 0;
    if (q < njobs) {
      uint32_t jc, jd1, jd2, nodes = 0;
      const int row = nq_tile_job(t, t.jobq[q], msk, jc, jd1, jd2);
      n = nq_split_job<G1, false>(jc, jd1, jd2, nq_split_levels(S, N - row), msk, g, nodes,
                                  [](uint32_t, uint32_t, uint32_t) {});
      out.nodes += nodes;
    }
    uint32_t tot;
    const uint32_t pre = block_excl_scan(n, tot);
    if (q < njobs) d.joboff[q] = static_cast<uint16_t>(run + pre);
    run += tot;
  }
  if (threadIdx.x == 0) d.joboff[njobs] = static_cast<uint16_t>(run);
  __syncthreads();
  // rounds: the longest run of jobs whose sub-jobs fit the queue
  // is written out and drained. A wave refills all of its idle lanes at
  // once when `refill` of them are idle (nq_refill_now: one LDS add per
  // refill, two LDS reads per lane); otherwise a scalar branch skips the
  // fetch.
  NqFlat<NQ_FLAT_LEVELS_DEV> st;
  st.tree = 0;
  st.sol = 0;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const uint32_t T = static_cast<uint32_t>(refill);
  for (uint32_t jb = 0; jb < njobs;) {  // block-uniform: je comes from LDS alone
    const uint32_t je = nq_round_end(d.joboff, jb, njobs, NQ_SPLIT_QCAP);
    const uint32_t base = d.joboff[jb];
    const uint32_t nsub = d.joboff[je] - base;
    for (uint32_t q = jb + threadIdx.x; q < je; q += BLOCK) {
      const uint32_t e = t.jobq[q];
      uint32_t jc, jd1, jd2, nodes = 0;
      const int row = nq_tile_job(t, e, msk, jc, jd1, jd2);
      uint32_t w = d.joboff[q] - base;
      nq_split_job<true, true>(jc, jd1, jd2, nq_split_levels(S, N - row), msk, 1, nodes,
                               [&](uint32_t nc, uint32_t c1, uint32_t c2) {
                                 d.subq[w++] = nq_sub_encode(e, nc, c1, c2);
                               });
    }
    if (threadIdx.x == 0) d.qhead = 0;
    __syncthreads();
    // Every lane of the wave stays in the loop until the wave leaves it
    // (the ballots need them all): `drained`, the refill decision and the
    // exit are wave-uniform. Why it ends: see nq_refill_now (nq_finish.hpp).
    // The iterations that only step are an inner loop of their own: one
    // ballot, one scalar compare against nq_refill_level, no fetch code.
    bool drained = false;
    st.cand = 0;
    st.stack = 0;
    bool idle = true;                  // every lane starts without a walk,
    unsigned long long im = ~0ull;     // so the all-idle rule starts the wave
    uint32_t nidle = 64u;
    for (;;) {
      if (nq_wave_done(nidle, 64u, drained)) break;
      // here nq_refill_now(nidle, 64, T, drained) holds
      uint32_t got = 0;
      if (lane == 0) got = atomicAdd(&d.qhead, nidle);
      got = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(got)));
      drained = nq_refill_drains(got, nidle, nsub);
      const uint32_t qi = got + static_cast<uint32_t>(__popcll(im & lt));
      if (idle && qi < nsub) {  // qi < nsub <= NQ_SPLIT_QCAP: inside subq
        const uint32_t e = d.subq[qi];
        uint32_t jc, jd1, jd2;
        const int row = nq_tile_job(t, nq_sub_ref(e), msk, jc, jd1, jd2);
        nq_sub_load<G1>(st, e, jc, jd1, jd2, row, N, msk, g);
      }
      const uint32_t level = nq_refill_level(64u, T, drained);
      do {
        if (st.cand == 0 && st.stack > 1) st.pop(msk);
        if (st.cand) st.template take<G1>(msk, g);
        idle = nq_lane_idle(st.cand, st.stack);
        im = __builtin_amdgcn_ballot_w64(idle);
        nidle = static_cast<uint32_t>(__popcll(im));
      } while (nidle < level);
    }
    __syncthreads();  // the next round rewrites subq and qhead
    jb = je;
  }
  out.tree = st.tree;
  out.sol = st.sol;
  return out;
}

template <bool G1, NqDrain D>
__global__ void k_nq_x(const DevCtl* ctl, const NQNode* pool, NQNode* childbuf,
                       uint32_t* blockCounts, unsigned long long* blockSols,
                       unsigned long long* blockExtra, int N, int g, int finish, int refill,
                       int stack_cap, unsigned long long m, unsigned long long M) {
  __shared__ NqLds<D> lds;
  static_assert(nq_x_lds_bytes<D> <= 20480, "k_nq_x's LDS must leave eight blocks per CU");
  NqTileLds& tile = lds.tile;
  const unsigned long long c = derive_chunk(ctl, m, M);
  // child indices fit u32: the engine enforces M * branching <= 2^31
  const uint32_t total = static_cast<uint32_t>(c * N);
  const NQNode* parents = pool + (ctl->size - c);
  const uint32_t c0 = static_cast<uint32_t>(blockIdx.x) * EMIT_TILE;
  uint32_t cnt = 0;
  unsigned long long sols = 0, extra = 0;
  unsigned int first = 0;
  uint8_t lab[EMIT_TILE / BLOCK] = {0, 0, 0, 0};  // 1 = pushed child, 2 = finisher job
  uint16_t lpid[EMIT_TILE / BLOCK];
  uint8_t lk[EMIT_TILE / BLOCK];
  uint8_t lcol[EMIT_TILE / BLOCK] = {0, 0, 0, 0};  // the slot's column (job slots)
  if (c0 < total) {
    const uint32_t msk = (1u << N) - 1u;
    uint32_t c1 = c0 + EMIT_TILE;
    if (c1 > total) c1 = total;
    first = stage_range(parents, c0, c1, N, tile.s);
    __syncthreads();
    nq_tile_masks(tile, static_cast<int>((c1 - 1) / N - first + 1), N, msk);  // phase A
    __syncthreads();
#pragma unroll
    for (int j = 0; j < EMIT_TILE / BLOCK; j++) {  // phase B: classify the child slots
      const uint32_t t = c0 + j * BLOCK + threadIdx.x;
      if (t < total) {
        const uint32_t pid = t / static_cast<uint32_t>(N);
        const int k = static_cast<int>(t - pid * N);
        lpid[j] = static_cast<uint16_t>(pid - first);
        lk[j] = static_cast<uint8_t>(k);
        const NQNode& p = tile.s[pid - first];
        const int depth = p.depth;
        if (depth == N) {
          sols += (k == 0);  // leaf parent counted once (nqueens_chpl.chpl:78-80)
        } else if (k >= depth) {
          uint32_t pc, pd1, pd2;
          nq_pmask_unpack(tile.pmask[pid - first], pc, pd1, pd2);
          const uint32_t occ = pc | pd1 | pd2;
          lcol[j] = p.board[k];
          const uint32_t b = 1u << lcol[j];
          const uint32_t freemask = G1 ? (~occ & msk) : nq_free_occ_g(occ, msk, g);
          if (b & freemask) {  // == nq_safe (diagonal masks)
            const int rem = N - (depth + 1);  // levels below the child
            if (rem <= finish) {
              // child + its whole subtree counted here, nothing pushed
              extra += 1;
              if (rem == 0)
                sols += 1;
              else
                lab[j] = 2;
            } else {
              lab[j] = 1;
            }
          }
        }
        cnt += (lab[j] == 1);
      }
    }
    const uint32_t njobs = nq_tile_rank_jobs(tile, lab, lpid, lcol);
    NqDrained d;  // phase C
    if constexpr (D == NqDrain::flat) {
      d = nq_drain_flat<G1>(tile, njobs, msk, N, g);
    } else if constexpr (D == NqDrain::stack) {
      d = nq_drain_stack<G1>(tile, lds.drain, njobs, msk, N, g, refill, stack_cap);
    } else {
      constexpr int S = D == NqDrain::split1 ? 1 : 2;
      d = nq_drain_split<G1, S>(tile, lds.drain, njobs, msk, N, g, refill);
    }
    extra += d.nodes;
    extra += d.tree;
    sols += d.sol;
  }
  uint32_t totC;
  const uint32_t pre = block_excl_scan(cnt, totC);
  const unsigned long long totS = block_reduce_u64(sols);
  const unsigned long long totE = block_reduce_u64(extra);
  if (threadIdx.x == 0) {
    blockCounts[blockIdx.x] = totC;
    blockSols[blockIdx.x] = totS;
    blockExtra[blockIdx.x] = totE;
  }
  if (cnt > 0) {
    unsigned long long slot = static_cast<unsigned long long>(blockIdx.x) * EMIT_TILE + pre;
#pragma unroll
    for (int j = 0; j < EMIT_TILE / BLOCK; j++) {
      if (lab[j] == 1) {
        const NQNode& p = tile.s[lpid[j]];
        emit_nq_child(childbuf, slot++, p, p.depth, lk[j]);
      }
    }
  }
}


// K1 for PFSP lb1 / lb2 (one child per thread-slot).
template <int MM, int LB>
__global__ void k_pfsp_x(DevCtl* ctl, const PFSPNode* pool, PFSPNode* childbuf,
                         uint32_t* blockCounts, unsigned long long* blockSols, int jobs,
                         PfspDevTables tb, unsigned long long m, unsigned long long M) {
  using LDS = typename std::conditional<LB == 2, LdsLb2<MM>, LdsLb1<MM>>::type;
  __shared__ LDS lds;
  __shared__ PFSPNode s[EMIT_TILE / 5 + 2];  // jobs >= 5
  if constexpr (LB == 2)
    stage_lb2_tables<MM>(lds, tb, jobs);
  else
    stage_lb1_tables<MM>(lds, tb, jobs);
  const unsigned long long c = derive_chunk(ctl, m, M);
  const uint32_t total = static_cast<uint32_t>(c * jobs);
  const PFSPNode* parents = pool + (ctl->size - c);
  const uint32_t c0 = static_cast<uint32_t>(blockIdx.x) * EMIT_TILE;
  const int best = ctl->best;
  uint32_t cnt = 0;
  unsigned long long sols = 0;
  unsigned int first = 0;
  uint8_t lab[EMIT_TILE / BLOCK] = {0, 0, 0, 0};
  uint16_t lpid[EMIT_TILE / BLOCK];
  uint8_t lk[EMIT_TILE / BLOCK];
  if (c0 < total) {
    uint32_t c1 = c0 + EMIT_TILE;
    if (c1 > total) c1 = total;
    first = stage_range(parents, c0, c1, jobs, s);
  }
  __syncthreads();
  if (c0 < total) {
    for (int j = 0; j < EMIT_TILE / BLOCK; j++) {
      const uint32_t t = c0 + j * BLOCK + threadIdx.x;
      if (t < total) {
        const uint32_t pid = t / static_cast<uint32_t>(jobs);
        const int k = static_cast<int>(t - pid * jobs);
        lpid[j] = static_cast<uint16_t>(pid - first);
        lk[j] = static_cast<uint8_t>(k);
        const PFSPNode& p = s[pid - first];
        const int depth = p.depth;
        if (k >= p.limit1 + 1) {
          int lb;
          if constexpr (LB == 2) {
            lb = lb2_child_bound<MM>(lds, p.prmu, depth, k, jobs, best);
          } else {
            lb = lb1_child_bound<MM>(lds, p.prmu, depth, k, jobs);
          }
          if (depth + 1 == jobs) {
            lab[j] = 2;
            if (lb < best) atomicMin(&ctl->best, lb);
          } else if (lb < best) {
            lab[j] = 1;
          }
        }
        cnt += (lab[j] == 1);
        sols += (lab[j] == 2);
      }
    }
  }
  uint32_t totC;
  const uint32_t pre = block_excl_scan(cnt, totC);
  const unsigned long long totS = block_reduce_u64(sols);
  if (threadIdx.x == 0) {
    blockCounts[blockIdx.x] = totC;
    blockSols[blockIdx.x] = totS;
  }
  if (cnt > 0) {
    unsigned long long slot = static_cast<unsigned long long>(blockIdx.x) * EMIT_TILE + pre;
#pragma unroll
    for (int j = 0; j < EMIT_TILE / BLOCK; j++) {
      if (lab[j] == 1) {
        const PFSPNode& p = s[lpid[j]];
        emit_pfsp_child(childbuf, slot++, p, p.depth, p.limit1, lk[j]);
      }
    }
  }
}

// K1 for PFSP lb1_d: one thread per parent (O(mn) setup amortized over all
// children); bounds are O(m) so the write pass just recomputes them instead
// of storing a job-indexed local array (which would spill to scratch).
template <int MM>
__global__ void k_pfsp_x_lb1d(DevCtl* ctl, const PFSPNode* pool, PFSPNode* childbuf,
                              uint32_t* blockCounts, unsigned long long* blockSols, int jobs,
                              PfspDevTables tb, unsigned long long m,
                              unsigned long long M) {
  __shared__ LdsLb1<MM> lds;
  __shared__ PFSPNode s[BLOCK];
  stage_lb1_tables<MM>(lds, tb, jobs);
  const unsigned long long c = derive_chunk(ctl, m, M);
  const PFSPNode* parents = pool + (ctl->size - c);
  const unsigned long long t =
      static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int lp = stage_parents(parents, c, 1, s, t);
  __syncthreads();
  const int best = ctl->best;

  int front[MM], remain[MM];
  uint32_t cnt = 0;
  unsigned long long sols = 0;
  int depth = 0, limit1 = 0;
  if (lp >= 0) {
    const PFSPNode& p = s[lp];
    depth = p.depth;
    limit1 = p.limit1;
    lb1d_setup<MM>(lds, p.prmu, limit1, jobs, front, remain);
    for (int k = limit1 + 1; k < jobs; k++) {
      const int lb = lb1d_child_bound<MM>(lds, front, remain, s[lp].prmu[k], jobs);
      if (depth + 1 == jobs) {
        sols++;
        if (lb < best) atomicMin(&ctl->best, lb);
      } else if (lb < best) {
        cnt++;
      }
    }
  }
  uint32_t totC;
  const uint32_t pre = block_excl_scan(cnt, totC);
  const unsigned long long totS = block_reduce_u64(sols);
  if (threadIdx.x == 0) {
    blockCounts[blockIdx.x] = totC;
    blockSols[blockIdx.x] = totS;
  }
  if (cnt > 0) {
    unsigned long long slot =
        static_cast<unsigned long long>(blockIdx.x) * (BLOCK * MAX_JOBS) + pre;
    for (int k = limit1 + 1; k < jobs; k++) {
      const int lb = lb1d_child_bound<MM>(lds, front, remain, s[lp].prmu[k], jobs);
      if (depth + 1 != jobs && lb < best)
        emit_pfsp_child(childbuf, slot++, s[lp], depth, limit1, k);
    }
  }
}

// K1 for PFSP lb1_d under a non-forward branching rule (br: 1 bwd, 2 alt,
// 3 minbranch): same contract and geometry as k_pfsp_x_lb1d — one thread per
// parent, survivors compacted into the block's BLOCK*MAX_JOBS slab, per-block
// counts out, atomicMin on ctl->best at leaves only. Each thread builds the
// parent's front / back / remain once, pass 1 evaluates the O(m) child bounds
// (both directions for minbranch, only the rule's direction otherwise) and
// accumulates the survivor counts and bound sums, the direction is decided,
// and pass 2 recomputes the chosen direction's bounds and emits (recompute,
// not store: a job-indexed local array would spill to scratch).
template <int MM>
__global__ void k_pfsp_x_lb1d_bi(DevCtl* ctl, const PFSPNode* pool, PFSPNode* childbuf,
                                 uint32_t* blockCounts, unsigned long long* blockSols,
                                 int jobs, PfspDevTables tb, unsigned long long m,
                                 unsigned long long M, int br) {
  __shared__ LdsLb1Bi<MM> lds;
  __shared__ PFSPNode s[BLOCK];
  stage_lb1bi_tables<MM>(lds, tb, jobs);
  const unsigned long long c = derive_chunk(ctl, m, M);
  const PFSPNode* parents = pool + (ctl->size - c);
  const unsigned long long t =
      static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int lp = stage_parents(parents, c, 1, s, t);
  __syncthreads();
  const int best = ctl->best;

  int front[MM], back[MM], remain[MM];
  uint32_t cnt = 0;
  unsigned long long sols = 0;
  int depth = 0, limit1 = 0, limit2 = 0;
  bool bwd = false;
  if (lp >= 0) {
    const PFSPNode& p = s[lp];
    depth = p.depth;
    limit1 = p.limit1;
    limit2 = jobs - p.nback;
    lb1d_bi_setup<MM>(lds, p.prmu, limit1, limit2, jobs, front, back, remain);
    const bool dyn = br == 3;
    bwd = br == 1 || (br == 2 && (depth & 1));
    int cntF = 0, cntB = 0, sumF = 0, sumB = 0;
    int minF = 0x7fffffff, minB = 0x7fffffff;
    for (int k = limit1 + 1; k < limit2; k++) {
      const int job = s[lp].prmu[k];
      if (dyn || !bwd) {
        const int lb = lb1d_bound_front<MM>(lds, front, back, remain, job, jobs);
        cntF += lb < best;
        sumF += lb;
        minF = min(minF, lb);
      }
      if (dyn || bwd) {
        const int lb = lb1d_bound_back<MM>(lds, front, back, remain, job, jobs);
        cntB += lb < best;
        sumB += lb;
        minB = min(minB, lb);
      }
    }
    if (dyn) bwd = cntB < cntF || (cntB == cntF && sumB > sumF);
    if (depth + 1 == jobs) {
      sols = static_cast<unsigned long long>(limit2 - (limit1 + 1));
      const int lb = bwd ? minB : minF;
      if (limit2 > limit1 + 1 && lb < best) atomicMin(&ctl->best, lb);
    } else {
      cnt = static_cast<uint32_t>(bwd ? cntB : cntF);
    }
  }
  uint32_t totC;
  const uint32_t pre = block_excl_scan(cnt, totC);
  const unsigned long long totS = block_reduce_u64(sols);
  if (threadIdx.x == 0) {
    blockCounts[blockIdx.x] = totC;
    blockSols[blockIdx.x] = totS;
  }
  if (cnt > 0) {
    unsigned long long slot =
        static_cast<unsigned long long>(blockIdx.x) * (BLOCK * MAX_JOBS) + pre;
    const int nback = jobs - limit2;
    for (int k = limit1 + 1; k < limit2; k++) {
      const int job = s[lp].prmu[k];
      if (bwd) {
        if (lb1d_bound_back<MM>(lds, front, back, remain, job, jobs) < best)
          emit_pfsp_child_back(childbuf, slot++, s[lp], depth, nback, jobs, k);
      } else {
        if (lb1d_bound_front<MM>(lds, front, back, remain, job, jobs) < best)
          emit_pfsp_child_front(childbuf, slot++, s[lp], depth, limit1, k);
      }
    }
  }
}



// Wave-cooperative lb2 expand: phase A builds each child's front schedule and
// scheduled-mask into LDS (one thread per child, fully parallel); phase B
// assigns each 64-lane wave ONE child at a time — lanes evaluate machine
// pairs in parallel and a shfl max-reduce after each 64-pair round makes the
// early exit COLLECTIVE. The per-lane kernel's exit was wave-granular (a wave
// ran all 190 pairs whenever any lane's child was pushed, i.e. essentially
// always); here the serial chain per child shrinks from 190x20 to ceil(190/64)
// rounds of 20 steps, and pruned children really do stop early.
// Decision parity: an exit implies partial-max > best => prune (identical to
// the full max's decision); a completed reduce IS the exact full max, so leaf
// best-updates only use exact values (reference semantics,
// c_bound_johnson.c:211-254).
template <int MM>
struct LdsLb2w {
  static constexpr int PAIRS = MM * (MM - 1) / 2;
  // only the ROUND-0 pair rows live in LDS: with the collective early exit
  // and strength-ordered pairs most children never touch rounds 1-2, so
  // those rows read from global (L2-resident, the table is ~15 KB) — the
  // 10 KB of LDS saved lifts occupancy from 5 to 7 blocks/CU at MM=20
  static constexpr int JP_LDS = PAIRS < 64 ? PAIRS : 64;
  int16_t p[MM * MAX_JOBS];
  int32_t min_tails[MM];
  uint32_t jp[JP_LDS * MAX_JOBS];
  uint8_t pair1[PAIRS], pair2[PAIRS];
  uint16_t fronts[BLOCK][MM + 1];  // child completion times (values <= 20*20*99)
  uint8_t lpar[BLOCK];             // child's parent index in snodes
  int8_t ck[BLOCK];                // child's k, or -1 invalid, <=-2 leaf (-2-k)
  PFSPNode snodes[BLOCK / 5 + 2];
  // per-PARENT prefix state (phase A0): every child of a parent shares the
  // parent's front schedule and scheduled mask, so they are computed once
  // per parent and each child's phase A is a single O(m) forward step.
  // (The per-child scheduled mask is pmask[parent] | bit(job_k), derived in
  // phase B — keeping a per-child copy would cost 1 KB of LDS and a
  // block/CU of occupancy.)
  uint16_t pfront[BLOCK / 5 + 2][MM + 1];
  uint32_t pmask[BLOCK / 5 + 2];
};

__device__ inline int wave_max_i32(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}

// One child's Johnson sweep spread over a wave: lane l bounds the
// strength-ordered pairs l, l + 64, ... and after each 64-pair round a shfl
// max-reduce decides the collective early exit. `fr` / `bk` are the child's
// front / back schedules (LDS rows, runtime-indexed by the pair's machines;
// bk is the min_tails row under forward branching), `sched` its scheduled-job
// mask. LDS supplies jp (round-0 pair rows), pair1 / pair2 and JP_LDS. Returns
// the wave-wide max: the exact bound when `exited` stays false, otherwise some
// partial max > best.
template <int MM, class LDS, class BackT>
__device__ inline int wave_lb2_sweep(const LDS& lds, const PfspDevTables& tb,
                                     const uint16_t* fr, const BackT* bk, uint32_t sched,
                                     int jobs, int best, int lane, bool& exited) {
  constexpr int PAIRS = MM * (MM - 1) / 2;
  constexpr int ROUNDS = (PAIRS + 63) / 64;
  int mylb = 0;
#pragma unroll
  for (int r = 0; r < ROUNDS; r++) {
    if (!exited) {
      const int pr = lane + r * 64;
      if (pr < PAIRS) {
        const int ma0 = lds.pair1[pr];
        const int ma1 = lds.pair2[pr];
        int t0 = fr[ma0];
        int t1 = fr[ma1];
        const uint32_t* jp =
            (pr < LDS::JP_LDS) ? &lds.jp[pr * jobs] : &tb.johnson_packed_w[pr * jobs];
        // jobs == MAX_JOBS for every GPU-supported Taillard instance:
        // full unrolling lets the compiler batch the 20 dependent
        // ds_read_b32s instead of serializing load->use 20 times
        if (jobs == MAX_JOBS) {
#pragma unroll
          for (int j = 0; j < MAX_JOBS; j++) {
            const uint32_t v = jp[j];
            const int job = static_cast<int>(v >> 27);
            if (!(sched >> job & 1u)) {
              t0 += static_cast<int>(v & 0xffu);
              t1 = max(t1, t0 + static_cast<int>((v >> 16) & 0x7ffu));
              t1 += static_cast<int>((v >> 8) & 0xffu);
            }
          }
        } else {
          for (int j = 0; j < jobs; j++) {
            const uint32_t v = jp[j];
            const int job = static_cast<int>(v >> 27);
            if (!(sched >> job & 1u)) {
              t0 += static_cast<int>(v & 0xffu);
              t1 = max(t1, t0 + static_cast<int>((v >> 16) & 0x7ffu));
              t1 += static_cast<int>((v >> 8) & 0xffu);
            }
          }
        }
        mylb = max(mylb, max(t1 + static_cast<int>(bk[ma1]), t0 + static_cast<int>(bk[ma0])));
      }
      if (wave_max_i32(mylb) > best) exited = true;  // collective early exit
    }
  }
  return wave_max_i32(mylb);
}

template <int MM>
__global__ void k_pfsp_x_lb2w(DevCtl* ctl, const PFSPNode* pool, PFSPNode* childbuf,
                              uint32_t* waveCounts, unsigned long long* waveSols, int jobs,
                              PfspDevTables tb, unsigned long long m,
                              unsigned long long M) {
  __shared__ LdsLb2w<MM> lds;
  constexpr int PAIRS = LdsLb2w<MM>::PAIRS;
  for (int i = threadIdx.x; i < MM * jobs; i += blockDim.x) lds.p[i] = tb.p_times[i];
  if (threadIdx.x < MM) lds.min_tails[threadIdx.x] = tb.min_tails[threadIdx.x];
  // strength-ordered tables: strongest pairs land in the first 64-pair round
  // so the collective early exit fires there (see PfspDevTables)
  for (int i = threadIdx.x; i < LdsLb2w<MM>::JP_LDS * jobs; i += blockDim.x)
    lds.jp[i] = tb.johnson_packed_w[i];
  if (threadIdx.x < PAIRS) {
    lds.pair1[threadIdx.x] = tb.pairs1_w[threadIdx.x];
    lds.pair2[threadIdx.x] = tb.pairs2_w[threadIdx.x];
  }

  const unsigned long long c = derive_chunk(ctl, m, M);
  const uint32_t total = static_cast<uint32_t>(c * jobs);
  const PFSPNode* parents = pool + (ctl->size - c);
  const uint32_t c0 = static_cast<uint32_t>(blockIdx.x) * BLOCK;
  unsigned int first = 0;
  if (c0 < total) {
    uint32_t c1 = c0 + BLOCK;
    if (c1 > total) c1 = total;
    first = stage_range(parents, c0, c1, jobs, lds.snodes);
  }
  __syncthreads();

  // ---- phase A0: one thread per PARENT (prefix front + scheduled mask) ----
  if (c0 < total) {
    uint32_t c1 = c0 + BLOCK;
    if (c1 > total) c1 = total;
    const int nblk = static_cast<int>((c1 - 1) / jobs - first + 1);
    for (int pi = threadIdx.x; pi < nblk; pi += blockDim.x) {
      const PFSPNode& p = lds.snodes[pi];
      int front[MM];
#pragma unroll
      for (int i = 0; i < MM; i++) front[i] = 0;
      uint32_t sched = 0;
      for (int i = 0; i < p.depth; i++) {
        const int job = p.prmu[i];
        sched |= 1u << job;
        front[0] += lds.p[job];
#pragma unroll
        for (int j = 1; j < MM; j++)
          front[j] = max(front[j - 1], front[j]) + lds.p[j * jobs + job];
      }
#pragma unroll
      for (int i = 0; i < MM; i++)
        lds.pfront[pi][i] = static_cast<uint16_t>(front[i]);
      lds.pmask[pi] = sched;
    }
  }
  __syncthreads();

  // ---- phase A: one thread per child slot — a single O(m) step from the
  // parent's front ----
  {
    const uint32_t t = c0 + threadIdx.x;
    int8_t state = -1;
    if (c0 < total && t < total) {
      const uint32_t pid = t / static_cast<uint32_t>(jobs);
      const int k = static_cast<int>(t - pid * jobs);
      const PFSPNode& p = lds.snodes[pid - first];
      lds.lpar[threadIdx.x] = static_cast<uint8_t>(pid - first);
      if (k >= p.limit1 + 1) {
        const int job_k = p.prmu[k];
        const uint16_t* pf = lds.pfront[pid - first];
        int prev = pf[0] + lds.p[job_k];
        lds.fronts[threadIdx.x][0] = static_cast<uint16_t>(prev);
#pragma unroll
        for (int j = 1; j < MM; j++) {
          prev = max(prev, static_cast<int>(pf[j])) + lds.p[j * jobs + job_k];
          lds.fronts[threadIdx.x][j] = static_cast<uint16_t>(prev);
        }
        state = (p.depth + 1 == jobs) ? static_cast<int8_t>(-2 - k)
                                      : static_cast<int8_t>(k);
      }
    }
    lds.ck[threadIdx.x] = state;
  }
  // phase B consumes only THIS wave's phase-A slots (ct = wid*64 + cc, all
  // written by lanes of the same wave), so no block barrier is needed — just
  // order this wave's own LDS traffic
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();

  // ---- phase B: one child per wave at a time, pairs across lanes ----
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int best = ctl->best;
  uint32_t mycnt = 0;
  unsigned long long mysols = 0;
  const unsigned long long wave_slab =
      (static_cast<unsigned long long>(blockIdx.x) * 4 + wid) * 64ull;

  for (int cc = 0; cc < 64; cc++) {
    const int ct = wid * 64 + cc;
    const int8_t state = lds.ck[ct];  // same address across the wave: broadcast
    if (state == -1) continue;
    const bool leaf = state <= -2;
    const int k = leaf ? (-2 - state) : state;
    const uint16_t* fr = lds.fronts[ct];
    const int lp = lds.lpar[ct];
    const uint32_t sched = lds.pmask[lp] | (1u << lds.snodes[lp].prmu[k]);

    bool exited = false;
    const int lb = wave_lb2_sweep<MM>(lds, tb, fr, lds.min_tails, sched, jobs, best, lane, exited);
    if (lane == 0) {
      if (leaf) {
        mysols++;
        if (!exited && lb < best) atomicMin(&ctl->best, lb);
      } else if (!exited && lb < best) {
        const PFSPNode& p = lds.snodes[lds.lpar[ct]];
        emit_pfsp_child(childbuf, wave_slab + mycnt, p, p.depth, p.limit1, k);
        mycnt++;
      }
    }
  }
  if (lane == 0) {
    const unsigned long long gw = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
    waveCounts[gw] = mycnt;
    waveSols[gw] = mysols;
  }
}


// ---------------------------------------------------------------------------
// lb12: lb1_d picks the direction and filters the children (one thread per
// parent), lb2 refines only the survivors (one wave per survivor). Few
// children pass the filter (1.2-1.6 per parent on ta0xx with ub=1), so the
// survivors of a whole block go through one LDS queue and the waves take
// queue entries round-robin: the Johnson sweep runs on a dense set however
// unevenly the survivors are spread over the parents.
//
// lb1_d bounds a child from the PARENT's front / back, which are min_heads /
// min_tails where nothing is fixed; lb2 bounds the CHILD, whose changed side
// is one add_forward / add_backward step from ZEROS in that case. The rows
// phase 1 leaves in LDS are therefore the ones a child starts from: zeros on
// the side the parent's direction extends when nothing is fixed there, the
// lb1_d schedule (min_heads / min_tails included) on the other side.
// ---------------------------------------------------------------------------
template <int MM>
struct LdsLb12 {
  static constexpr int PAIRS = MM * (MM - 1) / 2;
  static constexpr int JP_LDS = PAIRS < 64 ? PAIRS : 64;  // as LdsLb2w: round-0 rows only
  LdsLb1Bi<MM> b1;
  uint32_t jp[JP_LDS * MAX_JOBS];
  uint8_t pair1[PAIRS], pair2[PAIRS];
  alignas(8) PFSPNode snodes[BLOCK];
  uint16_t fronts[BLOCK][MM + 1];  // per parent (values <= 20*20*99)
  uint16_t backs[BLOCK][MM + 1];
  uint32_t mask[BLOCK];  // jobs fixed at the front or at the back
  uint8_t dir[BLOCK];    // 0 front, 1 back
  // lb1_d survivors of the block in parent order, then position order:
  // parent << 8 | k; phase 2 sets LB12_PRUNED where lb2 prunes
  uint16_t queue[BLOCK * MAX_JOBS];
  uint16_t wrow[BLOCK / 64][MM + 2];  // a wave's current child: its changed side
};
constexpr uint16_t LB12_PRUNED = 0x80;

template <int MM>
__device__ inline void stage_lb12_tables(LdsLb12<MM>& lds, const PfspDevTables& tb, int jobs) {
  stage_lb1bi_tables<MM>(lds.b1, tb, jobs);
  for (int i = threadIdx.x; i < LdsLb12<MM>::JP_LDS * jobs; i += blockDim.x)
    lds.jp[i] = tb.johnson_packed_w[i];
  if (threadIdx.x < LdsLb12<MM>::PAIRS) {
    lds.pair1[threadIdx.x] = tb.pairs1_w[threadIdx.x];
    lds.pair2[threadIdx.x] = tb.pairs2_w[threadIdx.x];
  }
}

// What phase 1 found out about this thread's parent.
struct Lb12Parent {
  int depth = 0, limit1 = 0, limit2 = 0;
  bool bwd = false, leaf = false;
  int leaf_min = 0x7fffffff;  // leaf parent: min lb1_d value of the chosen direction
  uint32_t nsurv = 0;         // children passing the lb1_d filter (0 for a leaf)
  uint32_t qpos = 0;          // its first queue entry
};

// Phase 1, every thread of the block (lp < 0: no parent): lb1_d setup, pass 1
// and the direction as in k_pfsp_x_lb1d_bi; rows, mask and direction to LDS;
// pass 2 appends the survivors to the queue at the position an exclusive scan
// of the survivor counts gives (no atomics: the queue order is parent order,
// then position order). on_b1(k, b1) sees every child that gets no lb2: a
// leaf's children and the ones the filter pruned. Returns the queue length;
// ends with a block barrier.
template <int MM, class OnB1>
__device__ inline uint32_t lb12_phase1(LdsLb12<MM>& lds, int lp, int jobs, int best, int br,
                                       Lb12Parent& P, OnB1&& on_b1) {
  int front[MM], back[MM], remain[MM];
  if (lp >= 0) {
    const PFSPNode& p = lds.snodes[lp];
    P.depth = p.depth;
    P.limit1 = p.limit1;
    P.limit2 = jobs - p.nback;
    P.leaf = P.depth + 1 == jobs;
    lb1d_bi_setup<MM>(lds.b1, p.prmu, P.limit1, P.limit2, jobs, front, back, remain);
    const bool dyn = br == 3;
    P.bwd = br == 1 || (br == 2 && (P.depth & 1));
    int cntF = 0, cntB = 0, sumF = 0, sumB = 0;
    int minF = 0x7fffffff, minB = 0x7fffffff;
    for (int k = P.limit1 + 1; k < P.limit2; k++) {
      const int job = p.prmu[k];
      if (dyn || !P.bwd) {
        const int lb = lb1d_bound_front<MM>(lds.b1, front, back, remain, job, jobs);
        cntF += lb < best;
        sumF += lb;
        minF = min(minF, lb);
      }
      if (dyn || P.bwd) {
        const int lb = lb1d_bound_back<MM>(lds.b1, front, back, remain, job, jobs);
        cntB += lb < best;
        sumB += lb;
        minB = min(minB, lb);
      }
    }
    if (dyn) P.bwd = cntB < cntF || (cntB == cntF && sumB > sumF);
    P.leaf_min = P.bwd ? minB : minF;
    if (!P.leaf) P.nsurv = static_cast<uint32_t>(P.bwd ? cntB : cntF);
    uint32_t sched = 0;
    for (int i = 0; i <= P.limit1; i++) sched |= 1u << p.prmu[i];
    for (int i = P.limit2; i < jobs; i++) sched |= 1u << p.prmu[i];
    lds.mask[lp] = sched;
    lds.dir[lp] = P.bwd ? 1 : 0;
    const bool zero_front = !P.bwd && P.limit1 == -1;
    const bool zero_back = P.bwd && P.limit2 == jobs;
#pragma unroll
    for (int j = 0; j < MM; j++) {
      lds.fronts[lp][j] = static_cast<uint16_t>(zero_front ? 0 : front[j]);
      lds.backs[lp][j] = static_cast<uint16_t>(zero_back ? 0 : back[j]);
    }
  }
  uint32_t Q;
  P.qpos = block_excl_scan(P.nsurv, Q);
  if (lp >= 0) {
    const PFSPNode& p = lds.snodes[lp];
    uint32_t q = P.qpos;
    for (int k = P.limit1 + 1; k < P.limit2; k++) {
      const int job = p.prmu[k];
      const int b1 = P.bwd ? lb1d_bound_back<MM>(lds.b1, front, back, remain, job, jobs)
                           : lb1d_bound_front<MM>(lds.b1, front, back, remain, job, jobs);
      if (!P.leaf && b1 < best)
        lds.queue[q++] = static_cast<uint16_t>(lp << 8 | k);
      else
        on_b1(k, b1);
    }
  }
  __syncthreads();
  return Q;
}

// Phase 2: the block's waves take queue entries round-robin. One O(m) step
// from the parent's row makes the child's changed side (a wave-private LDS
// row: the sweep indexes it by the pair's machines), the other side is the
// parent's row, and the lanes sweep the pairs 64 per round. Lane 0 hands
// done(entry, parent, k, lb2, keep) the outcome; lb2 is exact unless the
// collective exit fired (then it is some value > best).
template <int MM, class Done>
__device__ inline void lb12_phase2(LdsLb12<MM>& lds, const PfspDevTables& tb, uint32_t Q,
                                   int jobs, int best, Done&& done) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  uint16_t* row = lds.wrow[wid];
  for (uint32_t e = wid; e < Q; e += BLOCK / 64) {
    const uint32_t ent = lds.queue[e];  // same address across the wave: broadcast
    const int lp = static_cast<int>(ent >> 8);
    const int k = static_cast<int>(ent & 0x7fu);
    const int job = lds.snodes[lp].prmu[k];
    const bool bwd = lds.dir[lp] != 0;
    if (!bwd) {  // add_forward
      const uint16_t* pf = lds.fronts[lp];
      int prev = pf[0] + lds.b1.p[job];
      if (lane == 0) row[0] = static_cast<uint16_t>(prev);
#pragma unroll
      for (int j = 1; j < MM; j++) {
        prev = max(prev, static_cast<int>(pf[j])) + lds.b1.p[j * jobs + job];
        if (lane == 0) row[j] = static_cast<uint16_t>(prev);
      }
    } else {  // add_backward
      const uint16_t* pb = lds.backs[lp];
      int prev = pb[MM - 1] + lds.b1.p[(MM - 1) * jobs + job];
      if (lane == 0) row[MM - 1] = static_cast<uint16_t>(prev);
#pragma unroll
      for (int jj = 0; jj < MM - 1; jj++) {
        const int j = MM - 2 - jj;
        prev = max(prev, static_cast<int>(pb[j])) + lds.b1.p[j * jobs + job];
        if (lane == 0) row[j] = static_cast<uint16_t>(prev);
      }
    }
    // lane 0 wrote the row the whole wave reads next: order this wave's LDS traffic
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const uint32_t sched = lds.mask[lp] | (1u << job);
    const uint16_t* fr = bwd ? lds.fronts[lp] : row;
    const uint16_t* bk = bwd ? row : lds.backs[lp];
    bool exited = false;
    const int lb = wave_lb2_sweep<MM>(lds, tb, fr, bk, sched, jobs, best, lane, exited);
    if (lane == 0) done(e, lp, k, lb, !exited && lb < best);
    // the next entry overwrites the row: every lane's reads of it come first
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
}

// K1 for PFSP lb12, geometry code 4 = the lb1_d geometry: one parent per
// thread, grid ceil(M / BLOCK), one BLOCK*MAX_JOBS slab and one count per
// block, so k_presum / k_gather2 see the contract of code 0. br: 0 fwd, 1 bwd,
// 2 alt, 3 minbranch. `best` is the snapshot read at kernel start; only leaves
// atomicMin into ctl->best.
template <int MM>
__global__ void k_pfsp_x_lb12(DevCtl* ctl, const PFSPNode* pool, PFSPNode* childbuf,
                              uint32_t* blockCounts, unsigned long long* blockSols, int jobs,
                              PfspDevTables tb, unsigned long long m, unsigned long long M,
                              int br) {
  __shared__ LdsLb12<MM> lds;
  stage_lb12_tables<MM>(lds, tb, jobs);
  const unsigned long long c = derive_chunk(ctl, m, M);
  const PFSPNode* parents = pool + (ctl->size - c);
  const unsigned long long t =
      static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int lp = stage_parents(parents, c, 1, lds.snodes, t);
  __syncthreads();
  const int best = ctl->best;

  Lb12Parent P;
  const uint32_t Q = lb12_phase1<MM>(lds, lp, jobs, best, br, P, [](int, int) {});
  unsigned long long sols = 0;
  if (lp >= 0 && P.leaf) {
    sols = static_cast<unsigned long long>(P.limit2 - (P.limit1 + 1));
    if (sols > 0 && P.leaf_min < best) atomicMin(&ctl->best, P.leaf_min);
  }
  lb12_phase2<MM>(lds, tb, Q, jobs, best, [&](uint32_t e, int, int, int, bool keep) {
    if (!keep) lds.queue[e] |= LB12_PRUNED;
  });
  __syncthreads();

  // phase 3: rank the kept children by a second scan, in queue order
  uint32_t cnt = 0;
  for (uint32_t e = P.qpos; e < P.qpos + P.nsurv; e++) cnt += !(lds.queue[e] & LB12_PRUNED);
  uint32_t totC;
  const uint32_t pre = block_excl_scan(cnt, totC);
  const unsigned long long totS = block_reduce_u64(sols);
  if (threadIdx.x == 0) {
    blockCounts[blockIdx.x] = totC;
    blockSols[blockIdx.x] = totS;
  }
  if (cnt > 0) {
    unsigned long long slot =
        static_cast<unsigned long long>(blockIdx.x) * (BLOCK * MAX_JOBS) + pre;
    const PFSPNode& p = lds.snodes[lp];
    for (uint32_t e = P.qpos; e < P.qpos + P.nsurv; e++) {
      const uint32_t ent = lds.queue[e];
      if (ent & LB12_PRUNED) continue;
      const int k = static_cast<int>(ent & 0x7fu);
      if (P.bwd)
        emit_pfsp_child_back(childbuf, slot++, p, P.depth, jobs - P.limit2, jobs, k);
      else
        emit_pfsp_child_front(childbuf, slot++, p, P.depth, P.limit1, k);
    }
  }
}

// lb12 hostpool / test kernel: phases 1-2 of the expand, outcomes written out
// instead of children. dir[n]: 0 front, 1 back. bounds[n * jobs] by position:
// untouched outside the unscheduled range (callers preset -1), the lb1_d value
// for a leaf's children and for the ones the filter pruned, else the lb2 value
// (exact when <= best; any value > best once the collective exit fired).
template <int MM>
__global__ void k_pfsp_eval_lb12(const PFSPNode* parents, int n, int jobs, PfspDevTables tb,
                                 int best, int br, uint8_t* dir, int32_t* bounds) {
  __shared__ LdsLb12<MM> lds;
  stage_lb12_tables<MM>(lds, tb, jobs);
  const unsigned long long t =
      static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int lp = stage_parents(parents, static_cast<unsigned long long>(n), 1, lds.snodes, t);
  __syncthreads();
  Lb12Parent P;
  int32_t* mine = bounds + t * jobs;
  const uint32_t Q =
      lb12_phase1<MM>(lds, lp, jobs, best, br, P, [&](int k, int b1) { mine[k] = b1; });
  if (lp >= 0) dir[t] = P.bwd ? 1 : 0;
  int32_t* blk = bounds + static_cast<unsigned long long>(blockIdx.x) * blockDim.x * jobs;
  lb12_phase2<MM>(lds, tb, Q, jobs, best, [&](uint32_t, int lp2, int k, int lb, bool) {
    blk[lp2 * jobs + k] = lb;
  });
}

// Per-256-entry group sums of the wave counts: with per-WAVE count granularity
// (lb2's G ~ 15k at M = 50000) the gather blocks' linear prefix walk costs
// more than the expand itself; group sums cut each block's walk from G loads
// to G/256 + 255.
__global__ void k_presum(const uint32_t* blockCounts, uint32_t* groupSums, int G) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  const uint32_t v = (i < G) ? blockCounts[i] : 0;
  uint32_t tot;
  block_excl_scan(v, tot);
  if (threadIdx.x == 0) groupSums[blockIdx.x] = tot;
}

// K2+K3 merged ("gather2"), one RUN of R consecutive count entries per block.
// Every wave of the block loads the run's R counts into its lanes [0, R); a
// run that carries no children returns there, before any walk or barrier
// (most runs do: slabs of parents whose children all went to the in-kernel
// finisher, and the grid's tail beyond the live chunk). The others derive the
// run's pool offset once — whole-group sums before the run's group plus the
// counts of its group before its first entry (R divides 256, so a run never
// straddles a k_presum group); without groupSums a linear walk over the
// entries before it — and the in-run offsets by a wave scan of the R counts.
// Each wave does this redundantly (the loads hit L2), so the copy needs no
// LDS and no barrier: small slabs go one per wave, a slab above
// GATHER_WAVE_WORDS is copied by the whole block; destinations are disjoint.
// The LAST block alone sums the sol / extra counts and writes the next
// iteration's control block. Control blocks alternate per iteration (parity)
// so readers of iteration i never race the writer: expand(i) and gather2(i)
// read ctl_cur, gather2's last block writes ctl_next, and the kernel boundary
// publishes it for iteration i+1 (placement-independent). Count entries at
// index >= G are never read: the buffers hold stale counts of wider
// iterations there.
constexpr int GATHER_WAVE_WORDS = 256;  // largest slab (8-byte words) left to one wave

template <class NodeT, int R>
__global__ void k_gather2(const DevCtl* ctl_cur, DevCtl* ctl_next, const uint32_t* blockCounts,
                          const unsigned long long* blockSols,
                          const unsigned long long* blockExtra, const uint32_t* groupSums,
                          const NodeT* childbuf, NodeT* pool, int strideNodes, int G,
                          unsigned long long m, unsigned long long M,
                          unsigned long long capacity) {
  static_assert(R >= 1 && R <= 64 && (R & (R - 1)) == 0 && BLOCK % R == 0,
                "a run is a power of two that divides a presum group and fits a wave");
  static_assert(sizeof(NodeT) % 8 == 0, "nodes are copied as 8-byte words");
  constexpr int WPN = static_cast<int>(sizeof(NodeT) / 8);
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int e0 = static_cast<int>(blockIdx.x) * R;  // first count entry of the run
  const bool last = (blockIdx.x == gridDim.x - 1);

  // the run's counts, in lanes [0, R) of every wave: the same values in all
  // four waves, so what follows from them is block-uniform
  const uint32_t cnt = (lane < R && e0 + lane < G) ? blockCounts[e0 + lane] : 0;
  if (!last && __ballot(cnt != 0) == 0) return;

  const unsigned long long c = derive_chunk(ctl_cur, m, M);
  const unsigned long long base = ctl_cur->size - c;
  const bool dead = ctl_cur->overflow != 0;

  // prefix over count entries [0, e0), once per run
  uint32_t pre = 0;
  if (groupSums) {
    const int gfull = e0 / BLOCK;  // whole groups strictly before the run
    for (int i = lane; i < gfull; i += 64) pre += groupSums[i];
    for (int i = gfull * BLOCK + lane; i < e0; i += 64) pre += blockCounts[i];
  } else {
    for (int i = lane; i < e0; i += 64) pre += blockCounts[i];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) pre += __shfl_xor(pre, d);

  // inclusive scan of the run's counts over lanes [0, R)
  uint32_t inc = cnt;
#pragma unroll
  for (int d = 1; d < R; d <<= 1) {
    const uint32_t y = __shfl_up(inc, d);
    if (lane >= d) inc += y;
  }
  const uint32_t run_tot = static_cast<uint32_t>(
      __builtin_amdgcn_readlane(static_cast<int>(inc), R - 1));

  // copy the non-empty slabs, in entry order of the pool
  bool over = dead;
  for (int s = 0; s < R; s++) {
    const uint32_t cs = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cnt), s));
    if (cs == 0) continue;
    const uint32_t is = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(inc), s));
    const unsigned long long off = base + pre + (is - cs);
    if (dead || off + cs > capacity) {
      over = true;
      continue;
    }
    const int words = static_cast<int>(cs) * WPN;
    const bool whole = words > GATHER_WAVE_WORDS;
    if (!whole && (s & 3) != wid) continue;
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(
        childbuf + static_cast<unsigned long long>(e0 + s) * strideNodes);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(pool + off);
    const int step = whole ? BLOCK : 64;
    for (int i = whole ? static_cast<int>(threadIdx.x) : lane; i < words; i += step)
      dst[i] = src[i];
  }
  if (over && threadIdx.x == 0) ctl_next->overflow = 1;  // sticky; host aborts

  if (last) {  // block-uniform: the barriers below are reached by the whole block
    unsigned long long my_sols = 0, my_extra = 0;
    for (int i = threadIdx.x; i < G; i += BLOCK) {
      my_sols += blockSols[i];
      if (blockExtra) my_extra += blockExtra[i];
    }
    const unsigned long long sol_tot = block_reduce_u64(my_sols);
    const unsigned long long extra_tot = block_reduce_u64(my_extra);
    if (threadIdx.x == 0) {
      const unsigned long long total = static_cast<unsigned long long>(pre) + run_tot;
      if (!dead && base + total <= capacity) {
        ctl_next->size = base + total;
        ctl_next->tree = ctl_cur->tree + total + extra_tot;
        ctl_next->sol = ctl_cur->sol + sol_tot;
        ctl_next->iters = ctl_cur->iters + (c > 0);
        ctl_next->chunk = c;
        ctl_next->overflow = ctl_cur->overflow;
      }
      ctl_next->best = ctl_cur->best;  // carries expand's atomicMin updates
    }
  }
}

// ---------------------------------------------------------------------------
// Host-callable launchers (C++ linkage, used by engine_gpu.cpp)
// ---------------------------------------------------------------------------

static inline int grid_for(unsigned long long threads) {
  return static_cast<int>((threads + BLOCK - 1) / BLOCK);
}

void launch_nq_eval(const NQNode* parents, int n, int N, int g, uint8_t* labels,
                    hipStream_t s) {
  hipLaunchKernelGGL(k_nq_eval, dim3(grid_for(static_cast<unsigned long long>(n) * N)),
                     dim3(BLOCK), 0, s, parents, n, N, g, labels);
}

template <int MM>
static void launch_pfsp_eval_mm(const PFSPNode* parents, int n, int jobs, int lbk,
                                const PfspDevTables& tb, int best, int32_t* bounds,
                                hipStream_t s, int br, int32_t* bounds_end, uint8_t* dir) {
  if (lbk == 4) {  // lb12: thread per parent, then wave per lb1_d survivor
    hipLaunchKernelGGL((k_pfsp_eval_lb12<MM>), dim3(grid_for(n)), dim3(BLOCK), 0, s, parents,
                       n, jobs, tb, best, br, dir, bounds);
  } else if (br != 0) {  // lb1_d in both directions (launch_pfsp_eval rejects other bounds)
    hipLaunchKernelGGL((k_pfsp_eval_lb1d_bi<MM>), dim3(grid_for(n)), dim3(BLOCK), 0, s,
                       parents, n, jobs, tb, bounds, bounds_end);
  } else if (lbk == 0) {  // lb1_d: thread per parent
    hipLaunchKernelGGL((k_pfsp_eval_lb1d<MM>), dim3(grid_for(n)), dim3(BLOCK), 0, s, parents,
                       n, jobs, tb, bounds);
  } else if (lbk == 1) {
    hipLaunchKernelGGL((k_pfsp_eval_lb1<MM>),
                       dim3(grid_for(static_cast<unsigned long long>(n) * jobs)), dim3(BLOCK),
                       0, s, parents, n, jobs, tb, bounds);
  } else {
    hipLaunchKernelGGL((k_pfsp_eval_lb2<MM>),
                       dim3(grid_for(static_cast<unsigned long long>(n) * jobs)), dim3(BLOCK),
                       0, s, parents, n, jobs, tb, best, bounds);
  }
}

void launch_pfsp_eval(const PFSPNode* parents, int n, int jobs, int machines, int lbk,
                      const PfspDevTables& tb, int best, int32_t* bounds, hipStream_t s,
                      int br, int32_t* bounds_end, uint8_t* dir) {
  if (lbk == 4 && dir == nullptr)
    throw std::invalid_argument("launch_pfsp_eval: lb12 needs a dir buffer");
  if (lbk != 4 && br != 0 && (lbk != 0 || bounds_end == nullptr))
    throw std::invalid_argument(
        "launch_pfsp_eval: a non-fwd branching rule needs lb1_d and a bounds_end buffer");
  if (machines == 5)
    launch_pfsp_eval_mm<5>(parents, n, jobs, lbk, tb, best, bounds, s, br, bounds_end, dir);
  else if (machines == 10)
    launch_pfsp_eval_mm<10>(parents, n, jobs, lbk, tb, best, bounds, s, br, bounds_end, dir);
  else
    launch_pfsp_eval_mm<20>(parents, n, jobs, lbk, tb, best, bounds, s, br, bounds_end, dir);
}

// ---- devpool v3 launchers ----

// lbk geometry codes: 0 = lb1_d (thread per parent), 1 = thread-per-child
// (lb1), 2 = wave-cooperative lb2 (per-wave slabs), 3 = PER-LANE lb2 with
// thread-per-child geometry — used when machines <= 10: with only 10-45
// machine pairs the wave-cooperative kernel leaves most of a wave idle and
// its collective early exit buys little, while the per-lane full sweep is a
// short fully-unrolled register loop (ta005 20x5 measured 3x faster).
// 4 = lb12: the lb1_d geometry (thread per parent, per-block slabs and counts).
int devpool_lbk_geom(int lbk, int machines) {
  if (lbk != 2) return lbk;
  // per-lane for m=5 (10 pairs: the wave kernel idles 54/64 lanes, ta005
  // 31.5 -> 10.9 s); wave for m=10+ (45+ pairs: measured 25% faster on
  // ta018 at m=10, and the collective exit dominates at m=20)
  int cut = 5;
  if (const char* e = std::getenv("GATS_LB2_LANE_MAX")) cut = atoi(e);
  return (machines <= cut) ? 3 : lbk;
}

int devpool_grid(unsigned long long M, int per, int lbk) {
  if (lbk == 0 || lbk == 4)  // lb1_d, lb12: one thread per parent
    return static_cast<int>((M + BLOCK - 1) / BLOCK);
  if (lbk == 2)  // wave-cooperative lb2: counts/slabs are per WAVE (64 slots),
                 // padded to whole 4-wave blocks (gw index = blockIdx*4 + wid)
    return static_cast<int>((M * per + BLOCK - 1) / BLOCK) * 4;
  return static_cast<int>((M * per + EMIT_TILE - 1) / EMIT_TILE);
}

int devpool_stride(int lbk) {
  if (lbk == 0 || lbk == 4) return BLOCK * MAX_JOBS;
  if (lbk == 2) return 64;  // one wave's child slab
  return EMIT_TILE;
}

void launch_nq_x(const DevCtl* ctl, const NQNode* pool, NQNode* childbuf,
                 uint32_t* blockCounts, unsigned long long* blockSols,
                 unsigned long long* blockExtra, int N, int g, const NqFinishOpts& o,
                 unsigned long long m, unsigned long long M, hipStream_t s) {
  // resolved options (nq_finish_opts): refill counts idle lanes of a 64-lane
  // wave, and the kernel's stack writes stay below stack_cap, inside the array
  if (o.refill < 1 || o.refill > 64 || o.stack_cap < 0 || o.stack_cap > NQ_STACK_CAP)
    throw std::logic_error("launch_nq_x: finisher options were not resolved");
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(devpool_grid(M, N, 1)), dim3(BLOCK), 0, s, ctl, pool,
                       childbuf, blockCounts, blockSols, blockExtra, N, g, o.finish, o.refill,
                       o.stack_cap, m, M);
  };
  const NqDrain d = o.stack        ? NqDrain::stack
                    : o.split <= 0 ? NqDrain::flat
                    : o.split == 1 ? NqDrain::split1
                                   : NqDrain::split2;
  auto pick = [&](auto g1) {
    constexpr bool G1 = decltype(g1)::value;
    switch (d) {
      case NqDrain::flat: return go(k_nq_x<G1, NqDrain::flat>);
      case NqDrain::split1: return go(k_nq_x<G1, NqDrain::split1>);
      case NqDrain::split2: return go(k_nq_x<G1, NqDrain::split2>);
      case NqDrain::stack: return go(k_nq_x<G1, NqDrain::stack>);
    }
  };
  g == 1 ? pick(std::true_type{}) : pick(std::false_type{});
}

template <int MM>
static void launch_pfsp_x_mm(DevCtl* ctl, const PFSPNode* pool, PFSPNode* childbuf,
                             uint32_t* bc, unsigned long long* bs, int jobs, int lbk,
                             const PfspDevTables& tb, unsigned long long m,
                             unsigned long long M, hipStream_t s, int br) {
  if (lbk == 4) {  // lb12, every branching rule
    hipLaunchKernelGGL((k_pfsp_x_lb12<MM>), dim3(devpool_grid(M, jobs, 4)), dim3(BLOCK), 0, s,
                       ctl, pool, childbuf, bc, bs, jobs, tb, m, M, br);
  } else if (br != 0) {  // lb1_d geometry (code 0), both-directions kernel
    hipLaunchKernelGGL((k_pfsp_x_lb1d_bi<MM>), dim3(devpool_grid(M, jobs, 0)), dim3(BLOCK), 0,
                       s, ctl, pool, childbuf, bc, bs, jobs, tb, m, M, br);
  } else if (lbk == 0) {
    hipLaunchKernelGGL((k_pfsp_x_lb1d<MM>), dim3(devpool_grid(M, jobs, 0)), dim3(BLOCK), 0, s,
                       ctl, pool, childbuf, bc, bs, jobs, tb, m, M);
  } else if (lbk == 1) {
    hipLaunchKernelGGL((k_pfsp_x<MM, 1>), dim3(devpool_grid(M, jobs, 1)), dim3(BLOCK), 0, s,
                       ctl, pool, childbuf, bc, bs, jobs, tb, m, M);
  } else if (lbk == 3) {  // per-lane lb2, thread-per-child geometry
    hipLaunchKernelGGL((k_pfsp_x<MM, 2>), dim3(devpool_grid(M, jobs, 1)), dim3(BLOCK), 0, s,
                       ctl, pool, childbuf, bc, bs, jobs, tb, m, M);
  } else {
    // 256 child slots per block (4 waves x 64); count arrays are per wave
    const int blocks = static_cast<int>((M * jobs + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL((k_pfsp_x_lb2w<MM>), dim3(blocks), dim3(BLOCK), 0, s, ctl, pool,
                       childbuf, bc, bs, jobs, tb, m, M);
  }
}

void launch_pfsp_x(DevCtl* ctl, const PFSPNode* pool, PFSPNode* childbuf, uint32_t* bc,
                   unsigned long long* bs, int jobs, int machines, int lbk,
                   const PfspDevTables& tb,
                   unsigned long long m, unsigned long long M, hipStream_t s, int br) {
  if (br != 0 && lbk != 0 && lbk != 4)
    throw std::invalid_argument("launch_pfsp_x: a non-fwd branching rule needs lb1_d or lb12");
  if (machines == 5)
    launch_pfsp_x_mm<5>(ctl, pool, childbuf, bc, bs, jobs, lbk, tb, m, M, s, br);
  else if (machines == 10)
    launch_pfsp_x_mm<10>(ctl, pool, childbuf, bc, bs, jobs, lbk, tb, m, M, s, br);
  else
    launch_pfsp_x_mm<20>(ctl, pool, childbuf, bc, bs, jobs, lbk, tb, m, M, s, br);
}

void launch_presum(const uint32_t* bc, uint32_t* groupSums, int G, hipStream_t s) {
  hipLaunchKernelGGL(k_presum, dim3((G + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, bc,
                     groupSums, G);
}

// Count entries per gather block. One value serves every geometry (BASELINE.md,
// "Gather by runs"); GATS_GATHER_R = 4 / 8 / 16 / 32 overrides it for sweeps.
constexpr int GATHER_RUN = 4;

static int gather_run() {
  static const int r = [] {
    if (const char* e = std::getenv("GATS_GATHER_R")) {
      const int v = atoi(e);
      if (v == 4 || v == 8 || v == 16 || v == 32) return v;
    }
    return GATHER_RUN;
  }();
  return r;
}

template <class NodeT>
static void launch_gather2(const DevCtl* ctl_cur, DevCtl* ctl_next, const uint32_t* bc,
                           const unsigned long long* bs, const unsigned long long* be,
                           const uint32_t* groupSums, const NodeT* childbuf, NodeT* pool,
                           int strideNodes, int G, unsigned long long m, unsigned long long M,
                           unsigned long long capacity, hipStream_t s) {
  const int R = gather_run();
  const dim3 grid((G + R - 1) / R);
#define GATS_GATHER_CASE(RR)                                                                  \
  case RR:                                                                                    \
    hipLaunchKernelGGL((k_gather2<NodeT, RR>), grid, dim3(BLOCK), 0, s, ctl_cur, ctl_next, bc, \
                       bs, be, groupSums, childbuf, pool, strideNodes, G, m, M, capacity);    \
    break;
  switch (R) {
    GATS_GATHER_CASE(4)
    GATS_GATHER_CASE(8)
    GATS_GATHER_CASE(32)
    default:
      GATS_GATHER_CASE(16)
  }
#undef GATS_GATHER_CASE
}

void launch_gather2_nq(const DevCtl* ctl_cur, DevCtl* ctl_next, const uint32_t* bc,
                       const unsigned long long* bs, const unsigned long long* be,
                       const uint32_t* groupSums, const NQNode* childbuf, NQNode* pool,
                       int strideNodes, int G, unsigned long long m, unsigned long long M,
                       unsigned long long capacity, hipStream_t s) {
  launch_gather2<NQNode>(ctl_cur, ctl_next, bc, bs, be, groupSums, childbuf, pool, strideNodes,
                         G, m, M, capacity, s);
}

void launch_gather2_pfsp(const DevCtl* ctl_cur, DevCtl* ctl_next, const uint32_t* bc,
                         const unsigned long long* bs, const uint32_t* groupSums,
                         const PFSPNode* childbuf, PFSPNode* pool, int strideNodes, int G,
                         unsigned long long m, unsigned long long M,
                         unsigned long long capacity, hipStream_t s) {
  launch_gather2<PFSPNode>(ctl_cur, ctl_next, bc, bs, nullptr, groupSums, childbuf, pool,
                           strideNodes, G, m, M, capacity, s);
}

}  // namespace gats
