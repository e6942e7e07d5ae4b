// eppk_bounded.hip.h — the picker "best-score under per-pod caps" (SEMANTICS.md §3d; include/eppk.h eppk_bounded_resolve_device).
//
// Included by eppk.hip alone: the thirty pick units do not see this file, so a change here rebuilds one unit.
//
// The resolve takes every request's ordered list of k pods and a room per pod, and works in k ROUNDS: in round j every request that is
// still unassigned bids for entry j of its list, and of a pod's bidders the first `room` IN BATCH ORDER are accepted.  All of a round
// is decided on the loads as the round before left them.  Nothing here lets the arrival order of an atomic decide a pick: a request's
// place among the bidders of its pod comes from its index alone --
//     place = (bidders for the pod in the CHUNKS in front of the request's chunk)      bounded_scan_kernel: exclusive prefix over chunks
//           + (bidders for the pod in front of the request INSIDE its chunk)           bounded_wave_round: one wavefront walks the chunk
// -- so the result does not depend on the chunk size, the grid or the number of CUs.  The only atomics are adds whose result is not
// read (histogram counts in LDS; the load of a pod that takes spilled requests).
//
// A chunk is `chunk` consecutive requests (a power of two >= 64; eppk_bounded_geometry).  Two forms:
//   batch <= chunk    bounded_resolve_one_kernel: one workgroup, all k rounds and the finish in one launch (the small-batch latency case)
//   batch >  chunk    per round bounded_count_kernel   per chunk, a histogram of the round's bids            -> hist[chunk][pod]
//                               bounded_scan_kernel    per pod: hist := exclusive prefix over the chunks, room[pod], load[pod] += accepted
//                               bounded_assign_kernel  per chunk: place < room -> pick, score, rank
//                     then bounded_finish_kernel for what no round placed (SHED / SPILL / no valid entry).  Launches are ordered by the
//                     stream; no workgroup waits for another.
// `state` is one byte per request: kBoundUnassigned until a round places the request, then its rank.  It is the caller's rank array when
// there is one.
#ifndef EPPK_BOUNDED_HIP_H
#define EPPK_BOUNDED_HIP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eppk.h"

namespace eppk {

constexpr uint32_t kBoundUnassigned = 0xFFu;       // state of a request no round has placed yet (no rank has this value)
constexpr uint32_t kBoundThreads = 256u;
constexpr uint32_t kBoundDefaultChunk = 512u;      // EPPK_BOUND_CHUNK

__device__ __forceinline__ bool bounded_valid(int32_t e, uint32_t n_pods) { return (uint32_t)e < n_pods; }   // (a negative entry is a huge unsigned)

// Room of pod p in the one-launch kernel: from the caps and the loads in LDS, which stay as they are for the length of a round.
struct BoundRoomLds {
  const uint32_t* cap; uint32_t cap_all; const uint32_t* load;
  __device__ __forceinline__ uint32_t operator()(uint32_t p) const {
    const uint32_t c = cap ? cap[p] : cap_all, l = load[p];
    return c > l ? c - l : 0u;
  }
};
// ... and in the assign pass: what the scan pass wrote.
struct BoundRoomArray {
  const uint32_t* room;
  __device__ __forceinline__ uint32_t operator()(uint32_t p) const { return room[p]; }
};

// The request at place i of the order the wavefront walks: the batch's own order here; eppk_banded.hip.h walks a permutation.
struct BoundRowSelf {
  __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return i; }
};

// ONE wavefront takes places [r0, r1) through round j, 64 per trip in ascending order; place i holds request row(i).  cnt[] (LDS, one
// counter per pod) holds, for every pod, the number of this round's bidders in front of the place the wavefront is at: the caller sets
// it for r0, every trip carries it on.  Within a trip the lanes that bid for one pod find each other by ballot; a lane's place is the counter plus the bidding lanes
// below it.  Every index into cnt[] has passed bounded_valid (p < n_pods <= EPPK_MAX_PODS).
template <class Room, class Row = BoundRowSelf>
__device__ __forceinline__ void bounded_wave_round(const int32_t* __restrict__ lists, const double* __restrict__ scores, uint32_t k, uint32_t j,
                                                   uint64_t r0, uint64_t r1, uint32_t n_pods, uint32_t* cnt, const Room room,
                                                   uint8_t* state, int32_t* __restrict__ out_pick, double* __restrict__ out_score,
                                                   const Row row = Row{}) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint64_t t0 = r0; t0 < r1; t0 += 64u) {
    uint64_t r = t0 + lane;
    int32_t e = EPPK_NO_PICK;
    bool bid = false;
    if (r < r1) {
      r = row(r);
      if (state[r] == kBoundUnassigned) {
        e = lists[r * k + j];
        bid = bounded_valid(e, n_pods);
      }
    }
    bool take = false;
    for (uint64_t todo = __ballot(bid); todo != 0ull;) {            // (wave-uniform: one trip of this loop per distinct pod)
      const int32_t p0 = __shfl(e, (int)__builtin_ctzll(todo));
      const bool mine = bid && e == p0;
      const uint64_t m = __ballot(mine);
      const uint32_t before = cnt[p0];                              // (every lane reads the same word: a broadcast)
      if (mine) take = before + (uint32_t)__popcll(m & below) < room((uint32_t)p0);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (mine && (m & below) == 0ull) cnt[p0] = before + (uint32_t)__popcll(m);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      todo &= ~m;
    }
    if (take) {
      state[r] = (uint8_t)j;
      out_pick[r] = e;
      if (out_score) out_score[r] = scores ? scores[r * k + j] : 0.0;
    }
  }
}

// What is left of request r when the rounds are over (state[r] == kBoundUnassigned), and the check of every entry of its list.
// Returns the pod that takes a spilled request, else EPPK_NO_PICK.
__device__ __forceinline__ int32_t bounded_finish_row(const int32_t* __restrict__ lists, const double* __restrict__ scores, uint32_t k, uint64_t r,
                                                      uint32_t n_pods, uint32_t policy, uint8_t* state, int32_t* __restrict__ out_pick,
                                                      double* __restrict__ out_score, uint32_t* __restrict__ status) {
  uint32_t first = k;
  bool bad = false;
  for (uint32_t i = 0; i < k; ++i) {
    const int32_t e = lists[r * k + i];
    if (bounded_valid(e, n_pods)) { if (first == k) first = i; }
    else if (e != EPPK_NO_PICK) bad = true;
  }
  if (bad) atomicOr(status, EPPK_LAUNCH_BAD_PICK);
  if (state[r] != kBoundUnassigned) return EPPK_NO_PICK;           // (placed by a round: pick, score and rank are written)
  int32_t pick = EPPK_NO_PICK;
  double score = 0.0;
  uint32_t rank = EPPK_RANK_NONE;
  if (first != k) {
    rank = EPPK_RANK_OVERFLOW;
    if (policy == EPPK_BOUNDED_SPILL) {
      pick = lists[r * k + first];
      score = scores ? scores[r * k + first] : 0.0;
      rank |= first;
    }
  }
  out_pick[r] = pick;
  if (out_score) out_score[r] = score;
  state[r] = (uint8_t)rank;
  return pick;
}

// batch <= chunk: one workgroup.  Wavefront 0 walks the rows, all four take the passes over the pods.
__global__ __launch_bounds__(kBoundThreads) void bounded_resolve_one_kernel(const int32_t* __restrict__ lists, const double* __restrict__ scores,
                                                                            uint32_t n_reqs, uint32_t k, uint32_t n_pods,
                                                                            const uint32_t* __restrict__ cap, uint32_t cap_all, uint32_t policy,
                                                                            uint32_t* load, int32_t* __restrict__ out_pick,
                                                                            double* __restrict__ out_score, uint8_t* state, uint32_t* __restrict__ status) {
  __shared__ uint32_t s_cnt[EPPK_MAX_PODS], s_load[EPPK_MAX_PODS];
  if (n_pods > EPPK_MAX_PODS) return;
  for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) { s_cnt[p] = 0u; s_load[p] = load ? load[p] : 0u; }
  for (uint32_t r = threadIdx.x; r < n_reqs; r += kBoundThreads) state[r] = (uint8_t)kBoundUnassigned;
  __syncthreads();
  const BoundRoomLds room{cap, cap_all, s_load};
  for (uint32_t j = 0; j < k; ++j) {
    if (threadIdx.x < 64u) bounded_wave_round(lists, scores, k, j, 0ull, (uint64_t)n_reqs, n_pods, s_cnt, room, state, out_pick, out_score);
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) {    // the loads the next round sees; the counters start over
      const uint32_t bids = s_cnt[p];
      if (bids) {
        const uint32_t rm = room(p);
        s_load[p] += bids < rm ? bids : rm;
        s_cnt[p] = 0u;
      }
    }
    __syncthreads();
  }
  for (uint32_t r = threadIdx.x; r < n_reqs; r += kBoundThreads) {
    const int32_t spill = bounded_finish_row(lists, scores, k, r, n_pods, policy, state, out_pick, out_score, status);
    if (spill != EPPK_NO_PICK) atomicAdd(&s_load[spill], 1u);          // (a count: the result of the add is not read)
  }
  __syncthreads();
  if (load) for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) load[p] = s_load[p];
}

// Count pass of round j.  A workgroup per chunk (grid-stride): the histogram of the chunk's bids, in LDS, then row `chunk` of hist.
__global__ __launch_bounds__(kBoundThreads) void bounded_count_kernel(const int32_t* __restrict__ lists, uint32_t n_reqs, uint32_t k, uint32_t j,
                                                                      uint32_t n_pods, uint32_t chunk, uint32_t n_chunks,
                                                                      const uint8_t* __restrict__ state, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_cnt[EPPK_MAX_PODS];
  if (n_pods > EPPK_MAX_PODS) return;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) s_cnt[p] = 0u;
    __syncthreads();
    const uint64_t r0 = (uint64_t)c * chunk, r1 = r0 + chunk < n_reqs ? r0 + chunk : n_reqs;
    for (uint64_t r = r0 + threadIdx.x; r < r1; r += kBoundThreads)
      if (state[r] == kBoundUnassigned) {
        const int32_t e = lists[r * k + j];
        if (bounded_valid(e, n_pods)) atomicAdd(&s_cnt[e], 1u);        // (a count: the result of the add is not read)
      }
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) hist[(size_t)c * n_pods + p] = s_cnt[p];
    __syncthreads();
  }
}

// Scan pass.  Per pod: its column of hist becomes the exclusive prefix over the chunks; the room of the round, from the load as the round
// before left it; the load the round leaves.  A workgroup takes kBoundScanPods pods at a time (grid-stride) and cuts the chunks into
// kBoundScanSegs segments, one thread per (segment, pod): segment sums, their prefix through LDS, then the prefix inside the segment --
// a thread per pod alone would walk the chunks one dependent load at a time.  Integer sums: the cut does not show in the result.
constexpr uint32_t kBoundScanSegs = 16u, kBoundScanPods = 16u;
__global__ __launch_bounds__(kBoundScanSegs * kBoundScanPods) void bounded_scan_kernel(uint32_t* hist, uint32_t n_chunks, uint32_t n_pods,
                                                                                      const uint32_t* __restrict__ cap, uint32_t cap_all,
                                                                                      uint32_t* __restrict__ load, uint32_t* __restrict__ room) {
  __shared__ uint32_t s_sum[kBoundScanSegs][kBoundScanPods];
  const uint32_t lp = threadIdx.x % kBoundScanPods, seg = threadIdx.x / kBoundScanPods;
  const uint32_t seg_len = (n_chunks + kBoundScanSegs - 1u) / kBoundScanSegs;
  const uint32_t c0 = seg * seg_len < n_chunks ? seg * seg_len : n_chunks, c1 = c0 + seg_len < n_chunks ? c0 + seg_len : n_chunks;
  for (uint32_t pb = blockIdx.x * kBoundScanPods; pb < n_pods; pb += gridDim.x * kBoundScanPods) {     // (uniform over the workgroup)
    const uint32_t p = pb + lp;
    const bool live = p < n_pods;
    uint32_t sum = 0u;
    if (live) {
#pragma unroll 8
      for (uint32_t c = c0; c < c1; ++c) sum += hist[(size_t)c * n_pods + p];
    }
    s_sum[seg][lp] = sum;
    __syncthreads();
    uint32_t run = 0u, total = 0u;
    for (uint32_t s2 = 0; s2 < kBoundScanSegs; ++s2) {
      const uint32_t v = s_sum[s2][lp];
      if (s2 < seg) run += v;
      total += v;
    }
    if (live) {
      for (uint32_t c = c0; c < c1; c += 8u) {                     // eight loads in flight, then their prefix
        uint32_t v[8];
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) v[i] = c + i < c1 ? hist[(size_t)(c + i) * n_pods + p] : 0u;
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i)
          if (c + i < c1) { hist[(size_t)(c + i) * n_pods + p] = run; run += v[i]; }
      }
      if (seg == 0u) {
        const uint32_t cp = cap ? cap[p] : cap_all, l = load[p];
        const uint32_t rm = cp > l ? cp - l : 0u;
        room[p] = rm;
        load[p] = l + (total < rm ? total : rm);
      }
    }
    __syncthreads();
  }
}

// Assign pass of round j.  A workgroup per chunk (grid-stride): the counters start at the chunk's row of the scanned hist, wavefront 0
// walks the chunk.
__global__ __launch_bounds__(kBoundThreads) void bounded_assign_kernel(const int32_t* __restrict__ lists, const double* __restrict__ scores,
                                                                       uint32_t n_reqs, uint32_t k, uint32_t j, uint32_t n_pods, uint32_t chunk,
                                                                       uint32_t n_chunks, const uint32_t* __restrict__ hist,
                                                                       const uint32_t* __restrict__ room, uint8_t* state,
                                                                       int32_t* __restrict__ out_pick, double* __restrict__ out_score) {
  __shared__ uint32_t s_cnt[EPPK_MAX_PODS];
  if (n_pods > EPPK_MAX_PODS) return;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) s_cnt[p] = hist[(size_t)c * n_pods + p];
    __syncthreads();
    const uint64_t r0 = (uint64_t)c * chunk, r1 = r0 + chunk < n_reqs ? r0 + chunk : n_reqs;
    if (threadIdx.x < 64u) bounded_wave_round(lists, scores, k, j, r0, r1, n_pods, s_cnt, BoundRoomArray{room}, state, out_pick, out_score);
    __syncthreads();
  }
}

// After the last round: a thread per request (grid-stride).
__global__ __launch_bounds__(kBoundThreads) void bounded_finish_kernel(const int32_t* __restrict__ lists, const double* __restrict__ scores,
                                                                       uint32_t n_reqs, uint32_t k, uint32_t n_pods, uint32_t policy,
                                                                       uint32_t* __restrict__ load, uint8_t* state, int32_t* __restrict__ out_pick,
                                                                       double* __restrict__ out_score, uint32_t* __restrict__ status) {
  for (uint64_t r = (uint64_t)blockIdx.x * kBoundThreads + threadIdx.x; r < n_reqs; r += (uint64_t)gridDim.x * kBoundThreads) {
    const int32_t spill = bounded_finish_row(lists, scores, k, r, n_pods, policy, state, out_pick, out_score, status);
    if (spill != EPPK_NO_PICK) atomicAdd(&load[spill], 1u);            // (a count, modulo 2^32: the result of the add is not read)
  }
}

}  // namespace eppk
#endif
