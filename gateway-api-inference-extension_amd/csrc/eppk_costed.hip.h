// eppk_costed.hip.h — cost-weighted caps for the bounded and banded pickers (SEMANTICS.md §3f; include/eppk.h eppk_costed_resolve_device).
//
// Included by eppk.hip alone, behind eppk_banded.hip.h.  The band order (banded_hist_kernel, banded_offsets_kernel,
// banded_scatter_kernel) is reused as it is: it does not depend on cost.  Everything else is repeated here, not shared: no kernel of
// eppk_bounded.hip.h or eppk_banded.hip.h may move by an instruction.
//
// Every request carries a cost c (1 .. EPPK_MAX_COST), per request or per list entry; cap, load and reserve are in the same units.  In
// round j of band b a request whose entry j is pod p is a BIDDER iff c <= room[p]; its place among the bidders of p is
//     S = (costs of p's bidders in the CHUNKS in front of the request's chunk)       costed_scan_kernel: exclusive prefix over chunks
//       + (costs of p's bidders in front of the request INSIDE its chunk)            costed_wave_round: one wavefront walks the chunk
// and it gets p iff S + c <= room[p].  S comes from the request's index alone: no atomic's return value is read anywhere.
//
// Exactness.  Inside a 64-row trip a sum is below 64 * 2^24 = 2^30 and is carried exactly in 32 bits.  Everything longer -- the carried
// counter of a chunk, a chunk's total, the prefix over the chunks -- SATURATES at 2^32 - 1: since c >= 1 and room <= 2^32 - 1, a
// saturated S can never satisfy S + c <= room, so saturation decides as the exact sum would; and min(sum of min(x, M), M) = min(sum x, M),
// so saturated pieces add up to the saturated whole.  A chunk's total is built with 64-bit LDS adds (a 32-bit histogram could wrap:
// 512 rows carry 2^33) and clamped when it is written.
//
// The load a round leaves is the TAKERS' total, which no prefix of bidders' sums knows.  The assign pass adds it to acc[pod] -- one add
// per pod and trip, by the trip's last taker, result not read, so the order of the adds does not show -- and nobody reads acc[] as room
// while an assign pass runs: the count pass of the next round takes room from cap, load + acc (all stable while it runs), the scan pass
// folds acc into load and writes the room the assign pass reads.  The finish folds what the last round left.
//
//   batch <= chunk    costed_resolve_one_kernel: one workgroup, one launch; load, carried counters and takers' totals in LDS.
//   batch >  chunk    the band order, then per band b and round j costed_count_kernel / costed_scan_kernel / costed_assign_kernel over
//                     places [seg[b], seg[b+1]) read on the device, then costed_finish_kernel, a thread per request.
// A bad row (cost outside 1 .. EPPK_MAX_COST -- per entry: at a position whose entry is a valid pod -- or band byte >= n_bands) is marked
// kCostBad when its band's first round meets it, bids nowhere, and ends as EPPK_NO_PICK / 0.0 / EPPK_RANK_NONE with
// EPPK_LAUNCH_BAD_REQUEST_ROW raised; its list is still checked.
#ifndef EPPK_COSTED_HIP_H
#define EPPK_COSTED_HIP_H

#include "eppk_banded.hip.h"

namespace eppk {

constexpr uint32_t kCostBad = 0xFCu;       // state of a request whose cost is out of range (no rank has this value)
constexpr uint32_t kCostSat = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t cost_sat_add(uint32_t a, uint32_t b) { const uint32_t s = a + b; return s < a ? kCostSat : s; }
__device__ __forceinline__ uint32_t cost_clamp(uint64_t v) { return v > (uint64_t)kCostSat ? kCostSat : (uint32_t)v; }
__device__ __forceinline__ bool cost_ok(uint32_t c) { return c - 1u < EPPK_MAX_COST; }     // (0 - 1 is huge)

// The cost of request r at list position j.
struct CostOf {
  const uint32_t* cost; uint32_t k, per_entry;
  __device__ __forceinline__ uint32_t operator()(uint64_t r, uint32_t j) const { return cost[per_entry ? r * k + j : r]; }
};

// A cost out of range: per request the row's one cost; per entry only where the list entry is a valid pod.
__device__ __forceinline__ bool costed_row_bad(const int32_t* __restrict__ lists, uint32_t k, uint64_t r, uint32_t n_pods, const CostOf cost) {
  if (!cost.per_entry) return !cost_ok(cost(r, 0u));
  bool bad = false;
  for (uint32_t i = 0; i < k; ++i)
    if (bounded_valid(lists[r * k + i], n_pods) && !cost_ok(cost(r, i))) bad = true;
  return bad;
}

// Room of pod p for a band from the caps and loads in global memory, with what the assign pass of the round before added to acc[].
struct CostRoomGlobal {
  const uint32_t* cap; uint32_t cap_all, reserve; const uint32_t* load; const uint32_t* acc;
  __device__ __forceinline__ uint32_t operator()(uint32_t p) const {
    const uint32_t cf = cap ? cap[p] : cap_all, c = cf - (cf < reserve ? cf : reserve), l = load[p] + acc[p];
    return c > l ? c - l : 0u;
  }
};

// Where the takers' total of a pod and trip goes: LDS in the one-launch kernel (one wavefront writes it), acc[] in the assign pass.
struct CostAccLds {
  uint32_t* take;
  __device__ __forceinline__ void operator()(uint32_t p, uint32_t v) const { take[p] += v; }
};
struct CostAccGlobal {
  uint32_t* acc;
  __device__ __forceinline__ void operator()(uint32_t p, uint32_t v) const { atomicAdd(&acc[p], v); }   // (the result of the add is not read)
};

// ONE wavefront takes places [r0, r1) through round j, 64 per trip in ascending order; place i holds request row(i).  cnt[] (LDS, one
// saturating counter per pod) holds, for every pod, the costs of this round's bidders in front of the place the wavefront is at.  Within
// a trip the lanes that bid for one pod find each other by ballot (one trip of the loop per distinct pod: wave-uniform); a lane's S is the
// counter plus the exclusive prefix sum of the costs of the lanes below it that bid for the same pod -- a masked wavefront scan where
// bounded_wave_round has a popcount; a pod with one bidder in the trip needs none.  A lane decides for itself, before the loop, whether it
// is a bidder (c <= room of its pod): a request that could not fit alone never enters a ballot.  Every index into cnt[] has passed
// bounded_valid.
template <class Room, class Acc, class Row>
__device__ __forceinline__ void costed_wave_round(const int32_t* __restrict__ lists, const double* __restrict__ scores, uint32_t k, uint32_t j,
                                                  uint64_t r0, uint64_t r1, uint32_t n_pods, const CostOf cost, uint32_t* cnt, const Room room,
                                                  const Acc acc, uint8_t* state, int32_t* __restrict__ out_pick, double* __restrict__ out_score,
                                                  const Row row) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t t0 = r0; t0 < r1; t0 += 64u) {
    uint64_t r = t0 + lane;
    int32_t e = EPPK_NO_PICK;
    uint32_t c = 0u, rm = 0u;
    bool bid = false;
    if (r < r1) {
      r = row(r);
      if (state[r] == kBoundUnassigned) {
        e = lists[r * k + j];
        if (bounded_valid(e, n_pods)) {
          c = cost(r, j);
          rm = room((uint32_t)e);                                     // (a gather, outside the ballot loop: the room stays for the length of the round)
          bid = c <= rm;                                              // could fit alone: a bidder (§3f); the others count for nothing
        }
      }
    }
    bool take = false;
    for (uint64_t todo = __ballot(bid); todo != 0ull;) {            // (wave-uniform: one trip of this loop per distinct pod)
      const int32_t p0 = __shfl(e, (int)__builtin_ctzll(todo));
      const bool mine = bid && e == p0;
      const uint64_t m = __ballot(mine);
      const uint32_t before = cnt[p0];                              // (every lane reads the same word: a broadcast)
      const uint32_t v = mine ? c : 0u;
      uint32_t incl = v;                                            // inclusive prefix over the lanes: < 64 * 2^24, exact in 32 bits
      if ((m & (m - 1ull)) != 0ull) {                               // (uniform: more than one bidder in this trip)
#pragma unroll
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
          const uint32_t up = __shfl_up(incl, d);
          if (lane >= d) incl += up;
        }
      }
      const int hi = 63 - (int)__builtin_clzll(m);                  // the last bidder: its inclusive prefix is the trip's total
      const uint32_t total = __shfl(incl, hi);
      if (mine) take = (uint64_t)before + (uint64_t)incl <= (uint64_t)rm;        // S + c <= room, S = before + (incl - c)
      const uint64_t tm = __ballot(mine && take);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if ((int)lane == hi) cnt[p0] = cost_sat_add(before, total);
      if (tm != 0ull && (int)lane == 63 - (int)__builtin_clzll(tm)) acc((uint32_t)p0, incl);     // the takers are a prefix: the last one's incl is their total
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

// What is left of request r behind the last band, and the check of its band byte, its cost(s) and every entry of its list.  Returns the
// pod that takes a spilled request, else EPPK_NO_PICK; *spill_cost: what the spill adds to that pod's load.
__device__ __forceinline__ int32_t costed_finish_row(const int32_t* __restrict__ lists, const double* __restrict__ scores, uint32_t k, uint64_t r,
                                                     uint32_t n_pods, const CostOf cost, const uint8_t* __restrict__ band, uint32_t n_bands,
                                                     uint32_t spill, uint8_t* state, int32_t* __restrict__ out_pick, double* __restrict__ out_score,
                                                     uint32_t* __restrict__ status, uint32_t* spill_cost) {
  const uint32_t b = band_of(band, r), st = state[r];
  uint32_t first = k;
  bool bad_pick = false, bad_row = b >= n_bands;
  for (uint32_t i = 0; i < k; ++i) {
    const int32_t e = lists[r * k + i];
    if (bounded_valid(e, n_pods)) {
      if (first == k) first = i;
      if (cost.per_entry && !cost_ok(cost(r, i))) bad_row = true;
    } else if (e != EPPK_NO_PICK) bad_pick = true;
  }
  if (!cost.per_entry && !cost_ok(cost(r, 0u))) bad_row = true;
  if (bad_pick) atomicOr(status, EPPK_LAUNCH_BAD_PICK);
  int32_t pick = EPPK_NO_PICK;
  double score = 0.0;
  uint32_t rank = EPPK_RANK_NONE;
  if (bad_row) atomicOr(status, EPPK_LAUNCH_BAD_REQUEST_ROW);      // in no band, or no usable cost: nothing bid for it
  else {
    if (st != kBoundUnassigned && st != kBandLeft && st != kBandWaits) return EPPK_NO_PICK;   // (placed by a round: pick, score and rank are written)
    if (first != k) {
      rank = EPPK_RANK_OVERFLOW;
      if (band_policy(spill, b) == EPPK_BOUNDED_SPILL) {
        pick = lists[r * k + first];
        score = scores ? scores[r * k + first] : 0.0;
        rank |= first;
        *spill_cost = cost(r, first);
      }
    }
  }
  out_pick[r] = pick;
  if (out_score) out_score[r] = score;
  state[r] = (uint8_t)rank;
  return pick;
}

// batch <= chunk: one workgroup.  Per band: wavefront 0 walks all rows (only the band's rows are kBoundUnassigned), all four wavefronts
// take the passes over the pods.  A band without rows is skipped.
__global__ __launch_bounds__(kBoundThreads) void costed_resolve_one_kernel(const int32_t* __restrict__ lists, const double* __restrict__ scores,
                                                                           uint32_t n_reqs, uint32_t k, uint32_t n_pods, const CostOf cost,
                                                                           const uint8_t* __restrict__ band, const BandTab tab,
                                                                           const uint32_t* __restrict__ cap, uint32_t cap_all, uint32_t* load,
                                                                           int32_t* __restrict__ out_pick, double* __restrict__ out_score,
                                                                           uint8_t* state, uint32_t* __restrict__ status) {
  __shared__ uint32_t s_cnt[EPPK_MAX_PODS], s_load[EPPK_MAX_PODS], s_take[EPPK_MAX_PODS];
  if (n_pods > EPPK_MAX_PODS) return;
  for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) { s_cnt[p] = 0u; s_take[p] = 0u; s_load[p] = load ? load[p] : 0u; }
  for (uint32_t r = threadIdx.x; r < n_reqs; r += kBoundThreads) state[r] = (uint8_t)kBandWaits;
  __syncthreads();
  for (uint32_t b = 0; b < tab.n_bands; ++b) {
    int rows = 0;
    for (uint32_t r = threadIdx.x; r < n_reqs; r += kBoundThreads) {  // (a thread meets the rows it set itself)
      if (band_of(band, r) == b) {
        if (costed_row_bad(lists, k, r, n_pods, cost)) state[r] = (uint8_t)kCostBad;
        else { state[r] = (uint8_t)kBoundUnassigned; rows = 1; }
      } else if (state[r] == kBoundUnassigned) state[r] = (uint8_t)kBandLeft;
    }
    if (!__syncthreads_or(rows)) continue;                            // (uniform over the workgroup)
    const BandRoomLds room{cap, cap_all, band_reserve(tab, b), s_load};
    for (uint32_t j = 0; j < k; ++j) {
      if (threadIdx.x < 64u)
        costed_wave_round(lists, scores, k, j, 0ull, (uint64_t)n_reqs, n_pods, cost, s_cnt, room, CostAccLds{s_take}, state, out_pick, out_score,
                          BoundRowSelf{});
      __syncthreads();
      for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) {  // the loads the next round sees; the counters start over
        if (s_cnt[p]) { s_load[p] += s_take[p]; s_take[p] = 0u; s_cnt[p] = 0u; }
      }
      __syncthreads();
    }
  }
  for (uint32_t r = threadIdx.x; r < n_reqs; r += kBoundThreads) {
    uint32_t sc = 0u;
    const int32_t to = costed_finish_row(lists, scores, k, r, n_pods, cost, band, tab.n_bands, tab.spill, state, out_pick, out_score, status, &sc);
    if (to != EPPK_NO_PICK) atomicAdd(&s_load[to], sc);                // (modulo 2^32: the result of the add is not read)
  }
  __syncthreads();
  if (load) for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) load[p] = s_load[p];
}

// ---- band b, round j over places [seg[b], seg[b + 1]) of the band order ------------------------------------------------------

// Count pass.  A workgroup per chunk (grid-stride), a thread per row: the costs of the chunk's bidders per pod, summed in 64 bits in
// LDS, then row `chunk` of hist, clamped to 32 bits.  Round 0 of a band meets every row of the band once: it marks the bad ones.
__global__ __launch_bounds__(kBoundThreads) void costed_count_kernel(const int32_t* __restrict__ lists, uint32_t k, uint32_t j, uint32_t n_pods,
                                                                     uint32_t chunk, const uint32_t* __restrict__ seg, uint32_t b,
                                                                     const uint32_t* __restrict__ perm, const CostOf cost, const CostRoomGlobal room,
                                                                     uint8_t* state, uint32_t* __restrict__ hist) {
  __shared__ unsigned long long s_sum[EPPK_MAX_PODS];
  if (n_pods > EPPK_MAX_PODS) return;
  const BandRange g = band_range(seg, b, chunk);
  for (uint32_t c = blockIdx.x; c < g.n_chunks; c += gridDim.x) {
    for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) s_sum[p] = 0ull;
    __syncthreads();
    const uint64_t i0 = g.s0 + (uint64_t)c * chunk, i1 = i0 + chunk < g.s1 ? i0 + chunk : g.s1;
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += kBoundThreads) {
      const uint64_t r = perm[i];
      uint32_t st = state[r];
      if (j == 0u && costed_row_bad(lists, k, r, n_pods, cost)) { st = kCostBad; state[r] = (uint8_t)kCostBad; }
      if (st == kBoundUnassigned) {
        const int32_t e = lists[r * k + j];
        if (bounded_valid(e, n_pods)) {
          const uint32_t cr = cost(r, j);
          if (cr <= room((uint32_t)e)) atomicAdd(&s_sum[e], (unsigned long long)cr);   // (an exact 64-bit sum: the result of the add is not read)
        }
      }
    }
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) hist[(size_t)c * n_pods + p] = cost_clamp(s_sum[p]);
    __syncthreads();
  }
}

// Scan pass: banded_scan_kernel's cut of the chunks with 64-bit running sums, clamped when written.  Per pod it also folds what the
// assign pass of the round before added to acc[] into the load, and writes the room this round's assign pass reads.
__global__ __launch_bounds__(kBoundScanSegs * kBoundScanPods) void costed_scan_kernel(uint32_t* hist, uint32_t chunk, const uint32_t* __restrict__ seg,
                                                                                     uint32_t b, uint32_t n_pods, const uint32_t* __restrict__ cap,
                                                                                     uint32_t cap_all, uint32_t reserve, uint32_t* __restrict__ load,
                                                                                     uint32_t* __restrict__ acc, uint32_t* __restrict__ room) {
  const BandRange g = band_range(seg, b, chunk);
  const uint32_t n_chunks = g.n_chunks;
  if (n_chunks == 0u) return;                                         // nobody bids: acc[] waits for the next fold, and no assign pass reads room
  __shared__ uint64_t s_sum[kBoundScanSegs][kBoundScanPods];
  const uint32_t lp = threadIdx.x % kBoundScanPods, sg = threadIdx.x / kBoundScanPods;
  const uint32_t seg_len = (n_chunks + kBoundScanSegs - 1u) / kBoundScanSegs;
  const uint32_t c0 = sg * seg_len < n_chunks ? sg * seg_len : n_chunks, c1 = c0 + seg_len < n_chunks ? c0 + seg_len : n_chunks;
  for (uint32_t pb = blockIdx.x * kBoundScanPods; pb < n_pods; pb += gridDim.x * kBoundScanPods) {     // (uniform over the workgroup)
    const uint32_t p = pb + lp;
    const bool live = p < n_pods;
    uint64_t sum = 0ull;
    if (live) {
#pragma unroll 8
      for (uint32_t c = c0; c < c1; ++c) sum += hist[(size_t)c * n_pods + p];
    }
    s_sum[sg][lp] = sum;
    __syncthreads();
    uint64_t run = 0ull;
    for (uint32_t s2 = 0; s2 < kBoundScanSegs; ++s2) {
      const uint64_t v = s_sum[s2][lp];
      if (s2 < sg) run += v;
    }
    if (live) {
      for (uint32_t c = c0; c < c1; c += 8u) {                     // eight loads in flight, then their prefix
        uint32_t v[8];
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) v[i] = c + i < c1 ? hist[(size_t)(c + i) * n_pods + p] : 0u;
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i)
          if (c + i < c1) { hist[(size_t)(c + i) * n_pods + p] = cost_clamp(run); run += v[i]; }
      }
      if (sg == 0u) {
        const uint32_t cf = cap ? cap[p] : cap_all, cp = cf - (cf < reserve ? cf : reserve), l = load[p] + acc[p];
        load[p] = l;
        acc[p] = 0u;
        room[p] = cp > l ? cp - l : 0u;
      }
    }
    __syncthreads();
  }
}

// Assign pass.  A workgroup per chunk (grid-stride): the counters start at the chunk's row of the scanned hist, wavefront 0 walks the
// chunk; the takers' totals go to acc[], which nobody reads before the next launch.
__global__ __launch_bounds__(kBoundThreads) void costed_assign_kernel(const int32_t* __restrict__ lists, const double* __restrict__ scores, uint32_t k,
                                                                      uint32_t j, uint32_t n_pods, uint32_t chunk, const uint32_t* __restrict__ seg,
                                                                      uint32_t b, const uint32_t* __restrict__ perm, const CostOf cost,
                                                                      const uint32_t* __restrict__ hist, const uint32_t* __restrict__ room,
                                                                      uint32_t* __restrict__ acc, uint8_t* state, int32_t* __restrict__ out_pick,
                                                                      double* __restrict__ out_score) {
  __shared__ uint32_t s_cnt[EPPK_MAX_PODS];
  if (n_pods > EPPK_MAX_PODS) return;
  const BandRange g = band_range(seg, b, chunk);
  for (uint32_t c = blockIdx.x; c < g.n_chunks; c += gridDim.x) {
    for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) s_cnt[p] = hist[(size_t)c * n_pods + p];
    __syncthreads();
    const uint64_t i0 = g.s0 + (uint64_t)c * chunk, i1 = i0 + chunk < g.s1 ? i0 + chunk : g.s1;
    if (threadIdx.x < 64u)
      costed_wave_round(lists, scores, k, j, i0, i1, n_pods, cost, s_cnt, BoundRoomArray{room}, CostAccGlobal{acc}, state, out_pick, out_score,
                        BandRowPerm{perm});
    __syncthreads();
  }
}

// Behind the last band: a thread per request (grid-stride), in batch order; the first n_pods threads also fold what the last round
// left in acc[] into the load.  All adds to load[] commute modulo 2^32 and none is read.
__global__ __launch_bounds__(kBoundThreads) void costed_finish_kernel(const int32_t* __restrict__ lists, const double* __restrict__ scores,
                                                                      uint32_t n_reqs, uint32_t k, uint32_t n_pods, const CostOf cost,
                                                                      const uint8_t* __restrict__ band, uint32_t n_bands, uint32_t spill,
                                                                      uint32_t* __restrict__ load, const uint32_t* __restrict__ acc, uint8_t* state,
                                                                      int32_t* __restrict__ out_pick, double* __restrict__ out_score,
                                                                      uint32_t* __restrict__ status) {
  for (uint64_t p = (uint64_t)blockIdx.x * kBoundThreads + threadIdx.x; p < n_pods; p += (uint64_t)gridDim.x * kBoundThreads) {
    const uint32_t a = acc[p];
    if (a) atomicAdd(&load[p], a);
  }
  for (uint64_t r = (uint64_t)blockIdx.x * kBoundThreads + threadIdx.x; r < n_reqs; r += (uint64_t)gridDim.x * kBoundThreads) {
    uint32_t sc = 0u;
    const int32_t to = costed_finish_row(lists, scores, k, r, n_pods, cost, band, n_bands, spill, state, out_pick, out_score, status, &sc);
    if (to != EPPK_NO_PICK) atomicAdd(&load[to], sc);                  // (modulo 2^32: the result of the add is not read)
  }
}

}  // namespace eppk
#endif
