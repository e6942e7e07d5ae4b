// eppk_banded.hip.h — priority bands over the bounded picker (SEMANTICS.md §3e; include/eppk.h eppk_banded_resolve_device).
//
// Included by eppk.hip alone, behind eppk_bounded.hip.h, whose bounded_wave_round and bounded_finish_row do the work.
//
// Every request carries a band byte; band 0 is the most important.  The bands go through the whole of §3d one after the other: band b's
// requests, in batch order, take their k rounds under cap_b[p] = cap[p] - min(cap[p], reserve_b) on the loads band b-1 left.  What no
// round placed is finished ONCE, behind the last band, with the policy of the request's own band (§3e: a request left unassigned has
// its first valid entry on a pod its own band filled to cap_b, and no later band has room there, so the deferred finish changes no pick).
// As in §3d no atomic's return value is read anywhere: a request's place comes from its index alone.
//
//   batch <= chunk    banded_resolve_one_kernel: one workgroup, one launch.  The bands take turns through the state byte: a request that
//                     waits for its band is kBandWaits, one its band's rounds did not place is kBandLeft, and only kBoundUnassigned bids.
//   batch >  chunk    the rows are put in band order first, stable in batch order, as a permutation (the lists are not copied):
//                       banded_hist_kernel     per chunk, the number of rows of every band                      -> bh[chunk][8]
//                       banded_offsets_kernel  bh := where the chunk's rows of the band start in the order; seg[b] = where band b starts
//                       banded_scatter_kernel  per chunk, one wavefront: place = offset + rows of the band below the lane -> perm[place] = row
//                     then per band b and round j the count / scan / assign passes of §3d over places [seg[b], seg[b+1]) -- read on the
//                     device, so that the *_device form needs no host sync to learn the band sizes; chunks count from seg[b]; a workgroup
//                     past the segment's last chunk exits -- and banded_finish_kernel, a thread per request.
// A band byte >= n_bands: the request is in no band's segment, takes no room, and ends as EPPK_NO_PICK / 0.0 / EPPK_RANK_NONE with
// EPPK_LAUNCH_BAD_REQUEST_ROW raised; its list is still checked.
#ifndef EPPK_BANDED_HIP_H
#define EPPK_BANDED_HIP_H

#include "eppk_bounded.hip.h"

namespace eppk {

constexpr uint32_t kBandWaits = 0xFEu;     // state of a request whose band has not had its rounds yet (no rank has this value)
constexpr uint32_t kBandLeft = 0xFDu;      // ... whose band's rounds did not place it: it bids no more and waits for the finish
constexpr uint32_t kBandSegWords = 16u;    // seg[0 .. EPPK_MAX_BANDS] in front of the band histogram, padded

// The band table as the kernels take it: bit b of `spill` = policy_b is EPPK_BOUNDED_SPILL.
struct BandTab { uint32_t n_bands, spill; uint32_t reserve[EPPK_MAX_BANDS]; };

// reserve[b] without a dynamic index into the kernel's arguments
__device__ __forceinline__ uint32_t band_reserve(const BandTab& t, uint32_t b) {
  uint32_t v = 0u;
#pragma unroll
  for (uint32_t i = 0; i < EPPK_MAX_BANDS; ++i) if (i == b) v = t.reserve[i];
  return v;
}
__device__ __forceinline__ uint32_t band_policy(uint32_t spill, uint32_t b) { return (spill >> b) & 1u ? EPPK_BOUNDED_SPILL : EPPK_BOUNDED_SHED; }
__device__ __forceinline__ uint32_t band_of(const uint8_t* __restrict__ band, uint64_t r) { return band ? (uint32_t)band[r] : 0u; }

// Room of pod p for a band in the one-launch kernel (BoundRoomLds with the band's reserve).
struct BandRoomLds {
  const uint32_t* cap; uint32_t cap_all, reserve; const uint32_t* load;
  __device__ __forceinline__ uint32_t operator()(uint32_t p) const {
    const uint32_t cf = cap ? cap[p] : cap_all, c = cf - (cf < reserve ? cf : reserve), l = load[p];
    return c > l ? c - l : 0u;
  }
};
// Place i of the band order holds request perm[i].
struct BandRowPerm {
  const uint32_t* perm;
  __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return perm[i]; }
};

// What is left of request r behind the last band; returns the pod that takes a spilled request, else EPPK_NO_PICK.
__device__ __forceinline__ int32_t banded_finish_row(const int32_t* __restrict__ lists, const double* __restrict__ scores, uint32_t k, uint64_t r,
                                                     uint32_t n_pods, const uint8_t* __restrict__ band, uint32_t n_bands, uint32_t spill,
                                                     uint8_t* state, int32_t* __restrict__ out_pick, double* __restrict__ out_score,
                                                     uint32_t* __restrict__ status) {
  const uint32_t b = band_of(band, r), st = state[r];
  if (b >= n_bands) {                                                // in no band: nothing bid for it; SHED writes NO_PICK / 0.0 and checks the list
    state[r] = (uint8_t)kBoundUnassigned;
    (void)bounded_finish_row(lists, scores, k, r, n_pods, EPPK_BOUNDED_SHED, state, out_pick, out_score, status);
    state[r] = (uint8_t)EPPK_RANK_NONE;
    atomicOr(status, EPPK_LAUNCH_BAD_REQUEST_ROW);
    return EPPK_NO_PICK;
  }
  if (st == kBandLeft || st == kBandWaits) state[r] = (uint8_t)kBoundUnassigned;
  return bounded_finish_row(lists, scores, k, r, n_pods, band_policy(spill, b), state, out_pick, out_score, status);
}

// batch <= chunk: one workgroup.  Per band: wavefront 0 walks all rows (only the band's rows are kBoundUnassigned), all four wavefronts
// take the passes over the pods.  A band without rows is skipped.
__global__ __launch_bounds__(kBoundThreads) void banded_resolve_one_kernel(const int32_t* __restrict__ lists, const double* __restrict__ scores,
                                                                           uint32_t n_reqs, uint32_t k, uint32_t n_pods,
                                                                           const uint8_t* __restrict__ band, const BandTab tab,
                                                                           const uint32_t* __restrict__ cap, uint32_t cap_all, uint32_t* load,
                                                                           int32_t* __restrict__ out_pick, double* __restrict__ out_score,
                                                                           uint8_t* state, uint32_t* __restrict__ status) {
  __shared__ uint32_t s_cnt[EPPK_MAX_PODS], s_load[EPPK_MAX_PODS];
  if (n_pods > EPPK_MAX_PODS) return;
  for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) { s_cnt[p] = 0u; s_load[p] = load ? load[p] : 0u; }
  for (uint32_t r = threadIdx.x; r < n_reqs; r += kBoundThreads) state[r] = (uint8_t)kBandWaits;
  __syncthreads();
  for (uint32_t b = 0; b < tab.n_bands; ++b) {
    int rows = 0;
    for (uint32_t r = threadIdx.x; r < n_reqs; r += kBoundThreads) {  // (a thread meets the rows it set itself)
      if (band_of(band, r) == b) { state[r] = (uint8_t)kBoundUnassigned; rows = 1; }
      else if (state[r] == kBoundUnassigned) state[r] = (uint8_t)kBandLeft;
    }
    if (!__syncthreads_or(rows)) continue;                            // (uniform over the workgroup)
    const BandRoomLds room{cap, cap_all, band_reserve(tab, b), s_load};
    for (uint32_t j = 0; j < k; ++j) {
      if (threadIdx.x < 64u) bounded_wave_round(lists, scores, k, j, 0ull, (uint64_t)n_reqs, n_pods, s_cnt, room, state, out_pick, out_score);
      __syncthreads();
      for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) {  // the loads the next round sees; the counters start over
        const uint32_t bids = s_cnt[p];
        if (bids) {
          const uint32_t rm = room(p);
          s_load[p] += bids < rm ? bids : rm;
          s_cnt[p] = 0u;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t r = threadIdx.x; r < n_reqs; r += kBoundThreads) {
    const int32_t spill = banded_finish_row(lists, scores, k, r, n_pods, band, tab.n_bands, tab.spill, state, out_pick, out_score, status);
    if (spill != EPPK_NO_PICK) atomicAdd(&s_load[spill], 1u);          // (a count: the result of the add is not read)
  }
  __syncthreads();
  if (load) for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) load[p] = s_load[p];
}

// ---- the band order ---------------------------------------------------------------------------------------------------------

// A workgroup per chunk (grid-stride): the chunk's rows per band, row `chunk` of bh.  A band byte >= n_bands is counted nowhere.
__global__ __launch_bounds__(kBoundThreads) void banded_hist_kernel(const uint8_t* __restrict__ band, uint32_t n_reqs, uint32_t n_bands, uint32_t chunk,
                                                                    uint32_t n_chunks, uint32_t* __restrict__ bh) {
  __shared__ uint32_t s_h[EPPK_MAX_BANDS];
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    if (threadIdx.x < EPPK_MAX_BANDS) s_h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t r0 = (uint64_t)c * chunk, r1 = r0 + chunk < n_reqs ? r0 + chunk : n_reqs;
    for (uint64_t r = r0 + threadIdx.x; r < r1; r += kBoundThreads) {
      const uint32_t b = band_of(band, r);
      if (b < n_bands) atomicAdd(&s_h[b], 1u);                        // (a count: the result of the add is not read)
    }
    __syncthreads();
    if (threadIdx.x < EPPK_MAX_BANDS) bh[(size_t)c * EPPK_MAX_BANDS + threadIdx.x] = s_h[threadIdx.x];
    __syncthreads();
  }
}

// ONE workgroup: bh[c][b] := seg[b] + (rows of band b in the chunks in front of c); seg[b] = rows of the bands in front of b, seg[8] = all
// rows that are in a band.  A thread per (chunk segment, band), as bounded_scan_kernel cuts its columns.
constexpr uint32_t kBandScanSegs = kBoundThreads / EPPK_MAX_BANDS;
__global__ __launch_bounds__(kBoundThreads) void banded_offsets_kernel(uint32_t* bh, uint32_t n_chunks, uint32_t* __restrict__ seg) {
  __shared__ uint32_t s_sum[kBandScanSegs][EPPK_MAX_BANDS], s_tot[EPPK_MAX_BANDS];
  const uint32_t b = threadIdx.x % EPPK_MAX_BANDS, sg = threadIdx.x / EPPK_MAX_BANDS;
  const uint32_t seg_len = (n_chunks + kBandScanSegs - 1u) / kBandScanSegs;
  const uint32_t c0 = sg * seg_len < n_chunks ? sg * seg_len : n_chunks, c1 = c0 + seg_len < n_chunks ? c0 + seg_len : n_chunks;
  uint32_t sum = 0u;
  for (uint32_t c = c0; c < c1; ++c) sum += bh[(size_t)c * EPPK_MAX_BANDS + b];
  s_sum[sg][b] = sum;
  __syncthreads();
  uint32_t run = 0u, total = 0u;
  for (uint32_t s2 = 0; s2 < kBandScanSegs; ++s2) {
    const uint32_t v = s_sum[s2][b];
    if (s2 < sg) run += v;
    total += v;
  }
  if (sg == 0u) s_tot[b] = total;
  __syncthreads();
  uint32_t base = 0u;
  for (uint32_t b2 = 0; b2 < EPPK_MAX_BANDS; ++b2) if (b2 < b) base += s_tot[b2];
  run += base;
  for (uint32_t c = c0; c < c1; ++c) {
    const uint32_t v = bh[(size_t)c * EPPK_MAX_BANDS + b];
    bh[(size_t)c * EPPK_MAX_BANDS + b] = run;
    run += v;
  }
  if (sg == 0u) {
    seg[b] = base;
    if (b == EPPK_MAX_BANDS - 1u) seg[EPPK_MAX_BANDS] = base + total;
  }
}

// A workgroup of ONE wavefront per chunk (grid-stride): 64 rows per trip in ascending order; a row's place is the band's offset plus the
// rows of its band in the lanes below it, and the offsets are carried from trip to trip.  Stable: batch order inside every band.
// Every place is < seg[8] <= n_reqs, the size of perm (checked all the same: the band bytes are the caller's memory).
__global__ __launch_bounds__(64) void banded_scatter_kernel(const uint8_t* __restrict__ band, uint32_t n_reqs, uint32_t n_bands, uint32_t chunk,
                                                            uint32_t n_chunks, const uint32_t* __restrict__ bh, uint32_t* __restrict__ perm) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    uint32_t off[EPPK_MAX_BANDS];
#pragma unroll
    for (uint32_t b = 0; b < EPPK_MAX_BANDS; ++b) off[b] = bh[(size_t)c * EPPK_MAX_BANDS + b];
    const uint64_t r0 = (uint64_t)c * chunk, r1 = r0 + chunk < n_reqs ? r0 + chunk : n_reqs;
    for (uint64_t t0 = r0; t0 < r1; t0 += 64u) {
      const uint64_t r = t0 + lane;
      const uint32_t mine = r < r1 ? band_of(band, r) : EPPK_MAX_BANDS;
#pragma unroll
      for (uint32_t b = 0; b < EPPK_MAX_BANDS; ++b) {
        const bool in = mine == b && b < n_bands;
        const uint64_t m = __ballot(in);
        const uint32_t place = off[b] + (uint32_t)__popcll(m & below);
        if (in && place < n_reqs) perm[place] = (uint32_t)r;
        off[b] += (uint32_t)__popcll(m);
      }
    }
  }
}

// ---- band b, round j: the passes of §3d over places [seg[b], seg[b + 1]) of the band order ------------------------------------

struct BandRange { uint32_t s0, s1, n_chunks; };
__device__ __forceinline__ BandRange band_range(const uint32_t* __restrict__ seg, uint32_t b, uint32_t chunk) {
  const uint32_t s0 = seg[b], s1 = seg[b + 1u];                       // (b < n_bands <= EPPK_MAX_BANDS: inside seg[0 .. 8])
  return BandRange{s0, s1, (uint32_t)(((uint64_t)(s1 - s0) + chunk - 1u) / chunk)};
}

__global__ __launch_bounds__(kBoundThreads) void banded_count_kernel(const int32_t* __restrict__ lists, uint32_t k, uint32_t j, uint32_t n_pods,
                                                                     uint32_t chunk, const uint32_t* __restrict__ seg, uint32_t b,
                                                                     const uint32_t* __restrict__ perm, const uint8_t* __restrict__ state,
                                                                     uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_cnt[EPPK_MAX_PODS];
  if (n_pods > EPPK_MAX_PODS) return;
  const BandRange g = band_range(seg, b, chunk);
  for (uint32_t c = blockIdx.x; c < g.n_chunks; c += gridDim.x) {
    for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) s_cnt[p] = 0u;
    __syncthreads();
    const uint64_t i0 = g.s0 + (uint64_t)c * chunk, i1 = i0 + chunk < g.s1 ? i0 + chunk : g.s1;
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += kBoundThreads) {
      const uint64_t r = perm[i];
      if (state[r] == kBoundUnassigned) {
        const int32_t e = lists[r * k + j];
        if (bounded_valid(e, n_pods)) atomicAdd(&s_cnt[e], 1u);        // (a count: the result of the add is not read)
      }
    }
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) hist[(size_t)c * n_pods + p] = s_cnt[p];
    __syncthreads();
  }
}

// The scan pass of bounded_scan_kernel over the band's chunks, with the band's reserve taken off the cap.  The body is repeated, not
// shared: through an inlined function bounded_scan_kernel kept its registers but not its instruction order.
__global__ __launch_bounds__(kBoundScanSegs * kBoundScanPods) void banded_scan_kernel(uint32_t* hist, uint32_t chunk, const uint32_t* __restrict__ seg,
                                                                                     uint32_t b, uint32_t n_pods, const uint32_t* __restrict__ cap,
                                                                                     uint32_t cap_all, uint32_t reserve, uint32_t* __restrict__ load,
                                                                                     uint32_t* __restrict__ room) {
  const BandRange g = band_range(seg, b, chunk);
  const uint32_t n_chunks = g.n_chunks;
  if (n_chunks == 0u) return;                                         // nobody bids: the loads stay, and no assign pass reads room
  __shared__ uint32_t s_sum[kBoundScanSegs][kBoundScanPods];
  const uint32_t lp = threadIdx.x % kBoundScanPods, sg = threadIdx.x / kBoundScanPods;
  const uint32_t seg_len = (n_chunks + kBoundScanSegs - 1u) / kBoundScanSegs;
  const uint32_t c0 = sg * seg_len < n_chunks ? sg * seg_len : n_chunks, c1 = c0 + seg_len < n_chunks ? c0 + seg_len : n_chunks;
  for (uint32_t pb = blockIdx.x * kBoundScanPods; pb < n_pods; pb += gridDim.x * kBoundScanPods) {     // (uniform over the workgroup)
    const uint32_t p = pb + lp;
    const bool live = p < n_pods;
    uint32_t sum = 0u;
    if (live) {
#pragma unroll 8
      for (uint32_t c = c0; c < c1; ++c) sum += hist[(size_t)c * n_pods + p];
    }
    s_sum[sg][lp] = sum;
    __syncthreads();
    uint32_t run = 0u, total = 0u;
    for (uint32_t s2 = 0; s2 < kBoundScanSegs; ++s2) {
      const uint32_t v = s_sum[s2][lp];
      if (s2 < sg) run += v;
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
      if (sg == 0u) {
        const uint32_t cf = cap ? cap[p] : cap_all, cp = cf - (cf < reserve ? cf : reserve), l = load[p];
        const uint32_t rm = cp > l ? cp - l : 0u;
        room[p] = rm;
        load[p] = l + (total < rm ? total : rm);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBoundThreads) void banded_assign_kernel(const int32_t* __restrict__ lists, const double* __restrict__ scores, uint32_t k,
                                                                      uint32_t j, uint32_t n_pods, uint32_t chunk, const uint32_t* __restrict__ seg,
                                                                      uint32_t b, const uint32_t* __restrict__ perm,
                                                                      const uint32_t* __restrict__ hist, const uint32_t* __restrict__ room,
                                                                      uint8_t* state, int32_t* __restrict__ out_pick, double* __restrict__ out_score) {
  __shared__ uint32_t s_cnt[EPPK_MAX_PODS];
  if (n_pods > EPPK_MAX_PODS) return;
  const BandRange g = band_range(seg, b, chunk);
  for (uint32_t c = blockIdx.x; c < g.n_chunks; c += gridDim.x) {
    for (uint32_t p = threadIdx.x; p < n_pods; p += kBoundThreads) s_cnt[p] = hist[(size_t)c * n_pods + p];
    __syncthreads();
    const uint64_t i0 = g.s0 + (uint64_t)c * chunk, i1 = i0 + chunk < g.s1 ? i0 + chunk : g.s1;
    if (threadIdx.x < 64u)
      bounded_wave_round(lists, scores, k, j, i0, i1, n_pods, s_cnt, BoundRoomArray{room}, state, out_pick, out_score, BandRowPerm{perm});
    __syncthreads();
  }
}

// Behind the last band: a thread per request (grid-stride), in batch order -- the permutation is not needed any more.
__global__ __launch_bounds__(kBoundThreads) void banded_finish_kernel(const int32_t* __restrict__ lists, const double* __restrict__ scores,
                                                                      uint32_t n_reqs, uint32_t k, uint32_t n_pods, const uint8_t* __restrict__ band,
                                                                      uint32_t n_bands, uint32_t spill, uint32_t* __restrict__ load, uint8_t* state,
                                                                      int32_t* __restrict__ out_pick, double* __restrict__ out_score,
                                                                      uint32_t* __restrict__ status) {
  for (uint64_t r = (uint64_t)blockIdx.x * kBoundThreads + threadIdx.x; r < n_reqs; r += (uint64_t)gridDim.x * kBoundThreads) {
    const int32_t to = banded_finish_row(lists, scores, k, r, n_pods, band, n_bands, spill, state, out_pick, out_score, status);
    if (to != EPPK_NO_PICK) atomicAdd(&load[to], 1u);                  // (a count, modulo 2^32: the result of the add is not read)
  }
}

}  // namespace eppk
#endif
