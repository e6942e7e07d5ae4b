// eppk_wfair.hip.h — weighted fair shares between flows, with turns carried from one batch to the next (SEMANTICS.md §3h; include/eppk.h
// eppk_wfair_resolve_device).
//
// Included by eppk.hip alone, behind eppk_fair.hip.h.  Nothing of eppk_fair.hip.h, eppk_bounded.hip.h, eppk_banded.hip.h or
// eppk_costed.hip.h is edited: fair_offsets_kernel and the count / scan / assign / finish kernels are launched as they are.  The kernels
// here write ANOTHER permutation into the layout those walk (perm, seg[0 .. 8]), a key and an effective band byte per row, and behind the
// finish the turns every (band, flow) has taken.
//
// Every flow has a WEIGHT w (u16; NULL: 1) and every (band, flow) the TURNS t it took in earlier batches (u32; NULL: 0).  A row is IN THE
// ORDER iff band < n_bands, flow < n_flows and w[flow] >= 1; its key is g = band * n_flows + flow, its TURN q the rows in front of it in
// the batch with the same key, its CYCLE c = (t[g] + q) / w[flow] (floor, 64 bits).  Band b's rows are placed by (c, flow, q) ascending:
// in every cycle flow f takes up to w[f] consecutive turns, the flows in flow-id order.  The place needs no sort: with n[f'] the rows of
// (b, f'),
//     place = seg[b] + q + sum over f' != f of clamp((c + [f' < f]) * w[f'] - t[b][f'], 0, n[f'])
// in signed 64 bits (c < 2^33, w < 2^16: the product stays below 2^50).  With every w = 1 and every t = 0 it is eppk_fair.hip.h's form.
//
//   wfair_stage_kernel    the caller's weights and turns -> the context's own memory (NULL: ones, zeros), and taken[] := 0.  A launch of
//                         its own, so that the caller's bytes are read exactly ONCE: every workgroup of every later pass reads the same
//                         copy whatever the caller does to its arrays meanwhile, and the carry adds to the values the order was built from
//   wfair_hist_kernel     fair_hist_kernel plus the weight test for "in the order"
//   fair_offsets_kernel   (eppk_fair.hip.h, as it is)
//   wfair_scatter_kernel  fair_scatter_kernel's structure -- one wavefront per chunk, the ballot loop per distinct key, carried s_run --
//                         with the closed form above: one division per row for its own cycle, a multiply, a subtract and a clamp per
//                         (row, flow)
//   wfair_taken_kernel    behind the finish: per chunk an LDS histogram over the keys of the rows with out_pick != EPPK_NO_PICK (placed and
//                         spilled rows; not shed rows, not rows without a valid entry), added into taken[G]
//   wfair_carry_kernel    turns[g] := min(2^32 - 1, t[g] + taken[g])
// As everywhere in the resolves no atomic's return value is read: every add is a count.
// Not here: turns in cost units (a turn is a request, whatever it costs); a tie-break by arrival instead of flow id; assumed load.
#ifndef EPPK_WFAIR_HIP_H
#define EPPK_WFAIR_HIP_H

#include "eppk_fair.hip.h"

namespace eppk {

// words of the context's own copy (eppk_ctx::d_wf): t[kFairMaxKeys] | taken[kFairMaxKeys] | w[EPPK_MAX_FLOWS], then the areas the
// host-buffer forms upload into: turns[kFairMaxKeys] | weights (u16 [EPPK_MAX_FLOWS], two to a word)
constexpr uint32_t kWfairT = 0u, kWfairTaken = kFairMaxKeys, kWfairW = 2u * kFairMaxKeys, kWfairHostT = kWfairW + EPPK_MAX_FLOWS,
                   kWfairHostW = kWfairHostT + kFairMaxKeys, kWfairWords = kWfairHostW + EPPK_MAX_FLOWS / 2u;
// dynamic LDS of wfair_scatter_kernel: (n, t)[G], run[G], w[n_flows]; 100 KiB at 8 bands x 1 024 flows
constexpr size_t wfair_lds_bytes(size_t G, size_t n_flows) { return (3u * G + n_flows) * sizeof(uint32_t); }
constexpr size_t kWfairMaxLds = wfair_lds_bytes(kFairMaxKeys, EPPK_MAX_FLOWS);

// Grid-stride over the keys: own copies of turns and weights, taken[] zeroed.
__global__ __launch_bounds__(kBoundThreads) void wfair_stage_kernel(const uint16_t* __restrict__ weight, const uint32_t* __restrict__ turns, uint32_t n_bands,
                                                                    uint32_t n_flows, uint32_t* __restrict__ w_own, uint32_t* __restrict__ t_own,
                                                                    uint32_t* __restrict__ taken) {
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  const uint32_t G = n_bands * n_flows;
  for (uint32_t g = blockIdx.x * kBoundThreads + threadIdx.x; g < G; g += gridDim.x * kBoundThreads) {
    t_own[g] = turns ? turns[g] : 0u;
    taken[g] = 0u;
    if (g < n_flows) w_own[g] = weight ? (uint32_t)weight[g] : 1u;
  }
}

// A workgroup per chunk (grid-stride): row `chunk` of fh, and key[] / eband[] of the chunk's rows.  w_own: wfair_stage_kernel's copy.
__global__ __launch_bounds__(kBoundThreads) void wfair_hist_kernel(const uint8_t* __restrict__ band, const uint16_t* __restrict__ flow,
                                                                   const uint32_t* __restrict__ w_own, uint32_t n_reqs, uint32_t n_bands, uint32_t n_flows,
                                                                   uint32_t chunk, uint32_t n_chunks, uint32_t* __restrict__ fh, uint16_t* __restrict__ key,
                                                                   uint8_t* __restrict__ eband) {
  __shared__ uint32_t s_h[kFairMaxKeys];
  const uint32_t G = n_bands * n_flows;
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    for (uint32_t g = threadIdx.x; g < G; g += kBoundThreads) s_h[g] = 0u;
    __syncthreads();
    const uint64_t r0 = (uint64_t)c * chunk, r1 = r0 + chunk < n_reqs ? r0 + chunk : n_reqs;
    for (uint64_t r = r0 + threadIdx.x; r < r1; r += kBoundThreads) {
      const uint32_t b = band_of(band, r), f = flow ? (uint32_t)flow[r] : 0u;
      const bool in = b < n_bands && f < n_flows && w_own[f < n_flows ? f : 0u] >= 1u;
      const uint32_t g = b * n_flows + f;
      key[r] = (uint16_t)(in ? g : kFairNoKey);
      eband[r] = (uint8_t)(in ? b : kFairBadBand);
      if (in) atomicAdd(&s_h[g], 1u);                                 // (a count: the result of the add is not read)
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < G; g += kBoundThreads) fh[(size_t)c * G + g] = s_h[g];
    __syncthreads();
  }
}

// A workgroup of ONE wavefront per chunk (grid-stride), with 3 * G + n_flows words of dynamic LDS (wfair_lds_bytes): s_nt, for every key
// its rows and its carried turns side by side (one 8-byte read per (row, flow)); s_run, for every key the rows in front of the place the
// wavefront is at; s_w, the weights.  The turn q is found as in fair_scatter_kernel.  The loop over the flows has the SAME bounds in every
// lane (0 .. n_flows; the row's own flow contributes 0 by a select, the [f' < f] term is a select too): bounds that depend on the lane's
// flow would run both halves to the longest lane's end.  Every index into s_nt / s_run is < G and every index into s_w < n_flows: a key
// read from key[] is either < G or kFairNoKey, and is checked against G all the same.  Every place is < seg[8] <= n_reqs, the size of
// perm, and is checked all the same.  A key in the order has a weight >= 1 (wfair_hist_kernel read the same copy); the division is
// guarded all the same.
__global__ __launch_bounds__(64) void wfair_scatter_kernel(const uint16_t* __restrict__ key, uint32_t n_reqs, uint32_t n_bands, uint32_t n_flows,
                                                           uint32_t chunk, uint32_t n_chunks, const uint32_t* __restrict__ fh,
                                                           const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ seg,
                                                           const uint32_t* __restrict__ t_own, const uint32_t* __restrict__ w_own,
                                                           uint32_t* __restrict__ perm) {
  extern __shared__ uint2 s_wfair[];                                  // sized by the launch: s_nt[G] (8 bytes each), s_run[G], s_w[n_flows]
  const uint32_t G = n_bands * n_flows;
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  uint2* const s_nt = s_wfair;                                        // .x: the rows of the key (the same for every chunk), .y: its carried turns
  uint32_t* const s_run = (uint32_t*)(s_wfair + G);
  uint32_t* const s_w = s_run + G;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t g = lane; g < G; g += 64u) s_nt[g] = make_uint2(cnt[g], t_own[g]);
  for (uint32_t f = lane; f < n_flows; f += 64u) s_w[f] = w_own[f];
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    __syncthreads();                                                  // (one wavefront: the trips of the chunk before are done with s_run)
    for (uint32_t g = lane; g < G; g += 64u) s_run[g] = fh[(size_t)c * G + g];
    __syncthreads();
    const uint64_t r0 = (uint64_t)c * chunk, r1 = r0 + chunk < n_reqs ? r0 + chunk : n_reqs;
    for (uint64_t t0 = r0; t0 < r1; t0 += 64u) {
      const uint64_t r = t0 + lane;
      const uint32_t g = r < r1 ? (uint32_t)key[r] : kFairNoKey;
      const bool in = g < G;
      uint32_t q = 0u;
      for (uint64_t todo = __ballot(in); todo != 0ull;) {             // (wave-uniform: one trip of this loop per distinct key)
        const int first = (int)__builtin_ctzll(todo);
        const uint32_t g0 = (uint32_t)__shfl((int)g, first);          // (< G: the lane `first` is in the ballot)
        const bool mine = in && g == g0;
        const uint64_t m = __ballot(mine);
        const uint32_t before = s_run[g0];                            // (every lane reads the same word: a broadcast)
        if (mine) q = before + (uint32_t)__popcll(m & below);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if ((int)lane == first) s_run[g0] = before + (uint32_t)__popcll(m);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        todo &= ~m;
      }
      if (in) {
        const uint32_t b = g / n_flows, f = g - b * n_flows;
        const uint2* row = s_nt + b * n_flows;                        // (b < n_bands: the whole row is inside s_nt[0 .. G))
        const uint64_t wf = s_w[f];
        const int64_t cyc = (int64_t)(((uint64_t)row[f].y + q) / (wf ? wf : 1ull));
        int64_t place = (int64_t)seg[b] + (int64_t)q;
#pragma unroll 4
        for (uint32_t f2 = 0; f2 < n_flows; ++f2) {                   // (the flows in front take their turns of this cycle first)
          const uint2 nt = row[f2];
          const int64_t x = (cyc + (f2 < f ? 1 : 0)) * (int64_t)s_w[f2] - (int64_t)nt.y, n = f2 == f ? 0 : (int64_t)nt.x;
          place += x < 0 ? 0 : x > n ? n : x;
        }
        if (place >= 0 && place < (int64_t)n_reqs) perm[place] = (uint32_t)r;
      }
    }
  }
}

// A workgroup per chunk (grid-stride), behind the finish: taken[g] += the chunk's rows of key g that hold an endpoint.
__global__ __launch_bounds__(kBoundThreads) void wfair_taken_kernel(const uint16_t* __restrict__ key, const int32_t* __restrict__ out_pick, uint32_t n_reqs,
                                                                    uint32_t n_bands, uint32_t n_flows, uint32_t chunk, uint32_t n_chunks,
                                                                    uint32_t* __restrict__ taken) {
  __shared__ uint32_t s_h[kFairMaxKeys];
  const uint32_t G = n_bands * n_flows;
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    for (uint32_t g = threadIdx.x; g < G; g += kBoundThreads) s_h[g] = 0u;
    __syncthreads();
    const uint64_t r0 = (uint64_t)c * chunk, r1 = r0 + chunk < n_reqs ? r0 + chunk : n_reqs;
    for (uint64_t r = r0 + threadIdx.x; r < r1; r += kBoundThreads) {
      const uint32_t g = (uint32_t)key[r];
      if (g < G && out_pick[r] != EPPK_NO_PICK) atomicAdd(&s_h[g], 1u);      // (a count: the result of the add is not read)
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < G; g += kBoundThreads) {
      const uint32_t v = s_h[g];
      if (v) atomicAdd(&taken[g], v);                                 // (g < G; counts commute, and nobody reads taken before the next launch)
    }
    __syncthreads();
  }
}

// Grid-stride over the keys: the turns handed back, saturating.
__global__ __launch_bounds__(kBoundThreads) void wfair_carry_kernel(const uint32_t* __restrict__ t_own, const uint32_t* __restrict__ taken, uint32_t n_bands,
                                                                    uint32_t n_flows, uint32_t* __restrict__ turns) {
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  const uint32_t G = n_bands * n_flows;
  for (uint32_t g = blockIdx.x * kBoundThreads + threadIdx.x; g < G; g += gridDim.x * kBoundThreads) {
    const uint64_t sum = (uint64_t)t_own[g] + taken[g];
    turns[g] = sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum;
  }
}

}  // namespace eppk
#endif
