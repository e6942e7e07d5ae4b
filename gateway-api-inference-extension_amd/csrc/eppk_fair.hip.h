// eppk_fair.hip.h — fair shares between flows for the banded and costed pickers (SEMANTICS.md §3g; include/eppk.h eppk_fair_resolve_device).
//
// Included by eppk.hip alone, behind eppk_costed.hip.h.  Nothing of eppk_bounded.hip.h, eppk_banded.hip.h or eppk_costed.hip.h is
// edited: their count / scan / assign / finish kernels are launched as they are.  They walk places [seg[b], seg[b + 1]) of a permutation;
// the kernels here write ANOTHER permutation into the same layout (perm, seg[0 .. 8]; seg[8] = all rows in the order), and a band byte
// per row of their own for the round and finish kernels to read.
//
// Every request carries a flow id.  A row is IN THE ORDER iff band < n_bands and flow < n_flows; its key is g = band * n_flows + flow
// (< 8 * 1024), its TURN q the number of rows in front of it in the batch with the same key.  Band b's rows are placed by (q, flow)
// ascending -- round-robin over the flows in flow-id order -- and the place needs no sort: with cnt[g] the rows of key g,
//     place = seg[b] + sum over the band's flows f' of min(cnt[b][f'], q) + #{f' < f : cnt[b][f'] > q}.
//
//   fair_hist_kernel     per chunk, the rows of every key -> fh[chunk][G], G = n_bands * n_flows; and per row its key (0xFFFF: not in the
//                        order) and its EFFECTIVE band byte (the band, or 0xFF), both into the context's own memory: the caller's band and
//                        flow bytes are read exactly once, so the three passes agree whatever the caller does to them meanwhile
//   fair_offsets_kernel  per key, fh := the rows of the key in the chunks in front (exclusive scan over the chunks, the chunk axis cut
//                        into segments across threads as bounded_scan_kernel cuts it); cnt[g]; seg[] from the band sums
//   fair_scatter_kernel  per chunk, one wavefront, 64 rows per trip in ascending order: q = fh[chunk][g] + the rows of g in earlier
//                        trips (a carried LDS counter per key) + the lanes below with the same g; perm[place] = row
// A row with a good band and a bad flow gets the effective band byte 0xFF, which the round and finish kernels treat as they treat any
// band byte >= n_bands: in no segment, EPPK_NO_PICK / 0.0 / EPPK_RANK_NONE, EPPK_LAUNCH_BAD_REQUEST_ROW raised, its list still checked.
// As everywhere in the resolves no atomic's return value is read: every add is a count.
#ifndef EPPK_FAIR_HIP_H
#define EPPK_FAIR_HIP_H

#include "eppk_costed.hip.h"

namespace eppk {

constexpr uint32_t kFairMaxKeys = EPPK_MAX_BANDS * EPPK_MAX_FLOWS;   // 8 192 counters of 4 bytes: 32 KiB of LDS
constexpr uint32_t kFairNoKey = 0xFFFFu;                             // key of a row that is not in the order (every key is < kFairMaxKeys)
constexpr uint32_t kFairBadBand = 0xFFu;                             // effective band byte of such a row (>= EPPK_MAX_BANDS)

// A workgroup per chunk (grid-stride): row `chunk` of fh, and key[] / eband[] of the chunk's rows.
__global__ __launch_bounds__(kBoundThreads) void fair_hist_kernel(const uint8_t* __restrict__ band, const uint16_t* __restrict__ flow, uint32_t n_reqs,
                                                                  uint32_t n_bands, uint32_t n_flows, uint32_t chunk, uint32_t n_chunks,
                                                                  uint32_t* __restrict__ fh, uint16_t* __restrict__ key, uint8_t* __restrict__ eband) {
  __shared__ uint32_t s_h[kFairMaxKeys];
  const uint32_t G = n_bands * n_flows;
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    for (uint32_t g = threadIdx.x; g < G; g += kBoundThreads) s_h[g] = 0u;
    __syncthreads();
    const uint64_t r0 = (uint64_t)c * chunk, r1 = r0 + chunk < n_reqs ? r0 + chunk : n_reqs;
    for (uint64_t r = r0 + threadIdx.x; r < r1; r += kBoundThreads) {
      const uint32_t b = band_of(band, r), f = flow ? (uint32_t)flow[r] : 0u;
      const bool in = b < n_bands && f < n_flows;
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

// A workgroup per kBoundScanPods keys (grid-stride), a thread per (chunk segment, key) as in bounded_scan_kernel:
// fh[c][g] := rows of key g in the chunks in front of c; cnt[g] = all rows of key g; seg[b + 1 .. 8] += the rows of band b (seg[] is
// zeroed in front of the launch; the adds are counts, they commute, and nobody reads seg before the next launch).
__global__ __launch_bounds__(kBoundScanSegs * kBoundScanPods) void fair_offsets_kernel(uint32_t* fh, uint32_t n_chunks, uint32_t n_bands, uint32_t n_flows,
                                                                                      uint32_t* __restrict__ cnt, uint32_t* __restrict__ seg) {
  __shared__ uint32_t s_sum[kBoundScanSegs][kBoundScanPods], s_band[EPPK_MAX_BANDS];
  const uint32_t G = n_bands * n_flows;
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  const uint32_t lp = threadIdx.x % kBoundScanPods, sg = threadIdx.x / kBoundScanPods;
  const uint32_t seg_len = (n_chunks + kBoundScanSegs - 1u) / kBoundScanSegs;
  const uint32_t c0 = sg * seg_len < n_chunks ? sg * seg_len : n_chunks, c1 = c0 + seg_len < n_chunks ? c0 + seg_len : n_chunks;
  for (uint32_t gb = blockIdx.x * kBoundScanPods; gb < G; gb += gridDim.x * kBoundScanPods) {          // (uniform over the workgroup)
    if (threadIdx.x < EPPK_MAX_BANDS) s_band[threadIdx.x] = 0u;
    const uint32_t g = gb + lp;
    const bool live = g < G;
    uint32_t sum = 0u;
    if (live) {
#pragma unroll 8
      for (uint32_t c = c0; c < c1; ++c) sum += fh[(size_t)c * G + g];
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
      for (uint32_t c = c0; c < c1; c += 8u) {                       // eight loads in flight, then their prefix
        uint32_t v[8];
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) v[i] = c + i < c1 ? fh[(size_t)(c + i) * G + g] : 0u;
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i)
          if (c + i < c1) { fh[(size_t)(c + i) * G + g] = run; run += v[i]; }
      }
      if (sg == 0u) {
        cnt[g] = total;
        atomicAdd(&s_band[g / n_flows], total);                       // (g < G: the band is < n_bands; the result of the add is not read)
      }
    }
    __syncthreads();
    if (threadIdx.x < EPPK_MAX_BANDS) {
      const uint32_t t = s_band[threadIdx.x];
      if (t) for (uint32_t b2 = threadIdx.x + 1u; b2 <= EPPK_MAX_BANDS; ++b2) atomicAdd(&seg[b2], t);   // (inside seg[0 .. 8]; not read)
    }
    __syncthreads();
  }
}

// A workgroup of ONE wavefront per chunk (grid-stride), with 2 * G words of dynamic LDS (8 bytes per key: 128 bytes for 16 flows in one
// band, 64 KiB for 1 024 flows in 8 bands, so that a small G does not cap the wavefronts per CU).  s_cnt: the rows of every key (the
// same for every chunk); s_run: for every key the rows in front of the place the wavefront is at.  Within a trip the lanes of one key
// find each other by ballot (one trip of the loop per distinct key in the wavefront: wave-uniform, nobody waits for a wave-mate).  Every index into s_cnt / s_run is < G: a key
// read from key[] is either < G or kFairNoKey, and is checked against G all the same.  Every place is < seg[8] <= n_reqs, the size of
// perm, and is checked all the same.
__global__ __launch_bounds__(64) void fair_scatter_kernel(const uint16_t* __restrict__ key, uint32_t n_reqs, uint32_t n_bands, uint32_t n_flows,
                                                          uint32_t chunk, uint32_t n_chunks, const uint32_t* __restrict__ fh,
                                                          const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ seg,
                                                          uint32_t* __restrict__ perm) {
  extern __shared__ uint32_t s_fair[];                                // 2 * G words, sized by the launch: s_cnt[G], s_run[G]
  const uint32_t G = n_bands * n_flows;
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  uint32_t* const s_cnt = s_fair;
  uint32_t* const s_run = s_fair + G;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t g = lane; g < G; g += 64u) s_cnt[g] = cnt[g];
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
        const uint32_t* row = s_cnt + b * n_flows;                    // (b < n_bands: the whole row is inside s_cnt[0 .. G))
        uint32_t place = seg[b];
        for (uint32_t f2 = 0; f2 < n_flows; ++f2) {
          const uint32_t cf = row[f2];
          place += (cf < q ? cf : q) + (f2 < f && cf > q ? 1u : 0u);
        }
        if (place < n_reqs) perm[place] = (uint32_t)r;
      }
    }
  }
}

}  // namespace eppk
#endif
