// eppk_index_export.hip.h — the prefix index read out as (hash, pod, age) triples (SEMANTICS.md §6d; include/eppk.h eppk_index_export).
//
// Included by eppk.hip alone, behind eppk_score_lists.hip.h.  Read-only on the index: the walk of index_pod_hist_kernel (a lane per
// row, 64 consecutive rows of the PHYSICAL table per wavefront trip, the dense rows behind a ballot by the whole wavefront), made twice
// with a scan in between, so that every triple has ONE place that no atomic's arrival order decides:
//   count     export_count_kernel<LW>   tile t = rows 64 t .. 64 t + 63 of the slots + 2 rows (the table's words, then the rows of the
//                                       hashes 0 and ~0).  Lane = row: the pairs of its set -- the list's count dword, or the popcount
//                                       of its dense row (summed over the wavefront, one overflowed row after the other).  tiles[t] = the
//                                       wavefront's sum, 64 bits.
//   scan      export_scan_tiles_kernel  a workgroup per kExScanTiles tiles: tiles[t] := the pairs of the tiles in front of t INSIDE the
//                                       workgroup's run, blocks[b] = the run's sum.
//             export_scan_top_kernel    ONE workgroup, a segment of blocks[] per thread (banded_offsets_kernel's shape): blocks[b] := the
//                                       pairs in front of run b; *total = all of them; the sticky flag when they exceed `cap`.
//                                       2^29 rows = 2^23 tiles = 2^13 runs: both levels are one pass over their words.
//   scatter   export_scatter_kernel<LW> the same tile walk.  An exclusive scan of the 64 per-row counts over the wavefront (DPP: row_shr
//                                       1 / 2 / 4 / 8, row_bcast 15 / 31) + blocks[t / kExScanTiles] + tiles[t] = the row's first place.
//                                       A listed row is written by its lane (its ids ascend: the index's invariant); a dense row by the
//                                       wavefront: lane l holds word l, bit j of it = pod 64 j + l, ascending pods are j-major, so for
//                                       every j the lanes whose bit j is set store behind the running count, each at the popcount of the
//                                       ballot below it.
// Order: ascending physical row, pods ascending inside a row.  Every store is a plain vector store behind `place < cap`: with more
// triples than `cap` exactly the first `cap` of that order are written.  No LDS but the scan's, no atomics but the sticky flag.
#ifndef EPPK_INDEX_EXPORT_HIP_H
#define EPPK_INDEX_EXPORT_HIP_H

#include "eppk_kernels.hip.h"

namespace eppk {

constexpr uint32_t kExThreads = 256u;                  // count and scatter passes
constexpr uint32_t kExScanThreads = 256u, kExScanPer = 4u, kExScanTiles = kExScanThreads * kExScanPer;   // tiles per workgroup of the first scan level
constexpr uint32_t kExTopThreads = 1024u;
constexpr uint32_t kStatusExportShort = 16u;           // eppk.h: EPPK_LAUNCH_EXPORT_TRUNCATED

// sum / inclusive scan of a u32 over the wavefront (every lane takes part).  Lanes without a source take the `old` operand, 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t ex_dpp0(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false); }
__device__ __forceinline__ uint32_t ex_wave_scan(uint32_t v) {
  v += ex_dpp0<0x111, 0xf>(v);       // row_shr:1
  v += ex_dpp0<0x112, 0xf>(v);       // row_shr:2
  v += ex_dpp0<0x114, 0xf>(v);       // row_shr:4
  v += ex_dpp0<0x118, 0xf>(v);       // row_shr:8: every row of 16 lanes holds its own inclusive scan
  v += ex_dpp0<0x142, 0xa>(v);       // row_bcast:15 into rows 1 and 3
  v += ex_dpp0<0x143, 0xc>(v);       // row_bcast:31 into rows 2 and 3
  return v;
}
__device__ __forceinline__ uint32_t ex_wave_sum(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)ex_wave_scan(v), 63); }

// What lane `lane` of a tile sees of its row base + lane: the key word, the list line of a present key (d is written for those alone)
// and the pairs of its set; om = the lanes whose set lives in its dense row.  Both passes go through here, so they agree on every count.
template <typename LW>
__device__ __forceinline__ uint32_t ex_tile_counts(const uint64_t* keys, const void* bitmaps, const uint32_t* lists, uint32_t slots, uint32_t base,
                                                   uint32_t lane, uint64_t& k, uint32_t (&d)[16], unsigned long long& om) {
  const uint32_t total = slots + 2u, row = base + lane;
  k = row < total ? keys[row] : 0ull;
  bool present = false;
  if (row < total && !(row < slots && !is_key_word(row)))             // (the meta words of a bucket are not keys)
    present = k != 0ull && !(row < slots && k == kTomb);
  bool over = false;
  uint32_t cnt = 0u;
  if (present) {
    load_line16<false>(lists + (size_t)row * kListDwords, d);         // (nothing writes the index during the launch)
    over = d[3] > kListCap;
    cnt = over ? 0u : d[3];
  }
  om = __ballot(over);
  for (unsigned long long m = om; m; m &= m - 1ull) {
    const uint32_t src = (uint32_t)__builtin_ctzll(m);
    const LW v = ((const LW*)bitmaps)[(size_t)(base + src) * 64u + lane];
    const uint32_t members = ex_wave_sum((uint32_t)__builtin_popcountll((unsigned long long)v));
    if (lane == src) cnt = members;
  }
  return cnt;
}

template <typename LW>
__global__ __launch_bounds__(kExThreads) void export_count_kernel(const uint64_t* keys, const void* bitmaps, const uint32_t* lists, uint32_t slots,
                                                                  uint32_t n_tiles, uint64_t* __restrict__ tiles) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t t = wave; t < n_tiles; t += nwaves) {
    uint64_t k;
    uint32_t d[16];
    unsigned long long om;
    const uint32_t cnt = ex_tile_counts<LW>(keys, bitmaps, lists, slots, t * 64u, lane, k, d, om);
    const uint32_t sum = ex_wave_sum(cnt);                            // (at most 64 rows of 4096 pods)
    if (lane == 0u) tiles[t] = (uint64_t)sum;
  }
}

// exclusive scan of one 64-bit value per thread over the workgroup (THREADS / 64 wavefronts); total = the workgroup's sum
template <uint32_t THREADS>
__device__ __forceinline__ uint64_t ex_block_scan(uint64_t v, uint64_t* s_w, uint64_t& total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (uint32_t dd = 1u; dd < 64u; dd <<= 1) {
    const uint64_t o = (uint64_t)__shfl_up((unsigned long long)inc, dd);
    if (lane >= dd) inc += o;
  }
  if (lane == 63u) s_w[w] = inc;
  __syncthreads();
  uint64_t front = 0ull, all = 0ull;
#pragma unroll
  for (uint32_t i = 0; i < THREADS / 64u; ++i) {
    const uint64_t x = s_w[i];
    front += i < w ? x : 0ull;
    all += x;
  }
  total = all;
  return front + inc - v;
}

__global__ __launch_bounds__(kExScanThreads) void export_scan_tiles_kernel(uint64_t* tiles, uint32_t n_tiles, uint64_t* __restrict__ blocks) {
  __shared__ uint64_t s_w[kExScanThreads / 64u];
  const uint32_t t0 = blockIdx.x * kExScanTiles + threadIdx.x * kExScanPer;      // (n_tiles <= 2^23 + 1: no overflow)
  uint64_t v[kExScanPer], sum = 0ull;
#pragma unroll
  for (uint32_t u = 0; u < kExScanPer; ++u) {
    v[u] = t0 + u < n_tiles ? tiles[t0 + u] : 0ull;
    sum += v[u];
  }
  uint64_t all;
  uint64_t run = ex_block_scan<kExScanThreads>(sum, s_w, all);
#pragma unroll
  for (uint32_t u = 0; u < kExScanPer; ++u) {
    if (t0 + u < n_tiles) tiles[t0 + u] = run;
    run += v[u];
  }
  if (threadIdx.x == 0u) blocks[blockIdx.x] = all;
}

// ONE workgroup.  n_blocks = 0 (a context without an index): *total = 0.  status (nullable): raised when `cap` is not a count query
// (cap != 0) and does not hold every triple.
__global__ __launch_bounds__(kExTopThreads) void export_scan_top_kernel(uint64_t* blocks, uint32_t n_blocks, uint64_t cap, uint64_t* __restrict__ total,
                                                                         uint32_t* status) {
  __shared__ uint64_t s_w[kExTopThreads / 64u];
  const uint32_t seg_len = (n_blocks + kExTopThreads - 1u) / kExTopThreads;
  const uint32_t b0 = threadIdx.x * seg_len < n_blocks ? threadIdx.x * seg_len : n_blocks, b1 = b0 + seg_len < n_blocks ? b0 + seg_len : n_blocks;
  uint64_t sum = 0ull;
  for (uint32_t b = b0; b < b1; ++b) sum += blocks[b];
  uint64_t all;
  uint64_t run = ex_block_scan<kExTopThreads>(sum, s_w, all);
  for (uint32_t b = b0; b < b1; ++b) {
    const uint64_t v = blocks[b];
    blocks[b] = run;
    run += v;
  }
  if (threadIdx.x == 0u) {
    *total = all;
    if (status && cap != 0ull && all > cap) atomicOr(status, kStatusExportShort);
  }
}

template <typename LW>
__global__ __launch_bounds__(kExThreads) void export_scatter_kernel(const uint64_t* keys, const void* bitmaps, const uint32_t* lists, const uint32_t* rstamps,
                                                                    uint32_t slots, uint32_t epoch, uint32_t cur_tag, uint32_t n_tiles, const uint64_t* __restrict__ tiles,
                                                                    const uint64_t* __restrict__ blocks, uint64_t* __restrict__ out_hash,
                                                                    uint32_t* __restrict__ out_pod, uint8_t* __restrict__ out_age, uint64_t cap) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t t = wave; t < n_tiles; t += nwaves) {                // (cur_tag: tag_of_epoch(epoch), from the host)
    const uint32_t base = t * 64u, row = base + lane;
    uint64_t k;
    uint32_t d[16];
    unsigned long long om;
    const uint32_t cnt = ex_tile_counts<LW>(keys, bitmaps, lists, slots, base, lane, k, d, om);
    const uint64_t tile_at = blocks[t / kExScanTiles] + tiles[t];
    if (ex_wave_sum(cnt) == 0u || tile_at >= cap) continue;           // (wave-uniform: an empty tile, or one wholly behind `cap`)
    // the age in full (the trim's slot_age stops at 63): the tag's for a word of the table, the exact stamp's for the two rows behind it
    // (spelled out here, not through tag_age: a caller of its own would widen the argument ranges the other index kernels are compiled under)
    const uint32_t tag = meta_of_lane(k, lane) >> 24;
    uint32_t age = (cur_tag + kTagMod - tag) % kTagMod;                // a present key of the table has a tag in 1 .. 255
    if (row >= slots && row < slots + 2u) age = epoch - rstamps[row - slots];
    const uint64_t h = row < slots ? k : (row == slots ? 0ull : kTomb);
    const uint64_t at = tile_at + (uint64_t)(ex_wave_scan(cnt) - cnt);
    if (cnt != 0u && !((om >> lane) & 1ull)) {                       // a listed row: its own lane
#pragma unroll
      for (uint32_t j = 0; j < kListCap; ++j) {
        if (j < cnt && at + j < cap) {
          out_hash[at + j] = h;
          out_pod[at + j] = list_id(d, j);
          out_age[at + j] = (uint8_t)age;
        }
      }
    }
    for (unsigned long long m = om; m; m &= m - 1ull) {               // a dense row: the wavefront
      const int src = __builtin_ctzll(m);
      const LW v = ((const LW*)bitmaps)[(size_t)(base + (uint32_t)src) * 64u + lane];
      const uint64_t vh = u64_of((uint32_t)__shfl((int)(uint32_t)h, src), (uint32_t)__shfl((int)(uint32_t)(h >> 32), src));
      uint64_t vat = u64_of((uint32_t)__shfl((int)(uint32_t)at, src), (uint32_t)__shfl((int)(uint32_t)(at >> 32), src));
      const uint32_t vage = (uint32_t)__shfl((int)age, src);
      for (uint32_t j = 0; j < 8u * (uint32_t)sizeof(LW); ++j) {
        if (!__any((LW)(v >> j) != 0)) break;                         // (no pod at 64 j and beyond)
        const bool in = ((v >> j) & (LW)1) != 0;
        const unsigned long long bm = __ballot(in);
        const uint64_t place = vat + (uint64_t)__builtin_popcountll(bm & below);
        if (in && place < cap) {
          out_hash[place] = vh;
          out_pod[place] = j * 64u + lane;
          out_age[place] = (uint8_t)vage;
        }
        vat += (uint64_t)__builtin_popcountll(bm);
      }
    }
  }
}

}  // namespace eppk

#endif  // EPPK_INDEX_EXPORT_HIP_H
