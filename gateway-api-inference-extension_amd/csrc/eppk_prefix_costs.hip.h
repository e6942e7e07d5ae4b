// eppk_prefix_costs.hip.h — matched prefix blocks and costs per LIST ENTRY (SEMANTICS.md §3k; include/eppk.h eppk_prefix_costs).
//
// Included by eppk.hip alone: the thirty pick units do not see this file, so a change here rebuilds one unit.
//
// The question is list-major: for request r, how many of its leading index hits contain each of the k <= 8 pods its list names?  The pick
// kernels put a lane or a bit per POD and cost O(pods) or O(candidates) per request; here a lane is a BLOCK of the request:
//   split      a request takes a GROUP of G = 16, 32 or 64 lanes, G the smallest of those that holds min(max_blocks, 64) blocks (chosen
//              at launch), so a wavefront serves 64 / G requests per pass and a 16-block workload fills it.  Only G = 64 meets rows longer
//              than its group: they take further trips of 64 blocks while every block so far hit.  Persistent grid, 256 threads.
//   fetch      everything that depends on r alone is requested together, one pass AHEAD of its use: the header (one address per group),
//              lane i's hash i (inside the row whatever n_blocks says: the load does not wait for the header), list entry j in lane j,
//              base[r].  The k pods reach every lane of their group without a second load: v_readlane at G = 64 (they are SGPRs
//              there), two v_readlane and a select at G = 32, DPP row_newbcast at G = 16 (a DPP row IS a group).  A pod that is no
//              candidate of the walk (EPPK_NO_PICK, out of range, a hole: one word of the snapshot's active set, read by lane j) becomes
//              0xFFFFFFFF, which no list id and no dense row equals.
//   probe      probe() per lane: displaced keys, tombstones, the reserved hashes and the small layout are its business.
//   stop       the ballot of "block missed", cut to the group, then ctz: the lanes in front of it are the walk (§3 PREFIX).
//   sets       each lane in front of the stop loads its slot's 64-byte list line (the others the all-zero row's empty line: no divergence
//              around the load).  A listed set: its ids, eight at a time (positions 0..7 are dwords 0, 4, 8, 12 of the line; the next eight
//              are skipped when no lane of the wavefront holds more), each compared with the k pods -- v_cmp writes the lane mask of
//              "has pod j" into an SGPR pair and s_or accumulates it: one vector instruction per (id, pod).  An overflowed set (count >
//              kListCap; a wave-uniform branch on its ballot): the k words [slot * 64 + (p & 63)] >> (p >> 6) of its dense row, loaded
//              together.  A present key with an empty set ends the walk as a miss does (prefix_walk's rule).
//   count      matched[j] = popcount(the group's part of mask j, in front of the stop), kept by lane j of the group across trips.
//   results    lane j stores matched[r][j] and cost[r][j]: a request's outputs are one contiguous store.
// Of the snapshot the kernel takes three words -- the active-set plane KSnap::nat, n_pods, KSnap::status -- not the block of twenty pointers.
// No LDS, no atomics but the sticky status flag of a bad row (one lane, once per pass that meets one).  A bad row and a context without
// index walk nothing.
#ifndef EPPK_PREFIX_COSTS_HIP_H
#define EPPK_PREFIX_COSTS_HIP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "eppk_kernels.hip.h"

namespace eppk {

constexpr uint32_t kPcThreads = 256u;        // four wavefronts per workgroup
constexpr uint32_t kPcNoPod = 0xFFFFFFFFu;   // a list entry the walk does not count for

__host__ __device__ __forceinline__ constexpr uint32_t pc_group(uint32_t max_blocks) { return max_blocks <= 16u ? 16u : max_blocks <= 32u ? 32u : 64u; }

// Lane J of every group of G lanes, in all lanes of that group.
template <uint32_t G, uint32_t J>
__device__ __forceinline__ uint32_t pc_group_bcast(uint32_t v, uint32_t lane) {
  if constexpr (G == 64u) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)J);
  } else if constexpr (G == 32u) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)J), hi = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)(32u + J));
    return lane < 32u ? lo : hi;
  } else if constexpr (G == 16u) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x150 + (int)J, 0xf, 0xf, false);      // row_newbcast:J
  } else {                                                                                          // G = 8 (score_lists_kernel): half a DPP row
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x150 + (int)J, 0xf, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x158 + (int)J, 0xf, 0xf, false);
    return (lane & 8u) ? hi : lo;
  }
}
template <uint32_t G, size_t... Js>
__device__ __forceinline__ void pc_group_bcast_all(uint32_t v, uint32_t lane, uint32_t (&out)[EPPK_MAX_TOPK], std::index_sequence<Js...>) {
  ((out[Js] = pc_group_bcast<G, (uint32_t)Js>(v, lane)), ...);
}

// The block walk of one pass: lane gl of a group probes block t0 + gl of its request (`h` = that block's hash for the first trip, `row`
// the request row for further ones, `nbe` the blocks the group walks: 0 = none) and returns, in lane j < k of the group, how many of the
// leading hits hold pod P[j] (kPcNoPod: none).  Written once: prefix_costs_kernel and score_lists_kernel (eppk_score_lists.hip.h) call it.
template <typename LW, uint32_t G>
__device__ __forceinline__ uint32_t pc_walk(const KIndex& ix, const uint64_t* row, uint64_t h, uint32_t nbe, const uint32_t (&P)[EPPK_MAX_TOPK], const uint32_t k,
                                            const uint32_t lane) {
  constexpr uint64_t GM = G == 64u ? ~0ull : (1ull << (G & 63u)) - 1ull;
  const uint32_t gl = lane & (G - 1u), gs = lane & ~(G - 1u);
  auto grp = [&](uint64_t m) -> uint64_t { return G == 64u ? m : (m >> gs) & GM; };     // the lane's group's part of a ballot
  uint32_t acc = 0u;
  for (uint32_t t0 = 0u; __ballot(nbe > t0) != 0ull; t0 += G) {      // one trip unless G = 64 and a row is longer
    const bool act = t0 + gl < nbe;
    const uint32_t slot = probe(ix, h, act);
    const uint64_t miss = grp(__ballot(act && slot == kNotFound));
    const uint32_t nloc = nbe > t0 ? (nbe - t0 < G ? nbe - t0 : G) : 0u;
    const uint32_t stop1 = miss ? (uint32_t)__builtin_ctzll(miss) : nloc;
    const bool front = gl < stop1;
    uint32_t d[16];
    load_line16<false>(ix.lists_all + (size_t)(front ? slot : ix.slots + 2u) * kListDwords, d);      // (others: the all-zero row's empty line)
    const uint32_t cnt = d[3];
    const uint64_t empty = grp(__ballot(front && cnt == 0u));
    const uint32_t stop = empty ? (uint32_t)__builtin_ctzll(empty) : stop1;
    const uint64_t in_front = stop >= 64u ? ~0ull : (1ull << stop) - 1ull;      // group-relative
    const uint64_t listed = __ballot(cnt - 1u < kListCap);
    const uint64_t over = __ballot(front && cnt > kListCap);
    uint64_t m[EPPK_MAX_TOPK];
#pragma unroll
    for (uint32_t j = 0; j < EPPK_MAX_TOPK; ++j) m[j] = 0ull;
#pragma unroll
    for (uint32_t c8 = 0; c8 < kListCap; c8 += 8u) {
      if (c8 != 0u && __ballot(cnt > c8 && cnt <= kListCap) == 0ull) break;
#pragma unroll
      for (uint32_t e = 0; e < 8u; ++e) {
        const uint32_t id = list_id(d, c8 + e);
#pragma unroll
        for (uint32_t j = 0; j < EPPK_MAX_TOPK; ++j)
          if (j < k) m[j] |= __ballot(id == P[j]);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < EPPK_MAX_TOPK; ++j) m[j] &= listed;
    if (__builtin_expect(over != 0ull, 0)) {                         // dense rows: the k words first, then their bits
      const LW* bm = (const LW*)ix.bitmaps + (size_t)slot * 64u;
      const bool mine = front && cnt > kListCap;
      LW w[EPPK_MAX_TOPK];
#pragma unroll
      for (uint32_t j = 0; j < EPPK_MAX_TOPK; ++j) w[j] = (mine && j < k && P[j] != kPcNoPod) ? bm[P[j] & 63u] : (LW)0;
#pragma unroll
      for (uint32_t j = 0; j < EPPK_MAX_TOPK; ++j)
        if (j < k) m[j] |= __ballot(((w[j] >> ((P[j] >> 6) & (8u * (uint32_t)sizeof(LW) - 1u))) & 1) != 0);
    }
#pragma unroll
    for (uint32_t j = 0; j < EPPK_MAX_TOPK; ++j) {
      const uint32_t cj = (uint32_t)__builtin_popcountll(grp(m[j]) & in_front);
      if (gl == j) acc += cj;
    }
    nbe = (stop == G && nbe > t0 + G) ? nbe : 0u;                    // every block of the trip hit and the row goes on
    h = t0 + G + gl < nbe ? row[1u + t0 + G + gl] : 0ull;
  }
  return acc;
}

// What a pass needs of its request before anything can be probed (one request per group; r is clamped, a group past the batch is not stored).
struct PcFetch { uint64_t hdr, h; int32_t p; uint32_t base; };

template <typename LW, uint32_t G>
__global__ __launch_bounds__(kPcThreads) void prefix_costs_kernel(const uint64_t* __restrict__ nat, uint32_t n_pods, uint32_t* status, KIndex ix,
                                                                  const uint8_t* __restrict__ reqs, uint32_t stride, uint32_t n_reqs,
                                                                  const int32_t* __restrict__ lists, uint32_t k, const uint32_t* __restrict__ base,
                                                                  uint32_t unit, uint32_t* __restrict__ out_cost, uint32_t* __restrict__ out_matched) {
  constexpr uint32_t NG = 64u / G;                                     // requests per pass
  const uint32_t lane = threadIdx.x & 63u, gl = lane & (G - 1u);
  const uint32_t wib = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  const uint32_t hwords = (stride - 8u) / 8u;
  const uint32_t n_pass = (n_reqs + NG - 1u) / NG, step = gridDim.x * wpb;
  auto fetch = [&](uint32_t q) -> PcFetch {
    const uint32_t r0 = q * NG + lane / G, r = r0 < n_reqs ? r0 : n_reqs - 1u;
    const uint64_t* row = (const uint64_t*)(reqs + (size_t)r * stride);
    PcFetch f;
    f.hdr = row[0];
    f.h = gl < hwords ? row[1u + gl] : 0ull;
    f.p = gl < k ? lists[(size_t)r * k + gl] : EPPK_NO_PICK;
    f.base = (base && gl < k) ? base[r] : 0u;
    return f;
  };

  uint32_t q = blockIdx.x * wpb + wib;
  if (q >= n_pass) return;
  PcFetch nxt = fetch(q);
  for (; q < n_pass; q += step) {
    const PcFetch cur = nxt;
    if (q + step < n_pass) nxt = fetch(q + step);                     // (wave-uniform)
    const uint32_t r = q * NG + lane / G;
    const bool live = r < n_reqs;
    const uint64_t* row = (const uint64_t*)(reqs + (size_t)(live ? r : n_reqs - 1u) * stride);
    const int32_t adapter = (int32_t)(uint32_t)cur.hdr;
    const uint32_t nb = (uint32_t)(cur.hdr >> 32);
    const bool bad = live && (nb > hwords || adapter < -1 || adapter >= (int32_t)EPPK_MAX_ADAPTERS);
    if (__builtin_expect(__ballot(bad) != 0ull, 0) && bad && gl == 0u) atomicOr(status, kStatusBadRow);
    uint32_t nbe = (bad || !live || ix.slots == 0u) ? 0u : nb;        // blocks this group still walks

    // the list: entry j in lane j of the group -> a pod the walk counts for, or kPcNoPod; then into every lane of the group
    uint32_t pv = kPcNoPod;
    if (cur.p >= 0 && (uint32_t)cur.p < n_pods && ((nat[(uint32_t)cur.p >> 6] >> ((uint32_t)cur.p & 63u)) & 1ull)) pv = (uint32_t)cur.p;
    uint32_t P[EPPK_MAX_TOPK];
    pc_group_bcast_all<G>(pv, lane, P, std::make_index_sequence<EPPK_MAX_TOPK>{});

    const uint32_t acc = pc_walk<LW, G>(ix, row, cur.h, nbe, P, k, lane);     // matched[gl] of the lane's request

    if (live && gl < k) {
      uint32_t b = cur.base;
      if (!base) {                                                     // n_blocks * unit, inside 1 .. 2^32 - 1
        const uint64_t b64 = (uint64_t)nb * unit;
        b = b64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : b64 ? (uint32_t)b64 : 1u;
      }
      uint32_t cost = b;
      if (b - 1u < EPPK_MAX_COST) {                                    // (a base out of range goes through unchanged: the resolve reports it)
        const uint64_t saved = (uint64_t)acc * unit;
        cost = saved >= b ? 1u : b - (uint32_t)saved;
      }
      const size_t at = (size_t)r * k + gl;
      if (out_matched) out_matched[at] = acc;
      if (out_cost) out_cost[at] = cost;
    }
  }
}

}  // namespace eppk

#endif  // EPPK_PREFIX_COSTS_HIP_H
