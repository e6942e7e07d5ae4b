// eppk_prefix_summary.hip.h — what the prefix index knows about a request, over EVERY candidate (SEMANTICS.md §3m; include/eppk.h
// eppk_prefix_summary), and the select pass of eppk_pick_hybrid built on it.
//
// Included by eppk.hip alone: the thirty pick units do not see this file, so a change here rebuilds one unit.
//
// The question is pod-major where prefix_costs_kernel's is list-major: for request r, how many of its leading index hits contain each of
// up to 4096 pods, and what is the maximum over the candidates?  A wavefront takes one request; persistent grid, 256 threads, no LDS.
//   fetch      one pass AHEAD of its use, everything that depends on r alone: the header, lane i's hash i (inside the row whatever n_blocks
//              says), word `lane` of the request's mask row.
//   probe      lane i probes block t0 + i with probe(): displaced keys, tombstones, the reserved hashes and the small layout stay its
//              business.  Rows longer than 64 blocks take further trips while every block so far hit.
//   stop       every lane in front of the first miss loads its slot's 64-byte list line (the others the all-zero row's empty line: no
//              divergence around the load).  The ballot of misses, then of present keys with an empty set, then ctz: the lanes in front
//              of it are the walk (§3 PREFIX) -- known after ONE parallel round, before any set is counted.
//   runs       an intact chain's sets are nested and mostly EQUAL.  Lane i compares its line (the twelve id dwords and the count) with
//              lane i - 1's by DPP row_shr:1; equal lines of listed sets are equal sets, so a run of m equal lines is added ONCE with
//              multiplicity m.  A run ends at a different line, at a dense set and at a DPP row boundary (m <= 16): a line that differs
//              only in unspecified bytes costs a second add, never a wrong count.
//   sets       a run's set S becomes one LW word per lane in the pick kernels' pod layout (bit j of lane word l = pod 64j + l, which is
//              also a dense row's).  Listed (at most kListCap ids): the ids are v_readlane'd out of the lane that holds the line, and lane
//              id & 63 sets bit id >> 6 -- no global write, no LDS.  Dense: one coalesced load of the slot's row.
//   count      bit-sliced in registers: nine planes c[0..8] of one LW word per lane (max_blocks = 256 makes best = 256 reachable).  Adding
//              m copies of S is one ripple add per set bit i of m, entered at plane i:  carry = S;  t = c[b] & carry, c[b] ^= carry,
//              carry = t  for b = i, i + 1, ...  until the wave's ballot of carry != 0 is empty (two planes on average).
//   max        cand = valid & active & the mask row, transposed in registers (ps_transpose); from the top plane down  t = cand & c[b]; any lane t != 0 -> cand = t,
//              best |= 1 << b.  Afterwards cand is exactly the holders: popcounts summed by DPP, the lowest ctz(cand) * 64 + lane by DPP.
//   results    lane 0 stores {walk, best, holders, first} as one 16-byte store.
// Of the snapshot the kernel takes three words -- the lane-transposed active set KSnap::act_t, n_pods, KSnap::status.  No atomics but the
// sticky status flag of a bad row.  No answer depends on the grid: a request is one wavefront's, start to end.
#ifndef EPPK_PREFIX_SUMMARY_HIP_H
#define EPPK_PREFIX_SUMMARY_HIP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eppk_kernels.hip.h"

namespace eppk {

constexpr uint32_t kPsThreads = 256u;        // four wavefronts per workgroup
constexpr int kPsPlanes = 9;                 // counts up to 256 (max_blocks)
constexpr uint32_t kPsNone = 0xFFFFFFFFu;    // `first` of a request nobody holds anything of

struct PsFetch { uint64_t hdr, h, m; };

// c += S in every pod's counter, entered at plane B (S counted 2^B times); ends as soon as no lane carries.  (Nested ifs, not a loop with
// a break: the planes stay registers.)
template <typename LW, int B>
__device__ __forceinline__ void ps_add(LW (&c)[kPsPlanes], LW carry) {
  if constexpr (B < kPsPlanes) {
    const LW t = c[B] & carry;
    c[B] ^= carry;
    if (__ballot(t != 0) != 0ull) ps_add<LW, B + 1>(c, t);
  }
}

// ... m <= 64 times (m wave-uniform).
template <typename LW>
__device__ __forceinline__ void ps_add_times(LW (&c)[kPsPlanes], LW s, uint32_t m) {
  if (m & 1u) ps_add<LW, 0>(c, s);
  if (m & 2u) ps_add<LW, 1>(c, s);
  if (m & 4u) ps_add<LW, 2>(c, s);
  if (m & 8u) ps_add<LW, 3>(c, s);
  if (m & 16u) ps_add<LW, 4>(c, s);
  if (m & 32u) ps_add<LW, 5>(c, s);
  if (m & 64u) ps_add<LW, 6>(c, s);
}

// The listed set whose line lane `b` holds (cnt ids, b and cnt wave-uniform) as a lane word: id E travels through an SGPR to lane id & 63.
template <typename LW, uint32_t E = 0u>
__device__ __forceinline__ void ps_set_from_line(const uint32_t (&d)[16], uint32_t b, uint32_t cnt, uint32_t lane, LW& s) {
  if constexpr (E < kListCap) {
    if (E < cnt) {
      const uint32_t dw = (uint32_t)__builtin_amdgcn_readlane((int)d[list_dw(E)], (int)b);
      const uint32_t id = list_hi(E) ? (dw >> 16) : (dw & 0xFFFFu);
      const uint32_t j = id >> 6;
      if (j < 8u * (uint32_t)sizeof(LW) && lane == (id & 63u)) s |= (LW)((LW)1 << j);
      ps_set_from_line<LW, E + 1u>(d, b, cnt, lane, s);
    }
  }
}

// sum over the wavefront, wave-uniform: wave_min_u32's steps (quad xor 1, xor 2, half mirror, mirror, row_bcast:15, row_bcast:31)
__device__ __forceinline__ uint32_t ps_wave_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// A natural-layout pod set (lane w holds word w: bit p = pod 64 w + p; lanes past the row hold 0) as lane words (bit j of lane l = pod
// 64 j + l): the 64 x 64 bit transpose in six butterfly steps -- lanes l and l ^ s swap the s-wide blocks off their diagonal -- where
// transpose_words takes a v_readlane pair per word (61 us of a masked 64k batch against 47 us for everything else).
__device__ __forceinline__ uint64_t ps_transpose(uint64_t x, uint32_t lane) {
#pragma unroll
  for (uint32_t s = 32u; s >= 1u; s >>= 1) {
    const uint64_t m = ~0ull / ((1ull << s) + 1ull);                   // the low s bits of every 2s: 0x00000000FFFFFFFF ... 0x5555555555555555
    const uint64_t p = ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), (int)s) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)x, (int)s);
    x = (lane & s) ? (((p >> s) & m) | (x & ~m)) : ((x & m) | ((p & m) << s));
  }
  return x;
}

template <typename LW>
__global__ __launch_bounds__(kPsThreads) void prefix_summary_kernel(const LW* __restrict__ act_t, uint32_t n_pods, uint32_t* status, KIndex ix,
                                                                    const uint8_t* __restrict__ reqs, uint32_t stride, uint32_t n_reqs,
                                                                    const uint64_t* __restrict__ mask, uint4* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wib = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  const uint32_t hwords = (stride - 8u) / 8u, J = (n_pods + 63u) / 64u;
  const uint32_t step = gridDim.x * wpb;
  auto fetch = [&](uint32_t r) -> PsFetch {
    const uint64_t* row = (const uint64_t*)(reqs + (size_t)r * stride);
    PsFetch f;
    f.hdr = row[0];
    f.h = lane < hwords ? row[1u + lane] : 0ull;
    f.m = (mask && lane < J) ? mask[(size_t)r * J + lane] : 0ull;
    return f;
  };

  uint32_t r = blockIdx.x * wpb + wib;
  if (r >= n_reqs) return;
  const LW open = (LW)(valid_word<LW>(n_pods, (int)lane) & act_t[lane]);      // the unmasked candidates: does not depend on the request
  const LW* bm = (const LW*)ix.bitmaps;
  PsFetch nxt = fetch(r);
  for (; r < n_reqs; r += step) {
    const PsFetch cur = nxt;
    if (r + step < n_reqs) nxt = fetch(r + step);                      // (wave-uniform)
    const uint64_t* row = (const uint64_t*)(reqs + (size_t)r * stride);
    const int32_t adapter = (int32_t)(uint32_t)cur.hdr;
    const uint32_t nb = (uint32_t)(cur.hdr >> 32);
    const bool bad = nb > hwords || adapter < -1 || adapter >= (int32_t)EPPK_MAX_ADAPTERS;
    if (__builtin_expect(bad, 0) && lane == 0u) atomicOr(status, kStatusBadRow);
    const uint32_t nbe = (uint32_t)__builtin_amdgcn_readfirstlane((int)((bad || ix.slots == 0u) ? 0u : nb));      // blocks to walk

    LW c[kPsPlanes];
#pragma unroll
    for (int b = 0; b < kPsPlanes; ++b) c[b] = 0;
    uint32_t walk = 0u;
    uint64_t h = cur.h;
    for (uint32_t t0 = 0u; t0 < nbe; t0 += 64u) {                      // one trip unless the row is longer than 64 blocks
      const bool act = t0 + lane < nbe;
      const uint32_t slot = probe(ix, h, act);
      const uint64_t miss = __ballot(act && slot == kNotFound);
      const uint32_t nloc = nbe - t0 < 64u ? nbe - t0 : 64u;
      const uint32_t stop1 = miss ? (uint32_t)__builtin_ctzll(miss) : nloc;
      const bool front = lane < stop1;
      uint32_t d[16];
      load_line16<false>(ix.lists_all + (size_t)(front ? slot : ix.slots + 2u) * kListDwords, d);      // (others: the all-zero row's empty line)
      const uint32_t cnt = d[3];
      const uint64_t empty = __ballot(front && cnt == 0u);
      const uint32_t stop = empty ? (uint32_t)__builtin_ctzll(empty) : stop1;
      const uint64_t in_front = stop >= 64u ? ~0ull : (1ull << stop) - 1ull;

      // runs of equal listed sets: lane i against lane i - 1 of its DPP row (lane 0 of a row compares with itself and starts a run)
      bool same = (lane & 15u) != 0u && cnt - 1u < kListCap;
#pragma unroll
      for (uint32_t w = 0; w < kListDwords; ++w)                        // the count (dword 3) and the id dwords 0..2, 4..6, 8..10, 12..14
        if (w == 3u || (w & 3u) != 3u) {                                // (every lane takes part in every shift: no && in front of it)
          const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp((int)d[w], (int)d[w], 0x111, 0xf, 0xf, false);
          same = same & (d[w] == prev);
        }
      uint64_t heads = in_front & ~__ballot(same);                      // first lane of every run in front of the stop
      while (heads != 0ull) {
        const uint32_t b = (uint32_t)__builtin_ctzll(heads);
        heads &= heads - 1ull;
        const uint32_t m = (heads ? (uint32_t)__builtin_ctzll(heads) : stop) - b;
        const uint32_t cb = (uint32_t)__builtin_amdgcn_readlane((int)cnt, (int)b);
        LW s = 0;
        if (cb > kListCap) s = bm[(size_t)(uint32_t)__builtin_amdgcn_readlane((int)slot, (int)b) * 64u + lane];
        else ps_set_from_line<LW>(d, b, cb, lane, s);
        ps_add_times<LW>(c, s, m);
      }
      walk += stop;
      if (stop < 64u || nbe <= t0 + 64u) break;                         // a miss, an empty set, or the row's end
      h = t0 + 64u + lane < nbe ? row[1u + t0 + 64u + lane] : 0ull;
    }

    LW cand = open;
    if (mask) cand &= (LW)ps_transpose(cur.m, lane);
    uint32_t best = 0u;
#pragma unroll
    for (int b = kPsPlanes - 1; b >= 0; --b) {
      const LW t = cand & c[b];
      if (__ballot(t != 0) != 0ull) { cand = t; best |= 1u << b; }
    }
    uint32_t holders = 0u, first = kPsNone;
    if (best != 0u) {                                                   // (wave-uniform) cand: the candidates with matched == best
      holders = ps_wave_sum((uint32_t)__builtin_popcountll((uint64_t)cand));
      first = wave_min_u32(cand != 0 ? (uint32_t)__builtin_ctzll((uint64_t)cand) * 64u + lane : kPsNone);
    }
    if (lane == 0u) out[r] = make_uint4(walk, best, holders, first);
  }
}

// The select pass of eppk_pick_hybrid (SEMANTICS.md §3m): a thread per list entry.  A warm row (best >= min_hit) keeps what the top-k pass
// wrote into pick / score; a cold row takes the rendezvous-scored pass's entries out of the context's scratch.  Thread 0 of a row's k
// writes its route byte.
__global__ void hybrid_select_kernel(const uint4* __restrict__ sum, uint32_t min_hit, uint32_t n_reqs, uint32_t k, const int32_t* __restrict__ cold_pick,
                                     const double* __restrict__ cold_score, int32_t* __restrict__ pick, double* __restrict__ score,
                                     uint8_t* __restrict__ route) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_reqs * k) return;
  const uint32_t r = i / k;
  const bool warm = sum[r].y >= min_hit;
  if (!warm) {
    pick[i] = cold_pick[i];
    if (score) score[i] = cold_score[i];
  }
  if (route && i == r * k) route[r] = warm ? 1u : 0u;
}

}  // namespace eppk

#endif  // EPPK_PREFIX_SUMMARY_HIP_H
