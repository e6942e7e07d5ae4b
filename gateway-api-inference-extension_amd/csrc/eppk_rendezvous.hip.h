// eppk_rendezvous.hip.h — the picker "rendezvous" (highest-random-weight hashing; SEMANTICS.md §3j; include/eppk.h eppk_pick_rendezvous).
//
// Included by eppk.hip alone: the thirty pick units do not see this file, so a change here rebuilds one unit.
//
// The list of request r is its candidates sorted by h(r, p) = fmix32(a[r] ^ c[p]) descending, ties by p ascending, cut at k.  The kernel is
// nothing but that pair hash, so everything around it is shared or hoisted:
//   prologue   the workgroup computes c[p] = fold(splitmix64(pod_key[p])) for every pod once and keeps it in LDS, 65 words per row of 64
//              pods: the pair loop reads row j at lane stride 1, the rescan of a round reads COLUMN w at stride 65 -- both without a
//              bank conflict.  The pod keys of a trip are loaded together before the first is mixed.  The snapshot's active-set word l
//              (pods 64l .. 64l+63, natural layout) lives in lane l's registers: no LDS copy, a row's word comes out by v_readlane.
//   a pass     one wavefront takes kRdvReqs = 8 consecutive requests.  Lane i < 8 loads request i's affinity key (session form: key[r];
//              prefix form: the row header, then hash[min(depth, n_blocks) - 1] -- inside this kernel, no launch in front), mixes it and
//              the eight a[] go to SGPRs (v_readlane): a pair costs no register for its request.  Lane l loads word l of each of the
//              eight mask rows (one coalesced 8-byte load per row) and ANDs the active word in: m[i], 2 VGPRs per request.
//   pair loop  lane l owns the pods 64j + l.  Per j: one ds_read of c, one ~p, then for each of the eight requests word j of m[i] by
//              v_readlane into an SGPR pair -- which IS the lane mask of "pod 64j + lane is a candidate" -- the hash (xor + the eight
//              operations of fmix32, two of them multiplies; h ^ h >> 16 compiles to one SDWA v_xor), one 64-bit compare of
//              (h, ~p) against the lane's best and two v_cndmask under (compare AND mask word).  10 vector instructions per pair,
//              12 with a mask.  The lane's best is the 64-bit key h << 32 | ~p as two registers: unsigned order = (h descending,
//              p ascending), 0 = none yet (~p != 0).  Eight requests per pass: 8 x (2 best + 2 mask) = 32 VGPRs of state, 8 SGPRs
//              of a[]; the kernel takes 84 VGPRs (92 masked).  Sixteen requests per pass would go past 128 -- half the wavefronts
//              per SIMD -- to share one ds_read and one v_not among ~170 instructions instead of ~85.
//   round 0    the wavefront's maximum of h (six DPP steps), then of ~p among the lanes that hold it: both wave-uniform.
//   round i>0  only the winner's column w = p* mod 64 changed.  Lane t clears the pick's bit in its m[i] (t = p* / 64), then hashes pod
//              64t + w if bit w of ITS word m[i] is still set -- one hash per lane, the taken pods and the non-candidates drop out by
//              the same bit -- one (h, ~p) maximum gives lane w its new best, a second one the round's winner.  A round costs one
//              hash and four 32-bit reductions, not J hashes.
//   results    lane 8i + round keeps request i's entry; one pick store and one score store per pass.
// No atomics, no fence, nothing but vector stores.  A row out of range (prefix form) gets no candidates -- EPPK_NO_PICK / 0.0 in every
// entry -- and the sticky status word of the snapshot blob is set by a plain store of the one value that word ever holds.
// ONE geometry: 64 lanes per group of eight requests for every snapshot size (DESIGN.md §3.19 has the time of a 64-pod snapshot, where
// a pass is reductions only, and why no sub-wave instantiation was added).
#ifndef EPPK_RENDEZVOUS_HIP_H
#define EPPK_RENDEZVOUS_HIP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eppk_kernels.hip.h"

namespace eppk {

constexpr uint32_t kRdvReqs = 8u;        // requests per pass of a wavefront
constexpr uint32_t kRdvRow = 65u;        // LDS words per row of 64 pods (one word of padding: column reads are conflict-free)
constexpr uint32_t kRdvMaxWaves = 16u;   // wavefronts per workgroup at most

__host__ __device__ __forceinline__ constexpr size_t rdv_lds_bytes(uint32_t J) { return (size_t)J * kRdvRow * 4u; }

__device__ __forceinline__ uint32_t rdv_fold(uint64_t m) { return (uint32_t)(m ^ (m >> 32)); }
__device__ __forceinline__ uint32_t rdv_fmix32(uint32_t h) {     // the 32-bit murmur3 finaliser: a bijection
  h ^= h >> 16; h *= 0x85EBCA6Bu;
  h ^= h >> 13; h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}
// mask[lane] ? b : a, the mask a wave-uniform 64-bit word (an SGPR pair used as the lane mask it is: no shift, no compare)
__device__ __forceinline__ uint32_t rdv_select(uint32_t a, uint32_t b, uint64_t mask) {
  uint32_t r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(mask));
  return r;
}
__device__ __forceinline__ uint64_t rdv_readlane_u64(uint64_t v, uint32_t l) {
  return u64_of((uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l), (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max_u32(uint32_t v) {
  uint32_t o;
  if constexpr (ROW_MASK == 0xf) o = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, false);
  else o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false);
  return o > v ? o : v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {       // (wave_min_u32's steps)
  v = dpp_max_u32<0xB1, 0xf>(v);
  v = dpp_max_u32<0x4E, 0xf>(v);
  v = dpp_max_u32<0x141, 0xf>(v);
  v = dpp_max_u32<0x140, 0xf>(v);
  v = dpp_max_u32<0x142, 0xa>(v);
  v = dpp_max_u32<0x143, 0xc>(v);
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// The largest key h << 32 | np over the lanes, wave-uniform.  np differs between the lanes that hold a key and is 0 in a lane without one.
__device__ __forceinline__ void rdv_wave_best(uint32_t h, uint32_t np, uint32_t& hmax, uint32_t& npmax) {
  hmax = wave_max_u32(h);
  npmax = wave_max_u32(h == hmax ? np : 0u);
}

template <bool MASKED>
__global__ __launch_bounds__(1024) void pick_rendezvous_kernel(KSnap sn, const uint8_t* __restrict__ reqs, uint32_t stride, uint32_t n_reqs,
                                                               const uint64_t* __restrict__ key, uint32_t depth,
                                                               const uint64_t* __restrict__ pod_key, const uint64_t* __restrict__ cand_mask,
                                                               uint32_t k, uint64_t seed, int32_t* __restrict__ out_pick,
                                                               double* __restrict__ out_score) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_c[];       // [J][kRdvRow]: c[p] at p + p / 64
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wib = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  const uint32_t J = sn.J, np_all = J * 64u;

  // prologue: c[] of every pod, four pod keys per thread in flight before the first is mixed
  for (uint32_t p0 = 0; p0 < np_all; p0 += 4u * blockDim.x) {
    uint64_t pk[4];
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
      const uint32_t p = p0 + u * blockDim.x + threadIdx.x;
      pk[u] = (pod_key && p < sn.n_pods) ? pod_key[p] : (uint64_t)p;
    }
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
      const uint32_t p = p0 + u * blockDim.x + threadIdx.x;
      if (p < np_all) s_c[p + (p >> 6)] = rdv_fold(splitmix64(pk[u]));
    }
  }
  const uint64_t act = sn.nat[lane];            // existing AND active pods 64 * lane .. 64 * lane + 63 (0 from word J on)
  __syncthreads();

  const uint32_t n_pass = (n_reqs + kRdvReqs - 1u) / kRdvReqs;
  for (uint32_t q = blockIdx.x * wpb + wib; q < n_pass; q += gridDim.x * wpb) {
    const uint32_t rb = q * kRdvReqs;
    const uint32_t cnt = n_reqs - rb < kRdvReqs ? n_reqs - rb : kRdvReqs;

    // the affinity keys: lane i takes request rb + i
    uint64_t kv = 0;
    bool bad = false;
    if (lane < cnt) {
      if (key) {
        kv = key[rb + lane];
      } else {
        const uint64_t* row = (const uint64_t*)(reqs + (size_t)(rb + lane) * stride);
        const uint64_t hd = row[0];
        const int32_t adapter = (int32_t)(uint32_t)hd;
        const uint32_t nb = (uint32_t)(hd >> 32);
        bad = nb > (stride - 8u) / 8u || adapter < -1 || adapter >= (int32_t)EPPK_MAX_ADAPTERS;
        const uint32_t at = bad ? 0u : (depth < nb ? depth : nb);      // hash[at - 1] is word `at` of the row
        if (at) kv = row[at];
      }
    }
    const uint32_t av = rdv_fold(splitmix64(kv + seed * 0x9E3779B97F4A7C15ull));
    const uint64_t badm = __ballot(bad);
    if (__builtin_expect(badm != 0ull, 0) && lane == 0u)          // out-of-range row on the *_device entry point: flagged (eppk_launch_status)
      *(uint32_t*)(const_cast<uint8_t*>(sn.blob) + (sn.blob_bytes - kBlobStatusTail)) = kStatusBadRow;
    const uint32_t live = (cnt == kRdvReqs ? 0xFFu : (1u << cnt) - 1u) & ~(uint32_t)badm;     // bit i: request rb + i takes part

    uint32_t a[kRdvReqs];
    uint64_t m[kRdvReqs];
#pragma unroll
    for (uint32_t i = 0; i < kRdvReqs; ++i) {
      a[i] = (uint32_t)__builtin_amdgcn_readlane((int)av, (int)i);
      m[i] = 0ull;
      if ((live >> i) & 1u) {
        if (MASKED) m[i] = (lane < J ? cand_mask[(size_t)(rb + i) * J + lane] : 0ull) & act;
        else m[i] = act;
      }
    }

    // the pair loop: the lane's best key per request
    uint32_t bh[kRdvReqs], bn[kRdvReqs];
#pragma unroll
    for (uint32_t i = 0; i < kRdvReqs; ++i) bh[i] = bn[i] = 0u;
    for (uint32_t j = 0; j < J; ++j) {
      const uint32_t c = s_c[j * kRdvRow + lane];
      const uint32_t np = ~(j * 64u + lane);
      const uint64_t wu = MASKED ? 0ull : rdv_readlane_u64(act, j);
#pragma unroll
      for (uint32_t i = 0; i < kRdvReqs; ++i) {
        const uint64_t w = MASKED ? rdv_readlane_u64(m[i], j) : wu;
        const uint32_t h = rdv_fmix32(a[i] ^ c);
        const uint64_t take = __ballot(u64_of(np, h) > u64_of(bn[i], bh[i])) & w;
        bh[i] = rdv_select(bh[i], h, take);
        bn[i] = rdv_select(bn[i], np, take);
      }
    }

    // the k rounds; lane 8i + round keeps the entry
    uint32_t res_p = 0xFFFFFFFFu, res_h = 0u;
#pragma unroll
    for (uint32_t i = 0; i < kRdvReqs; ++i) {
      if (!MASKED && !((live >> i) & 1u)) bh[i] = bn[i] = 0u;       // (the unmasked pair loop does not look at m[])
      for (uint32_t rd = 0; rd < k; ++rd) {
        uint32_t hmax, npmax;
        rdv_wave_best(bh[i], bn[i], hmax, npmax);
        if (npmax == 0u) break;                                      // no candidate left: the rest of the list is padding
        const uint32_t p = ~npmax;
        if (lane == i * 8u + rd) { res_p = p; res_h = hmax; }
        if (rd + 1u == k) break;
        const uint32_t w = p & 63u;
        if (lane == (p >> 6)) m[i] &= ~(1ull << w);
        uint32_t kh = 0u, kn = 0u;
        if ((m[i] >> w) & 1ull) {                                    // lane t: pod 64t + w, if it is a candidate that no round has taken
          kh = rdv_fmix32(a[i] ^ s_c[lane * kRdvRow + w]);
          kn = ~(lane * 64u + w);
        }
        uint32_t ch, cn;
        rdv_wave_best(kh, kn, ch, cn);
        if (lane == w) { bh[i] = ch; bn[i] = cn; }
      }
    }
    {
      const uint32_t i = lane >> 3, rd = lane & 7u;
      if (rd < k && i < cnt) {
        const size_t at = (size_t)(rb + i) * k + rd;
        out_pick[at] = (int32_t)res_p;
        if (out_score) out_score[at] = (double)res_h * 0x1p-32;
      }
    }
  }
}

}  // namespace eppk

#endif  // EPPK_RENDEZVOUS_HIP_H
