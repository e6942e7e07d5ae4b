// eppk_sfair.hip.h — fair shares between flows counted in COST UNITS: the rows ordered by carried service (SEMANTICS.md §3i;
// include/eppk.h eppk_sfair_resolve_device).
//
// Included by eppk.hip alone, behind eppk_wfair.hip.h.  Nothing of eppk_wfair.hip.h, eppk_fair.hip.h, eppk_bounded.hip.h,
// eppk_banded.hip.h or eppk_costed.hip.h is edited: fair_offsets_kernel and the count / scan / assign / finish kernels are launched as
// they are.  The kernels here write ANOTHER permutation into the layout those walk (perm, seg[0 .. 8]), a key, an effective band byte and
// a charge per row, and behind the finish the cost units every (band, flow) was served.
//
// Every flow has a WEIGHT w (u16; NULL: 1) and every (band, flow) the SERVICE s it got in earlier batches, in cost units (u32; NULL: 0).
// A row is IN THE ORDER iff band < n_bands, flow < n_flows and w[flow] >= 1; its key is g = band * n_flows + flow; its CHARGE is its
// cost if that is 1 .. EPPK_MAX_COST and 0 otherwise (NULL costs: 1); S = s[g] + the charges of the rows in front of it in the batch
// with the same key; its TAG = S / w[flow] (floor, 64 bits) -- the start tag of start-time fair queuing.  Band b's rows are placed by
// (tag - base[b], flow, q) ascending, base[b] the band's least tag, q the row's turn (§3g).  There is no closed form for that place
// (where a flow's running cost crosses a tag depends on every cost in front): the rows are SORTED, by a stable least-significant-digit
// radix sort of
//     sort key = band : 3 | tag - base[band] : 42 | flow : 10          (55 bits; a row that is not in the order: all 55 ones)
// in five passes of 11 bits.  tag - base < 2^32 + n_reqs * 2^24 <= 2^32 + 2^41 < 2^42 - 1 for n_reqs <= EPPK_SFAIR_MAX_REQS, so nothing
// is clamped and the key of a row out of the order is above every other.  The sort is stable and starts from batch order, so rows of
// one (band, tag, flow) stay in batch order, which IS ascending q: q is never computed.  The band is the top digit's top bits, so
// fair_offsets_kernel's seg[0 .. 8] describes the result; the rows out of the order land behind seg[8], where no round kernel walks.
//
//   sfair_stage_kernel     the caller's weights and service -> the context's own memory (NULL: ones, zeros); taken[] := 0, base[] := ~0
//   sfair_hist_kernel      per chunk, over the keys, the rows (32-bit LDS adds) and the charges (64-bit LDS adds) -> fh[chunk][G],
//                          ch[chunk][G]; per row its key, effective band byte and charge: the caller's band, flow and cost arrays are
//                          read exactly once
//   fair_offsets_kernel    (eppk_fair.hip.h, as it is) over fh: seg[]
//   sfair_offsets_kernel   the same cut of the chunk axis -- 16 segments of ceil(n_chunks / 16) chunks, trips of eight -- over ANY count
//                          of keys and a 32- or 64-bit word: the charges over the G keys (64 bits), the five passes' digit histograms
//                          over 2 048 digit values (32 bits)
//   sfair_tag_kernel       one wavefront per chunk, 64 rows per trip in ascending order: wfair_scatter_kernel's ballot loop per distinct
//                          key with a carried 64-bit charge sum per key, a lane's share the masked wavefront scan of
//                          costed_wave_round; one 64-bit division per row; tag[row]; base[band] by an LDS minimum per workgroup and
//                          one 64-bit atomic minimum per band and workgroup
//   sfair_digit_kernel     pass p, per chunk of PLACES of the current permutation (pass 0: the identity): the digit histogram
//   sfair_sort_kernel      pass p, one wavefront per chunk, 64 places per trip in ascending order.  A lane finds its wave-mates with the
//                          same digit by 11 ballots, one per digit bit, each ANDed or AND-NOTed into a peer mask; its place is the
//                          digit's running LDS counter + popcount(peers & below); the lowest peer adds popcount(peers).  No loop whose
//                          trip count depends on the digits, nobody waits for a wave-mate
//   sfair_taken_kernel     behind the finish: per chunk 64-bit LDS sums over the keys of the charges of the rows with
//                          out_pick != EPPK_NO_PICK, added into taken[G]
//   sfair_carry_kernel     service[g] := min(2^32 - 1, s[g] + taken[g])
// As everywhere in the resolves no atomic's return value is read: every atomic is a count, a sum or a minimum.
// Not here: costs per entry (the order needs one cost per row before any list is read); a one-launch form; assumed load.
#ifndef EPPK_SFAIR_HIP_H
#define EPPK_SFAIR_HIP_H

#include "eppk_wfair.hip.h"

namespace eppk {

constexpr uint32_t kSfairDigitBits = 11u, kSfairDigits = 1u << kSfairDigitBits, kSfairPasses = 5u;
constexpr uint64_t kSfairKeyOut = (1ull << (kSfairDigitBits * kSfairPasses)) - 1ull;      // 55 ones: a row that is not in the order
constexpr uint64_t kSfairNoTag = ~0ull;
// 64-bit words of the context's own tables (eppk_ctx::d_sf): base[EPPK_MAX_BANDS] | taken[kFairMaxKeys], then as 32-bit words
// s[kFairMaxKeys] | w[EPPK_MAX_FLOWS], then the areas the host-buffer forms upload into: service[kFairMaxKeys] | weights (u16, two to a word)
constexpr uint32_t kSfairBase = 0u, kSfairTaken = EPPK_MAX_BANDS, kSfairWords32 = 2u * (kSfairTaken + kFairMaxKeys);
constexpr uint32_t kSfairS = kSfairWords32, kSfairW = kSfairS + kFairMaxKeys, kSfairHostS = kSfairW + EPPK_MAX_FLOWS,
                   kSfairHostW = kSfairHostS + kFairMaxKeys, kSfairWords = (kSfairHostW + EPPK_MAX_FLOWS / 2u + 1u) / 2u;      // (64-bit words)
// dynamic LDS: sfair_hist_kernel charges[G] (8 bytes) + rows[G]; sfair_tag_kernel min[8] + sums[G] (8 bytes) + w[n_flows];
// sfair_taken_kernel sums[G] (8 bytes)
constexpr size_t sfair_hist_lds(size_t G) { return G * 12u; }
constexpr size_t sfair_tag_lds(size_t G, size_t n_flows) { return EPPK_MAX_BANDS * 8u + G * 8u + n_flows * 4u; }
constexpr size_t sfair_taken_lds(size_t G) { return G * 8u; }
constexpr size_t kSfairHistMaxLds = sfair_hist_lds(kFairMaxKeys), kSfairTagMaxLds = sfair_tag_lds(kFairMaxKeys, EPPK_MAX_FLOWS);

// Grid-stride over the keys: own copies of service and weights, taken[] zeroed, base[] at the top.
__global__ __launch_bounds__(kBoundThreads) void sfair_stage_kernel(const uint16_t* __restrict__ weight, const uint32_t* __restrict__ service, uint32_t n_bands,
                                                                    uint32_t n_flows, uint32_t* __restrict__ w_own, uint32_t* __restrict__ s_own,
                                                                    uint64_t* __restrict__ taken, uint64_t* __restrict__ base) {
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  const uint32_t G = n_bands * n_flows, tid = blockIdx.x * kBoundThreads + threadIdx.x;
  if (tid < EPPK_MAX_BANDS) base[tid] = kSfairNoTag;
  for (uint32_t g = tid; g < G; g += gridDim.x * kBoundThreads) {
    s_own[g] = service ? service[g] : 0u;
    taken[g] = 0ull;
    if (g < n_flows) w_own[g] = weight ? (uint32_t)weight[g] : 1u;
  }
}

// A workgroup per chunk (grid-stride), 12 * G bytes of dynamic LDS: row `chunk` of fh and of ch, and key[] / eband[] / charge[] of the
// chunk's rows.  w_own: sfair_stage_kernel's copy.
__global__ __launch_bounds__(kBoundThreads) void sfair_hist_kernel(const uint8_t* __restrict__ band, const uint16_t* __restrict__ flow,
                                                                   const uint32_t* __restrict__ cost, const uint32_t* __restrict__ w_own, uint32_t n_reqs,
                                                                   uint32_t n_bands, uint32_t n_flows, uint32_t chunk, uint32_t n_chunks, uint32_t* __restrict__ fh,
                                                                   uint64_t* __restrict__ ch, uint16_t* __restrict__ key, uint8_t* __restrict__ eband,
                                                                   uint32_t* __restrict__ charge) {
  extern __shared__ unsigned long long s_sfair_hist[];                // sized by the launch: s_c[G] (8 bytes each), s_h[G]
  const uint32_t G = n_bands * n_flows;
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  unsigned long long* const s_c = s_sfair_hist;
  uint32_t* const s_h = (uint32_t*)(s_sfair_hist + G);
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    for (uint32_t g = threadIdx.x; g < G; g += kBoundThreads) { s_h[g] = 0u; s_c[g] = 0ull; }
    __syncthreads();
    const uint64_t r0 = (uint64_t)c * chunk, r1 = r0 + chunk < n_reqs ? r0 + chunk : n_reqs;
    for (uint64_t r = r0 + threadIdx.x; r < r1; r += kBoundThreads) {
      const uint32_t b = band_of(band, r), f = flow ? (uint32_t)flow[r] : 0u, c0 = cost ? cost[r] : 1u;
      const bool in = b < n_bands && f < n_flows && w_own[f < n_flows ? f : 0u] >= 1u;
      const uint32_t g = b * n_flows + f, v = in && cost_ok(c0) ? c0 : 0u;           // a bad cost holds its place and is charged nothing
      key[r] = (uint16_t)(in ? g : kFairNoKey);
      eband[r] = (uint8_t)(in ? b : kFairBadBand);
      charge[r] = v;
      if (in) atomicAdd(&s_h[g], 1u);                                 // (a count: the result of the add is not read)
      if (v) atomicAdd(&s_c[g], (unsigned long long)v);               // (a sum, g < G: not read either)
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < G; g += kBoundThreads) { fh[(size_t)c * G + g] = s_h[g]; ch[(size_t)c * G + g] = s_c[g]; }
    __syncthreads();
  }
}

// fair_offsets_kernel's scan over ANY count of keys K and a word T of 32 or 64 bits: a workgroup per kBoundScanPods keys (grid-stride), a
// thread per (chunk segment, key); h[c][x] := the sum of key x over the chunks in front of c; total[x] (nullable) = its sum over all chunks.
template <class T>
__global__ __launch_bounds__(kBoundScanSegs * kBoundScanPods) void sfair_offsets_kernel(T* h, uint32_t n_chunks, uint32_t K, T* __restrict__ total) {
  __shared__ T s_sum[kBoundScanSegs][kBoundScanPods];
  const uint32_t lp = threadIdx.x % kBoundScanPods, sg = threadIdx.x / kBoundScanPods;
  const uint32_t seg_len = (n_chunks + kBoundScanSegs - 1u) / kBoundScanSegs;
  const uint32_t c0 = sg * seg_len < n_chunks ? sg * seg_len : n_chunks, c1 = c0 + seg_len < n_chunks ? c0 + seg_len : n_chunks;
  for (uint32_t xb = blockIdx.x * kBoundScanPods; xb < K; xb += gridDim.x * kBoundScanPods) {          // (uniform over the workgroup)
    const uint32_t x = xb + lp;
    const bool live = x < K;
    T sum = 0;
    if (live) {
#pragma unroll 8
      for (uint32_t c = c0; c < c1; ++c) sum += h[(size_t)c * K + x];
    }
    s_sum[sg][lp] = sum;
    __syncthreads();
    T run = 0, all = 0;
    for (uint32_t s2 = 0; s2 < kBoundScanSegs; ++s2) {
      const T v = s_sum[s2][lp];
      if (s2 < sg) run += v;
      all += v;
    }
    if (live) {
      for (uint32_t c = c0; c < c1; c += 8u) {                       // eight loads in flight, then their prefix
        T v[8];
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) v[i] = c + i < c1 ? h[(size_t)(c + i) * K + x] : (T)0;
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i)
          if (c + i < c1) { h[(size_t)(c + i) * K + x] = run; run += v[i]; }
      }
      if (sg == 0u && total) total[x] = all;
    }
    __syncthreads();
  }
}

// A workgroup of ONE wavefront per chunk (grid-stride), with sfair_tag_lds bytes of dynamic LDS: s_min, the least tag per band this
// workgroup has seen; s_sum, for every key its carried service plus the charges of its rows in front of the place the wavefront is at;
// s_w, the weights.  Every index into s_sum is < G and every index into s_w < n_flows: a key read from key[] is either < G or
// kFairNoKey, and is checked against G all the same.  A key in the order has a weight >= 1; the division is guarded all the same.
__global__ __launch_bounds__(64) void sfair_tag_kernel(const uint16_t* __restrict__ key, const uint32_t* __restrict__ charge, uint32_t n_reqs, uint32_t n_bands,
                                                       uint32_t n_flows, uint32_t chunk, uint32_t n_chunks, const uint64_t* __restrict__ ch,
                                                       const uint32_t* __restrict__ s_own, const uint32_t* __restrict__ w_own, uint64_t* __restrict__ tag,
                                                       uint64_t* __restrict__ base) {
  extern __shared__ unsigned long long s_sfair_tag[];                 // sized by the launch: s_min[8], s_sum[G], s_w[n_flows]
  const uint32_t G = n_bands * n_flows;
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  unsigned long long* const s_min = s_sfair_tag;
  unsigned long long* const s_sum = s_sfair_tag + EPPK_MAX_BANDS;
  uint32_t* const s_w = (uint32_t*)(s_sum + G);
  const uint32_t lane = threadIdx.x & 63u;
  if (lane < EPPK_MAX_BANDS) s_min[lane] = kSfairNoTag;
  for (uint32_t f = lane; f < n_flows; f += 64u) s_w[f] = w_own[f];
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    __syncthreads();                                                  // (one wavefront: the trips of the chunk before are done with s_sum)
    for (uint32_t g = lane; g < G; g += 64u) s_sum[g] = (unsigned long long)s_own[g] + ch[(size_t)c * G + g];
    __syncthreads();
    const uint64_t r0 = (uint64_t)c * chunk, r1 = r0 + chunk < n_reqs ? r0 + chunk : n_reqs;
    for (uint64_t t0 = r0; t0 < r1; t0 += 64u) {
      const uint64_t r = t0 + lane;
      const uint32_t g = r < r1 ? (uint32_t)key[r] : kFairNoKey;
      const bool in = g < G;
      const uint32_t v = in ? charge[r] : 0u;
      uint64_t S = 0ull;
      for (uint64_t todo = __ballot(in); todo != 0ull;) {             // (wave-uniform: one trip of this loop per distinct key)
        const int first = (int)__builtin_ctzll(todo);
        const uint32_t g0 = (uint32_t)__shfl((int)g, first);          // (< G: the lane `first` is in the ballot)
        const bool mine = in && g == g0;
        const uint64_t m = __ballot(mine);
        const uint64_t before = s_sum[g0];                            // (every lane reads the same word: a broadcast)
        uint32_t incl = mine ? v : 0u;                                // inclusive prefix over the lanes: < 64 * 2^24, exact in 32 bits
        if ((m & (m - 1ull)) != 0ull) {                               // (uniform: more than one row of the key in this trip)
#pragma unroll
          for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
          }
        }
        const uint32_t total = __shfl(incl, 63 - (int)__builtin_clzll(m));       // the last row's inclusive prefix is the trip's total
        if (mine) S = before + (uint64_t)(incl - v);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if ((int)lane == first) s_sum[g0] = before + total;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        todo &= ~m;
      }
      if (in) {
        const uint32_t b = g / n_flows, f = g - b * n_flows;          // (b < n_bands <= 8, f < n_flows)
        const uint64_t wf = s_w[f], t = S / (wf ? wf : 1ull);
        tag[r] = t;
        atomicMin(&s_min[b], (unsigned long long)t);                  // (a minimum: the result is not read)
      } else if (r < r1) {
        tag[r] = 0ull;
      }
    }
  }
  __syncthreads();
  if (lane < n_bands && s_min[lane] != kSfairNoTag) atomicMin((unsigned long long*)&base[lane], s_min[lane]);      // (not read before the next launch)
}

// The 55-bit sort key of a row from its key, effective band byte and tag (the module comment).  base[b] <= tag for every row of band b
// in the order; the fields are masked to their widths all the same.
__device__ __forceinline__ uint64_t sfair_sort_key(uint64_t r, const uint16_t* __restrict__ key, const uint8_t* __restrict__ eband,
                                                   const uint64_t* __restrict__ tag, const uint64_t* __restrict__ base, uint32_t n_flows, uint32_t G) {
  const uint32_t g = (uint32_t)key[r], b = (uint32_t)eband[r];
  if (g >= G || b >= EPPK_MAX_BANDS) return kSfairKeyOut;
  const uint64_t d = tag[r] - base[b];
  return ((uint64_t)b << 52) | ((d & ((1ull << 42) - 1ull)) << 10) | (uint64_t)((g - b * n_flows) & 1023u);
}

// A workgroup per chunk of places (grid-stride): row `chunk` of dh = the places of the chunk per value of digit `pass`.  src: the
// current permutation, place -> row (NULL: the identity); a row it names is checked against n_reqs.
__global__ __launch_bounds__(kBoundThreads) void sfair_digit_kernel(const uint32_t* __restrict__ src, uint32_t pass, const uint16_t* __restrict__ key,
                                                                    const uint8_t* __restrict__ eband, const uint64_t* __restrict__ tag,
                                                                    const uint64_t* __restrict__ base, uint32_t n_reqs, uint32_t n_bands, uint32_t n_flows,
                                                                    uint32_t chunk, uint32_t n_chunks, uint32_t* __restrict__ dh) {
  __shared__ uint32_t s_h[kSfairDigits];
  const uint32_t G = n_bands * n_flows, shift = pass * kSfairDigitBits;
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS || pass >= kSfairPasses) return;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    for (uint32_t x = threadIdx.x; x < kSfairDigits; x += kBoundThreads) s_h[x] = 0u;
    __syncthreads();
    const uint64_t i0 = (uint64_t)c * chunk, i1 = i0 + chunk < n_reqs ? i0 + chunk : n_reqs;
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += kBoundThreads) {
      const uint32_t r = src ? src[i] : (uint32_t)i;
      const uint64_t sk = r < n_reqs ? sfair_sort_key(r, key, eband, tag, base, n_flows, G) : kSfairKeyOut;
      atomicAdd(&s_h[(uint32_t)(sk >> shift) & (kSfairDigits - 1u)], 1u);      // (a count: the result of the add is not read)
    }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < kSfairDigits; x += kBoundThreads) dh[(size_t)c * kSfairDigits + x] = s_h[x];
    __syncthreads();
  }
}

// A workgroup of ONE wavefront per chunk of places (grid-stride).  s_first[x]: the places of all digit values below x (an exclusive
// scan of total[], once per workgroup); s_run[x]: where the next place of digit x goes -- s_first[x] + dh[chunk][x] (the places of x
// in the chunks in front) + those of the chunk's earlier trips.  Places are taken 64 per trip in ascending order and a lane's rank among
// its peers is its lane order, so equal digits keep their order: the pass is stable.  Every destination is < n_reqs (the histograms
// count exactly the places read here), and is checked all the same.
__global__ __launch_bounds__(64) void sfair_sort_kernel(const uint32_t* __restrict__ src, uint32_t pass, const uint16_t* __restrict__ key,
                                                        const uint8_t* __restrict__ eband, const uint64_t* __restrict__ tag, const uint64_t* __restrict__ base,
                                                        uint32_t n_reqs, uint32_t n_bands, uint32_t n_flows, uint32_t chunk, uint32_t n_chunks,
                                                        const uint32_t* __restrict__ dh, const uint32_t* __restrict__ total, uint32_t* __restrict__ dst) {
  __shared__ uint32_t s_first[kSfairDigits], s_run[kSfairDigits];
  const uint32_t G = n_bands * n_flows, shift = pass * kSfairDigitBits;
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS || pass >= kSfairPasses) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t below = (1ull << lane) - 1ull;
  {   // the exclusive scan of total[0 .. 2048): lane l sums digits [32 l, 32 l + 32), a wavefront scan of the 64 sums, then the 32 again
    constexpr uint32_t per = kSfairDigits / 64u;
    uint32_t sum = 0u;
    for (uint32_t i = 0; i < per; ++i) sum += total[lane * per + i];
    uint32_t incl = sum;
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    uint32_t run = incl - sum;
    for (uint32_t i = 0; i < per; ++i) { s_first[lane * per + i] = run; run += total[lane * per + i]; }
  }
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    __syncthreads();                                                  // (one wavefront: the trips of the chunk before are done with s_run)
    for (uint32_t x = lane; x < kSfairDigits; x += 64u) s_run[x] = s_first[x] + dh[(size_t)c * kSfairDigits + x];
    __syncthreads();
    const uint64_t i0 = (uint64_t)c * chunk, i1 = i0 + chunk < n_reqs ? i0 + chunk : n_reqs;
    for (uint64_t t0 = i0; t0 < i1; t0 += 64u) {
      const uint64_t i = t0 + lane;
      const bool live = i < i1;
      const uint32_t r = live ? (src ? src[i] : (uint32_t)i) : 0u;
      const uint64_t sk = live && r < n_reqs ? sfair_sort_key(r, key, eband, tag, base, n_flows, G) : kSfairKeyOut;
      const uint32_t x = (uint32_t)(sk >> shift) & (kSfairDigits - 1u);
      uint64_t peers = __ballot(live);                                // the match: the live lanes whose digit equals mine, bit by bit
#pragma unroll
      for (uint32_t bit = 0; bit < kSfairDigitBits; ++bit) {
        const bool one = (x >> bit) & 1u;
        const uint64_t ones = __ballot(one);
        peers &= one ? ones : ~ones;
      }
      const uint32_t at = s_run[x] + (uint32_t)__popcll(peers & below);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (live && (peers & below) == 0ull) s_run[x] += (uint32_t)__popcll(peers);      // the lowest peer: one writer per digit value
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (live && at < n_reqs) dst[at] = r;
    }
  }
}

// A workgroup per chunk (grid-stride), behind the finish, 8 * G bytes of dynamic LDS: taken[g] += the charges of the chunk's rows of key
// g that hold an endpoint.
__global__ __launch_bounds__(kBoundThreads) void sfair_taken_kernel(const uint16_t* __restrict__ key, const uint32_t* __restrict__ charge,
                                                                    const int32_t* __restrict__ out_pick, uint32_t n_reqs, uint32_t n_bands, uint32_t n_flows,
                                                                    uint32_t chunk, uint32_t n_chunks, uint64_t* __restrict__ taken) {
  extern __shared__ unsigned long long s_sfair_taken[];               // sized by the launch: G sums
  const uint32_t G = n_bands * n_flows;
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    for (uint32_t g = threadIdx.x; g < G; g += kBoundThreads) s_sfair_taken[g] = 0ull;
    __syncthreads();
    const uint64_t r0 = (uint64_t)c * chunk, r1 = r0 + chunk < n_reqs ? r0 + chunk : n_reqs;
    for (uint64_t r = r0 + threadIdx.x; r < r1; r += kBoundThreads) {
      const uint32_t g = (uint32_t)key[r], v = charge[r];
      if (g < G && v && out_pick[r] != EPPK_NO_PICK) atomicAdd(&s_sfair_taken[g], (unsigned long long)v);      // (a sum: the result is not read)
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < G; g += kBoundThreads) {
      const unsigned long long v = s_sfair_taken[g];
      if (v) atomicAdd((unsigned long long*)&taken[g], v);            // (g < G; sums commute, and nobody reads taken before the next launch)
    }
    __syncthreads();
  }
}

// Grid-stride over the keys: the service handed back, saturating.  taken[g] <= n_reqs * 2^24 < 2^42: the sum stays far inside 64 bits.
__global__ __launch_bounds__(kBoundThreads) void sfair_carry_kernel(const uint32_t* __restrict__ s_own, const uint64_t* __restrict__ taken, uint32_t n_bands,
                                                                    uint32_t n_flows, uint32_t* __restrict__ service) {
  if (n_bands > EPPK_MAX_BANDS || n_flows > EPPK_MAX_FLOWS) return;
  const uint32_t G = n_bands * n_flows;
  for (uint32_t g = blockIdx.x * kBoundThreads + threadIdx.x; g < G; g += gridDim.x * kBoundThreads) {
    const uint64_t sum = (uint64_t)s_own[g] + taken[g];
    service[g] = sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum;
  }
}

}  // namespace eppk
#endif
