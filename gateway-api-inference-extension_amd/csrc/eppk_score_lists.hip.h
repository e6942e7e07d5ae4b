// eppk_score_lists.hip.h — the scorer chain's totals for LISTED pods, ordered best first (SEMANTICS.md §3l; include/eppk.h eppk_score_lists).
//
// Included by eppk.hip alone, behind eppk_prefix_costs.hip.h, whose group split, broadcasts and block walk (pc_group, pc_group_bcast,
// pc_walk) this kernel shares: the question is list-major again -- k <= 8 named pods per request -- and the answer is the binary64 total of
// each (request, pod) pair as every exact route computes it (exact_chain + exact_total of eppk_kernels.hip.h, called unchanged).
//   split      a request takes a group of G lanes.  HAS_P (a PREFIX scorer in the chain and an index): G = pc_group(max_blocks), lane =
//              block, as in prefix_costs_kernel.  Otherwise there is no walk: G = 8, lane = list entry, eight requests per wavefront pass,
//              and the instantiation holds no probe code.  Persistent grid, 256 threads.
//   fetch      one pass AHEAD of its use, everything that depends on r alone: the header, lane i's hash i (HAS_P), list entry j in lane j
//              and -- masked, default candidate set, a QUEUE scorer in the chain -- word gl of the request's mask row.
//   gauges     as soon as the entries are known lane j asks for its pod's queue depth, kv utilisation, the {hi, lo} tier pair of (adapter
//              row, pod), the pod's word of the active set and of the mask row.  All of them are issued in front of the probe, so their
//              latency lies under the bucket -> list line chain of the walk.  (The entry's own mask word hangs on the entry, so it rides
//              here and not in the fetch: a dependent load there would hold up the pass in front.)
//   walk       pc_walk: matched[j] in lane j.
//   range      the QUEUE normalisers of the request.  Unmasked: KSnap::qrange.  EPPK_SCORE_WITHIN_LIST: minimum / maximum over the valid
//              entries, a shuffle reduction over the group's first eight lanes.  Masked: the group ANDs the mask row with the active set and
//              with the pods at the snapshot's minimum / maximum (KSnap::nat, G words per trip; the first trip's words wait in registers);
//              candidates at both extremes -> qrange, else the exact range over the row's set bits, four gauges in flight per lane
//              (exact_qrange<LW, true>'s loop, cut to the group).
//   totals     lane j: exact_total(chain, range, queue, kv, tier, clamp01(matched / n_blocks)).
//   sort       EPPK_SCORE_SORT: eight broadcasts of (total, pod) inside the group; lane j counts the entries that beat it (total
//              descending, pod ascending, position ascending; an invalid entry behind every valid one) and stores at that rank.
//   results    out_pick / out_score of a request are one contiguous run; out_pick may BE lists (a pass reads its entries one pass before
//              it stores them, and no other wavefront touches the row).
// No LDS, no atomics but the sticky status flag of a bad row.
#ifndef EPPK_SCORE_LISTS_HIP_H
#define EPPK_SCORE_LISTS_HIP_H

#include "eppk_prefix_costs.hip.h"

namespace eppk {

constexpr uint32_t kSlSort = 1u, kSlWithin = 2u;       // eppk.h: EPPK_SCORE_SORT, EPPK_SCORE_WITHIN_LIST
constexpr uint32_t kSlNoWalkGroup = 8u;                // G of the instantiations without a walk

// minimum / maximum over aligned runs of W lanes (every lane of the wavefront takes part)
template <uint32_t W>
__device__ __forceinline__ void sl_minmax(uint32_t& mn, uint32_t& mx) {
#pragma unroll
  for (uint32_t off = W / 2u; off >= 1u; off >>= 1) {
    const uint32_t omn = (uint32_t)__shfl_xor((int)mn, (int)off), omx = (uint32_t)__shfl_xor((int)mx, (int)off);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
  }
}

struct SlFetch { uint64_t hdr, h, m0; int32_t p; };

template <typename LW, uint32_t G, bool HAS_P>
__global__ __launch_bounds__(kPcThreads) void score_lists_kernel(KSnap sn, KIndex ix, KChain ch, const uint8_t* __restrict__ reqs, uint32_t stride,
                                                                 uint32_t n_reqs, const uint64_t* __restrict__ mask, const int32_t* lists, uint32_t k,
                                                                 uint32_t flags, int32_t* out_pick, double* out_score) {
  constexpr uint32_t NG = 64u / G;                                     // requests per pass
  constexpr uint64_t GM = G == 64u ? ~0ull : (1ull << (G & 63u)) - 1ull;
  const uint32_t lane = threadIdx.x & 63u, gl = lane & (G - 1u), gs = lane & ~(G - 1u);
  const uint32_t wib = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  const uint32_t hwords = (stride - 8u) / 8u, J = sn.J, n_pods = sn.n_pods;
  const uint32_t n_pass = (n_reqs + NG - 1u) / NG, step = gridDim.x * wpb;
  const ExactChain ec = exact_chain(ch);
  const bool sort = (flags & kSlSort) != 0u, within = (flags & kSlWithin) != 0u;
  const bool mrange = mask && ec.has_q && !within;                    // the normalisers come from the mask row
  const LW* thl_t = (const LW*)(sn.blob + SnapOff<LW>::thl);
  auto grp = [&](uint64_t m) -> uint64_t { return G == 64u ? m : (m >> gs) & GM; };     // the lane's group's part of a ballot
  auto fetch = [&](uint32_t q) -> SlFetch {
    const uint32_t r0 = q * NG + lane / G, r = r0 < n_reqs ? r0 : n_reqs - 1u;
    const uint64_t* row = (const uint64_t*)(reqs + (size_t)r * stride);
    SlFetch f;
    f.hdr = row[0];
    f.h = (HAS_P && gl < hwords) ? row[1u + gl] : 0ull;
    f.m0 = (mrange && gl < J) ? mask[(size_t)r * J + gl] : 0ull;
    f.p = gl < k ? lists[(size_t)r * k + gl] : EPPK_NO_PICK;
    return f;
  };

  uint32_t q = blockIdx.x * wpb + wib;
  if (q >= n_pass) return;
  // the first trip's words of the active set and of the pods at the snapshot's extremes: they do not depend on the request
  const bool w0 = mrange && gl < J;
  const uint64_t nat_a = w0 ? sn.nat[gl] : 0ull, nat_lo = w0 ? sn.nat[64u + gl] : 0ull, nat_hi = w0 ? sn.nat[128u + gl] : 0ull;
  SlFetch nxt = fetch(q);
  for (; q < n_pass; q += step) {
    const SlFetch cur = nxt;
    if (q + step < n_pass) nxt = fetch(q + step);                     // (wave-uniform)
    const uint32_t r = q * NG + lane / G;
    const bool live = r < n_reqs;
    const size_t rr = live ? r : n_reqs - 1u;
    const int32_t adapter = (int32_t)(uint32_t)cur.hdr;
    const uint32_t nb = (uint32_t)(cur.hdr >> 32);
    const bool bad = live && (nb > hwords || adapter < -1 || adapter >= (int32_t)EPPK_MAX_ADAPTERS);
    if (__builtin_expect(__ballot(bad) != 0ull, 0) && bad && gl == 0u) atomicOr(sn.status, kStatusBadRow);
    const uint32_t arow = (adapter >= 0 && adapter < (int32_t)EPPK_MAX_ADAPTERS) ? (uint32_t)adapter : 128u;

    // lane j: the gauges of entry j, asked for in front of the probe
    const bool inr = live && !bad && cur.p >= 0 && (uint32_t)cur.p < n_pods;
    const uint32_t p = inr ? (uint32_t)cur.p : 0u;
    uint64_t actw = 0ull, mw = ~0ull;
    uint32_t qd = 0u;
    double kvu = 0.0;
    LW th = 0, tl = 0;
    if (inr) {
      actw = sn.nat[p >> 6];
      if (mask) mw = mask[rr * J + (p >> 6)];
      qd = sn.queue[p];
      kvu = sn.kv[p];
      const LW* t2 = thl_t + (size_t)arow * 128u + (p & 63u) * 2u;
      th = t2[0]; tl = t2[1];
    }
    const bool valid = inr && ((actw & mw) >> (p & 63u)) & 1ull;      // p is a candidate of the request
    const uint32_t pv = valid ? p : kPcNoPod;
    uint32_t P[EPPK_MAX_TOPK];
    if (HAS_P || sort) pc_group_bcast_all<G>(pv, lane, P, std::make_index_sequence<EPPK_MAX_TOPK>{});

    uint32_t matched = 0u;
    if constexpr (HAS_P) {
      const uint32_t nbe = (bad || !live) ? 0u : nb;
      matched = pc_walk<LW, G>(ix, (const uint64_t*)(reqs + rr * stride), cur.h, nbe, P, k, lane);
    }

    // the QUEUE normalisers of the request
    uint32_t qmin = sn.qrange[0], qmax = sn.qrange[1];
    if (ec.has_q && within) {
      qmin = valid ? qd : 0xFFFFFFFFu; qmax = valid ? qd : 0u;
      sl_minmax<8u>(qmin, qmax);
    } else if (mrange) {
      uint64_t a = cur.m0 & nat_a;
      bool any = a != 0ull, lo = (a & nat_lo) != 0ull, hi = (a & nat_hi) != 0ull;
      for (uint32_t w = G + gl; w - gl < J; w += G) {                  // (J > G: wave-uniform trips)
        a = (live && w < J) ? mask[rr * J + w] & sn.nat[w] : 0ull;
        any |= a != 0ull;
        lo |= w < J && (a & sn.nat[64u + w]) != 0ull;
        hi |= w < J && (a & sn.nat[128u + w]) != 0ull;
      }
      const bool own = grp(__ballot(any)) != 0ull && !(grp(__ballot(lo)) != 0ull && grp(__ballot(hi)) != 0ull);
      if (__builtin_expect(__any(own), 0)) {                           // a mask dropped every pod at an extreme: the exact range of the row's set bits
        constexpr int U = 4;
        uint32_t mn = 0xFFFFFFFFu, mx = 0u;
        for (uint32_t w = gl; w - gl < J; w += G) {
          uint64_t rem = (own && live && w < J) ? mask[rr * J + w] & sn.nat[w] : 0ull;
          while (__any(rem != 0ull)) {
            uint32_t qv[U];
            bool v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              v[u] = rem != 0ull;
              const uint32_t j = v[u] ? (uint32_t)__builtin_ctzll(rem) : 0u;
              rem &= rem - 1ull;
              qv[u] = sn.queue[v[u] ? w * 64u + j : 0u];              // (a lane that has run out re-reads pod 0: in bounds, never used)
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
              mn = (v[u] && qv[u] < mn) ? qv[u] : mn;
              mx = (v[u] && qv[u] > mx) ? qv[u] : mx;
            }
          }
        }
        sl_minmax<G>(mn, mx);
        if (own) { qmin = mn; qmax = mx; }
      }
    }

    // totals: the one expression of every exact route
    double t = 0.0;
    {
      const uint32_t bit = p >> 6;
      const uint32_t tier = (uint32_t)((((uint64_t)th >> bit) & 1ull) << 1) | (uint32_t)(((uint64_t)tl >> bit) & 1ull);
      double sp = 0.0;
      if (HAS_P && nb != 0u && matched != 0u) sp = clamp01((double)matched / (double)nb);      // (0 / nb == +0.0)
      const double tt = exact_total(ec, qmin, qmax, (double)(qmax - qmin), qd, kvu, tier, sp);
      t = valid ? tt : 0.0;
    }

    uint32_t pos = gl;
    if (sort) {                                                        // rank = the entries that beat this one
      uint32_t TL[EPPK_MAX_TOPK], TH[EPPK_MAX_TOPK];
      const uint64_t tb = (uint64_t)__double_as_longlong(t);
      pc_group_bcast_all<G>((uint32_t)tb, lane, TL, std::make_index_sequence<EPPK_MAX_TOPK>{});
      pc_group_bcast_all<G>((uint32_t)(tb >> 32), lane, TH, std::make_index_sequence<EPPK_MAX_TOPK>{});
      pos = 0u;
#pragma unroll
      for (uint32_t j = 0; j < EPPK_MAX_TOPK; ++j) {
        const double tj = __longlong_as_double((long long)(((uint64_t)TH[j] << 32) | TL[j]));
        const bool vj = P[j] != kPcNoPod;
        const bool beats = vj ? (!valid || tj > t || (tj == t && (P[j] < pv || (P[j] == pv && j < gl)))) : (!valid && j < gl);
        pos += (j < k && beats) ? 1u : 0u;
      }
    }
    if (live && gl < k) {
      const size_t at = (size_t)r * k + pos;
      if (out_pick) out_pick[at] = valid ? (int32_t)p : EPPK_NO_PICK;
      if (out_score) out_score[at] = t;
    }
  }
}

}  // namespace eppk

#endif  // EPPK_SCORE_LISTS_HIP_H
