// eppk_filter.hip.h — the metric predicates of the Filter phase (SEMANTICS.md §2c; include/eppk.h eppk_set_filters), on the device.
//
// Included by eppk.hip alone: the thirty pick units do not see this file, so a change here rebuilds one unit.
//
// Two kernels.  filter_planes_kernel turns the raw pod rows of the latest publish (plus the assumed-load bumps they have taken since)
// into PLANES: one bit per pod for "is no hole", for every pod-only stage of every program, and -- when a program asks for them -- for
// either LoRA predicate under each of the 129 adapter values a request can carry.  filter_masks_kernel then is a handful of ANDs per
// request: a wavefront per request, lane l holds word l of the request's candidate row.
//
// Layout.  Planes use the bit layout of the API's mask rows (word p / 64, bit p % 64 = pod p), NOT the pick kernels' lane words: a
// candidate row is loaded, ANDed and stored as it is.  Every plane is kFilterPlaneWords = 64 words long whatever the snapshot's size
// (words behind ceil(n_pods / 64) are zero), so that a lane may read "its" word of any plane without a bound.
//     plane 0                                  pods that are no hole (bits >= n_pods clear)
//     plane 1 + 4 * program + stage            QUEUE_LE / RUNNING_LE / KV_LE stages (others: unused)
//     plane 17 + (adapter + 1)                 LORA_LOADED   for adapter -1 .. 127      (written only when a program uses the kind)
//     plane 146 + (adapter + 1)                LORA_SERVABLE for adapter -1 .. 127
//     behind the planes: queue[] transposed, u32 [64][64]: entry [b][l] = queue[64 * l + b] -- what QUEUE_WITHIN stages into LDS
#ifndef EPPK_FILTER_HIP_H
#define EPPK_FILTER_HIP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eppk.h"

namespace eppk {

constexpr uint32_t kFilterPlaneWords = 64u;                       // words per plane (EPPK_MAX_PODS / 64)
constexpr uint32_t kFilterStagePlane0 = 1u;
constexpr uint32_t kFilterLoadedPlane0 = 1u + EPPK_MAX_FILTER_PROGRAMS * EPPK_MAX_PREDICATES;
constexpr uint32_t kFilterServablePlane0 = kFilterLoadedPlane0 + EPPK_MAX_ADAPTERS + 1u;
constexpr uint32_t kFilterPlanes = kFilterServablePlane0 + EPPK_MAX_ADAPTERS + 1u;
constexpr size_t kFilterQueueOff = (size_t)kFilterPlanes * kFilterPlaneWords;          // in u64 words
constexpr size_t kFilterBufBytes = kFilterQueueOff * 8u + 4096u * 4u;
constexpr uint32_t kFilterQueueLds = 4096u * 4u;                  // dynamic LDS of filter_masks_kernel when a program uses QUEUE_WITHIN

// The programs of a context as the kernels take them: by value, in the kernel argument segment (every index into it is wave-uniform).
struct KFilter {
  uint32_t n_programs;
  uint32_t uses_lora;        // bit 0: some stage is LORA_LOADED, bit 1: some stage is LORA_SERVABLE
  uint32_t uses_within;      // some stage is QUEUE_WITHIN
  uint32_t pad;
  uint32_t n_stages[EPPK_MAX_FILTER_PROGRAMS];
  uint32_t kind[EPPK_MAX_FILTER_PROGRAMS][EPPK_MAX_PREDICATES];
  uint32_t on_empty[EPPK_MAX_FILTER_PROGRAMS][EPPK_MAX_PREDICATES];
  uint32_t u[EPPK_MAX_FILTER_PROGRAMS][EPPK_MAX_PREDICATES];
  double   f[EPPK_MAX_FILTER_PROGRAMS][EPPK_MAX_PREDICATES];
};

__device__ __forceinline__ bool filter_any(bool x) { return __ballot(x) != 0ull; }

// Grid: 64 workgroups of one wavefront; wavefront j builds word j of every plane, lane b looks at pod 64 j + b.
__global__ __launch_bounds__(64) void filter_planes_kernel(const eppk_pod_row* __restrict__ rows, uint32_t n_pods, KFilter fp,
                                                           uint64_t* __restrict__ planes) {
  const uint32_t lane = threadIdx.x & 63u, j = blockIdx.x;
  if (j >= kFilterPlaneWords) return;
  const uint32_t p = j * 64u + lane;
  const bool exists = p < n_pods;
  uint32_t queue = 0u, running = 0u, max_lora = 0u, flags = EPPK_POD_INACTIVE;
  double kv = 0.0;
  uint64_t act0 = 0ull, act1 = 0ull, wai0 = 0ull, wai1 = 0ull;
  if (exists) {
    const eppk_pod_row& row = rows[p];
    queue = row.queue; running = row.running; kv = row.kv_util; max_lora = row.max_lora; flags = row.flags;
    act0 = row.active[0]; act1 = row.active[1]; wai0 = row.waiting[0]; wai1 = row.waiting[1];
  }
  uint32_t* qt = (uint32_t*)(planes + kFilterQueueOff);
  qt[lane * 64u + j] = queue;                                       // [b][l]: bit b of word l (pods that do not exist: 0, never read)
  const uint64_t live = __ballot(exists && !(flags & EPPK_POD_INACTIVE));
  if (lane == 0u) planes[j] = live;
  for (uint32_t g = 0; g < fp.n_programs; ++g)
    for (uint32_t s = 0; s < fp.n_stages[g]; ++s) {
      const uint32_t kind = fp.kind[g][s];
      bool ok;
      if (kind == EPPK_PRED_QUEUE_LE) ok = queue <= fp.u[g][s];
      else if (kind == EPPK_PRED_RUNNING_LE) ok = running <= fp.u[g][s];
      else if (kind == EPPK_PRED_KV_LE) ok = kv <= fp.f[g][s];                  // raw IEEE compare: a NaN on either side passes nothing
      else continue;
      const uint64_t w = __ballot(exists && ok);
      if (lane == 0u) planes[(size_t)(kFilterStagePlane0 + g * EPPK_MAX_PREDICATES + s) * kFilterPlaneWords + j] = w;
    }
  if (fp.uses_lora) {
    const uint64_t held0 = act0 | wai0, held1 = act1 | wai1;
    const uint32_t loaded = (uint32_t)(__popcll(act0) + __popcll(act1) + __popcll(wai0) + __popcll(wai1));
    const bool room = loaded < max_lora;
    // adapter -1 (the base model): passes both predicates on every pod -- it needs no slot
    const uint64_t all = __ballot(exists);
    if (lane == 0u) {
      if (fp.uses_lora & 1u) planes[(size_t)kFilterLoadedPlane0 * kFilterPlaneWords + j] = all;
      if (fp.uses_lora & 2u) planes[(size_t)kFilterServablePlane0 * kFilterPlaneWords + j] = all;
    }
    for (uint32_t a = 0; a < EPPK_MAX_ADAPTERS; ++a) {
      const bool held = (((a < 64u ? held0 : held1) >> (a & 63u)) & 1ull) != 0ull;
      if (fp.uses_lora & 1u) {
        const uint64_t w = __ballot(exists && held);
        if (lane == 0u) planes[(size_t)(kFilterLoadedPlane0 + 1u + a) * kFilterPlaneWords + j] = w;
      }
      if (fp.uses_lora & 2u) {
        const uint64_t w = __ballot(exists && (held || room));
        if (lane == 0u) planes[(size_t)(kFilterServablePlane0 + 1u + a) * kFilterPlaneWords + j] = w;
      }
    }
  }
}

// A wavefront per request (grid-stride, as subset_masks_kernel).  mask_in nullable (all ones), cls nullable (program 0), verdict
// nullable; mask_out may be mask_in: a wavefront has read its row before it writes it.  reqs is read only for the adapter.
__global__ __launch_bounds__(256) void filter_masks_kernel(const uint8_t* __restrict__ reqs, uint32_t stride, uint32_t n_reqs,
                                                           const uint8_t* __restrict__ cls, const uint64_t* mask_in, uint64_t* mask_out,
                                                           uint8_t* __restrict__ verdict, uint32_t n_pods, const uint64_t* __restrict__ planes,
                                                           KFilter fp, uint32_t* __restrict__ status) {
  extern __shared__ uint32_t s_queue[];                             // [64][64] u32, [b][l] (only with QUEUE_WITHIN: else no LDS at all)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t J = (n_pods + 63u) / 64u;
  if (fp.uses_within) {                                             // (uniform: a kernel argument)
    const uint32_t* qt = (const uint32_t*)(planes + kFilterQueueOff);
    for (uint32_t i = threadIdx.x; i < 4096u; i += blockDim.x) s_queue[i] = qt[i];
    __syncthreads();
  }
  const uint64_t live = planes[lane];                               // (words >= J are zero)
  uint64_t tail = ~0ull;
  if (lane + 1u == J && (n_pods & 63u)) tail = (1ull << (n_pods & 63u)) - 1ull;
  if (lane >= J) tail = 0ull;
  for (uint32_t r = wave; r < n_reqs; r += nwaves) {
    uint64_t w = ~0ull;
    if (mask_in && lane < J) w = mask_in[(size_t)r * J + lane];
    w &= live & tail;
    uint32_t g = cls ? (uint32_t)cls[r] : 0u;
    g = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
    int32_t a = EPPK_ADAPTER_BASE;
    if (reqs) a = (int32_t)__builtin_amdgcn_readfirstlane(*(const int32_t*)(reqs + (size_t)r * stride));
    uint32_t v = 0u;
    if (a < -1 || a >= (int32_t)EPPK_MAX_ADAPTERS) {                // a row out of range has no candidates (the pick kernels' rule)
      w = 0ull;
      if (lane == 0u) atomicOr(status, EPPK_LAUNCH_BAD_REQUEST_ROW);
    } else if (fp.n_programs != 0u && g >= fp.n_programs) {
      w = 0ull;
      v = EPPK_VERDICT_BAD_CLASS;
    } else if (fp.n_programs != 0u) {
      const uint32_t n = fp.n_stages[g];
      for (uint32_t s = 0; s < n; ++s) {
        if (!filter_any(w != 0ull)) break;                          // C_s is empty: nothing happens, no bit
        const uint32_t kind = fp.kind[g][s];
        uint64_t k;
        if (kind == EPPK_PRED_QUEUE_WITHIN) {
          uint32_t mn = 0xFFFFFFFFu;
          for (uint64_t t = w; t; t &= t - 1ull) {
            const uint32_t q = s_queue[(uint32_t)__builtin_ctzll(t) * 64u + lane];
            mn = q < mn ? q : mn;
          }
          for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)mn, off);
            mn = o < mn ? o : mn;
          }
          const uint32_t u = fp.u[g][s];
          k = 0ull;
          for (uint64_t t = w; t; t &= t - 1ull) {
            const uint32_t b = (uint32_t)__builtin_ctzll(t);
            if (s_queue[b * 64u + lane] - mn <= u) k |= 1ull << b;
          }
        } else {
          uint32_t plane = kFilterStagePlane0 + g * EPPK_MAX_PREDICATES + s;
          if (kind == EPPK_PRED_LORA_LOADED) plane = kFilterLoadedPlane0 + (uint32_t)(a + 1);
          else if (kind == EPPK_PRED_LORA_SERVABLE) plane = kFilterServablePlane0 + (uint32_t)(a + 1);
          k = w & planes[(size_t)plane * kFilterPlaneWords + lane];
        }
        if (filter_any(k != 0ull)) w = k;
        else {
          v |= 1u << s;
          if (fp.on_empty[g][s] == EPPK_ON_EMPTY_REQUIRE) { w = 0ull; v |= EPPK_VERDICT_SHED; }
        }
      }
    }
    if (lane < J) mask_out[(size_t)r * J + lane] = w;
    if (verdict && lane == 0u) verdict[r] = (uint8_t)v;
  }
}

}  // namespace eppk
#endif
