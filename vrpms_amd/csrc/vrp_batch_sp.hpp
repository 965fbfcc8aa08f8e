// What vrp_batch_sp.hip shares with vrp_batch_tdsp.hip: one team's partition
// layer of A15 over LDS-resident arrays and the helpers of its backtrack
// (DESIGN.md §2 A19, §4.3j).  They do not care where the route durations came
// from.  None of these functions contains a barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "tsp_batch_dp.hpp"
#include "tsp_dp.hpp"
#include "vrp_sp.hpp"

namespace vrpms {

constexpr int kBatchSpMaxK = kSpMaxK;
constexpr int kBatchSpDemWords = 16;
// lanes that share one set of a partition layer: 2^2, the fastest of the A/B
// builds (tools/ab_build.py -DVRPMS_BATCH_SP_GROUP_LOG=0, 2, 3, 4; 0 is one
// thread per set, heaviest sets first; DESIGN.md §4.3j has the measurements)
#ifndef VRPMS_BATCH_SP_GROUP_LOG
#define VRPMS_BATCH_SP_GROUP_LOG 2
#endif
constexpr int kBatchSpGroupLog = VRPMS_BATCH_SP_GROUP_LOG;
constexpr int kBatchSpGroup = 1 << kBatchSpGroupLog;
static_assert(kBatchSpGroupLog >= 0 && kBatchSpGroupLog <= 4, "a group lies inside the smallest team");

// 2^n words padded to four (n = 1 has two)
inline size_t batch_sp_set_words(int n) { return (((size_t)1 << n) + 3) & ~(size_t)3; }

// the demand of T, saturated at unreachable (as vrp_sp_route_kernel's)
VRPMS_DEV uint32_t batch_sp_demand(const uint32_t* dem, uint32_t T) {
  uint64_t dm = 0;
  for (uint32_t m = T; m; m &= m - 1u) dm += dem[__builtin_ctz(m)];
  return dm < kSpInf ? (uint32_t)dm : kSpInf;
}

template <int OBJ>
VRPMS_DEV uint32_t batch_sp_join(uint32_t rc, uint32_t fv) {
  return OBJ ? max(rc, fv) : __builtin_elementwise_add_sat(rc, fv);
}

// minimum over the aligned group of W lanes (W a power of two, at most 64)
template <int W>
VRPMS_DEV uint32_t batch_sp_group_min(uint32_t v) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, W));
  return v;
}

// One partition layer of one team: fn[S] for every S from rc and fk.
template <int T, int OBJ>
VRPMS_DEV void batch_sp_layer(const uint32_t* B, int n, const uint32_t* rc, const uint32_t* fk,
                              uint32_t* fn, int tl, bool active) {
  constexpr int NG = T / kBatchSpGroup;
  const int grp = tl / kBatchSpGroup, l = tl % kBatchSpGroup;
  for (int c = n; c >= 0; --c) {
    const uint32_t count = active ? B[n * kBatchDpNodes + c] : 0u;
    const uint32_t gr = (uint32_t)(grp + 5 * c) % NG;   // 5 is odd: a rotation for every NG
    const uint32_t lo = gr * count / NG, hi = (gr + 1u) * count / NG;
    if (lo >= hi) continue;
    const int q = c < kBatchSpGroupLog ? c : kBatchSpGroupLog;
    const uint32_t steps = 1u << (c - q);
    uint32_t S = c == 0 ? 0u : (c == n ? (1u << n) - 1u : dp_unrank(B, kBatchDpNodes, n, c, lo));
    for (uint32_t r = lo; r < hi; ++r) {
      uint32_t rest = S;   // S without its q lowest customers
      for (int i = 0; i < q; ++i) rest &= rest - 1u;
      uint32_t best = kSpInf;
      if (l < (1 << q)) {
        const uint32_t P = sp_deposit((uint32_t)l, S ^ rest);
        uint32_t U = rest;
        if (steps >= 4u) {
          // four steps' masks first, then their eight reads in flight together
          for (uint32_t i = 0; i < steps; i += 4u) {
            uint32_t t[4], a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              t[u] = P | U;
              U = (U - 1u) & rest;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              a[u] = rc[t[u]];
              b[u] = fk[S ^ t[u]];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) best = min(best, batch_sp_join<OBJ>(a[u], b[u]));
          }
        } else {
          for (uint32_t i = 0; i < steps; ++i) {
            const uint32_t t = P | U;
            best = min(best, batch_sp_join<OBJ>(rc[t], fk[S ^ t]));
            U = (U - 1u) & rest;
          }
        }
      }
      best = batch_sp_group_min<kBatchSpGroup>(best);
      if (l == 0) fn[S] = best;
      if (r + 1u < hi) S = dp_next_mask(S);
    }
  }
}

}  // namespace vrpms
