// What the integer ant-colony kernels share (search.hip: the unbatched
// aco_construct_lds_kernel and its update kernels; vrp_batch_aco.hip, A24):
// the static attractiveness, the per-wavefront Philox draws, the roulette of a
// wavefront whose lanes own CH consecutive nodes each, evaporation and the
// deposit.  oracle/search.py aco_eta / aco_iteration state the same arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"

namespace vrpms {

// eta of an edge of duration d (hour slice 0): floor(2^24 / (1 + d)^2)
VRPMS_DEV uint32_t aco_eta_cell(uint32_t d) {
  const uint64_t d1 = 1ull + (uint64_t)d;
  return (uint32_t)((1ull << 24) / (d1 * d1));
}

// one cell's evaporation, clamped into [tau_min, tau_max]
VRPMS_DEV uint32_t aco_evaporated(uint32_t t, uint32_t evap_shift, uint32_t tau_min, uint32_t tau_max) {
  return min(tau_max, max(tau_min, t - (t >> evap_shift)));
}

// what a tour of A8 key `key` deposits on each of its edges: floor(2^30 / (1 + primary))
VRPMS_DEV uint32_t aco_deposit_of(uint64_t key) {
  const uint32_t primary = (uint32_t)((key >> 28) & ((1u << 28) - 1u));
  return (uint32_t)((1u << 30) / (1ull + primary));
}

// The draws of one ant whose wavefront walks it: the Philox blocks of 64 steps
// at once, lane l computing step s0 + l's in VALU and each step reading its own
// with v_readlane (a per-step block on the scalar unit made the construction
// SALU-issue bound).  Block (it & M32, it >> 32, ant, s), words x (low) and y.
struct AcoDraws {
  uint32_t rx = 0, ry = 0;
  // call at every step, by every lane: refills when s is a multiple of 64
  VRPMS_DEV void step(uint64_t iter, uint32_t ant, int s, int lane, uint32_t seed_lo, uint32_t seed_hi) {
    if ((s & 63) == 0) {
      const u32x4 r = philox((uint32_t)iter, (uint32_t)(iter >> 32), ant, (uint32_t)(s + lane), seed_lo,
                             seed_hi);
      rx = r.x;
      ry = r.y;
    }
  }
  VRPMS_DEV uint64_t at(int s) const {
    const uint32_t r_x = (uint32_t)__builtin_amdgcn_readlane((int)rx, s & 63);
    const uint32_t r_y = (uint32_t)__builtin_amdgcn_readlane((int)ry, s & 63);
    return ((uint64_t)r_y << 32) | r_x;
  }
};

// Lane l owns the CH consecutive nodes CH l .. CH l + CH - 1; bit c of its mask:
// node CH l + c is visited, or past N, or the depot.  The start of every ant.
template <int CH>
VRPMS_DEV uint32_t aco_owned_start(int lane, int N) {
  uint32_t vm = lane == 0 ? 1u : 0u;
#pragma unroll
  for (int c = 0; c < CH; ++c)
    if (CH * lane + c >= N) vm |= 1u << c;
  return vm;
}

// One roulette step of such a wavefront, every lane active.  w[c]: the weight
// of the lane's node c, 0 where its mask bit is set; vm: the mask, which must
// have a clear bit in some lane; r: the step's 64-bit draw.  The roulette's
// prefix sums in node order are the lanes' prefix (ONE 64-bit wave scan of
// each lane's sum, not one per 64-node chunk) followed by the lane's own
// running sum: the first lane whose inclusive prefix passes r % tot holds the
// pick, the first of its nodes whose running sum passes it.  (The first node j
// with prefix P_j > r has w_j > 0.)  With every free weight 0: the first free
// node.  -> the pick, wave-uniform; it has a clear mask bit, so it is below N.
template <int CH>
VRPMS_DEV uint32_t aco_roulette_owned(const uint64_t (&w)[CH], uint32_t vm, uint64_t r, int lane) {
  constexpr uint32_t kAll = (1u << CH) - 1u;
  uint64_t sum = 0;
#pragma unroll
  for (int c = 0; c < CH; ++c) sum += w[c];
  uint64_t incl = sum;
  const uint64_t tot = wave_scan_add_u64(incl);
  uint32_t mine, L;  // this lane's candidate node, the lane that holds the pick
  if (tot != 0) {
    const uint64_t rr = umod64(r, tot);
    L = (uint32_t)__ffsll((long long)__ballot(incl > rr)) - 1u;  // exists: the last lane's is tot
    uint64_t run = incl - sum;
    uint32_t cc = CH - 1;
    bool found = false;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      run += w[c];
      if (!found && run > rr) {
        cc = (uint32_t)c;
        found = true;
      }
    }
    mine = CH * (uint32_t)lane + cc;
  } else {  // every free weight is 0: the first free node
    L = (uint32_t)__ffsll((long long)__ballot(vm != kAll)) - 1u;
    mine = CH * (uint32_t)lane + (uint32_t)__builtin_ctz((~vm & kAll) | (1u << CH));
  }
  return (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)L);
}

}  // namespace vrpms
