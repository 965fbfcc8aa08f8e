// What vrp_sp.hip shares with vrp_tdsp.hip: the capacity filter and the
// partition layer of A15, which do not care where the route durations came
// from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "ctx.hpp"

namespace vrpms {

constexpr int kSpMaxN = 20;
constexpr int kSpMaxK = 64;
constexpr uint32_t kSpInf = 0xffffffffu;

struct SpLayerArgs {
  const uint32_t* routecap;  // [2^n], vehicle k's
  const uint32_t* fk;        // [2^n] f_k
  uint32_t* fn;              // [2^n] f_{k+1}, preset to unreachable
  const uint32_t* dem;       // [2^n]
  const int32_t* cap;        // [K]
  int n, k;
  // first[j] = first work item of cardinality n - j (heaviest sets first);
  // first[n + 1] = the number of items
  uint32_t first[kSpMaxN + 2];
};

// the bits of r deposited, lowest first, into the set bits of S
VRPMS_DEV uint32_t sp_deposit(uint32_t r, uint32_t S) {
  uint32_t T = 0;
  for (uint32_t m = S; m; m &= m - 1u, r >>= 1) T |= (r & 1u) ? (m & (0u - m)) : 0u;
  return T;
}

// Enqueue vrp_sp_cap_kernel: out[T] = dem[T] <= cap[k] ? route[T] : unreachable
// for the `count` masks.
int vrp_sp_cap(const uint32_t* route, const uint32_t* dem, const int32_t* cap, int k, uint32_t count,
               uint32_t* out, hipStream_t s);

// The work-item table of vrp_sp_layer_kernel for n customers (a.n, a.first).
void vrp_sp_layer_items(int n, SpLayerArgs& a);

// Enqueue vrp_sp_layer_kernel<objective> for vehicle a.k >= 1: a.fn (preset
// to unreachable) from a.fk and a.routecap.
int vrp_sp_layer(const SpLayerArgs& a, int objective, hipStream_t s);

}  // namespace vrpms
