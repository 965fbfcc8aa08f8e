// What the two mappings of the local search over separator tours share (spec
// A26: vrp_batch_lsr.hip, one workgroup per request; vrp_batch_lsr_spread.hip,
// G workgroups per request): the launch's arguments, its shape checks, the LDS
// carve of the instance and the first-fit start.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "batch_ls.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "tour.hpp"

namespace vrpms {

constexpr int kBatchLsrMaxK = 64;      // one lane per route in the first-fit start
constexpr int kBatchLsrMaxN = 65535;   // tokens are uint16
constexpr int kBatchLsrMaxL = 65535;   // positions too
constexpr int kBatchLsrMaxS = 65535;

struct VrpBatchLsrArgs {
  const int32_t* mats;    // [R][H][N][N]
  const int32_t* demand;  // [R][N]
  const int32_t* cap;     // [R][K]
  const int32_t* start;   // [R][K]
  int R, N, K, H, objective, S, rounds;
  uint32_t seed_lo, seed_hi;
  uint16_t* tours;        // [R][L]
  uint64_t* keys;         // [R]
  int32_t* durs;          // [R][K]
  int8_t* veh;            // [R][L]
  int32_t* info;          // [R][2]: the answer's start, the capped descents
};

struct BatchLsrLds {
  size_t mat, dem, row, tour, total;   // bytes of the matrix, the demand row, one K row, one tour
};

inline BatchLsrLds batch_lsr_lds(int N, int K, int H, int wide) {
  BatchLsrLds l;
  l.mat = ((size_t)H * N * N * (wide ? 4 : 2) + 15) & ~(size_t)15;
  l.dem = (((size_t)N + 3) & ~(size_t)3) * 4;
  l.row = (((size_t)K + 3) & ~(size_t)3) * 4;
  l.tour = (((size_t)N - 1 + K - 1 + 7) & ~(size_t)7) * 2;
  l.total = l.mat + l.dem + 2 * l.row + 4 * 2 * l.tour + 4 * 16;
  return l;
}

// the shape checks every entry point shares; 0 or the refusal's code
inline int batch_lsr_check(const char* who, int32_t N, int32_t K, int32_t H, int32_t wide) {
  const std::string w(who);
  if (N < 2 || N > kBatchLsrMaxN)
    return fail(VRPMS_EINVAL, w + ": needs 2 <= N <= 65535 (" + std::to_string(N) + " given)");
  if (K < 1 || K > kBatchLsrMaxK)
    return fail(VRPMS_EINVAL, w + ": one lane per route needs 1 <= K <= 64 (" + std::to_string(K) + " given)");
  if (N - 1 + K - 1 > kBatchLsrMaxL)
    return fail(VRPMS_EINVAL, w + ": positions are uint16: needs N + K - 2 <= 65535 (" +
                                  std::to_string(N - 1 + K - 1) + " given)");
  if (H != 1 && H != 24)
    return fail(VRPMS_EINVAL, w + ": H must be 1 or 24 (" + std::to_string(H) + " given)");
  if (wide != 0 && wide != 1)
    return fail(VRPMS_EINVAL, w + ": wide must be 0 (uint16 matrix) or 1 (int32) (" + std::to_string(wide) +
                                  " given)");
  return VRPMS_OK;
}

// the checks of the search's own arguments; 0 or the refusal's code
inline int batch_lsr_check_search(const char* who, int32_t objective, int32_t S, int32_t rounds) {
  const std::string w(who);
  if (objective != VRPMS_OBJ_SUM && objective != VRPMS_OBJ_MAX)
    return fail(VRPMS_EINVAL, w + ": objective must be VRPMS_OBJ_SUM or VRPMS_OBJ_MAX");
  if (S < 1 || S > kBatchLsrMaxS)
    return fail(VRPMS_EINVAL, w + ": 1 <= S <= 65535 (" + std::to_string(S) + " given)");
  if (rounds < 0)
    return fail(VRPMS_EINVAL, w + ": rounds must not be negative (" + std::to_string(rounds) + " given)");
  return VRPMS_OK;
}

// the refusal of a launch whose request does not fit the device's LDS
inline int batch_lsr_lds_refusal(const char* who, int32_t N, int32_t K, int32_t H, int32_t wide,
                                 size_t lds, size_t have) {
  return fail(VRPMS_EINVAL, std::string(who) + ": a request of N = " + std::to_string(N) + ", K = " +
                                std::to_string(K) + ", H = " + std::to_string(H) +
                                (wide ? " (int32 matrix)" : " (uint16 matrix)") + " needs " +
                                std::to_string(lds) + " bytes of LDS (" + std::to_string(have) +
                                " available)");
}

// One wavefront builds start s in A (L = n + K - 1 tokens): K - 1 separators
// (K empty routes), then the shuffle of 1..n, then spec.pack_separators(perm,
// K - 1) in place: lane b holds route b's load, its room and `end`, the
// position just past its last customer (its separator's; for route K - 1 the
// next customer's own).  Customer q goes to the first route that has room for
// it, to the last one when none has.
VRPMS_DEV void batch_lsr_start(uint16_t* A, const int32_t* dem, const int32_t* cap, int n, int K, int s,
                               uint32_t seed_lo, uint32_t seed_hi, int lane) {
  for (int q = lane; q < K - 1; q += 64) A[q] = 0;
  batch_ls_shuffle(A + (K - 1), n, s, seed_lo, seed_hi, lane);
  const int64_t room = lane < K ? (int64_t)cap[lane] : -1;
  int64_t load = 0;
  int end = lane;
  for (int q = 0; q < n; ++q) {
    const int at = K - 1 + q;
    const int64_t d = dem[A[at]];
    const uint64_t fits = __builtin_amdgcn_ballot_w64(lane < K && load + d <= room);
    const int b = fits ? (int)__builtin_ctzll(fits) : K - 1;
    const int pos = __builtin_amdgcn_readlane(end, b);
    if (lane == b) load += d;
    if (lane >= b) ++end;
    if (pos < at) batch_ls_apply(A, Move{kMoveRelocate, at, pos}, lane);
  }
}

}  // namespace vrpms
