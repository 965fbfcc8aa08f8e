// What the VRP local searches share on top of batch_ls.hpp's descent:
// vrp_batch_ls.hip (A25, tours of n customers) and vrp_batch_lsr.hip (A26, tours
// of L = n + K - 1 tokens with separators) have one argument struct, one LDS
// size and one host tail behind their shape checks; vrp_batch_lsr_spread.hip
// (A26 with G workgroups per request) takes the arguments, the checks and the
// first-fit start.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "batch_launch.hpp"
#include "batch_ls.hpp"
#include "batch_stage.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "staging.hpp"
#include "tour.hpp"

namespace vrpms {

struct VrpBatchLsArgs {
  const int32_t* mats;    // [R][H][N][N]
  const int32_t* demand;  // [R][N]
  const int32_t* cap;     // [R][K]
  const int32_t* start;   // [R][K]
  int R, N, K, H, objective, S, rounds;
  uint32_t seed_lo, seed_hi;
  uint16_t* tours;        // [R][L]; L = n for vrp_batch_ls
  uint64_t* keys;         // [R]
  int32_t* durs;          // [R][K]
  int8_t* veh;            // [R][L]
  int32_t* info;          // [R][2]: the answer's start, the capped descents
};

// vrp_batch_ls (L = n) and vrp_batch_lsr (L = n + K - 1): behind the instance 4
// waves x (current, best end) uint16 tours of align8(L), then [4] BatchLsWave
inline size_t batch_ls_lds(int N, int K, int H, int wide, int L) {
  return batch_inst_bytes(N, K, H, wide) + 4 * 2 * batch_align<size_t>(L, 8) * 2 + 4 * sizeof(BatchLsWave);
}

// the shape checks of every lsr entry point: vrp_batch_ls's with the bound on L
// behind K
inline int batch_lsr_check(const char* who, int32_t N, int32_t K, int32_t H, int32_t wide) {
  if (const int rc = batch_check_N(who, N)) return rc;
  if (const int rc = batch_check_K(who, K)) return rc;
  if (N - 1 + K - 1 > kBatchMaxN)
    return fail(VRPMS_EINVAL, std::string(who) + ": positions are uint16: needs N + K - 2 <= 65535 (" +
                                  std::to_string(N - 1 + K - 1) + " given)");
  return batch_check_matrix(who, H, wide);
}

// the checks of a local search's own arguments
inline int batch_ls_check_search(const char* who, int32_t objective, int32_t S, int32_t rounds) {
  if (const int rc = batch_check_objective(who, objective)) return rc;
  if (const int rc = batch_check_count(who, "S", S, kBatchMaxS)) return rc;
  return batch_check_rounds(who, rounds);
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

// What the entry points vrpms_vrp_batch_ls (SEP = false) and vrpms_vrp_batch_lsr
// (SEP = true) do behind their shape check; `kernel` picks the instantiation
// of the one's or the other's __global__ wrapper.
template <class Kernel>
int batch_ls_launch(const char* who, vrpms_ctx* ctx, const VrpBatchLsArgs& a, int wide, int L, void* stream,
                    Kernel&& kernel) {
  if (const int rc = batch_ls_check_search(who, a.objective, a.S, a.rounds)) return rc;
  if (a.R == 0) return VRPMS_OK;
  if (const int rc = batch_check_buffers(
          who, "matrix/demand/capacity/start/tour/key/duration/vehicle/info",
          {a.mats, a.demand, a.cap, a.start, a.tours, a.keys, a.durs, a.veh, a.info}))
    return rc;
  const size_t lds = batch_ls_lds(a.N, a.K, a.H, wide, L);
  if (lds > ctx->max_lds) return batch_lds_refusal(who, a.N, a.K, a.H, wide, "", lds, ctx->max_lds);
  VRPMS_HIP(hipSetDevice(ctx->device));
  const char* what = "";
  const hipError_t e = batch_with_matrix(wide, a.H, [&](auto m, auto hm) {
    return batch_launch_blocks(kernel(m, hm), a, (unsigned)a.R, lds, (hipStream_t)stream, &what);
  });
  if (e != hipSuccess) return hip_fail(e, what);
  return VRPMS_OK;
}

}  // namespace vrpms
