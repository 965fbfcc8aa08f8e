// Batched exact time-dependent TSP: the time-expanded subset DP for many small
// requests, each request's whole table in LDS.
//
// The recurrence, the tie rule and the result are tsp_tdp.hip's (A16), per
// request: the state is (visited set S, last customer c, clock), the clocks of
// one (S, c) are a bitset, one 64-bit word per hour (bits 0..59, word w bit m =
// clock 60 (start / 60) + 60 w + m), a transition is a shift by d % 60 into
// words w + d / 60 and w + d / 60 + 1, and the departure word picks the matrix
// slice.  What differs is where the table lives and who fills it:
//
//   - The table is compact and resident: only rows (S, c) with c in S exist,
//     n 2^(n-1) rows of W words, indexed as tsp_batch_dp.hip indexes its
//     table: by customer, then by S with bit c squeezed out.  Row (S, c) is at
//     (c 2^(n-1) + squeeze(S, c)) W.  Nothing but the matrix, the start and the
//     horizon is read from memory, nothing but the tour and the key written.
//   - Only the matrix slices the words can use are staged, at word position:
//     slice (start / 60 + p) % 24 at p < min(W, 24) (word w reads position
//     w % 24), one slice when H = 1.
//   - A team of T threads owns one request; a 256-thread workgroup holds
//     256 / T requests of the same N, so every team runs the same layers and
//     the workgroup-wide barrier between them is uniform.  A team past the end
//     of the batch reaches every barrier and touches nothing.
//   - A layer ORs straight into its destination rows (zeroed at stage time).
//     The rows (S, c) of cardinality k, in (rank of S, position of c) order,
//     are dealt in consecutive runs (dp_unrank for the first mask, dp_next_mask
//     from there).  Two fills take a run:
//       owner   one thread per row: it walks the row's predecessors and their
//               words and does plain read-modify-write on the row, which is
//               its alone;
//       atomic  a group of G lanes per row (G the power of two at or above W,
//               within 4..min(T, 64)), the lanes spread over the row's
//               (predecessor, word) items, 64-bit LDS atomic OR.
//     §4.3k has both measured: the owner fill is the faster one at narrow rows
//     (few items per row: the group's lanes idle), the atomic one at wide rows
//     (few rows per layer at small n: the owners idle), so the launch picks by
//     W (kBatchTdpAtomicWords); -DVRPMS_BATCH_TDP_FILL=0 / 1 force one.
//   - The horizon clip is applied where a word is produced.  A request's
//     effective horizon is min(horizon, 60 W - 1 - start % 60): words past its
//     last one are never produced, the last one is masked, so a request with
//     fewer words than the launch's W leaves the rest of its rows zero and a
//     W below a request's need prunes its answer but never leaves its rows.
//   - The walk runs in-kernel after the last layer on the team's first
//     min(T, 64) lanes, which lie in one wavefront: tsp_tdp_walk_kernel's two
//     minimisations with its (value << 24 | c << 16 | clock) packing.
#include <hip/hip_runtime.h>

#include <string>

#include "batch_launch.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "tsp_batch_dp.hpp"
#include "tsp_batch_tdp.hpp"
#include "tsp_dp.hpp"
#include "tsp_tdp.hpp"

namespace vrpms {

// the auto team: kBatchTdpTeam[n] (tsp_batch_tdp.hpp), or the next larger T
// whose 256 / T requests fit kBatchTdpTeamLds, a fifth of the CU's LDS, so
// that five workgroups share a CU -- at every measured (n, W) the fastest T or
// within 7 % of it -- and 256 if none does
constexpr size_t kBatchTdpTeamLds = 32 * 1024;

__constant__ DpBinom kBatchTdpBinom = dp_make_binom();

struct BatchTdpArgs {
  const int32_t* mats;     // [R][H][N][N]
  const int32_t* start;    // [R]
  const int32_t* horizon;  // [R]
  int R, N, H, W;
  int16_t* tours;          // [R][N-1]
  uint64_t* keys;          // [R]
};

// bytes of one team: the table, then the staged slices padded to 8 bytes
inline size_t batch_tdp_team_bytes(int n, int H, int W) {
  const size_t table = ((size_t)n << (n - 1)) * (size_t)W * 8;
  const size_t mat = ((size_t)batch_tdp_slices(H, W) * (n + 1) * (n + 1) + 1) & ~(size_t)1;
  return table + mat * 4;
}

inline size_t batch_tdp_lds_bytes(int n, int H, int W, int T) {
  return (size_t)kBatchDpBinomWords * 4 + (size_t)(256 / T) * batch_tdp_team_bytes(n, H, W);
}

// the table's T, or the next larger one whose 256 / T requests fit kBatchTdpTeamLds; 256 if none does
inline int batch_tdp_auto_team(int n, int H, int W) {
  int T = kBatchTdpTeam[n];
  while (T < 256 && batch_tdp_lds_bytes(n, H, W, T) > kBatchTdpTeamLds) T *= 2;
  return T;
}

template <int T, int FILL>
__global__ __launch_bounds__(256) void tsp_batch_tdp_kernel(BatchTdpArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint64_t batch_tdp_lds[];
  const int N = a.N, n = N - 1, W = a.W, NN2 = N * N;
  const uint32_t full = (1u << n) - 1u;
  const int team = threadIdx.x / T, tl = threadIdx.x % T;
  const int64_t req = (int64_t)blockIdx.x * (256 / T) + team;
  const bool active = req < a.R;
  const int ns = a.H == 1 ? 1 : (W < 24 ? W : 24);
  const uint32_t table_words = ((uint32_t)n << (n - 1)) * (uint32_t)W;          // 64-bit words
  const uint32_t team_words = table_words + (((uint32_t)(ns * NN2) + 1u) >> 1);  // 64-bit words

  uint32_t* B = reinterpret_cast<uint32_t*>(batch_tdp_lds);       // B[c][t] = C(c, t)
  uint64_t* tab = batch_tdp_lds + kBatchDpBinomWords / 2 + (size_t)team * team_words;
  int32_t* Dl = reinterpret_cast<int32_t*>(tab + table_words);    // Dl[p][i][j], slice (h0 + p) % 24

  batch_dp_stage_binom(kBatchTdpBinom, B);
  BatchTdpReq q{0, -1, -1, 0};
  bool live = false;   // a request with a negative start or horizon has no tour
  if (active) {
    const int start = a.start[req], horizon = a.horizon[req];
    live = start >= 0 && horizon >= 0;
    if (live) q = batch_tdp_req(start, horizon, W);
    batch_tdp_stage<T>(a.mats + req * (int64_t)a.H * NN2, N, a.H, W, ns, live ? start : 0, full, n, tl, Dl,
                       tab);
  }
  __syncthreads();
  batch_tdp_fill<T, FILL>(B, tab, Dl, n, W, ns, q, tl, live, n);

  constexpr int WL = T < 64 ? T : 64;
  if (!active || tl >= WL) return;
  int16_t* tour = a.tours + req * n;
  const uint32_t dur = batch_tdp_walk<T>(tab, Dl, n, W, ns, q, full, tl, live, tour);
  if (dur == 0xffffffffu) {
    if (tl < n) tour[tl] = 0;
    if (tl == 0) a.keys[req] = ~0ull;
    return;
  }
  if (tl == 0) a.keys[req] = pack_key(0, dur, 0);
}

static int batch_tdp_check(const char* who, int n, int H, int W, int team) {
  const std::string f(who);
  if (n < 1 || n > kBatchTdpMaxN)
    return fail(VRPMS_EINVAL, f + ": the LDS-resident table needs 2 <= N <= 12, 1 <= n <= 11 (n = " +
                                  std::to_string(n) + " given)");
  if (H != 1 && H != 24)
    return fail(VRPMS_EINVAL, f + ": the matrices must be static or have 24 hour slices (H = " +
                                  std::to_string(H) + " given)");
  if (W < 1 || W > kTdpMaxWords)
    return fail(VRPMS_EINVAL, f + ": a row has 1 <= W <= 512 hour words (" + std::to_string(W) +
                                  " given)");
  if (!batch_team_ok(team)) return batch_team_fail(who, team);
  return VRPMS_OK;
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_tsp_batch_tdp_lds(int32_t n, int32_t H, int32_t W, int32_t team,
                                       uint64_t* bytes) {
  if (!bytes) return fail(VRPMS_EINVAL, "vrpms_tsp_batch_tdp_lds: bytes is NULL");
  const int rc = batch_tdp_check("vrpms_tsp_batch_tdp_lds", n, H, W, team);
  if (rc != VRPMS_OK) return rc;
  *bytes = batch_tdp_lds_bytes(n, H, W, team ? team : batch_tdp_auto_team(n, H, W));
  return VRPMS_OK;
}

extern "C" int vrpms_tsp_batch_tdp(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_start,
                                   const int32_t* d_horizon, int32_t R, int32_t N, int32_t H,
                                   int32_t W, int32_t team, int16_t* d_tours, uint64_t* d_keys,
                                   void* stream) {
  if (!ctx) return fail(VRPMS_EINVAL, "vrpms_tsp_batch_tdp: ctx is NULL");
  if (R < 0) return fail(VRPMS_EINVAL, "vrpms_tsp_batch_tdp: R must not be negative");
  const int rc = batch_tdp_check("vrpms_tsp_batch_tdp", N - 1, H, W, team);
  if (rc != VRPMS_OK) return rc;
  if (R == 0) return VRPMS_OK;
  if (!d_mats || !d_start || !d_horizon || !d_tours || !d_keys)
    return fail(VRPMS_EINVAL, "vrpms_tsp_batch_tdp: NULL matrix/start/horizon/tour/key buffer");
  const int n = N - 1;
  const int T = team ? team : batch_tdp_auto_team(n, H, W);
  const size_t lds = batch_tdp_lds_bytes(n, H, W, T);
  if (lds > ctx->max_lds)
    return fail(VRPMS_EINVAL, "vrpms_tsp_batch_tdp: " + std::to_string(256 / T) + " tables of n = " +
                                  std::to_string(n) + ", W = " + std::to_string(W) + " need " +
                                  std::to_string(lds) + " bytes of LDS (" +
                                  std::to_string(ctx->max_lds) + " available)");
  VRPMS_HIP(hipSetDevice(ctx->device));
  const BatchTdpArgs a{d_mats, d_start, d_horizon, R, N, H, W, d_tours, d_keys};
  hipStream_t s = (hipStream_t)stream;
  const bool atomic = batch_tdp_atomic(W);
  const hipError_t e = batch_with_team(T, [&](auto t) {
    constexpr int TT = decltype(t)::value;
    return batch_launch(atomic ? tsp_batch_tdp_kernel<TT, 1> : tsp_batch_tdp_kernel<TT, 0>, a, R, T,
                        lds, s);
  });
  VRPMS_HIP(e);
  return VRPMS_OK;
}
