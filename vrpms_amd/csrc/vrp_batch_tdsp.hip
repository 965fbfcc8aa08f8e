// Batched exact time-dependent VRP: the time-expanded partition DP for many
// small requests, each request's whole state in LDS.
//
// The recurrence, the tie rule and the result are vrp_tdsp.hip's (A17), per
// request; the pieces are A20's LDS-resident time-expanded table
// (tsp_batch_tdp.hpp: staging, fill, walk) and A19's LDS-resident partition
// layers and backtrack (vrp_batch_sp.hpp).  A team of T threads owns one
// request, a 256-thread workgroup holds 256 / T requests of the same N, K and
// H.  Only the matrices, the demands, the capacities, the start times and the
// horizon are read from memory, only the tour, the key and the K route
// durations are written to it.
//
// One team's LDS:
//   tab    n 2^(n-1) rows of W 64-bit words: the compact A16 table, refilled
//          per start-time group and afterwards, from its front, per route
//   Dl     the staged slices of the table being filled, min(W, 24) (one when
//          H = 1) of (n + 1)^2 32-bit words, padded to 8 bytes
//   fixed  dem[16] | cap[K] | st[K] | grp[K] (vehicle -> group) | sel[K]
//          (first appearances while the groups are formed, then the chosen
//          T_k) | gst[G] (the groups' start times), each padded to four words
//   route  G x 2^n   route_g[T], A17's route table of group g
//   rc     2^n       (K >= 2) the routes that fit the vehicle at hand
//   f      K x 2^n   f_1 .. f_K; all stay, the backtrack reads them
// and once per workgroup the binomial table.
//
// Steps (the unbatched entry point's, in one kernel):
//   1. the groups: the distinct start times in order of first appearance;
//   2. per group: stage its slices, zero and fill the table, then route_g[T] =
//      min over (j in T, word) of the word's lowest bit plus the closing edge
//      of that word's slice, unreachable above the horizon, route_g[0] = 0;
//   3. f_1 and A19's layers with rc_k[T] = dem(T) <= cap[k] ? route_g(k)[T] :
//      unreachable (rc is kept while the next vehicle has the same group and
//      capacity; a vehicle with vehicle 0's reads f_1);
//   4. the backtrack on the team's first min(T, 64) lanes: S*, then per
//      vehicle the smallest submask attaining f_{k+1}[S];
//   5. per vehicle with a non-empty T_k: the table's front is refilled as the
//      sub-problem over T_k's customers (node map = T_k's members ascending,
//      start = the vehicle's, horizon = the route's duration) and walked with
//      A16's tie rule into the tour at |S \ T_k| + k, as the unbatched
//      backtrack does step by step.
//
// A request outside the launch's contract -- more than G distinct start
// times, a negative start time or horizon -- gets an all-ones key, an all-zero
// tour and durations of -1, and touches nothing else.
//
// BARRIER RULE.  Every __syncthreads() is reached by every thread of the
// workgroup the same number of times: every loop that contains a barrier runs
// a launch-uniform count (G groups, K vehicles, n layers -- the kernel's
// arguments), never a request's own (its number of groups, |T_k|, the size of
// its served set).  A team with nothing to do in a round -- a group index past
// its own groups, an empty route, a sub-problem smaller than the layer, a team
// past the end of the batch, a request outside the contract -- idles through
// the round and reaches its barriers.  No thread returns before the last
// barrier.  The shared device functions state their barrier counts
// (batch_tdp_fill: exactly `rounds`; the others: none).
#include <hip/hip_runtime.h>

#include <string>

#include "batch_launch.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "tsp_batch_dp.hpp"
#include "tsp_batch_tdp.hpp"
#include "tsp_dp.hpp"
#include "tsp_tdp.hpp"
#include "vrp_batch_sp.hpp"
#include "vrp_sp.hpp"

namespace vrpms {

// the auto team: A20's kBatchTdpTeam[n], or the next larger T whose 256 / T
// requests fit kBatchTdspTeamLds (A20's rule: five workgroups share a CU), and
// 256 if none does.  Unmeasured for this kernel beyond what DESIGN.md §4.3l
// quotes.
constexpr size_t kBatchTdspTeamLds = 32 * 1024;

__constant__ DpBinom kBatchTdspBinom = dp_make_binom();

struct BatchTdspArgs {
  const int32_t* mats;     // [R][H][N][N]
  const int32_t* demand;   // [R][N]
  const int32_t* cap;      // [R][K]
  const int32_t* start;    // [R][K]
  const int32_t* horizon;  // [R]
  int R, N, K, G, H, W;
  int16_t* tours;          // [R][N-1+K]
  uint64_t* keys;          // [R]
  int32_t* durs;           // [R][K]
};

inline size_t batch_tdsp_pad4(int x) { return ((size_t)x + 3) & ~(size_t)3; }

// 32-bit words of dem | cap | st | grp | sel | gst
inline size_t batch_tdsp_fixed_words(int K, int G) {
  return kBatchSpDemWords + 4 * batch_tdsp_pad4(K) + batch_tdsp_pad4(G);
}

inline size_t batch_tdsp_team_bytes(int n, int K, int G, int H, int W) {
  const size_t table = ((size_t)n << (n - 1)) * (size_t)W * 8;
  const size_t mat = ((size_t)batch_tdp_slices(H, W) * (n + 1) * (n + 1) + 1) & ~(size_t)1;
  const size_t sets = (size_t)(G + (K >= 2 ? 1 : 0) + K) * batch_sp_set_words(n);
  return table + (mat + batch_tdsp_fixed_words(K, G) + sets) * 4;
}

inline size_t batch_tdsp_lds_bytes(int n, int K, int G, int H, int W, int T) {
  return (size_t)kBatchDpBinomWords * 4 + (size_t)(256 / T) * batch_tdsp_team_bytes(n, K, G, H, W);
}

inline int batch_tdsp_auto_team(int n, int K, int G, int H, int W) {
  int T = kBatchTdpTeam[n];
  while (T < 256 && batch_tdsp_lds_bytes(n, K, G, H, W, T) > kBatchTdspTeamLds) T *= 2;
  return T;
}

template <int T, int FILL, int OBJ>
__global__ __launch_bounds__(256) void vrp_batch_tdsp_kernel(BatchTdspArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint64_t batch_tdsp_lds[];
  const int N = a.N, n = N - 1, K = a.K, G = a.G, W = a.W, NN2 = N * N;
  const uint32_t half = 1u << (n - 1), sets = 1u << n, full = sets - 1u;
  const uint32_t set_words = (sets + 3u) & ~3u;
  const uint32_t Kp = ((uint32_t)K + 3u) & ~3u, Gp = ((uint32_t)G + 3u) & ~3u;
  const int ns = a.H == 1 ? 1 : (W < 24 ? W : 24);
  const uint32_t table_words = ((uint32_t)n << (n - 1)) * (uint32_t)W;     // 64-bit words
  const uint32_t mat_words = ((uint32_t)(ns * NN2) + 1u) & ~1u;            // 32-bit words
  const uint32_t fixed_words = kBatchSpDemWords + 4u * Kp + Gp;
  const uint32_t small_words = mat_words + fixed_words + ((uint32_t)G + (K >= 2 ? 1u : 0u) + (uint32_t)K) * set_words;
  const uint32_t team_words = table_words + small_words / 2u;              // 64-bit words
  const int team = threadIdx.x / T, tl = threadIdx.x % T;
  const int64_t req = (int64_t)blockIdx.x * (256 / T) + team;
  const bool active = req < a.R;
  constexpr int WL = T < 64 ? T : 64;

  uint32_t* B = reinterpret_cast<uint32_t*>(batch_tdsp_lds);
  uint64_t* tab = batch_tdsp_lds + kBatchDpBinomWords / 2 + (size_t)team * team_words;
  int32_t* Dl = reinterpret_cast<int32_t*>(tab + table_words);
  uint32_t* dem = reinterpret_cast<uint32_t*>(Dl) + mat_words;
  uint32_t* cap = dem + kBatchSpDemWords;
  int32_t* st = reinterpret_cast<int32_t*>(cap + Kp);
  uint32_t* grp = cap + 2u * Kp;
  uint32_t* sel = cap + 3u * Kp;
  int32_t* gst = reinterpret_cast<int32_t*>(cap + 4u * Kp);
  uint32_t* route = cap + 4u * Kp + Gp;                       // route_g at route + g set_words
  uint32_t* rcs = route + (uint32_t)G * set_words;            // only with K >= 2
  uint32_t* f = rcs + (K >= 2 ? set_words : 0u);              // f_{k+1} at f + k set_words
  const int32_t* D = a.mats + (active ? req : 0) * (int64_t)a.H * NN2;

  // 1. the request's scalars, then the groups
  batch_dp_stage_binom(kBatchTdspBinom, B);
  if (active) {
    for (int i = tl; i < kBatchSpDemWords; i += T) dem[i] = i < n ? (uint32_t)a.demand[req * N + i + 1] : 0u;
    for (int k = tl; k < K; k += T) {
      cap[k] = (uint32_t)a.cap[req * K + k];
      st[k] = a.start[req * K + k];
    }
  }
  __syncthreads();
  if (active)
    for (int k = tl; k < K; k += T) {   // sel[k] = the first vehicle with k's start time
      int j = 0;
      while (st[j] != st[k]) ++j;
      sel[k] = (uint32_t)j;
    }
  __syncthreads();
  int ng = 0;          // the request's distinct start times
  bool ok = active;    // inside the launch's contract
  if (active) {
    ok = a.horizon[req] >= 0;
    for (int k = 0; k < K; ++k) {
      ng += sel[k] == (uint32_t)k ? 1 : 0;
      ok = ok && st[k] >= 0;
    }
    ok = ok && ng <= G;
    for (int k = tl; k < K; k += T) {
      const uint32_t j = sel[k];
      uint32_t g = 0;
      for (uint32_t i = 0; i < j; ++i) g += sel[i] == i ? 1u : 0u;
      grp[k] = g;
      if (j == (uint32_t)k && g < (uint32_t)G) gst[g] = st[k];
    }
  }
  __syncthreads();
  const int horizon = ok ? a.horizon[req] : 0;

  // 2. one table and one route_g per group; G is the launch's, a team with
  // fewer groups idles through the rest
  for (int g = 0; g < G; ++g) {
    const bool live = ok && g < ng;
    BatchTdpReq q{0, -1, -1, 0};
    if (live) {
      const int start = gst[g];
      q = batch_tdp_req(start, horizon, W);
      batch_tdp_stage<T>(D, N, a.H, W, ns, start, full, n, tl, Dl, tab);
    }
    __syncthreads();
    batch_tdp_fill<T, FILL>(B, tab, Dl, n, W, ns, q, tl, live, n);
    if (live) {
      uint32_t* rg = route + (uint32_t)g * set_words;
      const int nw = q.lw + 1;
      for (uint32_t S = tl; S < sets; S += T) {
        uint32_t best = S ? kSpInf : 0u;
        for (uint32_t m = S; m; m &= m - 1u) {
          const int j = __builtin_ctz(m);
          const uint64_t* row = tab + (size_t)(j * half + batch_dp_squeeze(S, j)) * W;
          for (int w = 0; w < nw; ++w) {
            const uint64_t x = row[w];
            if (!x) continue;
            const int64_t val =
                (int64_t)(60 * w + __builtin_ctzll(x) - q.off) + Dl[((w % 24 % ns) * N + j + 1) * N];
            if (val >= 0 && val <= q.hz) best = min(best, (uint32_t)val);
          }
        }
        rg[S] = best;
      }
    }
    __syncthreads();
  }

  // 3. f_1 = vehicle 0's routes that fit, then the K - 1 layers
  if (ok) {
    const uint32_t cap0 = cap[0];
    const uint32_t* r0 = route + grp[0] * set_words;
    for (uint32_t S = tl; S < sets; S += T) f[S] = batch_sp_demand(dem, S) <= cap0 ? r0[S] : kSpInf;
  }
  __syncthreads();
  uint32_t held_cap = 0, held_grp = 0;   // the (group, capacity) rcs holds
  bool holds = false;
  for (int k = 1; k < K; ++k) {
    const uint32_t* rc = f;
    if (ok) {
      const uint32_t capk = cap[k], gk = grp[k];
      if (capk != cap[0] || gk != grp[0]) {
        rc = rcs;
        if (!holds || held_cap != capk || held_grp != gk) {
          const uint32_t* rg = route + gk * set_words;
          for (uint32_t S = tl; S < sets; S += T) rcs[S] = batch_sp_demand(dem, S) <= capk ? rg[S] : kSpInf;
          holds = true;
          held_cap = capk;
          held_grp = gk;
        }
      }
    }
    __syncthreads();
    batch_sp_layer<T, OBJ>(B, n, rc, f + (uint32_t)(k - 1) * set_words, f + (uint32_t)k * set_words, tl, ok);
    __syncthreads();
  }

  // 4. the backtrack: S*, then T_k for k = K-1 .. 1 (vehicle 0 takes what is
  // left) into sel[]
  uint32_t served = 0;
  if (ok && tl < WL) {
    const uint32_t* fK = f + (uint32_t)(K - 1) * set_words;
    uint64_t top = ~0ull;   // least (unserved, f_K[S], S) over the reachable S; S = 0 always is
    for (uint32_t S = tl; S < sets; S += WL) {
      const uint32_t v = fK[S];
      const uint64_t t = ((uint64_t)(n - __popc(S)) << 52) | ((uint64_t)v << 20) | S;
      if (v != kSpInf && t < top) top = t;
    }
#pragma unroll
    for (int off = WL / 2; off > 0; off >>= 1) {
      const uint64_t o = __shfl_xor(top, off, WL);
      top = o < top ? o : top;
    }
    served = (uint32_t)top & full;
    uint32_t S = served;
    for (int k = K - 1; k >= 0; --k) {
      uint32_t Tk = S;
      if (k > 0) {
        const uint32_t want = f[(uint32_t)k * set_words + S];
        const uint32_t capk = cap[k];
        const uint32_t* rg = route + grp[k] * set_words;
        const uint32_t* fk = f + (uint32_t)(k - 1) * set_words;
        const uint32_t cnt = 1u << __popc(S);
        Tk = kSpInf;
        for (uint32_t b = 0; b < cnt && Tk == kSpInf; b += WL) {
          uint32_t hit = kSpInf;
          if (b + tl < cnt) {
            const uint32_t t = sp_deposit(b + tl, S);
            const uint32_t fv = fk[S ^ t], rt = rg[t];
            if (fv != kSpInf && rt != kSpInf && batch_sp_demand(dem, t) <= capk &&
                (OBJ ? max(rt, fv) : rt + fv) == want)
              hit = t;
          }
          Tk = batch_sp_group_min<WL>(hit);   // ranks increase with the mask: the least mask
        }
        if (Tk == kSpInf) Tk = 0;  // cannot happen: want was built from one such T
      }
      if (tl == 0) sel[k] = Tk;
      S ^= Tk;
    }
  }
  __syncthreads();

  // 5. the routes: K rounds, each a refill of the table's front and a walk; a
  // team whose vehicle k is empty idles through round k
  int16_t* tour = a.tours + (active ? req : 0) * (n + K);
  uint32_t S = served, dsum = 0, dmax = 0;   // meaningful on the walking lanes
  for (int k = K - 1; k >= 0; --k) {
    const uint32_t Tk = ok ? sel[k] : 0u;
    const int m = __popc(Tk);
    const uint32_t rt = ok ? route[grp[k] * set_words + Tk] : 0u;
    const bool live = Tk != 0u && rt != kSpInf;   // a chosen route is reachable
    BatchTdpReq q{0, -1, -1, 0};
    if (live) {
      q = batch_tdp_req(st[k], (int)rt, W);
      batch_tdp_stage<T>(D, N, a.H, W, ns, st[k], Tk, m, tl, Dl, tab);
    }
    __syncthreads();
    batch_tdp_fill<T, FILL>(B, tab, Dl, m, W, ns, q, tl, live, n);
    if (ok && tl < WL) {
      S ^= Tk;
      const int pos = __popc(S) + k;
      if (live) batch_tdp_walk<T>(tab, Dl, m, W, ns, q, Tk, tl, true, tour + pos);
      if (tl == 0) {
        tour[pos + m] = 0;
        a.durs[req * K + k] = (int32_t)rt;
      }
      dsum += rt;
      dmax = max(dmax, rt);
    }
    __syncthreads();
  }

  if (!active || tl != 0) return;
  if (!ok) {
    for (int i = 0; i < n + K; ++i) tour[i] = 0;
    for (int k = 0; k < K; ++k) a.durs[req * K + k] = -1;
    a.keys[req] = ~0ull;
    return;
  }
  int pos = __popc(served) + K;
  for (int c = 0; c < n; ++c)
    if (!((served >> c) & 1u)) tour[pos++] = (int16_t)(c + 1);
  a.keys[req] = cvrp_key((uint32_t)(n - __popc(served)), dsum, dmax, OBJ);
}

// the argument checks both entry points share, in the established order; N
// is n + 1 and what the message names is chosen by `launch`
static int batch_tdsp_check(const char* who, bool launch, int n, int K, int G, int H, int W) {
  const std::string f(who);
  if (n < 1 || n > kBatchTdpMaxN)
    return fail(VRPMS_EINVAL, f + (launch ? ": the LDS-resident state needs 2 <= N <= 12 (N = " +
                                                std::to_string(n + 1) + " given)"
                                          : ": the LDS-resident state needs 1 <= n <= 11 (n = " +
                                                std::to_string(n) + " given)"));
  if (K < 1 || K > kBatchSpMaxK)
    return fail(VRPMS_EINVAL, f + ": the time-expanded partition DP needs 1 <= K <= 64 (" +
                                  std::to_string(K) + " given)");
  if (G < 1 || G > K)
    return fail(VRPMS_EINVAL, f + ": the limit on distinct start times must be in 1 <= G <= K (" +
                                  std::to_string(G) + " given)");
  if (H != 1 && H != 24)
    return fail(VRPMS_EINVAL, f + ": the matrices must be static or have 24 hour slices (H = " +
                                  std::to_string(H) + " given)");
  if (W < 1 || W > kTdpMaxWords)
    return fail(VRPMS_EINVAL, f + ": a row has 1 <= W <= 512 hour words (" + std::to_string(W) +
                                  " given)");
  return VRPMS_OK;
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_vrp_batch_tdsp_lds(int32_t n, int32_t K, int32_t G, int32_t H, int32_t W,
                                        int32_t team, uint64_t* bytes) {
  if (!bytes) return fail(VRPMS_EINVAL, "vrpms_vrp_batch_tdsp_lds: bytes is NULL");
  const int rc = batch_tdsp_check("vrpms_vrp_batch_tdsp_lds", false, n, K, G, H, W);
  if (rc != VRPMS_OK) return rc;
  if (!batch_team_ok(team)) return batch_team_fail("vrpms_vrp_batch_tdsp_lds", team);
  *bytes = batch_tdsp_lds_bytes(n, K, G, H, W, team ? team : batch_tdsp_auto_team(n, K, G, H, W));
  return VRPMS_OK;
}

extern "C" int vrpms_vrp_batch_tdsp(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                                    const int32_t* d_cap, const int32_t* d_start,
                                    const int32_t* d_horizon, int32_t R, int32_t N, int32_t K,
                                    int32_t G, int32_t H, int32_t W, int32_t objective, int32_t team,
                                    int16_t* d_tours, uint64_t* d_keys, int32_t* d_durs,
                                    void* stream) {
  if (!ctx) return fail(VRPMS_EINVAL, "vrpms_vrp_batch_tdsp: ctx is NULL");
  if (R < 0) return fail(VRPMS_EINVAL, "vrpms_vrp_batch_tdsp: R must not be negative");
  const int rc = batch_tdsp_check("vrpms_vrp_batch_tdsp", true, N - 1, K, G, H, W);
  if (rc != VRPMS_OK) return rc;
  if (objective != VRPMS_OBJ_SUM && objective != VRPMS_OBJ_MAX)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_tdsp: objective must be VRPMS_OBJ_SUM or VRPMS_OBJ_MAX");
  if (!batch_team_ok(team)) return batch_team_fail("vrpms_vrp_batch_tdsp", team);
  if (R == 0) return VRPMS_OK;
  if (!d_mats || !d_demand || !d_cap || !d_start || !d_horizon || !d_tours || !d_keys || !d_durs)
    return fail(VRPMS_EINVAL,
                "vrpms_vrp_batch_tdsp: NULL matrix/demand/capacity/start/horizon/tour/key/duration buffer");
  const int n = N - 1;
  const int T = team ? team : batch_tdsp_auto_team(n, K, G, H, W);
  const size_t lds = batch_tdsp_lds_bytes(n, K, G, H, W, T);
  if (lds > ctx->max_lds)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_tdsp: " + std::to_string(256 / T) + " requests of n = " +
                                  std::to_string(n) + ", K = " + std::to_string(K) + ", G = " +
                                  std::to_string(G) + ", W = " + std::to_string(W) + " need " +
                                  std::to_string(lds) + " bytes of LDS (" +
                                  std::to_string(ctx->max_lds) + " available)");
  VRPMS_HIP(hipSetDevice(ctx->device));
  const BatchTdspArgs a{d_mats, d_demand, d_cap, d_start, d_horizon, R, N, K, G, H, W, d_tours, d_keys, d_durs};
  hipStream_t s = (hipStream_t)stream;
  const bool atomic = batch_tdp_atomic(W), mx = objective == VRPMS_OBJ_MAX;
  const hipError_t e = batch_with_team(T, [&](auto t) {
    constexpr int TT = decltype(t)::value;
    return batch_launch(atomic ? (mx ? vrp_batch_tdsp_kernel<TT, 1, 1> : vrp_batch_tdsp_kernel<TT, 1, 0>)
                               : (mx ? vrp_batch_tdsp_kernel<TT, 0, 1> : vrp_batch_tdsp_kernel<TT, 0, 0>),
                        a, R, T, lds, s);
  });
  VRPMS_HIP(e);
  return VRPMS_OK;
}
