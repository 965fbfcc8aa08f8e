// Batched exact VRP: the subset partition DP for many small requests, each
// request's whole state in LDS.
//
// The recurrence, the tie rule and the result are vrp_sp.hip's (A15), per
// request; the Held-Karp table is tsp_batch_dp.hip's compact one (A18), filled
// by the same device functions (tsp_batch_dp.hpp).  A team of T threads owns
// one request, a 256-thread workgroup holds 256 / T requests of the same N and
// K, so every barrier is workgroup-uniform; a team past the end of the batch
// reaches every barrier and touches no memory.  Only the matrix, the demands
// and the capacities are read from memory, only the tour, the key and the K
// route durations are written to it.
//
// One team's LDS, in 32-bit words (every part padded to four):
//   Dr    13 x 16      the matrix image, Dr[node][i] = D[node][i + 1]
//   dem   16           dem[i] = the demand of customer i + 1
//   cap   K
//   g     n 2^(n-1)    the compact Held-Karp table g[j][c]
//   route 2^n          route[T] = min over i in T of D[0][i] + g[T \ {i}][i]
//   rc    2^n          (K >= 2) vehicle k's routes that fit: dem(T) <= cap[k] ?
//                      route[T] : unreachable.  A vehicle with cap[0] reads f_1
//                      instead, one with the capacity rc already holds reuses it.
//   f     K x 2^n      f_1 .. f_K; all stay, the backtrack reads them
// and once per workgroup the binomial table.
//
// A partition layer f_{k+1}[S] = min over T subset of S of rc_k[T] (+) f_k[S \ T]
// costs 2^|S| steps for S, so a set is not one thread's: a group of four lanes
// shares S, lane l fixes its own pattern on the (at most) two lowest
// customers of S and steps through the submasks of the rest, and a four-lane
// minimum ends S.  The sets of one cardinality are dealt to the team's T / 4
// groups in consecutive runs of ranks (unrank the first, Gosper to the next),
// the groups rotated from one cardinality to the next so that the run that is
// one set longer does not land on the same group every time.
//
// The backtrack runs on the team's first min(T, 64) lanes, which lie in one
// wavefront: S* by a packed-tuple minimum over f_K, then per vehicle
// k = K-1 .. 1 the smallest submask of the remaining set that attains
// f_{k+1}[S] (ranks in increasing order, min(T, 64) at a time; vehicle 0 takes
// what is left), and at once A14's forward walk on it by 16 lanes, written at
// the position the remaining set fixes: routes 0..k serve exactly S, so route
// k starts at |S \ T_k| + k.
#include <hip/hip_runtime.h>

#include <string>

#include "batch_launch.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "tsp_batch_dp.hpp"
#include "tsp_dp.hpp"
#include "vrp_batch_sp.hpp"
#include "vrp_sp.hpp"

namespace vrpms {

// the LDS of one CU of gfx950: what the auto team is sized for.  The launch
// itself checks ctx->max_lds
constexpr size_t kBatchSpLdsBytes = 160 * 1024;

// threads per request by n (index n), before the LDS has its say: the fastest
// T of tools/batch_sp_rate.py --teams 16,32,64,128,256 at K = 3 (K = 1 at
// n = 12; DESIGN.md §4.3j has the measurements; n = 1 is not measured and
// takes n = 2's).  Where 256 / T requests of (n, K) do not fit the LDS the
// auto team is the next larger T that does
constexpr int kBatchSpTeam[kBatchDpMaxN + 1] = {16, 16, 16, 16, 16, 16, 32, 64, 128, 256, 256, 256,
                                                256};

__constant__ DpBinom kBatchSpBinom = dp_make_binom();

struct BatchSpArgs {
  const int32_t* mats;    // [R][N][N]
  const int32_t* demand;  // [R][N]
  const int32_t* cap;     // [R][K]
  int R, N, K;
  int16_t* tours;         // [R][N-1+K]
  uint64_t* keys;         // [R]
  int32_t* durs;          // [R][K]
};

inline size_t batch_sp_fixed_words(int K) { return kBatchSpDemWords + (((size_t)K + 3) & ~(size_t)3); }

inline size_t batch_sp_team_words(int n, int K) {
  return kBatchDpMatWords + batch_sp_fixed_words(K) + batch_dp_table_words(n) +
         (size_t)(1 + (K >= 2 ? 1 : 0) + K) * batch_sp_set_words(n);
}

inline size_t batch_sp_lds_bytes(int n, int K, int T) {
  return (kBatchDpBinomWords + (size_t)(256 / T) * batch_sp_team_words(n, K)) * 4;
}

// the table's T, or the next larger one whose 256 / T requests fit; 256 if none does
inline int batch_sp_auto_team(int n, int K) {
  int T = kBatchSpTeam[n];
  while (T < 256 && batch_sp_lds_bytes(n, K, T) > kBatchSpLdsBytes) T *= 2;
  return T;
}

template <int T, int OBJ>
__global__ __launch_bounds__(256) void vrp_batch_sp_kernel(BatchSpArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t batch_sp_lds[];
  const int N = a.N, n = N - 1, K = a.K;
  const uint32_t half = 1u << (n - 1), sets = 1u << n;
  const uint32_t set_words = (sets + 3u) & ~3u;
  const uint32_t fixed_words = kBatchSpDemWords + (((uint32_t)K + 3u) & ~3u);
  const uint32_t table_words = (((uint32_t)n << (n - 1)) + 3u) & ~3u;
  const uint32_t team_words =
      kBatchDpMatWords + fixed_words + table_words + (1u + (K >= 2 ? 1u : 0u) + (uint32_t)K) * set_words;
  const int team = threadIdx.x / T, tl = threadIdx.x % T;
  const int64_t req = (int64_t)blockIdx.x * (256 / T) + team;
  const bool active = req < a.R;

  uint32_t* B = batch_sp_lds;
  uint32_t* Dr = batch_sp_lds + kBatchDpBinomWords + team * team_words;
  uint32_t* dem = Dr + kBatchDpMatWords;
  uint32_t* cap = dem + kBatchSpDemWords;
  uint32_t* g = Dr + kBatchDpMatWords + fixed_words;
  uint32_t* route = g + table_words;
  uint32_t* rcs = route + set_words;                    // only with K >= 2
  uint32_t* f = route + (K >= 2 ? 2u : 1u) * set_words; // f_{k+1} at f + k set_words

  batch_dp_stage_binom(kBatchSpBinom, B);
  if (active) {
    batch_dp_stage<T>(a.mats + req * N * N, N, tl, Dr, g);
    for (int i = tl; i < kBatchSpDemWords; i += T) dem[i] = i < n ? (uint32_t)a.demand[req * N + i + 1] : 0u;
    for (int k = tl; k < K; k += T) cap[k] = (uint32_t)a.cap[req * K + k];
  }
  __syncthreads();

  batch_dp_fill<T>(B, Dr, g, n, tl, active);

  // route[] and f_1 = vehicle 0's routes that fit
  if (active) {
    const uint32_t cap0 = cap[0];
    for (uint32_t S = tl; S < sets; S += T) {
      uint32_t val = S ? kSpInf : 0u;
      for (uint32_t m = S; m; m &= m - 1u) {
        const int i = __builtin_ctz(m);
        val = min(val, Dr[i] + g[i * half + batch_dp_squeeze(S, i)]);
      }
      route[S] = val;
      f[S] = batch_sp_demand(dem, S) <= cap0 ? val : kSpInf;
    }
  }
  __syncthreads();

  uint32_t held = 0;       // the capacity rcs holds
  bool holds = false;
  for (int k = 1; k < K; ++k) {
    const uint32_t* rc = f;
    if (active) {
      const uint32_t capk = cap[k];
      if (capk != cap[0]) {
        rc = rcs;
        if (!holds || held != capk) {
          for (uint32_t S = tl; S < sets; S += T)
            rcs[S] = batch_sp_demand(dem, S) <= capk ? route[S] : kSpInf;
          holds = true;
          held = capk;
        }
      }
    }
    __syncthreads();
    batch_sp_layer<T, OBJ>(B, n, rc, f + (uint32_t)(k - 1) * set_words, f + (uint32_t)k * set_words, tl,
                           active);
    __syncthreads();
  }

  constexpr int W = T < 64 ? T : 64;
  if (!active || tl >= W) return;
  const uint32_t* fK = f + (uint32_t)(K - 1) * set_words;
  uint64_t top = ~0ull;   // least (unserved, f_K[S], S) over the reachable S; S = 0 always is
  for (uint32_t S = tl; S < sets; S += W) {
    const uint32_t v = fK[S];
    const uint64_t t = ((uint64_t)(n - __popc(S)) << 52) | ((uint64_t)v << 20) | S;
    if (v != kSpInf && t < top) top = t;
  }
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor(top, off, W);
    top = o < top ? o : top;
  }
  const uint32_t served = (uint32_t)top & (sets - 1u);

  const int l = tl & 15;   // the walk's lane: every 16-lane group of the W walks alike
  int16_t* tour = a.tours + req * (n + K);
  uint32_t S = served, dsum = 0, dmax = 0;
  for (int k = K - 1; k >= 0; --k) {
    uint32_t Tk = S;       // vehicle 0 takes what is left: f_1[S] is route[S]
    if (k > 0) {
      const uint32_t want = f[(uint32_t)k * set_words + S];
      const uint32_t capk = cap[k];
      const uint32_t* fk = f + (uint32_t)(k - 1) * set_words;
      const uint32_t cnt = 1u << __popc(S);
      Tk = kSpInf;
      for (uint32_t b = 0; b < cnt && Tk == kSpInf; b += W) {
        uint32_t hit = kSpInf;
        if (b + tl < cnt) {
          const uint32_t t = sp_deposit(b + tl, S);
          const uint32_t fv = fk[S ^ t];
          if (fv != kSpInf && batch_sp_demand(dem, t) <= capk) {
            const uint32_t rt = route[t];
            if ((OBJ ? max(rt, fv) : rt + fv) == want) hit = t;
          }
        }
        Tk = batch_sp_group_min<W>(hit);   // ranks increase with the mask: the least mask
      }
      if (Tk == kSpInf) Tk = 0;  // cannot happen: want was built from one such T
    }
    const uint32_t rt = route[Tk];
    dsum += rt;
    dmax = max(dmax, rt);
    if (tl == 0) a.durs[req * K + k] = (int32_t)rt;
    S ^= Tk;
    int pos = __popc(S) + k, cur = 0;
    for (uint32_t Rm = Tk; Rm;) {
      uint32_t val = kSpInf;
      if (l < n && ((Rm >> l) & 1u))
        val = Dr[cur * kBatchDpRow + l] + g[l * half + batch_dp_squeeze(Rm, l)];
      uint64_t v = ((uint64_t)val << 8) | (uint32_t)l;
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 16);
        v = o < v ? o : v;
      }
      const int i = (int)(v & 0xffu);
      if (tl == 0) tour[pos] = (int16_t)(i + 1);
      ++pos;
      cur = i + 1;
      Rm &= ~(1u << i);
    }
    if (tl == 0) tour[pos] = 0;
  }
  if (tl == 0) {
    int pos = __popc(served) + K;
    for (int c = 0; c < n; ++c)
      if (!((served >> c) & 1u)) tour[pos++] = (int16_t)(c + 1);
    a.keys[req] = cvrp_key((uint32_t)(n - __popc(served)), dsum, dmax, OBJ);
  }
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_vrp_batch_sp_lds(int32_t n, int32_t K, int32_t team, uint64_t* bytes) {
  if (!bytes) return fail(VRPMS_EINVAL, "vrpms_vrp_batch_sp_lds: bytes is NULL");
  if (n < 1 || n > kBatchDpMaxN)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_sp_lds: the LDS-resident state needs 1 <= n <= 12 (" +
                                  std::to_string(n) + " given)");
  if (K < 1 || K > kBatchSpMaxK)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_sp_lds: set partitioning needs 1 <= K <= 64 (" +
                                  std::to_string(K) + " given)");
  if (!batch_team_ok(team)) return batch_team_fail("vrpms_vrp_batch_sp_lds", team);
  *bytes = batch_sp_lds_bytes(n, K, team ? team : batch_sp_auto_team(n, K));
  return VRPMS_OK;
}

extern "C" int vrpms_vrp_batch_sp(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                                  const int32_t* d_cap, int32_t R, int32_t N, int32_t K,
                                  int32_t objective, int32_t team, int16_t* d_tours, uint64_t* d_keys,
                                  int32_t* d_durs, void* stream) {
  if (!ctx) return fail(VRPMS_EINVAL, "vrpms_vrp_batch_sp: ctx is NULL");
  if (R < 0) return fail(VRPMS_EINVAL, "vrpms_vrp_batch_sp: R must not be negative");
  if (N < 2 || N > kBatchDpNodes)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_sp: the LDS-resident state needs 2 <= N <= 13 (" +
                                  std::to_string(N) + " given)");
  if (K < 1 || K > kBatchSpMaxK)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_sp: set partitioning needs 1 <= K <= 64 (" +
                                  std::to_string(K) + " given)");
  if (objective != VRPMS_OBJ_SUM && objective != VRPMS_OBJ_MAX)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_sp: objective must be VRPMS_OBJ_SUM or VRPMS_OBJ_MAX");
  if (!batch_team_ok(team)) return batch_team_fail("vrpms_vrp_batch_sp", team);
  if (R == 0) return VRPMS_OK;
  if (!d_mats || !d_demand || !d_cap || !d_tours || !d_keys || !d_durs)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_sp: NULL matrix/demand/capacity/tour/key/duration buffer");
  const int n = N - 1;
  const int T = team ? team : batch_sp_auto_team(n, K);
  const size_t lds = batch_sp_lds_bytes(n, K, T);
  if (lds > ctx->max_lds)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_sp: " + std::to_string(256 / T) + " requests of n = " +
                                  std::to_string(n) + ", K = " + std::to_string(K) + " need " +
                                  std::to_string(lds) + " bytes of LDS (" +
                                  std::to_string(ctx->max_lds) + " available)");
  VRPMS_HIP(hipSetDevice(ctx->device));
  const BatchSpArgs a{d_mats, d_demand, d_cap, R, N, K, d_tours, d_keys, d_durs};
  hipStream_t s = (hipStream_t)stream;
  const bool mx = objective == VRPMS_OBJ_MAX;
  const hipError_t e = batch_with_team(T, [&](auto t) {
    constexpr int TT = decltype(t)::value;
    return batch_launch(mx ? vrp_batch_sp_kernel<TT, 1> : vrp_batch_sp_kernel<TT, 0>, a, R, T, lds, s);
  });
  VRPMS_HIP(e);
  return VRPMS_OK;
}
