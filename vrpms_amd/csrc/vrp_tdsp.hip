// Exact time-dependent CVRP by time-expanded partition dynamic programming
// (DESIGN.md §2 A17, §4.3h).
//
// A15's partition recurrence (vrp_sp.hip) does not care where the route
// durations come from, and A16's clock table (tsp_tdp.hip), filled for a start
// time s over all subsets, holds every route's clock set: with R built for s
// and `horizon`
//   route_s[T] = min over j in T and the bits b of R[T][j] of
//                b + D[hour(b)][j][0] - s          (route_s[{}] = 0)
// where only values <= horizon count (otherwise 0xffffffff: unreachable,
// treated by the recurrence exactly like a route over capacity).  Within one
// word the slice is constant, so a word's lowest bit is its best: one
// candidate per (j, word).  One table is built per distinct start time, and
// vehicle k uses route_{start_times[k]}.
//
// Workspace: R [2^n][n][Wws] uint64 (the A16 table, Wws the row width of
// vrpms_vrp_tdsp_workspace; every start's own W <= Wws) | route_0 .. route_{G-1}
// [G][2^n] | dem [2^n] | routecap [2^n] | f_1 .. f_K [K][2^n], all uint32 | a
// tail of 8 K + 16 bytes: one uint64 the route walks' keys go to, then S* and
// the K pairs (T_k, duration).  The table is reused across start times, and
// afterwards, from its front, by the per-route tables of the backtrack.
//
//   vrp_tdsp_dem_kernel     dem[T] for every mask.
//   vrp_tdsp_route_kernel   after one start's fill: route_s[T] for every mask.
//                           A wavefront owns a mask; its lanes take the
//                           (j in T, word) pairs in row order (consecutive
//                           lanes, consecutive words of one row: coalesced;
//                           rows with j not in T are never written and never
//                           read), form 60 w + ctz(x) - off + D[slice(w)][j][0],
//                           drop values above the horizon, and a wave minimum
//                           ends the mask.  With n W < 64 a wavefront takes
//                           64 / L masks at a time, L the power of two >= n W
//                           lanes each.  It re-reads the table once (the rows
//                           with j in T: half of it).
//   vrp_sp_cap_kernel, vrp_sp_layer_kernel   unchanged (vrp_sp.hpp): routecap
//                           for vehicle k from route_{g(k)} and cap[k], g(k)
//                           the index of its start time among the distinct
//                           ones; a fleet with one start time and equal
//                           capacities keeps A15's shortcut (f_1 is routecap).
//   vrp_tdsp_choose_kernel  one workgroup: A15 tie-rule steps (1) and (2) --
//                           S*, then per vehicle the smallest submask T_k
//                           attaining f_{k+1}[S] -- into the tail.
// The entry point then synchronises the stream ONCE and reads the K pairs
// back: the launch shapes of what follows (table width and customer count per
// route) depend on them.  For each non-empty T_k it refills a table over T_k's
// customers alone (node map = T_k's members in ascending order, start =
// start_times[k], horizon = that route's duration) and tsp_tdp_walk_kernel
// writes R_k, A16's tie-ruled tour, at its offset in d_tour: the main tables
// were overwritten by later start times, so routes are recomputed rather than
// walked in place.
//   vrp_tdsp_finish_kernel  separators, unserved customers, key.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.hpp"
#include "ctx.hpp"
#include "tsp_tdp.hpp"
#include "vrp_sp.hpp"

namespace vrpms {

__global__ __launch_bounds__(256) void vrp_tdsp_dem_kernel(const int32_t* demand, int n, uint32_t* dem) {
  const uint32_t T = blockIdx.x * 256u + threadIdx.x;
  if (T >> n) return;
  uint64_t d = 0;
  for (int c = 0; c < n; ++c)
    if (T >> c & 1u) d += (uint32_t)demand[c + 1];
  dem[T] = d < kSpInf ? (uint32_t)d : kSpInf;
}

struct TdspRouteArgs {
  const int32_t* D;  // [H][N][N] of the loaded instance
  int N, H, n, W;
  int h0m, off;      // slice of word 0, the start's bit in word 0 (as TdpArgs)
  int horizon;
  int L;             // lanes per mask: 64, or the power of two >= n W below it
  const uint64_t* R; // [2^n][n][W]
  uint32_t* route;   // [2^n]
};

__global__ __launch_bounds__(256) void vrp_tdsp_route_kernel(TdspRouteArgs a) {
  __shared__ int32_t back[24 * kTdpMaxN];  // back[h n + c] = D[h][c + 1][0]
  const int n = a.n, W = a.W, L = a.L;
  for (int e = threadIdx.x; e < a.H * n; e += 256) {
    const int h = e / n, c = e - h * n;
    back[e] = a.D[((int64_t)h * a.N + c + 1) * a.N];
  }
  __syncthreads();
  const uint32_t full = 1u << n;
  const int sub = threadIdx.x & (L - 1);
  // lane -> (member index p, word w) of item `sub`, and the step of L items
  const int pstep = L / W, wstep = L - pstep * W;
  const int p0 = sub / W, w0 = sub - p0 * W;
  const uint64_t* __restrict__ R = a.R;
  const uint32_t per_wave = 64u / (uint32_t)L;
  const uint32_t stride = gridDim.x * 4u * per_wave;
  // `base` is wave-uniform: the shuffles below run with every lane present
  for (uint32_t base = (blockIdx.x * 4u + (threadIdx.x >> 6)) * per_wave; base < full; base += stride) {
    const uint32_t T = base + ((threadIdx.x & 63u) / (uint32_t)L);
    const bool valid = T < full;
    const int items = valid ? __builtin_popcount(T) * W : 0;
    uint32_t best = kSpInf;
    uint32_t m = T;   // T without its first p members
    int w = w0;
    for (int i = 0; i < p0; ++i) m &= m - 1u;
    for (int e = sub; e < items; e += L) {
      const int c = __builtin_ctz(m);   // e < |T| W: m is not empty
      const uint64_t x = R[((uint64_t)T * n + c) * W + w];
      if (x) {
        const int slice = a.H == 1 ? 0 : (a.h0m + w) % 24;
        const int64_t val = (int64_t)(60 * w + __builtin_ctzll(x) - a.off) + back[slice * n + c];
        if (val <= a.horizon) best = min(best, (uint32_t)val);
      }
      int dp = pstep;
      w += wstep;
      if (w >= W) {
        w -= W;
        ++dp;
      }
      for (int i = 0; i < dp; ++i) m &= m - 1u;
    }
    for (int o = L >> 1; o > 0; o >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o, kWave));
    if (valid && sub == 0) a.route[T] = T ? best : 0u;
  }
}

struct TdspChooseArgs {
  int n, K, objective;
  const uint32_t* routes;  // [G][2^n]
  const uint32_t* dem;     // [2^n]
  const uint32_t* f;       // f_1 .. f_K, [K][2^n]
  const int32_t* cap;      // [K]
  uint32_t* out;           // S*, then (T_k, duration) for k = 0..K-1
  uint8_t grp[kSpMaxK];    // vehicle -> index of its start time among the distinct ones
};

__global__ __launch_bounds__(1024) void vrp_tdsp_choose_kernel(TdspChooseArgs a) {
  __shared__ uint64_t red[16];
  __shared__ uint32_t found;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = a.n, K = a.K;
  const uint32_t full = 1u << n;

  // S*: least (unserved, f_K[S], S) over the reachable S; S = 0 always is
  uint64_t best = ~0ull;
  {
    const uint32_t* fK = a.f + ((size_t)(K - 1) << n);
    for (uint32_t S = tid; S < full; S += 1024) {
      const uint32_t v = fK[S];
      const uint64_t t = ((uint64_t)(n - __popc(S)) << 52) | ((uint64_t)v << 20) | S;
      if (v != kSpInf && t < best) best = t;
    }
    best = wave_min_u64(best);
    if (lane == 0) red[wv] = best;
    __syncthreads();
    for (int i = 0; i < 16; ++i) best = red[i] < best ? red[i] : best;
  }
  const uint32_t served = (uint32_t)best & (full - 1u);
  if (tid == 0) a.out[0] = served;

  // T_k for k = K-1 .. 0: the smallest submask of the remaining S that
  // attains f_{k+1}[S], found 1024 submask ranks at a time in increasing order
  uint32_t S = served;
  for (int k = K - 1; k >= 0; --k) {
    const uint32_t want = a.f[((size_t)k << n) + S];
    const uint32_t capk = (uint32_t)a.cap[k];
    const uint32_t* route = a.routes + ((size_t)a.grp[k] << n);
    const uint32_t* fk = k ? a.f + ((size_t)(k - 1) << n) : nullptr;
    const uint32_t cnt = 1u << __popc(S);
    uint32_t T = kSpInf;
    for (uint32_t b = 0; b < cnt && T == kSpInf; b += 1024) {
      if (tid == 0) found = kSpInf;
      __syncthreads();
      const uint32_t r = b + tid;
      if (r < cnt) {
        const uint32_t t = sp_deposit(r, S), rest = S ^ t;
        if (a.dem[t] <= capk) {
          const uint32_t fv = k ? fk[rest] : (rest ? kSpInf : 0u);
          const uint32_t rt = route[t];
          if (fv != kSpInf && rt != kSpInf && (a.objective ? max(rt, fv) : rt + fv) == want)
            atomicMin(&found, t);
        }
      }
      __syncthreads();
      T = found;
      __syncthreads();
    }
    if (T == kSpInf) T = 0;  // cannot happen: want was built from one such T
    if (tid == 0) {
      a.out[1 + 2 * k] = T;
      a.out[2 + 2 * k] = route[T];
    }
    S ^= T;
  }
}

// one lane: a separator behind each route (the walks wrote the routes), the
// unserved customers in ascending order, the key
__global__ __launch_bounds__(64) void vrp_tdsp_finish_kernel(int n, int K, int objective, const uint32_t* out,
                                                             int16_t* tour, uint64_t* key) {
  if (threadIdx.x != 0) return;
  const uint32_t served = out[0];
  int pos = 0;
  uint32_t dsum = 0, dmax = 0;
  for (int k = 0; k < K; ++k) {
    const uint32_t rt = out[2 + 2 * k];
    pos += __popc(out[1 + 2 * k]);
    tour[pos++] = 0;
    dsum += rt;
    dmax = max(dmax, rt);
  }
  for (int c = 0; c < n; ++c)
    if (!((served >> c) & 1u)) tour[pos++] = (int16_t)(c + 1);
  *key = cvrp_key((uint32_t)(n - __popc(served)), dsum, dmax, objective);
}

// the workspace's words per row: at least tdp_words(start, horizon) of every
// start <= max_start; 0 when out of range
static int tdsp_words(int64_t max_start, int64_t horizon) {
  if (max_start + horizon >= 2147483648LL) return 0;
  const int64_t W = (std::min<int64_t>(59, max_start) + horizon) / 60 + 1;
  return W > kTdpMaxWords ? 0 : (int)W;
}

static uint64_t tdsp_bytes(int n, int K, int G, int W) {
  return (((uint64_t)1 << n) * (uint64_t)n * (uint64_t)W) * 8u +
         ((uint64_t)4 << n) * (uint64_t)(G + K + 2) + 8u * (uint64_t)K + 16u;
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_vrp_tdsp_workspace(int32_t n, int32_t K, int32_t G, int32_t max_start,
                                        int32_t horizon, uint64_t* bytes) {
  if (!bytes) return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_workspace: bytes is NULL");
  if (n < 1 || n > kTdpMaxN)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_workspace: the time-expanded partition DP needs 1 <= n <= 20");
  if (K < 1 || K > kSpMaxK)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_workspace: the time-expanded partition DP needs 1 <= K <= 64");
  if (G < 1 || G > K)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_workspace: the number of distinct start times must be in [1, K]");
  if (max_start < 0 || horizon < 0)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_workspace: start time and horizon must be >= 0");
  const int W = tdsp_words(max_start, horizon);
  if (!W)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_workspace: horizon of " + std::to_string(horizon) +
                                  " minutes needs more than " + std::to_string(kTdpMaxWords) +
                                  " hour words per state");
  *bytes = tdsp_bytes(n, K, G, W);
  return VRPMS_OK;
}

extern "C" int vrpms_vrp_tdsp_run(vrpms_ctx* ctx, int32_t n, int32_t horizon, void* d_work,
                                  uint64_t work_bytes, int16_t* d_tour, uint64_t* d_key,
                                  void* stream) {
  if (!ctx) return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_run: ctx is NULL");
  if (!d_work || !d_tour || !d_key)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_run: NULL workspace/tour/key buffer");
  if (!ctx->has_instance) return fail(VRPMS_ESTATE, "vrpms_vrp_tdsp_run: no instance loaded");
  const Instance& in = ctx->inst;
  if (in.problem != VRPMS_CVRP)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_run: the time-expanded partition DP solves the CVRP only "
                              "(a TSP instance is loaded; vrpms_tsp_tdp_run solves that)");
  if (in.H != 1 && in.H != 24)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_run: the matrix must be static or have 24 hour slices "
                              "(it has " + std::to_string(in.H) + ")");
  if (n < 1 || n > kTdpMaxN || n > in.N - 1)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_run: the time-expanded partition DP needs 1 <= n <= min(20, N-1)");
  const int K = in.K;
  if (K < 1 || K > kSpMaxK || (int)in.h_start.size() != K)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_run: the time-expanded partition DP needs at most 64 "
                              "vehicles (" + std::to_string(K) + " loaded)");
  if (horizon < 0) return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_run: horizon must be >= 0");
  const int Wws = tdsp_words(in.max_start, horizon);
  if (!Wws)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_run: horizon of " + std::to_string(horizon) +
                                  " minutes needs more than " + std::to_string(kTdpMaxWords) +
                                  " hour words per state");
  // the distinct start times in order of first appearance, and each vehicle's index among them
  std::vector<int> starts;
  TdspChooseArgs ch{};
  for (int k = 0; k < K; ++k) {
    const auto it = std::find(starts.begin(), starts.end(), in.h_start[k]);
    ch.grp[k] = (uint8_t)(it - starts.begin());
    if (it == starts.end()) starts.push_back(in.h_start[k]);
  }
  const int G = (int)starts.size();
  const uint64_t need = tdsp_bytes(n, K, G, Wws);
  if (work_bytes < need)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_run: workspace of " + std::to_string(work_bytes) +
                                  " bytes is too small (" + std::to_string(need) + " needed)");
  if (reinterpret_cast<uintptr_t>(d_work) & 7u)
    return fail(VRPMS_EINVAL, "vrpms_vrp_tdsp_run: workspace must be 8-byte aligned");
  VRPMS_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t full = (size_t)1 << n;
  uint64_t* R = static_cast<uint64_t*>(d_work);
  uint32_t* routes = reinterpret_cast<uint32_t*>(R + full * n * Wws);
  uint32_t* dem = routes + (size_t)G * full;
  uint32_t* routecap = dem + full;
  uint32_t* f = routecap + full;  // f_{k+1} at f + k 2^n
  uint64_t* walk_key = reinterpret_cast<uint64_t*>(f + (size_t)K * full);  // (G + K + 2) 2^n words: 8-byte aligned
  uint32_t* chosen = reinterpret_cast<uint32_t*>(walk_key + 1);

  const unsigned mask_blocks = (unsigned)((full + 255) / 256);
  vrp_tdsp_dem_kernel<<<mask_blocks, 256, 0, s>>>(in.dem, n, dem);
  VRPMS_HIP(hipGetLastError());
  int rc;
  for (int g = 0; g < G; ++g) {
    const int W = tdp_words(starts[g], horizon);  // <= Wws, so never 0 here
    if ((rc = tsp_tdp_fill(ctx, tdp_identity(n, starts[g], horizon, W), R, s)) != VRPMS_OK) return rc;
    TdspRouteArgs a{};
    a.D = in.mat32;
    a.N = in.N;
    a.H = in.H;
    a.n = n;
    a.W = W;
    a.h0m = (starts[g] / 60) % in.H;
    a.off = starts[g] % 60;
    a.horizon = horizon;
    a.L = 64;
    while (a.L > 1 && a.L / 2 >= n * W) a.L /= 2;
    a.R = R;
    a.route = routes + (size_t)g * full;
    // memory-bound: at most eight workgroups per CU, striding over the masks
    const uint64_t waves = (full * (uint64_t)a.L + 63) / 64;
    const unsigned blocks = (unsigned)std::min<uint64_t>((waves + 3) / 4, (uint64_t)ctx->num_cus * 8);
    vrp_tdsp_route_kernel<<<blocks, 256, 0, s>>>(a);
    VRPMS_HIP(hipGetLastError());
  }

  if ((rc = vrp_sp_cap(routes + (size_t)ch.grp[0] * full, dem, in.cap, 0, (uint32_t)full, f, s)) != VRPMS_OK)
    return rc;
  if (K > 1) {
    VRPMS_HIP(hipMemsetAsync(f + full, 0xff, (size_t)(K - 1) * full * 4, s));
    SpLayerArgs a{};
    a.dem = dem;
    a.cap = in.cap;
    vrp_sp_layer_items(n, a);
    const bool shortcut = G == 1 && in.uniform_cap;  // A15's: routecap is f_1 for every vehicle
    for (int k = 1; k < K; ++k) {
      a.k = k;
      a.fk = f + (size_t)(k - 1) * full;
      a.fn = f + (size_t)k * full;
      if (shortcut) {
        a.routecap = f;
      } else {
        if ((rc = vrp_sp_cap(routes + (size_t)ch.grp[k] * full, dem, in.cap, k, (uint32_t)full, routecap,
                             s)) != VRPMS_OK)
          return rc;
        a.routecap = routecap;
      }
      if ((rc = vrp_sp_layer(a, in.objective, s)) != VRPMS_OK) return rc;
    }
  }

  ch.n = n;
  ch.K = K;
  ch.objective = in.objective == VRPMS_OBJ_MAX ? 1 : 0;
  ch.routes = routes;
  ch.dem = dem;
  ch.f = f;
  ch.cap = in.cap;
  ch.out = chosen;
  vrp_tdsp_choose_kernel<<<1, 1024, 0, s>>>(ch);
  VRPMS_HIP(hipGetLastError());
  // the one synchronisation: the routes' customer counts and durations shape
  // the launches below
  std::vector<uint32_t> host(1 + 2 * (size_t)K);
  VRPMS_HIP(hipMemcpyAsync(host.data(), chosen, host.size() * 4, hipMemcpyDeviceToHost, s));
  VRPMS_HIP(hipStreamSynchronize(s));

  int pos = 0;
  uint32_t seen = 0;
  for (int k = 0; k < K; ++k) {
    const uint32_t T = host[1 + 2 * k], dur = host[2 + 2 * k];
    // disjoint subsets of the n customers: the walks stay inside d_tour[n + K]
    if ((T >> n) || (T & seen))
      return fail(VRPMS_ESTATE, "vrpms_vrp_tdsp_run: the backtrack read an invalid route set");
    seen |= T;
    if (T) {
      TdpProblem p;
      for (int c = 0; c < n; ++c)
        if (T >> c & 1u) p.node[p.n++] = (uint8_t)(c + 1);
      p.start = in.h_start[k];
      p.horizon = (int)dur;
      p.W = dur <= (uint32_t)horizon ? tdp_words(p.start, p.horizon) : 0;
      if (!p.W) return fail(VRPMS_ESTATE, "vrpms_vrp_tdsp_run: the backtrack read an invalid route duration");
      if ((rc = tsp_tdp_fill(ctx, p, R, s)) != VRPMS_OK) return rc;
      if ((rc = tsp_tdp_walk(ctx, p, R, d_tour + pos, walk_key, s)) != VRPMS_OK) return rc;
      pos += p.n;
    }
    ++pos;  // the separator
  }
  vrp_tdsp_finish_kernel<<<1, 64, 0, s>>>(n, K, ch.objective, chosen, d_tour, d_key);
  VRPMS_HIP(hipGetLastError());
  return VRPMS_OK;
}
