// Exact small-fleet CVRP by subset partition dynamic programming (DESIGN.md
// §2 A15, §4.3f).
//
// Over subsets of the customers 1..n (bit c-1 = customer c), with g the
// Held-Karp table of tsp_dp.hip on the instance's static matrix D:
//   route[T] = min over i in T of D[0][i] + g[T \ {i}][i]      (route[0] = 0)
//   dem[T]   = the demand of T
//   f_0      = the one state {} at 0
//   f_{k+1}[S] = min over T subset of S, dem[T] <= cap[k], f_k[S \ T] reachable
//                of route[T] (+) f_k[S \ T]
// (+) is + for the sum objective and max for the max objective; vehicle k
// serves T.  An unreachable state is 0xffffffff and is never added to: the
// sum saturates there (every reachable value is below 2^31 by A9).
//
// Workspace, all uint32 words: g [2^n][NPAD] | route [2^n] | dem [2^n] |
// routecap [2^n] | f_1 .. f_K [K][2^n].  f_0 is not stored: its one state
// makes f_1[S] = routecap_0[S].
//
//   vrp_sp_route_kernel  route[] and dem[] for every mask: a group of NPAD
//                        lanes per mask, the walk kernel's first step.
//   vrp_sp_cap_kernel    routecap[T] = dem[T] <= cap[k] ? route[T] : unreachable
//                        (straight into f_1 for k = 0; a fleet of equal
//                        capacities reuses f_1 as routecap for every layer).
//   vrp_sp_layer_kernel  f_{k+1} from f_k, one launch per vehicle k >= 1; the
//                        kernel boundary is the hand-off.  A wavefront's 64
//                        lanes share one S: each lane deposits the top rank
//                        of its contiguous run of submask ranks into the
//                        bits of S once, steps down with T = (T - 1) & S and
//                        gathers routecap[T] and f_k[S ^ T]; a wave minimum
//                        ends S.  The work per S is 2^|S|, so work items are
//                        sized, not sets: an S of more than kSpItemLog
//                        customers is cut into 2^(|S| - kSpItemLog) items
//                        (combined by atomicMin into the preset unreachable
//                        word), smaller ones are batched per wavefront
//                        (unrank the first, Gosper to the next).  Items are
//                        ordered heaviest first.
//   vrp_sp_back_kernel   one workgroup: S* by a packed-tuple reduction over
//                        f_K, per vehicle the smallest submask attaining
//                        f_{k+1}[S] (1024 ranks at a time, in increasing
//                        order), then one wavefront walks every route as
//                        tsp_dp_walk_kernel does and writes tour and key.
//
// vrp_sp_cap / vrp_sp_layer_items / vrp_sp_layer (vrp_sp.hpp) enqueue the
// capacity filter and one partition layer; vrp_tdsp.hip runs the same two
// kernels on route tables that come from the time-expanded DP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "common.hpp"
#include "ctx.hpp"
#include "tsp_dp.hpp"
#include "vrp_sp.hpp"

namespace vrpms {

constexpr int kSpItemLog = 14;  // submasks per work item: 2^14 = 256 steps per lane
constexpr int kSpMaxSets = 64;  // small sets per work item at most
constexpr int kSpBatch = 8;     // steps whose gathers a lane keeps in flight together

__constant__ DpBinom kSpBinom = dp_make_binom();

template <int NPAD>
__global__ __launch_bounds__(256) void vrp_sp_route_kernel(const int32_t* D, int n, const int32_t* demand,
                                                           const uint32_t* __restrict__ g,
                                                           uint32_t* route, uint32_t* dem) {
  const int l = threadIdx.x & (NPAD - 1);  // lane l prices customer l + 1 first
  const uint64_t grp = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / NPAD;
  if (grp >> n) return;  // the whole lane group leaves together
  const uint32_t S = (uint32_t)grp;
  const bool in = l < n && ((S >> l) & 1u);
  uint32_t val = kSpInf;
  uint64_t dm = 0;
  if (in) {
    val = (uint32_t)D[l + 1] + g[(size_t)(S ^ (1u << l)) * NPAD + l];
    dm = (uint32_t)demand[l + 1];
  }
#pragma unroll
  for (int off = NPAD / 2; off > 0; off >>= 1) {
    val = min(val, (uint32_t)__shfl_xor((int)val, off, NPAD));
    dm += __shfl_xor(dm, off, NPAD);
  }
  if (l == 0) {
    route[S] = S ? val : 0u;
    dem[S] = dm < kSpInf ? (uint32_t)dm : kSpInf;
  }
}

__global__ __launch_bounds__(256) void vrp_sp_cap_kernel(const uint32_t* __restrict__ route,
                                                         const uint32_t* __restrict__ dem,
                                                         const int32_t* cap, int k, uint32_t count,
                                                         uint32_t* out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < count) out[i] = dem[i] <= (uint32_t)cap[k] ? route[i] : kSpInf;
}

template <int OBJ>
__global__ __launch_bounds__(256) void vrp_sp_layer_kernel(SpLayerArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = a.n;
  const uint32_t w = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= a.first[n + 1]) return;  // whole wavefronts leave
  int j = 0;
  while (w >= a.first[j + 1]) ++j;
  const int c = n - j;
  const uint32_t item = w - a.first[j];
  const uint32_t sets = kSpBinom.v[n][c];

  // vehicles 0..k carry at most this much: a heavier S stays unreachable
  uint64_t room = 0;
  for (int t = 0; t <= a.k; ++t) room += (uint32_t)a.cap[t];

  // this item: `count` consecutive sets from rank `srank`, of each the
  // submask ranks [base, base + 64 per)
  uint32_t srank, count, base = 0;
  const bool split = c > kSpItemLog;
  if (split) {
    srank = item >> (c - kSpItemLog);
    count = 1;
    base = (item & ((1u << (c - kSpItemLog)) - 1u)) << kSpItemLog;
  } else {
    const uint32_t per_item = min(1u << (kSpItemLog - c), (uint32_t)kSpMaxSets);
    srank = item * per_item;
    count = min(per_item, sets - srank);
  }
  const uint32_t per = c > 6 ? 1u << (min(c, kSpItemLog) - 6) : 1u;  // steps per lane
  const bool active = c >= 6 || lane < (1 << c);
  const uint32_t top = base + (uint32_t)(lane + 1) * per - 1u;       // the run's highest rank

  // rank -> mask, as tsp_dp_layer_kernel: combinations c_t > ... > c_1 with
  // rank = sum C(c_t, t)
  uint32_t S = 0;
  {
    uint32_t r = srank;
    int b = n - 1;
    for (int t = c; t >= 1; --t) {
      while (kSpBinom.v[b][t] > r) --b;
      S |= 1u << b;
      r -= kSpBinom.v[b][t];
      --b;
    }
  }

  const uint32_t* __restrict__ rcap = a.routecap;
  const uint32_t* __restrict__ fk = a.fk;
  for (uint32_t s = 0; s < count; ++s) {
    if (s) S = dp_next_mask(S);
    __builtin_assume(S < (1u << kSpMaxN));  // 32-bit byte offsets into the 2^n-word tables
    uint32_t best = kSpInf;
    if (a.dem[S] <= room) {  // wave-uniform
      if (active) {
        uint32_t T = sp_deposit(top, S);
        auto join = [](uint32_t rc, uint32_t fv) -> uint32_t {
          return OBJ ? max(rc, fv) : __builtin_elementwise_add_sat(rc, fv);
        };
        if (per >= kSpBatch) {
          // kSpBatch steps' masks first (two VALU each), then their 2 kSpBatch
          // gathers in flight together
          for (uint32_t i = 0; i < per; i += kSpBatch) {
            uint32_t t[kSpBatch], rc[kSpBatch], fv[kSpBatch];
#pragma unroll
            for (int u = 0; u < kSpBatch; ++u) {
              t[u] = T;
              T = (T - 1u) & S;
            }
#pragma unroll
            for (int u = 0; u < kSpBatch; ++u) {
              rc[u] = rcap[t[u]];
              fv[u] = fk[S ^ t[u]];
            }
#pragma unroll
            for (int u = 0; u < kSpBatch; ++u) best = min(best, join(rc[u], fv[u]));
          }
        } else {
          for (uint32_t i = 0; i < per; ++i) {
            best = min(best, join(rcap[T], fk[S ^ T]));
            T = (T - 1u) & S;
          }
        }
      }
      best = wave_min_u32_uniform(best);
    }
    if (lane == 0) {
      if (!split)
        a.fn[S] = best;
      else if (best != kSpInf)
        atomicMin(&a.fn[S], best);
    }
  }
}

struct SpBackArgs {
  const int32_t* D;  // [N][N]
  int N, n, K, objective, npad;
  const uint32_t* g;      // [2^n][npad]
  const uint32_t* route;  // [2^n]
  const uint32_t* dem;    // [2^n]
  const uint32_t* f;      // f_1 .. f_K, [K][2^n]
  const int32_t* cap;     // [K]
  int16_t* tour;          // [n + K]
  uint64_t* key;
};

__global__ __launch_bounds__(1024) void vrp_sp_back_kernel(SpBackArgs a) {
  __shared__ uint64_t red[16];
  __shared__ uint32_t found;
  __shared__ uint32_t Tk[kSpMaxK];
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

  // T_k for k = K-1 .. 0: the smallest submask of the remaining S that
  // attains f_{k+1}[S], found 1024 submask ranks at a time in increasing order
  uint32_t S = served;
  for (int k = K - 1; k >= 0; --k) {
    const uint32_t want = a.f[((size_t)k << n) + S];
    const uint32_t capk = (uint32_t)a.cap[k];
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
          if (fv != kSpInf) {
            const uint32_t rt = a.route[t];
            if ((a.objective ? max(rt, fv) : rt + fv) == want) atomicMin(&found, t);
          }
        }
      }
      __syncthreads();
      T = found;
      __syncthreads();
    }
    if (T == kSpInf) T = 0;  // cannot happen: want was built from one such T
    if (tid == 0) Tk[k] = T;
    S ^= T;
  }
  __syncthreads();
  if (wv != 0) return;

  // one wavefront: the lexicographically smallest optimal route on each T_k
  // (lanes i in R price D[cur][i] + g[R \ {i}][i]; the lowest lane at the
  // minimum is next), a separator after each, then the unserved customers
  const bool mine = lane < n;
  const uint32_t bit = mine ? 1u << lane : 0u;
  int pos = 0;
  uint32_t dsum = 0, dmax = 0;
  for (int k = 0; k < K; ++k) {
    uint32_t R = Tk[k];
    const uint32_t rt = a.route[R];
    dsum += rt;
    dmax = max(dmax, rt);
    int cur = 0;
    while (R) {
      uint32_t val = kSpInf;
      if (R & bit)
        val = (uint32_t)a.D[(int64_t)cur * a.N + lane + 1] + a.g[(size_t)(R ^ bit) * a.npad + lane];
      const uint32_t mn = wave_min_u32_uniform(val);
      const int i = (int)__builtin_ctzll(__builtin_amdgcn_ballot_w64(val == mn));
      if (lane == 0) a.tour[pos] = (int16_t)(i + 1);
      ++pos;
      cur = i + 1;
      R &= ~(1u << i);
    }
    if (lane == 0) a.tour[pos] = 0;
    ++pos;
  }
  for (int c = 0; c < n; ++c)
    if (!((served >> c) & 1u)) {
      if (lane == 0) a.tour[pos] = (int16_t)(c + 1);
      ++pos;
    }
  if (lane == 0) *a.key = cvrp_key((uint32_t)(n - __popc(served)), dsum, dmax, a.objective);
}

int vrp_sp_cap(const uint32_t* route, const uint32_t* dem, const int32_t* cap, int k, uint32_t count,
               uint32_t* out, hipStream_t s) {
  vrp_sp_cap_kernel<<<(count + 255u) / 256u, 256, 0, s>>>(route, dem, cap, k, count, out);
  VRPMS_HIP(hipGetLastError());
  return VRPMS_OK;
}

void vrp_sp_layer_items(int n, SpLayerArgs& a) {
  a.n = n;
  uint32_t items = 0;
  for (int j = 0; j <= n; ++j) {
    const int c = n - j;
    const uint32_t sets = kDpBinomHost.v[n][c];
    a.first[j] = items;
    if (c > kSpItemLog) {
      items += sets << (c - kSpItemLog);
    } else {
      const uint32_t per_item = std::min<uint32_t>(1u << (kSpItemLog - c), kSpMaxSets);
      items += (sets + per_item - 1) / per_item;
    }
  }
  a.first[n + 1] = items;
}

int vrp_sp_layer(const SpLayerArgs& a, int objective, hipStream_t s) {
  const unsigned blocks = (a.first[a.n + 1] + 3) / 4;
  if (objective == VRPMS_OBJ_MAX)
    vrp_sp_layer_kernel<1><<<blocks, 256, 0, s>>>(a);
  else
    vrp_sp_layer_kernel<0><<<blocks, 256, 0, s>>>(a);
  VRPMS_HIP(hipGetLastError());
  return VRPMS_OK;
}

static uint64_t sp_words(int n, int K) { return (uint64_t)dp_npad(n) + 3u + (uint64_t)K; }

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_vrp_sp_workspace(int32_t n, int32_t K, uint64_t* bytes) {
  if (!bytes) return fail(VRPMS_EINVAL, "vrpms_vrp_sp_workspace: bytes is NULL");
  if (n < 1 || n > kSpMaxN)
    return fail(VRPMS_EINVAL, "vrpms_vrp_sp_workspace: set partitioning needs 1 <= n <= 20");
  if (K < 1 || K > kSpMaxK)
    return fail(VRPMS_EINVAL, "vrpms_vrp_sp_workspace: set partitioning needs 1 <= K <= 64");
  *bytes = ((uint64_t)4 << n) * sp_words(n, K);
  return VRPMS_OK;
}

extern "C" int vrpms_vrp_sp_run(vrpms_ctx* ctx, int32_t n, void* d_work, uint64_t work_bytes,
                                int16_t* d_tour, uint64_t* d_key, void* stream) {
  if (!ctx) return fail(VRPMS_EINVAL, "vrpms_vrp_sp_run: ctx is NULL");
  if (!d_work || !d_tour || !d_key)
    return fail(VRPMS_EINVAL, "vrpms_vrp_sp_run: NULL workspace/tour/key buffer");
  if (!ctx->has_instance) return fail(VRPMS_ESTATE, "vrpms_vrp_sp_run: no instance loaded");
  const Instance& in = ctx->inst;
  if (in.problem != VRPMS_CVRP)
    return fail(VRPMS_EINVAL, "vrpms_vrp_sp_run: set partitioning solves the CVRP only (a TSP "
                              "instance is loaded; vrpms_tsp_dp_run solves that)");
  if (in.H != 1)
    return fail(VRPMS_EINVAL, "vrpms_vrp_sp_run: set partitioning needs a static matrix (H = 1); "
                              "the loaded one has " + std::to_string(in.H) + " hour slices");
  if (n < 1 || n > kSpMaxN || n > in.N - 1)
    return fail(VRPMS_EINVAL, "vrpms_vrp_sp_run: set partitioning needs 1 <= n <= min(20, N-1)");
  const int K = in.K;
  if (K < 1 || K > kSpMaxK)
    return fail(VRPMS_EINVAL, "vrpms_vrp_sp_run: set partitioning needs at most 64 vehicles (" +
                                  std::to_string(K) + " loaded)");
  const uint64_t need = ((uint64_t)4 << n) * sp_words(n, K);
  if (work_bytes < need)
    return fail(VRPMS_EINVAL, "vrpms_vrp_sp_run: workspace of " + std::to_string(work_bytes) +
                                  " bytes is too small (" + std::to_string(need) + " needed)");
  if (reinterpret_cast<uintptr_t>(d_work) & 3u)
    return fail(VRPMS_EINVAL, "vrpms_vrp_sp_run: workspace must be 4-byte aligned");
  VRPMS_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const int npad = dp_npad(n);
  const size_t full = (size_t)1 << n;
  uint32_t* g = static_cast<uint32_t*>(d_work);
  uint32_t* route = g + full * npad;
  uint32_t* dem = route + full;
  uint32_t* routecap = dem + full;
  uint32_t* f = routecap + full;  // f_{k+1} at f + k 2^n

  const int rc = tsp_dp_fill(ctx, n, g, s);
  if (rc != VRPMS_OK) return rc;
  {
    const unsigned blocks = (unsigned)((full * npad + 255) / 256);
    if (npad == 16)
      vrp_sp_route_kernel<16><<<blocks, 256, 0, s>>>(in.mat32, n, in.dem, g, route, dem);
    else
      vrp_sp_route_kernel<32><<<blocks, 256, 0, s>>>(in.mat32, n, in.dem, g, route, dem);
    VRPMS_HIP(hipGetLastError());
  }
  int rc2 = vrp_sp_cap(route, dem, in.cap, 0, (uint32_t)full, f, s);
  if (rc2 != VRPMS_OK) return rc2;
  if (K > 1) {
    VRPMS_HIP(hipMemsetAsync(f + full, 0xff, (size_t)(K - 1) * full * 4, s));
    SpLayerArgs a{};
    a.dem = dem;
    a.cap = in.cap;
    vrp_sp_layer_items(n, a);
    for (int k = 1; k < K; ++k) {
      a.k = k;
      a.fk = f + (size_t)(k - 1) * full;
      a.fn = f + (size_t)k * full;
      if (in.uniform_cap) {
        a.routecap = f;  // equal capacities: routecap is f_1 for every vehicle
      } else {
        rc2 = vrp_sp_cap(route, dem, in.cap, k, (uint32_t)full, routecap, s);
        if (rc2 != VRPMS_OK) return rc2;
        a.routecap = routecap;
      }
      rc2 = vrp_sp_layer(a, in.objective, s);
      if (rc2 != VRPMS_OK) return rc2;
    }
  }
  const SpBackArgs b{in.mat32, in.N, n, K, in.objective == VRPMS_OBJ_MAX ? 1 : 0, npad, g, route, dem, f,
                     in.cap, d_tour, d_key};
  vrp_sp_back_kernel<<<1, 1024, 0, s>>>(b);
  VRPMS_HIP(hipGetLastError());
  return VRPMS_OK;
}
