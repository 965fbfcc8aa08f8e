// Exact time-dependent TSP by time-expanded subset dynamic programming
// (DESIGN.md §2 A16, §4.3g).
//
// With hour-indexed durations a later departure can arrive earlier, so the
// earliest arrival per (subset, node) is not an exact state (that is why
// tsp_dp.hip refuses H = 24).  The exact state is (visited set S, last
// customer j, clock t); durations are integer minutes and the clock of any
// tour no longer than `horizon` is bounded, so the reachable clocks of one
// (S, j) are a bitset over minutes:
//   R[{j}][j] = { start + D[hour(start)][0][j] }
//   R[S][j]   = OR over i in S \ {j} of shift(R[S \ {j}][i], i -> j)
// One 64-bit word holds one hour (bits 0..59; word w, bit m = clock
// base + 60 w + m, base = 60 (start / 60)), so every departure from a word
// uses one matrix slice and a transition is a shift by d % 60 into words
// w + d / 60 and w + d / 60 + 1.  Clocks above start + horizon are dropped
// (durations are non-negative: they cannot lead to a tour within the horizon).
//
// Table: row (S, c) -- S the customer bit mask (bit c = customer c + 1), c in
// S -- holds W words at (S n + c) W.  Rows with c not in S are never written
// nor read.  Every offset is 64-bit (13 GiB at n = 20, W = 80).
//
//   tsp_tdp_init_kernel   the n singleton rows.
//   tsp_tdp_layer_kernel  one launch per cardinality k = 2..n; the kernel
//                         boundary hands layer k-1 to layer k (no grid
//                         barrier, no flags).  A wavefront owns one subset at
//                         a time (a chunk of consecutive ranks: binomial
//                         unrank + Gosper step, tsp_dp.hpp) and, within it,
//                         one row (S, c) at a time: its lanes take the
//                         (k-1) W source words (predecessor, w) of that row
//                         in order -- consecutive lanes, consecutive words of
//                         one predecessor row; with W < 64 the spare lanes are
//                         on the next predecessors -- skip a zero word, read
//                         d from the LDS copy of the matrix, and OR the two
//                         shifted words into the wavefront's W accumulator
//                         words in LDS with ds_or_b64 (q = d / 60 varies with
//                         the hour, so two source words can meet in one
//                         destination word).  The W words then leave as one
//                         coalesced store.
//   tsp_tdp_walk_kernel   one wavefront: the closing edge (the optimum), then
//                         the walk back through the table; writes the tour and
//                         the A8 key (UINT64_MAX and a zero tour if no tour
//                         fits the horizon).
//
// tsp_tdp_fill / tsp_tdp_walk (tsp_tdp.hpp) enqueue these for an explicit
// start time and a node map (local customer bit c -> compact node), so
// vrp_tdsp.hip builds one table per vehicle start time and re-walks single
// routes over their own customers; vrpms_tsp_tdp_run passes the instance's
// start and the identity map.  The map is applied where the matrix is staged
// into LDS and in the init and walk kernels' direct reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "common.hpp"
#include "ctx.hpp"
#include "tsp_dp.hpp"
#include "tsp_tdp.hpp"

namespace vrpms {

constexpr int kTdpMaxWaves = 16;       // wavefronts per workgroup of the layer kernel: 16, 8 or 4 (tdp_lds_bytes)
constexpr size_t kTdpLdsLimit = 64 * 1024;
constexpr uint64_t kTdpMask60 = (1ull << 60) - 1;

__constant__ DpBinom kTdpBinom = dp_make_binom();

struct TdpArgs {
  const int32_t* D;    // [H][N][N] of the loaded instance
  int N, H, n, k, W;
  int h0m;             // (start / 60) % H: the slice of word 0
  int off;             // start % 60: the start's bit in word 0
  int horizon;
  uint32_t count;      // C(n, k) subsets in this layer
  uint32_t chunk;      // consecutive ranks per wavefront
  uint64_t last_mask;  // bits of word W-1 at or below start + horizon
  uint64_t* R;         // [2^n][n][W]
  uint8_t node[kTdpMaxN];  // local customer c (bit c) -> compact node
  int mapped;          // 0: node[c] = c + 1 for every c (the staging loop then needs no lookups)
};

VRPMS_DEV int tdp_slice(const TdpArgs& a, int w) { return a.H == 1 ? 0 : (a.h0m + w) % 24; }

__global__ __launch_bounds__(256) void tsp_tdp_init_kernel(TdpArgs a) {
  const int n = a.n, W = a.W;
  for (int e = threadIdx.x; e < n * W; e += 256) {
    const int c = e / W, w = e - c * W;
    const int64_t rel = (int64_t)a.off + a.D[(int64_t)a.h0m * a.N * a.N + a.node[c]];
    uint64_t v = 0;
    if (rel <= (int64_t)a.off + a.horizon && rel / 60 == w) v = 1ull << (rel % 60);
    a.R[(((uint64_t)1 << c) * n + c) * W + w] = v;
  }
}

// LDS of one layer workgroup of `waves` wavefronts: the accumulators, the
// matrix, the member lists
static size_t tdp_lds_bytes(int waves, int W, int H, int n) {
  return (size_t)waves * W * 8 + (size_t)H * (n + 1) * (n + 1) * 4 + (size_t)waves * 32;
}

__global__ __launch_bounds__(64 * kTdpMaxWaves) void tsp_tdp_layer_kernel(TdpArgs a) {
  extern __shared__ uint64_t tdp_smem[];
  const int n = a.n, k = a.k, W = a.W, NN = a.n + 1;
  const int waves = blockDim.x >> 6;
  int32_t* Dl = reinterpret_cast<int32_t*>(tdp_smem + waves * W);       // [H][n+1][n+1]
  uint8_t* members = reinterpret_cast<uint8_t*>(Dl + a.H * NN * NN);    // [waves][32]
  if (!a.mapped) {  // wave-uniform: the identity map costs the staging loop nothing
    for (int e = threadIdx.x; e < a.H * NN * NN; e += blockDim.x) {
      const int h = e / (NN * NN), r = e - h * NN * NN, i = r / NN, j = r - i * NN;
      Dl[e] = a.D[((int64_t)h * a.N + i) * a.N + j];
    }
  } else {
    for (int e = threadIdx.x; e < a.H * NN * NN; e += blockDim.x) {
      const int h = e / (NN * NN), r = e - h * NN * NN, i = r / NN, j = r - i * NN;
      const int gi = i ? a.node[i - 1] : 0, gj = j ? a.node[j - 1] : 0;
      Dl[e] = a.D[((int64_t)h * a.N + gi) * a.N + gj];
    }
  }
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(tdp_smem) + wv * W;
  uint8_t* mem = members + wv * 32;
  for (int w = lane; w < W; w += 64) acc[w] = 0;
  __syncthreads();

  const uint64_t lo = ((uint64_t)blockIdx.x * waves + wv) * a.chunk;
  if (lo >= a.count) return;  // the whole wavefront leaves together
  const uint32_t hi = lo + a.chunk < a.count ? (uint32_t)(lo + a.chunk) : a.count;

  // rank -> mask: the k-subsets in increasing mask order are the combinations
  // c_k > ... > c_1 with rank = sum C(c_t, t)
  uint32_t S = 0;
  {
    uint32_t r = (uint32_t)lo;
    int c = n - 1;
    for (int t = k; t >= 1; --t) {
      while (kTdpBinom.v[c][t] > r) --c;
      S |= 1u << c;
      r -= kTdpBinom.v[c][t];
      --c;
    }
  }

  // lane -> (predecessor index p, word w) of item `lane`, and the step of 64 items
  const int pstep = 64 / W, wstep = 64 - pstep * W;
  const int p0 = lane / W, w0 = lane - p0 * W;
  const int items = (k - 1) * W;
  uint64_t* __restrict__ R = a.R;

  for (uint32_t r = (uint32_t)lo; r < hi; ++r) {
    // mem[t] = the t-th customer of S
    if (lane < n && (S >> lane & 1u)) mem[__builtin_popcount(S & ((1u << lane) - 1u))] = (uint8_t)lane;
    wave_sync();
    for (int t = 0; t < k; ++t) {
      const int c = mem[t];
      const uint64_t src = (uint64_t)(S ^ (1u << c)) * n;
      const int32_t* col = Dl + c + 1;   // col[(slice * NN + i + 1) * NN] = D[slice][i + 1][c + 1]
      int p = p0, w = w0;
      for (int e = lane; e < items; e += 64) {
        const int i = mem[p + (p >= t)];
        const uint64_t x = R[(src + i) * W + w];
        if (x) {
          const int d = col[(tdp_slice(a, w) * NN + i + 1) * NN];
          const int q = d / 60, s = d - q * 60;
          const int dst = w + q;
          if (dst < W) {
            const uint64_t lo60 = (x << s) & kTdpMask60;
            if (lo60) atomicOr(&acc[dst], lo60);
            const uint64_t hi60 = x >> (60 - s);   // s = 0: x < 2^60, nothing carries
            if (hi60 && dst + 1 < W) atomicOr(&acc[dst + 1], hi60);
          }
        }
        p += pstep;
        w += wstep;
        if (w >= W) {
          w -= W;
          ++p;
        }
      }
      wave_sync();
      const uint64_t row = ((uint64_t)S * n + c) * W;
      for (int w2 = lane; w2 < W; w2 += 64) {
        const uint64_t v = acc[w2];
        R[row + w2] = w2 == W - 1 ? v & a.last_mask : v;
        acc[w2] = 0;
      }
      wave_sync();
    }
    S = dp_next_mask(S);
  }
}

// One wavefront.  Closing: every word of R[all][c] prices its lowest bit (one
// slice per word, so the lowest bit is the word's best); the minimum of
// (duration, c, clock) is the optimum under the tie rule.  Then n - 1 steps
// back: the smallest predecessor i, and for it the smallest clock, that
// reaches the current (customer, clock).
__global__ __launch_bounds__(64) void tsp_tdp_walk_kernel(TdpArgs a, int16_t* tour, uint64_t* key) {
  const int lane = threadIdx.x, n = a.n, W = a.W;
  const int64_t NN2 = (int64_t)a.N * a.N;
  uint32_t S = (1u << n) - 1u;
  uint64_t best = ~0ull;
  for (int e = lane; e < n * W; e += 64) {
    const int c = e / W, w = e - c * W;
    const uint64_t x = a.R[((uint64_t)S * n + c) * W + w];
    if (!x) continue;
    const int brel = 60 * w + __builtin_ctzll(x);
    const int64_t val = (int64_t)brel - a.off + a.D[tdp_slice(a, w) * NN2 + (int64_t)a.node[c] * a.N];
    if (val > a.horizon) continue;
    const uint64_t cand = ((uint64_t)val << 24) | ((uint64_t)c << 16) | (uint64_t)brel;
    best = cand < best ? cand : best;
  }
  best = wave_min_u64(best);
  if (best == ~0ull) {
    if (lane < n) tour[lane] = 0;
    if (lane == 0) *key = ~0ull;
    return;
  }
  int c = (int)(best >> 16 & 0xff), brel = (int)(best & 0xffff);
  for (int pos = n - 1; pos >= 1; --pos) {
    if (lane == 0) tour[pos] = (int16_t)a.node[c];
    S ^= 1u << c;
    const int nw = brel / 60 + 1;   // source words that can reach the clock
    uint64_t step = ~0ull;
    for (int e = lane; e < n * nw; e += 64) {
      const int i = e / nw, w = e - i * nw;
      if (!(S >> i & 1u)) continue;
      const uint64_t x = a.R[((uint64_t)S * n + i) * W + w];
      const int64_t m = (int64_t)brel - 60 * w - a.D[tdp_slice(a, w) * NN2 + (int64_t)a.node[i] * a.N + a.node[c]];
      if (m < 0 || m >= 60 || !(x >> m & 1ull)) continue;
      const uint64_t cand = ((uint64_t)i << 16) | (uint64_t)(60 * w + m);
      step = cand < step ? cand : step;
    }
    step = wave_min_u64(step);
    if (step == ~0ull) {  // unreachable for a table the layer kernels wrote
      if (lane < n) tour[lane] = 0;
      if (lane == 0) *key = ~0ull;
      return;
    }
    c = (int)(step >> 16);
    brel = (int)(step & 0xffff);
  }
  if (lane == 0) {
    tour[0] = (int16_t)a.node[c];
    *key = pack_key(0, (uint32_t)(best >> 24), 0);
  }
}

static TdpArgs tdp_args(const Instance& in, const TdpProblem& p, uint64_t* R) {
  TdpArgs a{};
  a.D = in.mat32;
  a.N = in.N;
  a.H = in.H;
  a.n = p.n;
  a.W = p.W;
  a.h0m = (p.start / 60) % in.H;
  a.off = p.start % 60;
  a.horizon = p.horizon;
  a.last_mask = (2ull << ((a.off + (int64_t)p.horizon) % 60)) - 1ull;
  a.R = R;
  for (int c = 0; c < p.n; ++c) {
    a.node[c] = p.node[c];
    a.mapped |= p.node[c] != c + 1;
  }
  return a;
}

int tsp_tdp_fill(vrpms_ctx* ctx, const TdpProblem& p, uint64_t* R, hipStream_t s) {
  const Instance& in = ctx->inst;
  const int n = p.n, W = p.W;
  TdpArgs a = tdp_args(in, p, R);
  tsp_tdp_init_kernel<<<1, 256, 0, s>>>(a);
  VRPMS_HIP(hipGetLastError());
  // the largest workgroup whose LDS stays within 64 KiB (the matrix is staged
  // once per workgroup, and two or three workgroups fit a CU); two rounds of a
  // full chip of wavefronts per layer
  int wg_waves = kTdpMaxWaves;
  while (wg_waves > 4 && tdp_lds_bytes(wg_waves, W, in.H, n) > kTdpLdsLimit) wg_waves /= 2;
  const size_t lds = tdp_lds_bytes(wg_waves, W, in.H, n);
  const uint64_t waves_target = (uint64_t)ctx->num_cus * 32 * 2;
  for (int k = 2; k <= n; ++k) {
    a.k = k;
    a.count = kDpBinomHost.v[n][k];
    a.chunk = (uint32_t)std::max<uint64_t>(1, (a.count + waves_target - 1) / waves_target);
    const uint64_t waves = ((uint64_t)a.count + a.chunk - 1) / a.chunk;
    const unsigned blocks = (unsigned)((waves + wg_waves - 1) / wg_waves);
    tsp_tdp_layer_kernel<<<blocks, 64 * wg_waves, lds, s>>>(a);
    VRPMS_HIP(hipGetLastError());
  }
  return VRPMS_OK;
}

int tsp_tdp_walk(vrpms_ctx* ctx, const TdpProblem& p, uint64_t* R, int16_t* tour, uint64_t* key,
                 hipStream_t s) {
  TdpArgs a = tdp_args(ctx->inst, p, R);
  a.k = p.n;
  tsp_tdp_walk_kernel<<<1, 64, 0, s>>>(a, tour, key);
  VRPMS_HIP(hipGetLastError());
  return VRPMS_OK;
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_tsp_tdp_workspace(int32_t n, int32_t start_time, int32_t horizon,
                                       uint64_t* bytes) {
  if (!bytes) return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_workspace: bytes is NULL");
  if (n < 1 || n > kTdpMaxN)
    return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_workspace: the time-expanded DP needs 1 <= n <= 20");
  if (start_time < 0 || horizon < 0)
    return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_workspace: start time and horizon must be >= 0");
  const int W = tdp_words(start_time, horizon);
  if (!W)
    return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_workspace: horizon of " + std::to_string(horizon) +
                                  " minutes needs more than " + std::to_string(kTdpMaxWords) +
                                  " hour words per state");
  *bytes = ((uint64_t)1 << n) * (uint64_t)n * (uint64_t)W * 8u;
  return VRPMS_OK;
}

extern "C" int vrpms_tsp_tdp_run(vrpms_ctx* ctx, int32_t n, int32_t horizon, void* d_work,
                                 uint64_t work_bytes, int16_t* d_tour, uint64_t* d_key,
                                 void* stream) {
  if (!ctx) return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_run: ctx is NULL");
  if (!d_work || !d_tour || !d_key)
    return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_run: NULL workspace/tour/key buffer");
  if (!ctx->has_instance) return fail(VRPMS_ESTATE, "vrpms_tsp_tdp_run: no instance loaded");
  const Instance& in = ctx->inst;
  if (in.problem != VRPMS_TSP)
    return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_run: the time-expanded DP solves the TSP only (a CVRP "
                              "instance is loaded)");
  if (in.H != 1 && in.H != 24)
    return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_run: the matrix must be static or have 24 hour slices "
                              "(it has " + std::to_string(in.H) + ")");
  if (n < 1 || n > kTdpMaxN || n > in.N - 1)
    return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_run: the time-expanded DP needs 1 <= n <= min(20, N-1)");
  if (horizon < 0) return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_run: horizon must be >= 0");
  const int start = in.min_start;
  const int W = tdp_words(start, horizon);
  if (!W)
    return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_run: horizon of " + std::to_string(horizon) +
                                  " minutes needs more than " + std::to_string(kTdpMaxWords) +
                                  " hour words per state");
  const uint64_t need = ((uint64_t)1 << n) * (uint64_t)n * (uint64_t)W * 8u;
  if (work_bytes < need)
    return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_run: workspace of " + std::to_string(work_bytes) +
                                  " bytes is too small (" + std::to_string(need) + " needed)");
  if (reinterpret_cast<uintptr_t>(d_work) & 7u)
    return fail(VRPMS_EINVAL, "vrpms_tsp_tdp_run: workspace must be 8-byte aligned");
  VRPMS_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;

  const TdpProblem p = tdp_identity(n, start, horizon, W);
  const int rc = tsp_tdp_fill(ctx, p, static_cast<uint64_t*>(d_work), s);
  if (rc != VRPMS_OK) return rc;
  return tsp_tdp_walk(ctx, p, static_cast<uint64_t*>(d_work), d_tour, d_key, s);
}
