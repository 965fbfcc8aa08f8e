// Exact TSP by Held-Karp subset dynamic programming.
//
// Backward cost-to-go over subsets S of the customers 1..n and a customer
// j not in S (node 0 is the start node, static matrix D):
//   g[0][j] = D[j][0]
//   g[S][j] = min over i in S of D[j][i] + g[S \ {i}][i]
// The optimum is min over i of D[0][i] + g[all \ {i}][i]; the tour returned
// is the lexicographically smallest optimal one (bf's tie rule): walking
// forward from node 0, the smallest i in S that attains g[S][cur].
//
// Table: row S (the customer bit mask, bit c-1 = customer c) holds NPAD uint32
// words, word c-1 = g[S][c]; NPAD = 16 for n <= 16, else 32, so a row is one
// 64- or 128-byte line.  Words of customers inside S (and past n) are never
// read; they are stored as 0xffffffff so that every row leaves as one whole
// coalesced store.  At n = 24 the table is 2 GiB: every offset is 64-bit.
//
//   tsp_dp_init_kernel    row 0 (the empty set).
//   tsp_dp_layer_kernel   one launch per cardinality k = 1..n-1; the kernel
//                         boundary hands layer k-1 to layer k (no grid
//                         barrier, no flags).  A group of NPAD lanes owns one
//                         subset at a time: lane c-1 in S loads the one word
//                         h[c] = g[S \ {c}][c] (it does not depend on j), the
//                         k-step min-plus loop broadcasts h over the group by
//                         a lane shuffle and reads D transposed from LDS
//                         (consecutive lanes, consecutive words).  The
//                         k-subsets are enumerated by rank: a group unranks
//                         the first mask of its chunk from a binomial table
//                         (combinatorial number system; masks of one
//                         popcount in increasing order) and steps with
//                         Gosper's next-same-popcount mask.
//   tsp_dp_walk_kernel    one wavefront: the last layer (g[all][0]) and the
//                         forward walk; writes the tour and the A8 key.
// tsp_dp_fill (the init and layer launches) is shared with vrp_sp.hip, whose
// route costs are this table's rows (tsp_dp.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "common.hpp"
#include "ctx.hpp"
#include "tsp_dp.hpp"

namespace vrpms {

constexpr int kDpLd = 33;        // LDS row stride of the transposed matrix (words)
constexpr int kDpMinChunk = 16;  // subsets per lane group at least: amortises the unrank

__constant__ DpBinom kDpBinom = dp_make_binom();

struct DpArgs {
  const int32_t* D;  // [N][N] static matrix of the loaded instance
  int N, n, k;
  uint32_t count;    // C(n, k) subsets in this layer
  uint32_t chunk;    // consecutive ranks per lane group
  uint32_t* g;       // [2^n][NPAD]
};

__global__ void tsp_dp_init_kernel(DpArgs a, int npad) {
  const int l = threadIdx.x;
  if (l < npad) a.g[l] = l < a.n ? (uint32_t)a.D[(int64_t)(l + 1) * a.N] : 0xffffffffu;
}

template <int NPAD>
__global__ __launch_bounds__(256) void tsp_dp_layer_kernel(DpArgs a) {
  __shared__ uint32_t Dt[kDpNodes * kDpLd];       // Dt[i][j] = D[j][i]
  __shared__ uint32_t B[kDpNodes * kDpNodes];
  for (int e = threadIdx.x; e < kDpNodes * kDpLd; e += 256) {
    const int i = e / kDpLd, j = e - i * kDpLd;
    Dt[e] = (i <= a.n && j <= a.n) ? (uint32_t)a.D[(int64_t)j * a.N + i] : 0u;
  }
  for (int e = threadIdx.x; e < kDpNodes * kDpNodes; e += 256)
    B[e] = kDpBinom.v[e / kDpNodes][e % kDpNodes];
  __syncthreads();

  const int n = a.n, k = a.k;
  const int l = threadIdx.x & (NPAD - 1);  // lane l owns customer l + 1
  const uint64_t grp = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / NPAD;
  const uint64_t lo = grp * a.chunk;
  if (lo >= a.count) return;  // the whole lane group leaves together
  const uint32_t hi = lo + a.chunk < a.count ? (uint32_t)(lo + a.chunk) : a.count;

  uint32_t S = dp_unrank(B, kDpNodes, n, k, (uint32_t)lo);

  const bool mine = l < n;
  const uint32_t bit = 1u << l;
  uint32_t* __restrict__ g = a.g;
  // h[l] = g[S \ {l}][l], only for members of S (any other row index could lie
  // outside the table)
  auto load_h = [&](uint32_t s) -> uint32_t {
    return (mine && (s & bit)) ? g[(size_t)(s ^ bit) * NPAD + l] : 0u;
  };
  const uint32_t* col = Dt + (l + 1);
  uint32_t h = load_h(S);
  for (uint32_t r = (uint32_t)lo; r < hi; ++r) {
    // the next subset's loads are in flight during this subset's loop
    const uint32_t Sn = dp_next_mask(S);
    const uint32_t hn = r + 1 < hi ? load_h(Sn) : 0u;
    uint32_t best = 0xffffffffu;
    uint32_t m = S;
    for (int t = 0; t < k; ++t) {
      const int i = __builtin_ctz(m);
      m &= m - 1u;
      const uint32_t hv = (uint32_t)__shfl((int)h, i, NPAD);
      best = min(best, col[(i + 1) * kDpLd] + hv);
    }
    g[(size_t)S * NPAD + l] = (mine && !(S & bit)) ? best : 0xffffffffu;
    S = Sn;
    h = hn;
  }
}

// One wavefront.  Step s: lanes i in S price D[cur][i] + g[S \ {i}][i]; the
// minimum is g[S][cur] (the optimum at s = 0) and the lowest lane attaining
// it is the next customer.
__global__ __launch_bounds__(64) void tsp_dp_walk_kernel(DpArgs a, int npad, int16_t* tour,
                                                         uint64_t* key) {
  const int l = threadIdx.x, n = a.n;
  const bool mine = l < n;
  const uint32_t bit = mine ? 1u << l : 0u;
  uint32_t S = (1u << n) - 1u;
  int cur = 0;
  uint32_t total = 0;
  for (int s = 0; s < n; ++s) {
    uint32_t val = 0xffffffffu;
    if (S & bit)
      val = (uint32_t)a.D[(int64_t)cur * a.N + l + 1] + a.g[(size_t)(S ^ bit) * npad + l];
    const uint32_t mn = wave_min_u32_uniform(val);
    const int i = (int)__builtin_ctzll(__builtin_amdgcn_ballot_w64(val == mn));
    if (s == 0) total = mn;
    if (l == 0) tour[s] = (int16_t)(i + 1);
    cur = i + 1;
    S &= ~(1u << i);
  }
  if (l == 0) *key = pack_key(0, total, 0);
}

int tsp_dp_fill(vrpms_ctx* ctx, int n, uint32_t* g, hipStream_t s) {
  const Instance& in = ctx->inst;
  const int npad = dp_npad(n);
  DpArgs a{in.mat32, in.N, n, 0, 1, 1, g};
  tsp_dp_init_kernel<<<1, 64, 0, s>>>(a, npad);
  VRPMS_HIP(hipGetLastError());
  // two rounds of a full chip of lane groups per layer, each group at least
  // kDpMinChunk consecutive subsets
  const uint64_t groups_per_block = 256 / npad;
  const uint64_t groups_target = (uint64_t)ctx->num_cus * 8 * groups_per_block * 2;
  for (int k = 1; k < n; ++k) {
    a.k = k;
    a.count = kDpBinomHost.v[n][k];
    a.chunk = (uint32_t)std::max<uint64_t>(kDpMinChunk, (a.count + groups_target - 1) / groups_target);
    const uint64_t groups = ((uint64_t)a.count + a.chunk - 1) / a.chunk;
    const unsigned blocks = (unsigned)((groups + groups_per_block - 1) / groups_per_block);
    if (npad == 16)
      tsp_dp_layer_kernel<16><<<blocks, 256, 0, s>>>(a);
    else
      tsp_dp_layer_kernel<32><<<blocks, 256, 0, s>>>(a);
    VRPMS_HIP(hipGetLastError());
  }
  return VRPMS_OK;
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_tsp_dp_workspace(int32_t n, uint64_t* bytes) {
  if (!bytes) return fail(VRPMS_EINVAL, "vrpms_tsp_dp_workspace: bytes is NULL");
  if (n < 1 || n > kDpMaxN)
    return fail(VRPMS_EINVAL, "vrpms_tsp_dp_workspace: Held-Karp needs 1 <= n <= 24");
  *bytes = ((uint64_t)1 << n) * (uint64_t)dp_npad(n) * 4u;
  return VRPMS_OK;
}

extern "C" int vrpms_tsp_dp_run(vrpms_ctx* ctx, int32_t n, void* d_work, uint64_t work_bytes,
                                int16_t* d_tour, uint64_t* d_key, void* stream) {
  if (!ctx) return fail(VRPMS_EINVAL, "vrpms_tsp_dp_run: ctx is NULL");
  if (!d_work || !d_tour || !d_key)
    return fail(VRPMS_EINVAL, "vrpms_tsp_dp_run: NULL workspace/tour/key buffer");
  if (!ctx->has_instance) return fail(VRPMS_ESTATE, "vrpms_tsp_dp_run: no instance loaded");
  const Instance& in = ctx->inst;
  if (in.problem != VRPMS_TSP)
    return fail(VRPMS_EINVAL, "vrpms_tsp_dp_run: Held-Karp solves the TSP only (a CVRP instance "
                              "is loaded)");
  if (in.H != 1)
    return fail(VRPMS_EINVAL, "vrpms_tsp_dp_run: Held-Karp needs a static matrix (H = 1); the "
                              "loaded one has " + std::to_string(in.H) + " hour slices");
  if (n < 1 || n > kDpMaxN || n > in.N - 1)
    return fail(VRPMS_EINVAL, "vrpms_tsp_dp_run: Held-Karp needs 1 <= n <= min(24, N-1)");
  const int npad = dp_npad(n);
  const uint64_t need = ((uint64_t)1 << n) * (uint64_t)npad * 4u;
  if (work_bytes < need)
    return fail(VRPMS_EINVAL, "vrpms_tsp_dp_run: workspace of " + std::to_string(work_bytes) +
                                  " bytes is too small (" + std::to_string(need) + " needed)");
  if (reinterpret_cast<uintptr_t>(d_work) & 3u)
    return fail(VRPMS_EINVAL, "vrpms_tsp_dp_run: workspace must be 4-byte aligned");
  VRPMS_HIP(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const int rc = tsp_dp_fill(ctx, n, static_cast<uint32_t*>(d_work), s);
  if (rc != VRPMS_OK) return rc;
  const DpArgs a{in.mat32, in.N, n, n, 0, 1, static_cast<uint32_t*>(d_work)};
  tsp_dp_walk_kernel<<<1, 64, 0, s>>>(a, npad, d_tour, d_key);
  VRPMS_HIP(hipGetLastError());
  return VRPMS_OK;
}
