// Batched exact TSP: Held-Karp for many small requests, each request's table
// in LDS.
//
// The recurrence, the tie rule and the result are tsp_dp.hip's (A14), per
// request: g[0][j] = D[j][0], g[S][j] = min over i in S of D[j][i] +
// g[S \ {i}][i], and the forward walk from node 0 that takes the smallest
// customer attaining the cost-to-go.  What differs is where the table lives
// and who fills it:
//
//   - A request has at most kBatchDpMaxN customers, so its whole table fits
//     one CU's LDS next to its matrix; nothing but the matrix is read from
//     memory and nothing but the tour and the key is written to it.
//   - The table is compact: g[S][j] exists only for j outside S, so customer
//     j's states are indexed by c = S with bit j squeezed out, 2^(n-1) words
//     per customer, n 2^(n-1) words in all.  The order is [j][c] (customer
//     major): a layer's reads are g[S \ {i}][i] for one i at a time over many
//     S, which are then the words base_i + c, consecutive subsets on
//     different banks (§4.3i).
//   - A team of T threads owns one request; a 256-thread workgroup holds
//     256 / T requests of the same N, so all of its teams run the same number
//     of layers and the workgroup-wide barrier between layers stays uniform.
//     A team past the end of the batch still reaches every barrier; it reads
//     and writes nothing (its layers are empty).
//   - A thread takes a run of consecutive ranks of the layer's k-subsets:
//     dp_unrank for the first mask, dp_next_mask from there (tsp_dp.hpp).
//     For its subset S it loads h[i] = g[S \ {i}][i] once (0x80000000 for i
//     outside S: above every real cost, and D + h cannot wrap since D < 2^31),
//     then for every j outside S reads row j of the matrix from LDS and
//     stores min over i of D[j][i] + h[i].
//   - The walk runs in-kernel after the last layer, on the first 16 lanes of
//     the team: lane i prices D[cur][i] + g[S \ {i}][i], a 16-lane shuffle
//     minimum over (value, lane) picks the smallest customer attaining it.
#include <hip/hip_runtime.h>

#include <string>

#include "batch_launch.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "tsp_batch_dp.hpp"
#include "tsp_dp.hpp"

namespace vrpms {

// threads per request by n (index n): the fastest T of tools/batch_dp_rate.py
// --teams 16,32,64,128,256 at each n (DESIGN.md §4.3i has the measurements)
constexpr int kBatchDpTeam[kBatchDpMaxN + 1] = {16, 16, 16, 16, 16, 16, 16, 32, 32, 128, 256, 256,
                                                256};

__constant__ DpBinom kBatchDpBinom = dp_make_binom();

struct BatchDpArgs {
  const int32_t* mats;  // [R][N][N]
  int R, N;
  uint16_t* tours;      // [R][N-1]
  uint64_t* keys;       // [R]
};

// words of one team: the matrix image, then the table padded to 16 bytes
inline size_t batch_dp_team_words(int n) { return kBatchDpMatWords + batch_dp_table_words(n); }

inline size_t batch_dp_lds_bytes(int n, int T) {
  return (kBatchDpBinomWords + (size_t)(256 / T) * batch_dp_team_words(n)) * 4;
}

template <int T>
__global__ __launch_bounds__(256) void tsp_batch_dp_kernel(BatchDpArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t batch_dp_lds[];
  const int N = a.N, n = N - 1;
  const uint32_t half = 1u << (n - 1), full = (1u << n) - 1u;
  const int team = threadIdx.x / T, tl = threadIdx.x % T;
  const int64_t req = (int64_t)blockIdx.x * (256 / T) + team;
  const bool active = req < a.R;
  const uint32_t team_words = kBatchDpMatWords + ((((uint32_t)n << (n - 1)) + 3u) & ~3u);

  uint32_t* B = batch_dp_lds;                                     // B[c][t] = C(c, t)
  uint32_t* Dr = batch_dp_lds + kBatchDpBinomWords + team * team_words;  // Dr[node][i] = D[node][i + 1]
  uint32_t* g = Dr + kBatchDpMatWords;                            // g[j][c], customer j + 1

  batch_dp_stage_binom(kBatchDpBinom, B);
  if (active) batch_dp_stage<T>(a.mats + req * N * N, N, tl, Dr, g);
  __syncthreads();

  batch_dp_fill<T>(B, Dr, g, n, tl, active);

  // the forward walk, on one 16-lane group (T is a multiple of 16, so the
  // group lies inside one wavefront and is active as a whole)
  if (active && tl < 16) {
    const int l = tl;
    uint32_t S = full, total = 0;
    int cur = 0;
    for (int s = 0; s < n; ++s) {
      uint32_t val = 0xffffffffu;
      if (l < n && ((S >> l) & 1u))
        val = Dr[cur * kBatchDpRow + l] + g[l * half + batch_dp_squeeze(S, l)];
      uint64_t v = ((uint64_t)val << 8) | (uint32_t)l;
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 16);
        v = o < v ? o : v;
      }
      const int i = (int)(v & 0xffu);
      if (s == 0) total = (uint32_t)(v >> 8);
      if (l == 0) a.tours[req * n + s] = (uint16_t)(i + 1);
      cur = i + 1;
      S &= ~(1u << i);
    }
    if (l == 0) a.keys[req] = pack_key(0, total, 0);
  }
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_tsp_batch_dp(vrpms_ctx* ctx, const int32_t* d_mats, int32_t R, int32_t N,
                                  uint16_t* d_tours, uint64_t* d_keys, void* stream) {
  if (!ctx) return fail(VRPMS_EINVAL, "vrpms_tsp_batch_dp: ctx is NULL");
  if (R < 0) return fail(VRPMS_EINVAL, "vrpms_tsp_batch_dp: R must not be negative");
  if (N < 2 || N > kBatchDpNodes)
    return fail(VRPMS_EINVAL, "vrpms_tsp_batch_dp: the LDS-resident table needs 2 <= N <= 13 (" +
                                  std::to_string(N) + " given)");
  if (R == 0) return VRPMS_OK;
  if (!d_mats || !d_tours || !d_keys)
    return fail(VRPMS_EINVAL, "vrpms_tsp_batch_dp: NULL matrix/tour/key buffer");
  const int n = N - 1;
  const int T = ctx->opt_batch_dp_team ? ctx->opt_batch_dp_team : kBatchDpTeam[n];
  const size_t lds = batch_dp_lds_bytes(n, T);
  if (lds > ctx->max_lds)
    return fail(VRPMS_EINVAL, "vrpms_tsp_batch_dp: " + std::to_string(256 / T) + " tables of n = " +
                                  std::to_string(n) + " need " + std::to_string(lds) +
                                  " bytes of LDS (" + std::to_string(ctx->max_lds) + " available)");
  VRPMS_HIP(hipSetDevice(ctx->device));
  const BatchDpArgs a{d_mats, R, N, d_tours, d_keys};
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = batch_with_team(T, [&](auto t) {
    return batch_launch(tsp_batch_dp_kernel<decltype(t)::value>, a, R, T, lds, s);
  });
  VRPMS_HIP(e);
  return VRPMS_OK;
}
