// Throughput mode of the VRP annealer: R independent
// small-fleet CVRP requests of one (N, K, H, objective) share one launch, ONE
// WORKGROUP PER REQUEST.  The workgroup stages its request's whole instance --
// the [H][N][N] matrix (uint16, or int32 when `wide`), the demand row, the
// capacity row and the start-time row -- into LDS once and checks it on the way
// (a negative entry, or one above 65535 under wide = 0, ends the request with
// an all-ones key; its neighbours in the launch never see it).  Its four
// wavefronts are four SA chains w = 0..3:
//
//   start   Philox Fisher-Yates of 1..n, counters (0xffffffff, 0xffffffff, w, i),
//           then spec.pack_separators: first fit into K routes, one lane per
//           route (the fitting routes by one ballot), K - 1 separators;
//   step s  lane l decodes word s & 3 of the block (s >> 2, 0, w, l) with A13's
//           decode_move1 over the ntok = n + K - 1 tokens and prices the moved
//           tour by eval_tour<true> over moved_index (the greedy split and the
//           departure times make a delta non-local); the (key, lane) minimum of
//           the wave is the proposal; the acceptance draw is word s & 3 of the
//           block (s >> 2, 1, w, 0) -- wave-uniform counters, so it sits on the
//           scalar unit;
//   answer  the best (key, w); that wavefront walks its best tour once more
//           and writes the K route durations and every token's vehicle.
//
// The counters carry w, not 4 r + w as tsp_batch_sa's do: a request's answer
// does not depend on the launch it rode in or on its row in it.
//
// LDS, every part as the kernel carves it (vrpms_vrp_batch_sa_lds):
//   align16(H N N (wide ? 4 : 2))            the matrix
// + 4 align4(N) + 2 * 4 align4(K)            demand, capacities, start times (int32)
// + 4 * 3 * 2 align8(ntok)                   4 chains x (current, scratch, best) uint16 tours
// + 4 * 8                                    the chains' best keys
#include <hip/hip_runtime.h>

#include <string>

#include "batch_launch.hpp"
#include "batch_stage.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "staging.hpp"
#include "tour.hpp"

namespace vrpms {

struct VrpBatchSaArgs {
  const int32_t* mats;    // [R][H][N][N]
  const int32_t* demand;  // [R][N]
  const int32_t* cap;     // [R][K]
  const int32_t* start;   // [R][K]
  const float* inv_t0;    // [R]
  int R, N, K, H, objective, steps;
  float inv_alpha;
  uint32_t seed_lo, seed_hi;
  uint16_t* tours;        // [R][ntok]
  uint64_t* keys;         // [R]
  int32_t* durs;          // [R][K]
  int8_t* veh;            // [R][ntok]
};

// the kernel's own parts behind the instance, in their order
template <typename I>
struct BatchSaParts {
  I tpad;   // a tour's padded tokens
  __host__ __device__ explicit BatchSaParts(I ntok) : tpad(batch_align<I>(ntok, 8)) {}
  __host__ __device__ I tour_tokens() const { return 4 * 3 * tpad; }   // 4 chains x (current, scratch, best), uint16
  __host__ __device__ I bytes() const { return 2 * tour_tokens() + 4 * 8; }   // then the chains' best keys, uint64
};

inline size_t batch_sa_lds(int N, int K, int H, int wide) {
  return batch_inst_bytes(N, K, H, wide) + BatchSaParts<size_t>((size_t)N - 1 + K - 1).bytes();
}

template <typename MatT, int HM>
__global__ __launch_bounds__(256) void vrp_batch_sa_kernel(VrpBatchSaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char batch_sa_lds_mem[];
  const int N = a.N, n = N - 1, K = a.K, ntok = n + K - 1;
  const int64_t r = blockIdx.x;
  const auto ip = BatchInst<MatT, HM>::parts(N, K);
  const BatchSaParts<uint32_t> l((uint32_t)ntok);
  const BatchInst<MatT, HM> c(batch_sa_lds_mem, ip, N, K);
  const uint32_t cells = c.cells, tpad = l.tpad;
  MatT* M = c.M;
  int32_t *dem = c.dem, *cap = c.cap, *start = c.start;
  uint16_t* tours = reinterpret_cast<uint16_t*>(c.rest);
  uint64_t* wbest = reinterpret_cast<uint64_t*>(tours + l.tour_tokens());

  // stage and check the request (batch_stage.hpp); the verdict goes through
  // a word of wbest, free until the chains end
  uint16_t* gtour = a.tours + r * ntok;
  int8_t* gveh = a.veh + r * ntok;
  int32_t* gdurs = a.durs + r * K;
  if (batch_stage_request(a.mats, a.demand, a.cap, a.start, r, cells, N, K, M, dem, cap, start,
                          reinterpret_cast<uint32_t*>(wbest))) {  // outside the launch's promise: no step
    batch_refuse(gtour, gveh, gdurs, a.keys + r, ntok, K);
    return;
  }

  const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
  uint16_t* A = tours + wave * 3 * tpad;   // current tour
  uint16_t* B = A + tpad;                  // scratch for the accepted move
  uint16_t* Best = A + 2 * tpad;
  const MatView<MatT, HM> D{M, (uint32_t)N, (uint32_t)N * (uint32_t)N, HM};
  const SplitParams sp{dem, cap, start, K, a.objective};

  // Philox Fisher-Yates start as in tsp_batch_body: lane l draws the block of
  // i = 64 c + l for a chunk of 64 swaps at once, lane 0 swaps
  for (int q = lane; q < n; q += 64) A[q] = (uint16_t)(q + 1);
  wave_sync();
  uint32_t jv = 0;
  for (int i = n - 1; i >= 1; --i) {
    if (i == n - 1 || (i & 63) == 63) {
      const uint32_t il = (uint32_t)(i & ~63) + (uint32_t)lane;
      const u32x4 x = philox(0xffffffffu, 0xffffffffu, (uint32_t)wave, il, a.seed_lo, a.seed_hi);
      jv = x.x % (il + 1u);
    }
    const int j = __builtin_amdgcn_readlane((int)jv, i & 63);
    if (lane == 0) {
      const uint16_t t = A[i];
      A[i] = A[j];
      A[j] = t;
    }
  }
  wave_sync();
  // spec.pack_separators(perm, K - 1): lane b holds route b's load and room;
  // customer q goes to the first route that has room for it, to the last one
  // when none has (B[q] = its route), then the routes are laid out in order
  // with a separator between them
  {
    const int64_t room = lane < K ? (int64_t)cap[lane] : -1;
    int64_t load = 0;
    int cnt = 0;
    for (int q = 0; q < n; ++q) {
      const int64_t d = dem[A[q]];
      const uint64_t fits = __builtin_amdgcn_ballot_w64(lane < K && load + d <= room);
      const int b = fits ? (int)__builtin_ctzll(fits) : K - 1;
      if (lane == b) {
        load += d;
        ++cnt;
      }
      if (lane == 0) B[q] = (uint16_t)b;
    }
    int off = 0, run = 0;   // route b starts at (customers of the routes before it) + b
    for (int b = 0; b < K; ++b) {
      if (lane == b) off = run + b;
      run += __builtin_amdgcn_readlane(cnt, b);
    }
    for (int q = lane; q < ntok; q += 64) Best[q] = 0;
    wave_sync();
    for (int q = 0; q < n; ++q) {
      const int b = __builtin_amdgcn_readfirstlane((int)B[q]);
      const int pos = __builtin_amdgcn_readlane(off, b);
      if (lane == b) ++off;
      if (lane == 0) Best[pos] = A[q];
    }
    wave_sync();
    uint16_t* t = A;   // the packed tour becomes the current one
    A = Best;
    Best = t;
  }

  uint64_t ck = eval_tour<true>(D, sp, [&](int i) { return (uint32_t)A[i]; }, ntok).key;
  uint64_t bk = ck;
  for (int q = lane; q < ntok; q += 64) Best[q] = A[q];
  wave_sync();
  float invT = a.inv_t0[r];
  // one SA step: xm = the lane's move word, xa = the chain's acceptance draw
  auto step = [&](uint32_t xm, uint32_t xa) __attribute__((always_inline)) {
    const Move m = decode_move1(xm, ntok);
    int bl;
    const uint64_t k = wave_argmin_lane(
        eval_tour<true>(D, sp, [&](int q) { return (uint32_t)A[moved_index(q, m)]; }, ntok).key, bl);
    bool accept = k <= ck;
    if (!accept) {
      const uint64_t d = (k >> 28) - (ck >> 28);
      const uint32_t dp = d > 0xffffffffull ? 0xffffffffu : (uint32_t)d;
      accept = accept_test(dp, invT, xa >> 8);   // (xa >> 8) < accept_threshold(dp, invT)
    }
    if (accept) {  // bl is wave-uniform: the winner's move by v_readlane
      Move mb;
      mb.typ = (uint32_t)wave_bcast((int)m.typ, bl);
      mb.i = wave_bcast(m.i, bl);
      mb.j = wave_bcast(m.j, bl);
      for (int q = lane; q < ntok; q += 64) B[q] = A[moved_index(q, mb)];
      wave_sync();
      uint16_t* t = A;
      A = B;
      B = t;
      ck = k;
      if (ck < bk) {
        bk = ck;
        for (int q = lane; q < ntok; q += 64) Best[q] = A[q];
      }
      wave_sync();
    }
    invT = invT * a.inv_alpha;
  };
  // A13: one Philox block per lane serves four steps, one per chain their
  // acceptance draws; unrolled by four, so each step reads its words without a
  // select
  if (ntok >= 2) {
    int s = 0;
    for (; s + 4 <= a.steps; s += 4) {
      const u32x4 rb = philox((uint32_t)(s >> 2), 0u, (uint32_t)wave, (uint32_t)lane, a.seed_lo, a.seed_hi);
      const u32x4 ra = philox((uint32_t)(s >> 2), 1u, (uint32_t)wave, 0u, a.seed_lo, a.seed_hi);
      step(rb.x, ra.x);
      step(rb.y, ra.y);
      step(rb.z, ra.z);
      step(rb.w, ra.w);
    }
    if (s < a.steps) {  // the last 1..3 steps
      const u32x4 rb = philox((uint32_t)(s >> 2), 0u, (uint32_t)wave, (uint32_t)lane, a.seed_lo, a.seed_hi);
      const u32x4 ra = philox((uint32_t)(s >> 2), 1u, (uint32_t)wave, 0u, a.seed_lo, a.seed_hi);
      for (int h = 0; s + h < a.steps; ++h)
        step(h == 0 ? rb.x : h == 1 ? rb.y : rb.z, h == 0 ? ra.x : h == 1 ? ra.y : ra.z);
    }
  }
  if (lane == 0) wbest[wave] = bk;
  __syncthreads();
  int bw = 0;
  for (int w = 1; w < 4; ++w)
    if (wbest[w] < wbest[bw]) bw = w;
  if (wave != bw) return;

  // the winner's best tour once more, as spec.eval_cvrp walks it: every lane
  // walks alike, lane k keeps route k's duration, lane 0 notes the vehicles
  // (as int16 in the chain's scratch tour)
  int16_t* V = reinterpret_cast<int16_t*>(B);
  const int mydur = batch_final_walk(D, dem, cap, start, K, n, Best, ntok, V, lane);
  wave_sync();
  for (int q = lane; q < ntok; q += 64) {
    gtour[q] = Best[q];
    gveh[q] = (int8_t)V[q];
  }
  if (lane < K) gdurs[lane] = mydur;
  if (lane == 0) a.keys[r] = bk;
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_vrp_batch_sa_lds(int32_t N, int32_t K, int32_t H, int32_t wide, uint64_t* bytes) {
  const char* who = "vrpms_vrp_batch_sa_lds";
  if (const int rc = batch_check_bytes(who, bytes)) return rc;
  if (const int rc = batch_check_shape(who, N, K, H, wide)) return rc;
  *bytes = batch_sa_lds(N, K, H, wide);
  return VRPMS_OK;
}

extern "C" int vrpms_vrp_batch_sa(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                                  const int32_t* d_cap, const int32_t* d_start, const float* d_inv_t0,
                                  int32_t R, int32_t N, int32_t K, int32_t H, int32_t objective,
                                  int32_t wide, int32_t steps, float inv_alpha, uint64_t seed,
                                  uint16_t* d_tours, uint64_t* d_keys, int32_t* d_durs, int8_t* d_veh,
                                  void* stream) {
  const char* who = "vrpms_vrp_batch_sa";
  if (const int rc = batch_check_ctx(who, ctx, R)) return rc;
  if (const int rc = batch_check_shape(who, N, K, H, wide)) return rc;
  if (const int rc = batch_check_objective(who, objective)) return rc;
  if (steps < 0) return fail(VRPMS_EINVAL, "vrpms_vrp_batch_sa: steps must not be negative");
  if (R == 0) return VRPMS_OK;
  if (const int rc = batch_check_buffers(
          who, "matrix/demand/capacity/start/inv_t0/tour/key/duration/vehicle",
          {d_mats, d_demand, d_cap, d_start, d_inv_t0, d_tours, d_keys, d_durs, d_veh}))
    return rc;
  const size_t lds = batch_sa_lds(N, K, H, wide);
  if (lds > ctx->max_lds) return batch_lds_refusal(who, N, K, H, wide, "", lds, ctx->max_lds);
  VRPMS_HIP(hipSetDevice(ctx->device));
  const VrpBatchSaArgs a{d_mats, d_demand, d_cap,  d_start, d_inv_t0, R,      N,      K,
                         H,      objective, steps, inv_alpha, (uint32_t)seed, (uint32_t)(seed >> 32),
                         d_tours, d_keys, d_durs, d_veh};
  const char* what = "";
  const hipError_t e = batch_with_matrix(wide, H, [&](auto m, auto hm) {
    return batch_launch_blocks(vrp_batch_sa_kernel<decltype(m), decltype(hm)::value>, a, (unsigned)R, lds,
                               (hipStream_t)stream, &what);
  });
  if (e != hipSuccess) return hip_fail(e, what);
  return VRPMS_OK;
}
