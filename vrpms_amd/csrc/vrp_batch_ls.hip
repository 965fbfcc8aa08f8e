// Throughput mode of a multi-start local search for the VRP (DESIGN.md §2 A25,
// §4.3p): R independent small-fleet CVRP requests of one (N, K, H, objective,
// S, rounds) share one launch, ONE WORKGROUP PER REQUEST.  The workgroup stages
// its request's whole instance into LDS exactly as vrp_batch_sa does
// (batch_stage.hpp: the [H][N][N] matrix as uint16, or int32 when `wide`, the
// demand, capacity and start-time rows; a negative entry, or one above 65535
// under wide = 0, ends the request with an all-ones key).  Its four wavefronts
// then work alone until the final selection; wavefront w descends the starts
// w, w + 4, ... one after the other on tours of n = N - 1 customers (no
// separators: the greedy split prices them):
//
//   start s  vrp_batch_ga's member s: the Philox Fisher-Yates shuffle of 1..n,
//            counters (0xffffffff, 0xffffffff, s, q);
//   round    every move (typ, i, j) -- swap and 2-opt with i < j, relocate with
//            i != j, 2 n (n - 1) in all -- is priced by eval_tour<true> over
//            map_src(move_map(m), q).  The moves are numbered in (typ, i, j)
//            order and lane l takes the ids [l per, (l + 1) per), per =
//            ceil(2 n (n - 1) / 64): it decodes its first move once a launch
//            and steps to the next by increments, keeping its least (key, id).
//            The (key, lane) minimum of the wave is then the least (key, typ,
//            i, j).  A key below the tour's applies the move in place (lane
//            0 swaps; lanes reverse a 2-opt window by pairs; a relocate shifts
//            by chunks of 64) and the next round follows; otherwise the tour
//            is a local optimum.  After `rounds` applied moves the descent
//            stops unproven and counts as capped.  n < 2 has no moves;
//   answer   the least (key, s) over the S end tours: each wave keeps its own,
//            and after the kernel's one barrier past staging the wave that
//            holds the least walks it once more and writes the K route
//            durations, every gene's vehicle, s and the capped count.
//
// The counters carry no request row: an answer does not depend on the launch
// the request rode in or on its row in it.  With rounds = 0 the answer is
// vrp_batch_ga's at P = S, G = 0.  The move order, the lane's share, the start
// shuffle, the in-place move and the round loop are batch_ls.hpp's, shared with
// vrp_batch_lsr.hip (A26).
//
// LDS, every part as the kernel carves it (vrpms_vrp_batch_ls_lds), never more
// than vrpms_vrp_batch_sa_lds of the same shape:
//   align16(H N N (wide ? 4 : 2))            the matrix
// + 4 align4(N) + 2 * 4 align4(K)            demand, capacities, start times (int32)
// + 4 * 2 * 2 align8(n)                      4 waves x (current, best end) uint16 tours
// + 4 * 16                                   the waves' best key, best s, capped count
#include <hip/hip_runtime.h>

#include "vrp_batch_lsr.hpp"

namespace vrpms {

template <typename MatT, int HM>
__global__ __launch_bounds__(256) void vrp_batch_ls_kernel(VrpBatchLsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char batch_ls_lds_mem[];
  const int N = a.N, n = N - 1, K = a.K;
  const int64_t r = blockIdx.x;
  const uint32_t cells = (uint32_t)HM * (uint32_t)N * (uint32_t)N;
  const uint32_t mat_bytes = (cells * (uint32_t)sizeof(MatT) + 15u) & ~15u;
  const uint32_t dem_words = ((uint32_t)N + 3u) & ~3u, row_words = ((uint32_t)K + 3u) & ~3u;
  const uint32_t tpad = ((uint32_t)n + 7u) & ~7u;
  MatT* M = reinterpret_cast<MatT*>(batch_ls_lds_mem);
  int32_t* dem = reinterpret_cast<int32_t*>(batch_ls_lds_mem + mat_bytes);
  int32_t* cap = dem + dem_words;
  int32_t* start = cap + row_words;
  uint16_t* tours = reinterpret_cast<uint16_t*>(start + row_words);          // [4][2][tpad]
  BatchLsWave* wst = reinterpret_cast<BatchLsWave*>(tours + 4 * 2 * tpad);    // [4]

  // stage and check the request (batch_stage.hpp); the verdict goes through
  // a word of the waves' records, free until the descents end
  uint16_t* gtour = a.tours + r * n;
  int8_t* gveh = a.veh + r * n;
  int32_t* gdurs = a.durs + r * K;
  if (batch_stage_request(a.mats, a.demand, a.cap, a.start, r, cells, N, K, M, dem, cap, start,
                          reinterpret_cast<uint32_t*>(wst))) {
    batch_refuse(gtour, gveh, gdurs, a.keys + r, n, K);
    if (threadIdx.x == 0) {
      a.info[2 * r] = -1;
      a.info[2 * r + 1] = 0;
    }
    return;
  }

  const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
  uint16_t* A = tours + wave * 2 * tpad;   // current tour
  uint16_t* Best = A + tpad;               // the wave's best end tour
  const MatView<MatT, HM> D{M, (uint32_t)N, (uint32_t)N * (uint32_t)N, HM};
  const SplitParams sp{dem, cap, start, K, a.objective};

  const BatchLsShare sh = batch_ls_share(n, lane);   // the lane's share of a round

  uint64_t bk = ~0ull;
  int bs = 0x7fffffff, capped = 0;
  for (int s = wave; s < a.S; s += 4) {
    batch_ls_shuffle(A, n, s, a.seed_lo, a.seed_hi, lane);
    uint64_t ck = readlane_u64(eval_tour<true>(D, sp, [&](int q) { return (uint32_t)A[q]; }, n).key, 0);
    if (n >= 2) ck = batch_ls_descend(D, sp, A, n, ck, a.rounds, sh, lane, capped);
    if (ck < bk) {   // s rises: the least s among equal keys stays
      bk = ck;
      bs = s;
      for (int q = lane; q < n; q += 64) Best[q] = A[q];
      wave_sync();
    }
  }
  if (lane == 0) wst[wave] = BatchLsWave{bk, bs, capped};
  __syncthreads();
  int ncap;
  const int bw = batch_ls_winner(wst, ncap);
  if (wave != bw) return;

  // the winner's best end tour once more, as spec.eval_cvrp walks it: every
  // lane walks alike, lane k keeps route k's duration, lane 0 notes the
  // vehicles (as int16 in the wave's current tour, no longer needed)
  int16_t* V = reinterpret_cast<int16_t*>(A);
  const int mydur = batch_final_walk(D, dem, cap, start, K, n, Best, n, V, lane);
  wave_sync();
  for (int q = lane; q < n; q += 64) {
    gtour[q] = Best[q];
    gveh[q] = (int8_t)V[q];
  }
  if (lane < K) gdurs[lane] = mydur;
  if (lane == 0) {
    a.keys[r] = bk;
    a.info[2 * r] = bs;
    a.info[2 * r + 1] = ncap;
  }
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_vrp_batch_ls_lds(int32_t N, int32_t K, int32_t H, int32_t wide, uint64_t* bytes) {
  const char* who = "vrpms_vrp_batch_ls_lds";
  if (const int rc = batch_check_bytes(who, bytes)) return rc;
  if (const int rc = batch_check_shape(who, N, K, H, wide)) return rc;
  *bytes = batch_ls_lds(N, K, H, wide, N - 1);
  return VRPMS_OK;
}

extern "C" int vrpms_vrp_batch_ls(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                                  const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                                  int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t S,
                                  int32_t rounds, uint64_t seed, uint16_t* d_tours, uint64_t* d_keys,
                                  int32_t* d_durs, int8_t* d_veh, int32_t* d_info, void* stream) {
  const char* who = "vrpms_vrp_batch_ls";
  if (const int rc = batch_check_ctx(who, ctx, R)) return rc;
  if (const int rc = batch_check_shape(who, N, K, H, wide)) return rc;
  const VrpBatchLsArgs a{d_mats, d_demand, d_cap,  d_start, R,      N,      K,      H,     objective,
                         S,      rounds,   (uint32_t)seed, (uint32_t)(seed >> 32), d_tours, d_keys,
                         d_durs, d_veh,    d_info};
  return batch_ls_launch(who, ctx, a, wide, N - 1, stream, [](auto m, auto hm) {
    return vrp_batch_ls_kernel<decltype(m), decltype(hm)::value>;
  });
}
