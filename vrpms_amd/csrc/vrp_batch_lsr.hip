// Throughput mode of a multi-start local search over separator tours for the
// VRP: vrp_batch_ls's descent (A25) on the tours
// vrp_batch_sa anneals (A22).  R independent small-fleet CVRP requests of one
// (N, K, H, objective, S, rounds) share one launch, ONE WORKGROUP PER REQUEST.
// The workgroup stages its request's whole instance into LDS exactly as
// vrp_batch_sa does (batch_stage.hpp).  Its four wavefronts then work alone
// until the final selection; wavefront w descends the starts w, w + 4, ... one
// after the other on tours of L = n + K - 1 tokens, n = N - 1 customers and
// K - 1 separators (the token 0, A10):
//
//   start s  vrp_batch_ls's start s, the Philox Fisher-Yates shuffle of 1..n
//            with counters (0xffffffff, 0xffffffff, s, q), then
//            spec.pack_separators: first fit into K routes, one lane per route
//            (the fitting routes by one ballot).  The wave has no third row
//            for it, so the packing is in place: the row starts as K - 1
//            separators followed by the shuffle, and customer q, at position
//            K - 1 + q, is relocated to the end of its route -- the tokens of
//            the later routes move up one place, by the descent's own relocate;
//   round    vrp_batch_ls's (batch_ls.hpp) over the L positions: all
//            2 L (L - 1) moves (typ, i, j), separators moved like customers,
//            lane l pricing the ids [l per, (l + 1) per), the least (key, typ,
//            i, j) applied in place while its key is below the tour's, at most
//            `rounds` applied moves.  L < 2 has no moves;
//   answer   the least (key, s) over the S end tours: each wave keeps its own,
//            and after the kernel's one barrier past staging the wave that
//            holds the least walks it once more and writes the K route
//            durations, every token's vehicle, s and the capped count.
//
// The counters carry no request row: an answer does not depend on the launch
// the request rode in or on its row in it.  With K = 1 the answer is
// vrp_batch_ls's; with S = 4 and rounds = 0 it is vrp_batch_sa's at steps = 0.
//
// LDS, every part as the kernel carves it (vrpms_vrp_batch_lsr_lds), never more
// than vrpms_vrp_batch_sa_lds of the same shape:
//   align16(H N N (wide ? 4 : 2))            the matrix
// + 4 align4(N) + 2 * 4 align4(K)            demand, capacities, start times (int32)
// + 4 * 2 * 2 align8(L)                      4 waves x (current, best end) uint16 tours
// + 4 * 16                                   the waves' best key, best s, capped count
#include <hip/hip_runtime.h>

#include "vrp_batch_lsr.hpp"

namespace vrpms {

template <typename MatT, int HM>
__global__ __launch_bounds__(256) void vrp_batch_lsr_kernel(VrpBatchLsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char batch_lsr_lds_mem[];
  const int N = a.N, n = N - 1, K = a.K, L = n + K - 1;
  const int64_t r = blockIdx.x;
  const uint32_t cells = (uint32_t)HM * (uint32_t)N * (uint32_t)N;
  const uint32_t mat_bytes = (cells * (uint32_t)sizeof(MatT) + 15u) & ~15u;
  const uint32_t dem_words = ((uint32_t)N + 3u) & ~3u, row_words = ((uint32_t)K + 3u) & ~3u;
  const uint32_t tpad = ((uint32_t)L + 7u) & ~7u;
  MatT* M = reinterpret_cast<MatT*>(batch_lsr_lds_mem);
  int32_t* dem = reinterpret_cast<int32_t*>(batch_lsr_lds_mem + mat_bytes);
  int32_t* cap = dem + dem_words;
  int32_t* start = cap + row_words;
  uint16_t* tours = reinterpret_cast<uint16_t*>(start + row_words);          // [4][2][tpad]
  BatchLsWave* wst = reinterpret_cast<BatchLsWave*>(tours + 4 * 2 * tpad);    // [4]

  // stage and check the request (batch_stage.hpp); the verdict goes through
  // a word of the waves' records, free until the descents end
  uint16_t* gtour = a.tours + r * L;
  int8_t* gveh = a.veh + r * L;
  int32_t* gdurs = a.durs + r * K;
  if (batch_stage_request(a.mats, a.demand, a.cap, a.start, r, cells, N, K, M, dem, cap, start,
                          reinterpret_cast<uint32_t*>(wst))) {
    batch_refuse(gtour, gveh, gdurs, a.keys + r, L, K);
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

  const BatchLsShare sh = batch_ls_share(L, lane);   // the lane's share of a round

  uint64_t bk = ~0ull;
  int bs = 0x7fffffff, capped = 0;
  for (int s = wave; s < a.S; s += 4) {
    // start s: the shuffle, packed first-fit in place (vrp_batch_lsr.hpp)
    batch_lsr_start(A, dem, cap, n, K, s, a.seed_lo, a.seed_hi, lane);
    uint64_t ck = readlane_u64(eval_tour<true>(D, sp, [&](int q) { return (uint32_t)A[q]; }, L).key, 0);
    if (L >= 2) ck = batch_ls_descend(D, sp, A, L, ck, a.rounds, sh, lane, capped);
    if (ck < bk) {   // s rises: the least s among equal keys stays
      bk = ck;
      bs = s;
      for (int q = lane; q < L; q += 64) Best[q] = A[q];
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
  const int mydur = batch_final_walk(D, dem, cap, start, K, n, Best, L, V, lane);
  wave_sync();
  for (int q = lane; q < L; q += 64) {
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

extern "C" int vrpms_vrp_batch_lsr_lds(int32_t N, int32_t K, int32_t H, int32_t wide, uint64_t* bytes) {
  const char* who = "vrpms_vrp_batch_lsr_lds";
  if (const int rc = batch_check_bytes(who, bytes)) return rc;
  if (const int rc = batch_lsr_check(who, N, K, H, wide)) return rc;
  *bytes = batch_ls_lds(N, K, H, wide, N - 1 + K - 1);
  return VRPMS_OK;
}

extern "C" int vrpms_vrp_batch_lsr(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                                   const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                                   int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t S,
                                   int32_t rounds, uint64_t seed, uint16_t* d_tours, uint64_t* d_keys,
                                   int32_t* d_durs, int8_t* d_veh, int32_t* d_info, void* stream) {
  const char* who = "vrpms_vrp_batch_lsr";
  if (const int rc = batch_check_ctx(who, ctx, R)) return rc;
  if (const int rc = batch_lsr_check(who, N, K, H, wide)) return rc;
  const VrpBatchLsArgs a{d_mats, d_demand, d_cap,  d_start, R,      N,      K,      H,     objective,
                         S,      rounds,   (uint32_t)seed, (uint32_t)(seed >> 32), d_tours, d_keys,
                         d_durs, d_veh,    d_info};
  return batch_ls_launch(who, ctx, a, wide, N - 1 + K - 1, stream, [](auto m, auto hm) {
    return vrp_batch_lsr_kernel<decltype(m), decltype(hm)::value>;
  });
}
