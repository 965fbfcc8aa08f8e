// Throughput mode of a multi-start local search over PLAIN separator tours for
// the VRP on a static matrix, with delta pricing:
// vrp_batch_lsr's mapping, starts, moves and answer (A26) on the neighbourhood
// of the tours whose K - 1 separators alone decide the routes.  R independent
// small-fleet CVRP requests of one (N, K, objective, S, rounds) share one
// launch, ONE WORKGROUP PER REQUEST.  The workgroup stages its request's whole
// instance into LDS (batch_stage.hpp) and zeroes the matrix cell 0 -> 0, which
// no walk reads: a separator then prices as the depot.  Its four wavefronts
// work alone until the final selection; wavefront w descends the starts w,
// w + 4, ... one after the other on tours of L = n + K - 1 tokens:
//
//   plain    a tour of n customers and K - 1 separators is plain when the
//            customers between separator g - 1 and separator g weigh at most
//            cap[g], g = 0 .. K - 1: the greedy split then overflows nowhere,
//            leaves nobody out, and route g's duration is the closed chain
//            depot -> segment g -> depot;
//   start s  vrp_batch_lsr's (batch_lsr_start), keyed by one walk.  A start
//            that is not plain -- the first fit found no room for a customer --
//            does not descend: it ends where it starts and is never capped;
//   round    vrp_batch_lsr's 2 L (L - 1) moves in its order and with its share
//            per lane, but a move whose moved tour is not plain is no
//            candidate, and a candidate is priced from the wavefront's rows
//            (vrp_batch_lsf.hpp): the sum is the current one plus the TSP
//            delta on the token chain, the capacities and the maximum come
//            from the segments the move spans.  No candidate is walked.  The
//            least (key, typ, i, j) is applied in place while its key is below
//            the tour's, the rows are rebuilt, at most `rounds` moves.  L < 2
//            has no moves;
//   answer   vrp_batch_lsr's: the least (key, s) over the S end tours, walked
//            once more for the durations and every token's vehicle.
//
// With every capacity at least the total demand every tour is plain and the
// rows are vrp_batch_lsr's bit for bit; with rounds = 0 they are for any
// capacities, but for the capped count, which leaves out the starts that are
// not plain.
//
// LDS, every part as the kernel carves it (vrpms_vrp_batch_lsf_lds), with
// L2 = L + 2:
//   align16(N N (wide ? 4 : 2))                   the matrix
// + 4 align4(N) + 2 * 4 align4(K)                 demand, capacities, start times (int32)
// + 4 * 16                                        the waves' best key, best s, capped count
// + 4 * 4 (3 align4(L2) + 5 align4(K + 1))        4 waves x int32 rows F, B, W and tables FD, BD, LD, PM, SM
// + 4 * 2 (align8(L2) + align8(L) + align8(K + 1))  4 waves x uint16 current tour, best end tour, S
// + 4 * align8(L2)                                4 waves x the uint8 segment row G
#include <hip/hip_runtime.h>

#include "vrp_batch_lsf.hpp"

namespace vrpms {

template <typename MatT>
__global__ __launch_bounds__(256) void vrp_batch_lsf_kernel(VrpBatchLsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char batch_lsf_lds_mem[];
  const int N = a.N, n = N - 1, K = a.K, L = n + K - 1;
  const int64_t r = blockIdx.x;
  const BatchInst<MatT, 1> in(batch_lsf_lds_mem, BatchInst<MatT, 1>::parts(N, K), N, K);
  const BatchLsfParts<uint32_t> lp((uint32_t)L, (uint32_t)K);
  BatchLsWave* wst = reinterpret_cast<BatchLsWave*>(in.rest);                 // [4]
  int32_t* words = reinterpret_cast<int32_t*>(wst + 4);                       // [4][lp.words()]
  uint16_t* halves = reinterpret_cast<uint16_t*>(words + 4 * lp.words());     // [4][lp.halves()]
  uint8_t* bytes = reinterpret_cast<uint8_t*>(halves + 4 * lp.halves());      // [4][lp.gpad]

  // stage and check the request (batch_stage.hpp); the verdict goes through
  // a word of the waves' records, free until the descents end
  uint16_t* gtour = a.tours + r * L;
  int8_t* gveh = a.veh + r * L;
  int32_t* gdurs = a.durs + r * K;
  if (batch_stage_request(a, r, in, wst)) {
    batch_refuse(gtour, gveh, gdurs, a.keys + r, L, K);
    if (threadIdx.x == 0) {
      a.info[2 * r] = -1;
      a.info[2 * r + 1] = 0;
    }
    return;
  }

  const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
  int32_t* w32 = words + wave * lp.words();
  uint16_t* w16 = halves + wave * lp.halves();
  LsfRows rows;
  rows.F = w32;
  rows.B = rows.F + lp.row_words;
  rows.W = reinterpret_cast<uint32_t*>(rows.B + lp.row_words);
  rows.FD = w32 + 3 * lp.row_words;
  rows.BD = rows.FD + lp.tab_words;
  rows.LD = reinterpret_cast<uint32_t*>(rows.BD + lp.tab_words);
  rows.PM = rows.BD + 2 * lp.tab_words;
  rows.SM = rows.PM + lp.tab_words;
  rows.P = w16;
  uint16_t* Best = w16 + lp.ppad;   // the wave's best end tour
  rows.S = Best + lp.bpad;
  rows.G = bytes + wave * lp.gpad;
  uint16_t* A = rows.P + 1;          // the current tour
  const int32_t *dem = in.dem, *cap = in.cap;
  const MatView<MatT, 1> D{in.M, (uint32_t)N, (uint32_t)N * (uint32_t)N, 1};
  const SplitParams sp{dem, cap, in.start, K, a.objective};

  // the staging check has seen the cell 0 -> 0; from here on a separator is
  // the depot at no cost.  Every wave writes the same zero before it reads.
  if (lane == 0) {
    in.M[0] = 0;
    rows.P[0] = 0;
    rows.P[L + 1] = 0;
  }
  wave_sync();

  const BatchLsShare sh = batch_ls_share(L, lane);   // the lane's share of a round

  uint64_t bk = ~0ull;
  int bs = 0x7fffffff, capped = 0;
  for (int s = wave; s < a.S; s += 4) {
    batch_lsr_start(A, dem, cap, n, K, s, a.seed_lo, a.seed_hi, lane);
    uint64_t ck = readlane_u64(eval_tour<true>(D, sp, [&](int q) { return (uint32_t)A[q]; }, L).key, 0);
    if (L >= 2) {
      int dmax;
      int sum = lsf_rows(D, dem, rows, L, K, lane, dmax);
      if (lsf_plain(dem, cap, rows, K, lane)) {
        for (int applied = 0;; ++applied) {
          if (applied >= a.rounds) {   // stopped unproven
            ++capped;
            break;
          }
          Move m = sh.m0, lm = sh.m0;
          uint64_t lk = ck;   // only a key below the tour's is of use
          for (int c = 0; c < sh.cnt; ++c) {
            const uint64_t k = lsf_price(D, cap, rows, L, sum, a.objective, m, lk);
            if (k < lk) {
              lk = k;
              lm = m;
            }
            batch_ls_next(m, L);
          }
          // the lanes hold ascending id ranges: the lowest lane among equal
          // keys holds the least (typ, i, j)
          int bl;
          const uint64_t k = wave_argmin_lane(lk, bl);
          if (!(k < ck)) break;   // a local optimum
          Move mb;
          mb.typ = (uint32_t)wave_bcast((int)lm.typ, bl);
          mb.i = wave_bcast(lm.i, bl);
          mb.j = wave_bcast(lm.j, bl);
          batch_ls_apply(A, mb, lane);
          sum = lsf_rows(D, dem, rows, L, K, lane, dmax);
          ck = cvrp_key(0, (uint32_t)sum, (uint32_t)dmax, a.objective);
        }
      }
    }
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
  const int mydur = batch_final_walk(D, dem, cap, in.start, K, n, Best, L, V, lane);
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

extern "C" int vrpms_vrp_batch_lsf_lds(int32_t N, int32_t K, int32_t wide, uint64_t* bytes) {
  const char* who = "vrpms_vrp_batch_lsf_lds";
  if (const int rc = batch_check_bytes(who, bytes)) return rc;
  if (const int rc = batch_lsf_check(who, N, K, 1, wide)) return rc;
  *bytes = batch_lsf_lds(N, K, wide);
  return VRPMS_OK;
}

extern "C" int vrpms_vrp_batch_lsf(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                                   const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                                   int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t S,
                                   int32_t rounds, uint64_t seed, uint16_t* d_tours, uint64_t* d_keys,
                                   int32_t* d_durs, int8_t* d_veh, int32_t* d_info, void* stream) {
  const char* who = "vrpms_vrp_batch_lsf";
  if (const int rc = batch_check_ctx(who, ctx, R)) return rc;
  if (const int rc = batch_lsf_check(who, N, K, H, wide)) return rc;
  if (const int rc = batch_ls_check_search(who, objective, S, rounds)) return rc;
  if (R == 0) return VRPMS_OK;
  if (const int rc = batch_check_buffers(
          who, "matrix/demand/capacity/start/tour/key/duration/vehicle/info",
          {d_mats, d_demand, d_cap, d_start, d_tours, d_keys, d_durs, d_veh, d_info}))
    return rc;
  const size_t lds = batch_lsf_lds(N, K, wide);
  if (lds > ctx->max_lds) return batch_lds_refusal(who, N, K, H, wide, "", lds, ctx->max_lds);
  VRPMS_HIP(hipSetDevice(ctx->device));
  const VrpBatchLsArgs a{d_mats, d_demand, d_cap,  d_start, R,      N,      K,      H,     objective,
                         S,      rounds,   (uint32_t)seed, (uint32_t)(seed >> 32), d_tours, d_keys,
                         d_durs, d_veh,    d_info};
  const char* what = "";
  const hipError_t e = batch_with_matrix(wide, 1, [&](auto m, auto) {
    return batch_launch_blocks(vrp_batch_lsf_kernel<decltype(m)>, a, (unsigned)R, lds, (hipStream_t)stream,
                               &what);
  });
  if (e != hipSuccess) return hip_fail(e, what);
  return VRPMS_OK;
}
