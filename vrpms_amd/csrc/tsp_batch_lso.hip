// Throughput mode of a multi-start local search for the TSP with Or-opt and
// delta pricing: R independent TSP requests of one
// (N, H, S, rounds, moves) share one launch, ONE WORKGROUP PER REQUEST.  The
// workgroup stages its request's [H][N][N] matrix into LDS as vrp_batch_ls does
// (uint16, or int32 when `wide`; a negative entry, or one above 65535 under
// wide = 0, ends the request with the refusal row).  Its four wavefronts then
// work alone until the final selection; wavefront w descends the starts w,
// w + 4, ... one after the other on closed tours 0 -> p[0..n-1] -> 0 of the
// n = N - 1 customers, leaving node 0 at the request's start time:
//
//   start s  vrp_batch_ls's start s (batch_ls_shuffle): the Philox Fisher-Yates
//            shuffle of 1..n, counters (0xffffffff, 0xffffffff, s, q);
//   round    the moves (typ, i, j) of the types `moves` enables (bit t: typ t)
//            -- swap (0) and 2-opt (1) with i < j, relocate (2) with i != j,
//            Or-opt of m = 2 (typ 3) and 3 (typ 4) customers: seg = p[i:i+m],
//            rest = p[:i] + p[i+m:], the moved tour rest[:j] + seg + rest[j:],
//            0 <= i, j <= n - m, j != i -- are numbered in (typ, i, j) order
//            and lane l takes the ids [l per, (l + 1) per), per = ceil(total /
//            64).  A candidate's key is spec.tsp_key of its duration
//            (spec.eval_tsp, A4), found WITHOUT walking the tour:
//              H = 1   duration + delta.  Per wavefront two int32 prefix rows,
//                      F[q] = sum D(v[t-1], v[t]) and B[q] = sum D(v[t],
//                      v[t-1]) over t = 1..q of the padded tour v = 0, p, 0,
//                      rebuilt after every applied move by a wave scan.  A
//                      2-opt is two F terms, two B terms and four edges; swap
//                      and relocate are tour.hpp's tsp_move_delta; an Or-opt
//                      is three edges out (a -> s0, s_last -> b, pred -> succ)
//                      and three in (a -> b, pred -> s0, s_last -> succ), pred
//                      and succ read from rest.  Integers only, inside int32
//                      by the A9 guard: duration + delta is the re-evaluation;
//              H = 24  per wavefront one row T[q], the arrival time at
//                      position q of the padded tour.  A candidate is walked
//                      from its first changed position with the clock T has
//                      there, and stops early once it is past the last changed
//                      position with its clock equal to T's: the remaining
//                      edges are then the current tour's, so the end is too.
//            The (key, lane) minimum of the wave is the least (key, typ, i,
//            j).  A key below the tour's applies the move in place (an Or-opt
//            shifts by chunks of 64 positions, as a relocate does) and the
//            next round follows; otherwise the tour is a local optimum.  After
//            `rounds` applied moves the descent stops unproven and counts as
//            capped.  n < 2 has no moves;
//   answer   the least (key, s) over the S end tours: each wave keeps its own,
//            and after the kernel's one barrier past staging the wave that
//            holds the least writes the tour, its key, its unclamped duration,
//            s and the capped count.
//
// The counters carry no request row: an answer does not depend on the launch
// the request rode in or on its row in it.  With moves = 7 the tour, s and the
// capped count are vrpms_vrp_batch_ls's at K = 1, zero demands, any capacity
// >= 0, vehicle start = the start time and objective sum; only the key's
// secondary field differs (0 here, the duration there).
// tsp_batch_lso_spread.hip computes the same rows with G workgroups a request;
// what the two share lives in tsp_batch_lso.hpp.
//
// LDS, every part as the kernel carves it (vrpms_tsp_batch_lso_lds):
//   align16(H N N (wide ? 4 : 2))            the matrix
// + 4 * (H == 1 ? 2 : 1) * 4 align4(n + 2)   4 waves x the rows F, B (H = 1) or T (H = 24), int32
// + 4 * 2 align8(n + 2)                      4 waves x the current tour, uint16, node 0 at both ends
// + 4 * 2 align8(n)                          4 waves x the best end tour, uint16
// + 4 * 16                                   the waves' best key, best s, capped count
#include <hip/hip_runtime.h>

#include <string>

#include "batch_ls.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "staging.hpp"
#include "tour.hpp"
#include "tsp_batch_lso.hpp"

namespace vrpms {

inline size_t batch_lso_lds(int N, int H, int wide) {
  // behind the shared parts: 4 waves' best end tours of align8(n) uint16, then [4] BatchLsWave
  return batch_lso_shared_bytes(N, H, wide) + 4 * batch_align<size_t>((size_t)N - 1, 8) * 2 +
         4 * sizeof(BatchLsWave);
}

template <typename MatT, int HM>
__global__ __launch_bounds__(256) void tsp_batch_lso_kernel(TspBatchLsoArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char batch_lso_lds_mem[];
  const int N = a.N, n = N - 1;
  const int64_t r = blockIdx.x;
  const uint32_t cells = (uint32_t)HM * (uint32_t)N * (uint32_t)N;
  const uint32_t mat_bytes = (cells * (uint32_t)sizeof(MatT) + 15u) & ~15u;
  constexpr uint32_t kRows = HM == 1 ? 2u : 1u;
  const uint32_t row_words = ((uint32_t)n + 2u + 3u) & ~3u;
  const uint32_t cpad = ((uint32_t)n + 2u + 7u) & ~7u, bpad = ((uint32_t)n + 7u) & ~7u;
  MatT* M = reinterpret_cast<MatT*>(batch_lso_lds_mem);
  int32_t* rows = reinterpret_cast<int32_t*>(batch_lso_lds_mem + mat_bytes);   // [4][kRows][row_words]
  uint16_t* curs = reinterpret_cast<uint16_t*>(rows + 4 * kRows * row_words);   // [4][cpad]
  uint16_t* bests = curs + 4 * cpad;                                            // [4][bpad]
  BatchLsWave* wst = reinterpret_cast<BatchLsWave*>(bests + 4 * bpad);          // [4]

  // stage and check the matrix as batch_stage_request does; the verdict goes
  // through a word of the waves' records, free until the descents end
  uint16_t* gtour = a.tours + r * n;
  if (lso_stage(a.mats, r, cells, M, reinterpret_cast<uint32_t*>(wst))) {
    lso_refuse(a, r, n);
    return;
  }

  const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
  int32_t* F = rows + wave * kRows * row_words;   // H = 24: the arrival row T
  int32_t* B = F + (kRows - 1) * row_words;       // H = 1 only
  uint16_t* P = curs + wave * cpad;               // the current tour, node 0 at both ends
  uint16_t* A = P + 1;
  uint16_t* Best = bests + wave * bpad;           // the wave's best end tour
  const MatView<MatT, HM> D{M, (uint32_t)N, (uint32_t)N * (uint32_t)N, HM};
  const int t0 = a.start[r];
  const uint32_t mask = a.moves;

  const BatchLsShare sh = lso_share(n, mask, lane);   // the lane's share of a round
  if (lane == 0) {
    P[0] = 0;
    P[n + 1] = 0;
  }

  auto measure = [&]() -> int {
    if constexpr (HM == 1) return lso_rows_static(D, P, n, F, B, lane);
    else return lso_row_clock(D, P, n, t0, F, lane);
  };

  uint64_t bk = ~0ull;
  int bs = 0x7fffffff, bd = 0, capped = 0;
  for (int s = wave; s < a.S; s += 4) {
    batch_ls_shuffle(A, n, s, a.seed_lo, a.seed_hi, lane);
    int dur = measure();
    uint64_t ck = pack_key(0, (uint32_t)dur, 0);
    if (n >= 2) {
      for (int applied = 0;; ++applied) {
        if (applied >= a.rounds) {   // stopped unproven
          ++capped;
          break;
        }
        Move m = sh.m0, lm = sh.m0;
        uint64_t lk = ~0ull;
        for (int c = 0; c < sh.cnt; ++c) {
          int cd;
          if constexpr (HM == 1) cd = dur + lso_delta_static(D, P, F, B, n, m);
          else cd = lso_walk_clock(D, P, F, n, m);
          const uint64_t k = pack_key(0, (uint32_t)cd, 0);
          if (k < lk) {
            lk = k;
            lm = m;
          }
          lso_next(m, n, mask);
        }
        // the lanes hold ascending id ranges: the lowest lane among equal keys
        // holds the least (typ, i, j)
        int bl;
        const uint64_t k = wave_argmin_lane(lk, bl);
        if (!(k < ck)) break;   // a local optimum
        Move mb;
        mb.typ = (uint32_t)wave_bcast((int)lm.typ, bl);
        mb.i = wave_bcast(lm.i, bl);
        mb.j = wave_bcast(lm.j, bl);
        lso_apply(A, mb, lane);
        dur = measure();
        ck = pack_key(0, (uint32_t)dur, 0);
      }
    }
    if (ck < bk) {   // s rises: the least s among equal keys stays
      bk = ck;
      bs = s;
      bd = dur;
      for (int q = lane; q < n; q += 64) Best[q] = A[q];
      wave_sync();
    }
  }
  if (lane == 0) wst[wave] = BatchLsWave{bk, bs, capped};
  __syncthreads();
  int ncap;
  const int bw = batch_ls_winner(wst, ncap);
  if (wave != bw) return;
  for (int q = lane; q < n; q += 64) gtour[q] = Best[q];
  if (lane == 0) {
    a.keys[r] = bk;
    a.durs[r] = bd;
    a.info[2 * r] = bs;
    a.info[2 * r + 1] = ncap;
  }
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_tsp_batch_lso_lds(int32_t N, int32_t H, int32_t wide, uint64_t* bytes) {
  const char* who = "vrpms_tsp_batch_lso_lds";
  if (const int rc = batch_check_bytes(who, bytes)) return rc;
  if (const int rc = batch_lso_check(who, N, H, wide)) return rc;
  *bytes = batch_lso_lds(N, H, wide);
  return VRPMS_OK;
}

extern "C" int vrpms_tsp_batch_lso(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_start,
                                   int32_t R, int32_t N, int32_t H, int32_t wide, int32_t S,
                                   int32_t rounds, int32_t moves, uint64_t seed, uint16_t* d_tours,
                                   uint64_t* d_keys, int32_t* d_durs, int32_t* d_info, void* stream) {
  const char* who = "vrpms_tsp_batch_lso";
  if (const int rc = batch_check_ctx(who, ctx, R)) return rc;
  if (const int rc = batch_lso_check(who, N, H, wide)) return rc;
  if (const int rc = batch_lso_check_search(who, S, rounds, moves)) return rc;
  if (R == 0) return VRPMS_OK;
  if (const int rc = batch_check_buffers(who, "matrix/start/tour/key/duration/info",
                                         {d_mats, d_start, d_tours, d_keys, d_durs, d_info}))
    return rc;
  const size_t lds = batch_lso_lds(N, H, wide);
  if (lds > ctx->max_lds) return batch_lds_refusal(who, N, -1, H, wide, "", lds, ctx->max_lds);
  VRPMS_HIP(hipSetDevice(ctx->device));
  const TspBatchLsoArgs a{d_mats, d_start, R, N, S, rounds, (uint32_t)moves, (uint32_t)seed,
                          (uint32_t)(seed >> 32), d_tours, d_keys, d_durs, d_info};
  const char* what = "";
  const hipError_t e = batch_with_matrix(wide, H, [&](auto m, auto hm) {
    return batch_launch_blocks(tsp_batch_lso_kernel<decltype(m), decltype(hm)::value>, a, (unsigned)R, lds,
                               (hipStream_t)stream, &what);
  });
  if (e != hipSuccess) return hip_fail(e, what);
  return VRPMS_OK;
}
