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

constexpr int kBatchLsoMaxN = 65535;   // genes are uint16
constexpr int kBatchLsoMaxS = 65535;

struct TspBatchLsoArgs {
  const int32_t* mats;    // [R][H][N][N]
  const int32_t* start;   // [R]
  int R, N, S, rounds;
  uint32_t moves, seed_lo, seed_hi;
  uint16_t* tours;        // [R][n]
  uint64_t* keys;         // [R]
  int32_t* durs;          // [R]
  int32_t* info;          // [R][2]: the answer's start, the capped descents
};

struct BatchLsoLds {
  size_t mat, row, cur, best, total;   // bytes of the matrix, one int32 row, one padded tour, one tour
};

inline BatchLsoLds batch_lso_lds(int N, int H, int wide) {
  BatchLsoLds l;
  const size_t n = (size_t)N - 1;
  l.mat = ((size_t)H * N * N * (wide ? 4 : 2) + 15) & ~(size_t)15;
  l.row = ((n + 2 + 3) & ~(size_t)3) * 4;
  l.cur = ((n + 2 + 7) & ~(size_t)7) * 2;
  l.best = ((n + 7) & ~(size_t)7) * 2;
  l.total = l.mat + 4 * ((H == 1 ? 2 : 1) * l.row + l.cur + l.best) + 4 * 16;
  return l;
}

// duration of the padded tour P (node 0 at P[0] and P[n + 1]) on a static
// matrix, with the rows F and B filled on the way: 64 edges a step, the
// forward edge in the low and the backward edge in the high half of one scan
template <typename Mat>
VRPMS_DEV int lso_rows_static(const Mat& D, const uint16_t* P, int n, int32_t* F, int32_t* B,
                              int lane) {
  uint32_t cf = 0, cb = 0;
  if (lane == 0) {
    F[0] = 0;
    B[0] = 0;
  }
  for (int base = 1; base <= n + 1; base += 64) {
    const int q = base + lane;
    uint64_t v = 0;
    if (q <= n + 1) {
      const uint32_t x = P[q - 1], y = P[q];
      v = ((uint64_t)(uint32_t)D(0, y, x) << 32) | (uint32_t)D(0, x, y);
    }
    const uint64_t tot = wave_scan_add_u64(v);
    if (q <= n + 1) {
      F[q] = (int32_t)(cf + (uint32_t)v);
      B[q] = (int32_t)(cb + (uint32_t)(v >> 32));
    }
    cf += (uint32_t)tot;
    cb += (uint32_t)(tot >> 32);
  }
  wave_sync();
  return (int)cf;
}

// duration of the padded tour P from time t0 on the clock, with the arrival
// row T filled on the way: every lane walks alike, lane 0 writes
template <typename Mat>
VRPMS_DEV int lso_row_clock(const Mat& D, const uint16_t* P, int n, int t0, int32_t* T, int lane) {
  int t = t0;
  uint32_t prev = 0;
  if (lane == 0) T[0] = t;
  for (int q = 1; q <= n + 1; ++q) {
    const uint32_t c = P[q];
    t += D(t, prev, c);
    prev = c;
    if (lane == 0) T[q] = t;
  }
  wave_sync();
  return t - t0;
}

// exact duration change of the static closed tour under move m; P is the
// padded tour (P[q + 1] = position q), F and B its prefix rows
template <typename Mat>
VRPMS_DEV int lso_delta_static(const Mat& D, const uint16_t* P, const int32_t* F, const int32_t* B,
                               int n, const Move& m) {
  auto d = [&](uint32_t a, uint32_t b) { return D(0, a, b); };
  const int i = m.i, j = m.j;
  if (m.typ == kMove2Opt) {
    const uint32_t a = P[i], pi = P[i + 1], pj = P[j + 1], b = P[j + 2];
    return d(a, pj) + d(pi, b) - d(a, pi) - d(pj, b) + (B[j + 1] - B[i + 1]) - (F[j + 1] - F[i + 1]);
  }
  if (m.typ <= kMoveRelocate)
    return tsp_move_delta(d, [&](int q) { return (uint32_t)P[q + 1]; }, n, m, true);
  const int sl = (int)m.typ - 1;
  const uint32_t a = P[i], s0 = P[i + 1], s1 = P[i + sl], b = P[i + sl + 1];
  // rest's padded position x is P[x] up to i and P[x + m] past it
  const uint32_t pred = P[j <= i ? j : j + sl], succ = P[j + 1 <= i ? j + 1 : j + 1 + sl];
  return d(a, b) + d(pred, s0) + d(s1, succ) - d(a, s0) - d(s1, b) - d(pred, succ);
}

// duration of the moved tour on the clock: the walk from the move's first
// changed position with T's clock there
template <typename Mat>
VRPMS_DEV int lso_walk_clock(const Mat& D, const uint16_t* P, const int32_t* T, int n, const Move& m) {
  const LsoMap mm = lso_map(m);
  const int f = lso_first(m), l = lso_last(m);
  int t = T[f];
  uint32_t prev = P[f];
  for (int q = f; q < n; ++q) {
    const uint32_t c = P[lso_src(mm, q) + 1];
    t += D(t, prev, c);
    prev = c;
    if (q > l && t == T[q + 1]) return T[n + 1] - T[0];   // the rest is the current tour's
  }
  t += D(t, prev, 0);
  return t - T[0];
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
  {
    uint32_t* flag = reinterpret_cast<uint32_t*>(wst);
    const int32_t* src = a.mats + r * (int64_t)cells;
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    bool bad = false;
    for (uint32_t i = threadIdx.x; i < cells; i += 256) {
      const int32_t v = src[i];
      bad |= v < 0 || (sizeof(MatT) == 2 && v > 65535);
      M[i] = (MatT)v;
    }
    if (bad) *flag = 1;
    __syncthreads();
    bad = *flag != 0;
    __syncthreads();   // every wavefront has read the word before anything replaces it
    if (bad) {         // the refusal row
      for (int q = threadIdx.x; q < n; q += 256) gtour[q] = 0;
      if (threadIdx.x == 0) {
        a.keys[r] = ~0ull;
        a.durs[r] = 0;
        a.info[2 * r] = -1;
        a.info[2 * r + 1] = 0;
      }
      return;
    }
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

// the shape checks both entry points share; 0 or the refusal's code
static int batch_lso_check(const char* who, int32_t N, int32_t H, int32_t wide) {
  const std::string w(who);
  if (N < 2 || N > kBatchLsoMaxN)
    return fail(VRPMS_EINVAL, w + ": needs 2 <= N <= 65535 (" + std::to_string(N) + " given)");
  if (H != 1 && H != 24)
    return fail(VRPMS_EINVAL, w + ": H must be 1 or 24 (" + std::to_string(H) + " given)");
  if (wide != 0 && wide != 1)
    return fail(VRPMS_EINVAL, w + ": wide must be 0 (uint16 matrix) or 1 (int32) (" + std::to_string(wide) +
                                  " given)");
  return VRPMS_OK;
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_tsp_batch_lso_lds(int32_t N, int32_t H, int32_t wide, uint64_t* bytes) {
  if (!bytes) return fail(VRPMS_EINVAL, "vrpms_tsp_batch_lso_lds: bytes is NULL");
  const int rc = batch_lso_check("vrpms_tsp_batch_lso_lds", N, H, wide);
  if (rc) return rc;
  *bytes = batch_lso_lds(N, H, wide).total;
  return VRPMS_OK;
}

extern "C" int vrpms_tsp_batch_lso(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_start,
                                   int32_t R, int32_t N, int32_t H, int32_t wide, int32_t S,
                                   int32_t rounds, int32_t moves, uint64_t seed, uint16_t* d_tours,
                                   uint64_t* d_keys, int32_t* d_durs, int32_t* d_info, void* stream) {
  if (!ctx) return fail(VRPMS_EINVAL, "vrpms_tsp_batch_lso: ctx is NULL");
  if (R < 0) return fail(VRPMS_EINVAL, "vrpms_tsp_batch_lso: R must not be negative");
  const int rc = batch_lso_check("vrpms_tsp_batch_lso", N, H, wide);
  if (rc) return rc;
  if (S < 1 || S > kBatchLsoMaxS)
    return fail(VRPMS_EINVAL, "vrpms_tsp_batch_lso: 1 <= S <= 65535 (" + std::to_string(S) + " given)");
  if (rounds < 0)
    return fail(VRPMS_EINVAL,
                "vrpms_tsp_batch_lso: rounds must not be negative (" + std::to_string(rounds) + " given)");
  if (moves < 1 || moves > 31)
    return fail(VRPMS_EINVAL, "vrpms_tsp_batch_lso: 1 <= moves <= 31, bit t enabling move type t (" +
                                  std::to_string(moves) + " given)");
  if (R == 0) return VRPMS_OK;
  if (!d_mats || !d_start || !d_tours || !d_keys || !d_durs || !d_info)
    return fail(VRPMS_EINVAL, "vrpms_tsp_batch_lso: NULL matrix/start/tour/key/duration/info buffer");
  const size_t lds = batch_lso_lds(N, H, wide).total;
  if (lds > ctx->max_lds)
    return fail(VRPMS_EINVAL, "vrpms_tsp_batch_lso: a request of N = " + std::to_string(N) + ", H = " +
                                  std::to_string(H) + (wide ? " (int32 matrix)" : " (uint16 matrix)") +
                                  " needs " + std::to_string(lds) + " bytes of LDS (" +
                                  std::to_string(ctx->max_lds) + " available)");
  VRPMS_HIP(hipSetDevice(ctx->device));
  const TspBatchLsoArgs a{d_mats, d_start, R, N, S, rounds, (uint32_t)moves, (uint32_t)seed,
                          (uint32_t)(seed >> 32), d_tours, d_keys, d_durs, d_info};
  void (*kernel)(TspBatchLsoArgs) =
      wide ? (H == 24 ? tsp_batch_lso_kernel<int32_t, 24> : tsp_batch_lso_kernel<int32_t, 1>)
           : (H == 24 ? tsp_batch_lso_kernel<uint16_t, 24> : tsp_batch_lso_kernel<uint16_t, 1>);
  if (lds > 65536)
    VRPMS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kernel<<<(unsigned)R, 256, lds, (hipStream_t)stream>>>(a);
  VRPMS_HIP(hipGetLastError());
  return VRPMS_OK;
}
