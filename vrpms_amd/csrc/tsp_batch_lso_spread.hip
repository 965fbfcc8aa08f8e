// A second mapping of the TSP local search with Or-opt and delta pricing
// (DESIGN.md §2 A27, §4.3t): the starts, the rounds, the move order, the tie
// rules and the answer are tsp_batch_lso.hip's, bit for bit -- the descent of
// start s depends on (request, seed, s, rounds, moves) alone and the answer is
// the least (key, s) over the end tours -- but a request's S starts are spread
// over G workgroups, and a workgroup's 256 threads price one round of ONE tour
// instead of four wavefronts descending four starts.  For a lone request, or a
// few, that puts R G workgroups on the device instead of R.
//
//   descents   tsp_batch_lso_spread_kernel, grid R x G, 256 threads.  Workgroup
//              g of request r stages the matrix into LDS (lso_stage, the entry
//              check with it) and descends the starts g, g + G, ... one after
//              the other.  Every wavefront builds the start in its own padded
//              tour and fills its own rows (F and B at H = 1, T at H = 24) --
//              the shuffle and the rows are deterministic, so the four copies
//              are equal with no barrier -- and lso_descend_wg
//              (tsp_batch_lso.hpp) runs the rounds: thread t prices the enabled
//              ids [t per, (t + 1) per), per = ceil(total / 256), by
//              lso_delta_static or lso_walk_clock, the four wavefronts' least
//              records meet in LDS behind the round's one barrier, and each
//              wavefront applies the winning move to its own copy and rebuilds
//              its rows.  Whenever an end tour's key is below the workgroup's
//              best, wavefront 0 writes it to the workgroup's record of the
//              workspace; after the last start thread 0 writes the record's
//              header in front of it.  A workgroup whose request fails the
//              entry check writes a header marked `refused` and nothing else.
//   selection  tsp_batch_lso_select_kernel, the next launch on the stream, one
//              workgroup per request and no LDS: a marked record 0 gives
//              tsp_batch_lso's refusal row; otherwise it takes the least (key,
//              s) of the G records and the sum of their capped counts and
//              writes tours, keys, durs and info as tsp_batch_lso_kernel does.
//
// The kernel boundary orders the records; there is no counter of arrived
// workgroups and no hand-off inside a kernel.
//
// Workspace: R G records of 24 + 2 align8(n) bytes, n = N - 1: uint64 key,
// int32 s, int32 capped count, int32 unclamped duration, int32 refused, then n
// uint16 customers (vrpms_tsp_batch_lso_spread_work).
//
// LDS of the descents (vrpms_tsp_batch_lso_spread_lds), never more than
// vrpms_tsp_batch_lso_lds of the same shape, as a best tour has at least 8
// padded customers:
//   align16(H N N (wide ? 4 : 2))            the matrix
// + 4 * (H == 1 ? 2 : 1) * 4 align4(n + 2)   4 wavefronts x the rows F, B (H = 1) or T (H = 24), int32
// + 4 * 2 align8(n + 2)                      4 wavefronts x the current tour, uint16, node 0 at both ends
// + 2 * 4 * 16                               the wavefronts' round records, by barrier parity
// (the best end tour lives in the workspace, not in LDS).
#include <hip/hip_runtime.h>

#include <string>

#include "batch_ls.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "staging.hpp"
#include "tour.hpp"
#include "tsp_batch_lso.hpp"

namespace vrpms {

struct LsoSpreadHead {   // 24 bytes, in front of a record's tour
  uint64_t key;
  int32_t s, capped, dur, refused;
};

struct TspBatchLsoSpreadArgs {
  TspBatchLsoArgs a;
  int G;                  // workgroups per request, 1 <= G <= S
  unsigned char* work;    // [R][G] records of rec_bytes
  uint32_t rec_bytes;     // 24 + 2 align8(n)
};

inline size_t batch_lso_spread_lds(int N, int H, int wide) {
  return batch_lso_shared_bytes(N, H, wide) + kBatchLsoSpreadOwnBytes;
}

inline uint64_t batch_lso_spread_rec_bytes(int N) {
  return sizeof(LsoSpreadHead) + 2 * batch_align<uint64_t>((uint64_t)N - 1, 8);
}

template <typename MatT, int HM>
__global__ __launch_bounds__(256) void tsp_batch_lso_spread_kernel(TspBatchLsoSpreadArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char batch_lso_spread_lds_mem[];
  const TspBatchLsoArgs& a = p.a;
  const int N = a.N, n = N - 1, G = p.G;
  const int64_t r = blockIdx.x / (uint32_t)G;
  const int g = (int)(blockIdx.x % (uint32_t)G);
  const LsoCarve<MatT, HM> c(batch_lso_spread_lds_mem, N);
  BatchLsRec* rec = reinterpret_cast<BatchLsRec*>(c.rest);   // [2][4]

  unsigned char* mine = p.work + (r * G + g) * (int64_t)p.rec_bytes;
  LsoSpreadHead* head = reinterpret_cast<LsoSpreadHead*>(mine);
  uint16_t* wtour = reinterpret_cast<uint16_t*>(mine + sizeof(LsoSpreadHead));

  // stage and check the matrix; the selection kernel writes the refusal row.
  // The verdict goes through a word of the round records, free until then
  if (lso_stage(a.mats, r, c.cells, c.M, reinterpret_cast<uint32_t*>(rec))) {
    if (threadIdx.x == 0) *head = LsoSpreadHead{~0ull, -1, 0, 0, 1};
    return;
  }

  const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
  int32_t *F = c.F(wave), *B = c.B(wave);
  uint16_t* P = c.P(wave);                        // the wavefront's copy of the current tour
  uint16_t* A = P + 1;
  const MatView<MatT, HM> D{c.M, (uint32_t)N, (uint32_t)N * (uint32_t)N, HM};
  const int t0 = a.start[r];
  const uint32_t mask = a.moves;

  const BatchLsShare sh = lso_share_wg(n, mask, (int)threadIdx.x);   // the thread's share of a round
  if (lane == 0) {
    P[0] = 0;
    P[n + 1] = 0;
  }

  uint64_t bk = ~0ull;
  int bs = 0x7fffffff, bd = 0, capped = 0, parity = 0;
  for (int s = g; s < a.S; s += G) {
    batch_ls_shuffle(A, n, s, a.seed_lo, a.seed_hi, lane);
    int dur = lso_measure<HM>(D, P, n, t0, F, B, lane);
    if (n >= 2)
      dur = lso_descend_wg<HM>(D, P, F, B, n, t0, mask, dur, a.rounds, sh, wave, lane, rec, parity, capped);
    const uint64_t ck = pack_key(0, (uint32_t)dur, 0);
    if (ck < bk) {   // s rises: the least s among equal keys stays
      bk = ck;
      bs = s;
      bd = dur;
      if (wave == 0)
        for (int q = lane; q < n; q += 64) wtour[q] = A[q];
    }
  }
  if (threadIdx.x == 0) *head = LsoSpreadHead{bk, bs, capped, bd, 0};
}

__global__ __launch_bounds__(256) void tsp_batch_lso_select_kernel(TspBatchLsoSpreadArgs p) {
  const TspBatchLsoArgs& a = p.a;
  const int n = a.N - 1, G = p.G;
  const int64_t r = blockIdx.x;
  const unsigned char* recs = p.work + r * G * (int64_t)p.rec_bytes;
  auto head = [&](int g) {
    return *reinterpret_cast<const LsoSpreadHead*>(recs + (int64_t)g * p.rec_bytes);
  };
  if (head(0).refused) {   // every workgroup of the request saw the same matrix
    lso_refuse(a, r, n);
    return;
  }

  // the least (key, s) of the request's G records and the sum of their capped
  // counts, in every wavefront alike: lane l takes the records l, l + 64, ...
  const int lane = lane_id();
  uint64_t bk = ~0ull, bs = 0x7fffffffu;
  int ncap = 0;
  for (int g = lane; g < G; g += 64) {
    const LsoSpreadHead h = head(g);
    if (h.key < bk || (h.key == bk && (uint64_t)(uint32_t)h.s < bs)) {
      bk = h.key;
      bs = (uint32_t)h.s;
    }
    ncap += h.capped;
  }
  wave_argmin(bk, bs);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ncap += __shfl_xor(ncap, off, kWave);
  const int s = __builtin_amdgcn_readfirstlane((int)(uint32_t)bs);
  const int bg = (int)((uint32_t)s % (uint32_t)G);   // workgroup g descended the starts g mod G

  const uint16_t* wtour =
      reinterpret_cast<const uint16_t*>(recs + (int64_t)bg * p.rec_bytes + sizeof(LsoSpreadHead));
  uint16_t* gtour = a.tours + r * n;
  for (int q = threadIdx.x; q < n; q += 256) gtour[q] = wtour[q];
  if (threadIdx.x == 0) {
    const LsoSpreadHead h = head(bg);
    a.keys[r] = h.key;
    a.durs[r] = h.dur;
    a.info[2 * r] = s;
    a.info[2 * r + 1] = ncap;
  }
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_tsp_batch_lso_spread_lds(int32_t N, int32_t H, int32_t wide, uint64_t* bytes) {
  const char* who = "vrpms_tsp_batch_lso_spread_lds";
  if (const int rc = batch_check_bytes(who, bytes)) return rc;
  if (const int rc = batch_lso_check(who, N, H, wide)) return rc;
  *bytes = batch_lso_spread_lds(N, H, wide);
  return VRPMS_OK;
}

extern "C" int vrpms_tsp_batch_lso_spread_work(int32_t R, int32_t N, int32_t G, uint64_t* bytes) {
  const char* who = "vrpms_tsp_batch_lso_spread_work";
  if (const int rc = batch_check_bytes(who, bytes)) return rc;
  if (const int rc = batch_check_R(who, R)) return rc;
  if (const int rc = batch_lso_check(who, N, 1, 0)) return rc;
  return batch_work_bytes(who, R, G, batch_lso_spread_rec_bytes(N), bytes);
}

extern "C" int vrpms_tsp_batch_lso_spread(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_start,
                                          int32_t R, int32_t N, int32_t H, int32_t wide, int32_t S,
                                          int32_t rounds, int32_t moves, uint64_t seed, int32_t G,
                                          void* d_work, uint64_t work_bytes, uint16_t* d_tours,
                                          uint64_t* d_keys, int32_t* d_durs, int32_t* d_info,
                                          void* stream) {
  const char* who = "vrpms_tsp_batch_lso_spread";
  if (const int rc = batch_check_ctx(who, ctx, R)) return rc;
  if (const int rc = batch_lso_check(who, N, H, wide)) return rc;
  if (const int rc = batch_lso_check_search(who, S, rounds, moves)) return rc;
  if (const int rc = batch_check_count(who, "G", G, kBatchMaxG)) return rc;
  if (R == 0) return VRPMS_OK;
  if (const int rc = batch_check_buffers(who, "matrix/start/tour/key/duration/info",
                                         {d_mats, d_start, d_tours, d_keys, d_durs, d_info}))
    return rc;
  const int Gc = G < S ? G : S;   // a workgroup without a start cannot occur
  const uint64_t rec = batch_lso_spread_rec_bytes(N);
  if (const int rc = batch_check_work(who, R, Gc, rec, d_work, work_bytes)) return rc;
  const size_t lds = batch_lso_spread_lds(N, H, wide);
  if (lds > ctx->max_lds) return batch_lds_refusal(who, N, -1, H, wide, "", lds, ctx->max_lds);
  VRPMS_HIP(hipSetDevice(ctx->device));
  const TspBatchLsoSpreadArgs p{
      TspBatchLsoArgs{d_mats, d_start, R, N, S, rounds, (uint32_t)moves, (uint32_t)seed,
                      (uint32_t)(seed >> 32), d_tours, d_keys, d_durs, d_info},
      Gc, static_cast<unsigned char*>(d_work), (uint32_t)rec};
  const hipStream_t s = (hipStream_t)stream;
  const char* what = "";
  hipError_t e = batch_with_matrix(wide, H, [&](auto m, auto hm) {
    return batch_launch_blocks(tsp_batch_lso_spread_kernel<decltype(m), decltype(hm)::value>, p,
                               (unsigned)((uint64_t)R * (uint64_t)Gc), lds, s, &what);
  });
  if (e == hipSuccess) e = batch_enqueue(tsp_batch_lso_select_kernel, p, (unsigned)R, 0, s, &what);
  if (e != hipSuccess) return hip_fail(e, what);
  return VRPMS_OK;
}
