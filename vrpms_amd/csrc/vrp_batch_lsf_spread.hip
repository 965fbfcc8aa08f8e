// A second mapping of the delta-priced local search over plain separator tours
// (DESIGN.md §2 A28, §4.3v, §4.3x): the starts, the rounds, the pricing and the
// answer are vrp_batch_lsf.hip's, bit for bit -- the descent of start s depends
// on (request, seed, s, rounds, objective) alone and the answer is the least
// (key, s) over the end tours -- but a request's S starts are spread over G
// workgroups, and a workgroup's 256 threads price one round of ONE tour instead
// of four wavefronts descending four starts.  For a lone request, or a few,
// that puts R G workgroups on the device instead of R.
//
//   descents   vrp_batch_lsf_spread_kernel, grid R x G, 256 threads.  Workgroup
//              g of request r stages the request into LDS (batch_stage.hpp),
//              every wavefront zeroes the matrix cell 0 -> 0, and the workgroup
//              descends the starts g, g + G, ... one after the other.  Every
//              wavefront builds the start in its own padded tour, keys it with
//              one walk and fills its own rows (lsf_rows, lsf_plain) -- all of
//              it deterministic, so the four copies are equal with no barrier.
//              A start that is not plain does not descend and is never capped,
//              in all four wavefronts alike.  lsf_descend_wg
//              (vrp_batch_lsf.hpp) runs the rounds of a plain one: thread t
//              prices the ids [t per, (t + 1) per), per = ceil(2 L (L - 1) /
//              256), by lsf_price, the four wavefronts' least records meet in
//              LDS behind the round's one barrier, and each wavefront applies
//              the winning move to its own copy and rebuilds its rows.
//              Whenever an end tour's key is below the workgroup's best,
//              wavefront 0 writes it to the workgroup's record of the
//              workspace; after the last start thread 0 writes (key, s, capped
//              count) in front of it.
//   selection  vrp_batch_lsf_select_kernel, the next launch on the stream, one
//              workgroup per request: it stages the request again (the entry
//              check with it: a refusal row is vrp_batch_lsf's), takes the
//              least (key, s) of the G records and the sum of their capped
//              counts, walks that tour once more (batch_final_walk) and writes
//              tours, keys, durs, veh and info as vrp_batch_lsf_kernel does.
//              It is vrp_batch_lsr_select_kernel at H = 1 on this file's carve.
//
// The kernel boundary orders the records; there is no counter of arrived
// workgroups and no hand-off inside a kernel.
//
// Workspace: R G records of 16 + 2 align8(L) bytes: uint64 key, int32 s, int32
// capped count, L uint16 tokens (vrpms_vrp_batch_lsf_spread_work).
//
// LDS of either kernel (vrpms_vrp_batch_lsf_spread_lds), with L2 = L + 2; the
// kernels carve the round records first, right behind the instance:
//   align16(N N (wide ? 4 : 2))                   the matrix
// + 4 align4(N) + 2 * 4 align4(K)                 demand, capacities, start times (int32)
// + 4 * 4 (3 align4(L2) + 5 align4(K + 1))        4 wavefronts x int32 rows F, B, W and tables FD, BD, LD, PM, SM
// + 4 * 2 (align8(L2) + align8(K + 1))            4 wavefronts x uint16 current tour, S
// + 4 * align8(L2)                                4 wavefronts x the uint8 segment row G
// + 2 * 4 * 16                                    the wavefronts' round records, by barrier parity
// That is vrpms_vrp_batch_lsf_lds less the four best end tours (they live in
// the workspace) and the four wave records, plus the round records: 8 align8(L)
// - 64 >= 0 bytes fewer.  The selection uses the first 4 align8(L) bytes behind
// the instance for the answer and its vehicles.
#include <hip/hip_runtime.h>

#include <string>

#include "vrp_batch_lsf.hpp"

namespace vrpms {

struct VrpBatchLsfSpreadArgs {
  VrpBatchLsArgs a;
  int G;                  // workgroups per request, 1 <= G <= S
  unsigned char* work;    // [R][G] records of rec_bytes
  uint32_t rec_bytes;     // 16 + 2 align8(L)
};

inline uint64_t batch_lsf_spread_rec_bytes(int N, int K) {
  return sizeof(BatchLsWave) + 2 * batch_align<uint64_t>((uint64_t)N - 1 + K - 1, 8);
}

template <typename MatT>
__global__ __launch_bounds__(256) void vrp_batch_lsf_spread_kernel(VrpBatchLsfSpreadArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char batch_lsf_spread_lds_mem[];
  const VrpBatchLsArgs& a = p.a;
  const int N = a.N, n = N - 1, K = a.K, L = n + K - 1, G = p.G;
  const int64_t r = blockIdx.x / (uint32_t)G;
  const int g = (int)(blockIdx.x % (uint32_t)G);
  const BatchInst<MatT, 1> in(batch_lsf_spread_lds_mem, BatchInst<MatT, 1>::parts(N, K), N, K);
  const BatchLsfSpreadParts<uint32_t> lp((uint32_t)L, (uint32_t)K);
  BatchLsRec* rec = reinterpret_cast<BatchLsRec*>(in.rest);                   // [2][4]
  int32_t* words = reinterpret_cast<int32_t*>(rec + 2 * 4);                   // [4][lp.words()]
  uint16_t* halves = reinterpret_cast<uint16_t*>(words + 4 * lp.words());     // [4][lp.halves()]
  uint8_t* bytes = reinterpret_cast<uint8_t*>(halves + 4 * lp.halves());      // [4][lp.gpad]

  // stage and check the request; the selection kernel writes the refusal row.
  // The verdict goes through a word of the round records, free until then
  if (batch_stage_request(a, r, in, rec)) return;

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
  rows.P = w16;                      // the wavefront's copy of the current tour, padded
  rows.S = w16 + lp.ppad;
  rows.G = bytes + wave * lp.gpad;
  uint16_t* A = rows.P + 1;
  const int32_t *dem = in.dem, *cap = in.cap;
  const MatView<MatT, 1> D{in.M, (uint32_t)N, (uint32_t)N * (uint32_t)N, 1};
  const SplitParams sp{dem, cap, in.start, K, a.objective};
  unsigned char* mine = p.work + (r * G + g) * (int64_t)p.rec_bytes;
  uint16_t* wtour = reinterpret_cast<uint16_t*>(mine + sizeof(BatchLsWave));

  // the staging check has seen the cell 0 -> 0; from here on a separator is
  // the depot at no cost.  Every wave writes the same zero before it reads.
  if (lane == 0) {
    in.M[0] = 0;
    rows.P[0] = 0;
    rows.P[L + 1] = 0;
  }
  wave_sync();

  const BatchLsShare sh = batch_ls_share_wg(L, (int)threadIdx.x);   // the thread's share of a round

  uint64_t bk = ~0ull;
  int bs = 0x7fffffff, capped = 0, parity = 0;
  for (int s = g; s < a.S; s += G) {
    batch_lsr_start(A, dem, cap, n, K, s, a.seed_lo, a.seed_hi, lane);
    uint64_t ck = readlane_u64(eval_tour<true>(D, sp, [&](int q) { return (uint32_t)A[q]; }, L).key, 0);
    if (L >= 2) {
      int dmax;
      const int sum = lsf_rows(D, dem, rows, L, K, lane, dmax);
      // the four copies of the start are equal, so the four verdicts are: all
      // wavefronts enter the descent and its barriers, or none does
      if (lsf_plain(dem, cap, rows, K, lane))
        ck = lsf_descend_wg(D, dem, cap, rows, L, K, ck, sum, dmax, a.objective, a.rounds, sh, wave, lane,
                            rec, parity, capped);
    }
    if (ck < bk) {   // s rises: the least s among equal keys stays
      bk = ck;
      bs = s;
      if (wave == 0)
        for (int q = lane; q < L; q += 64) wtour[q] = A[q];
    }
  }
  if (threadIdx.x == 0) *reinterpret_cast<BatchLsWave*>(mine) = BatchLsWave{bk, bs, capped};
}

template <typename MatT>
__global__ __launch_bounds__(256) void vrp_batch_lsf_select_kernel(VrpBatchLsfSpreadArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char batch_lsf_select_lds_mem[];
  const VrpBatchLsArgs& a = p.a;
  const int N = a.N, n = N - 1, K = a.K, L = n + K - 1, G = p.G;
  const int64_t r = blockIdx.x;
  const BatchInst<MatT, 1> in(batch_lsf_select_lds_mem, BatchInst<MatT, 1>::parts(N, K), N, K);

  uint16_t* gtour = a.tours + r * L;
  int8_t* gveh = a.veh + r * L;
  int32_t* gdurs = a.durs + r * K;
  if (batch_stage_request(a, r, in, in.rest)) {
    batch_refuse(gtour, gveh, gdurs, a.keys + r, L, K);
    if (threadIdx.x == 0) {
      a.info[2 * r] = -1;
      a.info[2 * r + 1] = 0;
    }
    return;
  }
  if (threadIdx.x >= 64) return;   // one wavefront selects and walks

  // the least (key, s) of the request's G records and the sum of their capped
  // counts: lane l takes the records l, l + 64, ...
  const int lane = lane_id();
  const unsigned char* recs = p.work + r * G * (int64_t)p.rec_bytes;
  uint64_t bk = ~0ull, bs = 0x7fffffffu;
  int ncap = 0;
  for (int g = lane; g < G; g += 64) {
    const BatchLsWave w = *reinterpret_cast<const BatchLsWave*>(recs + (int64_t)g * p.rec_bytes);
    if (w.key < bk || (w.key == bk && (uint64_t)(uint32_t)w.s < bs)) {
      bk = w.key;
      bs = (uint32_t)w.s;
    }
    ncap += w.capped;
  }
  wave_argmin(bk, bs);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ncap += __shfl_xor(ncap, off, kWave);
  bk = readlane_u64(bk, 0);
  const int s = __builtin_amdgcn_readfirstlane((int)(uint32_t)bs);
  const int bg = (int)((uint32_t)s % (uint32_t)G);   // workgroup g descended the starts g mod G

  // its tour into LDS, then once more as spec.eval_cvrp walks it: every lane
  // walks alike, lane k keeps route k's duration, lane 0 notes the vehicles
  const uint32_t tpad = batch_align<uint32_t>((uint32_t)L, 8);
  uint16_t* Best = reinterpret_cast<uint16_t*>(in.rest);
  int16_t* V = reinterpret_cast<int16_t*>(Best + tpad);
  const uint16_t* wtour =
      reinterpret_cast<const uint16_t*>(recs + (int64_t)bg * p.rec_bytes + sizeof(BatchLsWave));
  for (int q = lane; q < L; q += 64) Best[q] = wtour[q];
  wave_sync();
  const MatView<MatT, 1> D{in.M, (uint32_t)N, (uint32_t)N * (uint32_t)N, 1};
  const int mydur = batch_final_walk(D, in.dem, in.cap, in.start, K, n, Best, L, V, lane);
  wave_sync();
  for (int q = lane; q < L; q += 64) {
    gtour[q] = Best[q];
    gveh[q] = (int8_t)V[q];
  }
  if (lane < K) gdurs[lane] = mydur;
  if (lane == 0) {
    a.keys[r] = bk;
    a.info[2 * r] = s;
    a.info[2 * r + 1] = ncap;
  }
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_vrp_batch_lsf_spread_lds(int32_t N, int32_t K, int32_t wide, uint64_t* bytes) {
  const char* who = "vrpms_vrp_batch_lsf_spread_lds";
  if (const int rc = batch_check_bytes(who, bytes)) return rc;
  if (const int rc = batch_lsf_check(who, N, K, 1, wide)) return rc;
  *bytes = batch_lsf_spread_lds(N, K, wide);
  return VRPMS_OK;
}

extern "C" int vrpms_vrp_batch_lsf_spread_work(int32_t R, int32_t N, int32_t K, int32_t G,
                                               uint64_t* bytes) {
  const char* who = "vrpms_vrp_batch_lsf_spread_work";
  if (const int rc = batch_check_bytes(who, bytes)) return rc;
  if (const int rc = batch_check_R(who, R)) return rc;
  if (const int rc = batch_lsf_check(who, N, K, 1, 0)) return rc;
  return batch_work_bytes(who, R, G, batch_lsf_spread_rec_bytes(N, K), bytes);
}

extern "C" int vrpms_vrp_batch_lsf_spread(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                                          const int32_t* d_cap, const int32_t* d_start, int32_t R,
                                          int32_t N, int32_t K, int32_t H, int32_t objective,
                                          int32_t wide, int32_t S, int32_t rounds, uint64_t seed,
                                          int32_t G, void* d_work, uint64_t work_bytes,
                                          uint16_t* d_tours, uint64_t* d_keys, int32_t* d_durs,
                                          int8_t* d_veh, int32_t* d_info, void* stream) {
  const char* who = "vrpms_vrp_batch_lsf_spread";
  if (const int rc = batch_check_ctx(who, ctx, R)) return rc;
  if (const int rc = batch_lsf_check(who, N, K, H, wide)) return rc;
  if (const int rc = batch_ls_check_search(who, objective, S, rounds)) return rc;
  if (const int rc = batch_check_count(who, "G", G, kBatchMaxG)) return rc;
  if (R == 0) return VRPMS_OK;
  if (const int rc = batch_check_buffers(
          who, "matrix/demand/capacity/start/tour/key/duration/vehicle/info",
          {d_mats, d_demand, d_cap, d_start, d_tours, d_keys, d_durs, d_veh, d_info}))
    return rc;
  const int Gc = G < S ? G : S;   // a workgroup without a start cannot occur
  const uint64_t rec = batch_lsf_spread_rec_bytes(N, K);
  if (const int rc = batch_check_work(who, R, Gc, rec, d_work, work_bytes)) return rc;
  const size_t lds = batch_lsf_spread_lds(N, K, wide);
  if (lds > ctx->max_lds) return batch_lds_refusal(who, N, K, H, wide, "", lds, ctx->max_lds);
  VRPMS_HIP(hipSetDevice(ctx->device));
  const VrpBatchLsfSpreadArgs p{
      VrpBatchLsArgs{d_mats, d_demand, d_cap, d_start, R, N, K, H, objective, S, rounds, (uint32_t)seed,
                     (uint32_t)(seed >> 32), d_tours, d_keys, d_durs, d_veh, d_info},
      Gc, static_cast<unsigned char*>(d_work), (uint32_t)rec};
  const hipStream_t s = (hipStream_t)stream;
  const char* what = "";
  const hipError_t e = batch_with_matrix(wide, 1, [&](auto m, auto) {
    const auto descend = vrp_batch_lsf_spread_kernel<decltype(m)>;
    const auto select = vrp_batch_lsf_select_kernel<decltype(m)>;
    hipError_t x = batch_raise_lds(descend, lds, &what);   // both limits before either launch
    if (x == hipSuccess) x = batch_raise_lds(select, lds, &what);
    if (x == hipSuccess) x = batch_enqueue(descend, p, (unsigned)((uint64_t)R * (uint64_t)Gc), lds, s, &what);
    if (x == hipSuccess) x = batch_enqueue(select, p, (unsigned)R, lds, s, &what);
    return x;
  });
  if (e != hipSuccess) return hip_fail(e, what);
  return VRPMS_OK;
}
