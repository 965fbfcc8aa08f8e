// Throughput mode of the VRP genetic algorithm: R
// independent small-fleet CVRP requests of one (N, K, H, objective, P, G)
// share one launch, ONE WORKGROUP PER REQUEST.  The workgroup stages its
// request's whole instance into LDS exactly as vrp_batch_sa does
// (batch_stage.hpp: the [H][N][N] matrix as uint16, or int32 when `wide`, the
// demand, capacity and start-time rows; a negative entry, or one above 65535
// under wide = 0, ends the request with an all-ones key) and keeps a whole
// population there: 2P rows of n = N - 1 customers (no separators: the greedy
// split prices them), P of them parents and P children, by a slot -> row map
// (prow / crow, as ga_fused.hip), so a survivor is never copied and the next
// children go into the rows no survivor holds.
//
//   start   member i = the Philox Fisher-Yates shuffle of 1..n, counters
//           (0xffffffff, 0xffffffff, i, q), one lane per member; members keep
//           index order;
//   gen g   oracle.search.ga_generation on island 0 (blocks (g, 0, child,
//           0 / 1): two tournaments of two, OX1, a decode_move mutation iff
//           r2[2] < pmut, n < 2 copies parent A).  N <= 64: one lane per
//           child breeds it serially with the used genes as bits of one
//           64-bit register and prices it at once by eval_tour<true>.  N > 64:
//           wave w breeds children w, w + 4, ... by ga_breed_kernel's `used`
//           bitmap and ballot-prefix fill, then one lane per child prices it.
//           The P best of the 2P (key, index) pairs survive (block_sort_pairs
//           over M = the next power of two >= 2P pairs, padded with all-ones
//           keys);
//   answer  the least (key, slot) member; wave 0 walks it once more and writes
//           the K route durations and every gene's vehicle.
//
// The counters carry no request row: an answer does not depend on the launch
// the request rode in or on its row in it.
//
// LDS, every part as the kernel carves it (vrpms_vrp_batch_ga_lds), rs = the
// row stride in genes, 2 (ceil(n / 2) | 1) -- an odd number of words, so the
// lanes that walk one row each start in different banks:
//   align16(H N N (wide ? 4 : 2))            the matrix
// + 4 align4(N) + 2 * 4 align4(K)            demand, capacities, start times (int32)
// + 8 M + 4 M                                the sort pairs
// + 2 * 8 P                                  parent and child keys
// + 4 * 4 align4(ceil(N / 32))               the four wavefronts' `used` bitmaps
// + 2 P * 2 rs                               the rows
// + 2 * 2 P                                  prow, crow
#include <hip/hip_runtime.h>

#include <string>

#include "batch_launch.hpp"
#include "batch_stage.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "sort.hpp"
#include "staging.hpp"
#include "tour.hpp"

namespace vrpms {

constexpr int kBatchGaMaxP = 256;     // one lane per member

struct VrpBatchGaArgs {
  const int32_t* mats;    // [R][H][N][N]
  const int32_t* demand;  // [R][N]
  const int32_t* cap;     // [R][K]
  const int32_t* start;   // [R][K]
  int R, N, K, H, objective, P, G;
  uint32_t pmut;          // mutation iff philox word < pmut
  uint32_t seed_lo, seed_hi;
  uint16_t* tours;        // [R][n]
  uint64_t* keys;         // [R]
  int32_t* durs;          // [R][K]
  int8_t* veh;            // [R][n]
};

__host__ __device__ inline int batch_ga_sort_pairs(int P) {
  int M = 2;
  while (M < 2 * P) M <<= 1;
  return M;
}

__host__ __device__ inline uint32_t batch_ga_row_stride(int n) { return 2u * ((((uint32_t)n + 1u) >> 1) | 1u); }

__host__ __device__ inline uint32_t batch_ga_used_words(int N) {
  return ((((uint32_t)N + 31u) >> 5) + 3u) & ~3u;
}

// The kernel's own parts behind the instance: M2 sort pairs (uint64 key, uint32
// index), P parent and P child keys, the four `used` bitmaps, 2P rows of rs
// genes, prow and crow.  The kernel steps through them itself (below).
inline size_t batch_ga_lds(int N, int K, int H, int wide, int P) {
  const size_t M2 = batch_ga_sort_pairs(P), rs = batch_ga_row_stride(N - 1), uw = batch_ga_used_words(N);
  return batch_inst_bytes(N, K, H, wide) + 12 * M2 + 2 * 8 * (size_t)P + 4 * 4 * uw + 2 * (size_t)P * rs * 2 +
         2 * 2 * (size_t)P;
}

template <typename MatT, int HM>
__global__ __launch_bounds__(256) void vrp_batch_ga_kernel(VrpBatchGaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char batch_ga_lds_mem[];
  const int N = a.N, n = N - 1, K = a.K, P = a.P;
  const int64_t r = blockIdx.x;
  const uint32_t cells = (uint32_t)HM * (uint32_t)N * (uint32_t)N;
  const uint32_t mat_bytes = (cells * (uint32_t)sizeof(MatT) + 15u) & ~15u;
  const uint32_t dem_words = ((uint32_t)N + 3u) & ~3u, row_words = ((uint32_t)K + 3u) & ~3u;
  const int M2 = batch_ga_sort_pairs(P);
  const uint32_t rs = batch_ga_row_stride(n), uwords = batch_ga_used_words(N);
  MatT* M = reinterpret_cast<MatT*>(batch_ga_lds_mem);
  int32_t* dem = reinterpret_cast<int32_t*>(batch_ga_lds_mem + mat_bytes);
  int32_t* cap = dem + dem_words;
  int32_t* start = cap + row_words;
  uint64_t* sk = reinterpret_cast<uint64_t*>(start + row_words);   // [M2]
  uint64_t* pk = sk + M2;                                          // [P] parent keys by slot
  uint64_t* ck = pk + P;                                           // [P] child keys
  uint32_t* si = reinterpret_cast<uint32_t*>(ck + P);              // [M2]
  uint32_t* used_all = si + M2;                                    // [4][uwords]
  uint16_t* rows = reinterpret_cast<uint16_t*>(used_all + 4 * uwords);   // [2P][rs]
  uint16_t* prow = rows + (uint32_t)(2 * P) * rs;                  // [P] slot -> row
  uint16_t* crow = prow + P;                                       // [P] child -> row

  // stage and check the request (batch_stage.hpp); the verdict goes through
  // a word of the sort pairs, free until the first generation
  uint16_t* gtour = a.tours + r * n;
  int8_t* gveh = a.veh + r * n;
  int32_t* gdurs = a.durs + r * K;
  if (batch_stage_request(a.mats, a.demand, a.cap, a.start, r, cells, N, K, M, dem, cap, start,
                          reinterpret_cast<uint32_t*>(sk))) {
    batch_refuse(gtour, gveh, gdurs, a.keys + r, n, K);
    return;
  }

  const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
  const int tid = (int)threadIdx.x;
  const MatView<MatT, HM> D{M, (uint32_t)N, (uint32_t)N * (uint32_t)N, HM};
  const SplitParams sp{dem, cap, start, K, a.objective};
  auto score = [&](const uint16_t* T) {
    return eval_tour<true>(D, sp, [&](int i) { return (uint32_t)T[i]; }, n).key;
  };

  // the start: member i in row i, priced by its own lane
  if (tid < P) {
    uint16_t* T = rows + (uint32_t)tid * rs;
    for (int q = 0; q < n; ++q) T[q] = (uint16_t)(q + 1);
    for (int q = n - 1; q >= 1; --q) {
      const u32x4 x = philox(0xffffffffu, 0xffffffffu, (uint32_t)tid, (uint32_t)q, a.seed_lo, a.seed_hi);
      const int j = (int)(x.x % ((uint32_t)q + 1u));
      const uint16_t t = T[q];
      T[q] = T[j];
      T[j] = t;
    }
    pk[tid] = score(T);
    prow[tid] = (uint16_t)tid;
    crow[tid] = (uint16_t)(P + tid);
  }
  __syncthreads();

  uint32_t* used = used_all + (uint32_t)wave * uwords;
  const uint32_t words = ((uint32_t)N + 31u) >> 5;
  auto tourney = [&](uint32_t r0, uint32_t r1) {  // the lower (key, slot) wins
    const int u = (int)(r0 % (uint32_t)P), v = (int)(r1 % (uint32_t)P);
    const uint64_t ku = pk[u], kv = pk[v];
    return (kv < ku || (kv == ku && v < u)) ? v : u;
  };
  // one sampled move on a finished child, by one lane (O(n))
  auto mutate = [&](uint16_t* out, const u32x4& x, const u32x4& x2) {
    const Move m = decode_move(x2.w, x.x ^ x2.x, x.y ^ x2.y, n);
    if (m.typ == kMoveSwap) {
      const uint16_t t = out[m.i];
      out[m.i] = out[m.j];
      out[m.j] = t;
    } else if (m.typ == kMove2Opt) {
      for (int u = m.i, v = m.j; u < v; ++u, --v) {
        const uint16_t t = out[u];
        out[u] = out[v];
        out[v] = t;
      }
    } else if (m.i < m.j) {
      const uint16_t t = out[m.i];
      for (int u = m.i; u < m.j; ++u) out[u] = out[u + 1];
      out[m.j] = t;
    } else {
      const uint16_t t = out[m.i];
      for (int u = m.i; u > m.j; --u) out[u] = out[u - 1];
      out[m.j] = t;
    }
  };
  // N <= 64: every gene has a bit in one 64-bit register, so a lane breeds
  // its own child serially -- 256 children at once instead of four -- and
  // prices it straight away; larger tours take ga_breed_kernel's mapping
  const bool lanes = N <= 64;   // the same for every thread
  for (int g = 0; g < a.G; ++g) {
    if (lanes) {
      if (tid < P) {
        const u32x4 x = philox((uint32_t)g, 0u, (uint32_t)tid, 0u, a.seed_lo, a.seed_hi);
        const u32x4 x2 = philox((uint32_t)g, 0u, (uint32_t)tid, 1u, a.seed_lo, a.seed_hi);
        const uint16_t* A = rows + (uint32_t)prow[tourney(x.x, x.y)] * rs;
        const uint16_t* B = rows + (uint32_t)prow[tourney(x.z, x.w)] * rs;
        uint16_t* out = rows + (uint32_t)crow[tid] * rs;
        if (n < 2) {
          out[0] = A[0];
        } else {
          int lo = (int)(x2.x % (uint32_t)n), hi = (int)(x2.y % (uint32_t)n);
          if (lo > hi) {
            const int t = lo;
            lo = hi;
            hi = t;
          }
          uint64_t seen = 0;
          for (int q = lo; q <= hi; ++q) {
            const uint32_t gq = A[q];
            out[q] = (uint16_t)gq;
            seen |= 1ull << (gq & 63u);
          }
          // B from hi + 1 on (wrapping) fills the positions from hi + 1 on
          // (wrapping): B holds the same genes, so exactly the free positions
          int rd = hi + 1 == n ? 0 : hi + 1, wr = rd;
          for (int q = 0; q < n; ++q) {
            const uint32_t gq = B[rd];
            rd = rd + 1 == n ? 0 : rd + 1;
            if (!((seen >> (gq & 63u)) & 1ull) && wr != lo) {
              out[wr] = (uint16_t)gq;
              wr = wr + 1 == n ? 0 : wr + 1;
            }
          }
          if (x2.z < a.pmut) mutate(out, x, x2);
        }
        ck[tid] = score(out);
      }
      __syncthreads();
    } else {
      // breed: one wavefront per child at a time (ga_breed_kernel's OX1)
      for (int c = wave; c < P; c += 4) {
        const u32x4 x = philox((uint32_t)g, 0u, (uint32_t)c, 0u, a.seed_lo, a.seed_hi);
        const u32x4 x2 = philox((uint32_t)g, 0u, (uint32_t)c, 1u, a.seed_lo, a.seed_hi);
        const uint16_t* A = rows + (uint32_t)prow[tourney(x.x, x.y)] * rs;
        const uint16_t* B = rows + (uint32_t)prow[tourney(x.z, x.w)] * rs;
        uint16_t* out = rows + (uint32_t)crow[c] * rs;
        int lo = (int)(x2.x % (uint32_t)n), hi = (int)(x2.y % (uint32_t)n);   // n >= 64 here
        if (lo > hi) {
          const int t = lo;
          lo = hi;
          hi = t;
        }
        for (uint32_t w = lane; w < words; w += 64) used[w] = 0u;
        wave_sync();
        for (int q = lo + lane; q <= hi; q += 64) {
          const uint32_t gq = A[q];
          out[q] = (uint16_t)gq;
          atomicOr(&used[gq >> 5], 1u << (gq & 31u));
        }
        wave_sync();
        const int rest = n - (hi - lo + 1);
        int filled = 0;
        for (int base = 0; base < n; base += 64) {
          const int q = base + lane;
          uint32_t gq = 0;
          bool keep = false;
          if (q < n) {
            int p = hi + 1 + q;   // < 2n
            if (p >= n) p -= n;
            gq = B[p];
            keep = ((used[gq >> 5] >> (gq & 31u)) & 1u) == 0u;
          }
          const uint64_t ball = __ballot(keep);
          const int before = __popcll(ball & ((1ull << lane) - 1ull));
          if (keep) {
            const int slot = filled + before;   // slot-th free position after hi
            if (slot < rest) {
              int p = hi + 1 + slot;
              if (p >= n) p -= n;
              out[p] = (uint16_t)gq;
            }
          }
          filled += __popcll(ball);
        }
        wave_sync();
        if (x2.z < a.pmut && lane == 0) mutate(out, x, x2);
      }
      __syncthreads();
      // price: one lane per child
      if (tid < P) ck[tid] = score(rows + (uint32_t)crow[tid] * rs);
      __syncthreads();
    }
    // the 2P pairs, parents 0..P-1 by slot, children P..2P-1, padded to M2
    // with all-ones keys
    for (int i = tid; i < M2; i += 256) {
      sk[i] = i < 2 * P ? pk[i] : ~0ull;   // ck follows pk
      si[i] = (uint32_t)i;
    }
    __syncthreads();
    block_sort_pairs(sk, si, M2);
    // ranks 0..P-1 survive in their rows; the rows of ranks P..2P-1 take the
    // next children.  Every thread reads its (at most two) pairs' rows before
    // any map entry is replaced
    const int e0 = tid, e1 = tid + 256;
    uint32_t row0 = 0, row1 = 0;
    if (e0 < 2 * P) {
      const uint32_t i0 = si[e0];
      row0 = i0 < (uint32_t)P ? prow[i0] : crow[i0 - (uint32_t)P];
    }
    if (e1 < 2 * P) {
      const uint32_t i1 = si[e1];
      row1 = i1 < (uint32_t)P ? prow[i1] : crow[i1 - (uint32_t)P];
    }
    __syncthreads();
    if (e0 < P) pk[e0] = sk[e0];
    if (e0 < 2 * P) prow[e0] = (uint16_t)row0;   // crow follows prow
    if (e1 < 2 * P) prow[e1] = (uint16_t)row1;
    __syncthreads();
  }

  // the least (key, slot): lane l of wave 0 takes the slots [l per, (l + 1) per)
  // in order, so the lowest lane among equal keys holds the lowest slot
  if (wave != 0) return;
  const int per = (P + 63) >> 6;
  uint64_t bk = ~0ull;
  int bs = P;
  for (int s = lane * per; s < min(P, (lane + 1) * per); ++s)
    if (pk[s] < bk || bs == P) {
      bk = pk[s];
      bs = s;
    }
  int bl;
  bk = wave_argmin_lane(bk, bl);
  bs = wave_bcast(bs, bl);
  const uint16_t* Best = rows + (uint32_t)prow[bs] * rs;
  int16_t* V = reinterpret_cast<int16_t*>(rows + (uint32_t)crow[0] * rs);   // a row no member holds
  const int mydur = batch_final_walk(D, dem, cap, start, K, n, Best, n, V, lane);
  wave_sync();
  for (int q = lane; q < n; q += 64) {
    gtour[q] = Best[q];
    gveh[q] = (int8_t)V[q];
  }
  if (lane < K) gdurs[lane] = mydur;
  if (lane == 0) a.keys[r] = bk;
}

// the shape checks both entry points share; 0 or the refusal's code
static int batch_ga_check(const char* who, int32_t N, int32_t K, int32_t H, int32_t wide, int32_t P) {
  if (const int rc = batch_check_shape(who, N, K, H, wide)) return rc;
  if (P < 2 || P > kBatchGaMaxP)
    return fail(VRPMS_EINVAL, std::string(who) + ": one lane per member needs 2 <= P <= 256 (" +
                                  std::to_string(P) + " given)");
  return VRPMS_OK;
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_vrp_batch_ga_lds(int32_t N, int32_t K, int32_t H, int32_t wide, int32_t P,
                                      uint64_t* bytes) {
  const char* who = "vrpms_vrp_batch_ga_lds";
  if (const int rc = batch_check_bytes(who, bytes)) return rc;
  if (const int rc = batch_ga_check(who, N, K, H, wide, P)) return rc;
  *bytes = batch_ga_lds(N, K, H, wide, P);
  return VRPMS_OK;
}

extern "C" int vrpms_vrp_batch_ga(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                                  const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                                  int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t P,
                                  int32_t G, uint32_t pmut, uint64_t seed, uint16_t* d_tours,
                                  uint64_t* d_keys, int32_t* d_durs, int8_t* d_veh, void* stream) {
  const char* who = "vrpms_vrp_batch_ga";
  if (const int rc = batch_check_ctx(who, ctx, R)) return rc;
  if (const int rc = batch_ga_check(who, N, K, H, wide, P)) return rc;
  if (const int rc = batch_check_objective(who, objective)) return rc;
  if (G < 0)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_ga: G must not be negative (" + std::to_string(G) + " given)");
  if (R == 0) return VRPMS_OK;
  if (const int rc = batch_check_buffers(who, "matrix/demand/capacity/start/tour/key/duration/vehicle",
                                         {d_mats, d_demand, d_cap, d_start, d_tours, d_keys, d_durs, d_veh}))
    return rc;
  const size_t lds = batch_ga_lds(N, K, H, wide, P);
  if (lds > ctx->max_lds)
    return batch_lds_refusal(who, N, K, H, wide, " at P = " + std::to_string(P), lds, ctx->max_lds);
  VRPMS_HIP(hipSetDevice(ctx->device));
  const VrpBatchGaArgs a{d_mats, d_demand, d_cap, d_start, R,    N,
                         K,      H,        objective, P,   G,    pmut,
                         (uint32_t)seed, (uint32_t)(seed >> 32), d_tours, d_keys, d_durs, d_veh};
  const char* what = "";
  const hipError_t e = batch_with_matrix(wide, H, [&](auto m, auto hm) {
    return batch_launch_blocks(vrp_batch_ga_kernel<decltype(m), decltype(hm)::value>, a, (unsigned)R, lds,
                               (hipStream_t)stream, &what);
  });
  if (e != hipSuccess) return hip_fail(e, what);
  return VRPMS_OK;
}
