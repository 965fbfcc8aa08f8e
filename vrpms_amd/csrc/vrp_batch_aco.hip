// Throughput mode of the VRP ant colony: R
// independent small-fleet CVRP requests of one (N, K, H, objective, A, I) and
// one set of pheromone parameters share one launch, ONE WORKGROUP AND ONE
// COLONY PER REQUEST.  The workgroup stages its request's whole instance into
// LDS exactly as vrp_batch_sa / vrp_batch_ga do (batch_stage.hpp: the
// [H][N][N] matrix as uint16, or int32 when `wide`, the demand, capacity and
// start-time rows; a negative entry, or one above 65535 under wide = 0, ends
// the request with an all-ones key) and keeps the colony there: tau and eta as
// uint32 [N][N], A tours of n = N - 1 customers (no separators: the greedy
// split prices them) and the best-so-far tour.
//
//   start   tau = tau0 everywhere, eta = floor(2^24 / (1 + D[0][i][j])^2), the
//           hour-0 slice (aco_init_kernel's);
//   it      oracle.search.aco_iteration on colony 0: ant a, step s draws block
//           (it & M32, it >> 32, a, s), words 0 and 1; the roulette over
//           w_j = (tau[cur][j] >> 8) eta[cur][j], formed on the fly.  N <= 64:
//           one lane per ant, the visited set one 64-bit register, one pass
//           over the free nodes of row `cur` for the total and one for the
//           pick, the tour priced at once by eval_tour<true>.  N > 64: wave w
//           walks ants w, w + 4, ... by aco_construct_lds_kernel's roulette
//           (aco.hpp; lane l owns nodes 2 l and 2 l + 1 -- N <= 128 is all the
//           LDS formula admits), then one lane per ant prices.  The least
//           (key, ant) is the iteration best; it replaces the best-so-far when
//           strictly better; every cell evaporates and is clamped; the
//           iteration best -- or, when bsf_period > 0 and (it + 1) %
//           bsf_period == 0, the best-so-far -- deposits floor(2^30 / (1 +
//           primary)) on its n + 1 edges (distinct cells: no atomics);
//   answer  the best-so-far; wave 0 walks it once more and writes the K route
//           durations and every customer's vehicle.
//
// tau never wraps: a cell is at most tau_max <= 2^30 after evaporation and takes
// at most one deposit of at most 2^30 per iteration, so tau + dep <= 2^31 and
// the spec's `& M32` is idle.  Every pick is a node with a clear visited bit,
// and the bits of the nodes from N on are set from the start, so a pick indexes
// a row of the LDS tables on every path (the tot == 0 one included).
//
// The counters carry no request row: an answer does not depend on the launch
// the request rode in or on its row in it.
//
// LDS, every part as the kernel carves it (vrpms_vrp_batch_aco_lds), rs = the
// row stride in customers, 2 (ceil(n / 2) | 1) -- an odd number of words, so
// the lanes that walk one row each start in different banks:
//   align16(H N N (wide ? 4 : 2))            the matrix
// + 4 align4(N) + 2 * 4 align4(K)            demand, capacities, start times (int32)
// + 64                                       4 wave minima (8 each), the best-so-far
//                                            key (8), their 4 ants (4 each), 8 spare
// + 2 * 4 N N                                tau, eta
// + (A + 1) * 2 rs                           the ants' tours and the best-so-far's
// The ants' keys stay in registers: ant a is priced by thread a on both paths.
#include <hip/hip_runtime.h>

#include <string>

#include "aco.hpp"
#include "batch_launch.hpp"
#include "batch_stage.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "staging.hpp"
#include "tour.hpp"

// A/B builds only: 0 sends every N down the wavefront-per-ant
// construction.  Both constructions give the same tours.
#ifndef VRPMS_BATCH_ACO_LANE_MAX_N
#define VRPMS_BATCH_ACO_LANE_MAX_N 64
#endif

namespace vrpms {

constexpr int kBatchAcoMaxA = 256;     // one lane per ant
constexpr int kBatchAcoWaveMaxN = 128; // the wavefront-per-ant roulette at CH = 2
constexpr int kBatchAcoLaneMaxN = VRPMS_BATCH_ACO_LANE_MAX_N;
static_assert(kBatchAcoLaneMaxN <= 64, "the visited set of a lane's ant is one 64-bit register");

struct VrpBatchAcoArgs {
  const int32_t* mats;    // [R][H][N][N]
  const int32_t* demand;  // [R][N]
  const int32_t* cap;     // [R][K]
  const int32_t* start;   // [R][K]
  int R, N, K, H, objective, A, I;
  uint32_t tau0, tau_min, tau_max, evap_shift;
  int bsf_period;
  uint32_t seed_lo, seed_hi;
  uint16_t* tours;        // [R][n]
  uint64_t* keys;         // [R]
  int32_t* durs;          // [R][K]
  int8_t* veh;            // [R][n]
};

__host__ __device__ inline uint32_t batch_aco_row_stride(int n) { return 2u * ((((uint32_t)n + 1u) >> 1) | 1u); }

constexpr uint32_t kBatchAcoRedBytes = 64;

// The kernel's own parts behind the instance: the reduction words, tau and eta
// ([N][N] uint32 each), the A ants' rows and the best-so-far's (rs uint16 each).
// The kernel steps through them itself (below).
inline size_t batch_aco_lds(int N, int K, int H, int wide, int A) {
  const size_t rs = batch_aco_row_stride(N - 1);
  return batch_inst_bytes(N, K, H, wide) + kBatchAcoRedBytes + 2 * (size_t)N * N * 4 + ((size_t)A + 1) * rs * 2;
}

template <typename MatT, int HM>
__global__ __launch_bounds__(256) void vrp_batch_aco_kernel(VrpBatchAcoArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char batch_aco_lds_mem[];
  const int N = a.N, n = N - 1, K = a.K, A = a.A;
  const int64_t r = blockIdx.x;
  const uint32_t NN = (uint32_t)N * (uint32_t)N;
  const uint32_t cells = (uint32_t)HM * NN;
  const uint32_t mat_bytes = (cells * (uint32_t)sizeof(MatT) + 15u) & ~15u;
  const uint32_t dem_words = ((uint32_t)N + 3u) & ~3u, row_words = ((uint32_t)K + 3u) & ~3u;
  const uint32_t rs = batch_aco_row_stride(n);
  MatT* M = reinterpret_cast<MatT*>(batch_aco_lds_mem);
  int32_t* dem = reinterpret_cast<int32_t*>(batch_aco_lds_mem + mat_bytes);
  int32_t* cap = dem + dem_words;
  int32_t* start = cap + row_words;
  uint64_t* wk = reinterpret_cast<uint64_t*>(start + row_words);   // [4] the waves' minima
  uint64_t* bkey = wk + 4;                                         // the best-so-far key
  uint32_t* wa = reinterpret_cast<uint32_t*>(bkey + 1);            // [4] the waves' ants
  uint32_t* tau = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(wk) + kBatchAcoRedBytes);
  uint32_t* eta = tau + NN;                                        // [N][N] each
  uint16_t* rows = reinterpret_cast<uint16_t*>(eta + NN);          // [A][rs]
  uint16_t* bsf = rows + (uint32_t)A * rs;                         // [rs]

  // stage and check the request (batch_stage.hpp); the verdict goes through
  // a word of the waves' ants, free until the first iteration
  uint16_t* gtour = a.tours + r * n;
  int8_t* gveh = a.veh + r * n;
  int32_t* gdurs = a.durs + r * K;
  if (batch_stage_request(a.mats, a.demand, a.cap, a.start, r, cells, N, K, M, dem, cap, start, wa)) {
    batch_refuse(gtour, gveh, gdurs, a.keys + r, n, K);
    return;
  }

  const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
  const int tid = (int)threadIdx.x;
  const MatView<MatT, HM> D{M, (uint32_t)N, NN, HM};
  const SplitParams sp{dem, cap, start, K, a.objective};
  auto score = [&](const uint16_t* T) {
    return eval_tour<true>(D, sp, [&](int i) { return (uint32_t)T[i]; }, n).key;
  };

  for (uint32_t i = threadIdx.x; i < NN; i += 256) {
    tau[i] = a.tau0;
    eta[i] = aco_eta_cell((uint32_t)M[i]);   // hour slice 0
  }
  if (tid == 0) *bkey = ~0ull;
  __syncthreads();

  const bool lanes = N <= kBatchAcoLaneMaxN;   // the same for every thread
  for (int it = 0; it < a.I; ++it) {
    uint64_t key = ~0ull;   // ant tid's; all-ones for the threads past A
    if (lanes) {
      if (tid < A) {
        uint16_t* T = rows + (uint32_t)tid * rs;
        // bit j: node j is visited, or the depot, or past N
        uint64_t vis = 1ull | (N < 64 ? ~0ull << N : 0ull);
        uint32_t cur = 0;
        for (int s = 0; s < n; ++s) {   // n - s free nodes in every lane: the loops below run alike
          const u32x4 x = philox((uint32_t)it, 0u, (uint32_t)tid, (uint32_t)s, a.seed_lo, a.seed_hi);
          const uint32_t* Tr = tau + cur * (uint32_t)N;
          const uint32_t* Er = eta + cur * (uint32_t)N;
          uint64_t tot = 0;
          for (uint64_t m = ~vis; m; m &= m - 1) {
            const int j = __builtin_ctzll(m);
            tot += (uint64_t)(Tr[j] >> 8) * Er[j];
          }
          uint32_t pick = (uint32_t)__builtin_ctzll(~vis);   // the first free node
          if (tot != 0) {
            const uint64_t rr = umod64(((uint64_t)x.y << 32) | x.x, tot);
            uint64_t run = 0;
            bool found = false;
            for (uint64_t m = ~vis; m; m &= m - 1) {
              const int j = __builtin_ctzll(m);
              const uint64_t w = (uint64_t)(Tr[j] >> 8) * Er[j];
              run += w;
              if (!found && w > 0 && run > rr) {   // always once: run ends at tot > rr
                pick = (uint32_t)j;
                found = true;
              }
            }
          }
          T[s] = (uint16_t)pick;
          vis |= 1ull << pick;
          cur = pick;
        }
        key = score(T);
      }
    } else {
      // one wavefront per ant at a time (aco.hpp's roulette at CH = 2)
      for (int ant = wave; ant < A; ant += 4) {
        uint16_t* T = rows + (uint32_t)ant * rs;
        uint32_t vm = aco_owned_start<2>(lane, N);
        uint32_t cur = 0;
        AcoDraws draws;
        for (int s = 0; s < n; ++s) {
          draws.step((uint64_t)(uint32_t)it, (uint32_t)ant, s, lane, a.seed_lo, a.seed_hi);
          const uint32_t* Tr = tau + cur * (uint32_t)N + 2 * lane;
          const uint32_t* Er = eta + cur * (uint32_t)N + 2 * lane;
          uint64_t w[2];
#pragma unroll
          for (int c = 0; c < 2; ++c) w[c] = !((vm >> c) & 1u) ? (uint64_t)(Tr[c] >> 8) * Er[c] : 0ull;
          const uint32_t pick = aco_roulette_owned<2>(w, vm, draws.at(s), lane);
          if (lane == 0) T[s] = (uint16_t)pick;
          if ((uint32_t)lane == pick / 2) vm |= 1u << (pick % 2);
          cur = pick;
        }
      }
      __syncthreads();
      // price: one lane per ant
      if (tid < A) key = score(rows + (uint32_t)tid * rs);
    }
    // the iteration best: the least (key, ant).  Ant = thread, so the lowest
    // lane of a wave and then the lowest wave hold the lowest ant among equals
    int who;
    const uint64_t wmin = wave_argmin_lane(key, who);
    if (lane == 0) {
      wk[wave] = wmin;
      wa[wave] = (uint32_t)(wave * 64 + who);
    }
    __syncthreads();   // also: every tour is written
    uint64_t ibk = wk[0];
    uint32_t iba = wa[0];
#pragma unroll
    for (int x = 1; x < 4; ++x)
      if (wk[x] < ibk) {
        ibk = wk[x];
        iba = wa[x];
      }
    const uint64_t old = *bkey;
    const bool better = ibk < old;   // the same for every thread
    __syncthreads();   // every thread has read the minima and the key before either changes
    const uint16_t* Ib = rows + iba * rs;
    if (better) {
      for (int q = tid; q < n; q += 256) bsf[q] = Ib[q];
      if (tid == 0) *bkey = ibk;
    }
    for (uint32_t i = threadIdx.x; i < NN; i += 256)
      tau[i] = aco_evaporated(tau[i], a.evap_shift, a.tau_min, a.tau_max);
    __syncthreads();
    const bool global = a.bsf_period > 0 && (it + 1) % a.bsf_period == 0;
    const uint16_t* Dt = global ? bsf : Ib;
    const uint32_t dep = aco_deposit_of(global && !better ? old : ibk);
    for (int q = tid; q <= n; q += 256) {
      const uint32_t from = q == 0 ? 0u : Dt[q - 1];
      const uint32_t to = q == n ? 0u : Dt[q];
      tau[from * (uint32_t)N + to] += dep;   // n + 1 distinct cells
    }
    __syncthreads();
  }

  if (wave != 0) return;
  int16_t* V = reinterpret_cast<int16_t*>(rows);   // ant 0's row: no ant walks again
  const int mydur = batch_final_walk(D, dem, cap, start, K, n, bsf, n, V, lane);
  wave_sync();
  for (int q = lane; q < n; q += 64) {
    gtour[q] = bsf[q];
    gveh[q] = (int8_t)V[q];
  }
  if (lane < K) gdurs[lane] = mydur;
  if (lane == 0) a.keys[r] = *bkey;
}

// the shape checks both entry points share; 0 or the refusal's code
static int batch_aco_check(const char* who, int32_t N, int32_t K, int32_t H, int32_t wide, int32_t A) {
  if (const int rc = batch_check_shape(who, N, K, H, wide)) return rc;
  if (A < 1 || A > kBatchAcoMaxA)
    return fail(VRPMS_EINVAL,
                std::string(who) + ": one lane per ant needs 1 <= A <= 256 (" + std::to_string(A) + " given)");
  return VRPMS_OK;
}

}  // namespace vrpms

using namespace vrpms;

extern "C" int vrpms_vrp_batch_aco_lds(int32_t N, int32_t K, int32_t H, int32_t wide, int32_t A,
                                       uint64_t* bytes) {
  const char* who = "vrpms_vrp_batch_aco_lds";
  if (const int rc = batch_check_bytes(who, bytes)) return rc;
  if (const int rc = batch_aco_check(who, N, K, H, wide, A)) return rc;
  *bytes = batch_aco_lds(N, K, H, wide, A);
  return VRPMS_OK;
}

extern "C" int vrpms_vrp_batch_aco(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                                   const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                                   int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t A,
                                   int32_t I, uint32_t tau0, uint32_t tau_min, uint32_t tau_max,
                                   int32_t evap_shift, int32_t bsf_period, uint64_t seed,
                                   uint16_t* d_tours, uint64_t* d_keys, int32_t* d_durs, int8_t* d_veh,
                                   void* stream) {
  const char* who = "vrpms_vrp_batch_aco";
  if (const int rc = batch_check_ctx(who, ctx, R)) return rc;
  if (const int rc = batch_aco_check(who, N, K, H, wide, A)) return rc;
  if (const int rc = batch_check_objective(who, objective)) return rc;
  if (I < 1)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_aco: I must be at least 1 (" + std::to_string(I) + " given)");
  if (evap_shift < 1 || evap_shift > 31)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_aco: evap_shift must be in [1, 31] (" +
                                  std::to_string(evap_shift) + " given)");
  if (bsf_period < 0)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_aco: bsf_period must not be negative (" +
                                  std::to_string(bsf_period) + " given)");
  if (!(0u < tau_min && tau_min <= tau0 && tau0 <= tau_max && tau_max <= (1u << 30)))
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_aco: needs 0 < tau_min <= tau0 <= tau_max <= 2^30 (" +
                                  std::to_string(tau_min) + ", " + std::to_string(tau0) + ", " +
                                  std::to_string(tau_max) + " given)");
  if (R == 0) return VRPMS_OK;
  if (const int rc = batch_check_buffers(who, "matrix/demand/capacity/start/tour/key/duration/vehicle",
                                         {d_mats, d_demand, d_cap, d_start, d_tours, d_keys, d_durs, d_veh}))
    return rc;
  const size_t lds = batch_aco_lds(N, K, H, wide, A);
  if (lds > ctx->max_lds)
    return batch_lds_refusal(who, N, K, H, wide, " at A = " + std::to_string(A), lds, ctx->max_lds);
  // 10 * 129 * 129 bytes are above the 160 KiB of a CU, so this refuses nothing
  // the formula admits there; it keeps a larger LDS from outgrowing CH = 2
  if (N > kBatchAcoWaveMaxN)
    return fail(VRPMS_EINVAL, "vrpms_vrp_batch_aco: N = " + std::to_string(N) + " is above the 128 nodes of the "
                                  "wavefront-per-ant construction");
  VRPMS_HIP(hipSetDevice(ctx->device));
  const VrpBatchAcoArgs a{d_mats, d_demand, d_cap, d_start, R, N, K, H, objective, A, I,
                          tau0, tau_min, tau_max, (uint32_t)evap_shift, bsf_period,
                          (uint32_t)seed, (uint32_t)(seed >> 32), d_tours, d_keys, d_durs, d_veh};
  const char* what = "";
  const hipError_t e = batch_with_matrix(wide, H, [&](auto m, auto hm) {
    return batch_launch_blocks(vrp_batch_aco_kernel<decltype(m), decltype(hm)::value>, a, (unsigned)R, lds,
                               (hipStream_t)stream, &what);
  });
  if (e != hipSuccess) return hip_fail(e, what);
  return VRPMS_OK;
}
