/* vrpms.h -- C ABI of the MI355X (gfx950) vrpms solver core.
 *
 * The reference (metehkaya/vrpms) has no native code and no FFI: its solver
 * slot is the `# TODO: Run algorithm` block of each HTTP handler and the stub
 * `src/solver.py`.  This header is the boundary the Python front-end
 * (`vrpms_amd/solver.py`, which keeps the `src/solver.py` entry points and the
 * handler result dicts) binds through ctypes.  Each entry point names the
 * reference line whose behaviour it supplies.
 *
 * Conventions
 *   - Every function returns 0 (VRPMS_OK) or a negative VRPMS_E* code; the
 *     message is in vrpms_last_error() (thread-local).  No C++ exception ever
 *     crosses this boundary.
 *   - All `d_*` pointers are DEVICE pointers owned by the caller (PyTorch-ROCm
 *     tensors in the Python front-end); the library never frees them.  The
 *     context owns its own scratch and derived matrix layouts.
 *   - `stream` is a hipStream_t (NULL = default stream).  Every call after
 *     vrpms_set_instance is asynchronous on that stream; nothing synchronises
 *     except vrpms_set_instance (validation readback) and vrpms_ctx_destroy.
 *   - Nodes are compact indices: node 0 is the depot (VRP, A1) or the
 *     startNode (TSP, A4); customers are 1..N-1.  Tours are "giant tours":
 *     a permutation of customers without the depot, stored as uint8 (N<=256)
 *     or uint16 rows of `ld` elements.  A CVRP tour may also hold the token
 *     0 any number of times (A10 route separator: it closes the current
 *     vehicle's route and opens the next); `n` then counts tokens.
 *   - Semantics are SURVEY.md Appendix A (frozen in oracle/spec.py).
 */
#ifndef VRPMS_H
#define VRPMS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRPMS_OK 0
#define VRPMS_EINVAL (-1)   /* bad argument / shape */
#define VRPMS_EHIP (-2)     /* HIP runtime error */
#define VRPMS_ERANGE (-3)   /* A9 overflow guard: clock could exceed int32 */
#define VRPMS_ESTATE (-4)   /* no instance loaded */
#define VRPMS_ENOMEM (-5)
#define VRPMS_ETIMEOUT (-6) /* a collective did not complete within its deadline */

#define VRPMS_TSP 0
#define VRPMS_CVRP 1

#define VRPMS_OBJ_SUM 0 /* primary durationSum, secondary durationMax */
#define VRPMS_OBJ_MAX 1 /* primary durationMax, secondary durationSum */

typedef struct vrpms_ctx vrpms_ctx;

/* Library version, (major << 16) | minor. */
int vrpms_version(void);

/* Thread-local message for the last failing call on this thread. */
const char* vrpms_last_error(void);

/* Create / destroy a solver context bound to HIP device `device`. */
int vrpms_ctx_create(int device, vrpms_ctx** out);
int vrpms_ctx_destroy(vrpms_ctx* ctx);

/* Load an instance (replaces the DB fetch result consumed at
 * api/vrp/ga/index.py:41-42 / api/tsp/ga/index.py:33-34).
 *   problem  VRPMS_TSP or VRPMS_CVRP
 *   d_dur    int32 [H][N][N] durations in minutes (A2/A3), any H in
 *            [1, 1024] with H * N * N < 2^31: an edge leaving at minute t
 *            reads slice (t / 60) % H.  Scoring and the SA / GA / ACO / BF
 *            kernels take every such H (H = 1 and 24 have kernels of their
 *            own); the exact solvers still need H = 1 (tsp_dp, vrp_sp) or
 *            H = 1 or 24 (tsp_tdp, vrp_tdsp) and refuse any other
 *   d_demand int32 [N] (demand[0] ignored); NULL for TSP
 *   d_cap    int32 [K] vehicle capacities (api/parameters.py:11); NULL for TSP
 *   d_start  int32 [K] start minutes (api/parameters.py:12; TSP: K = 1 and
 *            d_start[0] = startTime, api/parameters.py:43)
 * Validates non-negativity and the A9 int32 guard (synchronises once).
 * Chooses the on-chip tier (LDS-resident / L2-resident) and builds the
 * packed device layouts used by the kernels. */
int vrpms_set_instance(vrpms_ctx* ctx, int32_t problem, const int32_t* d_dur, int32_t H,
                       int32_t N, const int32_t* d_demand, const int32_t* d_cap,
                       const int32_t* d_start, int32_t K, int32_t objective, void* stream);

/* Batched full evaluation of C candidate giant tours (the scoring half of
 * the hot path; the reference's would-be cost function behind
 * api/{tsp,vrp}/<algo>/index.py's TODO slot).
 *   d_perms   [C][ld] uint8 (perm_bytes=1) or uint16 (perm_bytes=2), n used
 *   d_keys    [C] A8 objective keys (required)
 *   d_sum     [C] durationSum (TSP: duration)  -- nullable
 *   d_max     [C] durationMax (TSP: duration)  -- nullable
 *   d_unv     [C] unvisited customer count     -- nullable */
int vrpms_eval(vrpms_ctx* ctx, const void* d_perms, int32_t perm_bytes, int64_t C, int32_t n,
               int64_t ld, uint64_t* d_keys, int32_t* d_sum, int32_t* d_max, int32_t* d_unv,
               void* stream);

/* Same scoring on the word-interleaved tour layout (VRPMS_LAYOUT_WORDS):
 *   d_words   uint32 [ceil(n/4)][C]; word w of candidate c packs customers
 *             4w..4w+3 (uint8 each, low byte first).  N <= 256.
 * Lane c's loads of word w form one contiguous 256-B wave access, so tours
 * stream HBM -> registers with no LDS staging.  This is the layout the GA
 * breed and ACO construct kernels emit for CVRP with N <= 256, so their
 * children / ants are scored by this kernel (eval_cvrp_words2).  Outputs
 * as vrpms_eval. */
int vrpms_eval_words(vrpms_ctx* ctx, const uint32_t* d_words, int64_t C, int32_t n,
                     uint64_t* d_keys, int32_t* d_sum, int32_t* d_max, int32_t* d_unv,
                     void* stream);

/* Re-layout uint8 rows [C][ld] into the word-interleaved layout. */
int vrpms_rows_to_words(vrpms_ctx* ctx, const uint8_t* d_rows, int64_t C, int32_t n, int64_t ld,
                        uint32_t* d_words, void* stream);

/* Which scoring kernel vrpms_eval picks for these tour buffers:
 * 0 = eval_cvrp_packed (LDS packed matrix + LDS-staged tiles),
 * 1 = eval_tsp_staged, 2 = eval_staged (LDS-staged tours, L2-resident or
 * LDS matrix, depot legs in LDS tables; eval_generic when its tables do not
 * fit the LDS); -1 = no instance. */
int vrpms_eval_path(vrpms_ctx* ctx, int32_t perm_bytes, int64_t ld, const void* d_perms);

/* The data layouts vrpms_set_instance chose for the loaded instance, and
 * whether the branch-free split (eval_cvrp_rows2 / eval_cvrp_words2, the
 * packed SA / GA / ACO scorers) takes tours of n customers.  Host only:
 * launches and copies nothing.  Fills out[0 .. VRPMS_LAYOUT_FIELDS), count >=
 * VRPMS_LAYOUT_FIELDS:
 *    0 use16        the matrix is also held as uint16 (max duration <= 65535)
 *    1 tier         0 packed u64 matrix in LDS, 1 plain matrix in LDS, 2 L2
 *    2 pack_w       width of the packed ret / out fields; 0 = no packed matrix
 *    3 pref_S       width of the prefix-ret duration field; 0 = no such layout
 *    4 pref_lim     (cap + 1) << pref_S, the uint32 bit pattern
 *    5 uniform_cap  every vehicle has the same capacity
 *    6 symmetric    hour slice 0 is symmetric
 *    7 sym_all      every hour slice is symmetric
 *    8 flex         some demand exceeds the smallest capacity (vehicle skipping)
 *    9 fast         the branch-free split takes tours of n customers
 *   10 ks           fast: bit position of its vehicle counter, else 0
 *   11 B            fast: width of that counter (31 - ks), else 0
 *   12 carry        fast: the fit test is the add's carry (every demand >= 1)
 *   13 hour_minor   the hour-minor uint16 copy exists (H = 24, use16) */
#define VRPMS_LAYOUT_FIELDS 14
int vrpms_instance_layout(vrpms_ctx* ctx, int32_t n, int32_t* out, int32_t count);

/* Context options (kernel-variant overrides for A/B tests and profiling).
 *   VRPMS_OPT_SPLIT_MODE: 0 = auto (branch-free prefix-ret split whenever its
 *   packed layout fits), 2 = force the branchy split in eval_cvrp_packed,
 *   3 = the words kernel's compare form of the fit test instead of the
 *   add's carry (the two give identical keys; tests check both). */
#define VRPMS_OPT_SPLIT_MODE 1
/*   VRPMS_OPT_STAGED_M: candidates interleaved per lane in eval_staged
 *   (0 = auto: 1; 1 forces 1; 2 asks for two, which the launcher grants
 *   only on an hour-indexed matrix (H > 1) whose fleet needs no vehicle
 *   skipping (every demand fits the smallest vehicle) and whose two-candidate
 *   tile fits the LDS -- otherwise it runs one; A/B, the results are the
 *   same). */
#define VRPMS_OPT_STAGED_M 2
/*   VRPMS_OPT_WORDS_KERNEL: LDS-packed kernel for path 0 of vrpms_eval
 *   (0 = auto: eval_cvrp_rows2; 1 = eval_cvrp_packed, the LDS-tile kernel
 *   also used for heterogeneous fleets, A/B only). */
#define VRPMS_OPT_WORDS_KERNEL 3
/*   VRPMS_OPT_WORDS_ILP: candidates per lane in eval_cvrp_words2 (0 = auto:
 *   2; 2 force; 1 only in libraries built with -DVRPMS_AB, A/B, where 3..6
 *   also force two per lane in workgroup shape 0..3 of launch_words2). */
#define VRPMS_OPT_WORDS_ILP 4
/*   VRPMS_OPT_WORDS_LOOKAHEAD: words ahead whose gathers eval_cvrp_words2
 *   keeps in flight (0 = auto, 1 or 2 force; A/B). */
#define VRPMS_OPT_WORDS_LOOKAHEAD 5
/*   VRPMS_OPT_ROWS_CONFIG: eval_cvrp_rows2's (chunk words, candidates per
 *   lane): 0 = auto (fewest chunks that fit the LDS), 1 = (8, 2),
 *   2 = (16, 1), 3 = (4, 2), 4 = (8, 1), 5 = (4, 1); A/B. */
#define VRPMS_OPT_ROWS_CONFIG 6
/*   VRPMS_OPT_GA_FUSED: 0 = auto (the fused one-workgroup-per-island GA
 *   kernel whenever the island fits the LDS), 2 = force the three-kernel
 *   path (breed / score / select launches per generation); A/B. */
#define VRPMS_OPT_GA_FUSED 7
/*   VRPMS_OPT_SA_ROUTE: 0 = auto (static symmetric matrix, every demand
 *   fitting the smallest vehicle: every move priced from per-position prefix
 *   sums, sa_seg_kernel -- one capacity, or per-vehicle capacities with each
 *   route tracked on its vehicle; hour-indexed matrix (H = 24): full walks
 *   whose durations come from 24-hour edge rows cached per tour position in
 *   LDS, sa_td_kernel, any fleet; otherwise windowed SA on an exchangeable
 *   fleet prices moves by route-local walks, sa_route_kernel), 2 = force full
 *   re-evaluation of every move (sa_kernel), 3 = force the route-local walks,
 *   4 = force the hour-row walks; A/B. */
#define VRPMS_OPT_SA_ROUTE 8
/*   VRPMS_OPT_ROUTE_WG_PER_CU: workgroups of sa_route_kernel per CU (0 =
 *   auto: 1 for multi-wavefront chains, whose LDS request is padded past
 *   half the CU so each wavefront has a SIMD to itself -- the pricing walk
 *   is VALU-issue bound, so a lone wavefront steps up to twice as fast --
 *   and as many as fit for one-wavefront chains; 1 or 2 force). */
#define VRPMS_OPT_ROUTE_WG_PER_CU 9
/*   VRPMS_OPT_ISLAND_TIMEOUT_S: deadline in seconds of vrpms_island_init
 *   (default 120): the RCCL communicator is created non-blocking and aborted
 *   when not every rank has joined by then, so a rank that never arrives
 *   yields VRPMS_ETIMEOUT instead of a hang. */
#define VRPMS_OPT_ISLAND_TIMEOUT_S 10
/*   VRPMS_OPT_SEG_WAVES: wavefronts per chain of the segment-priced SA kernel
 *   (0 = auto: moves / 64 up to 4 while every chain's wavefronts stay
 *   resident; 1..4 force, A/B -- the trajectories do not depend on it). */
#define VRPMS_OPT_SEG_WAVES 11
/*   VRPMS_OPT_ACO_CONSTRUCT: 0 = auto (ant construction reads the colony's
 *   weights (tau >> 8) * eta from LDS, staged once per iteration by a
 *   workgroup of up to 16 ants of one colony, whenever N * N * 8 bytes fit;
 *   else from L2), 2 = force the L2 path; A/B -- the tours are the same. */
#define VRPMS_OPT_ACO_CONSTRUCT 12
/*   VRPMS_OPT_BATCH_DP_TEAM: threads per request of vrpms_tsp_batch_dp (0 =
 *   auto: the measured n -> T table of DESIGN.md §4.3i; 16, 32, 64, 128 or
 *   256 force, A/B -- the results do not depend on it; a forced T whose
 *   256 / T tables do not fit the LDS makes the call fail). */
#define VRPMS_OPT_BATCH_DP_TEAM 13
int vrpms_set_option(vrpms_ctx* ctx, int32_t option, int32_t value);

/* Decode ONE giant tour into the result dict of api/vrp/ga/index.py:49-53
 * (A6/A7): d_vehicle_of[i] = vehicle serving perm position i, or -1 when
 * unvisited; d_route_dur[k] = duration of vehicle k (0 if unused). */
int vrpms_decode(vrpms_ctx* ctx, const void* d_perm, int32_t perm_bytes, int32_t n,
                 int32_t* d_vehicle_of, int32_t* d_route_dur, void* stream);

/* Argmin over C keys: d_out[0] = min key, d_out[1] = smallest index holding
 * it.  Wave64 shuffle reduction + one 64-bit atomicMin pass. */
int vrpms_argmin(vrpms_ctx* ctx, const uint64_t* d_keys, int64_t C, uint64_t* d_out,
                 void* stream);

/* ------------------------------------------------------------------------
 * Search kernels: the algorithms behind api/{tsp,vrp}/{sa,ga,aco,bf}/index.py
 * (each stops at `# TODO: Run algorithm` in the reference).  Tours here are
 * uint16 rows [..][n] (n = N - 1 customers).  Every random choice is
 * Philox4x32-10 keyed by `seed` with counters (step/generation/iteration,
 * chain/island/ant, lane/stream), so oracle/spec.py replays them exactly.
 * ---------------------------------------------------------------------- */

/* Simulated annealing (api/{tsp,vrp}/sa/index.py; knobs: api/parameters.py:26-27
 * declares none, so the front-end supplies defaults).  One wavefront per
 * chain: every step the 64 lanes score 64 Philox-sampled moves (swap /
 * 2-opt / relocate) of the chain's tour, the best (key, lane) is accepted if
 * it is no worse or if (u >> 8) < floor(2^24 exp(-dp * invT)); invT is
 * multiplied by inv_alpha after every step (geometric cooling). */
typedef struct {
  int32_t chains;   /* one wavefront each */
  int32_t steps;    /* steps in this call */
  float inv_t0;     /* 1 / temperature at the first step of this call */
  float inv_alpha;  /* per-step factor on 1/T (1/alpha for T *= alpha) */
  uint64_t seed;
  uint64_t step0;   /* global index of the first step (Philox counter) */
  int32_t window;   /* A11: 0 = moves over the whole tour; W > 0 = the second
                       position within W of the first (large tours) */
  uint32_t window_types; /* A12: move types the window applies to, bit t for
                            type t (1 swap, 2 2-opt, 4 relocate); 0 = all */
  int32_t moves;    /* moves sampled per step: 0 or 64 = one wavefront per chain;
                       64 W (W = 2..8) = W wavefronts per chain, move index
                       lane + 64 w (route-local kernel: window > 0 on a fleet
                       of one capacity and start time).  vrpms_tsp_batch_sa
                       ignores it. */
} vrpms_sa_params;

/* d_cur [chains][n] in/out (cur_key out); d_best/d_best_key in/out (set
 * d_best_key to UINT64_MAX before the first call).  CVRP tours may carry
 * A10 separator tokens (n <= N - 1 + K): the moves then also shift route
 * boundaries (relocating a separator), exchange customers across routes and
 * reverse route sequences. */
int vrpms_sa_run(vrpms_ctx* ctx, const vrpms_sa_params* p, uint16_t* d_cur, uint64_t* d_cur_key,
                 uint16_t* d_best, uint64_t* d_best_key, int32_t n, void* stream);

/* Genetic algorithm (api/vrp/ga/index.py; randomPermutationCount -> pop,
 * iterationCount -> generations, api/parameters.py:18-23).  Per generation:
 * binary tournaments, OX1 crossover, Philox-gated mutation (one move),
 * batched scoring, (mu + lambda) survivors per island. */
typedef struct {
  int32_t islands;
  int32_t pop;          /* 2..4096 */
  int32_t generations;  /* generations in this call */
  uint32_t pmut;        /* mutate iff a Philox word < pmut (pmut/2^32 = probability) */
  uint64_t seed;
  uint64_t gen0;        /* global index of the first generation */
} vrpms_ga_params;

/* d_pop [islands][pop][n] and d_keys [islands][pop] in/out (keys must
 * score d_pop on entry, e.g. by vrpms_eval).  For uniform-fleet CVRP on the
 * packed-LDS instances (N <= 128) one 1024-lane workgroup per island runs
 * all `generations` in LDS (ga_fused.hip) when the island fits beside the
 * matrix (CVRP-100: pop <= 256); otherwise each generation is breed ->
 * score -> select launches, the children emitted in the word-interleaved
 * layout and scored by eval_cvrp_words2 when that kernel applies. */
int vrpms_ga_generation(vrpms_ctx* ctx, const vrpms_ga_params* p, uint16_t* d_pop,
                        uint64_t* d_keys, int32_t n, void* stream);

/* Ant colony (api/{tsp,vrp}/aco/index.py), integer pheromone so every
 * update is exact and order-independent: w_ij = (tau_ij >> 8) * eta_ij,
 * eta_ij = floor(2^24 / (1 + D_ij)^2); tau <- clamp(tau - tau >> evap_shift);
 * the iteration-best ant deposits floor(2^30 / (1 + primary)) per edge --
 * or, every bsf_period-th iteration ((iter + 1) % bsf_period == 0, best-so-far
 * buffers given), the colony's best-so-far does (max-min global-best update:
 * an island migrant injected into the best-so-far then shapes tau). */
typedef struct {
  int32_t colonies;
  int32_t ants;        /* per colony, one wavefront each */
  int32_t evap_shift;  /* rho = 2^-evap_shift */
  uint32_t tau_min, tau_max;  /* tau_max <= 2^31 */
  uint64_t seed;
  uint64_t iter;       /* global iteration index (Philox counter) */
  uint32_t bsf_period; /* 0: the iteration best always deposits */
} vrpms_aco_params;

/* d_tau [colonies][N][N] <- tau0, d_eta [N][N] <- floor(2^24 / (1 + D)^2). */
int vrpms_aco_init(vrpms_ctx* ctx, int32_t colonies, uint32_t tau0, uint32_t* d_tau,
                   uint32_t* d_eta, void* stream);

/* One iteration: construct d_tours [colonies][ants][n] (n = N - 1), score
 * them into d_keys, d_iter_best [colonies][2] = (key, ant), update tau.
 * d_best_tours [colonies][n] / d_best_keys [colonies] (nullable, both or
 * neither): each colony's best-so-far, replaced by its iteration best when
 * strictly better (set the keys to UINT64_MAX before the first call).
 * For CVRP with N <= 256 the ants also emit the word-interleaved layout and
 * are scored by the headline kernel (eval_cvrp_words2). */
int vrpms_aco_iteration(vrpms_ctx* ctx, const vrpms_aco_params* p, uint32_t* d_tau,
                        const uint32_t* d_eta, uint16_t* d_tours, uint64_t* d_keys,
                        uint64_t* d_iter_best, uint16_t* d_best_tours, uint64_t* d_best_keys,
                        int32_t n, void* stream);

/* Brute force (api/{tsp,vrp}/bf/index.py): lexicographic ranks
 * [rank_begin, rank_end) of the permutations of customers 1..n (n <= 15);
 * d_out[0] = min key, d_out[1] = smallest rank holding it (UINT64_MAX if
 * the range is empty).  Multi-GPU: disjoint rank ranges + a min. */
int vrpms_bf_run(vrpms_ctx* ctx, int32_t n, uint64_t rank_begin, uint64_t rank_end,
                 uint64_t* d_out, void* stream);

/* Exact TSP by Held-Karp subset dynamic programming (spec A14): customers
 * 1..n (1 <= n <= min(24, N-1)) of the loaded TSP instance, static matrix
 * only (H = 1; it may be asymmetric), node 0 the start node.  The caller owns
 * the table: vrpms_tsp_dp_workspace gives its size in bytes (host only, no
 * context; 2^n rows of 16 words for n <= 16, of 32 words above: 2 GiB at
 * n = 24).  vrpms_tsp_dp_run enqueues one launch per subset cardinality on
 * `stream` and writes d_tour[n] -- the lexicographically smallest optimal
 * tour, the same tie rule as vrpms_bf_run's smallest rank -- and d_key[0],
 * its A8 key.  VRPMS_EINVAL for a CVRP or hour-indexed instance, n out of
 * range or a workspace smaller than vrpms_tsp_dp_workspace's. */
int vrpms_tsp_dp_workspace(int32_t n, uint64_t* bytes);
int vrpms_tsp_dp_run(vrpms_ctx* ctx, int32_t n, void* d_work, uint64_t work_bytes,
                     int16_t* d_tour, uint64_t* d_key, void* stream);

/* Exact small-fleet CVRP by subset partition dynamic programming (spec A15):
 * customers 1..n (1 <= n <= min(20, N-1)) of the loaded CVRP instance, static
 * matrix only (H = 1; it may be asymmetric), node 0 the depot, the K <= 64
 * vehicles, their capacities, the demands and the objective as loaded.
 * Minimises (unvisited, primary) exactly over all A10 separator tours; the
 * secondary field is whatever the returned solution has.  The caller owns the
 * workspace: vrpms_vrp_sp_workspace gives its size in bytes (host only, no
 * context: the Held-Karp table of vrpms_tsp_dp_workspace plus K + 3 arrays of
 * 2^n words).  vrpms_vrp_sp_run enqueues the Held-Karp layers, then one
 * launch per vehicle, on `stream` and writes d_tour[n + K] -- route 0, a
 * separator 0, route 1, 0, ..., route K-1, 0, then the unserved customers in
 * ascending order -- and d_key[0], the A8 key of that tour.  VRPMS_EINVAL,
 * with nothing launched, for a TSP or hour-indexed instance, n out of range,
 * more than 64 vehicles or a workspace smaller than vrpms_vrp_sp_workspace's
 * or not 4-byte aligned. */
int vrpms_vrp_sp_workspace(int32_t n, int32_t K, uint64_t* bytes);
int vrpms_vrp_sp_run(vrpms_ctx* ctx, int32_t n, void* d_work, uint64_t work_bytes,
                     int16_t* d_tour, uint64_t* d_key, void* stream);

/* Exact time-dependent TSP by time-expanded subset dynamic programming (spec
 * A16): customers 1..n (1 <= n <= min(20, N-1)) of the loaded TSP instance,
 * H = 1 or H = 24 (the matrix may be asymmetric, non-metric and non-FIFO),
 * node 0 the start node, the instance's start time.  `horizon` >= 0 is an
 * upper bound in minutes on the tour duration: the optimum is found if it is
 * at most `horizon`, and key and tour do not depend on `horizon` then.  The
 * caller owns the table: vrpms_tsp_tdp_workspace gives its size in bytes (host
 * only, no context): 2^n * n rows of W = (start_time % 60 + horizon) / 60 + 1
 * uint64 words (one hour of clock bits each), W <= 512.  vrpms_tsp_tdp_run
 * enqueues one launch per subset cardinality on `stream` and writes d_tour[n]
 * -- the optimal tour whose reversed sequence is lexicographically smallest --
 * and d_key[0], its A8 key; when no tour fits the horizon d_key[0] is
 * UINT64_MAX and d_tour all zeros.  VRPMS_EINVAL, with nothing launched, for a
 * CVRP instance, H other than 1 or 24, n out of range, a negative horizon, one
 * that needs more than 512 words, or a workspace smaller than
 * vrpms_tsp_tdp_workspace's or not 8-byte aligned. */
int vrpms_tsp_tdp_workspace(int32_t n, int32_t start_time, int32_t horizon, uint64_t* bytes);
int vrpms_tsp_tdp_run(vrpms_ctx* ctx, int32_t n, int32_t horizon, void* d_work,
                      uint64_t work_bytes, int16_t* d_tour, uint64_t* d_key, void* stream);

/* Exact time-dependent CVRP by time-expanded partition dynamic programming
 * (spec A17): customers 1..n (1 <= n <= min(20, N-1)) of the loaded CVRP
 * instance, H = 1 or H = 24 (the matrix may be asymmetric, non-metric and
 * non-FIFO), node 0 the depot, the K <= 64 vehicles in their given order with
 * their capacities and start times (vehicle k leaves at start_times[k], no
 * waiting anywhere), the demands and the objective as loaded.  Minimises
 * (unvisited, primary) exactly over all A10 separator tours; the secondary
 * field is whatever the returned solution has.  `horizon` >= 0 is an upper
 * bound in minutes on the duration of every single route: if it is at least
 * the optimum's primary, key and tour are those of any larger horizon.  Below
 * that the answer is the optimum among solutions whose every route fits
 * `horizon`, which may leave more customers unvisited: the caller owns that
 * promise.  The caller owns the workspace: vrpms_vrp_tdsp_workspace gives its
 * size in bytes (host only, no context) for G distinct start times, the
 * largest being max_start: one A16 table of 2^n * n rows of
 * W = (min(59, max_start) + horizon) / 60 + 1 uint64 words (W <= 512; every
 * start's own row width is at most that), then G + K + 2 arrays of 2^n uint32
 * (the G route tables, demand, capacity-masked routes, f_1..f_K), then 8 K + 16
 * bytes for the chosen route sets.  vrpms_vrp_tdsp_run enqueues, per distinct
 * start time, the A16 layers and the route kernel, then one launch per
 * vehicle, on `stream`; it then SYNCHRONISES `stream` once to read the K
 * chosen (route set, duration) pairs back, because the launches that rebuild
 * each route's tour are shaped by them, and enqueues those.  d_tour[n + K] --
 * route 0, a separator 0, ..., route K-1, 0, then the unserved customers in
 * ascending order, each route A16's tie-ruled tour of its customers from its
 * vehicle's start time -- and d_key[0], the A8 key of that tour, are written on
 * `stream`.  VRPMS_EINVAL, with nothing launched, for a TSP instance, H other
 * than 1 or 24, n or K out of range, a negative horizon, one that needs more
 * than 512 words, or a workspace smaller than vrpms_vrp_tdsp_workspace's or not
 * 8-byte aligned. */
int vrpms_vrp_tdsp_workspace(int32_t n, int32_t K, int32_t G, int32_t max_start,
                             int32_t horizon, uint64_t* bytes);
int vrpms_vrp_tdsp_run(vrpms_ctx* ctx, int32_t n, int32_t horizon, void* d_work,
                       uint64_t work_bytes, int16_t* d_tour, uint64_t* d_key, void* stream);

/* Throughput mode (BASELINE.json config 5: many concurrent TSP requests):
 * R independent static TSP requests, each with its own int32 [N][N] matrix
 * (d_mats [R][N][N], node 0 = start node), ONE WORKGROUP PER REQUEST: 4 SA
 * chains per request from Philox Fisher-Yates starts, moves priced by exact
 * O(1) integer deltas (2-opt re-prices the reversed segment when the matrix
 * is asymmetric).  Uses p->steps, inv_t0, inv_alpha, seed (chains/step0
 * ignored).  Out: d_best_tours [R][N-1], d_best_keys [R].  No instance needed. */
int vrpms_tsp_batch_sa(vrpms_ctx* ctx, const int32_t* d_mats, int32_t R, int32_t N,
                       const vrpms_sa_params* p, uint16_t* d_best_tours, uint64_t* d_best_keys,
                       void* stream);

/* Throughput mode of the exact TSP: R independent static
 * TSP requests of one node count N, 2 <= N <= 13 (1..12 customers), each with
 * its own int32 [N][N] matrix (d_mats [R][N][N], node 0 = start node,
 * asymmetric and non-metric allowed; N * max(D) < 2^31 is the caller's
 * promise, A9).  Each request's Held-Karp table lives in LDS: a team of T
 * threads per request, 256 / T requests per workgroup, one launch for all R.
 * Out: d_tours [R][N-1] (int16 customers) and d_keys [R], per request exactly
 * what vrpms_tsp_dp_run writes for that matrix: the A8 key of the optimum and
 * the lexicographically smallest optimal tour.  No instance and no workspace
 * needed; asynchronous on `stream`.  R = 0 launches nothing.  VRPMS_EINVAL,
 * with nothing launched, for a NULL ctx, R < 0, N outside 2..13, or a NULL
 * buffer with R > 0. */
int vrpms_tsp_batch_dp(vrpms_ctx* ctx, const int32_t* d_mats, int32_t R, int32_t N,
                       uint16_t* d_tours, uint64_t* d_keys, void* stream);

/* Throughput mode of the exact VRP: R independent static
 * CVRP requests of one node count N, 2 <= N <= 13 (n = N - 1 customers, node 0
 * the depot), one fleet size K, 1 <= K <= 64, and one objective, each with its
 * own int32 [N][N] matrix (d_mats [R][N][N], asymmetric and non-metric
 * allowed), demands (d_demand [R][N], entry 0 ignored) and capacities (d_cap
 * [R][K], in vehicle order; they may differ or be 0).  (N + K + 1) * max(D) <
 * 2^31 (A9) and non-negative demands and capacities are the caller's promise.
 * A request's whole state -- the compact Held-Karp table, the route table and
 * the K partition layers -- lives in LDS: a team of `team` threads per request
 * (0 = the measured n -> T table, raised where fewer requests fit the LDS; or
 * 16, 32, 64, 128, 256: the answers do not depend on it), 256 / team requests
 * per workgroup, one launch for all R.  vrpms_vrp_batch_sp_lds gives the
 * launch's dynamic-LDS bytes for (n, K, team) (host only, no context); a
 * launch that needs more than the device has is refused with that byte count
 * in the message.  Out: d_tours [R][N-1+K] and d_keys [R], per request exactly
 * what vrpms_vrp_sp_run writes for that instance (route 0, a separator 0, ...,
 * route K-1, 0, then the unserved customers ascending; its A8 key), and d_durs
 * [R][K], the K route durations, unclamped.  No instance and no workspace
 * needed; asynchronous on `stream`.  R = 0 launches nothing.  VRPMS_EINVAL,
 * with nothing launched and nothing written, for a NULL ctx, R < 0, N outside
 * 2..13, K outside 1..64, an unknown objective or team, a NULL buffer with
 * R > 0, or an LDS need above the device's. */
int vrpms_vrp_batch_sp_lds(int32_t n, int32_t K, int32_t team, uint64_t* bytes);
int vrpms_vrp_batch_sp(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                       const int32_t* d_cap, int32_t R, int32_t N, int32_t K, int32_t objective,
                       int32_t team, int16_t* d_tours, uint64_t* d_keys, int32_t* d_durs,
                       void* stream);

/* Throughput mode of the exact time-dependent TSP: R
 * independent TSP requests of one node count N, 2 <= N <= 12 (n = N - 1
 * customers, node 0 the start node), and one hour count H (1 or 24), each with
 * its own int32 [H][N][N] matrix (d_mats [R][H][N][N], non-negative entries),
 * start time (d_start [R], minutes, >= 0) and horizon (d_horizon [R], minutes,
 * >= 0).  A request's whole time-expanded table -- n 2^(n-1) rows of W hour
 * words -- lives in LDS next to the matrix slices its words can use: a team of
 * `team` threads per request (0 = the measured n -> T table, raised until the
 * workgroup's 256 / T requests fit a fifth of a CU's LDS; or 16, 32, 64, 128,
 * 256: the answers do not depend on it), 256 / team requests per workgroup,
 * one launch for all R.  W,
 * 1 <= W <= 512, is the launch's row width in hour words; W at least every
 * request's (start % 60 + horizon) / 60 + 1 is the caller's promise.  A
 * request's effective horizon is min(horizon, 60 W - 1 - start % 60): a
 * smaller W can prune an answer but never leaves the request's rows.
 * vrpms_tsp_batch_tdp_lds gives the launch's dynamic-LDS bytes for (n, H, W,
 * team) (host only, no context); a launch that needs more than the device has
 * is refused with that byte count in the message.  Out: d_tours [R][N-1] and
 * d_keys [R], per request exactly what vrpms_tsp_tdp_run writes for that
 * matrix, start and (effective) horizon: the A8 key of the optimum among tours
 * of at most that many minutes and A16's tie-ruled tour, or UINT64_MAX and an
 * all-zero tour when no tour fits.  No instance and no workspace needed;
 * asynchronous on `stream`.  R = 0 launches nothing.  VRPMS_EINVAL, with
 * nothing launched and nothing written, for a NULL ctx, R < 0, N outside
 * 2..12, H other than 1 or 24, W outside 1..512, an unknown team, a NULL
 * buffer with R > 0, or an LDS need above the device's. */
int vrpms_tsp_batch_tdp_lds(int32_t n, int32_t H, int32_t W, int32_t team, uint64_t* bytes);
int vrpms_tsp_batch_tdp(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_start,
                        const int32_t* d_horizon, int32_t R, int32_t N, int32_t H, int32_t W,
                        int32_t team, int16_t* d_tours, uint64_t* d_keys, void* stream);

/* Throughput mode of the exact time-dependent VRP: R
 * independent CVRP requests of one node count N, 2 <= N <= 12 (n = N - 1
 * customers, node 0 the depot), one fleet size K, 1 <= K <= 64, one hour count
 * H (1 or 24) and one objective, each with its own int32 [H][N][N] matrix
 * (d_mats [R][H][N][N], non-negative entries), demands (d_demand [R][N], entry
 * 0 ignored), capacities (d_cap [R][K], in vehicle order; they may differ or be
 * 0), start times (d_start [R][K], minutes) and horizon (d_horizon [R],
 * minutes: the bound on every single route).  G, 1 <= G <= K, is the launch's
 * limit on the distinct start times of one request; W, 1 <= W <= 512, its row
 * width in hour words, at least (start % 60 + horizon) / 60 + 1 for every
 * vehicle's start by the caller's promise.  For a start s the effective
 * horizon is min(horizon, 60 W - 1 - s % 60): a smaller W can prune an answer
 * but never leaves the request's rows.  A request's whole state -- the
 * time-expanded table (refilled per distinct start time and per route), the G
 * route tables and the K partition layers -- lives in LDS: a team of `team`
 * threads per request (0 = A20's n -> T table, raised until the workgroup's
 * 256 / T requests fit a fifth of a CU's LDS; or 16, 32, 64, 128, 256: the
 * answers do not depend on it, nor on G, W or the batch), 256 / team requests
 * per workgroup, one launch for all R.  vrpms_vrp_batch_tdsp_lds gives the
 * launch's dynamic-LDS bytes for (n, K, G, H, W, team) (host only, no
 * context); a launch that needs more than the device has is refused with that
 * byte count in the message.  The (N + K + 1) * max(D) + max(start) < 2^31
 * guard (A9) and non-negative demands and capacities are the caller's
 * promise.  Out: d_tours [R][N-1+K], d_keys [R] and d_durs [R][K], per request
 * exactly what vrpms_vrp_tdsp_run writes for that instance and horizon -- A17's
 * key, its tie-ruled tour (route 0, a separator 0, ..., route K-1, 0, then the
 * unserved customers ascending) -- and the K route durations, unclamped, 0 for
 * an empty route.  A request with more than G distinct start times, a negative
 * start time or a negative horizon gets UINT64_MAX, an all-zero tour and
 * durations of -1, and touches nothing else (A17 always has an answer, so all
 * ones means "outside the launch's contract").  No instance and no workspace
 * needed; asynchronous on `stream`.  R = 0 launches nothing.  VRPMS_EINVAL,
 * with nothing launched and nothing written, checked in this order and also
 * with R = 0: a NULL ctx, R < 0, N outside 2..12, K outside 1..64, G outside
 * 1..K, H other than 1 or 24, W outside 1..512, an unknown objective, an
 * unknown team; then, with R > 0, a NULL buffer or an LDS need above the
 * device's. */
int vrpms_vrp_batch_tdsp_lds(int32_t n, int32_t K, int32_t G, int32_t H, int32_t W, int32_t team,
                             uint64_t* bytes);
int vrpms_vrp_batch_tdsp(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                         const int32_t* d_cap, const int32_t* d_start, const int32_t* d_horizon,
                         int32_t R, int32_t N, int32_t K, int32_t G, int32_t H, int32_t W,
                         int32_t objective, int32_t team, int16_t* d_tours, uint64_t* d_keys,
                         int32_t* d_durs, void* stream);

/* Throughput mode of the VRP annealer: R independent CVRP
 * requests of one node count N >= 2 (n = N - 1 customers, node 0 the depot),
 * one fleet size K, 1 <= K <= 64, one hour count H (1 or 24), one objective,
 * one step count and one seed, each with its own int32 [H][N][N] matrix
 * (d_mats [R][H][N][N]), demands (d_demand [R][N], entry 0 ignored),
 * capacities (d_cap [R][K], in vehicle order; they may differ or be 0), start
 * times (d_start [R][K], minutes) and starting inverse temperature (d_inv_t0
 * [R]).  ONE WORKGROUP PER REQUEST: the request's whole instance is staged
 * into LDS once -- the matrix as uint16 with wide = 0, as int32 with wide = 1
 * -- and its four wavefronts run four SA chains of `steps` steps over tours of
 * ntok = n + K - 1 tokens (customers and K - 1 separators, A10): Philox
 * Fisher-Yates starts packed first fit (vrpms_pack_separators' rule), A13's
 * one-word moves, 64 candidates a step priced by full re-evaluation (A5-A8,
 * A3), the temperature multiplied by inv_alpha after every step; no step when
 * ntok < 2.  The Philox counters name the chain (0..3), not the request's row,
 * so a request's answer depends on the request, steps, its inv_t0, inv_alpha,
 * seed and objective alone: not on the launch it rode in nor on its row in it
 * (vrpms_tsp_batch_sa's counters do carry the row).  vrpms_vrp_batch_sa_lds
 * gives the launch's dynamic-LDS bytes for (N, K, H, wide) (host only, no
 * context); a launch that needs more than the device has is refused with that
 * byte count in the message.  (N + K + 1) * max(D) + max(start) < 2^31 and cap
 * + demand < 2^31 (A9) are the caller's promise.  Out, per request, the best
 * (key, chain) of the four: d_tours [R][ntok], d_keys [R] (its A8 key), d_durs
 * [R][K] (the K route durations of that tour, unclamped, 0 for an empty route)
 * and d_veh [R][ntok] (the vehicle of every token, -1 for an unvisited
 * customer, -2 for a separator).  A request whose matrix has a negative entry,
 * or with wide = 0 one above 65535, gets UINT64_MAX, an all-zero tour, zero
 * durations and vehicles of -1, runs no step and touches nothing else.  No
 * instance and no workspace needed; asynchronous on `stream`.  R = 0 launches
 * nothing.  VRPMS_EINVAL, with nothing launched and nothing written, for a
 * NULL ctx, R < 0, N outside 2..65535, K outside 1..64, H other than 1 or 24,
 * an unknown wide or objective, steps < 0, a NULL buffer with R > 0, or an LDS
 * need above the device's. */
int vrpms_vrp_batch_sa_lds(int32_t N, int32_t K, int32_t H, int32_t wide, uint64_t* bytes);
int vrpms_vrp_batch_sa(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                       const int32_t* d_cap, const int32_t* d_start, const float* d_inv_t0,
                       int32_t R, int32_t N, int32_t K, int32_t H, int32_t objective, int32_t wide,
                       int32_t steps, float inv_alpha, uint64_t seed, uint16_t* d_tours,
                       uint64_t* d_keys, int32_t* d_durs, int8_t* d_veh, void* stream);

/* Throughput mode of the VRP genetic algorithm: R
 * independent CVRP requests of one node count N >= 2 (n = N - 1 customers,
 * node 0 the depot), one fleet size K, 1 <= K <= 64, one hour count H (1 or
 * 24), one objective, one population size P, 2 <= P <= 256, one generation
 * count G >= 0, one mutation threshold pmut and one seed, each with its own
 * int32 [H][N][N] matrix (d_mats [R][H][N][N]), demands (d_demand [R][N],
 * entry 0 ignored), capacities (d_cap [R][K], in vehicle order; they may
 * differ or be 0) and start times (d_start [R][K], minutes).  ONE WORKGROUP
 * PER REQUEST: the request's whole instance is staged into LDS once -- the
 * matrix as uint16 with wide = 0, as int32 with wide = 1 -- next to 2P tours
 * of n customers (no separators; the greedy split A5-A7 prices them).  Member
 * i starts as the Philox Fisher-Yates shuffle of 1..n with counters
 * (0xffffffff, 0xffffffff, i, q); generation g is vrpms_ga_generation's on
 * island 0 with child ids 0..P-1 (blocks (g, 0, child, 0) and (g, 0, child,
 * 1): two tournaments of two, OX1, a three-word decode_move mutation iff the
 * third word of the second block < pmut, the P best of parents and children by
 * (key, index) survive; n < 2 copies parent A).  The counters carry no request
 * row, so a request's answer depends on the request, P, G, pmut, seed and
 * objective alone: not on the launch it rode in nor on its row in it.
 * vrpms_vrp_batch_ga_lds gives the launch's dynamic-LDS bytes for (N, K, H,
 * wide, P) (host only, no context); a launch that needs more than the device
 * has is refused with that byte count in the message.  (N + K + 1) * max(D) +
 * max(start) < 2^31 and cap + demand < 2^31 (A9) are the caller's promise.
 * Out, per request, the member of the least (key, index) after the last
 * generation (among the start members for G = 0): d_tours [R][n], d_keys [R]
 * (its A8 key), d_durs [R][K] (the K route durations of that tour, unclamped,
 * 0 for an empty route) and d_veh [R][n] (the vehicle of every gene, -1 for an
 * unvisited customer).  A request whose matrix has a negative entry, or with
 * wide = 0 one above 65535, gets UINT64_MAX, an all-zero tour, zero durations
 * and vehicles of -1, breeds nothing and touches nothing else.  No instance
 * and no workspace needed; asynchronous on `stream`.  R = 0 launches nothing.
 * VRPMS_EINVAL, with nothing launched and nothing written, for a NULL ctx,
 * R < 0, N outside 2..65535, K outside 1..64, H other than 1 or 24, an unknown
 * wide or objective, P outside 2..256, G < 0, a NULL buffer with R > 0, or an
 * LDS need above the device's. */
int vrpms_vrp_batch_ga_lds(int32_t N, int32_t K, int32_t H, int32_t wide, int32_t P,
                           uint64_t* bytes);
int vrpms_vrp_batch_ga(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                       const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                       int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t P, int32_t G,
                       uint32_t pmut, uint64_t seed, uint16_t* d_tours, uint64_t* d_keys,
                       int32_t* d_durs, int8_t* d_veh, void* stream);

/* Throughput mode of the VRP ant colony: R independent CVRP
 * requests of one node count N >= 2 (n = N - 1 customers, node 0 the depot),
 * one fleet size K, 1 <= K <= 64, one hour count H (1 or 24), one objective,
 * one ant count A, 1 <= A <= 256, one iteration count I >= 1, one seed and one
 * set of pheromone parameters (tau0, tau_min, tau_max, evap_shift,
 * bsf_period), each with its own int32 [H][N][N] matrix (d_mats [R][H][N][N]),
 * demands (d_demand [R][N], entry 0 ignored), capacities (d_cap [R][K], in
 * vehicle order; they may differ or be 0) and start times (d_start [R][K],
 * minutes).  ONE WORKGROUP AND ONE COLONY PER REQUEST: the request's whole
 * instance is staged into LDS once -- the matrix as uint16 with wide = 0, as
 * int32 with wide = 1 -- next to tau and eta (uint32 [N][N] each), A tours of
 * n customers (no separators; the greedy split A5-A7 prices them) and the
 * best-so-far tour.  tau starts at tau0 everywhere and eta is vrpms_aco_init's,
 * floor(2^24 / (1 + D)^2) of the hour-0 slice; iteration it = 0..I-1 is
 * vrpms_aco_iteration's on colony 0 of one: ant a, step s draws Philox block
 * (it, 0, a, s), words 0 and 1; the roulette over w_j = (tau[cur][j] >> 8) *
 * eta[cur][j] of the unvisited j picks the first j with w_j > 0 whose prefix
 * sum exceeds (r1 << 32 | r0) % tot, or the first unvisited node when tot = 0;
 * the least (key, ant) is the iteration best and replaces the best-so-far
 * when strictly better; every cell becomes min(tau_max, max(tau_min, tau -
 * (tau >> evap_shift))); then floor(2^30 / (1 + primary)), primary = bits
 * 28..55 of the key, is added on the n + 1 edges depot -> tour -> depot of the
 * iteration best, or of the best-so-far when bsf_period > 0 and (it + 1) %
 * bsf_period == 0.  tau_max <= 2^30 and one deposit per cell per iteration
 * keep tau + deposit at or below 2^31: it never wraps.  With the Python
 * ACORunner's values (tau0 = 2^24, tau_min = 2^12, tau_max = 2^30, evap_shift =
 * 3, bsf_period = 5) a request's row is the best-so-far of a single-colony
 * vrpms_aco_init + I vrpms_aco_iteration calls on the same instance.  The
 * counters carry no request row, so a request's answer depends on the
 * request, A, I, the pheromone parameters, seed and objective alone: not on
 * the launch it rode in nor on its row in it.  vrpms_vrp_batch_aco_lds gives
 * the launch's dynamic-LDS bytes for (N, K, H, wide, A) (host only, no
 * context); a launch that needs more than the device has is refused with that
 * byte count in the message.  (N + K + 1) * max(D) + max(start) < 2^31 and cap
 * + demand < 2^31 (A9) are the caller's promise.  Out, per request, the
 * best-so-far after the last iteration: d_tours [R][n], d_keys [R] (its A8
 * key), d_durs [R][K] (the K route durations of that tour, unclamped, 0 for an
 * empty route) and d_veh [R][n] (the vehicle of every customer of the tour, -1
 * for an unvisited one).  A request whose matrix has a negative entry, or with
 * wide = 0 one above 65535, gets UINT64_MAX, an all-zero tour, zero durations
 * and vehicles of -1, walks no ant and touches nothing else.  No instance and
 * no workspace needed; asynchronous on `stream`.  R = 0 launches nothing.
 * VRPMS_EINVAL, with nothing launched and nothing written, for a NULL ctx,
 * R < 0, N outside 2..65535, K outside 1..64, H other than 1 or 24, an unknown
 * wide or objective, A outside 1..256, I < 1, evap_shift outside 1..31,
 * bsf_period < 0, anything but 0 < tau_min <= tau0 <= tau_max <= 2^30, a NULL
 * buffer with R > 0, or an LDS need above the device's. */
int vrpms_vrp_batch_aco_lds(int32_t N, int32_t K, int32_t H, int32_t wide, int32_t A,
                            uint64_t* bytes);
int vrpms_vrp_batch_aco(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                        const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                        int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t A, int32_t I,
                        uint32_t tau0, uint32_t tau_min, uint32_t tau_max, int32_t evap_shift,
                        int32_t bsf_period, uint64_t seed, uint16_t* d_tours, uint64_t* d_keys,
                        int32_t* d_durs, int8_t* d_veh, void* stream);

/* Throughput mode of a multi-start local search for the VRP (DESIGN.md §2
 * A25): R independent CVRP requests of one node count N >= 2 (n = N - 1
 * customers, node 0 the depot), one fleet size K, 1 <= K <= 64, one hour count
 * H (1 or 24), one objective, one start count S, 1 <= S <= 65535, one round
 * cap `rounds` >= 0 and one seed, each with its own int32 [H][N][N] matrix
 * (d_mats [R][H][N][N]), demands (d_demand [R][N], entry 0 ignored),
 * capacities (d_cap [R][K], in vehicle order; they may differ or be 0) and
 * start times (d_start [R][K], minutes).  ONE WORKGROUP PER REQUEST: the
 * request's whole instance is staged into LDS once -- the matrix as uint16
 * with wide = 0, as int32 with wide = 1 -- next to two tours of n customers
 * per wavefront (no separators; the greedy split A5-A7 prices them).
 * Wavefront w descends the starts w, w + 4, ...: start s is
 * vrpms_vrp_batch_ga's member s, the Philox Fisher-Yates shuffle of 1..n with
 * counters (0xffffffff, 0xffffffff, s, q).  A round prices every move (typ, i,
 * j) on positions 0..n-1 -- swap (typ 0) and 2-opt (typ 1) with i < j,
 * relocate (typ 2) with i != j, each the A8 key of the moved tour -- and takes
 * the least (key, typ, i, j): a key below the tour's applies the move and the
 * next round follows, otherwise the descent has stopped at a local optimum.  A
 * descent also stops once `rounds` moves are applied; it then counts as capped
 * (it was not proven optimal: no further scan ran).  n < 2 has no moves and is
 * never capped.  The answer is the least (key, s) over the S end tours.  The
 * counters carry no request row, so a request's answer depends on the request,
 * S, rounds, seed and objective alone: not on the launch it rode in nor on its
 * row in it.  With rounds = 0 and 2 <= S <= 256 it is vrpms_vrp_batch_ga's at
 * P = S, G = 0.  vrpms_vrp_batch_ls_lds gives the launch's dynamic-LDS bytes
 * for (N, K, H, wide) (host only, no context), never more than
 * vrpms_vrp_batch_sa_lds of the same shape; a launch that needs more than the
 * device has is refused with that byte count in the message.  (N + K + 1) *
 * max(D) + max(start) < 2^31 and cap + demand < 2^31 (A9) are the caller's
 * promise.  Out, per request: d_tours [R][n] (the answer), d_keys [R] (its A8
 * key), d_durs [R][K] (the K route durations of that tour, unclamped, 0 for an
 * empty route), d_veh [R][n] (the vehicle of every customer of the tour, -1
 * for an unvisited one) and d_info [R][2] (the answer's start s, and the
 * number of capped descents among the S).  A request whose matrix has a
 * negative entry, or with wide = 0 one above 65535, gets UINT64_MAX, an
 * all-zero tour, zero durations, vehicles of -1 and d_info = (-1, 0), descends
 * nothing and touches nothing else.  No instance and no workspace needed;
 * asynchronous on `stream`.  R = 0 launches nothing.  VRPMS_EINVAL, with
 * nothing launched and nothing written, for a NULL ctx, R < 0, N outside
 * 2..65535, K outside 1..64, H other than 1 or 24, an unknown wide or
 * objective, S outside 1..65535, rounds < 0, a NULL buffer with R > 0, or an
 * LDS need above the device's. */
int vrpms_vrp_batch_ls_lds(int32_t N, int32_t K, int32_t H, int32_t wide, uint64_t* bytes);
int vrpms_vrp_batch_ls(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                       const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                       int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t S,
                       int32_t rounds, uint64_t seed, uint16_t* d_tours, uint64_t* d_keys,
                       int32_t* d_durs, int8_t* d_veh, int32_t* d_info, void* stream);

/* Throughput mode of a multi-start local search over separator tours for the
 * VRP: vrpms_vrp_batch_ls's descent on the tours
 * vrpms_vrp_batch_sa anneals.  The requests, their buffers, N, K, H, wide,
 * objective, S, rounds and seed are vrpms_vrp_batch_ls's; a tour has
 * L = n + K - 1 tokens, the n = N - 1 customers and K - 1 separators (the
 * token 0, A10), and L <= 65535.  ONE WORKGROUP PER REQUEST, the instance in
 * LDS next to two tours of L tokens per wavefront.  Wavefront w descends the
 * starts w, w + 4, ...: start s is vrpms_vrp_batch_ls's start s -- the Philox
 * Fisher-Yates shuffle of 1..n with counters (0xffffffff, 0xffffffff, s, q) --
 * packed first-fit into the K routes with a separator between them, as
 * vrpms_vrp_batch_sa packs chain w's (each customer, in shuffle order, to the
 * first route with room for it, to the last when none has).  A round prices
 * every move (typ, i, j) on positions 0..L-1, separators moved like customers
 * -- swap (typ 0) and 2-opt (typ 1) with i < j, relocate (typ 2) with i != j,
 * each the A8 key of the moved tour -- and takes the least (key, typ, i, j): a
 * key below the tour's applies the move and the next round follows, otherwise
 * the descent has stopped at a local optimum.  A descent also stops once
 * `rounds` moves are applied; it then counts as capped.  L < 2 has no moves
 * and is never capped.  The answer is the least (key, s) over the S end tours.
 * The counters carry no request row, so a request's answer depends on the
 * request, S, rounds, seed and objective alone: not on the launch it rode in
 * nor on its row in it.  With K = 1 it is vrpms_vrp_batch_ls's; with S = 4 and
 * rounds = 0 it is vrpms_vrp_batch_sa's at steps = 0.
 * vrpms_vrp_batch_lsr_lds gives the launch's dynamic-LDS bytes for (N, K, H,
 * wide) (host only, no context), never more than vrpms_vrp_batch_sa_lds of the
 * same shape; a launch that needs more than the device has is refused with
 * that byte count in the message.  (N + K + 1) * max(D) + max(start) < 2^31
 * and cap + demand < 2^31 (A9) are the caller's promise.  Out, per request:
 * d_tours [R][L] (the answer), d_keys [R] (its A8 key), d_durs [R][K] (the K
 * route durations of that tour, unclamped, 0 for an empty route), d_veh [R][L]
 * (the vehicle of every token of the tour, -1 for an unvisited customer, -2
 * for a separator) and d_info [R][2] (the answer's start s, and the number of
 * capped descents among the S).  A request whose matrix has a negative entry,
 * or with wide = 0 one above 65535, gets UINT64_MAX, an all-zero tour, zero
 * durations, vehicles of -1 and d_info = (-1, 0), descends nothing and touches
 * nothing else.  No instance and no workspace needed; asynchronous on
 * `stream`.  R = 0 launches nothing.  VRPMS_EINVAL, with nothing launched and
 * nothing written, for a NULL ctx, R < 0, N outside 2..65535, K outside 1..64,
 * N + K - 2 above 65535, H other than 1 or 24, an unknown wide or objective, S
 * outside 1..65535, rounds < 0, a NULL buffer with R > 0, or an LDS need above
 * the device's. */
int vrpms_vrp_batch_lsr_lds(int32_t N, int32_t K, int32_t H, int32_t wide, uint64_t* bytes);
int vrpms_vrp_batch_lsr(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                        const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                        int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t S,
                        int32_t rounds, uint64_t seed, uint16_t* d_tours, uint64_t* d_keys,
                        int32_t* d_durs, int8_t* d_veh, int32_t* d_info, void* stream);

/* Batched VRP local search over PLAIN separator tours on a static matrix, with
 * delta pricing (spec A28): vrpms_vrp_batch_lsr's requests,
 * buffers, arguments, mapping, starts, moves, answer and refusal row, with H
 * kept in the argument list and required to be 1 (an hour-indexed launch keeps
 * vrpms_vrp_batch_lsr).  A tour of n customers and K - 1 separators is plain
 * when the customers between separator g - 1 and separator g weigh at most
 * cap[g] for every g = 0..K-1, so that the separators alone decide the routes.
 * A round considers vrpms_vrp_batch_lsr's moves in its order, but a move whose
 * moved tour is not plain is no candidate; the rest are priced by their A8 key
 * -- from per-wavefront prefix rows, never by a walk -- and the least (key,
 * typ, i, j) is applied while it is below the tour's key.  A start that is not
 * plain (the first fit found no room for a customer) does not descend: its end
 * tour is its start tour with its A8 key, and it is never capped.  With every
 * capacity at least the total demand every tour is plain and the rows are
 * vrpms_vrp_batch_lsr's bit for bit; with K = 1 and such a capacity they are
 * vrpms_vrp_batch_ls's.  vrpms_vrp_batch_lsf_lds gives the launch's
 * dynamic-LDS bytes for (N, K, wide) (host only, no context); a launch that
 * needs more than the device has is refused with that byte count.
 * VRPMS_EINVAL as for vrpms_vrp_batch_lsr, and for H other than 1. */
int vrpms_vrp_batch_lsf_lds(int32_t N, int32_t K, int32_t wide, uint64_t* bytes);
int vrpms_vrp_batch_lsf(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                        const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                        int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t S,
                        int32_t rounds, uint64_t seed, uint16_t* d_tours, uint64_t* d_keys,
                        int32_t* d_durs, int8_t* d_veh, int32_t* d_info, void* stream);

/* vrpms_vrp_batch_lsr by another mapping: the same requests,
 * buffers and arguments, and per request the identical d_tours, d_keys, d_durs,
 * d_veh and d_info rows, refusal rows included -- A26 fixes the starts, the
 * rounds and the least (key, s), not which threads run them.  Here a request's
 * S starts are spread over min(G, S) WORKGROUPS, workgroup g descending the
 * starts g, g + G, ..., and a workgroup's 256 threads price one round of one
 * tour together (thread t the move ids [t per, (t + 1) per), per =
 * ceil(2 L (L - 1) / 256)), one workgroup barrier a round.  Each workgroup
 * leaves its best (key, s, capped count, tour) in the workspace; a second
 * launch on the same stream, one workgroup per request, takes the least
 * (key, s), sums the capped counts and writes the outputs.  For few requests
 * that occupies R * min(G, S) workgroups instead of R.
 * vrpms_vrp_batch_lsr_spread_lds gives either launch's dynamic-LDS bytes for
 * (N, K, H, wide) (host only, no context): never more than
 * vrpms_vrp_batch_lsr_lds of the same shape, so A26's domain holds.
 * vrpms_vrp_batch_lsr_spread_work gives the workspace bytes of R requests at G
 * workgroups each, R * G * (16 + 2 * align8(N + K - 2)) (host only;
 * VRPMS_EINVAL for R < 0, a shape outside vrpms_vrp_batch_lsr_lds's, G outside
 * 1..65535 or R * G above 2^31 - 1).  d_work: work_bytes bytes of device
 * memory, 8-byte aligned, at least vrpms_vrp_batch_lsr_spread_work(R, N, K,
 * min(G, S)); its contents before and after the call mean nothing.
 * Asynchronous on `stream`.  R = 0 launches nothing.  VRPMS_EINVAL, with
 * nothing launched and nothing written, for everything vrpms_vrp_batch_lsr
 * refuses, G outside 1..65535, a NULL, misaligned or too small workspace with
 * R > 0, or R * min(G, S) above 2^31 - 1. */
int vrpms_vrp_batch_lsr_spread_lds(int32_t N, int32_t K, int32_t H, int32_t wide, uint64_t* bytes);
int vrpms_vrp_batch_lsr_spread_work(int32_t R, int32_t N, int32_t K, int32_t G, uint64_t* bytes);
int vrpms_vrp_batch_lsr_spread(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                               const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                               int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t S,
                               int32_t rounds, uint64_t seed, int32_t G, void* d_work,
                               uint64_t work_bytes, uint16_t* d_tours, uint64_t* d_keys,
                               int32_t* d_durs, int8_t* d_veh, int32_t* d_info, void* stream);

/* vrpms_vrp_batch_lsf by vrpms_vrp_batch_lsr_spread's mapping (DESIGN.md
 * §4.3x): the same requests, buffers and arguments as vrpms_vrp_batch_lsf, and
 * per request the identical d_tours, d_keys, d_durs, d_veh and d_info rows,
 * refusal rows included -- A28 fixes the starts, the rounds and the least
 * (key, s), not which threads run them.  A request's S starts are spread over
 * min(G, S) WORKGROUPS, workgroup g descending the starts g, g + G, ..., and a
 * workgroup's 256 threads price one round of one plain tour together from the
 * wavefronts' rows (thread t the move ids [t per, (t + 1) per), per =
 * ceil(2 L (L - 1) / 256)), one workgroup barrier a round.  Each workgroup
 * leaves its best (key, s, capped count, tour) in the workspace; a second
 * launch on the same stream, one workgroup per request, takes the least
 * (key, s), sums the capped counts and writes the outputs.
 * vrpms_vrp_batch_lsf_spread_lds gives either launch's dynamic-LDS bytes for
 * (N, K, wide) (host only, no context): never more than
 * vrpms_vrp_batch_lsf_lds of the same shape, so A28's domain holds.
 * vrpms_vrp_batch_lsf_spread_work gives the workspace bytes of R requests at G
 * workgroups each, R * G * (16 + 2 * align8(N + K - 2)) (host only;
 * VRPMS_EINVAL for R < 0, a shape outside vrpms_vrp_batch_lsf_lds's, G outside
 * 1..65535 or R * G above 2^31 - 1).  d_work: work_bytes bytes of device
 * memory, 8-byte aligned, at least vrpms_vrp_batch_lsf_spread_work(R, N, K,
 * min(G, S)); its contents before and after the call mean nothing.
 * Asynchronous on `stream`.  R = 0 launches nothing.  VRPMS_EINVAL, with
 * nothing launched and nothing written, for everything vrpms_vrp_batch_lsf
 * refuses, G outside 1..65535, a NULL, misaligned or too small workspace with
 * R > 0, or R * min(G, S) above 2^31 - 1. */
int vrpms_vrp_batch_lsf_spread_lds(int32_t N, int32_t K, int32_t wide, uint64_t* bytes);
int vrpms_vrp_batch_lsf_spread_work(int32_t R, int32_t N, int32_t K, int32_t G, uint64_t* bytes);
int vrpms_vrp_batch_lsf_spread(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_demand,
                               const int32_t* d_cap, const int32_t* d_start, int32_t R, int32_t N,
                               int32_t K, int32_t H, int32_t objective, int32_t wide, int32_t S,
                               int32_t rounds, uint64_t seed, int32_t G, void* d_work,
                               uint64_t work_bytes, uint16_t* d_tours, uint64_t* d_keys,
                               int32_t* d_durs, int8_t* d_veh, int32_t* d_info, void* stream);

/* Throughput mode of a multi-start local search for the TSP with Or-opt moves
 * and delta pricing: R independent TSP requests of
 * one node count N >= 2 (n = N - 1 customers, node 0 the start node), one hour
 * count H (1 or 24), one start count S, 1 <= S <= 65535, one round cap `rounds`
 * >= 0, one move mask `moves`, 1..31, and one seed, each with its own int32
 * [H][N][N] matrix (d_mats [R][H][N][N]) and start time (d_start [R], minutes,
 * >= 0).  A tour is a permutation of 1..n on positions 0..n-1, its duration
 * spec.eval_tsp's (A4) from the start time, its key spec.tsp_key of it (A8:
 * min(duration, 2^28 - 1) << 28); tours compare by key.  ONE WORKGROUP PER
 * REQUEST: the matrix is staged into LDS once -- as uint16 with wide = 0, as
 * int32 with wide = 1.  Wavefront w descends the starts w, w + 4, ...: start s
 * is vrpms_vrp_batch_ls's start s, the Philox Fisher-Yates shuffle of 1..n with
 * counters (0xffffffff, 0xffffffff, s, q).  A round prices the moves (typ, i,
 * j) of every type whose bit `moves` has set (bit t: typ t) -- swap (typ 0) and
 * 2-opt (typ 1) with i < j, relocate (typ 2) with i != j, and Or-opt of m = 2
 * (typ 3) and m = 3 (typ 4) customers: with seg = p[i:i+m] and rest = p[:i] +
 * p[i+m:] the moved tour is rest[:j] + seg + rest[j:], 0 <= i, j <= n - m,
 * j != i (relocate is that formula at m = 1; a type has no moves when n <= m)
 * -- and takes the least (key, typ, i, j): a key below the tour's applies the
 * move and the next round follows, otherwise the descent has stopped at a
 * local optimum.  A descent also stops once `rounds` moves are applied; it then
 * counts as capped.  n < 2 has no moves and is never capped.  The answer is
 * the least (key, s) over the S end tours.  No candidate is walked in full: on
 * a static matrix its duration is the tour's plus an exact integer delta of a
 * fixed number of edges and prefix sums, on an hour-indexed one the walk
 * starts at the first changed position.  The counters carry no request row, so
 * a request's answer depends on the request, S, rounds, moves and seed alone:
 * not on the launch it rode in nor on its row in it.  With moves = 7 the tour,
 * s and the capped count are vrpms_vrp_batch_ls's at K = 1, zero demands, any
 * capacity >= 0, vehicle start = the start time and objective sum; only the
 * key's secondary field differs (0 here, the duration there).
 * vrpms_tsp_batch_lso_lds gives the launch's dynamic-LDS bytes for (N, H, wide)
 * (host only, no context): align16(H N N (wide ? 4 : 2)) for the matrix, per
 * wavefront (four of them) two int32 rows (H = 1) or one (H = 24) of
 * align4(n + 2) words, a uint16 tour of align8(n + 2) and one of align8(n)
 * genes, and 4 * 16 bytes of records; a launch that needs more than the device
 * has is refused with that byte count in the message.  (N + 2) * max(D) +
 * start < 2^31 (A9 with K = 1) is the caller's promise.  Out, per request:
 * d_tours [R][n] (the answer), d_keys [R] (its key), d_durs [R] (its duration,
 * unclamped) and d_info [R][2] (the answer's start s, and the number of capped
 * descents among the S).  A request whose matrix has a negative entry, or with
 * wide = 0 one above 65535, gets UINT64_MAX, an all-zero tour, duration 0 and
 * d_info = (-1, 0), descends nothing and touches nothing else.  No instance
 * and no workspace needed; asynchronous on `stream`.  R = 0 launches nothing.
 * VRPMS_EINVAL, with nothing launched and nothing written, for a NULL ctx,
 * R < 0, N outside 2..65535, H other than 1 or 24, an unknown wide, S outside
 * 1..65535, rounds < 0, moves outside 1..31, a NULL buffer with R > 0, or an
 * LDS need above the device's. */
int vrpms_tsp_batch_lso_lds(int32_t N, int32_t H, int32_t wide, uint64_t* bytes);
int vrpms_tsp_batch_lso(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_start, int32_t R,
                        int32_t N, int32_t H, int32_t wide, int32_t S, int32_t rounds,
                        int32_t moves, uint64_t seed, uint16_t* d_tours, uint64_t* d_keys,
                        int32_t* d_durs, int32_t* d_info, void* stream);

/* vrpms_tsp_batch_lso by another mapping: the same requests,
 * the same arguments and, per request, the identical d_tours, d_keys, d_durs
 * and d_info rows, refusal rows included -- but a request's S starts are
 * spread over min(G, S) workgroups, workgroup g descending the starts g,
 * g + G, ... one after the other with all 256 threads pricing one round of one
 * tour (thread t the enabled move ids [t per, (t + 1) per), per = ceil(moves /
 * 256)), and leaves its best (key, s, capped count, duration, tour) in the
 * workspace; a second launch on the same stream, one workgroup per request,
 * takes the least (key, s), sums the capped counts and writes the outputs.
 * For few requests that occupies R * min(G, S) workgroups instead of R.
 * vrpms_tsp_batch_lso_spread_lds gives the first launch's dynamic-LDS bytes
 * for (N, H, wide) (host only, no context): the matrix, per wavefront the
 * int32 rows and the uint16 tour of align8(n + 2) genes as above, and 2 * 4 *
 * 16 bytes of round records; never more than vrpms_tsp_batch_lso_lds of the
 * same shape, so A27's domain holds.  The second launch uses no LDS.
 * vrpms_tsp_batch_lso_spread_work gives the workspace bytes of R requests at G
 * workgroups each, R * G * (24 + 2 * align8(N - 1)) (host only; VRPMS_EINVAL
 * for R < 0, N outside 2..65535, G outside 1..65535 or R * G above 2^31 - 1).
 * d_work: work_bytes bytes of device memory, 8-byte aligned, at least
 * vrpms_tsp_batch_lso_spread_work(R, N, min(G, S)); its contents before and
 * after the call mean nothing.  Asynchronous on `stream`.  R = 0 launches
 * nothing.  VRPMS_EINVAL, with nothing launched and nothing written, for
 * everything vrpms_tsp_batch_lso refuses, G outside 1..65535, a NULL,
 * misaligned or too small workspace with R > 0, or R * min(G, S) above
 * 2^31 - 1. */
int vrpms_tsp_batch_lso_spread_lds(int32_t N, int32_t H, int32_t wide, uint64_t* bytes);
int vrpms_tsp_batch_lso_spread_work(int32_t R, int32_t N, int32_t G, uint64_t* bytes);
int vrpms_tsp_batch_lso_spread(vrpms_ctx* ctx, const int32_t* d_mats, const int32_t* d_start,
                               int32_t R, int32_t N, int32_t H, int32_t wide, int32_t S,
                               int32_t rounds, int32_t moves, uint64_t seed, int32_t G, void* d_work,
                               uint64_t work_bytes, uint16_t* d_tours, uint64_t* d_keys,
                               int32_t* d_durs, int32_t* d_info, void* stream);

/* ------------------------------------------------------------------------
 * Populations and the island model.  A pool is a set of
 * tours with their A8 keys: SA chains, a GA population ([islands][pop],
 * each island sorted by (key, index)), or the per-colony bests of ACO.
 * Everything here runs on the device, so the search path issues no torch
 * compute (torch only owns the buffers).
 * ---------------------------------------------------------------------- */
typedef struct {
  uint16_t* tours;   /* [count][n] */
  uint64_t* keys;    /* [count] */
  int32_t count;     /* rows */
  int32_t n;         /* customers per tour */
  int32_t groups;    /* VRPMS_INJECT_SORTED: `groups` sorted groups of count / groups rows */
} vrpms_pool;

/* How migrants enter a pool (vrpms_pool_inject / vrpms_island_exchange). */
#define VRPMS_INJECT_WORST 0  /* migrant e replaces the e-th worst row, by (key desc, index asc) */
#define VRPMS_INJECT_SORTED 1 /* migrant e takes slot count/groups - 1 - e/groups of group
                                 e % groups; every group is re-sorted by (key, index) */
#define VRPMS_INJECT_BETTER 2 /* migrant e replaces row e (< count) when its key is smaller */

/* Start tours (the front-end's initial SA chains / GA population, the
 * bench's candidate batch): row r of `count` is the Philox Fisher-Yates
 * permutation of the tokens 1..n+n_sep -- for i = n+n_sep-1 .. 1 swap t[i]
 * and t[w % (i+1)], w word (i & 3) of philox4x32_10((i >> 2, 0xfffffffe, r,
 * stream_id), seed) -- with tokens above n written as 0 (A10 route
 * separators; n_sep = 0 for plain permutations), as uint8 (tour_bytes 1,
 * n + n_sep <= 255) or uint16 rows of `ld` elements. */
int vrpms_random_tours(vrpms_ctx* ctx, int64_t count, int32_t n, int32_t n_sep, int64_t ld,
                       int32_t tour_bytes, uint64_t seed, uint32_t stream_id, void* d_tours,
                       void* stream);

/* Feasible separator tours for the SA start: row r of d_out [count][n+n_sep]
 * is row r of d_in [count][n] (customers only) with a separator (0) where
 * the loaded instance's greedy split would open the next route (at most
 * n_sep, never before the first customer; route i's capacity is
 * capacities[min(i, K-1)]) and the unused separators appended -- same cost
 * as the input while the fleet lasts (oracle/spec.py insert_separators). */
int vrpms_insert_separators(vrpms_ctx* ctx, const uint16_t* d_in, int64_t count, int32_t n,
                            int32_t n_sep, uint16_t* d_out, void* stream);

/* First-fit start tours (oracle/spec.py pack_separators): each customer of
 * row r of d_in [count][n], in order, joins the first of n_sep + 1 routes
 * with room for it (the last route when none has); d_out [count][n + n_sep]
 * lists the routes in order with one separator between consecutive routes.
 * Packs a fleet with little spare capacity into K routes, where
 * vrpms_insert_separators (next fit) runs out of vehicles on a random order. */
int vrpms_pack_separators(vrpms_ctx* ctx, const uint16_t* d_in, int64_t count, int32_t n,
                          int32_t n_sep, uint16_t* d_out, void* stream);

/* The E best rows of a pool by (key, index), ascending: d_tours [E][n],
 * d_keys [E] (0 < E <= min(count, 1024)). */
int vrpms_pool_elites(vrpms_ctx* ctx, const vrpms_pool* pool, int32_t E, uint16_t* d_tours,
                      uint64_t* d_keys, void* stream);

/* Put E migrants (d_tours [E][n], d_keys [E]) into a pool by `mode`. */
int vrpms_pool_inject(vrpms_ctx* ctx, const vrpms_pool* pool, int32_t mode,
                      const uint16_t* d_tours, const uint64_t* d_keys, int32_t E, void* stream);

/* Island message of E elites of n customers: [E keys u64][E x n tours u16],
 * zero padded to a multiple of 16 bytes.  Returns its size in bytes. */
int64_t vrpms_island_msg_bytes(int32_t E, int32_t n);

/* The E elites of `pool` as one message (d_msg, vrpms_island_msg_bytes). */
int vrpms_island_pack(vrpms_ctx* ctx, const vrpms_pool* pool, int32_t E, void* d_msg,
                      void* stream);

/* The E best of `world` gathered messages (d_msgs = world messages back to
 * back, in rank order) by (key, rank, position in the message). */
int vrpms_island_merge(vrpms_ctx* ctx, const void* d_msgs, int32_t world, int32_t E, int32_t n,
                       uint16_t* d_tours, uint64_t* d_keys, void* stream);

/* RCCL communicator of the island model: rank 0 calls vrpms_island_unique_id
 * (128 opaque bytes), shares them with every rank (the front-end uses its
 * torch.distributed group), and every rank calls vrpms_island_init.  One
 * process per GPU; the communicator runs over xGMI on an MI355X node.  The
 * communicator is created non-blocking with a deadline
 * (VRPMS_OPT_ISLAND_TIMEOUT_S): VRPMS_ETIMEOUT, and no communicator, when
 * the ranks did not all join in time. */
int vrpms_island_unique_id(void* out128);
int vrpms_island_init(vrpms_ctx* ctx, const void* unique_id, int32_t rank, int32_t world);
/* world of the context's communicator, 0 when none was initialised */
int vrpms_island_world(vrpms_ctx* ctx);

/* One migration: the E elites of `src` are packed, all-gathered over the
 * context's RCCL communicator (a local copy when none: world 1), merged by
 * (key, rank, position) and injected into `dst` by `mode` -- every rank ends
 * with the same E migrants.  SA: src = bests, dst = current chains, WORST;
 * GA: src = dst = population, SORTED; ACO: src = dst = colony bests, BETTER.
 * (SURVEY.md §8b names this vrpms_island_exchange(ctx, n_elite, stream); the
 * pools are passed per call instead of being registered in the context.) */
int vrpms_island_exchange(vrpms_ctx* ctx, const vrpms_pool* src, const vrpms_pool* dst,
                          int32_t mode, int32_t E, void* stream);

/* Roofline probe (measurement only): `blocks` x 1024 lanes each issue
 * 4 * iters random ds_read_b64 gathers over a `slots`-entry u64 table staged
 * in LDS -- the measured random LDS-gather ceiling R_gather of SURVEY.md §8d. */
int vrpms_probe_lds_gather(vrpms_ctx* ctx, const uint64_t* d_table, int32_t slots, int32_t iters,
                           int32_t blocks, uint64_t* d_sink, void* stream);

/* Roofline probe (measurement only): `blocks` x 256 lanes each issue
 * 8 * iters random 2-byte global loads over a `slots`-entry uint16 table --
 * the measured L2-gather ceiling of the staged kernels (cfg 3 / cfg 4). */
int vrpms_probe_l2_gather(vrpms_ctx* ctx, const uint16_t* d_table, int32_t slots, int32_t iters,
                          int32_t blocks, uint64_t* d_sink, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VRPMS_H */
