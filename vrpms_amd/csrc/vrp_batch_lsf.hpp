// What vrp_batch_lsf.hip and vrp_batch_lsf_spread.hip (A28, DESIGN.md §4.3v,
// §4.3x) add to vrp_batch_lsr's descent
// (A26): the rows a wavefront keeps of its current PLAIN tour -- a tour of n
// customers and K - 1 separators in which the customers between separator
// g - 1 and separator g weigh at most cap[g], so that the separators alone
// decide the routes -- and the pricing of a candidate from those rows, with
// no walk along the tour.
//
// The padded tour P holds node 0 at P[0] and P[L + 1] and token q at P[q + 1];
// a separator is the token 0, which reads as node 0, and the kernel has zeroed
// the matrix cell 0 -> 0, so the closed chain P[0] -> ... -> P[L + 1] is the
// routes' closed chains one after the other: its length is the duration sum.
// Separator g - 1 stands at the padded index S[g] (S[0] = 0, S[K] = L + 1), so
// segment g is P[S[g] + 1 .. S[g + 1] - 1].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "batch_launch.hpp"
#include "batch_ls.hpp"
#include "batch_stage.hpp"
#include "common.hpp"
#include "tour.hpp"
#include "tsp_batch_lso.hpp"
#include "vrp_batch_lsr.hpp"

namespace vrpms {

// The kernel's own parts behind the instance and the waves' records, per
// wavefront: int32 rows F, B, W of align4(L + 2) words and tables FD, BD, LD,
// PM, SM of align4(K + 1) words; uint16 rows P of align8(L + 2), the best end
// tour of align8(L) and S of align8(K + 1); the uint8 row G of align8(L + 2).
// The host sums them, the kernel steps through them (I as in BatchInstParts).
template <typename I>
struct BatchLsfParts {
  I row_words, tab_words, ppad, bpad, spad, gpad;
  __host__ __device__ BatchLsfParts(I L, I K) {
    row_words = batch_align<I>(L + 2, 4);
    tab_words = batch_align<I>(K + 1, 4);
    ppad = batch_align<I>(L + 2, 8);
    bpad = batch_align<I>(L, 8);
    spad = batch_align<I>(K + 1, 8);
    gpad = batch_align<I>(L + 2, 8);
  }
  __host__ __device__ I words() const { return 3 * row_words + 5 * tab_words; }
  __host__ __device__ I halves() const { return ppad + bpad + spad; }
  __host__ __device__ I wave_bytes() const { return 4 * words() + 2 * halves() + gpad; }
};

inline size_t batch_lsf_lds(int N, int K, int wide) {
  return batch_inst_bytes(N, K, 1, wide) + 4 * sizeof(BatchLsWave) +
         4 * BatchLsfParts<size_t>((size_t)(N - 1 + K - 1), (size_t)K).wave_bytes();
}

// a wavefront's rows of its current tour
struct LsfRows {
  int32_t *F, *B;      // [L + 2] forward and backward prefix sums of the chain's edges
  uint32_t* W;         // [L + 2] prefix sums of the demands, a separator weighing 0 (mod 2^32)
  int32_t *FD, *BD;    // [K] segment g forwards and backwards: F and B between S[g] and S[g + 1]
  uint32_t* LD;        // [K] segment g's load
  int32_t *PM, *SM;    // [K + 1] PM[g] = max FD[0 .. g - 1], SM[g] = max FD[g .. K - 1]
  uint16_t *P, *S;     // the padded tour [L + 2]; the separators' padded indices [K + 1]
  uint8_t* G;          // [L + 2] G[p] = the separators among P[1 .. p - 1]: p's segment
};

constexpr uint32_t kLsfLoadTop = 0x80000000u;   // above every capacity

// The rows and tables of the plain tour in r.P (L tokens, K - 1 of them
// separators), rebuilt by the whole wavefront -> the chain's length, the
// duration sum; `dmax` gets the longest route.  The caller has set P[0] and
// P[L + 1] to 0.
template <typename Mat>
VRPMS_DEV int lsf_rows(const Mat& D, const int32_t* dem, const LsfRows& r, int L, int K, int lane,
                       int& dmax) {
  const int sum = lso_rows_static(D, r.P, L, r.F, r.B, lane);
  // The demands by a scan of which only the low half is kept -- a chunk's
  // demands may sum past 2^32 (any load may stand on a start's last route),
  // and W is meant mod 2^32 --, the separators apart from them, by a ballot:
  // no carry of the one reaches the other
  uint32_t cw = 0, cg = 0;
  if (lane == 0) {
    r.W[0] = 0;
    r.S[0] = 0;
    r.S[K] = (uint16_t)(L + 1);
  }
  for (int base = 1; base <= L + 1; base += 64) {
    const int p = base + lane;
    uint64_t v = 0;
    uint32_t tok = 1;
    if (p <= L) {
      tok = r.P[p];
      v = tok ? (uint64_t)(uint32_t)dem[tok] : 0ull;
    }
    const uint64_t seps = __builtin_amdgcn_ballot_w64(tok == 0);
    const uint64_t tot = wave_scan_add_u64(v);
    if (p <= L + 1) {
      // the separators before p: the earlier chunks' and the lower lanes'
      const uint32_t g = cg + __builtin_amdgcn_mbcnt_hi((uint32_t)(seps >> 32),
                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)seps, 0u));
      r.W[p] = cw + (uint32_t)v;
      r.G[p] = (uint8_t)g;
      if (tok == 0) r.S[g + 1] = (uint16_t)p;
    }
    cw += (uint32_t)tot;
    cg += (uint32_t)__builtin_popcountll(seps);
  }
  wave_sync();
  // one lane per route, then the running maxima over the lanes
  int fd = 0;
  if (lane < K) {
    const int s0 = r.S[lane], s1 = r.S[lane + 1];
    fd = r.F[s1] - r.F[s0];
    r.FD[lane] = fd;
    r.BD[lane] = r.B[s1] - r.B[s0];
    r.LD[lane] = r.W[s1] - r.W[s0];
  }
  int pm = fd, sm = fd;   // durations are >= 0 and the lanes past K hold 0
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(pm, d), dn = __shfl_down(sm, d);
    if (lane >= d) pm = max(pm, up);
    if (lane + d < 64) sm = max(sm, dn);
  }
  if (lane < K) {
    r.PM[lane + 1] = pm;
    r.SM[lane] = sm;
  }
  if (lane == 0) {
    r.PM[0] = 0;
    r.SM[K] = 0;
  }
  dmax = __builtin_amdgcn_readlane(sm, 0);
  wave_sync();
  return sum;
}

// Whether the tour of the rows is plain: lane g adds up segment g's demands
// (in 64 bits: a start tour's last route may hold any load)
VRPMS_DEV bool lsf_plain(const int32_t* dem, const int32_t* cap, const LsfRows& r, int K, int lane) {
  bool ok = true;
  if (lane < K) {
    int64_t load = 0;
    for (int p = r.S[lane] + 1; p < (int)r.S[lane + 1]; ++p) load += dem[r.P[p]];
    ok = load <= (int64_t)cap[lane];
  }
  return __builtin_amdgcn_ballot_w64(!ok) == 0;
}

// The routes the move's span [lo, hi] touches, walked segment by segment
// through the ranges of the current tour that make up the moved one.  State:
// the open route k with its load, its duration so far and its last node.
template <typename Mat>
struct LsfWalk {
  const Mat& D;
  const int32_t* cap;
  const LsfRows& r;
  int k, dur, mx;
  uint32_t load, last;
  bool ok;

  VRPMS_DEV void add(uint32_t w) { load = min(load + w, kLsfLoadTop); }
  VRPMS_DEV void close() {
    dur += D(0, last, 0);
    ok &= (int64_t)load <= (int64_t)cap[k];
    mx = max(mx, dur);
    ++k;
    load = 0;
    dur = 0;
    last = 0;
  }
  // a whole segment g that keeps its customers: forwards or mirrored
  VRPMS_DEV void whole(int g, const int32_t* durs) {
    ok &= (int64_t)r.LD[g] <= (int64_t)cap[k];
    mx = max(mx, durs[g]);
    ++k;
  }
  // P[u .. v], u <= v, customers only, joined to the open route
  VRPMS_DEV void piece_f(int u, int v) {
    dur += D(0, last, (uint32_t)r.P[u]) + r.F[v] - r.F[u];
    add(r.W[v] - r.W[u - 1]);
    last = r.P[v];
  }
  // P[u], P[u - 1], ..., P[v], u >= v, customers only
  VRPMS_DEV void piece_r(int u, int v) {
    dur += D(0, last, (uint32_t)r.P[u]) + r.B[u] - r.B[v];
    add(r.W[u] - r.W[v - 1]);
    last = r.P[v];
  }
  // the padded range [x, y] of the current tour, forwards; empty when x > y
  VRPMS_DEV void fwd(int x, int y) {
    if (x > y) return;
    int g = r.G[x];
    int sn = r.S[g + 1];   // the first separator at or past x
    if (sn > y) {
      piece_f(x, y);
      return;
    }
    if (x < sn) piece_f(x, sn - 1);
    close();
    for (++g; (int)r.S[g + 1] <= y; ++g) {
      whole(g, r.FD);
      sn = r.S[g + 1];
    }
    if (sn < y) piece_f(sn + 1, y);
  }
  // the padded range [x, y] of the current tour, backwards from y; x <= y
  VRPMS_DEV void rev(int x, int y) {
    const int g = r.G[y];
    int h = (int)r.S[g + 1] == y ? g + 1 : g;   // S[h]: the last separator at or before y
    int sb = r.S[h];
    if (sb < x) {
      piece_r(y, x);
      return;
    }
    if (sb < y) piece_r(y, sb + 1);
    close();
    for (; h >= 1 && (int)r.S[h - 1] >= x; --h) whole(h - 1, r.BD);
    sb = r.S[h];
    if (sb > x) piece_r(sb - 1, x);
  }
};

// Candidate m on the plain tour of the rows (L >= 2 tokens, duration sum
// `sum`): its A8 key when that can be below `bound`, the all-ones key when a
// route of the moved tour is over its capacity, and otherwise some key that is
// not below `bound` -- the caller only ever takes a key below its bound.  The
// sum is `sum` plus the TSP delta on the token chain; the capacities and the
// maximum come from the segments the span touches.
template <typename Mat>
VRPMS_DEV uint64_t lsf_price(const Mat& D, const int32_t* cap, const LsfRows& r, int L, int sum,
                             int objective, const Move& m, uint64_t bound) {
  const int nsum = sum + lso_delta_static(D, r.P, r.F, r.B, L, m);
  const int lo = min(m.i, m.j), hi = max(m.i, m.j);
  const int a = r.G[lo + 1];
  // what no walk can improve on: the sum, and the routes outside the span
  const int outside = max(r.PM[a], r.SM[r.G[hi + 2] + 1]);
  if (cvrp_key(0, (uint32_t)nsum, (uint32_t)outside, objective) >= bound) return bound;
  LsfWalk<Mat> w{D, cap, r, a, r.F[lo] - r.F[r.S[a]], outside, r.W[lo] - r.W[r.S[a]], r.P[lo], true};
  const int i1 = m.i + 1, j1 = m.j + 1;   // padded
  if (m.typ == kMoveSwap) {
    w.fwd(j1, j1);
    w.fwd(i1 + 1, j1 - 1);
    w.fwd(i1, i1);
  } else if (m.typ == kMove2Opt) {
    w.rev(i1, j1);
  } else if (m.i < m.j) {
    w.fwd(i1 + 1, j1);
    w.fwd(i1, i1);
  } else {
    w.fwd(i1, i1);
    w.fwd(j1, i1 - 1);
  }
  // the rest of the last touched segment, up to its separator
  const int u = hi + 2, se = r.S[w.k + 1];
  w.dur += D(0, w.last, (uint32_t)r.P[u]) + r.F[se] - r.F[u];
  w.add(r.W[se] - r.W[u - 1]);
  w.ok &= (int64_t)w.load <= (int64_t)cap[w.k];
  w.mx = max(w.mx, w.dur);
  return w.ok ? cvrp_key(0, (uint32_t)nsum, (uint32_t)w.mx, objective) : ~0ull;
}

// The 256-thread forms: one descent per workgroup at a time (vrp_batch_lsf_spread.hip).
//
// A wavefront's own parts there, behind the instance: BatchLsfParts' less the
// best end tour, which lives in the workspace.  The [2][4] round records
// follow the four wavefronts' parts.
template <typename I>
struct BatchLsfSpreadParts {
  I row_words, tab_words, ppad, spad, gpad;
  __host__ __device__ BatchLsfSpreadParts(I L, I K) {
    const BatchLsfParts<I> f(L, K);
    row_words = f.row_words;
    tab_words = f.tab_words;
    ppad = f.ppad;
    spad = f.spad;
    gpad = f.gpad;
  }
  __host__ __device__ I words() const { return 3 * row_words + 5 * tab_words; }
  __host__ __device__ I halves() const { return ppad + spad; }
  __host__ __device__ I wave_bytes() const { return 4 * words() + 2 * halves() + gpad; }
};

inline size_t batch_lsf_spread_lds(int N, int K, int wide) {
  return batch_inst_bytes(N, K, 1, wide) +
         4 * BatchLsfSpreadParts<size_t>((size_t)(N - 1 + K - 1), (size_t)K).wave_bytes() +
         2 * 4 * sizeof(BatchLsRec);
}

// One steepest descent of the whole workgroup (four wavefronts, `sh` from
// batch_ls_share_wg) on one PLAIN tour of L >= 2 tokens with key ck, duration
// sum `sum` and longest route `dmax`: vrp_batch_lsf_kernel's rounds, the thread
// pricing its share with lsf_price.  As in batch_ls_descend_wg and
// lso_descend_wg every wavefront holds its own copy of the padded tour and of
// its rows -- equal on entry, and they stay equal, since each applies the same
// move and rebuilds its rows from the same tour -- so a round has one barrier:
// the wavefronts' records meet in rec[parity][wave] and each takes the least
// (key, wave), which is the least (key, typ, i, j) because the id ranges ascend
// with the thread.  A thread's running bound starts at ck and lsf_price may
// answer a candidate whose key is not below it with the bound itself: such a
// key is not below ck, or not below a key the same thread holds at a lower id,
// so the thread would not have taken it and no winner is withheld.  A thread
// without a candidate below ck sends ck; a round whose least key is ck ends
// the descent.  `parity` alternates with every barrier of the kernel past
// staging, over all its descents (batch_ls.hpp has the argument).  ck, `rounds`,
// the records and so every branch here are the same in all four wavefronts --
// the caller enters with a plainness all four agree on --; all of them reach
// every barrier.  -> the end tour's key.
template <typename Mat>
VRPMS_DEV uint64_t lsf_descend_wg(const Mat& D, const int32_t* dem, const int32_t* cap, const LsfRows& rows,
                                  int L, int K, uint64_t ck, int sum, int dmax, int objective, int rounds,
                                  const BatchLsShare& sh, int wave, int lane, BatchLsRec* rec, int& parity,
                                  int& capped) {
  uint16_t* A = rows.P + 1;
  for (int applied = 0;; ++applied) {
    if (applied >= rounds) {   // stopped unproven
      ++capped;
      break;
    }
    Move m = sh.m0, lm = sh.m0;
    uint64_t lk = ck;   // only a key below the tour's is of use
    for (int c = 0; c < sh.cnt; ++c) {
      const uint64_t k = lsf_price(D, cap, rows, L, sum, objective, m, lk);
      if (k < lk) {
        lk = k;
        lm = m;
      }
      batch_ls_next(m, L);
    }
    int bl;
    const uint64_t wk = wave_argmin_lane(lk, bl);
    BatchLsRec* mine = rec + 4 * parity;
    if (lane == bl) mine[wave] = BatchLsRec{wk, lm.typ, (uint16_t)lm.i, (uint16_t)lm.j};
    __syncthreads();
    int bw = 0;
    for (int w = 1; w < 4; ++w)
      if (mine[w].key < mine[bw].key) bw = w;   // the lowest wavefront among equal keys
    const BatchLsRec best = mine[bw];
    parity ^= 1;
    if (!(readlane_u64(best.key, 0) < ck)) break;   // a local optimum
    Move mb;
    mb.typ = (uint32_t)__builtin_amdgcn_readfirstlane((int)best.typ);
    mb.i = __builtin_amdgcn_readfirstlane((int)best.i);
    mb.j = __builtin_amdgcn_readfirstlane((int)best.j);
    batch_ls_apply(A, mb, lane);
    sum = lsf_rows(D, dem, rows, L, K, lane, dmax);
    ck = cvrp_key(0, (uint32_t)sum, (uint32_t)dmax, objective);
  }
  return ck;
}

// the shape checks of every lsf entry point: vrp_batch_lsr's on a static matrix
inline int batch_lsf_check(const char* who, int32_t N, int32_t K, int32_t H, int32_t wide) {
  if (const int rc = batch_lsr_check(who, N, K, H, wide)) return rc;
  return batch_check_static(who, H, "vrpms_vrp_batch_lsr");
}

}  // namespace vrpms
