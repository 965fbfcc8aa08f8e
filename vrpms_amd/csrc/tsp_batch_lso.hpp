// What tsp_batch_lso.hip (A27) adds to batch_ls.hpp's descent: the order of a
// round's moves over five types under a mask, a lane's share of them, where
// the moved tour reads from, and the in-place Or-opt.  Types 0..2 are
// batch_ls.hpp's (tour.hpp's swap, 2-opt and relocate); typ 3 and 4 move a
// segment of m = typ - 1 customers: with seg = p[i:i+m] and rest = p[:i] +
// p[i+m:], the moved tour is rest[:j] + seg + rest[j:], 0 <= i, j <= n - m,
// j != i.  Relocate is that formula at m = 1, so typ >= 2 shares one code path
// with m = typ - 1 and np = n - m + 1 values of i and of j.  batch_ls.hpp is
// left as it is: the VRP kernels that include it compile as before.
//
// And what A27's two mappings share (tsp_batch_lso.hip, one workgroup per
// request; tsp_batch_lso_spread.hip, G workgroups per request): the launch's
// arguments and checks, the LDS sizes, the matrix staging, the prefix rows and
// the pricing of a candidate, and for the second mapping the thread's share
// and the workgroup's round loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "batch_launch.hpp"
#include "batch_ls.hpp"
#include "batch_stage.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "tour.hpp"

namespace vrpms {

constexpr int kLsoTypes = 5;

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

// What both mappings keep in LDS, the first parts of their dynamic LDS, in their
// order: the [H][N][N] matrix (cells of `cell` bytes, padded to 16 bytes), per
// wavefront the int32 rows F and B (H = 1) or T (H = 24) of align4(n + 2)
// words, per wavefront the current tour of align8(n + 2) uint16 with node 0 at
// both ends.  The host sums the parts, a kernel steps through them (LsoCarve);
// I is size_t on the host and uint32_t in a kernel, as for BatchInstParts.
template <typename I>
struct BatchLsoParts {
  I cells, mat_bytes, rows, row_words, cpad;   // rows: F and B, or T alone
  __host__ __device__ BatchLsoParts(I N, I H, I cell) {
    cells = H * N * N;
    mat_bytes = batch_align<I>(cells * cell, 16);
    rows = H == 1 ? 2 : 1;
    row_words = batch_align<I>(N - 1 + 2, 4);
    cpad = batch_align<I>(N - 1 + 2, 8);
  }
  __host__ __device__ I bytes() const { return mat_bytes + 4 * rows * row_words * 4 + 4 * cpad * 2; }
};

// tsp_batch_lso_spread's own part behind them: [2][4] BatchLsRec
constexpr size_t kBatchLsoSpreadOwnBytes = 2 * 4 * sizeof(BatchLsRec);

inline size_t batch_lso_shared_bytes(int N, int H, int wide) {
  return BatchLsoParts<size_t>((size_t)N, (size_t)H, wide ? 4 : 2).bytes();
}

// the kernels' carve of the shared parts; the kernel's own follow at `rest`
template <typename MatT, int HM>
struct LsoCarve {
  static constexpr uint32_t kRows = HM == 1 ? 2u : 1u;
  MatT* M;
  int32_t* rows;    // [4][kRows][row_words]
  uint16_t* curs;   // [4][cpad]
  unsigned char* rest;
  uint32_t cells, row_words, cpad;
  VRPMS_DEV LsoCarve(unsigned char* mem, int N) {
    const BatchLsoParts<uint32_t> l((uint32_t)N, (uint32_t)HM, (uint32_t)sizeof(MatT));
    cells = l.cells;
    row_words = l.row_words;
    cpad = l.cpad;
    M = reinterpret_cast<MatT*>(mem);
    rows = reinterpret_cast<int32_t*>(mem + l.mat_bytes);
    curs = reinterpret_cast<uint16_t*>(rows + 4 * kRows * row_words);
    rest = reinterpret_cast<unsigned char*>(curs + 4 * cpad);
  }
  VRPMS_DEV int32_t* F(int wave) const { return rows + wave * kRows * row_words; }   // H = 24: the arrival row T
  VRPMS_DEV int32_t* B(int wave) const { return F(wave) + (kRows - 1) * row_words; }   // H = 1 only
  VRPMS_DEV uint16_t* P(int wave) const { return curs + wave * cpad; }   // node 0 at both ends
};

// the shape checks every entry point shares; 0 or the refusal's code
inline int batch_lso_check(const char* who, int32_t N, int32_t H, int32_t wide) {
  if (const int rc = batch_check_N(who, N)) return rc;
  return batch_check_matrix(who, H, wide);
}

// the checks of the search's own arguments; 0 or the refusal's code
inline int batch_lso_check_search(const char* who, int32_t S, int32_t rounds, int32_t moves) {
  if (const int rc = batch_check_count(who, "S", S, kBatchMaxS)) return rc;
  if (const int rc = batch_check_rounds(who, rounds)) return rc;
  if (moves < 1 || moves > 31)
    return fail(VRPMS_EINVAL, std::string(who) + ": 1 <= moves <= 31, bit t enabling move type t (" +
                                  std::to_string(moves) + " given)");
  return VRPMS_OK;
}

// the moves of type typ on n positions
VRPMS_DEV int lso_count(int typ, int n) {
  if (typ < 2) return n * (n - 1) / 2;
  const int np = n - typ + 2;
  return np >= 2 ? np * (np - 1) : 0;
}

// the first type from typ on that is enabled and has moves; kLsoTypes when none
VRPMS_DEV int lso_type_from(int typ, int n, uint32_t mask) {
  while (typ < kLsoTypes && (!((mask >> typ) & 1u) || lso_count(typ, n) == 0)) ++typ;
  return typ;
}

// the enabled moves of a round
VRPMS_DEV int lso_total(int n, uint32_t mask) {
  int total = 0;
  for (int typ = 0; typ < kLsoTypes; ++typ)
    if ((mask >> typ) & 1u) total += lso_count(typ, n);
  return total;
}

// the move after m in (typ, i, j) order over the enabled types; n >= 2.  Past
// the last move m.typ is kLsoTypes: the share's count keeps it from being used
VRPMS_DEV void lso_next(Move& m, int n, uint32_t mask) {
  bool done;
  if (m.typ < 2) {
    done = false;
    if (++m.j == n) {
      ++m.i;
      m.j = m.i + 1;
      done = m.j == n;
    }
  } else {
    const int np = n - (int)m.typ + 2;
    ++m.j;
    if (m.j == m.i) ++m.j;
    done = false;
    if (m.j >= np) {
      ++m.i;
      m.j = 0;
      done = m.i == np;
    }
  }
  if (done) {
    m.typ = (uint32_t)lso_type_from((int)m.typ + 1, n, mask);
    m.i = 0;
    m.j = 1;
  }
}

// enabled move number id, 0 <= id < lso_total(n, mask), n >= 2
VRPMS_DEV Move lso_move(int id, int n, uint32_t mask) {
  int typ = 0;
  for (; typ < kLsoTypes; ++typ) {
    if (!((mask >> typ) & 1u)) continue;
    const int c = lso_count(typ, n);
    if (id < c) break;
    id -= c;
  }
  Move m;
  m.typ = (uint32_t)typ;
  if (typ < 2) {
    int i = 0;
    while (id >= n - 1 - i) {   // row i holds j = i + 1 .. n - 1
      id -= n - 1 - i;
      ++i;
    }
    m.i = i;
    m.j = i + 1 + id;
  } else {
    const int np = n - typ + 2, jp = id % (np - 1);
    m.i = id / (np - 1);
    m.j = jp + (jp >= m.i ? 1 : 0);
  }
  return m;
}

// the lane's share of a round: the enabled ids [lane per, lane per + cnt) from
// move m0 on, per = ceil(total / 64)
VRPMS_DEV BatchLsShare lso_share(int n, uint32_t mask, int lane) {
  BatchLsShare sh{Move{kMoveSwap, 0, 1}, 0};
  if (n < 2) return sh;
  const int total = lso_total(n, mask), per = (total + 63) >> 6;
  const int id0 = lane * per;
  sh.cnt = max(0, min(per, total - id0));
  if (sh.cnt > 0) sh.m0 = lso_move(id0, n, mask);
  return sh;
}

// the thread's share of a round when a workgroup's 256 threads price one tour
// (tsp_batch_lso_spread.hip): the enabled ids [t per, t per + cnt) from move m0
// on, per = ceil(total / 256), t = 64 wave + lane
VRPMS_DEV BatchLsShare lso_share_wg(int n, uint32_t mask, int t) {
  BatchLsShare sh{Move{kMoveSwap, 0, 1}, 0};
  if (n < 2) return sh;
  const int total = lso_total(n, mask), per = (total + 255) >> 8;
  const int id0 = t * per;
  sh.cnt = max(0, min(per, total - id0));
  if (sh.cnt > 0) sh.m0 = lso_move(id0, n, mask);
  return sh;
}

// Position in the current tour read at position q of the moved tour, for all
// five types, as a select chain: one window read at a + s q (the reversal, the
// shift by m) and one read at q + a2 (the segment, a swap's other end).
struct LsoMap {
  int lo, len, a, s, lo2, len2, a2;
};

VRPMS_DEV LsoMap lso_map(const Move& m) {
  const int i = m.i, j = m.j;
  if (m.typ == kMoveSwap) return {i, 1, j, 0, j, 1, i - j};
  if (m.typ == kMove2Opt) return {i, j - i + 1, i + j, -1, 0, 0, 0};
  const int sl = (int)m.typ - 1;
  if (i < j) return {i, j - i, sl, 1, j, sl, i - j};
  return {j + sl, i - j, -sl, 1, j, sl, i - j};
}

VRPMS_DEV int lso_src(const LsoMap& mm, int q) {
  int r = (uint32_t)(q - mm.lo) < (uint32_t)mm.len ? mm.a + mm.s * q : q;
  return (uint32_t)(q - mm.lo2) < (uint32_t)mm.len2 ? q + mm.a2 : r;
}

// the first and the last position the move changes
VRPMS_DEV int lso_first(const Move& m) { return min(m.i, m.j); }
VRPMS_DEV int lso_last(const Move& m) {
  return max(m.i, m.j) + (m.typ > kMoveRelocate ? (int)m.typ - 2 : 0);
}

// the wave-uniform move mb on A, in place: batch_ls_apply for the types 0..2,
// and for an Or-opt the segment kept in registers while the positions between
// shift by m, 64 at a time -- from below when the segment moves up the tour
// (a chunk reads at most m places into the next one, not yet written), from
// above when it moves down
VRPMS_DEV void lso_apply(uint16_t* A, const Move& mb, int lane) {
  if (mb.typ <= kMoveRelocate) {
    batch_ls_apply(A, mb, lane);
    return;
  }
  const int i = mb.i, j = mb.j, sl = (int)mb.typ - 1;
  const uint16_t s0 = A[i], s1 = A[i + 1], s2 = A[i + sl - 1];
  wave_sync();
  if (i < j) {   // A[i .. j-1] = A[i+m .. j+m-1]
    for (int base = i; base < j; base += 64) {
      const int q = base + lane;
      uint16_t x = 0;
      if (q < j) x = A[q + sl];
      wave_sync();
      if (q < j) A[q] = x;
      wave_sync();
    }
  } else {       // A[j+m .. i+m-1] = A[j .. i-1]
    for (int top = i + sl - 1; top >= j + sl; top -= 64) {
      const int q = top - lane;
      uint16_t x = 0;
      if (q >= j + sl) x = A[q - sl];
      wave_sync();
      if (q >= j + sl) A[q] = x;
      wave_sync();
    }
  }
  if (lane == 0) {
    A[j] = s0;
    A[j + 1] = s1;
    A[j + sl - 1] = s2;
  }
  wave_sync();
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

// The workgroup stages request r's `cells` matrix entries into M and checks
// them as batch_stage_request does: a negative entry, or one above 65535 in a
// uint16 matrix, fails the request.  The verdict goes through `flag`, a word
// of LDS that is free until the last barrier here.  -> the request is refused
template <typename MatT>
VRPMS_DEV bool lso_stage(const int32_t* mats, int64_t r, uint32_t cells, MatT* M, uint32_t* flag) {
  const int32_t* src = mats + r * (int64_t)cells;
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
  return bad;
}

// the refusal row of request r, written by the whole workgroup
VRPMS_DEV void lso_refuse(const TspBatchLsoArgs& a, int64_t r, int n) {
  uint16_t* gtour = a.tours + r * n;
  for (int q = threadIdx.x; q < n; q += 256) gtour[q] = 0;
  if (threadIdx.x == 0) {
    a.keys[r] = ~0ull;
    a.durs[r] = 0;
    a.info[2 * r] = -1;
    a.info[2 * r + 1] = 0;
  }
}

// The 256-thread forms: one descent per workgroup at a time (tsp_batch_lso_spread.hip).
//
// the wavefront's rows of its padded tour P: F and B at HM = 1, the arrival
// row (in F) at HM = 24 -> the tour's duration
template <int HM, typename Mat>
VRPMS_DEV int lso_measure(const Mat& D, const uint16_t* P, int n, int t0, int32_t* F, int32_t* B,
                          int lane) {
  if constexpr (HM == 1) return lso_rows_static(D, P, n, F, B, lane);
  else return lso_row_clock(D, P, n, t0, F, lane);
}

// One steepest descent of the whole workgroup (four wavefronts, `sh` from
// lso_share_wg) on one tour of n >= 2 customers and duration `dur`:
// tsp_batch_lso_kernel's rounds, the thread pricing its share.  As in
// batch_ls_descend_wg every wavefront holds its own copy of the padded tour P
// and of its rows -- equal on entry, and they stay equal, since each applies
// the same move and rebuilds its rows from the same tour -- so a round has one
// barrier: the wavefronts' records meet in rec[parity][wave] and each takes
// the least (key, wave), which is the least (key, typ, i, j) because the id
// ranges ascend with the thread.  `parity` alternates with every barrier of the
// kernel past staging, over all its descents (batch_ls.hpp has the argument).
// dur, `rounds`, the records and so every branch here are the same in all four
// wavefronts; all of them reach every barrier.  -> the end tour's duration.
template <int HM, typename Mat>
VRPMS_DEV int lso_descend_wg(const Mat& D, uint16_t* P, int32_t* F, int32_t* B, int n, int t0,
                             uint32_t mask, int dur, int rounds, const BatchLsShare& sh, int wave,
                             int lane, BatchLsRec* rec, int& parity, int& capped) {
  uint64_t ck = pack_key(0, (uint32_t)dur, 0);
  for (int applied = 0;; ++applied) {
    if (applied >= rounds) {   // stopped unproven
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
    lso_apply(P + 1, mb, lane);
    dur = lso_measure<HM>(D, P, n, t0, F, B, lane);
    ck = pack_key(0, (uint32_t)dur, 0);
  }
  return dur;
}

}  // namespace vrpms
