// What the two batched local searches share (vrp_batch_ls.hip, A25, on tours of
// n customers; vrp_batch_lsr.hip, A26, on tours of n + K - 1 tokens): the order
// of a round's moves, a lane's share of them, the Philox Fisher-Yates start,
// the in-place move, the descent's round loop and the waves' records, and for
// vrp_batch_lsr_spread.hip (A26 with 256 threads on one descent) the thread's
// share and the workgroup's round loop.  `n` below is the number of positions
// of the tour the descent works on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "tour.hpp"

namespace vrpms {

struct BatchLsWave {   // 16 bytes
  uint64_t key;
  int32_t s, capped;
};

// the move after m in (typ, i, j) order; n >= 2
VRPMS_DEV void batch_ls_next(Move& m, int n) {
  if (m.typ != kMoveRelocate) {
    if (++m.j == n) {
      ++m.i;
      m.j = m.i + 1;
      if (m.j == n) {   // the triangle is done: 2-opt after swap, relocate after 2-opt
        ++m.typ;
        m.i = 0;
        m.j = 1;
      }
    }
  } else {
    ++m.j;
    if (m.j == m.i) ++m.j;
    if (m.j >= n) {
      ++m.i;
      m.j = 0;
    }
  }
}

// move number id of the 2 n (n - 1), n >= 2
VRPMS_DEV Move batch_ls_move(int id, int n) {
  const int tri = n * (n - 1) / 2;
  Move m;
  if (id >= 2 * tri) {
    const int r = id - 2 * tri, jp = r % (n - 1);
    m.typ = kMoveRelocate;
    m.i = r / (n - 1);
    m.j = jp + (jp >= m.i ? 1 : 0);
    return m;
  }
  m.typ = id >= tri ? kMove2Opt : kMoveSwap;
  int r = id >= tri ? id - tri : id, i = 0;
  while (r >= n - 1 - i) {   // row i holds j = i + 1 .. n - 1
    r -= n - 1 - i;
    ++i;
  }
  m.i = i;
  m.j = i + 1 + r;
  return m;
}

// the lane's share of a round: the ids [lane per, lane per + cnt) from move m0
// on, per = ceil(2 n (n - 1) / 64); n < 2 has no moves
struct BatchLsShare {
  Move m0;
  int cnt;
};

VRPMS_DEV BatchLsShare batch_ls_share(int n, int lane) {
  const int total = 2 * n * (n - 1), per = (total + 63) >> 6;
  const int id0 = lane * per;
  BatchLsShare sh{Move{kMoveSwap, 0, 1}, max(0, min(per, total - id0))};
  if (sh.cnt > 0) sh.m0 = batch_ls_move(id0, n);
  return sh;
}

// A[0..n) = the Philox Fisher-Yates shuffle of 1..n with counters (0xffffffff,
// 0xffffffff, s, q), as in vrp_batch_sa: lane l draws the block of q = 64 c + l
// for a chunk of 64 swaps at once, lane 0 swaps
VRPMS_DEV void batch_ls_shuffle(uint16_t* A, int n, int s, uint32_t seed_lo, uint32_t seed_hi,
                                int lane) {
  for (int q = lane; q < n; q += 64) A[q] = (uint16_t)(q + 1);
  wave_sync();
  uint32_t jv = 0;
  for (int i = n - 1; i >= 1; --i) {
    if (i == n - 1 || (i & 63) == 63) {
      const uint32_t il = (uint32_t)(i & ~63) + (uint32_t)lane;
      const u32x4 x = philox(0xffffffffu, 0xffffffffu, (uint32_t)s, il, seed_lo, seed_hi);
      jv = x.x % (il + 1u);
    }
    const int j = __builtin_amdgcn_readlane((int)jv, i & 63);
    if (lane == 0) {
      const uint16_t t = A[i];
      A[i] = A[j];
      A[j] = t;
    }
  }
  wave_sync();
}

// the wave-uniform move mb on A, in place (spec.apply_move)
VRPMS_DEV void batch_ls_apply(uint16_t* A, const Move& mb, int lane) {
  const int i = mb.i, j = mb.j;
  if (mb.typ == kMoveSwap) {
    if (lane == 0) {
      const uint16_t t = A[i];
      A[i] = A[j];
      A[j] = t;
    }
  } else if (mb.typ == kMove2Opt) {   // disjoint pairs (i + t, j - t)
    const int half = (j - i + 1) >> 1;
    for (int t = lane; t < half; t += 64) {
      const uint16_t x = A[i + t];
      A[i + t] = A[j - t];
      A[j - t] = x;
    }
  } else if (i < j) {   // A[i+1..j] moves down one place, 64 at a time from below
    const uint16_t v = A[i];
    wave_sync();
    for (int base = i; base < j; base += 64) {
      const int q = base + lane;
      uint16_t x = 0;
      if (q < j) x = A[q + 1];
      wave_sync();
      if (q < j) A[q] = x;
      wave_sync();
    }
    if (lane == 0) A[j] = v;
  } else {              // A[j..i-1] moves up one place, 64 at a time from above
    const uint16_t v = A[i];
    wave_sync();
    for (int top = i; top > j; top -= 64) {
      const int q = top - lane;
      uint16_t x = 0;
      if (q > j) x = A[q - 1];
      wave_sync();
      if (q > j) A[q] = x;
      wave_sync();
    }
    if (lane == 0) A[j] = v;
  }
  wave_sync();
}

// One steepest descent of the wave on A (n >= 2 positions, key ck): a round
// prices the lane's share by eval_tour<true> over map_src(move_map(m), q) and
// applies the least (key, typ, i, j) while its key is below the tour's; after
// `rounds` applied moves it stops unproven and adds one to `capped`.  -> the
// end tour's key.
template <typename Mat>
VRPMS_DEV uint64_t batch_ls_descend(const Mat& D, const SplitParams& sp, uint16_t* A, int n,
                                    uint64_t ck, int rounds, const BatchLsShare& sh, int lane,
                                    int& capped) {
  for (int applied = 0;; ++applied) {
    if (applied >= rounds) {   // stopped unproven
      ++capped;
      break;
    }
    Move m = sh.m0, lm = sh.m0;
    uint64_t lk = ~0ull;
    for (int c = 0; c < sh.cnt; ++c) {
      const MoveMap mm = move_map(m);
      const uint64_t k =
          eval_tour<true>(D, sp, [&](int q) { return (uint32_t)A[map_src(mm, q)]; }, n).key;
      if (k < lk) {
        lk = k;
        lm = m;
      }
      batch_ls_next(m, n);
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
    batch_ls_apply(A, mb, lane);
    ck = k;
  }
  return ck;
}

// The 256-thread forms: one descent per workgroup at a time (vrp_batch_lsr_spread.hip).
//
// the thread's share of a round: the ids [t per, t per + cnt) from move m0 on,
// per = ceil(2 n (n - 1) / 256), t = 64 wave + lane; n < 2 has no moves
VRPMS_DEV BatchLsShare batch_ls_share_wg(int n, int t) {
  const int total = 2 * n * (n - 1), per = (total + 255) >> 8;
  const int id0 = t * per;
  BatchLsShare sh{Move{kMoveSwap, 0, 1}, max(0, min(per, total - id0))};
  if (sh.cnt > 0) sh.m0 = batch_ls_move(id0, n);
  return sh;
}

// a wavefront's least (key, typ, i, j) of a round, as the four exchange it
struct BatchLsRec {   // 16 bytes
  uint64_t key;
  uint32_t typ;
  uint16_t i, j;      // positions are below 65535
};

// One steepest descent of the whole workgroup (four wavefronts, `sh` from
// batch_ls_share_wg) on one tour, n >= 2 positions, key ck: batch_ls_descend's
// rounds, the thread pricing its share.  Every wavefront holds its own copy A
// of the tour -- the four are equal on entry and stay equal, since each applies
// the same move -- so a round has one barrier: the wavefronts' records meet in
// rec[parity][wave], and each wavefront takes the least (key, wave), which is
// the least (key, typ, i, j) because the id ranges ascend with the thread.
// `parity` alternates with every barrier of the kernel, over all its descents:
// a wavefront writes rec[p] for the round after next only past the next
// round's barrier, which the slowest reaches after it has read rec[p].  ck,
// `rounds`, the records and so every branch here are the same in all four
// wavefronts; all of them reach every barrier.  -> the end tour's key.
template <typename Mat>
VRPMS_DEV uint64_t batch_ls_descend_wg(const Mat& D, const SplitParams& sp, uint16_t* A, int n,
                                       uint64_t ck, int rounds, const BatchLsShare& sh, int wave,
                                       int lane, BatchLsRec* rec, int& parity, int& capped) {
  for (int applied = 0;; ++applied) {
    if (applied >= rounds) {   // stopped unproven
      ++capped;
      break;
    }
    Move m = sh.m0, lm = sh.m0;
    uint64_t lk = ~0ull;
    for (int c = 0; c < sh.cnt; ++c) {
      const MoveMap mm = move_map(m);
      const uint64_t k =
          eval_tour<true>(D, sp, [&](int q) { return (uint32_t)A[map_src(mm, q)]; }, n).key;
      if (k < lk) {
        lk = k;
        lm = m;
      }
      batch_ls_next(m, n);
    }
    int bl;
    const uint64_t wk = wave_argmin_lane(lk, bl);
    BatchLsRec* mine = rec + 4 * parity;
    if (lane == bl)
      mine[wave] = BatchLsRec{wk, lm.typ, (uint16_t)lm.i, (uint16_t)lm.j};
    __syncthreads();
    int bw = 0;
    for (int w = 1; w < 4; ++w)
      if (mine[w].key < mine[bw].key) bw = w;   // the lowest wavefront among equal keys
    const BatchLsRec best = mine[bw];
    parity ^= 1;
    const uint64_t k = readlane_u64(best.key, 0);
    if (!(k < ck)) break;   // a local optimum
    Move mb;
    mb.typ = (uint32_t)__builtin_amdgcn_readfirstlane((int)best.typ);
    mb.i = __builtin_amdgcn_readfirstlane((int)best.i);
    mb.j = __builtin_amdgcn_readfirstlane((int)best.j);
    batch_ls_apply(A, mb, lane);
    ck = k;
  }
  return ck;
}

// After the kernel's barrier past the descents: the wave that holds the least
// (key, s) of the four records, and the capped descents of all of them.
VRPMS_DEV int batch_ls_winner(const BatchLsWave* wst, int& ncap) {
  int bw = 0;
  ncap = wst[0].capped;
  for (int w = 1; w < 4; ++w) {
    if (wst[w].key < wst[bw].key || (wst[w].key == wst[bw].key && wst[w].s < wst[bw].s)) bw = w;
    ncap += wst[w].capped;
  }
  return bw;
}

}  // namespace vrpms
