// What tsp_batch_lso.hip (A27) adds to batch_ls.hpp's descent: the order of a
// round's moves over five types under a mask, a lane's share of them, where
// the moved tour reads from, and the in-place Or-opt.  Types 0..2 are
// batch_ls.hpp's (tour.hpp's swap, 2-opt and relocate); typ 3 and 4 move a
// segment of m = typ - 1 customers: with seg = p[i:i+m] and rest = p[:i] +
// p[i+m:], the moved tour is rest[:j] + seg + rest[j:], 0 <= i, j <= n - m,
// j != i.  Relocate is that formula at m = 1, so typ >= 2 shares one code path
// with m = typ - 1 and np = n - m + 1 values of i and of j.  batch_ls.hpp is
// left as it is: the VRP kernels that include it compile as before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_ls.hpp"
#include "common.hpp"
#include "tour.hpp"

namespace vrpms {

constexpr int kLsoTypes = 5;

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

}  // namespace vrpms
