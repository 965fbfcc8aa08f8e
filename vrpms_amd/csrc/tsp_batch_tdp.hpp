// What tsp_batch_tdp.hip shares with vrp_batch_tdsp.hip: one team's staging,
// fill and walk of the compact LDS-resident A16 table (DESIGN.md §2 A20,
// §4.3k), over a subset of the request's customers from an explicit start.
//
// A sub-problem is a customer mask `members` of the request's n = N - 1
// customers: its m local customers are the members in ascending order (local
// customer p = the p-th member), local node 0 is the depot.  The staged slices
// are the sub-problem's own [slice][m + 1][m + 1] matrices, the table its own
// m 2^(m-1) rows of W words at the front of the team's table.  With every
// customer a member the node map is the identity and everything is A20's.
//
// None of these functions contains a barrier the caller cannot count:
// batch_tdp_stage has none, batch_tdp_fill has exactly `rounds` (one after the
// singleton rows, one after each layer 2..rounds, whatever m and `live` are),
// batch_tdp_walk has none.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "tsp_batch_dp.hpp"
#include "tsp_dp.hpp"

namespace vrpms {

// 0: owner thread per row at every W, 1: atomic OR at every W (the A/B builds
// of tools/ab_build.py), 2: the launch picks by W -- owner rows below
// kBatchTdpAtomicWords words, atomic OR from there (§4.3k: neither wins everywhere)
#ifndef VRPMS_BATCH_TDP_FILL
#define VRPMS_BATCH_TDP_FILL 2
#endif
constexpr int kBatchTdpFill = VRPMS_BATCH_TDP_FILL;
static_assert(kBatchTdpFill >= 0 && kBatchTdpFill <= 2, "0: owner, 1: atomic OR, 2: by W");
constexpr int kBatchTdpAtomicWords = 8;

constexpr int kBatchTdpMaxN = 11;      // customers: n = 12 is 196,608 B of table at W = 1
constexpr uint64_t kBatchTdpMask60 = (1ull << 60) - 1;

// threads per request by n (index n), before the LDS has its say: the fastest
// T of tools/batch_tdp_rate.py --teams 16,32,64,128,256 at each n and W = 1
// (DESIGN.md §4.3k has the measurements; n = 1 is not measured and takes
// n = 2's).
constexpr int kBatchTdpTeam[kBatchTdpMaxN + 1] = {16, 16, 16, 16, 16, 16, 32, 32, 128, 256, 256, 256};

// matrix slices one request stages
inline int batch_tdp_slices(int H, int W) { return H == 1 ? 1 : (W < 24 ? W : 24); }

inline bool batch_tdp_atomic(int W) { return kBatchTdpFill == 2 ? W >= kBatchTdpAtomicWords : kBatchTdpFill == 1; }

template <int FILL>
VRPMS_DEV void batch_tdp_or(uint64_t* p, uint64_t v) {
  if (FILL)
    atomicOr(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
  else
    *p |= v;
}

// What one request's lanes share after staging.
struct BatchTdpReq {
  int off;             // start % 60: the start's bit in word 0
  int hz;              // the effective horizon
  int lw;              // the last word a clock within the horizon can be in
  uint64_t last_mask;  // bits of word lw at or below start + hz
};

// start, horizon >= 0: the horizon clipped to the W words of a row
VRPMS_DEV BatchTdpReq batch_tdp_req(int start, int horizon, int W) {
  BatchTdpReq q;
  q.off = start % 60;
  const int cap = 60 * W - 1 - q.off;
  q.hz = horizon < cap ? horizon : cap;
  q.lw = (q.off + q.hz) / 60;
  q.last_mask = (2ull << ((q.off + q.hz) % 60)) - 1ull;
  return q;
}

// the request's node behind local node a of the sub-problem `members`
VRPMS_DEV int batch_tdp_node(uint32_t members, int a) {
  if (a == 0) return 0;
  for (int u = 1; u < a; ++u) members &= members - 1u;
  return __builtin_ctz(members) + 1;
}

// One source word x of row (P, i), at word w, moved along the edge i -> c into
// the destination row: the clip and the last-word mask are applied here.
template <int FILL>
VRPMS_DEV void batch_tdp_move(uint64_t x, int d, int w, const BatchTdpReq& q, uint64_t* dest) {
  const int dq = d / 60, s = d - dq * 60;
  const int dst = w + dq;
  if ((unsigned)dst > (unsigned)q.lw) return;
  uint64_t lo60 = (x << s) & kBatchTdpMask60;
  if (dst == q.lw) lo60 &= q.last_mask;
  if (lo60) batch_tdp_or<FILL>(dest + dst, lo60);
  if (dst < q.lw) {
    uint64_t hi60 = x >> (60 - s);   // s = 0: x < 2^60, nothing carries
    if (dst + 1 == q.lw) hi60 &= q.last_mask;
    if (hi60) batch_tdp_or<FILL>(dest + dst + 1, hi60);
  }
}

// Lane tl of a team of T stages the sub-problem's slices -- Dl[p][a][b] =
// D[slice (start / 60 + p) % 24][node a][node b] for p < ns, one slice when
// H = 1 -- and zeroes its m 2^(m-1) rows.  D is the request's [H][N][N].  The
// caller's barrier publishes both.
template <int T>
VRPMS_DEV void batch_tdp_stage(const int32_t* D, int N, int H, int W, int ns, int start, uint32_t members,
                               int m, int tl, int32_t* Dl, uint64_t* tab) {
  const int M = m + 1, MM = M * M, NN2 = N * N;
  const int h0 = (start / 60) % 24;
  const bool identity = m == N - 1;
  for (int e = tl; e < ns * MM; e += T) {
    const int p = e / MM, r = e - p * MM;
    const int slice = H == 1 ? 0 : (h0 + p) % 24;
    int at = r;
    if (!identity) {
      const int a = r / M, b = r - a * M;
      at = batch_tdp_node(members, a) * N + batch_tdp_node(members, b);
    }
    Dl[e] = D[slice * NN2 + at];
  }
  const uint32_t table_words = m ? ((uint32_t)m << (m - 1)) * (uint32_t)W : 0u;
  for (uint32_t e = tl; e < table_words; e += T) tab[e] = 0;
}

// The table of a staged sub-problem of m customers: the m singleton rows, a
// barrier, then the layers k = 2..rounds with a barrier after each; a team
// with m < k, or one that is not live, only keeps the barrier's count (rounds
// is the same for every team of the workgroup, rounds >= 1).  The rows (S, c)
// of cardinality k, in (rank of S, position of c) order, are dealt in
// consecutive runs; FILL = 0 gives a row to one thread, FILL = 1 to a group of
// lanes that OR atomically (tsp_batch_tdp.hip's header has both).
template <int T, int FILL>
VRPMS_DEV void batch_tdp_fill(const uint32_t* B, uint64_t* tab, const int32_t* Dl, int m, int W, int ns,
                              const BatchTdpReq& q, int tl, bool live, int rounds) {
  const int M = m + 1;
  const uint32_t half = m ? 1u << (m - 1) : 1u, full = (1u << m) - 1u;
  // the m singleton rows: ({c}, c) squeezes to 0
  if (live && tl < m) {
    const int64_t rel = (int64_t)q.off + Dl[tl + 1];
    if (rel >= 0 && rel <= (int64_t)q.off + q.hz)
      tab[(size_t)tl * half * W + rel / 60] = 1ull << (rel % 60);
  }
  __syncthreads();

  const int nw = q.lw + 1;   // words of a row that can hold a clock
  // lanes per destination row
  int G = 1;
  if (FILL) {
    G = 4;
    while (G < W && G < 64 && G < T) G *= 2;
  }
  // lane -> (predecessor index, word) of its first item of a row, and the step of G items
  const int gl = tl % G, nwd = nw > 0 ? nw : 1;
  const int p0 = gl / nwd, w0 = gl - p0 * nwd;
  const int pstep = G / nwd, wstep = G - pstep * nwd;
  for (int k = 2; k <= rounds; ++k) {
    if (live && k <= m) {
      const uint32_t rows = B[m * kBatchDpNodes + k] * (uint32_t)k;
      const uint32_t NG = (uint32_t)(T / G), grp = (uint32_t)(tl / G);
      const uint32_t lo = grp * rows / NG, hi = (grp + 1u) * rows / NG;
      if (lo < hi) {
        uint32_t r = lo / k;
        int t = (int)(lo - r * k);
        uint32_t S = k == m ? full : dp_unrank(B, kBatchDpNodes, m, k, r);
        for (uint32_t e = lo; e < hi; ++e) {
          uint32_t mm = S;   // c = the t-th customer of S
          for (int u = 0; u < t; ++u) mm &= mm - 1u;
          const int c = __builtin_ctz(mm);
          const uint32_t P = S ^ (1u << c);
          uint64_t* dest = tab + (size_t)(c * half + batch_dp_squeeze(S, c)) * W;
          const int32_t* col = Dl + c + 1;   // col[(p M + i + 1) M] = D[slice p][i + 1][c + 1]
          if (!FILL) {
            for (uint32_t pm = P; pm; pm &= pm - 1u) {
              const int i = __builtin_ctz(pm);
              const uint64_t* src = tab + (size_t)(i * half + batch_dp_squeeze(P, i)) * W;
              for (int w = 0; w < nw; ++w) {
                const uint64_t x = src[w];
                if (x) batch_tdp_move<FILL>(x, col[((w % 24 % ns) * M + i + 1) * M], w, q, dest);
              }
            }
          } else {
            const int items = (k - 1) * nw;
            int p = p0, w = w0;
            for (int it = gl; it < items; it += G) {
              uint32_t pm = P;   // i = the p-th customer of P
              for (int u = 0; u < p; ++u) pm &= pm - 1u;
              const int i = __builtin_ctz(pm);
              const uint64_t x = tab[(size_t)(i * half + batch_dp_squeeze(P, i)) * W + w];
              if (x) batch_tdp_move<FILL>(x, col[((w % 24 % ns) * M + i + 1) * M], w, q, dest);
              p += pstep;
              w += wstep;
              if (w >= nw) {
                w -= nw;
                ++p;
              }
            }
          }
          if (++t == k) {
            t = 0;
            if (e + 1u < hi) S = dp_next_mask(S);
          }
        }
      }
    }
    __syncthreads();
  }
}

// The walk on a filled sub-problem, by the team's first min(T, 64) lanes
// (which lie in one wavefront; the caller keeps the others out): the closing
// edge prices the lowest bit of every word of the m full-set rows (one slice
// per word, so the lowest bit is the word's best); then m - 1 steps back, each
// the smallest predecessor and for it the smallest clock that reaches the
// current (customer, clock) -- tsp_tdp_walk_kernel's two minimisations with its
// (value << 24 | c << 16 | clock) packing.  Lane 0 writes tour[0..m), the
// request's nodes; -> the tour's duration, or 0xffffffff where none fits the
// horizon (the caller owns what tour[] holds then).
template <int T>
VRPMS_DEV uint32_t batch_tdp_walk(const uint64_t* tab, const int32_t* Dl, int m, int W, int ns,
                                  const BatchTdpReq& q, uint32_t members, int tl, bool live, int16_t* tour) {
  constexpr int WL = T < 64 ? T : 64;
  const int M = m + 1, nw = q.lw + 1;
  const uint32_t half = m ? 1u << (m - 1) : 1u;
  uint32_t S = (1u << m) - 1u;
  uint64_t best = ~0ull;
  if (live) {
    for (int e = tl; e < m * nw; e += WL) {
      const int c = e / nw, w = e - c * nw;
      const uint64_t x = tab[(size_t)(c * half + batch_dp_squeeze(S, c)) * W + w];
      if (!x) continue;
      const int brel = 60 * w + __builtin_ctzll(x);
      const int64_t val = (int64_t)brel - q.off + Dl[((w % 24 % ns) * M + c + 1) * M];
      if (val < 0 || val > q.hz) continue;
      const uint64_t cand = ((uint64_t)val << 24) | ((uint64_t)c << 16) | (uint64_t)brel;
      best = cand < best ? cand : best;
    }
  }
#pragma unroll
  for (int o = WL / 2; o > 0; o >>= 1) {
    const uint64_t v = __shfl_xor(best, o, WL);
    best = v < best ? v : best;
  }
  if (best == ~0ull) return 0xffffffffu;
  int c = (int)(best >> 16 & 0xff), brel = (int)(best & 0xffff);
  for (int pos = m - 1; pos >= 1; --pos) {
    if (tl == 0) tour[pos] = (int16_t)batch_tdp_node(members, c + 1);
    S ^= 1u << c;
    const int sw = brel / 60 + 1;   // source words that can reach the clock
    uint64_t step = ~0ull;
    for (int e = tl; e < m * sw; e += WL) {
      const int i = e / sw, w = e - i * sw;
      if (!(S >> i & 1u)) continue;
      const uint64_t x = tab[(size_t)(i * half + batch_dp_squeeze(S, i)) * W + w];
      const int64_t mn = (int64_t)brel - 60 * w - Dl[((w % 24 % ns) * M + i + 1) * M + c + 1];
      if (mn < 0 || mn >= 60 || !(x >> mn & 1ull)) continue;
      const uint64_t cand = ((uint64_t)i << 16) | (uint64_t)(60 * w + mn);
      step = cand < step ? cand : step;
    }
#pragma unroll
    for (int o = WL / 2; o > 0; o >>= 1) {
      const uint64_t v = __shfl_xor(step, o, WL);
      step = v < step ? v : step;
    }
    if (step == ~0ull) return 0xffffffffu;  // unreachable for a table the layers wrote
    c = (int)(step >> 16);
    brel = (int)(step & 0xffff);
  }
  if (tl == 0) tour[0] = (int16_t)batch_tdp_node(members, c + 1);
  return (uint32_t)(best >> 24);
}

}  // namespace vrpms
