// What tsp_batch_dp.hip shares with vrp_batch_sp.hip: the LDS image of one
// small request's matrix and the fill of its compact Held-Karp table by a
// team of T threads.
//
// The table is compact: g[S][j] exists only for j outside S, so customer j's
// states are indexed by c = S with bit j squeezed out, 2^(n-1) words per
// customer, n 2^(n-1) words in all, in the order [j][c] (customer major).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "tsp_dp.hpp"

namespace vrpms {

// Why 12: the compact table has n 2^(n-1) 32-bit words, 98,304 B at n = 12;
// with the 13 x 16-word matrix image (832 B) and the binomial table (704 B)
// that is 99,840 B, within ctx->max_lds (160 KiB per CU).  At n = 13 the table
// alone is 13 * 4096 * 4 = 212,992 B, which does not fit.
constexpr int kBatchDpMaxN = 12;
constexpr int kBatchDpNodes = kBatchDpMaxN + 1;
constexpr int kBatchDpRow = 16;     // words per matrix row in LDS: three 16-byte reads per row
constexpr int kBatchDpBinomWords = (kBatchDpNodes * kBatchDpNodes + 3) & ~3;
constexpr int kBatchDpMatWords = kBatchDpNodes * kBatchDpRow;
constexpr uint32_t kBatchDpOut = 0x80000000u;   // h of a customer outside S

// words of the compact table, padded to 16 bytes
inline size_t batch_dp_table_words(int n) { return (((size_t)n << (n - 1)) + 3) & ~(size_t)3; }

// S with bit b squeezed out
VRPMS_DEV uint32_t batch_dp_squeeze(uint32_t S, int b) {
  return (S & ((1u << b) - 1u)) | ((S >> (b + 1)) << b);
}

// The workgroup's copy of the binomial table: B[c][t] = C(c, t), rows of
// kBatchDpNodes words.  The caller's barrier publishes it.
VRPMS_DEV void batch_dp_stage_binom(const DpBinom& binom, uint32_t* B) {
  for (int e = threadIdx.x; e < kBatchDpNodes * kBatchDpNodes; e += 256)
    B[e] = binom.v[e / kBatchDpNodes][e % kBatchDpNodes];
}

// Lane tl of a team of T stages its request's matrix D [N][N] as
// Dr[node][i] = D[node][i + 1] and the empty set's column g[j][0] = D[j + 1][0].
template <int T>
VRPMS_DEV void batch_dp_stage(const int32_t* D, int N, int tl, uint32_t* Dr, uint32_t* g) {
  const int n = N - 1;
  const uint32_t half = 1u << (n - 1);
  for (int e = tl; e < kBatchDpMatWords; e += T) {
    const int node = e / kBatchDpRow, i = e % kBatchDpRow;
    Dr[e] = (node <= n && i < n) ? (uint32_t)D[node * N + i + 1] : 0u;
  }
  for (int j = tl; j < n; j += T) g[j * half] = (uint32_t)D[(j + 1) * N];   // the empty set
}

// The layers k = 1..n-1 of the table, one workgroup-wide barrier after each
// (every team of the workgroup has the same n).  A thread takes a run of
// consecutive ranks of the layer's k-subsets: dp_unrank for the first mask,
// dp_next_mask from there.  For its subset S it loads h[i] = g[S \ {i}][i]
// once (kBatchDpOut for i outside S: above every real cost, and D + h cannot
// wrap since D < 2^31), then for every j outside S reads row j of the matrix
// from LDS and stores min over i of D[j][i] + h[i].  An inactive team has no
// subsets: it only keeps the barrier's count.
template <int T>
VRPMS_DEV void batch_dp_fill(const uint32_t* B, const uint32_t* Dr, uint32_t* g, int n, int tl,
                             bool active) {
  const uint32_t half = 1u << (n - 1), full = (1u << n) - 1u;
  for (int k = 1; k < n; ++k) {
    const uint32_t count = active ? B[n * kBatchDpNodes + k] : 0u;
    const uint32_t chunk = (count + T - 1) / T;
    const uint32_t lo = tl * chunk;
    const uint32_t hi = lo + chunk < count ? lo + chunk : count;
    if (lo < hi) {
      uint32_t S = dp_unrank(B, kBatchDpNodes, n, k, lo);
      for (uint32_t r = lo; r < hi; ++r) {
        uint32_t h[kBatchDpMaxN];
#pragma unroll
        for (int i = 0; i < kBatchDpMaxN; ++i)
          h[i] = ((S >> i) & 1u) ? g[i * half + batch_dp_squeeze(S, i)] : kBatchDpOut;
        for (uint32_t m = full & ~S; m; m &= m - 1u) {
          const int j = __builtin_ctz(m);
          const v4u* row = reinterpret_cast<const v4u*>(Dr + (j + 1) * kBatchDpRow);
          const v4u r0 = row[0];
          uint32_t best = min(min(r0.x + h[0], r0.y + h[1]), min(r0.z + h[2], r0.w + h[3]));
          if (n > 4) {
            const v4u r1 = row[1];
            best = min(best, min(min(r1.x + h[4], r1.y + h[5]), min(r1.z + h[6], r1.w + h[7])));
          }
          if (n > 8) {
            const v4u r2 = row[2];
            best = min(best, min(min(r2.x + h[8], r2.y + h[9]), min(r2.z + h[10], r2.w + h[11])));
          }
          g[j * half + batch_dp_squeeze(S, j)] = best;
        }
        S = dp_next_mask(S);
      }
    }
    __syncthreads();
  }
}

}  // namespace vrpms
