// What tsp_tdp.hip shares with vrp_tdsp.hip: the A16 table fill and the
// backward walk, over a subset of the loaded instance's customers from an
// explicit start time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "ctx.hpp"

namespace vrpms {

constexpr int kTdpMaxN = 20;
constexpr int kTdpMaxWords = 512;      // hours per row: 4 wavefronts' accumulators + the matrix < 64 KiB of LDS

// One A16 problem on the loaded matrix: the n customers node[0] < ... (local
// customer bit c = compact node node[c]; node[c] = c + 1 is the whole
// instance's first n), the depot node 0, leaving at `start` with tours of at
// most `horizon` minutes.  W = tdp_words(start, horizon) words per row.
struct TdpProblem {
  int n = 0, start = 0, horizon = 0, W = 0;
  uint8_t node[kTdpMaxN] = {};
};

inline TdpProblem tdp_identity(int n, int start, int horizon, int W) {
  TdpProblem p;
  p.n = n;
  p.start = start;
  p.horizon = horizon;
  p.W = W;
  for (int c = 0; c < n; ++c) p.node[c] = (uint8_t)(c + 1);
  return p;
}

// words per row, or 0 when start + horizon leaves int32 or the row the kernel's limit
inline int tdp_words(int64_t start, int64_t horizon) {
  if (start + horizon >= 2147483648LL) return 0;
  const int64_t W = (start % 60 + horizon) / 60 + 1;
  return W > kTdpMaxWords ? 0 : (int)W;
}

// Enqueue tsp_tdp_init_kernel and one tsp_tdp_layer_kernel per cardinality
// 2..n on `s`: afterwards R[(S n + c) W + w] holds A16's clock set of every
// (S, c), c in S.  The caller has checked the instance (H = 1 or 24, the
// nodes within N), W and the table's size (2^n n W words).
int tsp_tdp_fill(vrpms_ctx* ctx, const TdpProblem& p, uint64_t* R, hipStream_t s);

// Enqueue tsp_tdp_walk_kernel on the filled table: tour[n] (compact nodes, so
// node[c] for local customer c) and key[0] as vrpms_tsp_tdp_run documents.
int tsp_tdp_walk(vrpms_ctx* ctx, const TdpProblem& p, uint64_t* R, int16_t* tour, uint64_t* key,
                 hipStream_t s);

}  // namespace vrpms
