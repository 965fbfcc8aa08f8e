// What tsp_dp.hip shares with vrp_sp.hip: the subset enumeration helpers
// (binomial table for the rank -> mask unrank, Gosper's next mask) and the
// Held-Karp table fill both entry points run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "ctx.hpp"

namespace vrpms {

constexpr int kDpMaxN = 24;
constexpr int kDpNodes = kDpMaxN + 1;

struct DpBinom {
  uint32_t v[kDpNodes][kDpNodes];  // v[c][t] = C(c, t), 0 for t > c
};

constexpr DpBinom dp_make_binom() {
  DpBinom b{};
  for (int c = 0; c < kDpNodes; ++c) {
    b.v[c][0] = 1;
    for (int t = 1; t <= c; ++t) b.v[c][t] = b.v[c - 1][t - 1] + b.v[c - 1][t];
  }
  return b;
}

static constexpr DpBinom kDpBinomHost = dp_make_binom();

// the next larger mask with the same number of set bits (Gosper)
VRPMS_DEV uint32_t dp_next_mask(uint32_t m) {
  const uint32_t c = m & (0u - m), r = m + c;
  return (((r ^ m) >> 2) >> __builtin_ctz(c)) | r;
}

// rank -> mask: the k-subsets of n customers in increasing mask order are the
// combinations c_k > ... > c_1 with rank = sum C(c_t, t) (combinatorial number
// system).  B is a copy of the binomial table with rows of `ld` words,
// B[c * ld + t] = C(c, t), that covers c < n and t <= k.
VRPMS_DEV uint32_t dp_unrank(const uint32_t* B, int ld, int n, int k, uint32_t r) {
  uint32_t S = 0;
  int c = n - 1;
  for (int t = k; t >= 1; --t) {
    while (B[c * ld + t] > r) --c;
    S |= 1u << c;
    r -= B[c * ld + t];
    --c;
  }
  return S;
}

// words per table row: one 64- or 128-byte line
inline int dp_npad(int n) { return n > 16 ? 32 : 16; }

// Enqueue tsp_dp_init_kernel and one tsp_dp_layer_kernel per cardinality
// 1..n-1 on `s`: afterwards g[S][j] (row S, word j-1; dp_npad(n) words per
// row) holds A14's cost-to-go for every S of at most n-1 customers.  The
// caller has checked the instance (static matrix, 1 <= n <= min(24, N-1))
// and the table's size.
int tsp_dp_fill(vrpms_ctx* ctx, int n, uint32_t* g, hipStream_t s);

}  // namespace vrpms
