// What the one-workgroup-per-request VRP kernels share (vrp_batch_sa.hip, A22;
// vrp_batch_ga.hip, A23; vrp_batch_aco.hip, A24; vrp_batch_ls.hip, A25;
// vrp_batch_lsr.hip and vrp_batch_lsr_spread.hip, A26; vrp_batch_lsf.hip and
// vrp_batch_lsf_spread.hip, A28): the sizes of a request's
// instance in LDS -- one description for the host, which sizes the launch, and
// for a kernel that carves by it (vrp_batch_sa so far; DESIGN.md §4.3u has why
// the others keep their own) -- staging it with the entry check on the way, the
// refusal row, and the final walk of the winning tour.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "tour.hpp"

namespace vrpms {

// x rounded up to a multiple of the power of two `to`
template <typename I>
__host__ __device__ constexpr I batch_align(I x, I to) {
  return (x + (to - 1)) & ~(to - 1);
}

// The parts of a VRP request's instance, with which every kernel's dynamic LDS
// begins, in their order: the [H][N][N] matrix (cells of `cell` bytes, padded to
// 16 bytes), align4(N) demand words, align4(K) capacity words and align4(K)
// start-time words.  The host, which sizes the launch, sums them (bytes()); a
// kernel steps through them (BatchInst): both read the sizes here and nowhere
// else.  I is size_t on the host, which is asked about N up to 65535 (H N N 4
// is then far above 2^32), and uint32_t in a kernel, whose launch has passed
// the LDS check.
template <typename I>
struct BatchInstParts {
  I cells, mat_bytes, dem_words, row_words;
  __host__ __device__ BatchInstParts(I N, I K, I H, I cell) {
    cells = H * N * N;
    mat_bytes = batch_align<I>(cells * cell, 16);
    dem_words = batch_align<I>(N, 4);
    row_words = batch_align<I>(K, 4);
  }
  __host__ __device__ I bytes() const { return mat_bytes + 4 * dem_words + 2 * 4 * row_words; }
};

inline size_t batch_inst_bytes(int N, int K, int H, int wide) {
  return BatchInstParts<size_t>((size_t)N, (size_t)K, (size_t)H, wide ? 4 : 2).bytes();
}

// The kernel's carve of them; the kernel's own parts follow at `rest`.
template <typename MatT, int HM>
struct BatchInst {
  MatT* M;
  int32_t *dem, *cap, *start;
  unsigned char* rest;
  uint32_t cells;
  int N, K;
  using Parts = BatchInstParts<uint32_t>;
  static VRPMS_DEV Parts parts(int N, int K) {
    return Parts((uint32_t)N, (uint32_t)K, (uint32_t)HM, (uint32_t)sizeof(MatT));
  }
  VRPMS_DEV BatchInst(unsigned char* mem, const Parts& l, int N_, int K_) : N(N_), K(K_) {
    cells = l.cells;
    M = reinterpret_cast<MatT*>(mem);
    dem = reinterpret_cast<int32_t*>(mem + l.mat_bytes);
    cap = dem + l.dem_words;
    start = cap + l.row_words;
    rest = reinterpret_cast<unsigned char*>(start + l.row_words);
  }
};

// Request r's [HM][N][N] int32 matrix into M (as MatT), its demand row and its
// two fleet rows into dem / cap / start.  -> whether the request is outside
// the launch's promise (a negative entry, or one above 65535 under uint16
// cells), the same for every thread.  The verdict goes through `flag`, a word
// of the dynamic LDS that is free for any other use after the call:
// __syncthreads_or would add static LDS on top of the bytes the kernel's _lds
// function promises.  Every thread of the block must call it.
template <typename MatT>
VRPMS_DEV bool batch_stage_request(const int32_t* mats, const int32_t* demand, const int32_t* gcap,
                                   const int32_t* gstart, int64_t r, uint32_t cells, int N, int K,
                                   MatT* M, int32_t* dem, int32_t* cap, int32_t* start,
                                   uint32_t* flag) {
  const int32_t* src = mats + r * (int64_t)cells;
  if (threadIdx.x == 0) *flag = 0;
  __syncthreads();
  bool bad = false;
  for (uint32_t i = threadIdx.x; i < cells; i += 256) {
    const int32_t v = src[i];
    bad |= v < 0 || (sizeof(MatT) == 2 && v > 65535);
    M[i] = (MatT)v;
  }
  for (int i = threadIdx.x; i < N; i += 256) dem[i] = demand[r * N + i];
  for (int k = threadIdx.x; k < K; k += 256) {
    cap[k] = gcap[r * K + k];
    start[k] = gstart[r * K + k];
  }
  if (bad) *flag = 1;
  __syncthreads();
  bad = *flag != 0;
  __syncthreads();   // every wavefront has read the word before anything replaces it
  return bad;
}

// the same from a kernel's argument struct `a` (any of them) into its carve
template <typename Args, typename MatT, int HM>
VRPMS_DEV bool batch_stage_request(const Args& a, int64_t r, const BatchInst<MatT, HM>& c, void* flag) {
  return batch_stage_request(a.mats, a.demand, a.cap, a.start, r, c.cells, c.N, c.K, c.M, c.dem, c.cap,
                             c.start, static_cast<uint32_t*>(flag));
}

// The refusal row of a request outside the launch's promise: an all-ones key,
// a zero tour, zero durations and vehicles of -1.
VRPMS_DEV void batch_refuse(uint16_t* gtour, int8_t* gveh, int32_t* gdurs, uint64_t* gkey, int ntok,
                            int K) {
  for (int q = threadIdx.x; q < ntok; q += 256) {
    gtour[q] = 0;
    gveh[q] = -1;
  }
  for (int k = threadIdx.x; k < K; k += 256) gdurs[k] = 0;
  if (threadIdx.x == 0) *gkey = ~0ull;
}

// One wavefront walks `tour` (ntok tokens, 0 a separator) as spec.eval_cvrp
// does: every lane walks alike, lane k keeps route k's duration (the return
// value), lane 0 notes every token's vehicle in V (-1 unvisited, -2 separator).
template <typename Mat>
VRPMS_DEV int batch_final_walk(const Mat& D, const int32_t* dem, const int32_t* cap,
                               const int32_t* start, int K, int n, const uint16_t* tour, int ntok,
                               int16_t* V, int lane) {
  int mydur = 0;
  int k = 0, load = 0, t = start[0], prev = 0;
  auto close_route = [&]() {
    if (prev) {
      t += D(t, (uint32_t)prev, 0);
      if (lane == k) mydur = t - start[k];
    }
    ++k;
    if (k < K) {
      load = 0;
      t = start[k];
      prev = 0;
    }
  };
  for (int i = 0; i < ntok; ++i) {
    const int c = (int)min((uint32_t)tour[i], (uint32_t)n);
    int v;
    if (c == 0) {
      v = -2;
      if (k < K) close_route();
    } else {
      const int dc = dem[c];
      while (k < K && load + dc > cap[k]) close_route();
      if (k < K) {
        t += D(t, (uint32_t)prev, (uint32_t)c);
        load += dc;
        prev = c;
        v = k;
      } else {
        v = -1;
      }
    }
    if (lane == 0) V[i] = (int16_t)v;
  }
  if (k < K) close_route();
  return mydur;
}

}  // namespace vrpms
