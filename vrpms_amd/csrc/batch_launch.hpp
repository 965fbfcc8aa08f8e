// Host-side code the batched solvers share.  The exact ones (tsp_batch_dp,
// vrp_batch_sp, tsp_batch_tdp, vrp_batch_tdsp): a team of T threads owns one
// request and a 256-thread workgroup holds 256 / T requests.  The heuristic
// ones (vrp_batch_sa, _ga, _aco, _ls, _lsr, _lsr_spread, _lsf, _lsf_spread,
// tsp_batch_lso, _lso_spread): a workgroup owns a request whose instance lives in LDS
// (batch_stage.hpp has the layout); their argument checks, the LDS refusal,
// the choice of the kernel's matrix type and the launch are below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <string>
#include <type_traits>

#include "ctx.hpp"

namespace vrpms {

inline bool batch_team_ok(int team) {
  return team == 0 || team == 16 || team == 32 || team == 64 || team == 128 || team == 256;
}

// the refusal of a team outside batch_team_ok, in the entry point's name
inline int batch_team_fail(const char* who, int team) {
  return fail(VRPMS_EINVAL, std::string(who) + ": team must be 0 (auto), 16, 32, 64, 128 or 256 (" +
                                std::to_string(team) + " given)");
}

// f(std::integral_constant<int, T>{}) for the run-time team T: the one place
// that turns it into a template argument
template <class F>
hipError_t batch_with_team(int T, F&& f) {
  switch (T) {
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    case 128: return f(std::integral_constant<int, 128>{});
    default: return f(std::integral_constant<int, 256>{});
  }
}

// `kernel`'s limit of dynamic LDS raised to `lds` bytes where that is above the
// 64 KiB every kernel has.  Here and below `what`, when given, is left naming
// the HIP call whose error is returned, for hip_fail.
template <class Args>
hipError_t batch_raise_lds(void (*kernel)(Args), size_t lds, const char** what = nullptr) {
  if (lds <= 65536) return hipSuccess;
  if (what)
    *what = "hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), "
            "hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)";
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// `blocks` workgroups of 256 threads with `lds` bytes of dynamic LDS
template <class Args>
hipError_t batch_enqueue(void (*kernel)(Args), const Args& a, unsigned blocks, size_t lds, hipStream_t s,
                         const char** what = nullptr) {
  if (what) *what = "hipGetLastError()";
  kernel<<<blocks, 256, lds, s>>>(a);
  return hipGetLastError();
}

// One launch of `kernel`: the limit raised where needed, then the launch.
template <class Args>
hipError_t batch_launch_blocks(void (*kernel)(Args), const Args& a, unsigned blocks, size_t lds,
                               hipStream_t s, const char** what = nullptr) {
  const hipError_t e = batch_raise_lds(kernel, lds, what);
  return e != hipSuccess ? e : batch_enqueue(kernel, a, blocks, lds, s, what);
}

// One launch of `kernel` for R requests with teams of T: ceil(R / (256 / T))
// workgroups.
template <class Args>
hipError_t batch_launch(void (*kernel)(Args), const Args& a, int R, int T, size_t lds,
                        hipStream_t s) {
  const int per_wg = 256 / T;
  return batch_launch_blocks(kernel, a, (unsigned)(((int64_t)R + per_wg - 1) / per_wg), lds, s);
}

// ---------------------------------------------------------------------------
// The heuristic solvers.  Every check returns 0 or the refusal's code, with the
// text set in the entry point's name `who`.
// ---------------------------------------------------------------------------
constexpr int kBatchMaxN = 65535;   // tokens and positions are uint16
constexpr int kBatchMaxK = 64;      // one lane per route
constexpr int kBatchMaxS = 65535;   // starts of a local search
constexpr int kBatchMaxG = 65535;   // workgroups per request of a spread one

inline int batch_check_bytes(const char* who, const uint64_t* bytes) {
  return bytes ? VRPMS_OK : fail(VRPMS_EINVAL, std::string(who) + ": bytes is NULL");
}

inline int batch_check_R(const char* who, int32_t R) {
  return R >= 0 ? VRPMS_OK : fail(VRPMS_EINVAL, std::string(who) + ": R must not be negative");
}

// the first two checks of every launch
inline int batch_check_ctx(const char* who, const vrpms_ctx* ctx, int32_t R) {
  if (!ctx) return fail(VRPMS_EINVAL, std::string(who) + ": ctx is NULL");
  return batch_check_R(who, R);
}

inline int batch_check_N(const char* who, int32_t N) {
  if (N < 2 || N > kBatchMaxN)
    return fail(VRPMS_EINVAL, std::string(who) + ": needs 2 <= N <= 65535 (" + std::to_string(N) + " given)");
  return VRPMS_OK;
}

inline int batch_check_K(const char* who, int32_t K) {
  if (K < 1 || K > kBatchMaxK)
    return fail(VRPMS_EINVAL,
                std::string(who) + ": one lane per route needs 1 <= K <= 64 (" + std::to_string(K) + " given)");
  return VRPMS_OK;
}

inline int batch_check_matrix(const char* who, int32_t H, int32_t wide) {
  if (H != 1 && H != 24)
    return fail(VRPMS_EINVAL, std::string(who) + ": H must be 1 or 24 (" + std::to_string(H) + " given)");
  if (wide != 0 && wide != 1)
    return fail(VRPMS_EINVAL, std::string(who) + ": wide must be 0 (uint16 matrix) or 1 (int32) (" +
                                  std::to_string(wide) + " given)");
  return VRPMS_OK;
}

// behind batch_check_matrix, for a solver of static matrices only; `other` is
// the entry point that takes the hour-indexed ones
inline int batch_check_static(const char* who, int32_t H, const char* other) {
  if (H != 1)
    return fail(VRPMS_EINVAL, std::string(who) + ": H must be 1 (" + std::to_string(H) +
                                  " given): an hour-indexed matrix keeps " + other);
  return VRPMS_OK;
}

// the shape of a VRP launch; a solver's own bound (P, A) follows it
inline int batch_check_shape(const char* who, int32_t N, int32_t K, int32_t H, int32_t wide) {
  if (const int rc = batch_check_N(who, N)) return rc;
  if (const int rc = batch_check_K(who, K)) return rc;
  return batch_check_matrix(who, H, wide);
}

inline int batch_check_objective(const char* who, int32_t objective) {
  if (objective != VRPMS_OBJ_SUM && objective != VRPMS_OBJ_MAX)
    return fail(VRPMS_EINVAL, std::string(who) + ": objective must be VRPMS_OBJ_SUM or VRPMS_OBJ_MAX");
  return VRPMS_OK;
}

// 1 <= v <= hi for the S of a local search and the G of a spread one
inline int batch_check_count(const char* who, const char* name, int32_t v, int32_t hi) {
  if (v < 1 || v > hi)
    return fail(VRPMS_EINVAL, std::string(who) + ": 1 <= " + name + " <= " + std::to_string(hi) + " (" +
                                  std::to_string(v) + " given)");
  return VRPMS_OK;
}

inline int batch_check_rounds(const char* who, int32_t rounds) {
  if (rounds < 0)
    return fail(VRPMS_EINVAL,
                std::string(who) + ": rounds must not be negative (" + std::to_string(rounds) + " given)");
  return VRPMS_OK;
}

// `names` is the launch's list of buffers as its refusal spells it
inline int batch_check_buffers(const char* who, const char* names, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (!p) return fail(VRPMS_EINVAL, std::string(who) + ": NULL " + names + " buffer");
  return VRPMS_OK;
}

// A spread launch's workspace, after its buffers: R requests of Gc = min(G, S)
// workgroups, each with a record of `rec` bytes.
inline int batch_check_work(const char* who, int32_t R, int32_t Gc, uint64_t rec, const void* d_work,
                            uint64_t work_bytes) {
  const std::string w(who);
  if ((uint64_t)R * (uint64_t)Gc > 0x7fffffffull)
    return fail(VRPMS_EINVAL, w + ": R * min(G, S) = " + std::to_string((uint64_t)R * (uint64_t)Gc) +
                                  " workgroups are above 2^31 - 1");
  const uint64_t need = (uint64_t)R * (uint64_t)Gc * rec;
  if (!d_work) return fail(VRPMS_EINVAL, w + ": the workspace is NULL");
  if ((uintptr_t)d_work & 7u) return fail(VRPMS_EINVAL, w + ": the workspace must be 8-byte aligned");
  if (work_bytes < need)
    return fail(VRPMS_EINVAL, w + ": the workspace has " + std::to_string(work_bytes) + " bytes, R = " +
                                  std::to_string(R) + " requests of min(G, S) = " + std::to_string(Gc) +
                                  " workgroups need " + std::to_string(need));
  return VRPMS_OK;
}

// A _work entry point past its shape check: G, then R G records of `rec` bytes.
inline int batch_work_bytes(const char* who, int32_t R, int32_t G, uint64_t rec, uint64_t* bytes) {
  if (const int rc = batch_check_count(who, "G", G, kBatchMaxG)) return rc;
  if ((uint64_t)R * (uint64_t)G > 0x7fffffffull)
    return fail(VRPMS_EINVAL, std::string(who) + ": R * G = " + std::to_string((uint64_t)R * (uint64_t)G) +
                                  " records are above 2^31 - 1");
  *bytes = (uint64_t)R * (uint64_t)G * rec;   // < 2^31 2^18
  return VRPMS_OK;
}

// The refusal of a launch whose request does not fit the device's LDS.  K < 0:
// a TSP request, which has no K; `middle` is the owner's clause (" at P = 12").
inline int batch_lds_refusal(const char* who, int32_t N, int32_t K, int32_t H, int32_t wide,
                             const std::string& middle, size_t need, size_t have) {
  return fail(VRPMS_EINVAL, std::string(who) + ": a request of N = " + std::to_string(N) +
                                (K < 0 ? std::string() : ", K = " + std::to_string(K)) + ", H = " +
                                std::to_string(H) + (wide ? " (int32 matrix)" : " (uint16 matrix)") + middle +
                                " needs " + std::to_string(need) + " bytes of LDS (" + std::to_string(have) +
                                " available)");
}

// f(MatT{}, std::integral_constant<int, HM>{}) for the run-time (wide, H): the
// one place that turns them into a kernel's template arguments
template <class F>
hipError_t batch_with_matrix(int wide, int H, F&& f) {
  using H1 = std::integral_constant<int, 1>;
  using H24 = std::integral_constant<int, 24>;
  if (wide) return H == 24 ? f(int32_t{}, H24{}) : f(int32_t{}, H1{});
  return H == 24 ? f(uint16_t{}, H24{}) : f(uint16_t{}, H1{});
}

}  // namespace vrpms
