// Host-side launch code the batched exact solvers share (tsp_batch_dp,
// vrp_batch_sp, tsp_batch_tdp, vrp_batch_tdsp): a team of T threads owns one
// request and a 256-thread workgroup holds 256 / T requests.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// One launch of `kernel` for R requests with teams of T: ceil(R / (256 / T))
// workgroups of 256 threads and `lds` bytes of dynamic LDS (above 64 KiB the
// kernel's limit is raised first).
template <class Args>
hipError_t batch_launch(void (*kernel)(Args), const Args& a, int R, int T, size_t lds,
                        hipStream_t s) {
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const int per_wg = 256 / T;
  const unsigned blocks = (unsigned)(((int64_t)R + per_wg - 1) / per_wg);
  kernel<<<blocks, 256, lds, s>>>(a);
  return hipGetLastError();
}

}  // namespace vrpms
