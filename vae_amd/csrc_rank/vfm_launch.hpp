// vfm_launch.hpp -- the status of the launch just made, for every unit of csrc_rank/ (included at file scope).
#pragma once

#include <hip/hip_runtime.h>

namespace vfm {
int fail_hip(hipError_t e, const char* where);          // (vfm_abi.hip: the thread's vfm_last_error() text)
}  // namespace vfm

inline int launch_status(const char* where) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vfm::fail_hip(e, where);
}
