// pg_fail.hpp -- how every unit of libpong_ga.so reports a failure.  No HIP
// header: pg_hof_scan.cpp is plain host C++ (PG_HIP is for the units that have one).
#pragma once

#include <stdint.h>

namespace pg {

// Record a failure for pg_last_error() and return code (defined in pong_ga.hip).
int32_t fail(int32_t code, const char *fmt, ...);

#define PG_HIP(call)                                                                  \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fail(PG_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));        \
  } while (0)

}  // namespace pg
