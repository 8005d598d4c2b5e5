// Integer rounding helpers of the host code.  Plain C++ (nothing from HIP): common.h and the host-only headers
// that a plain g++ program reads (dw_plan.h) share them.
#pragma once
#include <stdint.h>

namespace spp {

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline int cdiv(int64_t x, int64_t m) { return (int)((x + m - 1) / m); }

}  // namespace spp
