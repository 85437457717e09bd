// ruleset_shim.h -- TEST INFRASTRUCTURE: what emqx_amd/csrc/gm_ruleset.inc needs beyond
// hip_shim.h (included after it): the workgroup size that lives in gm_kernels.hip and the one
// atomic the kernel's counter phase makes.  One lane runs at a time, so the atomic is a plain add.
#pragma once
#include <stdint.h>

namespace gm {
namespace {
constexpr uint32_t WG = 256;  // gm_kernels.hip
}
}  // namespace gm

static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) {
  const unsigned long long old = *p;
  *p = old + v;
  return old;
}
