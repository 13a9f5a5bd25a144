// dev_bufs.h — the device scratch of one host call (overlap_dev.hip, frontend_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace herro {
struct Bufs {   // device allocations of one call, freed together
  std::vector<void*> p;
  ~Bufs() { for (void* q : p) if (q) (void)hipFree(q); }
  template <typename T>
  hipError_t bytes(T** out, uint64_t n) {   // exactly n bytes
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, n);
    if (e == hipSuccess) p.push_back(q);
    *out = (T*)q;
    return e;
  }
  template <typename T>   // count elements (at least one) and 64 bytes behind them
  hipError_t get(T** out, uint64_t count) { return bytes(out, std::max<uint64_t>(count, 1) * sizeof(T) + 64); }
};
}  // namespace herro
