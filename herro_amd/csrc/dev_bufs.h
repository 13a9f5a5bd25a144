// dev_bufs.h — the device scratch of one host call (overlap_dev.hip, scan_sort_dev.h, frontend_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace herro {
struct BufsPeak { uint64_t held = 0, peak = 0; };   // bytes several Bufs of one call hold together, and the most they ever held

struct Bufs {   // device allocations of one call, freed together
  std::vector<void*> p;
  BufsPeak* acct = nullptr;   // (optional) where the bytes are counted
  uint64_t bytes_held = 0;
  Bufs() = default;
  explicit Bufs(BufsPeak* a) : acct(a) {}
  Bufs(const Bufs&) = delete;
  Bufs& operator=(const Bufs&) = delete;
  ~Bufs() {
    for (void* q : p) if (q) (void)hipFree(q);
    if (acct) acct->held -= bytes_held;
  }
  template <typename T>
  hipError_t bytes(T** out, uint64_t n) {   // exactly n bytes
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, n);
    if (e == hipSuccess) {
      p.push_back(q);
      bytes_held += n;
      if (acct) { acct->held += n; acct->peak = std::max(acct->peak, acct->held); }
    }
    *out = (T*)q;
    return e;
  }
  template <typename T>   // count elements (at least one) and 64 bytes behind them
  hipError_t get(T** out, uint64_t count) { return bytes(out, std::max<uint64_t>(count, 1) * sizeof(T) + 64); }
};
}  // namespace herro
