// cluster_plan.h — the host-only half of herro_cluster_graph / herro_pairs_cluster (include/herro_amd.h, "clusters"; DESIGN.md §14, tests/cluster_ref.py):
// what the call asks of its arguments, and the rule that turns a read's place in the order into its part.  Plain C++17 over integer arrays: no HIP
// call, no context (the part rule is also what k_cl_part of cluster_dev.hip runs: CL_HD).  tools/cluster_plan_check.cpp drives both in a sanitizer build.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/herro_amd.h"

#if defined(__HIPCC__)
#define CL_HD __host__ __device__
#else
#define CL_HD
#endif

namespace herro {

constexpr uint64_t CL_MAX_READS = 0x7fffffffull;   // ids and ranks are 32-bit, 2 E arcs stay inside the sort's 32-bit count
constexpr uint64_t CL_MAX_EDGES = 0x7fffffffull;
constexpr uint32_t CL_MAX_PARTS = 65535;

// step 5 of the specification: S = the weight before the read in the order, T = the total, k parts.  64-bit: S < T < 2^32, k < 2^16.
CL_HD inline uint32_t cluster_part(uint64_t S, uint64_t T, uint32_t k) {
  if (T == 0) return 0;
  const uint64_t p = S * k / T;
  return p < k - 1 ? (uint32_t)p : k - 1;
}

// The checks, in the order of the front end's other entries: HERRO_E_INVALID — the message names the first offending index —, then
// HERRO_E_UNSUPPORTED for the limits.  (HERRO_E_NO_DEVICE on a device-free context comes after both: the caller's.)  *T_out: the total weight.
inline int cluster_check(const char* who, uint64_t n, const uint32_t* w, uint64_t E, const uint32_t* a, const uint32_t* b, const herro_cluster_params* P,
                         uint64_t* T_out, std::string& why) {
  const std::string pre = std::string(who) + ": ";
  if (!P) { why = pre + "params is NULL"; return HERRO_E_INVALID; }
  if (P->n_parts < 1 || P->n_parts > CL_MAX_PARTS) { why = pre + "n_parts = " + std::to_string(P->n_parts) + ": 1 <= n_parts <= 65535"; return HERRO_E_INVALID; }
  if (P->reserved[0] || P->reserved[1]) { why = pre + "reserved fields must be 0"; return HERRO_E_INVALID; }
  if (E && (!a || !b)) { why = pre + "null edge arrays"; return HERRO_E_INVALID; }
  for (uint64_t e = 0; e < E; e++) {
    if (a[e] == b[e]) { why = pre + "edge " + std::to_string(e) + ": a == b = " + std::to_string(a[e]); return HERRO_E_INVALID; }
    if (a[e] >= n || b[e] >= n) {
      why = pre + "edge " + std::to_string(e) + ": read id " + std::to_string(a[e] >= n ? a[e] : b[e]) + " outside the " + std::to_string(n) + " reads";
      return HERRO_E_INVALID;
    }
  }
  if (n > CL_MAX_READS) { why = pre + "more than 2^31 - 1 reads"; return HERRO_E_UNSUPPORTED; }
  if (E > CL_MAX_EDGES) { why = pre + "more than 2^31 - 1 edges"; return HERRO_E_UNSUPPORTED; }
  uint64_t T = w ? 0 : n;
  if (w) for (uint64_t v = 0; v < n; v++) T += w[v];
  if (T >> 32) { why = pre + "the weights sum to " + std::to_string(T) + ": the total must stay below 2^32"; return HERRO_E_UNSUPPORTED; }
  if (T_out) *T_out = T;
  return HERRO_OK;
}

}  // namespace herro
