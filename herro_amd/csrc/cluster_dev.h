// cluster_dev.h — reads clustered by their overlap graph (cluster_dev.hip): the GPU counterpart of scripts/create_clusters.py, which partitions the
// overlap graph with METIS and writes the core / neighbour files that `herro inference -c` reads (lib.rs:208-239).  This is NOT METIS: it is the small
// all-integer specification of DESIGN.md §14 and tests/cluster_ref.py — components over the strong edges, two BFS sweeps from a pseudo-peripheral
// vertex of every component, the order (comp, level, id), a cut of that order by weight — and the kernels equal it field for field, whatever the
// order in which threads claim a vertex.  The argument checks and the part rule are host code: cluster_plan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace herro {

enum { CL_OK = 0, CL_HIP = 1 };

constexpr uint32_t CL_WAVE_DEG = 32;      // a frontier vertex with more arcs than this is expanded by its whole wave, any other by its own thread
constexpr uint32_t CL_LEVEL_BATCH = 64;   // BFS levels queued between two reads of the frontier counter by the host
constexpr uint32_t CL_HOOK_BATCH = 4;     // hook + jump rounds queued between two reads of the change flags

struct ClGraph {             // what stays on the device for the masks; it owns its memory
  uint32_t n = 0, E = 0, k = 0;
  uint32_t* d_a = nullptr;      // [E] the edges as given
  uint32_t* d_b = nullptr;
  uint32_t* d_part = nullptr;   // [n]
  uint8_t* d_mask = nullptr;    // [n] the mask being made
  ClGraph() = default;
  ClGraph(const ClGraph&) = delete;
  ClGraph& operator=(const ClGraph&) = delete;
  void release() {
    for (void* q : {(void*)d_a, (void*)d_b, (void*)d_part, (void*)d_mask}) if (q) (void)hipFree(q);
    d_a = d_b = d_part = nullptr; d_mask = nullptr; n = E = k = 0;
  }
  ~ClGraph() { release(); }
};

struct ClResult {            // host copies
  std::vector<uint32_t> part, rank, comp, level;   // [n]
  uint64_t stats[4] = {0, 0, 0, 0};                // n_components, n_levels, strong_edges, edge_cut
  std::vector<uint64_t> part_stats;                // [k][5]: n_core, weight, n_neighbours, pairs_inside, pairs_touching
};

struct ClTimes {             // HERRO_CLUSTER_STATS: the stages between events, and what the two host loops did
  float arcs_ms = 0, comp_ms = 0, bfs_ms = 0, order_ms = 0, stats_ms = 0;
  uint32_t hook_rounds = 0, bfs_launches = 0, host_reads = 0;
};

// The whole specification for arguments cluster_check passed (n <= 2^31 - 1, E <= 2^31 - 1, ids < n, a != b, 1 <= k <= 65535, T < 2^32).  w, a, b, span:
// host arrays (w NULL: all 1; span NULL: every edge is strong).  Queued on st; returns when the results are on the host.  times: NULL or the split.
int cl_build(uint32_t n, const uint32_t* w, uint32_t E, const uint32_t* a, const uint32_t* b, const uint32_t* span, uint32_t k, uint32_t min_span,
             hipStream_t st, ClGraph& G, ClResult& R, ClTimes* times, std::string& err);

// The mask of part p (1 core, 2 neighbour over all edges, 0 otherwise) into out[n] on the host: two kernels over the resident graph.
int cl_mask(const ClGraph& G, uint32_t p, hipStream_t st, uint8_t* out, std::string& err);

}  // namespace herro
