// cluster_dev.hip — the overlap graph's clusters on the device (cluster_dev.h; specification: DESIGN.md §14, tests/cluster_ref.py).  Stages:
//   k_cl_arcs        the 2 E arcs of the E edges: key = src << 32 | dst, payload = strong; degrees by integer atomicAdd.  Sorted by src with the finder's
//                    stable radix sort (dev_radix_sort), offsets by the scan (dev_scan_u32; scan_sort_dev.h): the CSR, adj = dst | strong << 31.
//   k_cl_hook, k_cl_jump   components: every strong arc hooks the larger label (and its label's label) to the smaller by atomicMin, then every label
//                    jumps to its label's label until it stands.  Labels only fall and stay inside their component, so the fixed point — a round
//                    whose flag stays clear — is the least id of the component, whatever the order.
//   k_cl_bfs         one level of a level-synchronous BFS over the strong arcs, all components at once: a vertex is claimed by atomicCAS on its
//                    distance, so the value is the distance whoever wins; the claimer appends it to the next frontier (the frontier's ORDER is
//                    arbitrary, nothing reads it).  A frontier vertex of up to CL_WAVE_DEG arcs is walked by its thread, a larger one by its wave.
//                    Frontier sizes are device counters: CL_LEVEL_BATCH levels are queued between two reads by the host.
//   k_cl_far         far[c] by a 64-bit atomicMax of d1 << 32 | ~v.
//   k_cl_keys        key = comp << 32 | level, payload = v: sorted by the level's digits, then by the component's, stable from ids in ascending order.
//   k_cl_rank, k_cl_part   rank, the weights in order, their scan, the part rule (cluster_plan.h), cores and weight per part.
//   k_cl_edge_stats, k_cl_nb_keys, k_cl_nb_heads   pairs inside / touching per part and the cut; neighbours per part = distinct (part[src], dst) with
//                    part[dst] != part[src] (the other arcs: part k, which no read has): sorted over all their bits, heads counted.
//   k_cl_mask_core, k_cl_mask_nb   a mask on demand.
// Nothing an atomic orders reaches the output: atomics are integer sums, minima, maxima and claims whose winner does not matter.
#include "cluster_dev.h"

#include <algorithm>

#include "cluster_plan.h"
#include "dev_bufs.h"
#include "scan_sort_dev.h"

namespace herro {
namespace {

constexpr uint32_t INF32 = 0xffffffffu;
constexpr uint32_t STRONG = 0x80000000u;     // adj: bit 31 (ids are below 2^31)
constexpr uint32_t LDS_PARTS = 1024;         // k_cl_edge_stats: up to this many parts are summed in LDS first

__device__ inline uint32_t ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void add64(uint64_t* p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

// sum of v over the lanes that are `on`, in every lane
__device__ inline uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// rows[p * 5 + c] += v for the lanes that are `on`: one atomic per wave where all of them name the same row (the order is sorted by part)
__device__ inline void row_add(uint64_t* rows, uint32_t p, uint32_t c, uint64_t v, bool on) {
  const uint64_t m = __ballot(on);
  if (!m) return;
  const int first = __ffsll((long long)m) - 1;
  const uint32_t p0 = __shfl(p, first, 64);
  const bool same = __ballot(on && p != p0) == 0;
  if (same) {
    const uint64_t s = wave_sum(on ? v : 0);
    if ((int)(threadIdx.x & 63) == first && s) add64(&rows[(uint64_t)p0 * 5 + c], s);
  } else if (on && v) {
    add64(&rows[(uint64_t)p * 5 + c], v);
  }
}

__global__ __launch_bounds__(256) void k_cl_arcs(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ span,
                                                 uint32_t E, uint32_t min_span, uint64_t* __restrict__ keys, uint64_t* __restrict__ pays,
                                                 uint32_t* __restrict__ deg, uint64_t* __restrict__ n_strong) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  bool strong = false;
  if (e < E) {
    const uint32_t x = a[e], y = b[e];
    strong = span ? span[e] >= min_span : true;
    keys[2ull * e] = ((uint64_t)x << 32) | y;
    keys[2ull * e + 1] = ((uint64_t)y << 32) | x;
    pays[2ull * e] = pays[2ull * e + 1] = strong;
    atomicAdd(&deg[x], 1u);
    atomicAdd(&deg[y], 1u);
  }
  const uint64_t m = __ballot(strong);
  if ((threadIdx.x & 63) == 0 && m) add64(n_strong, (uint64_t)__popcll(m));
}

__global__ __launch_bounds__(256) void k_cl_adj(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ pays, uint32_t m,
                                                uint32_t* __restrict__ adj) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < m) adj[i] = (uint32_t)keys[i] | ((pays[i] & 1u) ? STRONG : 0u);
}

__global__ __launch_bounds__(256) void k_cl_iota(uint32_t* __restrict__ label, uint32_t n) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v < n) label[v] = v;
}

// one thread per arc u -> v (both directions are arcs, so only "v's label is smaller" is handled)
__global__ __launch_bounds__(256) void k_cl_hook(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ adj, uint32_t m,
                                                 uint32_t* __restrict__ label, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const uint32_t x = adj[i];
  if (!(x & STRONG)) return;
  const uint32_t u = (uint32_t)(keys[i] >> 32), v = x & ~STRONG;
  const uint32_t lu = ld(&label[u]), lv = ld(&label[v]);
  if (lv < lu) {
    atomicMin(&label[lu], lv);
    atomicMin(&label[u], lv);
    *flag = 1u;
  }
}

__global__ __launch_bounds__(256) void k_cl_jump(uint32_t* __restrict__ label, uint32_t n) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  uint32_t l = ld(&label[v]);
  for (;;) {                      // labels only fall: at most l steps
    const uint32_t ll = ld(&label[l]);
    if (ll == l) break;
    l = ll;
  }
  label[v] = l;
}

// the sources of the first sweep: the roots (comp[v] == v)
__global__ __launch_bounds__(256) void k_cl_src_roots(const uint32_t* __restrict__ comp, uint32_t n, uint32_t* __restrict__ dist,
                                                      uint32_t* __restrict__ q, uint32_t* __restrict__ cnt) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  if (comp[v] == v) { dist[v] = 0; q[atomicAdd(cnt, 1u)] = v; }
  else dist[v] = INF32;
}

__global__ __launch_bounds__(256) void k_cl_far(const uint32_t* __restrict__ comp, const uint32_t* __restrict__ d1, uint32_t n,
                                                unsigned long long* __restrict__ far) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v < n) atomicMax(&far[comp[v]], ((unsigned long long)d1[v] << 32) | (uint32_t)~v);
}

// the sources of the second sweep: far[c] of every root c (dist is all INF32 before)
__global__ __launch_bounds__(256) void k_cl_src_far(const uint32_t* __restrict__ comp, const unsigned long long* __restrict__ far, uint32_t n,
                                                    uint32_t* __restrict__ dist, uint32_t* __restrict__ q, uint32_t* __restrict__ cnt) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n || comp[v] != v) return;
  const uint32_t f = ~(uint32_t)far[v];     // (a vertex of component v: below n)
  dist[f] = 0;
  q[atomicAdd(cnt, 1u)] = f;
}

__device__ inline void bfs_visit(uint32_t x, uint32_t level, uint32_t* __restrict__ dist, uint32_t* __restrict__ qout, uint32_t* __restrict__ nout) {
  if (!(x & STRONG)) return;
  const uint32_t v = x & ~STRONG;
  if (ld(&dist[v]) != INF32) return;
  if (atomicCAS(&dist[v], INF32, level) == INF32) qout[atomicAdd(nout, 1u)] = v;   // claimed once in a sweep: at most n entries in all
}

// one level: the frontier qin[0 .. *nin) -> qout[0 .. *nout), dist = level for the claimed
__global__ __launch_bounds__(256) void k_cl_bfs(const uint32_t* __restrict__ off, const uint32_t* __restrict__ adj, uint32_t* __restrict__ dist,
                                                const uint32_t* __restrict__ qin, uint32_t* __restrict__ qout, const uint32_t* __restrict__ nin,
                                                uint32_t* __restrict__ nout, uint32_t level) {
  const uint32_t nf = *nin;
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < nf; base += (uint64_t)gridDim.x * 256) {   // (uniform in a wave)
    const uint64_t i = base + lane;
    uint32_t s = 0, e = 0;
    if (i < nf) { const uint32_t u = qin[i]; s = off[u]; e = off[u + 1]; }
    const bool heavy = e - s > CL_WAVE_DEG;
    if (!heavy) for (uint32_t x = s; x < e; x++) bfs_visit(adj[x], level, dist, qout, nout);
    uint64_t hm = __ballot(heavy);
    while (hm) {                                   // a vertex above the threshold: its arcs over the 64 lanes
      const int src = __ffsll((long long)hm) - 1;
      hm &= hm - 1;
      const uint32_t hs = __shfl(s, src, 64), he = __shfl(e, src, 64);
      for (uint32_t x = hs + lane; x < he; x += 64) bfs_visit(adj[x], level, dist, qout, nout);
    }
  }
}

__global__ __launch_bounds__(256) void k_cl_keys(const uint32_t* __restrict__ comp, const uint32_t* __restrict__ level, uint32_t n,
                                                 uint64_t* __restrict__ keys, uint64_t* __restrict__ pays, uint32_t* __restrict__ n_levels) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  uint32_t top = 0;
  if (v < n) {
    keys[v] = ((uint64_t)comp[v] << 32) | level[v];
    pays[v] = v;
    top = level[v] + 1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) top = max(top, (uint32_t)__shfl_xor(top, o, 64));
  if ((threadIdx.x & 63) == 0 && top) atomicMax(n_levels, top);
}

__global__ __launch_bounds__(256) void k_cl_rank(const uint64_t* __restrict__ order, const uint32_t* __restrict__ w, uint32_t n,
                                                 uint32_t* __restrict__ rank, uint32_t* __restrict__ wo) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t v = (uint32_t)order[i];
  rank[v] = i;
  wo[i] = w ? w[v] : 1u;
}

__global__ __launch_bounds__(256) void k_cl_part(const uint64_t* __restrict__ order, const uint32_t* __restrict__ S, const uint32_t* __restrict__ wo,
                                                 uint32_t n, uint32_t k, uint32_t* __restrict__ part, uint64_t* __restrict__ rows) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool on = i < n;
  uint32_t p = 0, wv = 0;
  if (on) {
    p = cluster_part(S[i], S[n], k);
    wv = wo[i];
    part[(uint32_t)order[i]] = p;
  }
  row_add(rows, p, 0, 1, on);
  row_add(rows, p, 1, wv, on);
}

// pairs inside (column 3) and touching (column 4) per part, and the cut
__global__ __launch_bounds__(256) void k_cl_edge_stats(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t E,
                                                       const uint32_t* __restrict__ part, uint32_t k, uint64_t* __restrict__ rows,
                                                       uint64_t* __restrict__ cut) {
  __shared__ uint32_t lds[2 * LDS_PARTS];
  const bool in_lds = k <= LDS_PARTS;
  if (in_lds) {
    for (uint32_t x = threadIdx.x; x < 2 * k; x += 256) lds[x] = 0;
    __syncthreads();
  }
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  bool crosses = false;
  if (e < E) {
    const uint32_t pa = part[a[e]], pb = part[b[e]];
    crosses = pa != pb;
    if (in_lds) {
      if (!crosses) atomicAdd(&lds[2 * pa], 1u);
      atomicAdd(&lds[2 * pa + 1], 1u);
      if (crosses) atomicAdd(&lds[2 * pb + 1], 1u);
    } else {
      if (!crosses) add64(&rows[(uint64_t)pa * 5 + 3], 1);
      add64(&rows[(uint64_t)pa * 5 + 4], 1);
      if (crosses) add64(&rows[(uint64_t)pb * 5 + 4], 1);
    }
  }
  const uint64_t m = __ballot(crosses);
  if ((threadIdx.x & 63) == 0 && m) add64(cut, (uint64_t)__popcll(m));
  if (in_lds) {
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < 2 * k; x += 256)
      if (lds[x]) add64(&rows[(uint64_t)(x >> 1) * 5 + 3 + (x & 1u)], lds[x]);
  }
}

// arc i of edge i / 2: dst is a neighbour of part[src] when its own part is another.  An arc inside a part gets the part k, which no read has: the
// sort covers bits_of(k) bits of that field, so such a key differs from every real one in a digit the sort looks at, wherever dst falls.
__global__ __launch_bounds__(256) void k_cl_nb_keys(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t m,
                                                    const uint32_t* __restrict__ part, uint32_t k, uint64_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const uint32_t e = i >> 1;
  const uint32_t src = (i & 1u) ? b[e] : a[e], dst = (i & 1u) ? a[e] : b[e];
  const uint32_t ps = part[src];
  keys[i] = ((uint64_t)(ps != part[dst] ? ps : k) << 32) | dst;
}

__global__ __launch_bounds__(256) void k_cl_nb_heads(const uint64_t* __restrict__ keys, uint32_t m, uint32_t k, uint64_t* __restrict__ rows) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool head = false;
  uint32_t p = 0;
  if (i < m) {
    const uint64_t key = keys[i];
    p = (uint32_t)(key >> 32);
    head = p != k && (i == 0 || keys[i - 1] != key);
  }
  row_add(rows, p, 2, 1, head);
}

__global__ __launch_bounds__(256) void k_cl_mask_core(const uint32_t* __restrict__ part, uint32_t n, uint32_t p, uint8_t* __restrict__ mask) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v < n) mask[v] = part[v] == p ? 1 : 0;
}

// (every writer of a byte writes the same 2, and only into a read that is not core)
__global__ __launch_bounds__(256) void k_cl_mask_nb(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t E,
                                                    const uint32_t* __restrict__ part, uint32_t p, uint8_t* __restrict__ mask) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const uint32_t x = a[e], y = b[e];
  const bool cx = part[x] == p, cy = part[y] == p;
  if (cx && !cy) mask[y] = 2;
  if (cy && !cx) mask[x] = 2;
}

#define CL_TRY(expr)                                                                  \
  do {                                                                                \
    const hipError_t _e = (expr);                                                     \
    if (_e != hipSuccess) {                                                           \
      err = std::string("clusters: " #expr ": ") + hipGetErrorString(_e);             \
      return CL_HIP;                                                                  \
    }                                                                                 \
  } while (0)

struct Events {              // the stage timers (HERRO_CLUSTER_STATS): nothing is recorded without `on`
  bool on = false;
  hipEvent_t ev[6] = {};
  ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  hipError_t init() {
    for (hipEvent_t& e : ev) { const hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return r; }
    on = true;
    return hipSuccess;
  }
  hipError_t mark(int i, hipStream_t st) { return on ? hipEventRecord(ev[i], st) : hipSuccess; }
};

// A sweep from the sources already in q0 (their count in cnt[0], their dist 0, every other dist INF32).  *levels: an upper bound of the levels it found.
int bfs(const uint32_t* off, const uint32_t* adj, uint32_t n, uint32_t* dist, uint32_t* q0, uint32_t* q1, uint32_t* cnt, hipStream_t st, uint32_t* levels,
        ClTimes* times, std::string& err) {
  const uint32_t grid = std::min<uint32_t>(nblk(n), 1024);
  uint32_t level = 0;
  for (;;) {
    CL_TRY(hipMemsetAsync(cnt + 1, 0, 4ull * CL_LEVEL_BATCH, st));
    for (uint32_t i = 0; i < CL_LEVEL_BATCH; i++) {
      k_cl_bfs<<<grid, 256, 0, st>>>(off, adj, dist, q0, q1, cnt + i, cnt + i + 1, level + i + 1);
      std::swap(q0, q1);
    }
    CL_TRY(hipGetLastError());
    uint32_t left = 0;
    CL_TRY(hipMemcpyAsync(&left, cnt + CL_LEVEL_BATCH, 4, hipMemcpyDeviceToHost, st));
    CL_TRY(hipStreamSynchronize(st));
    level += CL_LEVEL_BATCH;
    if (times) { times->bfs_launches += CL_LEVEL_BATCH; times->host_reads++; }
    if (!left || level >= n) break;      // (a distance is below n)
    CL_TRY(hipMemcpyAsync(cnt, cnt + CL_LEVEL_BATCH, 4, hipMemcpyDeviceToDevice, st));
  }
  *levels = level;
  return CL_OK;
}

}  // namespace

int cl_build(uint32_t n, const uint32_t* w, uint32_t E, const uint32_t* a, const uint32_t* b, const uint32_t* span, uint32_t k, uint32_t min_span,
             hipStream_t st, ClGraph& G, ClResult& R, ClTimes* times, std::string& err) {
  G.release();
  R.part.assign(n, 0); R.rank.assign(n, 0); R.comp.assign(n, 0); R.level.assign(n, 0);
  R.part_stats.assign((size_t)k * 5, 0);
  for (uint64_t& s : R.stats) s = 0;
  G.k = k;
  if (n == 0) return CL_OK;     // (no read: no edge either)
  const uint32_t m = 2 * E;     // arcs (E <= 2^31 - 1)
  Events T;
  if (times) CL_TRY(T.init());
  Bufs B;
  // ---- what stays
  CL_TRY(hipMalloc((void**)&G.d_a, 4ull * std::max(E, 1u)));
  CL_TRY(hipMalloc((void**)&G.d_b, 4ull * std::max(E, 1u)));
  CL_TRY(hipMalloc((void**)&G.d_part, 4ull * n));
  CL_TRY(hipMalloc((void**)&G.d_mask, n));
  G.n = n; G.E = E;
  // ---- scratch of the call
  const uint64_t cap = std::max<uint64_t>(m, n);
  uint64_t *k0, *p0, *k1, *p1, *d_rows, *d_g;
  unsigned long long* d_far;
  uint32_t *d_span = nullptr, *d_w = nullptr, *d_deg, *d_off, *d_adj, *d_label, *d_d1, *d_level, *d_q0, *d_q1, *d_cnt, *d_flag, *d_sort, *d_partial, *d_rank, *d_wo,
           *d_S, *d_nlev;
  CL_TRY(B.get(&k0, cap)); CL_TRY(B.get(&p0, cap)); CL_TRY(B.get(&k1, cap)); CL_TRY(B.get(&p1, cap));
  CL_TRY(B.get(&d_rows, (uint64_t)k * 5));
  CL_TRY(B.get(&d_g, 2));                      // strong edges, edge cut
  CL_TRY(B.get(&d_far, n));
  if (span) CL_TRY(B.get(&d_span, E));
  if (w) CL_TRY(B.get(&d_w, n));
  CL_TRY(B.get(&d_deg, n)); CL_TRY(B.get(&d_off, (uint64_t)n + 1)); CL_TRY(B.get(&d_adj, m));
  CL_TRY(B.get(&d_label, n)); CL_TRY(B.get(&d_d1, n)); CL_TRY(B.get(&d_level, n)); CL_TRY(B.get(&d_q0, n)); CL_TRY(B.get(&d_q1, n));
  CL_TRY(B.get(&d_cnt, CL_LEVEL_BATCH + 1)); CL_TRY(B.get(&d_flag, CL_HOOK_BATCH)); CL_TRY(B.get(&d_nlev, 1));
  CL_TRY(B.get(&d_sort, dev_sort_scratch(cap)));
  CL_TRY(B.get(&d_partial, (uint64_t)dev_scan_partials(n) + 1));
  CL_TRY(B.get(&d_rank, n)); CL_TRY(B.get(&d_wo, n)); CL_TRY(B.get(&d_S, (uint64_t)n + 1));
  if (E) {
    CL_TRY(hipMemcpyAsync(G.d_a, a, 4ull * E, hipMemcpyHostToDevice, st));
    CL_TRY(hipMemcpyAsync(G.d_b, b, 4ull * E, hipMemcpyHostToDevice, st));
    if (span) CL_TRY(hipMemcpyAsync(d_span, span, 4ull * E, hipMemcpyHostToDevice, st));
  }
  if (w) CL_TRY(hipMemcpyAsync(d_w, w, 4ull * n, hipMemcpyHostToDevice, st));
  CL_TRY(hipMemsetAsync(d_rows, 0, 40ull * k, st));
  CL_TRY(hipMemsetAsync(d_g, 0, 16, st));
  CL_TRY(hipMemsetAsync(d_far, 0, 8ull * n, st));
  CL_TRY(hipMemsetAsync(d_deg, 0, 4ull * n, st));
  CL_TRY(hipMemsetAsync(d_nlev, 0, 4, st));
  CL_TRY(T.mark(0, st));
  // ---- CSR of the arcs
  const uint32_t id_bits = bits_of(n - 1);
  if (E) {
    k_cl_arcs<<<nblk(E), 256, 0, st>>>(G.d_a, G.d_b, d_span, E, min_span, k0, p0, d_deg, d_g);
    CL_TRY(hipGetLastError());
    std::vector<uint32_t> sh;
    field_shifts(sh, 32, id_bits);
    if (dev_radix_sort(&k0, &p0, &k1, &p1, m, sh, d_sort, st, err)) return CL_HIP;
    k_cl_adj<<<nblk(m), 256, 0, st>>>(k0, p0, m, d_adj);
    CL_TRY(hipGetLastError());
  }
  if (dev_scan_u32(d_deg, n, d_off, d_partial, st, err)) return CL_HIP;
  CL_TRY(T.mark(1, st));
  // ---- components (k0: the sorted arcs' keys, their src in the high half)
  k_cl_iota<<<nblk(n), 256, 0, st>>>(d_label, n);
  CL_TRY(hipGetLastError());
  for (uint64_t round = 0; E;) {
    CL_TRY(hipMemsetAsync(d_flag, 0, 4ull * CL_HOOK_BATCH, st));
    for (uint32_t i = 0; i < CL_HOOK_BATCH; i++) {
      k_cl_hook<<<nblk(m), 256, 0, st>>>(k0, d_adj, m, d_label, d_flag + i);
      k_cl_jump<<<nblk(n), 256, 0, st>>>(d_label, n);
    }
    CL_TRY(hipGetLastError());
    uint32_t flags[CL_HOOK_BATCH];
    CL_TRY(hipMemcpyAsync(flags, d_flag, 4ull * CL_HOOK_BATCH, hipMemcpyDeviceToHost, st));
    CL_TRY(hipStreamSynchronize(st));
    round += CL_HOOK_BATCH;
    if (times) { times->hook_rounds += CL_HOOK_BATCH; times->host_reads++; }
    if (!flags[CL_HOOK_BATCH - 1]) break;      // a round that changed nothing: the fixed point
    if (round > (uint64_t)n + CL_HOOK_BATCH) { err = "clusters: the component labels did not settle"; return CL_HIP; }   // (every round but the last lowers a label)
  }
  CL_TRY(T.mark(2, st));
  // ---- two sweeps
  uint32_t levels1 = 0, levels2 = 0;
  CL_TRY(hipMemsetAsync(d_cnt, 0, 4, st));
  k_cl_src_roots<<<nblk(n), 256, 0, st>>>(d_label, n, d_d1, d_q0, d_cnt);
  CL_TRY(hipGetLastError());
  uint32_t n_comp = 0;
  CL_TRY(hipMemcpyAsync(&n_comp, d_cnt, 4, hipMemcpyDeviceToHost, st));   // (read by the sweep's first synchronisation)
  if (int rc = bfs(d_off, d_adj, n, d_d1, d_q0, d_q1, d_cnt, st, &levels1, times, err)) return rc;
  k_cl_far<<<nblk(n), 256, 0, st>>>(d_label, d_d1, n, d_far);
  CL_TRY(hipMemsetAsync(d_level, 0xff, 4ull * n, st));
  CL_TRY(hipMemsetAsync(d_cnt, 0, 4, st));
  k_cl_src_far<<<nblk(n), 256, 0, st>>>(d_label, d_far, n, d_level, d_q0, d_cnt);
  CL_TRY(hipGetLastError());
  if (int rc = bfs(d_off, d_adj, n, d_level, d_q0, d_q1, d_cnt, st, &levels2, times, err)) return rc;
  CL_TRY(T.mark(3, st));
  // ---- order, cut
  {
    k_cl_keys<<<nblk(n), 256, 0, st>>>(d_label, d_level, n, k0, p0, d_nlev);
    CL_TRY(hipGetLastError());
    std::vector<uint32_t> sh;
    field_shifts(sh, 0, bits_of(std::min(levels2, n)));   // by level
    field_shifts(sh, 32, id_bits);                        // then by component, stable
    if (dev_radix_sort(&k0, &p0, &k1, &p1, n, sh, d_sort, st, err)) return CL_HIP;
    k_cl_rank<<<nblk(n), 256, 0, st>>>(p0, d_w, n, d_rank, d_wo);
    CL_TRY(hipGetLastError());
    if (dev_scan_u32(d_wo, n, d_S, d_partial, st, err)) return CL_HIP;
    k_cl_part<<<nblk(n), 256, 0, st>>>(p0, d_S, d_wo, n, k, G.d_part, d_rows);
    CL_TRY(hipGetLastError());
  }
  CL_TRY(T.mark(4, st));
  // ---- statistics
  if (E) {
    k_cl_edge_stats<<<nblk(E), 256, 0, st>>>(G.d_a, G.d_b, E, G.d_part, k, d_rows, d_g + 1);
    k_cl_nb_keys<<<nblk(m), 256, 0, st>>>(G.d_a, G.d_b, m, G.d_part, k, k0);
    CL_TRY(hipGetLastError());
    std::vector<uint32_t> sh;
    field_shifts(sh, 0, id_bits);
    field_shifts(sh, 32, bits_of(k));                     // (k itself: the part of the arcs that do not cross)
    if (dev_radix_sort(&k0, &p0, &k1, &p1, m, sh, d_sort, st, err)) return CL_HIP;
    k_cl_nb_heads<<<nblk(m), 256, 0, st>>>(k0, m, k, d_rows);
    CL_TRY(hipGetLastError());
  }
  CL_TRY(T.mark(5, st));
  uint64_t g[2] = {0, 0};
  uint32_t n_levels = 0;
  CL_TRY(hipMemcpyAsync(R.comp.data(), d_label, 4ull * n, hipMemcpyDeviceToHost, st));
  CL_TRY(hipMemcpyAsync(R.level.data(), d_level, 4ull * n, hipMemcpyDeviceToHost, st));
  CL_TRY(hipMemcpyAsync(R.rank.data(), d_rank, 4ull * n, hipMemcpyDeviceToHost, st));
  CL_TRY(hipMemcpyAsync(R.part.data(), G.d_part, 4ull * n, hipMemcpyDeviceToHost, st));
  CL_TRY(hipMemcpyAsync(R.part_stats.data(), d_rows, 40ull * k, hipMemcpyDeviceToHost, st));
  CL_TRY(hipMemcpyAsync(g, d_g, 16, hipMemcpyDeviceToHost, st));
  CL_TRY(hipMemcpyAsync(&n_levels, d_nlev, 4, hipMemcpyDeviceToHost, st));
  CL_TRY(hipStreamSynchronize(st));
  R.stats[0] = n_comp; R.stats[1] = n_levels; R.stats[2] = g[0]; R.stats[3] = g[1];
  if (times) {
    float* const out[5] = {&times->arcs_ms, &times->comp_ms, &times->bfs_ms, &times->order_ms, &times->stats_ms};
    for (int i = 0; i < 5; i++) CL_TRY(hipEventElapsedTime(out[i], T.ev[i], T.ev[i + 1]));
    times->host_reads++;
  }
  return CL_OK;
}

int cl_mask(const ClGraph& G, uint32_t p, hipStream_t st, uint8_t* out, std::string& err) {
  if (G.n == 0) return CL_OK;
  k_cl_mask_core<<<nblk(G.n), 256, 0, st>>>(G.d_part, G.n, p, G.d_mask);
  if (G.E) k_cl_mask_nb<<<nblk(G.E), 256, 0, st>>>(G.d_a, G.d_b, G.E, G.d_part, p, G.d_mask);
  CL_TRY(hipGetLastError());
  CL_TRY(hipMemcpyAsync(out, G.d_mask, G.n, hipMemcpyDeviceToHost, st));
  CL_TRY(hipStreamSynchronize(st));
  return CL_OK;
}

}  // namespace herro
