// scan_sort_dev.hip — the shared exclusive scan of u32 and the stable LSD radix sort (scan_sort_dev.h; tests/scan_sort_cases.py):
//   scan         k_scan_partial: the total of every tile of 2048 elements; k_scan_top: one workgroup walks the totals 256 at a time, carrying the
//                sum from round to round; k_scan_final: every tile again, from its total's prefix on.
//   radix sort   LSD, 8-bit digits, 64-bit key + 64-bit payload, stable (per-block histogram, scan, ranked scatter).
// No atomic decides a place: the histogram's sums are the only atomics.
#include "scan_sort_dev.h"

namespace herro {
namespace {

// ---- exclusive scan of u32 (out has n + 1 entries: out[n] = total) ---------------------------------------------------------
__global__ __launch_bounds__(256) void k_scan_partial(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ partial) {
  __shared__ uint32_t lds4[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * SC_TILE + threadIdx.x * SC_ITEMS;
  uint32_t s = 0;
#pragma unroll
  for (int e = 0; e < SC_ITEMS; e++) if (i0 + e < n) s += in[i0 + e];
  uint32_t total;
  (void)block_excl_scan(s, lds4, total);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_scan_top(uint32_t* __restrict__ partial, uint32_t nb) {
  __shared__ uint32_t lds4[4];
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < nb; b0 += 256) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < nb ? partial[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_excl_scan(v, lds4, total);
    if (i < nb) partial[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) partial[nb] = carry;
}

__global__ __launch_bounds__(256) void k_scan_final(const uint32_t* __restrict__ in, uint32_t n, const uint32_t* __restrict__ partial,
                                                    uint32_t nb, uint32_t* __restrict__ out) {
  __shared__ uint32_t lds4[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * SC_TILE + threadIdx.x * SC_ITEMS;
  uint32_t v[SC_ITEMS], s = 0;
#pragma unroll
  for (int e = 0; e < SC_ITEMS; e++) { v[e] = i0 + e < n ? in[i0 + e] : 0u; s += v[e]; }
  uint32_t total;
  uint32_t at = block_excl_scan(s, lds4, total) + partial[blockIdx.x];
#pragma unroll
  for (int e = 0; e < SC_ITEMS; e++) { if (i0 + e < n) out[i0 + e] = at; at += v[e]; }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = partial[nb];
}

// ---- radix sort: one 8-bit digit per pass ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rs_hist(const uint64_t* __restrict__ keys, uint32_t n, uint32_t shift, uint32_t nb,
                                                 uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * SC_TILE;
#pragma unroll
  for (int e = 0; e < SC_ITEMS; e++) {
    const uint64_t i = i0 + e * 256 + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(uint64_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];   // digit-major: the scan gives every (digit, block) its place
}

__global__ __launch_bounds__(256) void k_rs_scatter(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ pays, uint32_t n,
                                                    uint32_t shift, uint32_t nb, const uint32_t* __restrict__ offs,
                                                    uint64_t* __restrict__ keys_out, uint64_t* __restrict__ pays_out) {
  __shared__ uint32_t running[256];
  __shared__ uint32_t wcnt[4][256];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  running[tid] = offs[(uint64_t)tid * nb + blockIdx.x];
#pragma unroll
  for (int v = 0; v < 4; v++) wcnt[v][tid] = 0;
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * SC_TILE;
  for (int e = 0; e < SC_ITEMS; e++) {          // elements in index order: round e holds i0 + 256 e .. + 255
    const uint64_t i = i0 + e * 256 + tid;
    const bool valid = i < n;
    uint64_t key = 0, pay = 0;
    if (valid) { key = keys[i]; pay = pays[i]; }
    const uint32_t d = (uint32_t)(key >> shift) & 255u;
    uint64_t peers = __ballot(valid);          // lanes of this wave with my digit
#pragma unroll
    for (int bit = 0; bit < 8; bit++) {
      const bool one = (d >> bit) & 1u;
      const uint64_t bm = __ballot(valid && one);
      peers &= one ? bm : ~bm;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
    if (valid && rank == 0) wcnt[wave][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint32_t at = running[d] + rank;
      for (uint32_t v = 0; v < wave; v++) at += wcnt[v][d];
      keys_out[at] = key;
      pays_out[at] = pay;
    }
    __syncthreads();
    running[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
#pragma unroll
    for (int v = 0; v < 4; v++) wcnt[v][tid] = 0;
    __syncthreads();
  }
}

// (the text is the finder's: the callers' messages have always begun with it)
#define SS_TRY(expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) { err = std::string("overlap finder: " #expr ": ") + hipGetErrorString(_e); return 1; } } while (0)

}  // namespace

uint32_t dev_scan_partials(uint32_t n) { return nblk(n, SC_TILE) + 1; }

int dev_scan_u32(const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* partial, hipStream_t st, std::string& err) {
  if (n == 0) { SS_TRY(hipMemsetAsync(out, 0, 4, st)); return 0; }
  const uint32_t nb = nblk(n, SC_TILE);
  k_scan_partial<<<nb, 256, 0, st>>>(in, n, partial);
  k_scan_top<<<1, 256, 0, st>>>(partial, nb);
  k_scan_final<<<nb, 256, 0, st>>>(in, n, partial, nb, out);
  SS_TRY(hipGetLastError());
  return 0;
}

int dev_radix_sort(uint64_t** k0, uint64_t** p0, uint64_t** k1, uint64_t** p1, uint32_t n, const std::vector<uint32_t>& shifts, const SortScratch& S,
                   hipStream_t st, std::string& err) {
  if (n < 2) return 0;
  const uint32_t nb = nblk(n, SC_TILE);
  for (uint32_t sh : shifts) {
    k_rs_hist<<<nb, 256, 0, st>>>(*k0, n, sh, nb, S.hist);
    if (int rc = dev_scan_u32(S.hist, 256 * nb, S.offs, S.partial, st, err)) return rc;
    k_rs_scatter<<<nb, 256, 0, st>>>(*k0, *p0, n, sh, nb, S.offs, *k1, *p1);
    SS_TRY(hipGetLastError());
    std::swap(*k0, *k1);
    std::swap(*p0, *p1);
  }
  return 0;
}

}  // namespace herro
