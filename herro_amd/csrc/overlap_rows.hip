// overlap_rows.hip — behind the finder, on its records alone (overlap_dev.h; DESIGN.md §10, "Pairs on the device"): the row table of
// herro_find_overlaps' 2 P rows (ovl_row_table) and the records of an index in parts put into target order (ovl_sort_recs).  Both are a key per
// record, the shared stable radix sort and scan (scan_sort_dev.h) and a gather; nothing here reads the read store.
#include "overlap_dev.h"
#include "scan_sort_dev.h"

namespace herro {
namespace {

// row keys: primary p is the row (target t, query q), its mirror np + p the row (target q, query t)
__global__ __launch_bounds__(256) void k_row_keys(const OvlRec* __restrict__ rec, uint32_t np, uint64_t* __restrict__ keys,
                                                  uint64_t* __restrict__ pays) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= np) return;
  const uint64_t t = rec[p].tid, q = rec[p].qid;
  keys[p] = t << 32 | q;
  pays[p] = p;
  keys[np + p] = q << 32 | t;
  pays[np + p] = np + p;
}

// ... with a core mask: the row (t, q) only if t is core, the row (q, t) only if q is — rows_of[p] rows, written densely from row_at[p] on
__global__ __launch_bounds__(256) void k_row_count(const OvlRec* __restrict__ rec, uint32_t np, const uint8_t* __restrict__ core,
                                                   uint32_t* __restrict__ rows_of) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < np) rows_of[p] = (core[rec[p].tid] ? 1u : 0u) + (core[rec[p].qid] ? 1u : 0u);
}

__global__ __launch_bounds__(256) void k_row_keys_core(const OvlRec* __restrict__ rec, uint32_t np, const uint8_t* __restrict__ core,
                                                       const uint32_t* __restrict__ row_at, uint64_t* __restrict__ keys,
                                                       uint64_t* __restrict__ pays) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= np) return;
  const uint64_t t = rec[p].tid, q = rec[p].qid;
  uint32_t at = row_at[p];
  if (core[t]) { keys[at] = t << 32 | q; pays[at] = p; at++; }
  if (core[q]) { keys[at] = q << 32 | t; pays[at] = np + p; }
}

__global__ __launch_bounds__(256) void k_row_heads(const uint64_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) flag[i] = (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_row_write(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ pays,
                                                   const uint32_t* __restrict__ flag, const uint32_t* __restrict__ tidx, uint32_t n,
                                                   uint32_t* __restrict__ rids, uint64_t* __restrict__ aln_off, uint32_t* __restrict__ rec_of_row) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  rec_of_row[i] = (uint32_t)pays[i];
  if (flag[i]) { rids[tidx[i]] = (uint32_t)(keys[i] >> 32); aln_off[tidx[i]] = i; }
  if (i == 0) aln_off[tidx[n]] = n;
}

// the records of all block pairs into target order: the key of the stable sort, and the gather behind it
__global__ __launch_bounds__(256) void k_rec_keys(const OvlRec* __restrict__ rec, uint32_t n, uint64_t* __restrict__ keys, uint64_t* __restrict__ pays) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  keys[i] = rec[i].tid;
  pays[i] = i;
}

__global__ __launch_bounds__(256) void k_rec_gather(const OvlRec* __restrict__ rec, const uint64_t* __restrict__ pays, uint32_t n, OvlRec* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = rec[pays[i]];
}

}  // namespace

// A target's records come pair by pair — (i, i), (i, i + 1), ... —, in ascending q inside a pair and from pair to pair: one stable sort by t puts
// the call's records into ascending (t, q).  Nothing is queued on st that still writes R (the caller has synchronised).
int ovl_sort_recs(OvlRecs& R, uint32_t n_reads, hipStream_t st, std::string& err) {
  if (R.n < 2) return OVL_OK;
  const uint32_t n = (uint32_t)R.n;              // (<= 2^31 - 1: OVL_MAX_PAIRS)
  Bufs B;
  uint64_t *k0, *p0, *k1, *p1;
  uint32_t* scratch;
  OvlRec* sorted = nullptr;
  OVL_TRY(B.get(&k0, n)); OVL_TRY(B.get(&p0, n)); OVL_TRY(B.get(&k1, n)); OVL_TRY(B.get(&p1, n));
  OVL_TRY(B.get(&scratch, dev_sort_scratch(n)));
  OVL_TRY(hipMalloc((void**)&sorted, (uint64_t)n * sizeof(OvlRec)));
  k_rec_keys<<<nblk(n), 256, 0, st>>>(R.d, n, k0, p0);
  std::vector<uint32_t> shifts;
  field_shifts(shifts, 0, bits_of(n_reads - 1));
  int rc = dev_radix_sort(&k0, &p0, &k1, &p1, n, shifts, scratch, st, err);
  hipError_t e = hipSuccess;
  if (rc == OVL_OK) {
    k_rec_gather<<<nblk(n), 256, 0, st>>>(R.d, p0, n, sorted);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (rc != OVL_OK || e != hipSuccess) {
    (void)hipFree(sorted);
    if (rc != OVL_OK) return rc;
    OVL_TRY(e);
  }
  (void)hipFree(R.d);
  R.d = sorted;
  R.cap = n;
  return OVL_OK;
}

int ovl_row_table(const OvlRecs& R, uint32_t n_reads, const uint8_t* d_core, hipStream_t st, std::vector<uint32_t>& rids, std::vector<uint64_t>& aln_off,
                  std::vector<uint32_t>& rec_of_row, std::string& err) {
  rids.clear();
  aln_off.assign(1, 0);
  rec_of_row.clear();
  if (!R.n) return OVL_OK;
  if (R.n > OVL_MAX_PAIRS) { err = "overlap finder: more than 2^31 - 1 overlapping read pairs"; return OVL_UNSUPPORTED; }
  const uint32_t np = (uint32_t)R.n;
  uint32_t n = 2 * np;                            // rows; fewer with a core mask (counted below), the arrays are sized for 2 P
  Bufs B;
  SortScratch ss;
  OVL_TRY(ss.alloc(B, n));
  // one block for the nine arrays of 2 P (+ 1) elements: 8-byte elements first, every array on a 256-byte boundary
  const uint64_t a8 = (8ull * (n + 1ull) + 255) & ~255ull, a4 = (4ull * (n + 1ull) + 255) & ~255ull;
  uint8_t* blk = nullptr;
  OVL_TRY(B.bytes(&blk, 5 * a8 + 4 * a4));
  uint64_t *k0 = (uint64_t*)blk, *p0 = (uint64_t*)(blk + a8), *k1 = (uint64_t*)(blk + 2 * a8), *p1 = (uint64_t*)(blk + 3 * a8);
  uint64_t* d_off = (uint64_t*)(blk + 4 * a8);
  uint32_t *flag = (uint32_t*)(blk + 5 * a8), *tidx = (uint32_t*)(blk + 5 * a8 + a4), *d_rids = (uint32_t*)(blk + 5 * a8 + 2 * a4);
  uint32_t* d_rec = (uint32_t*)(blk + 5 * a8 + 3 * a4);
  if (d_core) {                                   // (flag / tidx hold the rows per primary and their scan until the keys are written)
    k_row_count<<<nblk(np), 256, 0, st>>>(R.d, np, d_core, flag);
    if (int rc = dev_scan_u32(flag, np, tidx, ss.partial, st, err)) return rc;
    k_row_keys_core<<<nblk(np), 256, 0, st>>>(R.d, np, d_core, tidx, k0, p0);
    OVL_TRY(hipGetLastError());
    OVL_TRY(hipMemcpyAsync(&n, tidx + np, 4, hipMemcpyDeviceToHost, st));
    OVL_TRY(hipStreamSynchronize(st));
    if (!n) return OVL_OK;
  } else {
    k_row_keys<<<nblk(np), 256, 0, st>>>(R.d, np, k0, p0);
    OVL_TRY(hipGetLastError());
  }
  {
    std::vector<uint32_t> shifts;                 // keys are unique: one overlap per pair
    field_shifts(shifts, 0, bits_of(n_reads - 1));
    field_shifts(shifts, 32, bits_of(n_reads - 1));
    if (int rc = dev_radix_sort(&k0, &p0, &k1, &p1, n, shifts, ss, st, err)) return rc;
  }
  k_row_heads<<<nblk(n), 256, 0, st>>>(k0, n, flag);
  if (int rc = dev_scan_u32(flag, n, tidx, ss.partial, st, err)) return rc;
  k_row_write<<<nblk(n), 256, 0, st>>>(k0, p0, flag, tidx, n, d_rids, d_off, d_rec);
  OVL_TRY(hipGetLastError());
  uint32_t nt = 0;
  OVL_TRY(hipMemcpyAsync(&nt, tidx + n, 4, hipMemcpyDeviceToHost, st));
  OVL_TRY(hipStreamSynchronize(st));
  rids.resize(nt);
  aln_off.resize((size_t)nt + 1);
  rec_of_row.resize(n);
  OVL_TRY(hipMemcpyAsync(rids.data(), d_rids, 4ull * nt, hipMemcpyDeviceToHost, st));
  OVL_TRY(hipMemcpyAsync(aln_off.data(), d_off, 8ull * (nt + 1ull), hipMemcpyDeviceToHost, st));
  OVL_TRY(hipMemcpyAsync(rec_of_row.data(), d_rec, 4ull * n, hipMemcpyDeviceToHost, st));
  OVL_TRY(hipStreamSynchronize(st));
  return OVL_OK;
}

}  // namespace herro
