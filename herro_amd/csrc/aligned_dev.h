// aligned_dev.h — what herro_job_create_aligned (job_create.hip) takes from the front end (frontend_api.hip): the handle over
// device-resident ops, a copy of a span of its store, and the ops' CIGAR text.
#pragma once
#include "api_ctx.h"

// Aligned records with their ops left on the device (herro_align_overlaps_dev, herro_aligned_dev_mirror), or a caller's own binary CIGARs (herro_aligned_dev_from_ops).
struct herro_aligned_dev {
  herro_ctx* ctx = nullptr;
  int device = 0;
  bool host_only = false;              // a handle of herro_debug_host_ctx (from_ops only): the store is h_ops
  std::vector<herro_alignment> alns;   // trimmed coordinates; cigar = NULL, cigar_len = 0
  std::vector<int32_t> scores;
  std::vector<uint32_t> n_ops;         // 0: failed
  std::vector<uint64_t> op_off;        // first op of every record in the store
  uint32_t failed = 0;
  uint32_t* d_ops = nullptr;           // the op store: every record's ops, `len << 2 | type`
  uint64_t used = 0, cap = 0;          // ... in ops
  std::vector<uint32_t> h_ops;
};

// ops [lo, hi) of the handle's store on the host
int aligned_dev_fetch(const herro_aligned_dev* a, uint64_t lo, uint64_t hi, std::vector<uint32_t>& v);

// The CIGAR text of records [r0, r1), "<len><M|I|D>" per op, records back to back in `text` with a terminating byte behind them: record r has
// n_ops[r] ops at ops + at[r], and alns[r].cigar / cigar_len are set to its text.  64 records per task of the context's host pool.
void ops_text_block(herro_ctx* ctx, const uint32_t* ops, const uint64_t* at, const uint32_t* n_ops, uint64_t r0, uint64_t r1, herro_alignment* alns,
                    std::string& text);
