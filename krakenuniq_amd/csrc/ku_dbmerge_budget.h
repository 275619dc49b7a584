// ku_dbmerge_budget.h -- the budget rule of ku_db_merge_files (include/krakenuniq_amd.h), written once for the library
// (ku_dbmerge.hip) and restated by the binding (capi.db_merge_capacity).  Plain C++, no HIP.
//
// One eighth of device_bytes is the bins': three offset slices (the fold's left side, the input being merged, the result) of
// 8 bytes per bin, each with one closing entry.  The rest is the records': 56 bytes per record of the chunk, all inputs
// counted together -- 12 in the left side's buffer, 12 in the buffer of the input being merged, 12 in the result's, 8 of rank,
// 8 of scanned duplicate count, 1 of duplicate flag, 3 of slack for the scan's scratch.
#pragma once
#include <stdint.h>

struct KuDbMergeBudget {
  uint64_t capacity;  // records of all inputs together that a chunk may hold
  uint64_t max_bins;  // bins a chunk may span
};

inline KuDbMergeBudget ku_dbmerge_budget(uint64_t device_bytes) {
  KuDbMergeBudget b;
  const uint64_t bin_bytes = device_bytes / 8;
  b.max_bins = bin_bytes / 24 - 1;
  b.capacity = (device_bytes - bin_bytes) / 56;
  return b;
}
