// ku_dbshrink_budget.h -- the budget rule and the chunk plan of ku_db_shrink_files (include/krakenuniq_amd.h), written once
// for the library (ku_dbshrink.hip) and the check program (dbshrink_check.cpp), and restated by the binding
// (capi.db_shrink_capacity).  Plain C++, no HIP.
//
// One eighth of device_bytes is the offset slice's: 8 bytes per offset, mapped in place.  The rest is the records': 24 bytes
// per record of an input chunk -- 12 in the chunk's buffer and 12 in the buffer of the records selected from it (a chunk of c
// records selects at most c; 12 is the longest record, key_len 8, and shorter records use the same counts).
//
// The input is cut into chunks of chunk_records consecutive records from record 0 on, whatever the blocks of the rule are:
// chunk c is [c * chunk_records, min((c + 1) * chunk_records, key_ct)).
#pragma once
#include <stdint.h>

struct KuDbShrinkBudget {
  uint64_t chunk_records;  // records of an input chunk
  uint64_t offset_slice;   // offsets of an index slice
};

inline KuDbShrinkBudget ku_dbshrink_budget(uint64_t device_bytes) {
  KuDbShrinkBudget b;
  const uint64_t offset_bytes = device_bytes / 8;
  b.offset_slice = offset_bytes / 8;
  b.chunk_records = (device_bytes - offset_bytes) / 24;
  return b;
}

inline uint64_t ku_dbshrink_chunks(uint64_t key_ct, uint64_t chunk_records) {
  return key_ct / chunk_records + (key_ct % chunk_records != 0);
}

// chunk c < ku_dbshrink_chunks(key_ct, chunk_records)
inline void ku_dbshrink_chunk(uint64_t key_ct, uint64_t chunk_records, uint64_t c, uint64_t &lo, uint64_t &hi) {
  lo = c * chunk_records;
  hi = key_ct - lo > chunk_records ? lo + chunk_records : key_ct;
}
