// ku_kmerdb_budget.h -- the budget rule of ku_kmerdb_open (include/krakenuniq_amd.h), written once for the library
// (ku_kmerdb.hip) and for bin/kmer_db, whose -P auto plans its passes against the same buffer.  Plain C++, no HIP.
#pragma once
#include <stdint.h>
#include <algorithm>

constexpr uint64_t KMD_MAX_SEGMENT = (uint64_t)64 << 20;

struct KuKmerdbBudget {
  uint64_t segment;   // bytes of the sequence segment: min(64 MiB, device_bytes / 64), rounded down to 1 KiB
  uint64_t capacity;  // k-mers in each of the two buffers (the second is the sort's and the merge's other side)
  uint64_t usable;    // of them, what the distinct set of a pass may fill: 1/64 of the buffer has to stay free
};

inline KuKmerdbBudget ku_kmerdb_budget(uint64_t device_bytes) {
  KuKmerdbBudget b;
  b.segment = std::min<uint64_t>(KMD_MAX_SEGMENT, device_bytes / 64) & ~(uint64_t)1023;
  b.capacity = (device_bytes - b.segment) / 16;
  b.usable = b.capacity - b.capacity / 64;
  return b;
}
