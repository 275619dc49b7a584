// ku_sketch.h -- device helpers of the k-mer sketches (ku_sketch_*, bin/count_unique, kmer_db -P auto; entry points and
// kernels in ku_sketch.hip): sequence bytes -> k-mers -> HyperLogLog registers of precision p = 4..18, one sketch per range of the
// minimizer bin keys.  The reference's count_unique (src/count_unique.cpp:52-82) inserts every unambiguous FORWARD k-mer of
// its input into dense counters and prints ertlCardinality of their merge; the registers of that merge depend only on the
// set of k-mers, so one pass over the bytes with max-updates of a register array gives the same registers.
#pragma once
#include "ku_device.h"
#include "ku_kmerdb.h"

#define KU_SKETCH_BLOCK 256  // threads of kmersketch_values_kernel

struct KuSketchScan {
  const uint8_t *seq;    // the uploaded segment, 16-byte aligned
  uint64_t seq_bytes;    // bytes that may be loaded (a multiple of 16); the windows below lie inside it
  uint64_t w_lo, w_hi;   // windows [w_lo, w_hi) of the segment: window w = bytes [w, w + k)
  uint32_t k, p;
  uint32_t canonical;    // 0: the forward k-mer is hashed (count_unique), 1: the canonical one
  uint32_t nt, xor_mask; // bin key of the groups (n_groups > 1)
  uint32_t n_groups;     // 1, or a power of two: group = bin key * n_groups >> 2 nt, the pass ranges of ku_kmerdb_open
  uint8_t *registers;    // [n_groups << p], 4-byte aligned (ku_hll_raise works on the enclosing dword)
  unsigned long long *n_observed;  // kept windows, duplicates included
};

// the register of hash h in sketch `group` of precision p, and the rank h has there: ku_hll_locate (ku_device.h) with p a
// run-time value.  idx = the top p bits; rank = clz of the bits behind them + 1, 64 - p + 1 when all are zero (bit p - 1,
// set below the hash's bits, stops the count there).
__device__ __forceinline__ uint8_t *ku_sketch_locate(uint8_t *registers, uint32_t group, uint64_t h, uint32_t p, uint32_t &rank) {
  const uint32_t idx = (uint32_t)(h >> (64 - p));
  const uint64_t rest = (h << p) | (1ull << (p - 1));
  rank = (uint32_t)__builtin_clzll(rest) + 1;
  return registers + ((size_t)group << p) + idx;
}
