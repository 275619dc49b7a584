// ku_sketch.h -- device code of the k-mer sketches (ku_sketch_*, bin/count_unique, kmer_db -P auto; entry points in
// ku_dbsort.hip): sequence bytes -> k-mers -> HyperLogLog registers of precision p = 4..18, one sketch per range of the
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

// One wave per tile of KMD_TILE windows, decoded as kmerdb_extract_kernel decodes them (kmd_pack_tile / kmd_window).  Every
// lane locates the registers of its 16 windows, requests all their bytes, and only then looks at them: the plain load is the
// pre-check of ku_hll_raise, and once the sketch has warmed up nearly every insert ends there.
__global__ __launch_bounds__(64 * KMD_WAVES) void kmersketch_kernel(KuSketchScan a) {
  __shared__ uint32_t s_code[KMD_WAVES][KMD_CHUNKS];
  __shared__ uint32_t s_amb[KMD_WAVES][KMD_CHUNKS];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t t0 = a.w_lo / KMD_TILE, t1 = (a.w_hi + KMD_TILE - 1) / KMD_TILE;
  const uint64_t per_iter = (uint64_t)gridDim.x * KMD_WAVES;
  const uint64_t n_iter = (t1 - t0 + per_iter - 1) / per_iter;  // the same in every block: the barriers below are uniform
  const uint32_t k = a.k, p = a.p;
  for (uint64_t it = 0; it < n_iter; ++it) {
    const uint64_t tile = t0 + (it * gridDim.x + blockIdx.x) * KMD_WAVES + wv;
    const bool live = tile < t1;  // wave-uniform
    if (live) kmd_pack_tile(a.seq, a.seq_bytes, tile, lane, s_code[wv], s_amb[wv]);
    __syncthreads();
    if (live) {
      uint8_t *reg[KMD_ROUNDS];
      uint32_t rank[KMD_ROUNDS], seen[KMD_ROUNDS];
      uint32_t total = 0;
#pragma unroll
      for (uint32_t j = 0; j < KMD_ROUNDS; ++j) {
        uint64_t fwd;
        const bool ambiguous = kmd_window(s_code[wv], s_amb[wv], j, lane, k, fwd);
        const uint64_t w = tile * KMD_TILE + j * 64 + lane;
        const bool keep = !ambiguous && w >= a.w_lo && w < a.w_hi;
        const uint64_t rc = ku_revcomp64(fwd, k);
        const uint64_t canon = fwd < rc ? fwd : rc;
        uint32_t group = 0;
        if (a.n_groups > 1 && keep)
          group = (uint32_t)(((uint64_t)ku_bin_key(canon, k, a.nt, a.xor_mask) * a.n_groups) >> (2 * a.nt));
        reg[j] = ku_sketch_locate(a.registers, group, ku_fmix64(a.canonical ? canon : fwd), p, rank[j]);
        if (!keep) {  // (the register of a dropped window is a valid address all the same: it is loaded, never raised)
          reg[j] = a.registers;
          rank[j] = 0;
        }
        total += (uint32_t)__popcll(__ballot(keep));
      }
#pragma unroll
      for (uint32_t j = 0; j < KMD_ROUNDS; ++j) seen[j] = *reg[j];
#pragma unroll
      for (uint32_t j = 0; j < KMD_ROUNDS; ++j) ku_hll_raise(reg[j], seen[j], rank[j]);
      if (lane == 0 && total) atomicAdd(a.n_observed, (unsigned long long)total);  // one per tile
    }
    __syncthreads();  // the next tile overwrites the packed words
  }
}

// values hashed as they are (ku_sketch_add_values): sketch 0 only
__global__ __launch_bounds__(KU_SKETCH_BLOCK) void kmersketch_values_kernel(const uint64_t *__restrict__ values, uint64_t n, uint32_t p,
                                                                            uint8_t *registers) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t rank;
    uint8_t *r = ku_sketch_locate(registers, 0, ku_fmix64(values[i]), p, rank);
    ku_hll_raise(r, *r, rank);
  }
}
