// ku_kmerdb.h -- device helpers of the k-mer set builder (ku_kmerdb_*, bin/kmer_db; entry points and the extraction
// kernel in ku_kmerdb.hip) and of the other build tools: the minimizer bin key (db_sort's second half, set_lcas), the on-disk
// record codec (db_sort, db_merge, db_shrink), the taxid -> node lookup (set_lcas, db_merge), and the tile decoding that turns sequence
// bytes into k-mers, shared with the sketch kernel (ku_sketch.hip).  Helpers, constants and argument structs only: a kernel
// lives in the one .hip file that launches it.
#pragma once
#include "ku_device.h"

// bin key of a canonical k-mer (KrakenDB::bin_key(kmer, nt), src/krakendb.cpp:182-215): the minimum over its k - nt + 1
// m-mers of the scrambled canonical m-mer
__device__ __forceinline__ uint32_t ku_bin_key(uint64_t canon, uint32_t k, uint32_t nt, uint32_t xor_mask) {
  const uint32_t w = k - nt + 1, mask = (uint32_t)((1ull << (2 * nt)) - 1);
  uint32_t best = 0xFFFFFFFFu;
  for (uint32_t j = 0; j < w; ++j) {
    const uint32_t mm = (uint32_t)(canon >> (2 * j)) & mask;
    const uint32_t rc = ku_revcomp32(mm, nt);
    const uint32_t v = (mm < rc ? mm : rc) ^ xor_mask;
    best = v < best ? v : best;
  }
  return best;
}

// ---- the on-disk record of a database: key_len little-endian key bytes + 4 value bytes, record i at raw + i * (key_len + 4).
// At key_len 8 a record is three aligned dwords; other lengths go byte by byte.
struct __attribute__((packed, aligned(4))) KuKey8 { uint32_t lo, hi; };
struct __attribute__((packed, aligned(4))) KuRec12 { uint32_t lo, hi, val; };

__device__ __forceinline__ uint64_t ku_rec_key(const uint8_t *__restrict__ raw, uint64_t i, uint32_t key_len) {
  if (key_len == 8) {
    const KuKey8 r = *reinterpret_cast<const KuKey8 *>(raw + i * 12);
    return (uint64_t)r.hi << 32 | r.lo;
  }
  const uint8_t *p = raw + i * (key_len + 4);
  uint64_t key = 0;
  for (uint32_t b = 0; b < key_len; ++b) key |= (uint64_t)p[b] << (8 * b);
  return key;
}
__device__ __forceinline__ void ku_rec_load(const uint8_t *__restrict__ raw, uint64_t i, uint32_t key_len, uint64_t &key, uint32_t &val) {
  if (key_len == 8) {
    const KuRec12 r = *reinterpret_cast<const KuRec12 *>(raw + i * 12);
    key = (uint64_t)r.hi << 32 | r.lo;
    val = r.val;
    return;
  }
  const uint8_t *p = raw + i * (key_len + 4);
  key = 0;
  val = 0;
  for (uint32_t b = 0; b < key_len; ++b) key |= (uint64_t)p[b] << (8 * b);
  for (uint32_t b = 0; b < 4; ++b) val |= (uint32_t)p[key_len + b] << (8 * b);
}
__device__ __forceinline__ void ku_rec_store(uint8_t *raw, uint64_t i, uint32_t key_len, uint64_t key, uint32_t val) {
  if (key_len == 8) {
    *reinterpret_cast<KuRec12 *>(raw + i * 12) = KuRec12{(uint32_t)key, (uint32_t)(key >> 32), val};
    return;
  }
  uint8_t *p = raw + i * (key_len + 4);
  for (uint32_t b = 0; b < key_len; ++b) p[b] = (uint8_t)(key >> (8 * b));
  for (uint32_t b = 0; b < 4; ++b) p[key_len + b] = (uint8_t)(val >> (8 * b));
}

// taxid -> node: the lower bound of the taxid in the ascending node universe (KuNodeTable, ku_build.h), n_nodes where
// every node's taxid is below it
__device__ __forceinline__ uint32_t ku_node_of(const uint32_t *__restrict__ node_taxid, uint32_t n_nodes, uint32_t taxid) {
  uint32_t lo = 0, hi = n_nodes;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (node_taxid[mid] < taxid) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One wave scans a tile of KMD_TILE consecutive windows: its 64 lanes load 16 sequence bytes each (plus the two chunks the
// last windows reach into), pack them to 2-bit codes and ambiguity bits in LDS, and every lane then takes 16 windows, one
// per round, lane l of round j the window j * 64 + l of the tile -- so the 16 lanes that share a packed word read it as
// a broadcast and the shift inside the word is the same in every round.
#define KMD_TILE 1024
#define KMD_ROUNDS (KMD_TILE / 64)
#define KMD_CHUNKS (KMD_TILE / 16 + 2)  // 16-byte chunks a tile's windows cover (k <= 31: 30 bytes past the tile)
#define KMD_WAVES 4

// the tile's KMD_CHUNKS 16-byte chunks -> packed words of the wave's LDS rows (code: 16 bases per word, the first one in bits
// 31..30; amb: 16 ambiguity bits per word, the first base in bit 15).  The caller puts a barrier between this and kmd_window.
__device__ __forceinline__ void kmd_pack_tile(const uint8_t *__restrict__ seq, uint64_t seq_bytes, uint64_t tile, uint32_t lane,
                                              uint32_t *s_code, uint32_t *s_amb) {
  for (uint32_t c = lane; c < KMD_CHUNKS; c += 64) {
    const uint64_t off = tile * KMD_TILE + 16ull * c;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);  // (bytes past the segment: ambiguous, and no window below reaches them)
    if (off + 16 <= seq_bytes) v = *reinterpret_cast<const uint4 *>(seq + off);
    uint32_t c0, c1, c2, c3, a0, a1, a2, a3;
    ku_pack_dword(v.x, c0, a0);
    ku_pack_dword(v.y, c1, a1);
    ku_pack_dword(v.z, c2, a2);
    ku_pack_dword(v.w, c3, a3);
    s_code[c] = (c0 << 24) | (c1 << 16) | (c2 << 8) | c3;
    s_amb[c] = (a0 << 12) | (a1 << 8) | (a2 << 4) | a3;
  }
}

// window j * 64 + lane of the packed tile: its forward k-mer; true when one of its k bytes is ambiguous
__device__ __forceinline__ bool kmd_window(const uint32_t *s_code, const uint32_t *s_amb, uint32_t j, uint32_t lane, uint32_t k,
                                           uint64_t &fwd) {
  const uint32_t word = j * 4 + (lane >> 4), sh = lane & 15;
  const uint32_t w0 = s_code[word], w1 = s_code[word + 1], w2 = s_code[word + 2];
  // 32 bases from the window's first one on: two funnel shifts over the three words it can touch
  const uint32_t hi = __funnelshift_l(w1, w0, 2 * sh), lo = __funnelshift_l(w2, w1, 2 * sh);
  fwd = (((uint64_t)hi << 32) | lo) >> (64 - 2 * k);
  const uint64_t amb48 = ((uint64_t)s_amb[word] << 48) | ((uint64_t)s_amb[word + 1] << 32) | ((uint64_t)s_amb[word + 2] << 16);
  return ((amb48 << sh) >> (64 - k)) != 0;
}

struct KmdScan {
  const uint8_t *seq;          // the uploaded segment, 16-byte aligned
  uint64_t seq_bytes;          // bytes that may be loaded (a multiple of 16); the windows below lie inside it
  uint64_t w_lo, w_hi;         // windows [w_lo, w_hi) of the segment: window w = bytes [w, w + k)
  uint32_t k, nt, xor_mask;
  uint32_t bin_lo, bin_hi;     // pass mode: keep the k-mers whose bin key lies in [bin_lo, bin_hi)
  uint32_t pass_mode;          // 0: one pass, the bin key is not computed
  uint64_t *out;               // the collection buffer
  uint64_t cap;                // its size in k-mers; the host never launches more windows than it has room for
  unsigned long long *cursor;  // k-mers in the buffer
  uint32_t *err;               // set when a tile would have written past cap (a host-side accounting bug): nothing is written
};
