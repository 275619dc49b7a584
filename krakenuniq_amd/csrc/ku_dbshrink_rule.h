// ku_dbshrink_rule.h -- the selection rule of db_shrink (src/db_shrink.cpp:83-113) as arithmetic, shared by the two kernels of
// ku_dbshrink.hip, their host code and csrc/dbshrink_check.cpp.  Plain C++ that also compiles without HIP; every quantity is 64
// bits wide.
//
// The key_ct records of the input are cut into n_out consecutive blocks: the first odd = key_ct % n_out of them hold
// bs + 1 = key_ct / n_out + 1 records, the others bs.  Of every block the record `offset` places before its end is kept
// (1 <= offset <= bs: compared with bs also where the block holds bs + 1).  So
//   src(j)  the input record that output record j is                  = (j + 1) * bs + min(j + 1, odd) - offset
//   S(x)    the output records that come from input records below x   = #{ j : src(j) < x }
// With m = j + 1 and t = x + offset - 1:  src(j) < x  <=>  m * bs + min(m, odd) <= t, which the m <= odd satisfy up to
// t / (bs + 1) and the m > odd up to (t - odd) / bs.  S is what maps an index of the input (offsets[b] = records in the bins
// below b) to the index of the output, and what tells a chunk [lo, hi) of the input which output records it holds:
// those in [S(lo), S(hi)).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KU_SHRINK_HD __host__ __device__ inline
#else
#define KU_SHRINK_HD inline
#endif

struct KuShrinkRule {
  uint64_t key_ct, n_out, offset;
  uint64_t bs, odd;  // block size, blocks with one record more
};

// 1 <= n_out <= key_ct < 2^62, 1 <= offset <= bs (the bound on key_ct keeps x + offset - 1 inside 64 bits; a file of that
// many records does not exist)
KU_SHRINK_HD bool ku_shrink_rule_ok(uint64_t key_ct, uint64_t n_out, uint64_t offset) {
  return n_out >= 1 && n_out <= key_ct && key_ct < (1ull << 62) && offset >= 1 && offset <= key_ct / n_out;
}

KU_SHRINK_HD KuShrinkRule ku_shrink_rule(uint64_t key_ct, uint64_t n_out, uint64_t offset) {
  KuShrinkRule r;
  r.key_ct = key_ct;
  r.n_out = n_out;
  r.offset = offset;
  r.bs = key_ct / n_out;
  r.odd = key_ct % n_out;
  return r;
}

// j < n_out
KU_SHRINK_HD uint64_t ku_shrink_src(const KuShrinkRule &r, uint64_t j) {
  const uint64_t m = j + 1;
  return m * r.bs + (m < r.odd ? m : r.odd) - r.offset;
}

// x <= key_ct; S(0) = 0, S(key_ct) = n_out
KU_SHRINK_HD uint64_t ku_shrink_S(const KuShrinkRule &r, uint64_t x) {
  const uint64_t t = x + r.offset - 1;
  const uint64_t in_odd = t / (r.bs + 1);
  uint64_t s = in_odd < r.odd ? in_odd : r.odd;
  if (t >= r.odd) {
    const uint64_t q = (t - r.odd) / r.bs, rest = r.n_out - r.odd;
    if (q > r.odd) s += q - r.odd < rest ? q - r.odd : rest;
  }
  return s;
}
