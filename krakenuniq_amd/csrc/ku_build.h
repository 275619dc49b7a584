// ku_build.h -- host plumbing shared by the database build tools' translation units (ku_dbsort.hip, ku_kmerdb.hip, ku_dbmerge.hip,
// ku_sketch.hip, ku_setlcas.hip): the device check, the KRAKIX2 scramble mask, the HIP check, launch geometry, rocPRIM's
// two-call protocol, and what the builder borrows from db_sort.  `fail` and KU_TRY are those of ku_ctx.h.  Not part of the
// public ABI.
#pragma once
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ku_ctx.h"
#include "ku_kmerdb.h"
#include "ku_kmerdb_budget.h"

// ---- device: the index names one of the HIP devices present (selecting it stays with the caller, whose HIP check reports a
// failure under its own name)
inline int ku_check_device(int device) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(KU_EHIP, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= n_dev) return fail(KU_EINVAL, "device index out of range");
  return KU_OK;
}

// ---- the scramble of a KRAKIX2 index's bin keys: INDEX2_XOR_MASK (krakendb.cpp:45), cut to the 2 nt bits of a bin key
inline uint32_t ku_index2_xor_mask(uint32_t nt) {
  return (uint32_t)(0xe37e28c4271b5a2dULL & ((1ull << (2 * nt)) - 1));
}

// ---- HIP check: KU_HIP(who, expr) returns from the calling function when expr fails, with the error text
// "<prefix><expr>: <HIP's message>[<oom_hint>, on out of memory]" set and, where `who` names a handle, that handle marked
// as failed.  `who` is looked at on failure only.
struct KuHipWho {
  const char *prefix;    // "db_sort: "
  const char *oom_hint;  // what the user can do about hipErrorOutOfMemory, or ""
  bool *failed;          // the handle's flag, or null
};
inline int ku_hip_fail(const KuHipWho &who, const char *expr, hipError_t e) {
  const bool oom = e == hipErrorOutOfMemory;
  if (who.failed) *who.failed = true;
  return fail(oom ? KU_ENOMEM : KU_EHIP, std::string(who.prefix) + expr + ": " + hipGetErrorString(e) + (oom ? who.oom_hint : ""));
}
#define KU_HIP(who, expr)                                              \
  do {                                                                 \
    hipError_t e_ = (expr);                                            \
    if (e_ != hipSuccess) return ku_hip_fail((who), #expr, e_);        \
  } while (0)

// ---- launch geometry: blocks of 256 threads over n items (grid-stride kernels), and blocks of KMD_WAVES waves over the
// tiles of a segment (ku_kmerdb.h)
inline unsigned ku_grid_256(uint64_t n) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 1u << 16); }
inline unsigned ku_tile_grid(uint64_t tiles) { return (unsigned)std::min<uint64_t>((tiles + KMD_WAVES - 1) / KMD_WAVES, 2048); }

// ---- rocPRIM's two-call protocol: call(nullptr, bytes) asks for the size of the scratch, reserve(bytes, tmp, have) provides
// a buffer of at least that size (and says how large it is), call(tmp, have) does the work.  Nothing here waits for the
// stream: whether the reservation does is the caller's business.  `what` names the call in the error text.
template <typename Reserve, typename Call>
int ku_rocprim(const KuHipWho &who, const char *what, Reserve reserve, Call call) {
  size_t bytes = 0;
  hipError_t e = call((void *)nullptr, bytes);
  if (e != hipSuccess) return ku_hip_fail(who, what, e);
  void *tmp = nullptr;
  KU_TRY(reserve(bytes, tmp, bytes));
  e = call(tmp, bytes);
  if (e != hipSuccess) return ku_hip_fail(who, what, e);
  return KU_OK;
}

// ---- device allocations of one call: frees what it owns on every exit path
struct Dev {
  std::vector<void *> ptrs;
  template <typename T> hipError_t alloc(T **p, size_t bytes) {
    hipError_t e = hipMalloc((void **)p, bytes ? bytes : 1);
    if (e == hipSuccess) ptrs.push_back(*p);
    return e;
  }
  void release(void *p) {
    for (auto &q : ptrs)
      if (q == p) { (void)hipFree(p); q = nullptr; }
  }
  ~Dev() {
    for (void *p : ptrs)
      if (p) (void)hipFree(p);
  }
};

inline bool write_all(int fd, const void *buf, size_t n) {
  const char *p = (const char *)buf;
  while (n) {
    ssize_t w = ::write(fd, p, n < ((size_t)1 << 30) ? n : ((size_t)1 << 30));
    if (w <= 0) return false;
    p += w;
    n -= (size_t)w;
  }
  return true;
}

// ---- the second half of db_sort (ku_dbsort.hip), shared with ku_kmerdb_end_pass.  In: n records sorted by k-mer (their
// values in d_val, or all 0 when it is null).  Computes the bin keys and their histogram over the bins [bin_lo, bin_lo +
// n_hist) -- every record's bin key must lie there --, sorts stably by bin key, which leaves the records in (bin key, k-mer)
// order, and packs them in their on-disk form.  Out (all enqueued on s, not yet waited for): *d_raw (allocated here when
// null) holds the n records, (*d_off)[b] = first_off + the number of records in the bins [bin_lo, bin_lo + b), b = 0 ..
// n_hist.  release_inputs: d_kmer and d_val belong to `dev` and are freed once they have been read.
int dbsort_bin_order_and_pack(Dev &dev, hipStream_t s, uint64_t *d_kmer, uint32_t *d_val, bool release_inputs, uint64_t n,
                              uint32_t k, uint32_t nt, uint32_t key_len, uint32_t bin_lo, uint64_t n_hist, uint64_t first_off,
                              uint8_t **d_raw, uint64_t **d_off);
