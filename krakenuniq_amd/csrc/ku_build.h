// ku_build.h -- host plumbing shared by the database build tools' translation units (ku_dbsort.hip, ku_kmerdb.hip, ku_dbmerge.hip,
// ku_dbshrink.hip, ku_sketch.hip, ku_setlcas.hip): the device check, the KRAKIX2 scramble mask, the HIP check, launch geometry, rocPRIM's
// two-call protocol and its grow-only scratch (KuScratch), the clock (ku_now), StreamGuard, the default device budget, the
// staged copy from the device into the files of a KuDbFiles (ku_dbfiles.h: the one writer of a database.kdb + database.idx
// pair), the taxonomy's node table (KuNodeTable), and what the other tools borrow from db_sort (dbsort_unpack,
// dbsort_bin_order_and_pack).  `fail` and KU_TRY are those of ku_ctx.h.  Not part of the public ABI.
#pragma once
#include <unistd.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "ku_ctx.h"
#include "ku_dbfiles.h"
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

// ---- one clock for the tools' stage times (host clock around stages that end in a synchronise)
inline double ku_now() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// ---- the stream of one call
struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } };

// ---- device budget 0: half of what is free now, not below the tool's minimum
inline int ku_default_budget(const KuHipWho &who, uint64_t min_bytes, uint64_t *device_bytes) {
  if (*device_bytes) return KU_OK;
  size_t free_b = 0, total_b = 0;
  KU_HIP(who, hipMemGetInfo(&free_b, &total_b));
  *device_bytes = std::max<uint64_t>(free_b / 2, min_bytes);
  return KU_OK;
}

// ---- rocPRIM's scratch (ku_rocprim), grow-only: one buffer, handed over whole; when a call needs more, the stream is waited
// for and the buffer replaced.
struct KuScratch {
  struct Free { void operator()(void *q) const { (void)hipFree(q); } };
  std::unique_ptr<void, Free> p;
  size_t bytes = 0;
  auto provider(const KuHipWho &who, hipStream_t s) {
    return [this, who, s](size_t need, void *&tmp, size_t &have) -> int {
      if (need > bytes) {
        KU_HIP(who, hipStreamSynchronize(s));
        p.reset();
        bytes = 0;
        void *q = nullptr;
        KU_HIP(who, hipMalloc(&q, need));
        p.reset(q);
        bytes = need;
      }
      tmp = p.get();
      have = bytes;
      return KU_OK;
    };
  }
};

// ---- device -> one of the two files of a KuDbFiles, in pieces of KU_IO_PIECE through one reusable host buffer
constexpr size_t KU_IO_PIECE = (size_t)32 << 20;
inline int ku_append_from_device(const KuHipWho &who, KuDbFiles &out, bool (KuDbFiles::*append)(const void *, size_t),
                                 const void *d_src, uint64_t bytes, std::vector<uint8_t> &h_buf) {
  for (uint64_t at = 0; at < bytes;) {
    const size_t part = (size_t)std::min<uint64_t>(KU_IO_PIECE, bytes - at);
    if (h_buf.size() < part) h_buf.resize(part);
    KU_HIP(who, hipMemcpy(h_buf.data(), (const uint8_t *)d_src + at, part, hipMemcpyDeviceToHost));
    if (!(out.*append)(h_buf.data(), part)) {
      if (who.failed) *who.failed = true;
      return fail(KU_ENOINPUT, out.error);
    }
    at += part;
  }
  return KU_OK;
}

// ---- the taxonomy as the folds see it (ku_setlcas.hip, ku_dbmerge.hip): node universe = taxDB ids U the values of the
// databases U {0, 1}, ascending (node 0 = taxid 0, node 1 = taxid 1); Parent_map as a node array, 0 = no parent pointer.
// On the device a taxid finds its node with ku_node_of (ku_kmerdb.h).
struct KuNodeTable {
  std::vector<uint32_t> node_taxid, parent;
  int build(const ku_tax *tax, const std::vector<const ku_db *> &dbs) {
    for (const ku_db *db : dbs) {
      uint64_t nv = 0;
      KU_TRY(ku_db_values(db, nullptr, &nv));
      const size_t at = node_taxid.size();
      node_taxid.resize(at + nv);
      if (nv) KU_TRY(ku_db_values(db, node_taxid.data() + at, &nv));
    }
    node_taxid.insert(node_taxid.end(), tax->ids.begin(), tax->ids.end());
    node_taxid.push_back(0);
    node_taxid.push_back(1);
    std::sort(node_taxid.begin(), node_taxid.end());
    node_taxid.erase(std::unique(node_taxid.begin(), node_taxid.end()), node_taxid.end());
    parent.assign(node_taxid.size(), 0);
    for (size_t i = 0; i < tax->ids.size(); ++i)
      if (tax->ids[i] != 0 && tax->parent_map[i] != 0) parent[node_of(tax->ids[i])] = node_of(tax->parent_map[i]);
    return KU_OK;
  }
  uint32_t size() const { return (uint32_t)node_taxid.size(); }
  uint32_t node_of(uint32_t taxid) const {
    return (uint32_t)(std::lower_bound(node_taxid.begin(), node_taxid.end(), taxid) - node_taxid.begin());
  }
  bool has(uint32_t taxid) const { return std::binary_search(node_taxid.begin(), node_taxid.end(), taxid); }
  // both arrays into the caller's device buffers of size() entries each, enqueued on s (the table outlives the copies)
  int upload(const KuHipWho &who, hipStream_t s, uint32_t *d_parent, uint32_t *d_node_taxid) const {
    KU_HIP(who, hipMemcpyAsync(d_parent, parent.data(), parent.size() * 4, hipMemcpyHostToDevice, s));
    KU_HIP(who, hipMemcpyAsync(d_node_taxid, node_taxid.data(), node_taxid.size() * 4, hipMemcpyHostToDevice, s));
    return KU_OK;
  }
};

// ---- records in their on-disk form -> k-mers and values, the values zeroed on request; enqueued on s (ku_dbsort.hip)
int dbsort_unpack(const KuHipWho &who, hipStream_t s, const uint8_t *d_raw, uint64_t n, uint32_t key_len, uint64_t *d_kmer,
                  uint32_t *d_val, bool zero_vals);

// ---- the second half of db_sort (ku_dbsort.hip), shared with ku_kmerdb_end_pass.  In: n records sorted by k-mer (their
// values in d_val, or all 0 when it is null).  Computes the bin keys and their histogram over the bins [bin_lo, bin_lo +
// n_hist) -- every record's bin key must lie there --, sorts stably by bin key, which leaves the records in (bin key, k-mer)
// order, and packs them in their on-disk form.  Out (all enqueued on s, not yet waited for): *d_raw (allocated here when
// null) holds the n records, (*d_off)[b] = first_off + the number of records in the bins [bin_lo, bin_lo + b), b = 0 ..
// n_hist.  release_inputs: d_kmer and d_val belong to `dev` and are freed once they have been read.
int dbsort_bin_order_and_pack(Dev &dev, hipStream_t s, uint64_t *d_kmer, uint32_t *d_val, bool release_inputs, uint64_t n,
                              uint32_t k, uint32_t nt, uint32_t key_len, uint32_t bin_lo, uint64_t n_hist, uint64_t first_off,
                              uint8_t **d_raw, uint64_t **d_off);
