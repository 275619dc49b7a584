// ku_dbsort.hip -- db_sort on the GPU: a Jellyfish-format k-mer list -> database.kdb + database.idx.
//
// The reference (src/db_sort.cpp:34-128 + KrakenDB::make_index, src/krakendb.cpp:118-148) counts the records per
// minimizer bin, scatters them into their bins and qsort()s every bin by k-mer.  Here the same order -- ascending
// (bin key, k-mer) -- comes from two stable LSD radix sorts on the device (rocPRIM: by k-mer, then by bin key), the
// index from a histogram of the bin keys + an exclusive scan.  Offline tool, not on the classify hot path.
//
// ku_kmerdb_* (below ku_db_sort_files) builds the same two files straight from the library's sequences: it collects the
// distinct canonical k-mers on the device (ku_kmerdb.h) and hands them, sorted by k-mer, to the second half above.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "ku_device.h"
#include "ku_host.h"
#include "ku_internal.h"
#include "ku_kmerdb.h"
#include "ku_sketch.h"

namespace {

struct Rec {  // what travels through the second sort
  uint64_t kmer;
  uint32_t val;
  uint32_t pad;
};

// records of key_len + 4 bytes -> k-mer keys and values
__global__ void dbsort_unpack_kernel(const uint8_t *__restrict__ raw, uint64_t n, uint32_t key_len, uint64_t *kmers,
                                     uint32_t *vals, int zero_vals) {
  const uint64_t ps = key_len + 4;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint8_t *p = raw + i * ps;
    uint64_t kmer = 0;
    for (uint32_t b = 0; b < key_len; ++b) kmer |= (uint64_t)p[b] << (8 * b);
    uint32_t v = 0;
    for (uint32_t b = 0; b < 4; ++b) v |= (uint32_t)p[key_len + b] << (8 * b);
    kmers[i] = kmer;
    vals[i] = zero_vals ? 0u : v;  // db_sort -z (src/db_sort.cpp:103-104)
  }
}

// bin key of the stored k-mer (ku_bin_key, with the KRAKIX2 scramble mask) + the histogram of the bins from bin_lo on;
// vals == nullptr: every value is 0
__global__ void dbsort_binkey_kernel(const uint64_t *__restrict__ kmers, const uint32_t *__restrict__ vals, uint64_t n,
                                     uint32_t k, uint32_t nt, uint32_t xor_mask, uint32_t bin_lo, uint32_t *bins, Rec *recs,
                                     unsigned long long *hist) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t c = kmers[i];
    const uint32_t best = ku_bin_key(c, k, nt, xor_mask);
    bins[i] = best;
    recs[i] = Rec{c, vals ? vals[i] : 0u, 0u};
    atomicAdd(&hist[best - bin_lo], 1ull);
  }
}

// sorted records -> the on-disk form (key_len little-endian key bytes, 4 value bytes)
__global__ void dbsort_pack_kernel(const Rec *__restrict__ recs, uint64_t n, uint32_t key_len, uint8_t *raw) {
  const uint64_t ps = key_len + 4;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const Rec r = recs[i];
    uint8_t *p = raw + i * ps;
    for (uint32_t b = 0; b < key_len; ++b) p[b] = (uint8_t)(r.kmer >> (8 * b));
    for (uint32_t b = 0; b < 4; ++b) p[key_len + b] = (uint8_t)(r.val >> (8 * b));
  }
}

struct Dev {  // frees what it owns on every exit path
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

int fail(int code, const std::string &msg) {
  ku_set_error(msg);
  return code;
}

bool write_all(int fd, const void *buf, size_t n) {
  const char *p = (const char *)buf;
  while (n) {
    ssize_t w = ::write(fd, p, n < ((size_t)1 << 30) ? n : ((size_t)1 << 30));
    if (w <= 0) return false;
    p += w;
    n -= (size_t)w;
  }
  return true;
}

}  // namespace

#define DS_HIP(expr)                                                                             \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return fail(e_ == hipErrorOutOfMemory ? KU_ENOMEM : KU_EHIP,           \
                                      std::string("db_sort: ") + #expr + ": " + hipGetErrorString(e_)); \
  } while (0)

// The second half of db_sort, shared with ku_kmerdb_end_pass.  In: n records sorted by k-mer (their values in d_val, or all
// 0 when it is null).  Computes the bin keys and their histogram over the bins [bin_lo, bin_lo + n_hist) -- every record's
// bin key must lie there --, sorts stably by bin key, which leaves the records in (bin key, k-mer) order, and packs them
// in their on-disk form.  Out (all enqueued on s, not yet waited for): *d_raw (allocated here when null) holds the n
// records, (*d_off)[b] = first_off + the number of records in the bins [bin_lo, bin_lo + b), b = 0 .. n_hist.
// release_inputs: d_kmer and d_val belong to `dev` and are freed once they have been read.
static int dbsort_bin_order_and_pack(Dev &dev, hipStream_t s, uint64_t *d_kmer, uint32_t *d_val, bool release_inputs,
                                     uint64_t n, uint32_t k, uint32_t nt, uint32_t key_len, uint32_t bin_lo, uint64_t n_hist,
                                     uint64_t first_off, uint8_t **d_raw, uint64_t **d_off) {
  const uint64_t INDEX2_XOR_MASK = 0xe37e28c4271b5a2dULL;  // krakendb.cpp:45 (KRAKIX2)
  const uint32_t xor_mask = (uint32_t)(INDEX2_XOR_MASK & ((1ull << (2 * nt)) - 1));
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256 ? (n + 255) / 256 : 1, 1u << 16);
  uint32_t *d_bin_a = nullptr, *d_bin_b = nullptr;
  Rec *d_rec_a = nullptr, *d_rec_b = nullptr;
  unsigned long long *d_hist = nullptr;
  void *d_tmp = nullptr;
  // bin keys + histogram
  DS_HIP(dev.alloc(&d_bin_a, n * 4));
  DS_HIP(dev.alloc(&d_bin_b, n * 4));
  DS_HIP(dev.alloc(&d_rec_a, n * sizeof(Rec)));
  DS_HIP(dev.alloc(&d_hist, n_hist * 8));
  DS_HIP(hipMemsetAsync(d_hist, 0, n_hist * 8, s));
  hipLaunchKernelGGL(dbsort_binkey_kernel, dim3(grid), dim3(256), 0, s, d_kmer, d_val, n, k, nt, xor_mask, bin_lo, d_bin_a,
                     d_rec_a, d_hist);
  DS_HIP(hipGetLastError());
  DS_HIP(hipStreamSynchronize(s));
  if (release_inputs) { dev.release(d_kmer); dev.release(d_val); }
  // stable by bin key (2 nt bits) -> (bin, k-mer) order
  DS_HIP(dev.alloc(&d_rec_b, n * sizeof(Rec)));
  size_t tmp_bytes = 0;
  DS_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_bin_a, d_bin_b, d_rec_a, d_rec_b, (size_t)n, 0u, 2u * nt, s));
  DS_HIP(dev.alloc(&d_tmp, tmp_bytes));
  DS_HIP(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, d_bin_a, d_bin_b, d_rec_a, d_rec_b, (size_t)n, 0u, 2u * nt, s));
  DS_HIP(hipStreamSynchronize(s));
  dev.release(d_tmp); d_tmp = nullptr;
  dev.release(d_rec_a); dev.release(d_bin_a); dev.release(d_bin_b);
  // offsets[b] = number of records in bins < b, offsets past the last bin = all of them (make_index, krakendb.cpp:136-139)
  DS_HIP(dev.alloc(d_off, (n_hist + 1) * 8));
  tmp_bytes = 0;
  DS_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, (const uint64_t *)d_hist, *d_off, first_off, (size_t)n_hist,
                                 rocprim::plus<uint64_t>(), s));
  DS_HIP(dev.alloc(&d_tmp, tmp_bytes));
  DS_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, (const uint64_t *)d_hist, *d_off, first_off, (size_t)n_hist,
                                 rocprim::plus<uint64_t>(), s));
  const uint64_t end_off = first_off + n;
  DS_HIP(hipMemcpyAsync(*d_off + n_hist, &end_off, 8, hipMemcpyHostToDevice, s));
  if (!*d_raw) DS_HIP(dev.alloc(d_raw, n * (key_len + 4)));
  hipLaunchKernelGGL(dbsort_pack_kernel, dim3(grid), dim3(256), 0, s, d_rec_b, n, key_len, *d_raw);
  DS_HIP(hipGetLastError());
  DS_HIP(hipStreamSynchronize(s));  // (end_off leaves the stack, and d_tmp / d_hist may be freed by the caller's Dev)
  return KU_OK;
}

extern "C" int ku_db_sort_files(int device, const char *in_path, const char *out_kdb_path, const char *out_idx_path,
                                uint32_t nt, int zero_vals) {
  if (!in_path || !out_kdb_path || !out_idx_path) return fail(KU_EINVAL, "ku_db_sort_files: null argument");
  if (nt < 1 || nt > 15) return fail(KU_EINVAL, "bin key length out of range (1..15: 32-bit minimizers, krakendb.cpp:203)");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(KU_EHIP, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= n_dev) return fail(KU_EINVAL, "device index out of range");
  DS_HIP(hipSetDevice(device));

  // ---- input: JFLISTDN header (krakendb.cpp:60-78,151-177) + unsorted records
  int fd = ::open(in_path, O_RDONLY);
  if (fd < 0) return fail(KU_ENOINPUT, std::string("can't open ") + in_path);
  struct stat st;
  if (fstat(fd, &st) != 0 || st.st_size < 72) { ::close(fd); return fail(KU_EDATA, "database in improper format"); }
  const size_t in_sz = (size_t)st.st_size;
  void *map = mmap(nullptr, in_sz, PROT_READ, MAP_PRIVATE, fd, 0);
  ::close(fd);
  if (map == MAP_FAILED) return fail(KU_ENOINPUT, std::string("can't map ") + in_path);
  struct Unmap { void *p; size_t n; ~Unmap() { munmap(p, n); } } unmap{map, in_sz};
  const uint8_t *in = (const uint8_t *)map;
  if (memcmp(in, "JFLISTDN", 8) != 0) return fail(KU_EDATA, "database in improper format");
  uint64_t key_bits, val_len, key_ct;
  memcpy(&key_bits, in + 8, 8);
  memcpy(&val_len, in + 16, 8);
  memcpy(&key_ct, in + 48, 8);
  if (val_len != 4) return fail(KU_EDATA, "can only handle 4 byte DB values");
  if (key_bits == 0 || key_bits > 62 || (key_bits & 1)) return fail(KU_EDATA, "unsupported key_bits");
  const uint32_t k = (uint32_t)(key_bits / 2), key_len = (uint32_t)((key_bits + 7) / 8);
  if (nt > k) return fail(KU_EINVAL, "bin key longer than the k-mers");
  const size_t hdr = 72 + 2 * (4 + 8 * key_bits), ps = key_len + 4;
  if (in_sz < hdr || key_ct > (in_sz - hdr) / ps) return fail(KU_EDATA, "database file truncated");
  const uint64_t n = key_ct, n_bins = 1ull << (2 * nt);

  // ---- device pipeline
  Dev dev;
  hipStream_t s = nullptr;
  DS_HIP(hipStreamCreate(&s));
  struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } sg{s};
  uint8_t *d_raw = nullptr;
  uint64_t *d_kmer_a = nullptr, *d_kmer_b = nullptr, *d_off = nullptr;
  uint32_t *d_val_a = nullptr, *d_val_b = nullptr;
  void *d_tmp = nullptr;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256 ? (n + 255) / 256 : 1, 1u << 16);
  DS_HIP(dev.alloc(&d_raw, n * ps));
  DS_HIP(dev.alloc(&d_kmer_a, n * 8));
  DS_HIP(dev.alloc(&d_val_a, n * 4));
  if (n) DS_HIP(hipMemcpyAsync(d_raw, in + hdr, n * ps, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(dbsort_unpack_kernel, dim3(grid), dim3(256), 0, s, d_raw, n, key_len, d_kmer_a, d_val_a, zero_vals);
  DS_HIP(hipGetLastError());
  // pass 1: by k-mer (2k significant bits)
  DS_HIP(dev.alloc(&d_kmer_b, n * 8));
  DS_HIP(dev.alloc(&d_val_b, n * 4));
  size_t tmp_bytes = 0;
  DS_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_kmer_a, d_kmer_b, d_val_a, d_val_b, (size_t)n, 0u, (unsigned)key_bits, s));
  DS_HIP(dev.alloc(&d_tmp, tmp_bytes));
  DS_HIP(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, d_kmer_a, d_kmer_b, d_val_a, d_val_b, (size_t)n, 0u, (unsigned)key_bits, s));
  DS_HIP(hipStreamSynchronize(s));
  dev.release(d_tmp); d_tmp = nullptr;
  dev.release(d_kmer_a); dev.release(d_val_a);
  // second half: (bin key, k-mer) order, index offsets, records back in their on-disk form
  {
    const int st = dbsort_bin_order_and_pack(dev, s, d_kmer_b, d_val_b, /*release_inputs=*/true, n, k, nt, key_len, 0u, n_bins,
                                             0, &d_raw, &d_off);
    if (st != KU_OK) return st;
  }

  // ---- outputs: header copied verbatim (src/db_sort.cpp:56-75), then the sorted records; KRAKIX2 index
  std::vector<uint8_t> h_raw(n * ps);
  std::vector<uint64_t> h_off(n_bins + 1);
  if (n) DS_HIP(hipMemcpy(h_raw.data(), d_raw, n * ps, hipMemcpyDeviceToHost));
  DS_HIP(hipMemcpy(h_off.data(), d_off, (n_bins + 1) * 8, hipMemcpyDeviceToHost));
  int ofd = ::open(out_kdb_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (ofd < 0) return fail(KU_ENOINPUT, std::string("can't write ") + out_kdb_path);
  bool ok = write_all(ofd, in, hdr) && write_all(ofd, h_raw.data(), h_raw.size());
  ok = (::close(ofd) == 0) && ok;
  if (!ok) return fail(KU_ENOINPUT, std::string("write error on ") + out_kdb_path);
  ofd = ::open(out_idx_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (ofd < 0) return fail(KU_ENOINPUT, std::string("can't write ") + out_idx_path);
  const uint8_t nt8 = (uint8_t)nt;
  ok = write_all(ofd, "KRAKIX2", 7) && write_all(ofd, &nt8, 1) && write_all(ofd, h_off.data(), h_off.size() * 8);
  ok = (::close(ofd) == 0) && ok;
  if (!ok) return fail(KU_ENOINPUT, std::string("write error on ") + out_idx_path);
  return KU_OK;
}

// =====================================================================================================================
// ku_kmerdb_*: library sequences -> sorted database.kdb + database.idx (scripts/build_db.sh steps 2-3: jellyfish count /
// merge / dump into database.jdb, then db_sort -z).  With zeroed values both files depend only on the SET of canonical
// k-mers, so no counts are kept: the extraction kernel (ku_kmerdb.h) appends every canonical, unambiguous k-mer of the
// uploaded segment to a device buffer; when the next launch might not fit, the candidates are sorted, made unique and
// merged into the pass's sorted distinct set, which lives at the front of the same buffer.  ku_kmerdb_end_pass hands the
// set to dbsort_bin_order_and_pack and appends its records and its part of the index to the files.  (ku_sketch_*, at the end
// of this file, estimates beforehand how many passes a library needs.)
//
// Budget rule (include/krakenuniq_amd.h): segment = min(64 MiB, device_bytes / 64) rounded down to 1 KiB, capacity =
// (device_bytes - segment) / 16 k-mers in each of two buffers (the second is the sort's and the merge's other side).
struct ku_kmerdb {
  int device = 0;
  uint32_t k = 0, nt = 0, n_passes = 0, key_len = 0;
  uint32_t pass = 0;  // passes ended
  bool finished = false, failed = false;
  uint64_t n_bins = 0, cap = 0, seg_bytes = 0;
  std::string kdb_path, idx_path;
  int kdb_fd = -1, idx_fd = -1;
  hipStream_t stream = nullptr;
  uint64_t *d_a = nullptr, *d_b = nullptr;  // d_a: the distinct set [0, n_set), then the candidates [n_set, fill)
  uint8_t *d_seq = nullptr;
  unsigned long long *d_ctl = nullptr;      // [0] the buffer's cursor, [1] rocPRIM's unique count, [2] the kernel's error word
  void *d_tmp = nullptr;
  size_t tmp_bytes = 0;
  uint64_t n_set = 0, fill = 0, key_ct = 0;
  uint64_t merge_piece = 0;  // keys of either input per rocprim::merge call (kmd_merge)
  uint64_t merge_calls = 0;  // of the running pass
  uint64_t windows = 0, candidates = 0, flushes = 0, segments = 0;  // of the running pass
  ku_kmerdb_stats stats{};
  std::vector<uint8_t> h_buf;
};

namespace {

constexpr uint64_t KMD_MAX_SEGMENT = (uint64_t)64 << 20;
constexpr size_t KMD_IO_CHUNK = (size_t)32 << 20;

int kmd_fail(ku_kmerdb *h, int code, const std::string &msg) {
  h->failed = true;
  return fail(code, msg);
}

double kmd_now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// bins of pass p: [p * 4^nt / n_passes, (p + 1) * 4^nt / n_passes)
uint64_t kmd_pass_bound(const ku_kmerdb *h, uint32_t p) { return (uint64_t)p * h->n_bins / h->n_passes; }

}  // namespace

#define KMD_HIP(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return kmd_fail(h, e_ == hipErrorOutOfMemory ? KU_ENOMEM : KU_EHIP,          \
                                          std::string("kmer_db: ") + #expr + ": " + hipGetErrorString(e_) + \
                                              (e_ == hipErrorOutOfMemory ? " (a smaller -s, or more passes: -P)" : "")); \
  } while (0)

static int kmd_reserve_tmp(ku_kmerdb *h, size_t bytes) {
  if (bytes <= h->tmp_bytes) return KU_OK;
  KMD_HIP(hipStreamSynchronize(h->stream));
  if (h->d_tmp) (void)hipFree(h->d_tmp);
  h->d_tmp = nullptr;
  h->tmp_bytes = 0;
  KMD_HIP(hipMalloc(&h->d_tmp, bytes));
  h->tmp_bytes = bytes;
  return KU_OK;
}

// first index in the sorted device array [0, n) whose key is not below `key` (host-driven: one 8-byte copy per step; used for
// the few cut points of kmd_merge only)
static int kmd_lower_bound(ku_kmerdb *h, const uint64_t *d, uint64_t n, uint64_t key, uint64_t *at) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    uint64_t v = 0;
    KMD_HIP(hipMemcpyAsync(&v, d + mid, 8, hipMemcpyDeviceToHost, h->stream));
    KMD_HIP(hipStreamSynchronize(h->stream));
    if (v < key) lo = mid + 1; else hi = mid;
  }
  *at = lo;
  return KU_OK;
}

// out[0, na + nb) = the merge of the sorted device arrays a[0, na) and b[0, nb).  rocprim::merge takes size_t sizes but works
// on 32-bit ones inside (the sum of both inputs, the partition indices and the block count of
// rocprim/device/detail/device_merge.hpp are unsigned int), and a buffer under the default budget holds more than 2^32 k-mers.
// So the merge goes in pieces cut at KEY boundaries: the cut keys are every `piece`-th key of a and of b; between two
// consecutive cut keys lie at most `piece` keys of each input (its own cuts are among them), a cut key's lower bound in
// either array says where the piece starts there, and the pieces follow each other in the output.  piece = h->merge_piece <=
// 2^30, so no call sees 2^31 keys or more; it is a quarter of the capacity below that, so that small budgets merge in
// several pieces too (the tests' budgets do).  The order of equal keys does not matter: a unique pass follows.
static int kmd_merge(ku_kmerdb *h, const uint64_t *a, uint64_t na, const uint64_t *b, uint64_t nb, uint64_t *out) {
  hipStream_t s = h->stream;
  const uint64_t piece = h->merge_piece;
  std::vector<uint64_t> cuts;
  for (int side = 0; side < 2; ++side) {
    const uint64_t *d = side ? b : a;
    const uint64_t n = side ? nb : na;
    for (uint64_t i = piece; i < n; i += piece) {
      uint64_t v = 0;
      KMD_HIP(hipMemcpyAsync(&v, d + i, 8, hipMemcpyDeviceToHost, s));
      KMD_HIP(hipStreamSynchronize(s));
      cuts.push_back(v);
    }
  }
  std::sort(cuts.begin(), cuts.end());
  cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
  uint64_t a0 = 0, b0 = 0;
  for (size_t c = 0; c <= cuts.size(); ++c) {
    uint64_t a1 = na, b1 = nb;
    if (c < cuts.size()) {
      if (int st = kmd_lower_bound(h, a, na, cuts[c], &a1)) return st;
      if (int st = kmd_lower_bound(h, b, nb, cuts[c], &b1)) return st;
    }
    const uint64_t la = a1 - a0, lb = b1 - b0;
    if (la > piece || lb > piece || la + lb >= (1ull << 32))  // (cannot happen by construction: never hand rocPRIM a size it would truncate)
      return kmd_fail(h, KU_EHIP, "kmer_db: a merge piece of " + std::to_string(la) + " + " + std::to_string(lb) + " k-mers exceeds the limit of rocprim::merge");
    if (la + lb) {
      size_t need = 0;
      KMD_HIP(rocprim::merge(nullptr, need, a + a0, b + b0, out + a0 + b0, (size_t)la, (size_t)lb, rocprim::less<uint64_t>(), s));
      if (int st = kmd_reserve_tmp(h, need)) return st;
      need = h->tmp_bytes;
      KMD_HIP(rocprim::merge(h->d_tmp, need, a + a0, b + b0, out + a0 + b0, (size_t)la, (size_t)lb, rocprim::less<uint64_t>(), s));
      h->merge_calls++;
    }
    a0 = a1;
    b0 = b1;
  }
  return KU_OK;
}

// candidates [n_set, fill) -> sorted, unique, merged into the sorted distinct set [0, n_set)
static int kmd_flush(ku_kmerdb *h) {
  const uint64_t m = h->fill - h->n_set;
  if (m == 0) return KU_OK;
  const double t0 = kmd_now();
  hipStream_t s = h->stream;
  uint64_t *a_side = h->d_a + h->n_set, *b_side = h->d_b + h->n_set;
  rocprim::double_buffer<uint64_t> keys(a_side, b_side);
  size_t need = 0;
  KMD_HIP(rocprim::radix_sort_keys(nullptr, need, keys, (size_t)m, 0u, 2u * h->k, s));
  if (int st = kmd_reserve_tmp(h, need)) return st;
  need = h->tmp_bytes;
  KMD_HIP(rocprim::radix_sort_keys(h->d_tmp, need, keys, (size_t)m, 0u, 2u * h->k, s));
  uint64_t *sorted = keys.current(), *uniq = sorted == a_side ? b_side : a_side;
  unsigned long long *d_count = h->d_ctl + 1;
  need = 0;
  KMD_HIP(rocprim::unique(nullptr, need, sorted, uniq, d_count, (size_t)m, rocprim::equal_to<uint64_t>(), s));
  if (int st = kmd_reserve_tmp(h, need)) return st;
  need = h->tmp_bytes;
  KMD_HIP(rocprim::unique(h->d_tmp, need, sorted, uniq, d_count, (size_t)m, rocprim::equal_to<uint64_t>(), s));
  unsigned long long u = 0;
  KMD_HIP(hipMemcpyAsync(&u, d_count, 8, hipMemcpyDeviceToHost, s));
  KMD_HIP(hipStreamSynchronize(s));
  // the new k-mers next to the set in d_a; the merge writes to d_b
  if (uniq != a_side) KMD_HIP(hipMemcpyAsync(a_side, uniq, u * 8, hipMemcpyDeviceToDevice, s));
  if (h->n_set == 0) {
    h->n_set = u;
  } else {
    if (int st = kmd_merge(h, h->d_a, h->n_set, a_side, u, h->d_b)) return st;
    const size_t merged = (size_t)(h->n_set + u);  // a k-mer of the set that came up again is there twice
    need = 0;
    KMD_HIP(rocprim::unique(nullptr, need, h->d_b, h->d_a, d_count, merged, rocprim::equal_to<uint64_t>(), s));
    if (int st = kmd_reserve_tmp(h, need)) return st;
    need = h->tmp_bytes;
    KMD_HIP(rocprim::unique(h->d_tmp, need, h->d_b, h->d_a, d_count, merged, rocprim::equal_to<uint64_t>(), s));
    KMD_HIP(hipMemcpyAsync(&u, d_count, 8, hipMemcpyDeviceToHost, s));
    KMD_HIP(hipStreamSynchronize(s));
    h->n_set = u;
  }
  h->fill = h->n_set;
  const unsigned long long cur = h->fill;
  KMD_HIP(hipMemcpyAsync(h->d_ctl, &cur, 8, hipMemcpyHostToDevice, s));
  KMD_HIP(hipStreamSynchronize(s));
  h->flushes++;
  h->stats.flush_s += kmd_now() - t0;
  if (h->n_set > h->cap - h->cap / 64)
    return kmd_fail(h, KU_ENOMEM, "kmer_db: the distinct k-mers of pass " + std::to_string(h->pass + 1) + " (" + std::to_string(h->n_set) +
                                      " so far) do not fit the device budget (" + std::to_string(h->cap) +
                                      " k-mers, 1/64 of them kept free): use more passes (-P) or a larger budget (-s)");
  return KU_OK;
}

static int kmd_open_impl(ku_kmerdb *h, uint64_t device_bytes) {
  KMD_HIP(hipSetDevice(h->device));
  if (device_bytes == 0) {  // half of what is free now: the rest is end_pass's (56 bytes per distinct k-mer of the pass)
    size_t free_b = 0, total_b = 0;
    KMD_HIP(hipMemGetInfo(&free_b, &total_b));
    device_bytes = free_b / 2;
  }
  if (device_bytes < KU_KMERDB_MIN_BYTES) return kmd_fail(h, KU_EINVAL, "kmer_db: the device budget is below the minimum of 64 KiB");
  h->seg_bytes = std::min<uint64_t>(KMD_MAX_SEGMENT, device_bytes / 64) & ~(uint64_t)1023;
  h->cap = (device_bytes - h->seg_bytes) / 16;
  h->merge_piece = std::min<uint64_t>((uint64_t)1 << 30, std::max<uint64_t>(h->cap / 4, 1024));
  // ---- outputs: both files exist (and are writable) before any work is done
  h->kdb_fd = ::open(h->kdb_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (h->kdb_fd < 0) return kmd_fail(h, KU_ENOINPUT, "can't write " + h->kdb_path);
  h->idx_fd = ::open(h->idx_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (h->idx_fd < 0) return kmd_fail(h, KU_ENOINPUT, "can't write " + h->idx_path);
  // Jellyfish-1 list header as KrakenDB reads it (krakendb.cpp:60-78,177): key_ct is patched in by ku_kmerdb_finish
  const uint64_t key_bits = 2ull * h->k, val_len = 4;
  std::vector<uint8_t> hdr(72 + 2 * (4 + 8 * key_bits), 0);
  memcpy(hdr.data(), "JFLISTDN", 8);
  memcpy(hdr.data() + 8, &key_bits, 8);
  memcpy(hdr.data() + 16, &val_len, 8);
  const uint8_t nt8 = (uint8_t)h->nt;
  if (!write_all(h->kdb_fd, hdr.data(), hdr.size())) return kmd_fail(h, KU_ENOINPUT, "write error on " + h->kdb_path);
  if (!write_all(h->idx_fd, "KRAKIX2", 7) || !write_all(h->idx_fd, &nt8, 1)) return kmd_fail(h, KU_ENOINPUT, "write error on " + h->idx_path);
  // ---- device
  KMD_HIP(hipStreamCreate(&h->stream));
  KMD_HIP(hipMalloc((void **)&h->d_a, h->cap * 8));
  KMD_HIP(hipMalloc((void **)&h->d_b, h->cap * 8));
  KMD_HIP(hipMalloc((void **)&h->d_seq, h->seg_bytes));
  KMD_HIP(hipMalloc((void **)&h->d_ctl, 3 * 8));
  KMD_HIP(hipMemsetAsync(h->d_ctl, 0, 3 * 8, h->stream));
  KMD_HIP(hipStreamSynchronize(h->stream));
  h->stats.capacity = h->cap;
  h->stats.segment_bytes = h->seg_bytes;
  return KU_OK;
}

extern "C" int ku_kmerdb_open(int device, uint32_t k, uint32_t nt, uint32_t n_passes, uint64_t device_bytes,
                              const char *out_kdb_path, const char *out_idx_path, ku_kmerdb **out) {
  if (!out_kdb_path || !out_idx_path || !out) return fail(KU_EINVAL, "ku_kmerdb_open: null argument");
  *out = nullptr;
  if (nt < 1 || nt > 15) return fail(KU_EINVAL, "bin key length out of range (1..15: 32-bit minimizers, krakendb.cpp:203)");
  if (k < nt || k > 31) return fail(KU_EINVAL, "k out of range (nt..31)");
  if (n_passes < 1 || n_passes > (1ull << (2 * nt))) return fail(KU_EINVAL, "the number of passes must lie in 1..4^nt (a pass owns at least one bin)");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(KU_EHIP, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= n_dev) return fail(KU_EINVAL, "device index out of range");
  ku_kmerdb *h = new ku_kmerdb();
  h->device = device;
  h->k = k;
  h->nt = nt;
  h->n_passes = n_passes;
  h->key_len = (2 * k + 7) / 8;
  h->n_bins = 1ull << (2 * nt);
  h->kdb_path = out_kdb_path;
  h->idx_path = out_idx_path;
  const int st = kmd_open_impl(h, device_bytes);
  if (st != KU_OK) { ku_kmerdb_close(h); return st; }
  *out = h;
  return KU_OK;
}

extern "C" void ku_kmerdb_close(ku_kmerdb *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void *p : {(void *)h->d_a, (void *)h->d_b, (void *)h->d_seq, (void *)h->d_ctl, h->d_tmp})
    if (p) (void)hipFree(p);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  // files of a build that did not reach the end of ku_kmerdb_finish are not databases: none is left behind
  if (h->kdb_fd >= 0) { ::close(h->kdb_fd); ::unlink(h->kdb_path.c_str()); }
  if (h->idx_fd >= 0) { ::close(h->idx_fd); ::unlink(h->idx_path.c_str()); }
  delete h;
}

extern "C" int ku_kmerdb_add(ku_kmerdb *h, const char *seq, uint64_t len) {
  if (!h || (len && !seq)) return fail(KU_EINVAL, "ku_kmerdb_add: null argument");
  if (h->failed) return fail(KU_EINVAL, "ku_kmerdb_add: an earlier call on this handle failed");
  if (h->finished || h->pass >= h->n_passes) return fail(KU_EINVAL, "ku_kmerdb_add: every pass has been ended");
  if (len < h->k) return KU_OK;
  KMD_HIP(hipSetDevice(h->device));
  const double t0 = kmd_now(), flush_s0 = h->stats.flush_s;
  hipStream_t s = h->stream;
  const uint32_t k = h->k;
  const uint64_t INDEX2_XOR_MASK = 0xe37e28c4271b5a2dULL;  // krakendb.cpp:45 (KRAKIX2)
  KmdScan a{};
  a.seq = h->d_seq;
  a.seq_bytes = h->seg_bytes;
  a.k = k;
  a.nt = h->nt;
  a.xor_mask = (uint32_t)(INDEX2_XOR_MASK & (h->n_bins - 1));
  a.bin_lo = (uint32_t)kmd_pass_bound(h, h->pass);
  a.bin_hi = (uint32_t)kmd_pass_bound(h, h->pass + 1);
  a.pass_mode = h->n_passes > 1;
  a.out = h->d_a;
  a.cap = h->cap;
  a.cursor = h->d_ctl;
  a.err = reinterpret_cast<uint32_t *>(h->d_ctl + 2);
  // A record longer than one segment is cut with k - 1 bytes of overlap: the windows that start in [pos, pos + n_win) belong to
  // the segment at pos and the next segment starts at pos + n_win, so every window is scanned exactly once.
  for (uint64_t pos = 0;;) {
    const uint64_t seg_len = std::min<uint64_t>(h->seg_bytes, len - pos), n_win = seg_len - k + 1;
    KMD_HIP(hipMemcpyAsync(h->d_seq, seq + pos, seg_len, hipMemcpyHostToDevice, s));
    h->segments++;
    for (uint64_t w = 0; w < n_win;) {
      // the buffer is flushed BEFORE a launch that could overflow it: a launch keeps at most one k-mer per window
      if (n_win - w > h->cap - h->fill && h->fill > h->n_set) {
        if (int st = kmd_flush(h)) return st;
      }
      const uint64_t take = std::min<uint64_t>(n_win - w, h->cap - h->fill);  // > 0: a flush leaves cap / 64 k-mers free
      a.w_lo = w;
      a.w_hi = w + take;
      const uint64_t tiles = (a.w_hi + KMD_TILE - 1) / KMD_TILE - a.w_lo / KMD_TILE;
      const unsigned grid = (unsigned)std::min<uint64_t>((tiles + KMD_WAVES - 1) / KMD_WAVES, 2048);
      hipLaunchKernelGGL(kmerdb_extract_kernel, dim3(grid), dim3(64 * KMD_WAVES), 0, s, a);
      KMD_HIP(hipGetLastError());
      unsigned long long ctl[3] = {0, 0, 0};
      KMD_HIP(hipMemcpyAsync(ctl, h->d_ctl, sizeof ctl, hipMemcpyDeviceToHost, s));
      KMD_HIP(hipStreamSynchronize(s));
      if (ctl[2] || ctl[0] < h->fill || ctl[0] > h->cap) return kmd_fail(h, KU_EHIP, "kmer_db: the extraction kernel ran out of the room it was given");
      h->windows += take;
      h->candidates += ctl[0] - h->fill;
      h->fill = ctl[0];
      w += take;
    }
    if (pos + seg_len == len) break;
    pos += n_win;
  }
  h->stats.scan_s += (kmd_now() - t0) - (h->stats.flush_s - flush_s0);  // upload + extraction: the flushes are counted apart
  return KU_OK;
}

extern "C" int ku_kmerdb_end_pass(ku_kmerdb *h) {
  if (!h) return fail(KU_EINVAL, "ku_kmerdb_end_pass: null argument");
  if (h->failed) return fail(KU_EINVAL, "ku_kmerdb_end_pass: an earlier call on this handle failed");
  if (h->finished || h->pass >= h->n_passes) return fail(KU_EINVAL, "ku_kmerdb_end_pass: every pass has been ended");
  KMD_HIP(hipSetDevice(h->device));
  if (int st = kmd_flush(h)) return st;
  const double t0 = kmd_now();
  hipStream_t s = h->stream;
  const uint64_t n = h->n_set, ps = h->key_len + 4;
  const uint64_t bin_lo = kmd_pass_bound(h, h->pass), n_hist = kmd_pass_bound(h, h->pass + 1) - bin_lo;
  // the second half's arrays: 56 bytes per k-mer at their peak, 16 per bin.  Where the device cannot hold them next to both
  // buffers, the sort's other side, idle now, makes room (an allocation of that size takes seconds: not given back needlessly)
  {
    size_t free_b = 0, total_b = 0;
    KMD_HIP(hipMemGetInfo(&free_b, &total_b));
    const uint64_t need = n * 56 + (n_hist + 1) * 16 + ((uint64_t)256 << 20);
    if (need > free_b) {
      (void)hipFree(h->d_b);
      h->d_b = nullptr;
    }
  }
  {
    Dev dev;
    uint8_t *d_raw = nullptr;
    uint64_t *d_off = nullptr;
    const int st = dbsort_bin_order_and_pack(dev, s, h->d_a, nullptr, /*release_inputs=*/false, n, h->k, h->nt, h->key_len,
                                             (uint32_t)bin_lo, n_hist, h->key_ct, &d_raw, &d_off);
    if (st != KU_OK) {
      h->failed = true;
      if (st == KU_ENOMEM) ku_set_error(std::string(ku_last_error()) + " -- kmer_db: use more passes (-P)");
      return st;
    }
    h->h_buf.resize(KMD_IO_CHUNK);
    for (uint64_t at = 0, total = n * ps; at < total;) {  // the pass's records, behind those of the passes before
      const size_t part = (size_t)std::min<uint64_t>(KMD_IO_CHUNK, total - at);
      KMD_HIP(hipMemcpy(h->h_buf.data(), d_raw + at, part, hipMemcpyDeviceToHost));
      if (!write_all(h->kdb_fd, h->h_buf.data(), part)) return kmd_fail(h, KU_ENOINPUT, "write error on " + h->kdb_path);
      at += part;
    }
    for (uint64_t at = 0, total = n_hist * 8; at < total;) {  // offsets of the pass's bins (the closing one: ku_kmerdb_finish)
      const size_t part = (size_t)std::min<uint64_t>(KMD_IO_CHUNK, total - at);
      KMD_HIP(hipMemcpy(h->h_buf.data(), (const uint8_t *)d_off + at, part, hipMemcpyDeviceToHost));
      if (!write_all(h->idx_fd, h->h_buf.data(), part)) return kmd_fail(h, KU_ENOINPUT, "write error on " + h->idx_path);
      at += part;
    }
  }
  h->key_ct += n;
  h->stats.windows = h->windows;
  h->stats.candidates = h->candidates;
  h->stats.flushes = h->flushes;
  h->stats.segments = h->segments;
  h->stats.merge_calls = h->merge_calls;
  h->stats.distinct = n;
  h->stats.total_distinct = h->key_ct;
  h->windows = h->candidates = h->flushes = h->segments = h->merge_calls = 0;
  h->n_set = h->fill = 0;
  h->pass++;
  h->stats.passes_done = h->pass;
  KMD_HIP(hipMemsetAsync(h->d_ctl, 0, 3 * 8, s));
  KMD_HIP(hipStreamSynchronize(s));
  if (!h->d_b && h->pass < h->n_passes) KMD_HIP(hipMalloc((void **)&h->d_b, h->cap * 8));
  h->stats.end_pass_s += kmd_now() - t0;
  return KU_OK;
}

extern "C" int ku_kmerdb_get_stats(const ku_kmerdb *h, ku_kmerdb_stats *out) {
  if (!h || !out) return fail(KU_EINVAL, "ku_kmerdb_get_stats: null argument");
  *out = h->stats;
  return KU_OK;
}

extern "C" int ku_kmerdb_finish(ku_kmerdb *h, uint64_t *key_ct) {
  if (!h) return fail(KU_EINVAL, "ku_kmerdb_finish: null argument");
  if (h->failed) return fail(KU_EINVAL, "ku_kmerdb_finish: an earlier call on this handle failed");
  if (h->finished) return fail(KU_EINVAL, "ku_kmerdb_finish: called twice");
  if (h->pass < h->n_passes)
    return fail(KU_EINVAL, "ku_kmerdb_finish: " + std::to_string(h->n_passes - h->pass) + " of " + std::to_string(h->n_passes) + " passes have not been ended");
  if (h->key_ct == 0) return kmd_fail(h, KU_EDATA, "kmer_db: no k-mers in the input");  // (ku_kmerdb_close removes the files)
  // offsets[4^nt] = key_ct (make_index, krakendb.cpp:136-139); key_ct into the header (krakendb.cpp:72)
  bool ok = write_all(h->idx_fd, &h->key_ct, 8);
  ok = (::close(h->idx_fd) == 0) && ok;
  h->idx_fd = -1;
  if (!ok) { ::unlink(h->idx_path.c_str()); return kmd_fail(h, KU_ENOINPUT, "write error on " + h->idx_path); }
  ok = ::pwrite(h->kdb_fd, &h->key_ct, 8, 48) == 8;
  ok = (::close(h->kdb_fd) == 0) && ok;
  h->kdb_fd = -1;
  if (!ok) { ::unlink(h->kdb_path.c_str()); ::unlink(h->idx_path.c_str()); return kmd_fail(h, KU_ENOINPUT, "write error on " + h->kdb_path); }
  h->finished = true;
  if (key_ct) *key_ct = h->key_ct;
  return KU_OK;
}

// =====================================================================================================================
// ku_sketch_*: HyperLogLog sketches of a library's k-mers (ku_sketch.h): bin/count_unique (one sketch of the forward k-mers,
// the reference's count_unique) and kmer_db -P auto (one sketch of the canonical k-mers per range of the bin keys).
//
// ku_sketch_add packs the records into one of two pinned staging segments, one non-ACGT byte between two of them -- a window
// across two records holds it and is dropped as ambiguous --, so a launch scans a whole segment however short the records
// are.  A full segment is uploaded and scanned on the handle's stream and an event recorded behind it; the host goes on
// packing into the other segment and waits for a segment's event only when it comes back to it.
struct ku_sketch {
  int device = 0;
  uint32_t k = 0, p = 0, flags = 0, nt = 0, n_groups = 1;
  uint64_t seg_bytes = 0;
  bool failed = false;
  hipStream_t stream = nullptr;
  char *h_seg[2] = {nullptr, nullptr};     // pinned
  uint8_t *d_seg[2] = {nullptr, nullptr};
  hipEvent_t done[2] = {nullptr, nullptr};  // behind the last work that reads h_seg[i] / d_seg[i]
  bool in_flight[2] = {false, false};
  int cur = 0;           // the segment being packed
  uint64_t fill = 0;     // bytes packed into it
  uint8_t *d_reg = nullptr;
  unsigned long long *d_obs = nullptr;
  uint64_t values_observed = 0;  // ku_sketch_add_values counts on the host
};

namespace {

constexpr uint64_t SK_MAX_GROUPS = 1024;
constexpr char SK_SEPARATOR = 'N';

int sk_fail(ku_sketch *h, int code, const std::string &msg) {
  h->failed = true;
  return fail(code, msg);
}

}  // namespace

#define SK_HIP(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) return sk_fail(h, e_ == hipErrorOutOfMemory ? KU_ENOMEM : KU_EHIP,      \
                                         std::string("sketch: ") + #expr + ": " + hipGetErrorString(e_)); \
  } while (0)

// the segment being packed may be written: what read it last has finished
static int sk_segment_ready(ku_sketch *h) {
  if (h->in_flight[h->cur]) {
    SK_HIP(hipEventSynchronize(h->done[h->cur]));
    h->in_flight[h->cur] = false;
  }
  return KU_OK;
}

// upload the packed segment and scan its windows; the other segment is packed next
static int sk_scan_segment(ku_sketch *h) {
  const uint64_t fill = h->fill;
  h->fill = 0;
  if (fill < h->k) return KU_OK;  // no window
  const int c = h->cur;
  hipStream_t s = h->stream;
  SK_HIP(hipMemcpyAsync(h->d_seg[c], h->h_seg[c], fill, hipMemcpyHostToDevice, s));
  const uint64_t INDEX2_XOR_MASK = 0xe37e28c4271b5a2dULL;  // krakendb.cpp:45 (KRAKIX2)
  KuSketchScan a{};
  a.seq = h->d_seg[c];
  a.seq_bytes = h->seg_bytes;  // (bytes behind `fill` are those of an earlier segment: no window below reaches them)
  a.w_lo = 0;
  a.w_hi = fill - h->k + 1;
  a.k = h->k;
  a.p = h->p;
  a.canonical = (h->flags & KU_SKETCH_CANONICAL) ? 1u : 0u;
  a.nt = h->nt;
  a.xor_mask = h->n_groups > 1 ? (uint32_t)(INDEX2_XOR_MASK & ((1ull << (2 * h->nt)) - 1)) : 0u;
  a.n_groups = h->n_groups;
  a.registers = h->d_reg;
  a.n_observed = h->d_obs;
  const uint64_t tiles = (a.w_hi + KMD_TILE - 1) / KMD_TILE;
  const unsigned grid = (unsigned)std::min<uint64_t>((tiles + KMD_WAVES - 1) / KMD_WAVES, 2048);
  hipLaunchKernelGGL(kmersketch_kernel, dim3(grid), dim3(64 * KMD_WAVES), 0, s, a);
  SK_HIP(hipGetLastError());
  SK_HIP(hipEventRecord(h->done[c], s));
  h->in_flight[c] = true;
  h->cur = c ^ 1;
  return KU_OK;
}

extern "C" int ku_sketch_open(int device, uint32_t k, uint32_t p, uint32_t flags, uint32_t nt, uint32_t n_groups,
                              uint64_t segment_bytes, ku_sketch **out) {
  if (!out) return fail(KU_EINVAL, "ku_sketch_open: null argument");
  *out = nullptr;
  if (k < 1 || k > 31) return fail(KU_EINVAL, "k out of range (1..31)");
  if (p < 4 || p > 18) return fail(KU_EINVAL, "HLL precision out of range (4..18)");
  if (flags & ~(uint32_t)KU_SKETCH_CANONICAL) return fail(KU_EINVAL, "ku_sketch_open: unknown flag");
  if (n_groups != 1) {
    if (nt < 1 || nt > 15) return fail(KU_EINVAL, "bin key length out of range (1..15: 32-bit minimizers, krakendb.cpp:203)");
    if (k < nt) return fail(KU_EINVAL, "bin key longer than the k-mers");
    if (n_groups == 0 || (n_groups & (n_groups - 1)) || n_groups > std::min<uint64_t>(SK_MAX_GROUPS, 1ull << (2 * nt)))
      return fail(KU_EINVAL, "the number of groups must be 1 or a power of two up to min(1024, 4^nt)");
    if (!(flags & KU_SKETCH_CANONICAL)) return fail(KU_EINVAL, "groups need KU_SKETCH_CANONICAL: the bin key is defined on canonical k-mers");
  }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(KU_EHIP, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= n_dev) return fail(KU_EINVAL, "device index out of range");
  ku_sketch *h = new ku_sketch();
  h->device = device;
  h->k = k;
  h->p = p;
  h->flags = flags;
  h->nt = nt;
  h->n_groups = n_groups;
  h->seg_bytes = std::max<uint64_t>((segment_bytes ? segment_bytes : KMD_MAX_SEGMENT) & ~(uint64_t)1023, 1024);
  const int st = [&]() -> int {
    SK_HIP(hipSetDevice(device));
    SK_HIP(hipStreamCreate(&h->stream));
    for (int i = 0; i < 2; ++i) {
      SK_HIP(hipHostMalloc((void **)&h->h_seg[i], h->seg_bytes, hipHostMallocDefault));
      SK_HIP(hipMalloc((void **)&h->d_seg[i], h->seg_bytes));
      SK_HIP(hipEventCreateWithFlags(&h->done[i], hipEventDisableTiming));
    }
    SK_HIP(hipMalloc((void **)&h->d_reg, (size_t)n_groups << p));
    SK_HIP(hipMalloc((void **)&h->d_obs, 8));
    SK_HIP(hipMemsetAsync(h->d_reg, 0, (size_t)n_groups << p, h->stream));
    SK_HIP(hipMemsetAsync(h->d_obs, 0, 8, h->stream));
    SK_HIP(hipStreamSynchronize(h->stream));
    return KU_OK;
  }();
  if (st != KU_OK) { ku_sketch_close(h); return st; }
  *out = h;
  return KU_OK;
}

extern "C" void ku_sketch_close(ku_sketch *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (int i = 0; i < 2; ++i) {
    if (h->done[i]) (void)hipEventDestroy(h->done[i]);
    if (h->d_seg[i]) (void)hipFree(h->d_seg[i]);
    if (h->h_seg[i]) (void)hipHostFree(h->h_seg[i]);
  }
  if (h->d_reg) (void)hipFree(h->d_reg);
  if (h->d_obs) (void)hipFree(h->d_obs);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int ku_sketch_add(ku_sketch *h, const char *seq, uint64_t len) {
  if (!h || (len && !seq)) return fail(KU_EINVAL, "ku_sketch_add: null argument");
  if (h->failed) return fail(KU_EINVAL, "ku_sketch_add: an earlier call on this handle failed");
  const uint64_t k = h->k, seg = h->seg_bytes;
  if (len < k) return KU_OK;  // no window
  SK_HIP(hipSetDevice(h->device));
  // A record longer than the room left is cut with k - 1 bytes of overlap: the part packed here ends the segment, its windows
  // are all those that start in [pos, pos + take - k], and the next part starts at the window behind them.
  for (uint64_t pos = 0;;) {
    const uint64_t rem = len - pos;  // >= k
    if (seg - h->fill < k) {         // not one window's worth of room (fill > 0: a segment holds at least 1 KiB)
      if (int st = sk_scan_segment(h)) return st;
      continue;
    }
    if (h->fill == 0)
      if (int st = sk_segment_ready(h)) return st;
    const uint64_t take = std::min<uint64_t>(rem, seg - h->fill);
    memcpy(h->h_seg[h->cur] + h->fill, seq + pos, take);
    h->fill += take;
    if (take == rem) {
      if (h->fill < seg) h->h_seg[h->cur][h->fill++] = SK_SEPARATOR;
      if (h->fill == seg)
        if (int st = sk_scan_segment(h)) return st;
      return KU_OK;
    }
    if (int st = sk_scan_segment(h)) return st;
    pos += take - (k - 1);
  }
}

extern "C" int ku_sketch_add_values(ku_sketch *h, const uint64_t *values, uint64_t n) {
  if (!h || (n && !values)) return fail(KU_EINVAL, "ku_sketch_add_values: null argument");
  if (h->failed) return fail(KU_EINVAL, "ku_sketch_add_values: an earlier call on this handle failed");
  if (h->n_groups != 1) return fail(KU_EINVAL, "ku_sketch_add_values: one group only (a value has no bin key)");
  SK_HIP(hipSetDevice(h->device));
  if (int st = sk_scan_segment(h)) return st;  // the values travel through the staging segments too
  const uint64_t per_seg = h->seg_bytes / 8;
  for (uint64_t at = 0; at < n;) {
    if (int st = sk_segment_ready(h)) return st;
    const int c = h->cur;
    const uint64_t take = std::min<uint64_t>(per_seg, n - at);
    memcpy(h->h_seg[c], values + at, take * 8);
    SK_HIP(hipMemcpyAsync(h->d_seg[c], h->h_seg[c], take * 8, hipMemcpyHostToDevice, h->stream));
    const unsigned grid = (unsigned)std::min<uint64_t>((take + KU_SKETCH_BLOCK - 1) / KU_SKETCH_BLOCK, 2048);
    hipLaunchKernelGGL(kmersketch_values_kernel, dim3(grid), dim3(KU_SKETCH_BLOCK), 0, h->stream,
                       reinterpret_cast<const uint64_t *>(h->d_seg[c]), take, h->p, h->d_reg);
    SK_HIP(hipGetLastError());
    SK_HIP(hipEventRecord(h->done[c], h->stream));
    h->in_flight[c] = true;
    h->cur = c ^ 1;
    h->values_observed += take;
    at += take;
  }
  return KU_OK;
}

extern "C" int ku_sketch_export(ku_sketch *h, uint8_t *registers, uint64_t *n_observed) {
  if (!h) return fail(KU_EINVAL, "ku_sketch_export: null argument");
  if (h->failed) return fail(KU_EINVAL, "ku_sketch_export: an earlier call on this handle failed");
  SK_HIP(hipSetDevice(h->device));
  if (int st = sk_scan_segment(h)) return st;  // what is staged
  unsigned long long obs = 0;
  if (registers) SK_HIP(hipMemcpyAsync(registers, h->d_reg, (size_t)h->n_groups << h->p, hipMemcpyDeviceToHost, h->stream));
  SK_HIP(hipMemcpyAsync(&obs, h->d_obs, 8, hipMemcpyDeviceToHost, h->stream));
  SK_HIP(hipStreamSynchronize(h->stream));
  if (n_observed) *n_observed = obs + h->values_observed;
  return KU_OK;
}

extern "C" int ku_sketch_estimate(ku_sketch *h, uint64_t *estimate) {
  if (!h || !estimate) return fail(KU_EINVAL, "ku_sketch_estimate: null argument");
  if (h->n_groups != 1) return fail(KU_EINVAL, "ku_sketch_estimate: one group only (ku_sketch_export gives every group's registers)");
  std::vector<uint8_t> regs((size_t)1 << h->p);
  uint64_t obs = 0;
  if (int st = ku_sketch_export(h, regs.data(), &obs)) return st;
  *estimate = ku_hll_cardinality(regs.data(), h->p, obs);  // min(n_observed, Ertl): what the reference's count_unique prints
  return KU_OK;
}
