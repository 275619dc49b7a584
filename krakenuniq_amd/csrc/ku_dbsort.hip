// ku_dbsort.hip -- db_sort on the GPU: a Jellyfish-format k-mer list -> database.kdb + database.idx.
//
// The reference (src/db_sort.cpp:34-128 + KrakenDB::make_index, src/krakendb.cpp:118-148) counts the records per
// minimizer bin, scatters them into their bins and qsort()s every bin by k-mer.  Here the same order -- ascending
// (bin key, k-mer) -- comes from two stable LSD radix sorts on the device (rocPRIM: by k-mer, then by bin key), the
// index from a histogram of the bin keys + an exclusive scan.  Offline tool, not on the classify hot path.
//
// ku_kmerdb_* (ku_kmerdb.hip) builds the same two files straight from the library's sequences: it collects the distinct
// canonical k-mers on the device and hands them, sorted by k-mer, to the second half here (dbsort_bin_order_and_pack).
#include <cstring>  // (rocPRIM uses memset without including it)

#include <rocprim/rocprim.hpp>

#include "ku_build.h"

namespace {

const KuHipWho DS{"db_sort: ", "", nullptr};

struct Rec {  // what travels through the second sort
  uint64_t kmer;
  uint32_t val;
  uint32_t pad;
};

// records in their on-disk form -> k-mer keys and values
__global__ void dbsort_unpack_kernel(const uint8_t *__restrict__ raw, uint64_t n, uint32_t key_len, uint64_t *kmers,
                                     uint32_t *vals, int zero_vals) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t kmer;
    uint32_t v;
    ku_rec_load(raw, i, key_len, kmer, v);
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

// sorted records -> the on-disk form
__global__ void dbsort_pack_kernel(const Rec *__restrict__ recs, uint64_t n, uint32_t key_len, uint8_t *raw) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const Rec r = recs[i];
    ku_rec_store(raw, i, key_len, r.kmer, r.val);
  }
}

// scratch of one rocPRIM call (ku_rocprim): allocated from `dev`, left in d_tmp for the caller to release
auto ds_scratch(Dev &dev, void *&d_tmp) {
  return [&dev, &d_tmp](size_t tmp_bytes, void *&tmp, size_t &have) -> int {
    KU_HIP(DS, dev.alloc(&d_tmp, tmp_bytes));
    tmp = d_tmp;
    have = tmp_bytes;
    return KU_OK;
  };
}

}  // namespace

// the first step of db_sort and of ku_setlcas_open (ku_build.h)
int dbsort_unpack(const KuHipWho &who, hipStream_t s, const uint8_t *d_raw, uint64_t n, uint32_t key_len, uint64_t *d_kmer,
                  uint32_t *d_val, bool zero_vals) {
  hipLaunchKernelGGL(dbsort_unpack_kernel, dim3(ku_grid_256(n)), dim3(256), 0, s, d_raw, n, key_len, d_kmer, d_val, (int)zero_vals);
  KU_HIP(who, hipGetLastError());
  return KU_OK;
}

// the second half of db_sort (ku_build.h says what goes in and what comes out)
int dbsort_bin_order_and_pack(Dev &dev, hipStream_t s, uint64_t *d_kmer, uint32_t *d_val, bool release_inputs, uint64_t n,
                              uint32_t k, uint32_t nt, uint32_t key_len, uint32_t bin_lo, uint64_t n_hist, uint64_t first_off,
                              uint8_t **d_raw, uint64_t **d_off) {
  const uint32_t xor_mask = ku_index2_xor_mask(nt);
  const unsigned grid = ku_grid_256(n);
  uint32_t *d_bin_a = nullptr, *d_bin_b = nullptr;
  Rec *d_rec_a = nullptr, *d_rec_b = nullptr;
  unsigned long long *d_hist = nullptr;
  void *d_tmp = nullptr;
  // bin keys + histogram
  KU_HIP(DS, dev.alloc(&d_bin_a, n * 4));
  KU_HIP(DS, dev.alloc(&d_bin_b, n * 4));
  KU_HIP(DS, dev.alloc(&d_rec_a, n * sizeof(Rec)));
  KU_HIP(DS, dev.alloc(&d_hist, n_hist * 8));
  KU_HIP(DS, hipMemsetAsync(d_hist, 0, n_hist * 8, s));
  hipLaunchKernelGGL(dbsort_binkey_kernel, dim3(grid), dim3(256), 0, s, d_kmer, d_val, n, k, nt, xor_mask, bin_lo, d_bin_a,
                     d_rec_a, d_hist);
  KU_HIP(DS, hipGetLastError());
  KU_HIP(DS, hipStreamSynchronize(s));
  if (release_inputs) { dev.release(d_kmer); dev.release(d_val); }
  // stable by bin key (2 nt bits) -> (bin, k-mer) order
  KU_HIP(DS, dev.alloc(&d_rec_b, n * sizeof(Rec)));
  KU_TRY(ku_rocprim(DS, "rocprim::radix_sort_pairs", ds_scratch(dev, d_tmp), [&](void *tmp, size_t &tmp_bytes) {
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, d_bin_a, d_bin_b, d_rec_a, d_rec_b, (size_t)n, 0u, 2u * nt, s);
  }));
  KU_HIP(DS, hipStreamSynchronize(s));
  dev.release(d_tmp); d_tmp = nullptr;
  dev.release(d_rec_a); dev.release(d_bin_a); dev.release(d_bin_b);
  // offsets[b] = number of records in bins < b, offsets past the last bin = all of them (make_index, krakendb.cpp:136-139)
  KU_HIP(DS, dev.alloc(d_off, (n_hist + 1) * 8));
  KU_TRY(ku_rocprim(DS, "rocprim::exclusive_scan", ds_scratch(dev, d_tmp), [&](void *tmp, size_t &tmp_bytes) {
    return rocprim::exclusive_scan(tmp, tmp_bytes, (const uint64_t *)d_hist, *d_off, first_off, (size_t)n_hist,
                                   rocprim::plus<uint64_t>(), s);
  }));
  const uint64_t end_off = first_off + n;
  KU_HIP(DS, hipMemcpyAsync(*d_off + n_hist, &end_off, 8, hipMemcpyHostToDevice, s));
  if (!*d_raw) KU_HIP(DS, dev.alloc(d_raw, n * (key_len + 4)));
  hipLaunchKernelGGL(dbsort_pack_kernel, dim3(grid), dim3(256), 0, s, d_rec_b, n, key_len, *d_raw);
  KU_HIP(DS, hipGetLastError());
  KU_HIP(DS, hipStreamSynchronize(s));  // (end_off leaves the stack, and d_tmp / d_hist may be freed by the caller's Dev)
  return KU_OK;
}

extern "C" int ku_db_sort_files(int device, const char *in_path, const char *out_kdb_path, const char *out_idx_path,
                                uint32_t nt, int zero_vals) {
  if (!in_path || !out_kdb_path || !out_idx_path) return fail(KU_EINVAL, "ku_db_sort_files: null argument");
  if (nt < 1 || nt > 15) return fail(KU_EINVAL, "bin key length out of range (1..15: 32-bit minimizers, krakendb.cpp:203)");
  KU_TRY(ku_check_device(device));
  KU_HIP(DS, hipSetDevice(device));

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
  KU_HIP(DS, hipStreamCreate(&s));
  StreamGuard sg{s};
  uint8_t *d_raw = nullptr;
  uint64_t *d_kmer_a = nullptr, *d_kmer_b = nullptr, *d_off = nullptr;
  uint32_t *d_val_a = nullptr, *d_val_b = nullptr;
  void *d_tmp = nullptr;
  KU_HIP(DS, dev.alloc(&d_raw, n * ps));
  KU_HIP(DS, dev.alloc(&d_kmer_a, n * 8));
  KU_HIP(DS, dev.alloc(&d_val_a, n * 4));
  if (n) KU_HIP(DS, hipMemcpyAsync(d_raw, in + hdr, n * ps, hipMemcpyHostToDevice, s));
  KU_TRY(dbsort_unpack(DS, s, d_raw, n, key_len, d_kmer_a, d_val_a, zero_vals != 0));
  // pass 1: by k-mer (2k significant bits)
  KU_HIP(DS, dev.alloc(&d_kmer_b, n * 8));
  KU_HIP(DS, dev.alloc(&d_val_b, n * 4));
  KU_TRY(ku_rocprim(DS, "rocprim::radix_sort_pairs", ds_scratch(dev, d_tmp), [&](void *tmp, size_t &tmp_bytes) {
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, d_kmer_a, d_kmer_b, d_val_a, d_val_b, (size_t)n, 0u, (unsigned)key_bits, s);
  }));
  KU_HIP(DS, hipStreamSynchronize(s));
  dev.release(d_tmp); d_tmp = nullptr;
  dev.release(d_kmer_a); dev.release(d_val_a);
  // second half: (bin key, k-mer) order, index offsets, records back in their on-disk form
  {
    const int st = dbsort_bin_order_and_pack(dev, s, d_kmer_b, d_val_b, /*release_inputs=*/true, n, k, nt, key_len, 0u, n_bins,
                                             0, &d_raw, &d_off);
    if (st != KU_OK) return st;
  }

  // ---- outputs: header copied verbatim (src/db_sort.cpp:56-75), then the sorted records; KRAKIX2 index
  // (key_ct at byte 48 is written once more with the value it has; the closing offset is d_off[n_bins])
  KuDbFiles out;
  std::vector<uint8_t> h_buf;
  if (!out.open(out_kdb_path, out_idx_path) || !out.begin(in, hdr, 2, nt)) return fail(KU_ENOINPUT, out.error);
  KU_TRY(ku_append_from_device(DS, out, &KuDbFiles::append_records, d_raw, n * ps, h_buf));
  KU_TRY(ku_append_from_device(DS, out, &KuDbFiles::append_offsets, d_off, n_bins * 8, h_buf));
  if (!out.finish(n)) return fail(KU_ENOINPUT, out.error);
  return KU_OK;
}
