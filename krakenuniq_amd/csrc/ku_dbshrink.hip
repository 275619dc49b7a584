// ku_dbshrink.hip -- db_shrink on the GPU (src/db_shrink.cpp): n_out of the key_ct records of a Jellyfish-1 list, evenly
// spread and in the input's order -- as a list, byte for byte the reference's, or, from a sorted database.kdb and its KRAKIX2
// index, as a sorted database with its index, byte for byte what the reference's db_shrink + db_sort -n nt write.
//
// The selection keeps the order, so a sorted database stays in (minimizer bin key, k-mer) order and the new index is the
// old one seen through S: no bin key is computed and nothing is sorted.  ku_dbshrink_rule.h has the arithmetic (src, S),
// ku_dbshrink_budget.h the budget rule and the chunk plan, include/krakenuniq_amd.h what is checked and in which order.
// Offline tool, not on the classify hot path.
//   dbshrink_select_kernel   thread per output record j of the chunk [lo, hi): record src(j) - lo of the chunk -> place
//                            j - S(lo) of the compact buffer; records in their on-disk form (key_len + 4 bytes; three dwords
//                            at key_len 8, byte by byte otherwise), neighbouring threads store to ascending addresses
//   dbshrink_offsets_kernel  thread per offset of the slice: off[i] = S(off[i]), in place
#include "ku_build.h"
#include "ku_dbshrink_budget.h"
#include "ku_dbshrink_rule.h"

namespace {

const KuHipWho SH{"db_shrink: ", " -- db_shrink: use a smaller budget (-s)", nullptr};

constexpr uint32_t SH_ERR_SELECT = 1u;  // src(j) outside the chunk (a host-side accounting bug): nothing is copied
constexpr uint32_t SH_ERR_INDEX = 2u;   // an offset above key_ct

// the chunk holds the input records [lo, hi); out takes the output records [j_lo, j_hi) = [S(lo), S(hi))
__global__ void dbshrink_select_kernel(KuShrinkRule r, const uint8_t *__restrict__ chunk, uint64_t lo, uint64_t hi, uint64_t j_lo,
                                       uint64_t j_hi, uint32_t key_len, uint8_t *__restrict__ out, uint32_t *err) {
  const uint64_t n = j_hi - j_lo;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t src = ku_shrink_src(r, j_lo + i);
    if (src < lo || src >= hi) {
      atomicOr(err, SH_ERR_SELECT);
      continue;
    }
    uint64_t key;
    uint32_t val;
    ku_rec_load(chunk, src - lo, key_len, key, val);
    ku_rec_store(out, i, key_len, key, val);
  }
}

__global__ void dbshrink_offsets_kernel(KuShrinkRule r, uint64_t *__restrict__ off, uint64_t n, uint32_t *err) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t x = off[i];
    if (x > r.key_ct) {
      atomicOr(err, SH_ERR_INDEX);
      x = r.key_ct;
    }
    off[i] = ku_shrink_S(r, x);
  }
}

// a file mapped for reading, unmapped on every exit path
struct ShMap {
  const uint8_t *p = nullptr;
  size_t n = 0;
  struct stat st {};
  ~ShMap() {
    if (p) munmap((void *)p, n);
  }
  int open(const char *path) {
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return fail(KU_ENOINPUT, std::string("can't open ") + path);
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
      ::close(fd);
      return fail(KU_ENOINPUT, std::string("can't read ") + path);
    }
    n = (size_t)st.st_size;
    if (n) {
      void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m == MAP_FAILED) {
        ::close(fd);
        n = 0;
        return fail(KU_ENOINPUT, std::string("can't map ") + path);
      }
      p = (const uint8_t *)m;
    }
    ::close(fd);
    return KU_OK;
  }
};

bool sh_same_file(const struct stat &a, const struct stat &b) { return a.st_dev == b.st_dev && a.st_ino == b.st_ino; }

}  // namespace

extern "C" int ku_db_shrink_files(int device, const char *in_kdb_path, const char *in_idx_path, uint64_t n_out, uint64_t offset,
                                  uint64_t device_bytes, const char *out_kdb_path, const char *out_idx_path,
                                  ku_db_shrink_stats *stats) {
  if (!in_kdb_path || !out_kdb_path) return fail(KU_EINVAL, "ku_db_shrink_files: null argument");
  if ((in_idx_path != nullptr) != (out_idx_path != nullptr))
    return fail(KU_EINVAL, "db_shrink: the input index and the output index go together (database mode), or neither is given (list mode)");
  if (out_idx_path && strcmp(out_kdb_path, out_idx_path) == 0) return fail(KU_EINVAL, "db_shrink: the two outputs are the same file");
  if (n_out == 0) return fail(KU_EINVAL, "db_shrink: output count must be positive");
  if (offset == 0) return fail(KU_EINVAL, "db_shrink: offset must be positive");
  if (device_bytes && device_bytes < KU_DBSHRINK_MIN_BYTES) return fail(KU_EINVAL, "db_shrink: the device budget is below the minimum of 64 KiB");
  if (stats) *stats = ku_db_shrink_stats{};
  const bool with_idx = in_idx_path != nullptr;

  // ---- input: JFLISTDN header (krakendb.cpp:60-78,151-177; src/db_shrink.cpp:45-70) + records
  ShMap kdb, idx;
  KU_TRY(kdb.open(in_kdb_path));
  if (kdb.n < 72 || memcmp(kdb.p, "JFLISTDN", 8) != 0) return fail(KU_EDATA, "db_shrink: input file not Jellyfish v1 database");
  uint64_t key_bits, val_len, key_ct;
  memcpy(&key_bits, kdb.p + 8, 8);
  memcpy(&val_len, kdb.p + 16, 8);
  memcpy(&key_ct, kdb.p + 48, 8);
  if (val_len != 4) return fail(KU_EDATA, "db_shrink: can only handle 4 byte DB values");
  if (key_bits == 0 || key_bits > 62 || (key_bits & 1)) return fail(KU_EDATA, "db_shrink: unsupported key_bits");
  const uint32_t key_len = (uint32_t)((key_bits + 7) / 8);
  const size_t hdr = 72 + 2 * (4 + 8 * key_bits), ps = key_len + 4;
  if (kdb.n < hdr || key_ct > (kdb.n - hdr) / ps)
    return fail(KU_EDATA, std::string("db_shrink: ") + in_kdb_path + " is truncated: its header counts " + std::to_string(key_ct) + " records");
  if (n_out > key_ct)
    return fail(KU_EDATA, "db_shrink: requested new key count " + std::to_string(n_out) + " larger than old key count " + std::to_string(key_ct));
  if (offset > key_ct / n_out)
    return fail(KU_EDATA, "db_shrink: offset " + std::to_string(offset) + " larger than block size " + std::to_string(key_ct / n_out));
  const KuShrinkRule rule = ku_shrink_rule(key_ct, n_out, offset);
  const uint8_t *records = kdb.p + hdr;

  // ---- the index of a sorted database: "KRAKIX2", nt, 4^nt + 1 offsets, the closing one = key_ct
  uint32_t nt = 0;
  uint64_t n_bins = 0;
  const uint64_t *offsets = nullptr;
  if (with_idx) {
    KU_TRY(idx.open(in_idx_path));
    if (idx.n >= 7 && memcmp(idx.p, "KRAKIDX", 7) == 0)
      return fail(KU_EINVAL, std::string("db_shrink: ") + in_idx_path + " is a KRAKIDX (type 1) index, whose bins are not those of a sorted "
                                 "database: db_sort -n re-indexes a database");
    if (idx.n < 8 || memcmp(idx.p, "KRAKIX2", 7) != 0) return fail(KU_EDATA, std::string("db_shrink: ") + in_idx_path + " is not a database index");
    nt = idx.p[7];
    if (nt < 1 || nt > 15 || 2 * nt > key_bits) return fail(KU_EDATA, std::string("db_shrink: ") + in_idx_path + ": minimizer length out of range");
    n_bins = 1ull << (2 * nt);
    if (idx.n != 8 + (n_bins + 1) * 8) return fail(KU_EDATA, std::string("db_shrink: ") + in_idx_path + " has not the size of an index of 4^nt bins");
    offsets = (const uint64_t *)(idx.p + 8);
    if (offsets[n_bins] != key_ct)
      return fail(KU_EDATA, std::string("db_shrink: ") + in_idx_path + " closes at " + std::to_string(offsets[n_bins]) + " records, " + in_kdb_path +
                                " holds " + std::to_string(key_ct) + ": not the index of this database");
  }
  {  // an output that is an input, under whatever name
    const char *outs[2] = {out_kdb_path, out_idx_path};
    struct stat so[2];
    bool have[2] = {false, false};
    for (int o = 0; o < (with_idx ? 2 : 1); ++o) have[o] = ::stat(outs[o], &so[o]) == 0;
    if (have[0] && have[1] && sh_same_file(so[0], so[1])) return fail(KU_EINVAL, "db_shrink: the two outputs are the same file");
    for (int o = 0; o < 2; ++o) {
      if (!have[o]) continue;
      if (sh_same_file(so[o], kdb.st)) return fail(KU_EINVAL, std::string("db_shrink: the output ") + outs[o] + " is the input " + in_kdb_path);
      if (with_idx && sh_same_file(so[o], idx.st)) return fail(KU_EINVAL, std::string("db_shrink: the output ") + outs[o] + " is the input " + in_idx_path);
    }
  }

  // ---- device: buffers for the largest chunk and slice of the plan (never more than the budget's)
  KU_TRY(ku_check_device(device));
  KU_HIP(SH, hipSetDevice(device));
  KU_TRY(ku_default_budget(SH, KU_DBSHRINK_MIN_BYTES, &device_bytes));
  const KuDbShrinkBudget budget = ku_dbshrink_budget(device_bytes);
  const uint64_t n_chunks = ku_dbshrink_chunks(key_ct, budget.chunk_records);
  const uint64_t cap_in = std::min(budget.chunk_records, key_ct), cap_out = std::min(cap_in, n_out);
  const uint64_t cap_off = std::min(budget.offset_slice, n_bins);
  Dev dev;
  hipStream_t s = nullptr;
  KU_HIP(SH, hipStreamCreate(&s));
  StreamGuard sg{s};
  uint8_t *d_in = nullptr, *d_out = nullptr;
  uint64_t *d_off = nullptr;
  uint32_t *d_err = nullptr;
  KU_HIP(SH, dev.alloc(&d_in, cap_in * ps));
  KU_HIP(SH, dev.alloc(&d_out, cap_out * ps));
  KU_HIP(SH, dev.alloc(&d_off, cap_off * 8));
  KU_HIP(SH, dev.alloc(&d_err, 4));
  KU_HIP(SH, hipMemsetAsync(d_err, 0, 4, s));

  // ---- outputs: the input's header (finish() puts n_out at byte 48), the index header as db_sort writes it
  KuDbFiles out;
  if (!(with_idx ? out.open(out_kdb_path, out_idx_path) : out.open(out_kdb_path)) || !out.begin(kdb.p, hdr, 2, nt))
    return fail(KU_ENOINPUT, out.error);

  ku_db_shrink_stats st{};
  st.key_ct_in = key_ct;
  st.key_ct_out = n_out;
  st.block_size = rule.bs;
  st.odd_blocks = rule.odd;
  st.chunks = n_chunks;
  st.chunk_records = budget.chunk_records;
  std::vector<uint8_t> h_buf;
  uint64_t written = 0;
  for (uint64_t c = 0; c < n_chunks; ++c) {
    uint64_t lo, hi;
    ku_dbshrink_chunk(key_ct, budget.chunk_records, c, lo, hi);
    const uint64_t j_lo = ku_shrink_S(rule, lo), j_hi = ku_shrink_S(rule, hi);
    if (j_hi == j_lo) continue;  // nothing of this chunk is kept
    if (j_hi < j_lo || j_hi - j_lo > cap_out || hi - lo > cap_in) return fail(KU_ESTATE, "db_shrink: a chunk does not fit its buffers");
    double t0 = ku_now();
    KU_HIP(SH, hipMemcpyAsync(d_in, records + lo * ps, (hi - lo) * ps, hipMemcpyHostToDevice, s));
    KU_HIP(SH, hipStreamSynchronize(s));
    st.read_s += ku_now() - t0;
    t0 = ku_now();
    hipLaunchKernelGGL(dbshrink_select_kernel, dim3(ku_grid_256(j_hi - j_lo)), dim3(256), 0, s, rule, d_in, lo, hi, j_lo, j_hi, key_len,
                       d_out, d_err);
    KU_HIP(SH, hipGetLastError());
    KU_HIP(SH, hipStreamSynchronize(s));
    st.select_s += ku_now() - t0;
    t0 = ku_now();
    KU_TRY(ku_append_from_device(SH, out, &KuDbFiles::append_records, d_out, (j_hi - j_lo) * ps, h_buf));
    written += j_hi - j_lo;
    st.write_s += ku_now() - t0;
  }
  // the index: new_offsets[b] = S(offsets[b]); the closing offset is finish()'s
  for (uint64_t b = 0; b < n_bins; b += cap_off) {
    const uint64_t nb = std::min(cap_off, n_bins - b);
    double t0 = ku_now();
    KU_HIP(SH, hipMemcpyAsync(d_off, offsets + b, nb * 8, hipMemcpyHostToDevice, s));
    KU_HIP(SH, hipStreamSynchronize(s));
    st.read_s += ku_now() - t0;
    t0 = ku_now();
    hipLaunchKernelGGL(dbshrink_offsets_kernel, dim3(ku_grid_256(nb)), dim3(256), 0, s, rule, d_off, nb, d_err);
    KU_HIP(SH, hipGetLastError());
    KU_HIP(SH, hipStreamSynchronize(s));
    st.select_s += ku_now() - t0;
    t0 = ku_now();
    KU_TRY(ku_append_from_device(SH, out, &KuDbFiles::append_offsets, d_off, nb * 8, h_buf));
    st.write_s += ku_now() - t0;
  }
  uint32_t err = 0;
  KU_HIP(SH, hipMemcpy(&err, d_err, 4, hipMemcpyDeviceToHost));
  if (err & SH_ERR_INDEX) return fail(KU_EDATA, std::string("db_shrink: ") + in_idx_path + " holds an offset above the database's key count");
  if ((err & SH_ERR_SELECT) || written != n_out) return fail(KU_ESTATE, "db_shrink: the chunks did not select the records of the rule");
  const double t0 = ku_now();
  if (!out.finish(n_out)) return fail(KU_ENOINPUT, out.error);
  st.write_s += ku_now() - t0;
  if (stats) *stats = st;
  return KU_OK;
}
