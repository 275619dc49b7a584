// ku_dbmerge.hip -- db_merge on the GPU: the union of 2..8 sorted databases (database.kdb + database.idx each) as one sorted
// database, the values of a k-mer that several inputs hold folded with lca().
//
// Every input is in (minimizer bin, k-mer) order (src/db_sort.cpp:34-128) and its index says where each bin starts, so the
// union is a merge by rank, not a sort, and no bin key is computed here.  With a taxonomy the value of a shared k-mer is
// lca(Parent_map, vA, vB) (krakenutil.cpp:90-118) in node space as in ku_setlcas.hip; lca() is associative and commutative
// with lca(0, x) = x, so merging databases that set_lcas built apart gives what set_lcas (src/set_lcas.cpp:429-476) builds
// over the union of their libraries.  Offline tool, not on the classify hot path.
//
// The run is cut into chunks, contiguous ranges of bins (ku_dbmerge_budget.h has the byte rule), so that databases larger
// than the device stream through.  Inside a chunk the inputs are folded left to right, out = merge(merge(A, B), C); the
// intermediate result and its offsets stay on the device.  One fold step:
//   1. dbmerge_rank_b_kernel   thread per record j of B: its bin by binary search of j in B's offsets, lower bound of its k-mer
//                              in A's slice of that bin -> rankA[j], dup[j]
//   2. rocPRIM exclusive scan  dup -> dupsBefore[0 .. nB]
//   3. dbmerge_scatter_b_kernel  records of B that A does not hold -> out[rankA[j] + j - dupsBefore[j]]
//   4. dbmerge_scatter_a_kernel  thread per record i of A: lower bound in B's slice of the bin -> rankB; the value folded where
//                              B[rankB] is the same k-mer; -> out[i + rankB - dupsBefore[rankB]]
//   5. dbmerge_offsets_kernel  offOut[b] = first + (offA[b] - baseA) + (offB[b] - baseB) - dupsBefore[offB[b] - baseB]
// Records are read and written in their on-disk form (key_len + 4 bytes; three dwords at key_len 8); all record indices are
// 64 bits wide.  Both scatters keep record order on each side, so neighbouring threads store to ascending addresses.
#include <cstring>  // (rocPRIM uses memset without including it)

#include <rocprim/rocprim.hpp>

#include "ku_build.h"
#include "ku_dbmerge_budget.h"

namespace {

const KuHipWho DM{"db_merge: ", " -- db_merge: use a smaller budget (-s)", nullptr};

constexpr uint32_t MG_ERR_VALUES = 1u;  // two different non-zero values of one k-mer, and no taxonomy to fold them
constexpr uint32_t MG_ERR_INDEX = 2u;   // offsets that do not ascend or leave the slice

// one side of a fold step: n records of the chunk in their on-disk form, and the offsets of the chunk's bins (nb + 1
// entries; off[b] - base = index of the first record of bin b within `raw`)
struct MgSide {
  const uint8_t *raw;
  const uint64_t *off;
  uint64_t base, n;
};

// the fold of two values, and what it needs
struct MgFold {
  const uint32_t *parent;      // node -> parent node (0 = none), or null: no taxonomy
  const uint32_t *node_taxid;  // sorted node universe
  uint32_t n_nodes;
};

// the bin of record j (j < s.n, nb >= 1): the b with off[b] <= base + j < off[b + 1]
__device__ __forceinline__ uint64_t mg_bin_of(const MgSide &s, uint64_t nb, uint64_t j) {
  const uint64_t t = s.base + j;
  uint64_t lo = 0, hi = nb;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (s.off[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}
// the records of bin b, as indices into s.raw: clamped to the slice whatever the index says, and the index reported
__device__ __forceinline__ void mg_slice(const MgSide &s, uint64_t b, uint64_t &lo, uint64_t &hi, uint32_t *err) {
  const uint64_t o0 = s.off[b], o1 = s.off[b + 1];
  const bool bad = o0 < s.base || o1 < o0 || o1 - s.base > s.n;
  if (bad) atomicOr(err, MG_ERR_INDEX);
  lo = bad ? 0 : o0 - s.base;
  hi = bad ? 0 : o1 - s.base;
}
__device__ __forceinline__ uint64_t mg_lower_bound(const uint8_t *__restrict__ raw, uint64_t lo, uint64_t hi, uint64_t key,
                                                   uint32_t key_len) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (ku_rec_key(raw, mid, key_len) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// (the node universe holds every value of every input: the clamp is never taken)
__device__ __forceinline__ uint32_t mg_node_of(const MgFold &f, uint32_t taxid) {
  const uint32_t node = ku_node_of(f.node_taxid, f.n_nodes, taxid);
  return node < f.n_nodes ? node : 0;
}

// step 1: B's records ranked in A
__global__ void dbmerge_rank_b_kernel(MgSide A, MgSide B, uint64_t nb, uint32_t key_len, uint64_t *__restrict__ rank,
                                      uint8_t *__restrict__ dup, uint32_t *err) {
  const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (first == 0) dup[B.n] = 0;  // the scan's closing entry: dupsBefore[nB] = all duplicates
  for (uint64_t j = first; j < B.n; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t b = mg_bin_of(B, nb, j);
    uint64_t lo, hi;
    mg_slice(A, b, lo, hi, err);
    const uint64_t key = ku_rec_key(B.raw, j, key_len);
    const uint64_t at = mg_lower_bound(A.raw, lo, hi, key, key_len);
    rank[j] = at;
    dup[j] = at < hi && ku_rec_key(A.raw, at, key_len) == key;
  }
}

// step 3: B's records that A does not hold
__global__ void dbmerge_scatter_b_kernel(MgSide B, uint32_t key_len, const uint64_t *__restrict__ rank, const uint8_t *__restrict__ dup,
                                         const uint64_t *__restrict__ dups_before, uint8_t *out, uint64_t out_cap) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < B.n; j += (uint64_t)gridDim.x * blockDim.x) {
    if (dup[j]) continue;
    uint64_t key;
    uint32_t val;
    ku_rec_load(B.raw, j, key_len, key, val);
    const uint64_t at = rank[j] + j - dups_before[j];
    if (at < out_cap) ku_rec_store(out, at, key_len, key, val);
  }
}

// step 4: A's records, the values of the shared k-mers folded
__global__ void dbmerge_scatter_a_kernel(MgSide A, MgSide B, uint64_t nb, uint32_t key_len, const uint64_t *__restrict__ dups_before,
                                         MgFold f, uint8_t *out, uint64_t out_cap, uint32_t *err, unsigned long long *folded) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t b = mg_bin_of(A, nb, i);
    uint64_t lo, hi;
    mg_slice(B, b, lo, hi, err);
    uint64_t key;
    uint32_t val;
    ku_rec_load(A.raw, i, key_len, key, val);
    const uint64_t at = mg_lower_bound(B.raw, lo, hi, key, key_len);
    if (at < hi) {
      uint64_t key_b;
      uint32_t val_b;
      ku_rec_load(B.raw, at, key_len, key_b, val_b);
      if (key_b == key && val_b != val) {
        if (val == 0 || val_b == 0) val |= val_b;  // lca(0, x) = x
        else {
          atomicAdd(folded, 1ull);
          if (f.parent) val = f.node_taxid[ku_lca_nodes(f.parent, mg_node_of(f, val), mg_node_of(f, val_b))];
          else atomicOr(err, MG_ERR_VALUES);
        }
      }
    }
    const uint64_t to = i + at - dups_before[at];
    if (to < out_cap) ku_rec_store(out, to, key_len, key, val);
  }
}

// step 5: the result's offsets, nb + 1 of them
__global__ void dbmerge_offsets_kernel(MgSide A, MgSide B, uint64_t nb, const uint64_t *__restrict__ dups_before, uint64_t first,
                                       uint64_t *__restrict__ off_out) {
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b <= nb; b += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t a = A.off[b] - A.base, at = B.off[b] - B.base;
    off_out[b] = first + a + at - dups_before[at < B.n ? at : B.n];
  }
}

struct MgWiden {
  __device__ uint64_t operator()(uint8_t x) const { return x; }
};

// the inputs of a run, closed on every exit path
struct MgInputs {
  std::vector<ku_db *> dbs;
  ~MgInputs() {
    for (ku_db *db : dbs) ku_db_close(db);
  }
};

bool mg_same_file(const struct stat &a, const struct stat &b) { return a.st_dev == b.st_dev && a.st_ino == b.st_ino; }

}  // namespace

// The union of sorted databases (the order db_sort gives them, src/db_sort.cpp:34-128), values folded as set_lcas folds
// them (src/set_lcas.cpp:429-476).  include/krakenuniq_amd.h says what is checked and in which order.
extern "C" int ku_db_merge_files(int device, const char *const *kdb_paths, const char *const *idx_paths, uint32_t n_inputs,
                                 const ku_tax *tax, uint64_t device_bytes, const char *out_kdb_path, const char *out_idx_path,
                                 ku_db_merge_stats *stats) {
  if (!kdb_paths || !idx_paths || !out_kdb_path || !out_idx_path) return fail(KU_EINVAL, "ku_db_merge_files: null argument");
  if (n_inputs < 2 || n_inputs > 8) return fail(KU_EINVAL, "ku_db_merge_files: the number of inputs must lie in 2..8");
  for (uint32_t i = 0; i < n_inputs; ++i)
    if (!kdb_paths[i] || !idx_paths[i]) return fail(KU_EINVAL, "ku_db_merge_files: null argument");
  if (device_bytes && device_bytes < KU_DBMERGE_MIN_BYTES) return fail(KU_EINVAL, "db_merge: the device budget is below the minimum of 64 KiB");
  if (stats) *stats = ku_db_merge_stats{};

  // ---- inputs: the host view of ku_db_open; they have to agree in what decides the order and the record layout
  MgInputs in;
  std::vector<ku_db_info> info(n_inputs);
  for (uint32_t i = 0; i < n_inputs; ++i) {
    ku_db *db = nullptr;
    KU_TRY(ku_db_open(kdb_paths[i], idx_paths[i], &db));
    in.dbs.push_back(db);
    info[i] = db->info;
    if (info[i].k != info[0].k || info[i].key_len != info[0].key_len || info[i].nt != info[0].nt || info[i].idx_type != info[0].idx_type)
      return fail(KU_EINVAL, std::string("db_merge: ") + kdb_paths[0] + " (k " + std::to_string(info[0].k) + ", minimizer length " +
                                 std::to_string(info[0].nt) + ", index type " + std::to_string(info[0].idx_type) + ") and " + kdb_paths[i] +
                                 " (k " + std::to_string(info[i].k) + ", minimizer length " + std::to_string(info[i].nt) + ", index type " +
                                 std::to_string(info[i].idx_type) + ") differ: db_sort -n re-indexes a database");
  }
  {
    struct stat so[2], si;
    const char *outs[2] = {out_kdb_path, out_idx_path};
    bool have[2];
    for (int o = 0; o < 2; ++o) have[o] = ::stat(outs[o], &so[o]) == 0;
    if (have[0] && have[1] && mg_same_file(so[0], so[1])) return fail(KU_EINVAL, "db_merge: the two outputs are the same file");
    for (uint32_t i = 0; i < n_inputs; ++i)
      for (const char *path : {kdb_paths[i], idx_paths[i]})
        for (int o = 0; o < 2; ++o)
          if (have[o] && ::stat(path, &si) == 0 && mg_same_file(so[o], si))
            return fail(KU_EINVAL, std::string("db_merge: the output ") + outs[o] + " is the input " + path);
  }
  const uint32_t key_len = info[0].key_len;
  const uint64_t ps = key_len + 4, n_bins = info[0].n_bins;

  KU_TRY(ku_check_device(device));
  KU_HIP(DM, hipSetDevice(device));
  KU_TRY(ku_default_budget(DM, KU_DBMERGE_MIN_BYTES, &device_bytes));
  const KuDbMergeBudget budget = ku_dbmerge_budget(device_bytes);

  // ---- chunk plan: from `lo`, the longest range of bins that holds at most `capacity` records of all inputs together and
  // spans at most `max_bins` bins (both grow with the end of the range: binary search)
  std::vector<const uint64_t *> off(n_inputs);
  for (uint32_t i = 0; i < n_inputs; ++i) off[i] = in.dbs[i]->offsets;
  auto records_in = [&](uint64_t lo, uint64_t hi, bool &ok) {
    uint64_t r = 0;
    for (uint32_t i = 0; i < n_inputs; ++i) {
      if (off[i][hi] < off[i][lo] || off[i][hi] > info[i].key_ct) { ok = false; return (uint64_t)0; }
      r += off[i][hi] - off[i][lo];
    }
    return r;
  };
  std::vector<uint64_t> bounds{0};
  uint64_t max_records = 0, max_span = 0;
  for (uint64_t lo = 0; lo < n_bins;) {
    bool ok = true;
    uint64_t good = lo, bad = std::min(n_bins, lo + budget.max_bins) + 1;  // records_in(lo, good) fits, (lo, bad) does not
    while (bad - good > 1) {
      const uint64_t mid = good + (bad - good) / 2;
      if (records_in(lo, mid, ok) <= budget.capacity && ok) good = mid; else bad = mid;
      if (!ok) return fail(KU_EDATA, "db_merge: the offsets of an input's index do not ascend");
    }
    if (good == lo)
      return fail(KU_ENOMEM, "db_merge: minimizer bin " + std::to_string(lo) + " holds " + std::to_string(records_in(lo, lo + 1, ok)) +
                                 " records, more than the " + std::to_string(budget.capacity) + " a chunk may hold under the device budget: use a larger budget (-s)");
    max_records = std::max(max_records, records_in(lo, good, ok));
    max_span = std::max(max_span, good - lo);
    bounds.push_back(good);
    lo = good;
  }

  // ---- taxonomy: the node table over the values of every input
  KuNodeTable nodes;
  if (tax) KU_TRY(nodes.build(tax, {in.dbs.begin(), in.dbs.end()}));

  // ---- device: buffers for the largest chunk of the plan (never more than the budget's capacity)
  Dev dev;
  hipStream_t s = nullptr;
  KU_HIP(DM, hipStreamCreate(&s));
  StreamGuard sg{s};
  uint8_t *d_acc = nullptr, *d_in = nullptr, *d_out = nullptr, *d_dup = nullptr;
  uint64_t *d_off_acc = nullptr, *d_off_in = nullptr, *d_off_out = nullptr, *d_rank = nullptr, *d_before = nullptr;
  uint32_t *d_parent = nullptr, *d_node_taxid = nullptr;
  unsigned long long *d_ctl = nullptr;  // [0] error bits, [1] folded
  KuScratch tmp;
  KU_HIP(DM, dev.alloc(&d_acc, max_records * ps));
  KU_HIP(DM, dev.alloc(&d_in, max_records * ps));
  KU_HIP(DM, dev.alloc(&d_out, max_records * ps));
  KU_HIP(DM, dev.alloc(&d_rank, max_records * 8));
  KU_HIP(DM, dev.alloc(&d_before, (max_records + 1) * 8));
  KU_HIP(DM, dev.alloc(&d_dup, max_records + 1));
  KU_HIP(DM, dev.alloc(&d_off_acc, (max_span + 1) * 8));
  KU_HIP(DM, dev.alloc(&d_off_in, (max_span + 1) * 8));
  KU_HIP(DM, dev.alloc(&d_off_out, (max_span + 1) * 8));
  KU_HIP(DM, dev.alloc(&d_ctl, 16));
  MgFold fold{nullptr, nullptr, 0};
  if (tax) {
    KU_HIP(DM, dev.alloc(&d_parent, nodes.size() * 4));
    KU_HIP(DM, dev.alloc(&d_node_taxid, nodes.size() * 4));
    KU_TRY(nodes.upload(DM, s, d_parent, d_node_taxid));
    fold = MgFold{d_parent, d_node_taxid, nodes.size()};
  }
  auto scratch = tmp.provider(DM, s);

  // ---- outputs: database header of input 0 (its key count is patched at the end), index header as db_sort writes it
  KuDbFiles out;
  if (!out.open(out_kdb_path, out_idx_path) ||
      !out.begin(in.dbs[0]->map_kdb, (size_t)(in.dbs[0]->pairs - (const uint8_t *)in.dbs[0]->map_kdb), info[0].idx_type, info[0].nt))
    return fail(KU_ENOINPUT, out.error);

  ku_db_merge_stats st{};
  st.capacity = budget.capacity;
  std::vector<uint8_t> h_buf;
  uint64_t key_ct = 0;
  for (size_t c = 0; c + 1 < bounds.size(); ++c) {
    const uint64_t lo = bounds[c], nb = bounds[c + 1] - lo;
    double t0 = ku_now();
    KU_HIP(DM, hipMemsetAsync(d_ctl, 0, 16, s));
    // the fold's left side starts as input 0's slice
    MgSide A{d_acc, d_off_acc, off[0][lo], off[0][lo + nb] - off[0][lo]};
    if (A.n) KU_HIP(DM, hipMemcpyAsync(d_acc, in.dbs[0]->pairs + A.base * ps, A.n * ps, hipMemcpyHostToDevice, s));
    KU_HIP(DM, hipMemcpyAsync(d_off_acc, off[0] + lo, (nb + 1) * 8, hipMemcpyHostToDevice, s));
    uint8_t *d_res = d_out, *d_left = d_acc;
    uint64_t *d_off_res = d_off_out, *d_off_left = d_off_acc;
    for (uint32_t i = 1; i < n_inputs; ++i) {
      MgSide B{d_in, d_off_in, off[i][lo], off[i][lo + nb] - off[i][lo]};
      if (B.n) KU_HIP(DM, hipMemcpyAsync(d_in, in.dbs[i]->pairs + B.base * ps, B.n * ps, hipMemcpyHostToDevice, s));
      KU_HIP(DM, hipMemcpyAsync(d_off_in, off[i] + lo, (nb + 1) * 8, hipMemcpyHostToDevice, s));
      KU_HIP(DM, hipStreamSynchronize(s));
      st.upload_s += ku_now() - t0;
      t0 = ku_now();
      const uint64_t out_cap = A.n + B.n;  // <= max_records: the chunk's records of the inputs 0 .. i
      hipLaunchKernelGGL(dbmerge_rank_b_kernel, dim3(ku_grid_256(B.n)), dim3(256), 0, s, A, B, nb, key_len, d_rank, d_dup,
                         reinterpret_cast<uint32_t *>(d_ctl));
      KU_HIP(DM, hipGetLastError());
      KU_TRY(ku_rocprim(DM, "rocprim::exclusive_scan", scratch, [&](void *tmp, size_t &tmp_bytes) {
        return rocprim::exclusive_scan(tmp, tmp_bytes, rocprim::make_transform_iterator((const uint8_t *)d_dup, MgWiden()), d_before,
                                       (uint64_t)0, (size_t)(B.n + 1), rocprim::plus<uint64_t>(), s);
      }));
      hipLaunchKernelGGL(dbmerge_scatter_b_kernel, dim3(ku_grid_256(B.n)), dim3(256), 0, s, B, key_len, d_rank, d_dup, d_before, d_res,
                         out_cap);
      hipLaunchKernelGGL(dbmerge_scatter_a_kernel, dim3(ku_grid_256(A.n)), dim3(256), 0, s, A, B, nb, key_len, d_before, fold, d_res,
                         out_cap, reinterpret_cast<uint32_t *>(d_ctl), d_ctl + 1);
      // the last step's offsets are the file's: they start at the records written so far
      hipLaunchKernelGGL(dbmerge_offsets_kernel, dim3(ku_grid_256(nb + 1)), dim3(256), 0, s, A, B, nb, d_before,
                         i + 1 == n_inputs ? key_ct : (uint64_t)0, d_off_res);
      KU_HIP(DM, hipGetLastError());
      uint64_t dups = 0;
      KU_HIP(DM, hipMemcpyAsync(&dups, d_before + B.n, 8, hipMemcpyDeviceToHost, s));
      KU_HIP(DM, hipStreamSynchronize(s));
      st.merge_s += ku_now() - t0;
      t0 = ku_now();
      st.duplicates += dups;
      // the result is the next step's left side
      A = MgSide{d_res, d_off_res, 0, out_cap - dups};
      std::swap(d_res, d_left);
      std::swap(d_off_res, d_off_left);
    }
    unsigned long long ctl[2] = {0, 0};
    KU_HIP(DM, hipMemcpy(ctl, d_ctl, 16, hipMemcpyDeviceToHost));
    if ((uint32_t)ctl[0] & MG_ERR_INDEX) return fail(KU_EDATA, "db_merge: the offsets of an input's index do not ascend");
    if ((uint32_t)ctl[0] & MG_ERR_VALUES)
      return fail(KU_EDATA, "db_merge: values differ for a k-mer present in both inputs; a taxonomy is needed to fold them");
    st.folded += ctl[1];
    // the chunk's records behind those of the chunks before, the offsets of its bins (the closing one: below)
    KU_TRY(ku_append_from_device(DM, out, &KuDbFiles::append_records, A.raw, A.n * ps, h_buf));
    KU_TRY(ku_append_from_device(DM, out, &KuDbFiles::append_offsets, A.off, nb * 8, h_buf));
    key_ct += A.n;
    st.chunks++;
    st.write_s += ku_now() - t0;
  }
  const double t0 = ku_now();
  if (!out.finish(key_ct)) return fail(KU_ENOINPUT, out.error);
  st.write_s += ku_now() - t0;
  st.key_ct = key_ct;
  if (stats) *stats = st;
  return KU_OK;
}
