// ku_kmerdb.hip -- ku_kmerdb_*: library sequences -> sorted database.kdb + database.idx (scripts/build_db.sh steps 2-3:
// jellyfish count / merge / dump into database.jdb, then db_sort -z).  With zeroed values both files depend only on the SET
// of canonical k-mers, so no counts are kept: the extraction kernel appends every canonical, unambiguous k-mer of the uploaded
// segment to a device buffer (the step the reference leaves to Jellyfish 1, scripts/build_db.sh:140-146); when the next launch
// might not fit, the candidates are sorted, made unique and merged into the pass's sorted distinct set, which lives at the
// front of the same buffer.  ku_kmerdb_end_pass hands the set to dbsort_bin_order_and_pack (ku_dbsort.hip) and appends its
// records and its part of the index to the files.  (ku_sketch_*, ku_sketch.hip, estimates beforehand how many passes a
// library needs.)  The budget rule is ku_kmerdb_budget (ku_kmerdb_budget.h).  Offline tool, not on the classify hot path.
#include <cstring>  // (rocPRIM uses memset without including it)

#include <rocprim/rocprim.hpp>

#include "ku_build.h"

__global__ __launch_bounds__(64 * KMD_WAVES) void kmerdb_extract_kernel(KmdScan a) {
  __shared__ uint32_t s_code[KMD_WAVES][KMD_CHUNKS];  // 16 bases per word, the first one in bits 31..30
  __shared__ uint32_t s_amb[KMD_WAVES][KMD_CHUNKS];   // 16 ambiguity bits per word, the first base in bit 15
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t t0 = a.w_lo / KMD_TILE, t1 = (a.w_hi + KMD_TILE - 1) / KMD_TILE;
  const uint64_t per_iter = (uint64_t)gridDim.x * KMD_WAVES;
  const uint64_t n_iter = (t1 - t0 + per_iter - 1) / per_iter;  // the same in every block: the barriers below are uniform
  const uint32_t k = a.k;
  for (uint64_t it = 0; it < n_iter; ++it) {
    const uint64_t tile = t0 + (it * gridDim.x + blockIdx.x) * KMD_WAVES + wv;
    const bool live = tile < t1;  // wave-uniform
    if (live) {
      kmd_pack_tile(a.seq, a.seq_bytes, tile, lane, s_code[wv], s_amb[wv]);
    }
    __syncthreads();
    if (live) {
      uint64_t canon[KMD_ROUNDS];
      uint64_t kept[KMD_ROUNDS];  // wave-uniform ballots
      uint32_t total = 0;
#pragma unroll
      for (uint32_t j = 0; j < KMD_ROUNDS; ++j) {
        uint64_t fwd;
        const bool ambiguous = kmd_window(s_code[wv], s_amb[wv], j, lane, k, fwd);
        const uint64_t w = tile * KMD_TILE + j * 64 + lane;
        bool keep = !ambiguous && w >= a.w_lo && w < a.w_hi;
        const uint64_t rc = ku_revcomp64(fwd, k);
        const uint64_t c = fwd < rc ? fwd : rc;
        if (a.pass_mode && keep) {
          const uint32_t bin = ku_bin_key(c, k, a.nt, a.xor_mask);
          keep = bin >= a.bin_lo && bin < a.bin_hi;
        }
        canon[j] = c;
        kept[j] = __ballot(keep);
        total += (uint32_t)__popcll(kept[j]);
      }
      // one reservation per tile; the order inside the buffer is arbitrary, the sort fixes it
      unsigned long long base = 0;
      if (lane == 0 && total) base = atomicAdd(a.cursor, (unsigned long long)total);
      base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
      if (base + total > a.cap) {
        if (lane == 0) atomicOr(a.err, 1u);
      } else {
        const uint64_t below = (1ull << lane) - 1;
#pragma unroll
        for (uint32_t j = 0; j < KMD_ROUNDS; ++j) {
          if ((kept[j] >> lane) & 1ull) a.out[base + (uint32_t)__popcll(kept[j] & below)] = canon[j];
          base += (uint32_t)__popcll(kept[j]);
        }
      }
    }
    __syncthreads();  // the next tile overwrites the packed words
  }
}

struct ku_kmerdb {
  int device = 0;
  uint32_t k = 0, nt = 0, n_passes = 0, key_len = 0;
  uint32_t pass = 0;  // passes ended
  bool finished = false, failed = false;
  uint64_t n_bins = 0, cap = 0, usable = 0, seg_bytes = 0;  // cap, usable, seg_bytes: ku_kmerdb_budget
  KuDbFiles out;  // removed by its destructor unless ku_kmerdb_finish got to its end
  hipStream_t stream = nullptr;
  uint64_t *d_a = nullptr, *d_b = nullptr;  // d_a: the distinct set [0, n_set), then the candidates [n_set, fill)
  uint8_t *d_seq = nullptr;
  unsigned long long *d_ctl = nullptr;      // [0] the buffer's cursor, [1] rocPRIM's unique count, [2] the kernel's error word
  KuScratch tmp;  // rocPRIM's
  uint64_t n_set = 0, fill = 0, key_ct = 0;
  uint64_t merge_piece = 0;  // keys of either input per rocprim::merge call (kmd_merge)
  uint64_t merge_calls = 0;  // of the running pass
  uint64_t windows = 0, candidates = 0, flushes = 0, segments = 0;  // of the running pass
  ku_kmerdb_stats stats{};
  std::vector<uint8_t> h_buf;
};

namespace {

KuHipWho KMD(ku_kmerdb *h) { return {"kmer_db: ", " (a smaller -s, or more passes: -P)", &h->failed}; }

int kmd_fail(ku_kmerdb *h, int code, const std::string &msg) {
  h->failed = true;
  return fail(code, msg);
}

// bins of pass p: [p * 4^nt / n_passes, (p + 1) * 4^nt / n_passes)
uint64_t kmd_pass_bound(const ku_kmerdb *h, uint32_t p) { return (uint64_t)p * h->n_bins / h->n_passes; }

}  // namespace

// rocPRIM's scratch (ku_rocprim): the handle's buffer
static auto kmd_scratch(ku_kmerdb *h) { return h->tmp.provider(KMD(h), h->stream); }

// first index in the sorted device array [0, n) whose key is not below `key` (host-driven: one 8-byte copy per step; used for
// the few cut points of kmd_merge only)
static int kmd_lower_bound(ku_kmerdb *h, const uint64_t *d, uint64_t n, uint64_t key, uint64_t *at) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    uint64_t v = 0;
    KU_HIP(KMD(h), hipMemcpyAsync(&v, d + mid, 8, hipMemcpyDeviceToHost, h->stream));
    KU_HIP(KMD(h), hipStreamSynchronize(h->stream));
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
      KU_HIP(KMD(h), hipMemcpyAsync(&v, d + i, 8, hipMemcpyDeviceToHost, s));
      KU_HIP(KMD(h), hipStreamSynchronize(s));
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
      KU_TRY(ku_rocprim(KMD(h), "rocprim::merge", kmd_scratch(h), [&](void *tmp, size_t &need) {
        return rocprim::merge(tmp, need, a + a0, b + b0, out + a0 + b0, (size_t)la, (size_t)lb, rocprim::less<uint64_t>(), s);
      }));
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
  const double t0 = ku_now();
  hipStream_t s = h->stream;
  uint64_t *a_side = h->d_a + h->n_set, *b_side = h->d_b + h->n_set;
  rocprim::double_buffer<uint64_t> keys(a_side, b_side);
  KU_TRY(ku_rocprim(KMD(h), "rocprim::radix_sort_keys", kmd_scratch(h), [&](void *tmp, size_t &need) {
    return rocprim::radix_sort_keys(tmp, need, keys, (size_t)m, 0u, 2u * h->k, s);
  }));
  uint64_t *sorted = keys.current(), *uniq = sorted == a_side ? b_side : a_side;
  unsigned long long *d_count = h->d_ctl + 1;
  KU_TRY(ku_rocprim(KMD(h), "rocprim::unique", kmd_scratch(h), [&](void *tmp, size_t &need) {
    return rocprim::unique(tmp, need, sorted, uniq, d_count, (size_t)m, rocprim::equal_to<uint64_t>(), s);
  }));
  unsigned long long u = 0;
  KU_HIP(KMD(h), hipMemcpyAsync(&u, d_count, 8, hipMemcpyDeviceToHost, s));
  KU_HIP(KMD(h), hipStreamSynchronize(s));
  // the new k-mers next to the set in d_a; the merge writes to d_b
  if (uniq != a_side) KU_HIP(KMD(h), hipMemcpyAsync(a_side, uniq, u * 8, hipMemcpyDeviceToDevice, s));
  if (h->n_set == 0) {
    h->n_set = u;
  } else {
    if (int st = kmd_merge(h, h->d_a, h->n_set, a_side, u, h->d_b)) return st;
    const size_t merged = (size_t)(h->n_set + u);  // a k-mer of the set that came up again is there twice
    KU_TRY(ku_rocprim(KMD(h), "rocprim::unique", kmd_scratch(h), [&](void *tmp, size_t &need) {
      return rocprim::unique(tmp, need, h->d_b, h->d_a, d_count, merged, rocprim::equal_to<uint64_t>(), s);
    }));
    KU_HIP(KMD(h), hipMemcpyAsync(&u, d_count, 8, hipMemcpyDeviceToHost, s));
    KU_HIP(KMD(h), hipStreamSynchronize(s));
    h->n_set = u;
  }
  h->fill = h->n_set;
  const unsigned long long cur = h->fill;
  KU_HIP(KMD(h), hipMemcpyAsync(h->d_ctl, &cur, 8, hipMemcpyHostToDevice, s));
  KU_HIP(KMD(h), hipStreamSynchronize(s));
  h->flushes++;
  h->stats.flush_s += ku_now() - t0;
  if (h->n_set > h->usable)
    return kmd_fail(h, KU_ENOMEM, "kmer_db: the distinct k-mers of pass " + std::to_string(h->pass + 1) + " (" + std::to_string(h->n_set) +
                                      " so far) do not fit the device budget (" + std::to_string(h->cap) +
                                      " k-mers, 1/64 of them kept free): use more passes (-P) or a larger budget (-s)");
  return KU_OK;
}

static int kmd_open_impl(ku_kmerdb *h, uint64_t device_bytes, const char *kdb_path, const char *idx_path) {
  KU_HIP(KMD(h), hipSetDevice(h->device));
  // (the default leaves the other half to end_pass: 56 bytes per distinct k-mer of the pass)
  KU_TRY(ku_default_budget(KMD(h), KU_KMERDB_MIN_BYTES, &device_bytes));
  if (device_bytes < KU_KMERDB_MIN_BYTES) return kmd_fail(h, KU_EINVAL, "kmer_db: the device budget is below the minimum of 64 KiB");
  const KuKmerdbBudget budget = ku_kmerdb_budget(device_bytes);
  h->seg_bytes = budget.segment;
  h->cap = budget.capacity;
  h->usable = budget.usable;
  h->merge_piece = std::min<uint64_t>((uint64_t)1 << 30, std::max<uint64_t>(h->cap / 4, 1024));
  // ---- outputs: both files exist (and are writable) before any work is done
  // (the list header's key_ct is patched in by ku_kmerdb_finish)
  const std::vector<uint8_t> hdr = ku_jflist_header(2ull * h->k);
  if (!h->out.open(kdb_path, idx_path) || !h->out.begin(hdr.data(), hdr.size(), 2, h->nt)) return kmd_fail(h, KU_ENOINPUT, h->out.error);
  // ---- device
  KU_HIP(KMD(h), hipStreamCreate(&h->stream));
  KU_HIP(KMD(h), hipMalloc((void **)&h->d_a, h->cap * 8));
  KU_HIP(KMD(h), hipMalloc((void **)&h->d_b, h->cap * 8));
  KU_HIP(KMD(h), hipMalloc((void **)&h->d_seq, h->seg_bytes));
  KU_HIP(KMD(h), hipMalloc((void **)&h->d_ctl, 3 * 8));
  KU_HIP(KMD(h), hipMemsetAsync(h->d_ctl, 0, 3 * 8, h->stream));
  KU_HIP(KMD(h), hipStreamSynchronize(h->stream));
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
  KU_TRY(ku_check_device(device));
  ku_kmerdb *h = new ku_kmerdb();
  h->device = device;
  h->k = k;
  h->nt = nt;
  h->n_passes = n_passes;
  h->key_len = (2 * k + 7) / 8;
  h->n_bins = 1ull << (2 * nt);
  const int st = kmd_open_impl(h, device_bytes, out_kdb_path, out_idx_path);
  if (st != KU_OK) { ku_kmerdb_close(h); return st; }
  *out = h;
  return KU_OK;
}

extern "C" void ku_kmerdb_close(ku_kmerdb *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void *p : {(void *)h->d_a, (void *)h->d_b, (void *)h->d_seq, (void *)h->d_ctl})
    if (p) (void)hipFree(p);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;  // (frees rocPRIM's scratch; files of a build that did not reach the end of ku_kmerdb_finish go with h->out)
}

extern "C" int ku_kmerdb_add(ku_kmerdb *h, const char *seq, uint64_t len) {
  if (!h || (len && !seq)) return fail(KU_EINVAL, "ku_kmerdb_add: null argument");
  if (h->failed) return fail(KU_EINVAL, "ku_kmerdb_add: an earlier call on this handle failed");
  if (h->finished || h->pass >= h->n_passes) return fail(KU_EINVAL, "ku_kmerdb_add: every pass has been ended");
  if (len < h->k) return KU_OK;
  KU_HIP(KMD(h), hipSetDevice(h->device));
  const double t0 = ku_now(), flush_s0 = h->stats.flush_s;
  hipStream_t s = h->stream;
  const uint32_t k = h->k;
  KmdScan a{};
  a.seq = h->d_seq;
  a.seq_bytes = h->seg_bytes;
  a.k = k;
  a.nt = h->nt;
  a.xor_mask = ku_index2_xor_mask(h->nt);
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
    KU_HIP(KMD(h), hipMemcpyAsync(h->d_seq, seq + pos, seg_len, hipMemcpyHostToDevice, s));
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
      const unsigned grid = ku_tile_grid(tiles);
      hipLaunchKernelGGL(kmerdb_extract_kernel, dim3(grid), dim3(64 * KMD_WAVES), 0, s, a);
      KU_HIP(KMD(h), hipGetLastError());
      unsigned long long ctl[3] = {0, 0, 0};
      KU_HIP(KMD(h), hipMemcpyAsync(ctl, h->d_ctl, sizeof ctl, hipMemcpyDeviceToHost, s));
      KU_HIP(KMD(h), hipStreamSynchronize(s));
      if (ctl[2] || ctl[0] < h->fill || ctl[0] > h->cap) return kmd_fail(h, KU_EHIP, "kmer_db: the extraction kernel ran out of the room it was given");
      h->windows += take;
      h->candidates += ctl[0] - h->fill;
      h->fill = ctl[0];
      w += take;
    }
    if (pos + seg_len == len) break;
    pos += n_win;
  }
  h->stats.scan_s += (ku_now() - t0) - (h->stats.flush_s - flush_s0);  // upload + extraction: the flushes are counted apart
  return KU_OK;
}

extern "C" int ku_kmerdb_end_pass(ku_kmerdb *h) {
  if (!h) return fail(KU_EINVAL, "ku_kmerdb_end_pass: null argument");
  if (h->failed) return fail(KU_EINVAL, "ku_kmerdb_end_pass: an earlier call on this handle failed");
  if (h->finished || h->pass >= h->n_passes) return fail(KU_EINVAL, "ku_kmerdb_end_pass: every pass has been ended");
  KU_HIP(KMD(h), hipSetDevice(h->device));
  if (int st = kmd_flush(h)) return st;
  const double t0 = ku_now();
  hipStream_t s = h->stream;
  const uint64_t n = h->n_set, ps = h->key_len + 4;
  const uint64_t bin_lo = kmd_pass_bound(h, h->pass), n_hist = kmd_pass_bound(h, h->pass + 1) - bin_lo;
  // the second half's arrays: 56 bytes per k-mer at their peak, 16 per bin.  Where the device cannot hold them next to both
  // buffers, the sort's other side, idle now, makes room (an allocation of that size takes seconds: not given back needlessly)
  {
    size_t free_b = 0, total_b = 0;
    KU_HIP(KMD(h), hipMemGetInfo(&free_b, &total_b));
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
    // the pass's records behind those of the passes before; the offsets of its bins (the closing one: ku_kmerdb_finish)
    KU_TRY(ku_append_from_device(KMD(h), h->out, &KuDbFiles::append_records, d_raw, n * ps, h->h_buf));
    KU_TRY(ku_append_from_device(KMD(h), h->out, &KuDbFiles::append_offsets, d_off, n_hist * 8, h->h_buf));
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
  KU_HIP(KMD(h), hipMemsetAsync(h->d_ctl, 0, 3 * 8, s));
  KU_HIP(KMD(h), hipStreamSynchronize(s));
  if (!h->d_b && h->pass < h->n_passes) KU_HIP(KMD(h), hipMalloc((void **)&h->d_b, h->cap * 8));
  h->stats.end_pass_s += ku_now() - t0;
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
  if (!h->out.finish(h->key_ct)) return kmd_fail(h, KU_ENOINPUT, h->out.error);
  h->finished = true;
  if (key_ct) *key_ct = h->key_ct;
  return KU_OK;
}
