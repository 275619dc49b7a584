// ku_sketch.hip -- ku_sketch_*: HyperLogLog sketches of a library's k-mers (ku_sketch.h): bin/count_unique (one sketch of the
// forward k-mers, the reference's count_unique) and kmer_db -P auto (one sketch of the canonical k-mers per range of the bin
// keys).  Offline tool, not on the classify hot path.
//
// ku_sketch_add packs the records into one of two pinned staging segments, one non-ACGT byte between two of them -- a window
// across two records holds it and is dropped as ambiguous --, so a launch scans a whole segment however short the records
// are.  A full segment is uploaded and scanned on the handle's stream and an event recorded behind it; the host goes on
// packing into the other segment and waits for a segment's event only when it comes back to it.
#include "ku_build.h"
#include "ku_sketch.h"

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

KuHipWho SK(ku_sketch *h) { return {"sketch: ", "", &h->failed}; }

}  // namespace

// the segment being packed may be written: what read it last has finished
static int sk_segment_ready(ku_sketch *h) {
  if (h->in_flight[h->cur]) {
    KU_HIP(SK(h), hipEventSynchronize(h->done[h->cur]));
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
  KU_HIP(SK(h), hipMemcpyAsync(h->d_seg[c], h->h_seg[c], fill, hipMemcpyHostToDevice, s));
  KuSketchScan a{};
  a.seq = h->d_seg[c];
  a.seq_bytes = h->seg_bytes;  // (bytes behind `fill` are those of an earlier segment: no window below reaches them)
  a.w_lo = 0;
  a.w_hi = fill - h->k + 1;
  a.k = h->k;
  a.p = h->p;
  a.canonical = (h->flags & KU_SKETCH_CANONICAL) ? 1u : 0u;
  a.nt = h->nt;
  a.xor_mask = h->n_groups > 1 ? ku_index2_xor_mask(h->nt) : 0u;
  a.n_groups = h->n_groups;
  a.registers = h->d_reg;
  a.n_observed = h->d_obs;
  const uint64_t tiles = (a.w_hi + KMD_TILE - 1) / KMD_TILE;
  const unsigned grid = ku_tile_grid(tiles);
  hipLaunchKernelGGL(kmersketch_kernel, dim3(grid), dim3(64 * KMD_WAVES), 0, s, a);
  KU_HIP(SK(h), hipGetLastError());
  KU_HIP(SK(h), hipEventRecord(h->done[c], s));
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
  KU_TRY(ku_check_device(device));
  ku_sketch *h = new ku_sketch();
  h->device = device;
  h->k = k;
  h->p = p;
  h->flags = flags;
  h->nt = nt;
  h->n_groups = n_groups;
  h->seg_bytes = std::max<uint64_t>((segment_bytes ? segment_bytes : KMD_MAX_SEGMENT) & ~(uint64_t)1023, 1024);
  const int st = [&]() -> int {
    KU_HIP(SK(h), hipSetDevice(device));
    KU_HIP(SK(h), hipStreamCreate(&h->stream));
    for (int i = 0; i < 2; ++i) {
      KU_HIP(SK(h), hipHostMalloc((void **)&h->h_seg[i], h->seg_bytes, hipHostMallocDefault));
      KU_HIP(SK(h), hipMalloc((void **)&h->d_seg[i], h->seg_bytes));
      KU_HIP(SK(h), hipEventCreateWithFlags(&h->done[i], hipEventDisableTiming));
    }
    KU_HIP(SK(h), hipMalloc((void **)&h->d_reg, (size_t)n_groups << p));
    KU_HIP(SK(h), hipMalloc((void **)&h->d_obs, 8));
    KU_HIP(SK(h), hipMemsetAsync(h->d_reg, 0, (size_t)n_groups << p, h->stream));
    KU_HIP(SK(h), hipMemsetAsync(h->d_obs, 0, 8, h->stream));
    KU_HIP(SK(h), hipStreamSynchronize(h->stream));
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
  KU_HIP(SK(h), hipSetDevice(h->device));
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
  KU_HIP(SK(h), hipSetDevice(h->device));
  if (int st = sk_scan_segment(h)) return st;  // the values travel through the staging segments too
  const uint64_t per_seg = h->seg_bytes / 8;
  for (uint64_t at = 0; at < n;) {
    if (int st = sk_segment_ready(h)) return st;
    const int c = h->cur;
    const uint64_t take = std::min<uint64_t>(per_seg, n - at);
    memcpy(h->h_seg[c], values + at, take * 8);
    KU_HIP(SK(h), hipMemcpyAsync(h->d_seg[c], h->h_seg[c], take * 8, hipMemcpyHostToDevice, h->stream));
    const unsigned grid = (unsigned)std::min<uint64_t>((take + KU_SKETCH_BLOCK - 1) / KU_SKETCH_BLOCK, 2048);
    hipLaunchKernelGGL(kmersketch_values_kernel, dim3(grid), dim3(KU_SKETCH_BLOCK), 0, h->stream,
                       reinterpret_cast<const uint64_t *>(h->d_seg[c]), take, h->p, h->d_reg);
    KU_HIP(SK(h), hipGetLastError());
    KU_HIP(SK(h), hipEventRecord(h->done[c], h->stream));
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
  KU_HIP(SK(h), hipSetDevice(h->device));
  if (int st = sk_scan_segment(h)) return st;  // what is staged
  unsigned long long obs = 0;
  if (registers) KU_HIP(SK(h), hipMemcpyAsync(registers, h->d_reg, (size_t)h->n_groups << h->p, hipMemcpyDeviceToHost, h->stream));
  KU_HIP(SK(h), hipMemcpyAsync(&obs, h->d_obs, 8, hipMemcpyDeviceToHost, h->stream));
  KU_HIP(SK(h), hipStreamSynchronize(h->stream));
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
