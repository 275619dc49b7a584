// ku_api_rle.cpp -- C ABI: host batches through the fused kernel with run-length encoded output, in one step and in two
// (ku_classify_batch_rle_enqueue / _finish: up to KU_RLE_MAX_IN_FLIGHT batches in flight)
#include "ku_ctx.h"

// ---- ku_classify_batch_rle through the fused kernel with run-length encoded output (ku_short.hip, OUT >= 1): no
// per-k-mer array, no second kernel; with the sparse-mode emulation on, its fast path.

// The open unit's reads in tail form (bases of each read followed by '\n') go up to the device and through the exact
// evaluation as local unit `unit` of the pass `d`: a count-less lookup gives their slots (the flat kernel; these reads were
// classified, booked and marked when their batch went through the fused kernel), ku_sparse_insert_kernel feeds L / U as
// for any staged batch.  Positions start at 2; *pos_end = the first position the reads behind the tail may use.
static int sparse_tail_insert(ku_ctx *ctx, const KuSparseDev &d, const std::vector<char> &text, const std::vector<uint32_t> &lens,
                              uint32_t unit, hipStream_t s, uint32_t *pos_end) {
  ku_ctx::Sparse &sp = ctx->sp;
  const uint64_t n_reads = lens.size(), n_bytes = text.size();
  if (pos_end) *pos_end = (uint32_t)n_bytes;
  if (n_reads == 0) return KU_OK;
  std::vector<uint64_t> off(n_reads);
  uint64_t at = 0;
  for (uint64_t r = 0; r < n_reads; ++r) { off[r] = at; at += (uint64_t)lens[r] + 1; }
  if (at != n_bytes) return fail(KU_ESTATE, "sparse-mode emulation: the open unit's reads are inconsistent");
  if (sp.t_seqs.reserve(n_bytes + 16) || sp.t_off.reserve(n_reads * 8) || sp.t_len.reserve(n_reads * 4) || sp.t_taxa.reserve((n_bytes + 16) * 4) ||
      sp.t_unit.reserve(n_reads * 4))
    return fail(KU_ENOMEM, "device memory for the open work unit's reads");
  HIP_TRY(hipMemcpyAsync(sp.t_seqs.p, text.data(), n_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(sp.t_off.p, off.data(), n_reads * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(sp.t_len.p, lens.data(), n_reads * 4, hipMemcpyHostToDevice, s));
  std::vector<uint32_t> units(n_reads, unit);
  HIP_TRY(hipMemcpyAsync(sp.t_unit.p, units.data(), n_reads * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // (`off`, `units` go out of scope; this path is rare)
  int st = ku_launch_lookup(ctx->m.db, ctx->cnt, (const uint8_t *)sp.t_seqs.p, n_bytes, (uint32_t *)sp.t_taxa.p, /*do_counts=*/false, false, false,
                            ctx->n_cu, s);
  if (st != KU_OK) return fail(st, "lookup kernel launch failed");
  return ku_launch_sparse_insert(d, ctx->m.db.k, (const uint8_t *)sp.t_seqs.p, (const uint64_t *)sp.t_off.p, (const uint32_t *)sp.t_len.p,
                                 (const uint32_t *)sp.t_unit.p, n_reads, (const uint32_t *)sp.t_taxa.p, 0u, ctx->n_cu, s);
}

// a read of the caller's batch joins the open unit's tail
static void sparse_tail_append(ku_ctx::Sparse &sp, const char *seqs, const uint64_t *seq_off, const uint32_t *seq_len, uint64_t r0, uint64_t r1) {
  for (uint64_t r = r0; r < r1; ++r) {
    sp.tail_text.insert(sp.tail_text.end(), seqs + seq_off[r], seqs + seq_off[r] + seq_len[r]);
    sp.tail_text.push_back('\n');
    sp.tail_len.push_back(seq_len[r]);
  }
}

// The open unit changes from tail form into the staged form (its L / U entries in the carry buffers): what a staged batch and
// ku_ctx_sparse_move_open_unit expect.  Every slot that is not dense is tracked, as the staged passes do.
int sparse_tail_to_carry(ku_ctx *ctx) {
  ku_ctx::Sparse &sp = ctx->sp;
  if (!sp.tail_open) return KU_OK;
  hipStream_t s = ctx->stream;
  KU_TRY(sparse_reserve_global(ctx, sp.tail_text.size(), s));
  KuSparseDev d;
  KU_TRY(sparse_pass_tables(ctx, sp.tail_text.size(), &d, s));
  KU_TRY(sparse_tail_insert(ctx, d, sp.tail_text, sp.tail_len, 0u, s, nullptr));
  KU_TRY(ku_launch_sparse_close(d, 0u, s));  // nothing closes: the largest first positions for the carry
  HIP_TRY(hipMemsetAsync(sp.d_counters + 1, 0, 16, s));
  KU_TRY(ku_launch_sparse_carry_out(d, 0u, (unsigned long long *)sp.carry_l.p, (uint32_t *)sp.carry_u.p, sp.d_counters + 1, sp.cap_carry_l,
                                    sp.cap_carry_u, s));
  unsigned long long c[3] = {0, 0, 0};
  uint32_t err = 0;
  HIP_TRY(hipMemcpyAsync(c, sp.d_counters, 24, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&err, sp.dev.err, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (err) return fail(KU_ENOMEM, "sparse-mode emulation: a device table is full");
  sp.g_count = c[0];
  sp.n_carry_l = std::min<uint64_t>(c[1], sp.cap_carry_l);
  sp.n_carry_u = std::min<uint64_t>(c[2], sp.cap_carry_u);
  sp.open = true;
  sp.tail_open = false;
  sp.tail_text.clear();
  sp.tail_len.clear();
  return KU_OK;
}

// The open unit in tail form ends here (end of an input file / of the run): it can only have turned a sketch dense if it gave
// it >= 1025 inserts -- then, and only then, the exact evaluation runs over its reads.
int sparse_tail_close(ku_ctx *ctx) {
  ku_ctx::Sparse &sp = ctx->sp;
  if (!sp.tail_open) return KU_OK;
  hipStream_t s = ctx->stream;
  if (sp.u_flag.reserve(4)) return fail(KU_ENOMEM, "device memory for the work-unit counters");
  HIP_TRY(hipMemsetAsync(sp.u_flag.p, 0, 4, s));
  KU_TRY(ku_launch_sparse_flag_units((const uint32_t *)sp.tail_row.p, ctx->tax.n_slots, ctx->tax.n_slots, sp.dev.dense, (uint8_t *)sp.u_flag.p, s));
  uint32_t flag = 0;
  HIP_TRY(hipMemcpyAsync(&flag, sp.u_flag.p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (flag & 0xFFu) {
    KU_TRY(sparse_reserve_global(ctx, sp.tail_text.size(), s));
    KuSparseDev d;
    KU_TRY(sparse_pass_tables(ctx, sp.tail_text.size(), &d, s));
    KU_TRY(sparse_tail_insert(ctx, d, sp.tail_text, sp.tail_len, 0u, s, nullptr));
    KU_TRY(ku_launch_sparse_close(d, 1u, s, /*skip_hits=*/true));
    unsigned long long c = 0;
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&c, sp.d_counters, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&err, sp.dev.err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err) return fail(KU_ENOMEM, "sparse-mode emulation: a device table is full");
    sp.g_count = c;
  }
  sp.tail_open = false;
  sp.tail_text.clear();
  sp.tail_len.clear();
  return KU_OK;
}

// KU_RLE_TIMES=1: where the batch calls spend their time on the host, summed over the run, printed when the context goes
struct RleTimes {
  double t[10] = {};  // checks, plan + enqueue, waiting for the device in _finish, behind the wait, calls; of the enqueue: [5] buffers + plan ([9]: sparse_reserve_global in it), [6] uploads, [7] launches, [8] copies back + events
  double x[6] = {};   // of 'behind the wait': [0] flagging again, [1] exact passes, [2] their number, [3] units they evaluated, [4] reads in them, [5] waiting for their kernels
  double kernel_ms = 0;  // HIP events around every batch's kernels (fused kernel + the emulation's flag kernel): the time
                         // covered by the batches' intervals -- they overlap since the batches' kernels run on two streams --
  double kernel_sum_ms = 0, cover_end = 0;  // ... their plain sum, and where the covered time ends (ms behind `ref`)
  unsigned long long reads = 0;
  static inline const bool on = getenv("KU_RLE_TIMES") != nullptr;
  static inline hipEvent_t ref = nullptr;  // (not part of the sums: the warm-up may set it)
  static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
  // the time between here and the end of the scope joins `slot`
  struct Lap {
    double &slot;
    const double t0 = on ? now() : 0.0;
    ~Lap() { if (on) slot += now() - t0; }
  };
  void count_finish() { if (on) t[4] += 1; }
  void count_exact_pass(double units, double n_reads) { if (on) { x[2] += 1; x[3] += units; x[4] += n_reads; } }
  // a finished batch's kernels, from the events around them
  void add_kernels(hipEvent_t k0, hipEvent_t k1, uint64_t n_reads) {
    float ms = 0, a = 0, b = 0;
    if (ref && hipEventElapsedTime(&ms, k0, k1) == hipSuccess && hipEventElapsedTime(&a, ref, k0) == hipSuccess &&
        hipEventElapsedTime(&b, ref, k1) == hipSuccess) {
      kernel_sum_ms += ms;
      kernel_ms += std::max(0.0, (double)b - std::max((double)a, cover_end));  // (the batches come in the order of their starts)
      cover_end = std::max(cover_end, (double)b);
      reads += n_reads;
    } else (void)hipGetLastError();
  }
  void print() const {
    if (on && t[4] > 0)
      fprintf(stderr, "ku_classify_batch_rle over %.0f batches: checks %.3f s, plan + enqueue %.3f s, waiting for the device %.3f s, behind the wait %.3f s; "
                      "kernels %.3f ms for %llu reads (HIP events on their streams: the time the batches' intervals cover; their sum is %.3f ms); of the enqueue: buffers + plan %.3f s, uploads %.3f s, launches %.3f s, "
                      "copies back + events %.3f s; of buffers + plan: room in the emulation's run-wide set %.3f s\n",
              t[4], t[0], t[1], t[2], t[3], kernel_ms, reads, kernel_sum_ms, t[5], t[6], t[7], t[8], t[9]);
    if (on && x[2] > 0)
      fprintf(stderr, "ku_classify_batch_rle, behind the wait: flagging again %.3f s, %.0f exact passes over %.0f work units (%.0f reads) %.3f s, of it %.3f s waiting for their kernels\n", x[0], x[2],
              x[3], x[4], x[1], x[5]);
  }
};
static RleTimes g_rle;
void rle_times_print() { g_rle.print(); }

// The exact per-unit evaluation of the emulation for the units the fused kernel could not settle by counting: `flagged`
// (ascending unit numbers of the job's batch; flag_all: every slot of the unit is tracked -- a unit in the staged form).
// last_is_open: the last flagged unit stays open behind the batch (staged form: its entries go into the carry buffers).
static int sparse_fast_exact(ku_ctx *ctx, RleJob &j, const std::vector<uint32_t> &flagged, const std::vector<uint8_t> &flag_all,
                             bool last_is_open, hipStream_t s) {
  ku_ctx::Sparse &sp = ctx->sp;
  const uint32_t *h_len = j.b.seq_len;
  const std::vector<uint64_t> &unit_first_read = j.unit_first_read;
  const uint32_t *d_u_cnt = (const uint32_t *)j.u_cnt.p;
  // the batch's runs: its own run array -- or, when that overflowed, the context's buffers, where rle_job_finish's redo (per-k-mer
  // codes + ku_rle_kernel, whose bound cannot overflow) left them; counts, SEEN marks and u_cnt are the fused kernel's either way
  const void *d_runs = j.runs_in_ctx ? ctx->b_runs.p : j.runs.p;
  const uint64_t *d_roff = (const uint64_t *)(j.runs_in_ctx ? ctx->b_roff.p : j.roff.p);
  const uint32_t *d_rcnt = (const uint32_t *)(j.runs_in_ctx ? ctx->b_rcnt.p : j.rcnt.p);
  // unit 0 continues a unit in tail form: its earlier reads are evaluated with it, and come first in the position space
  const bool with_tail = j.cont_tail && !flagged.empty() && flagged[0] == 0 && !j.tail_len.empty();
  const uint64_t tail_bytes = with_tail ? j.tail_text.size() : 0;
  size_t at = 0;
  bool first_pass = true;
  while (at < flagged.size()) {
    // units of this pass: at most 2^25 bases and KU_SPARSE_MAX_UNITS units (the tables of ku_sparse.hip)
    size_t end = at;
    uint64_t bases = first_pass ? tail_bytes : 0, n_list = 0;
    while (end < flagged.size() && end - at < KU_SPARSE_MAX_UNITS) {
      const uint32_t u = flagged[end];
      uint64_t ub = 0;
      for (uint64_t r = unit_first_read[u]; r < unit_first_read[u + 1]; ++r) ub += h_len[r];
      if (end > at && bases + ub > (1ull << 25)) break;
      bases += ub;
      n_list += unit_first_read[u + 1] - unit_first_read[u];
      ++end;
    }
    const bool has_open = last_is_open && end == flagged.size();
    std::vector<uint32_t> list(3 * n_list);
    uint64_t li = 0;
    for (size_t f = at; f < end; ++f) {
      const uint32_t u = flagged[f];
      for (uint64_t r = unit_first_read[u]; r < unit_first_read[u + 1]; ++r, ++li) {
        list[li] = (uint32_t)r;
        list[n_list + li] = (uint32_t)(f - at) | (flag_all[f] ? 0x80000000u : 0u);
        list[2 * n_list + li] = u;
      }
    }
    if (sp.list.reserve(std::max<uint64_t>(n_list, 1) * 12) != KU_OK) return fail(KU_ENOMEM, "device memory for the flagged work units' reads");
    KU_TRY(sparse_reserve_global(ctx, bases + sp.n_carry_l, s));
    KuSparseDev d;  // this pass's view: the run-wide set as it is now, L / U sized for the pass
    KU_TRY(sparse_pass_tables(ctx, bases + sp.n_carry_l + sp.n_carry_u, &d, s));
    if (first_pass && j.cont_carry)  // the unit carried over from the batch before is local unit 0 of the first pass
      KU_TRY(ku_launch_sparse_carry_in(d, (const unsigned long long *)sp.carry_l.p, sp.n_carry_l, (const uint32_t *)sp.carry_u.p, sp.n_carry_u, s));
    uint32_t pos_base = 0;
    if (first_pass && with_tail) KU_TRY(sparse_tail_insert(ctx, d, j.tail_text, j.tail_len, 0u, s, &pos_base));
    if (n_list) HIP_TRY(hipMemcpyAsync(sp.list.p, list.data(), n_list * 12, hipMemcpyHostToDevice, s));
    const uint32_t *dl = (const uint32_t *)sp.list.p;
    KU_TRY(ku_launch_sparse_insert_runs(d, ctx->m.db.k, (const uint8_t *)j.seqs.p, (const uint64_t *)j.off.p, (const uint32_t *)j.len.p,
                                        dl, dl + n_list, dl + 2 * n_list, n_list, d_runs, d_roff, d_rcnt, ctx->d_slot_taxid, ctx->tax.n_slots,
                                        d_u_cnt, ctx->n_cu, s, pos_base));
    const uint32_t n_local = (uint32_t)(end - at);
    // (a unit in the staged form may hold k-mers of a staged batch, which marks nothing in the probe table: its entries all
    // go into the set; the fast path's own units only contribute their misses)
    KU_TRY(ku_launch_sparse_close(d, has_open ? n_local - 1 : n_local, s, /*skip_hits=*/!j.cont_carry));
    if (first_pass && j.cont_carry) sp.n_carry_l = sp.n_carry_u = 0;
    unsigned long long c[3] = {0, 0, 0};
    if (has_open) {
      HIP_TRY(hipMemsetAsync(sp.d_counters + 1, 0, 16, s));
      KU_TRY(ku_launch_sparse_carry_out(d, n_local - 1, (unsigned long long *)sp.carry_l.p, (uint32_t *)sp.carry_u.p, sp.d_counters + 1,
                                        sp.cap_carry_l, sp.cap_carry_u, s));
    }
    HIP_TRY(hipMemcpyAsync(c, sp.d_counters, 24, hipMemcpyDeviceToHost, s));
    { RleTimes::Lap lap{g_rle.x[5]}; HIP_TRY(hipStreamSynchronize(s)); }  // `list` goes out of scope
    sp.g_count = std::max<uint64_t>(sp.g_count, c[0]);
    if (has_open) {
      sp.n_carry_l = std::min<uint64_t>(c[1], sp.cap_carry_l);
      sp.n_carry_u = std::min<uint64_t>(c[2], sp.cap_carry_u);
    }
    first_pass = false;
    at = end;
  }
  return KU_OK;
}

// may the batch take the fused kernel with run-length encoded output?  (the same conditions as the fused path of
// classify_device_impl, plus what the emulation's fast path needs)
static bool rle_fused_eligible(ku_ctx *ctx, uint32_t flags, uint32_t max_n, uint64_t n_bytes, uint64_t n_reads, bool monotonic) {
  if (getenv("KU_NO_FUSED") || getenv("KU_NO_FUSED_RLE") || !ctx->extra.empty() || ctx->d_exact_set) return false;
  if (flags & (KU_F_QUICK | KU_F_KEEP_SLOTS)) return false;
  const uint32_t short_max = ku_short_max_kmers(ctx->m.db);
  if (!short_max) return false;
  if (max_n > short_max && (max_n > ku_short_max_kmers_windowed(ctx->m.db) || getenv("KU_NO_WINDOWED"))) return false;
  if (n_reads >= (1ull << 32)) return false;
  const bool sparse = ctx->sp.on && !(flags & KU_F_NO_COUNTS);
  if (sparse) {
    const ku_ctx::Sparse &sp = ctx->sp;
    // (positions of the exact evaluation are 32-bit: the batch, behind the reads of an open unit of at most 2^24 nt + one read)
    if (getenv("KU_NO_SPARSE_FAST") || !monotonic || sp.unit_nt == 0 || sp.unit_nt > (1ull << 24) || n_bytes + (1ull << 26) >= (1ull << 32)) return false;
    const uint64_t max_units = n_bytes / sp.unit_nt + 2;
    if (max_units * ctx->tax.n_slots > (1ull << 29)) return false;  // the (unit, slot) counters: at most 2 GiB
  }
  return true;
}

// the windowed instance's spill workspace (reads beyond the one-pass instance's k-mers)
static uint64_t rle_workspace_bytes(const ku_ctx *ctx, uint32_t max_n, uint64_t n_reads) {
  if (max_n <= ku_short_max_kmers(ctx->m.db) || max_n > ku_short_max_kmers_windowed(ctx->m.db)) return 0;
  return ku_short_workspace_bytes(max_n, ctx->tax.n_slots, n_reads, ctx->n_cu);
}

// How a batch goes through the fused kernel: its segments, the run array, the workspace.  Host arithmetic only.
struct RlePlan {
  std::vector<uint64_t> seg;  // first read of every segment, and n_reads
  uint64_t total_waves = 0;   // waves of all the segments' launches
  uint32_t chunk = 0;         // entries of the run array a wave claims at a time
  uint64_t runs_cap = 0;      // entries of the run array
  uint64_t ws = 0;            // bytes of the windowed instance's workspace
  uint64_t n_seg() const { return seg.size() - 1; }
};
// seq_off: the reads' offsets when the batch may go up in segments (they ascend), else null: one segment.  test_hook: KU_RUNS_CAP applies.
// flags: the batch's (KU_F_NO_COUNTS selects other kernel instances, whose grids may differ).
static RlePlan rle_plan(const ku_ctx *ctx, uint64_t n_bytes, uint64_t n_reads, uint32_t max_n, uint32_t flags, const uint64_t *seq_off, bool test_hook) {
  RlePlan p;
  // ---- segments of the batch: cut at read boundaries, uploaded one after the other on the copy stream while the
  // compute stream classifies the ones before
  uint64_t n_seg = 1;
  // (16 MiB per segment since round 5 -- was 8: with several batches in flight the overlap of upload and kernels comes from the
  // OTHER batches, and a launch of 120 k reads costs 3.0 us per thousand reads where two of 60 k cost 3.8, ku_short.hip)
  constexpr uint64_t seg_bytes = 16ull << 20;
  if (seq_off && !getenv("KU_NO_H2D_OVERLAP")) n_seg = std::min<uint64_t>(8, std::max<uint64_t>(1, n_bytes / seg_bytes));
  p.seg.assign(n_seg + 1, 0);
  for (uint64_t g = 1; g < n_seg; ++g) {
    const uint64_t target = n_bytes / n_seg * g;
    p.seg[g] = std::max<uint64_t>(p.seg[g - 1], (uint64_t)(std::lower_bound(seq_off, seq_off + n_reads, target) - seq_off));
  }
  p.seg[n_seg] = n_reads;
  uint64_t max_seg_reads = 0;
  for (uint64_t g = 0; g < n_seg; ++g) {
    p.total_waves += ku_short_grid_waves(p.seg[g + 1] - p.seg[g], max_n, ctx->n_cu, !(flags & KU_F_NO_COUNTS));
    max_seg_reads = std::max(max_seg_reads, p.seg[g + 1] - p.seg[g]);
  }
  // a wave claims `chunk` run entries at a time: large enough for few claims, small enough that the unused tails of the
  // last chunks do not dominate a small batch
  const uint64_t reads_per_wave = n_reads / std::max<uint64_t>(p.total_waves, 1);
  p.chunk = reads_per_wave >= 64 ? 256u : (reads_per_wave >= 16 ? 64u : 16u);
  // room for ~ one run per 6 bases + the chunk tails; a batch that needs more (many taxa per read) is redone through
  // the per-k-mer array (in _finish), whose run-length encoder cannot overflow
  p.runs_cap = n_bytes / 6 + 4 * n_reads + p.total_waves * p.chunk + 4096;
  if (const char *e = test_hook ? getenv("KU_RUNS_CAP") : nullptr) p.runs_cap = std::max<uint64_t>(1, (uint64_t)atoll(e));
  p.ws = rle_workspace_bytes(ctx, max_n, max_seg_reads);
  return p;
}

// sizes that hold a batch whatever its flags (callers that size buffers ahead of the batches)
static RlePlan rle_plan_any_flags(const ku_ctx *ctx, uint64_t n_bytes, uint64_t n_reads, uint32_t max_n) {
  RlePlan p = rle_plan(ctx, n_bytes, n_reads, max_n, 0, nullptr, false);
  const RlePlan q = rle_plan(ctx, n_bytes, n_reads, max_n, KU_F_NO_COUNTS, nullptr, false);
  p.runs_cap = std::max(p.runs_cap, q.runs_cap);
  p.ws = std::max(p.ws, q.ws);
  return p;
}

// no batch may be in flight (entry points that read or change what the batches in flight work on)
int rle_idle(const ku_ctx *ctx, const char *who) {
  if (ctx->rle_in_flight) return fail(KU_ESTATE, std::string(who) + ": batches are in flight (ku_classify_batch_rle_finish first)");
  return KU_OK;
}

extern "C" uint64_t ku_device_rle_runs_cap(const ku_ctx *ctx, uint64_t n_bytes, uint64_t n_reads, uint32_t max_read_len) {
  if (!ctx || !ctx->tax_set) return 0;
  return rle_plan_any_flags(ctx, n_bytes, n_reads, ku_max_kmers(ctx->m.db.k, max_read_len)).runs_cap;
}

extern "C" int ku_classify_batch_device_rle(ku_ctx *ctx, const void *d_seqs, uint64_t n_bytes, const uint64_t *d_seq_off,
                                            const uint32_t *d_seq_len, uint64_t n_reads, const ku_opts *opts, uint32_t *d_calls,
                                            ku_run *d_runs, uint64_t runs_cap, uint64_t *d_run_off, uint32_t *d_run_cnt,
                                            uint64_t *d_n_runs, void *stream) {
  KU_TRY(check_ready(ctx));
  KU_TRY(rle_idle(ctx, "ku_classify_batch_device_rle"));
  if (!d_n_runs || (n_reads && (!d_seqs || !d_seq_off || !d_seq_len || !d_calls || !d_runs || !d_run_off || !d_run_cnt)))
    return fail(KU_EINVAL, "ku_classify_batch_device_rle: null buffer");
  const ku_opts o = opts ? *opts : ku_opts{0, 1, 0, 0};
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  HIP_TRY(hipMemsetAsync(d_n_runs, 0, 8, s));
  if (n_reads == 0) return KU_OK;
  if (o.max_read_len == 0) return fail(KU_EINVAL, "ku_classify_batch_device_rle: opts->max_read_len (the longest read of the batch) is required");
  const uint32_t max_n = ku_max_kmers(ctx->m.db.k, o.max_read_len);
  if (ctx->sp.on && !(o.flags & KU_F_NO_COUNTS))
    return fail(KU_EUNSUP, "the sparse-mode emulation runs through the host-buffer entry points (it needs the read lengths on the host)");
  if (!store_whole(ctx->m) || !rle_fused_eligible(ctx, o.flags, max_n, n_bytes, n_reads, true))
    return fail(KU_EUNSUP, "ku_classify_batch_device_rle: the fused kernel does not apply to this context / these options (ku_classify_batch_device does)");
  const RlePlan p = rle_plan(ctx, n_bytes, n_reads, max_n, o.flags, nullptr, false);  // (the caller's run array: its own runs_cap)
  if (p.ws > ctx->b_ws.cap) HIP_TRY(hipStreamSynchronize(s));
  if (ctx->b_ws.reserve(p.ws)) return fail(KU_ENOMEM, "device memory for the windowed kernel's workspace");
  KuRunsOut ro{};
  ro.runs = (uint2 *)d_runs;
  ro.counter = (unsigned long long *)d_n_runs;
  ro.cap = runs_cap;
  ro.chunk = p.chunk;
  ro.run_off = d_run_off;
  ro.run_cnt = d_run_cnt;
  // every wave owns its first chunk, the counter starts behind those (as in rle_job_enqueue: no claim storm at the launch's start)
  if (p.total_waves * p.chunk <= runs_cap && p.total_waves * p.chunk < (1ull << 31)) {
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_n_runs, (int)(p.total_waves * p.chunk), 1, s));
    ro.pre_base1 = 1;
  }
  int st = ku_launch_classify_short(ctx->m.db, ctx->tax, ctx->cnt, (const uint8_t *)d_seqs, n_bytes, d_seq_off, d_seq_len, n_reads, max_n, o.flags,
                                    d_calls, nullptr, nullptr, ctx->b_ws.p, ctx->b_ws.cap, ctx->n_cu, s, ctx->claim, &ro, nullptr);
  return st == KU_OK ? KU_OK : fail(st, "fused kernel launch failed");
}

// ---- step one: plan the batch, start its upload (in segments, on the copy stream), its kernels and the copies back.
// Nothing here waits for the device.  The stages come first, in the order rle_job_enqueue runs them.

// ---- sparse fast path: work-unit plan (the unit closes behind the read that fills it, classify.cpp:510-521).  Host only.
static int plan_work_units(ku_ctx *ctx, RleJob &j, const RleBatch &b, bool sparse) {
  const ku_ctx::Sparse &sp = ctx->sp;
  j.sparse = sparse;
  j.cont_carry = j.cont_tail = j.open_after = false;
  j.n_units = 0;
  j.kmers = 0;
  j.unit_first_read.clear();
  j.tail_text.clear();
  j.tail_len.clear();
  if (!sparse) return KU_OK;
  if (j.pin_unit.reserve(b.n_reads * 4)) return fail(KU_ENOMEM, "page-locked memory for the work-unit plan");
  uint32_t *h_unit = (uint32_t *)j.pin_unit.p;
  uint64_t acc = sp.acc_nt;
  uint32_t cur = 0;
  j.cont_carry = sp.open;
  j.cont_tail = sp.tail_open && !sp.open;
  j.unit_first_read.push_back(0);
  for (uint64_t r = 0; r < b.n_reads; ++r) {
    h_unit[r] = cur;
    acc += b.seq_len[r];
    if (acc >= sp.unit_nt) { ++cur; acc = 0; j.unit_first_read.push_back(r + 1); }
  }
  j.open_after = acc > 0;
  j.acc_after = acc;
  j.n_units = cur + (j.unit_first_read.back() < b.n_reads ? 1u : 0u);
  if (j.unit_first_read.back() < b.n_reads) j.unit_first_read.push_back(b.n_reads);
  for (uint64_t r = 0; r < b.n_reads; ++r) j.kmers += ku_max_kmers(ctx->m.db.k, b.seq_len[r]);
  return KU_OK;
}

// room in the run-wide set for what the batch may add, and the emulation's tables as the fused kernel sees them
static int sparse_fast_view(ku_ctx *ctx, RleJob &j, KuSparseFast *sf) {
  ku_ctx::Sparse &sp = ctx->sp;
  uint64_t in_flight_kmers = 0;  // what the batches in flight may still add: the host's count of the set lags behind them
  for (const RleJob &q : ctx->rle) if (q.busy && &q != &j && q.sparse) in_flight_kmers += q.kmers;
  // (drains the batches in flight when it grows the set)
  { RleTimes::Lap lap{g_rle.t[9]}; KU_TRY(sparse_reserve_global(ctx, j.kmers + in_flight_kmers + sp.n_carry_l, ctx->stream)); }
  sf->g_key = sp.dev.g_key;
  sf->g_mask = sp.dev.g_mask;
  sf->g_count = sp.dev.g_count;
  sf->dense = sp.dev.dense;
  sf->u_cnt = (uint32_t *)j.u_cnt.p;
  sf->err = sp.dev.err;
  sf->n_slots = ctx->tax.n_slots;
  sf->unit_base = 0;
  ctx->m.seen_dirty = true;  // the kernel books the k-mers the database holds by marking their table entries
  return KU_OK;
}

// the kernel stream `s` behind the context's own; the counters; every segment's upload on the copy stream and its launch behind it
static int queue_uploads_and_launches(ku_ctx *ctx, RleJob &j, const RleBatch &b, const RlePlan &p, hipStream_t s, KuSparseFast *sf, bool *clock_started) {
  const bool sparse = sf != nullptr;
  unsigned long long *h_tot = (unsigned long long *)j.pin.p;
  const uint32_t *h_unit = (const uint32_t *)j.pin_unit.p;
  // whatever was queued on the context's own stream before this batch comes first
  HIP_TRY(hipEventRecord(ctx->main_ev, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(s, ctx->main_ev, 0));
  unsigned long long *d_counter = j.d_counter;
  // (emulation) the per-(unit, slot) insert counts and the unit flags start at zero: one launch
  if (sparse) {
    if (ku_launch_zero3(d_counter, 2, j.u_cnt.p, std::max<uint64_t>((uint64_t)j.n_units * ctx->tax.n_slots, 1), j.u_flag.p,
                        ((uint64_t)std::max<uint32_t>(j.n_units, 1) + 3) / 4, s) != KU_OK)
      return fail(KU_EHIP, "clearing the batch counters failed");
    // (unit 0 continues the open unit: the inserts that unit has had so far join its row BEHIND the kernels, below)
  }
  // the run counter starts behind the chunks the waves own from the start (one per wave of every segment's launch)
  h_tot[3] = p.total_waves * (unsigned long long)p.chunk;
  HIP_TRY(hipMemcpyAsync(d_counter, &h_tot[3], 8, hipMemcpyHostToDevice, s));
  KuRunsOut ro{};
  ro.runs = (uint2 *)j.runs.p;
  ro.counter = d_counter;
  ro.cap = p.runs_cap;
  ro.chunk = p.chunk;
  if (RleTimes::on) { KU_TRY(ensure_event(j.t_k0, hipEventDefault)); KU_TRY(ensure_event(j.t_k1, hipEventDefault)); }
  uint64_t waves_before = 0;
  for (uint64_t g = 0; g < p.n_seg(); ++g) {
    const uint64_t a = p.seg[g], e = p.seg[g + 1];
    const uint64_t lo = g == 0 ? 0 : b.seq_off[a], hi = g + 1 == p.n_seg() ? b.n_bytes : b.seq_off[e];
    // (always the copy stream: with a batch in flight, this one's upload runs under that one's kernels)
    hipStream_t cs = ctx->h2d_stream;
    {
      RleTimes::Lap lap{g_rle.t[6]};
      if (hi > lo) HIP_TRY(hipMemcpyAsync((char *)j.seqs.p + lo, b.seqs + lo, hi - lo, hipMemcpyHostToDevice, cs));
      if (e > a) {
        HIP_TRY(hipMemcpyAsync((uint64_t *)j.off.p + a, b.seq_off + a, (e - a) * 8, hipMemcpyHostToDevice, cs));
        HIP_TRY(hipMemcpyAsync((uint32_t *)j.len.p + a, b.seq_len + a, (e - a) * 4, hipMemcpyHostToDevice, cs));
        if (sparse) HIP_TRY(hipMemcpyAsync((uint32_t *)j.unit.p + a, h_unit + a, (e - a) * 4, hipMemcpyHostToDevice, cs));
      }
      HIP_TRY(hipEventRecord(j.seg_events[g], cs));
      HIP_TRY(hipStreamWaitEvent(s, j.seg_events[g], 0));
    }
    if (e == a) continue;
    RleTimes::Lap lap{g_rle.t[7]};
    ro.run_off = (uint64_t *)j.roff.p + a;
    ro.run_cnt = (uint32_t *)j.rcnt.p + a;
    ro.pre_base1 = (uint32_t)(1 + waves_before);
    waves_before += ku_short_grid_waves(e - a, b.max_n, ctx->n_cu, !(b.o.flags & KU_F_NO_COUNTS));
    if (sparse) sf->unit_of = (const uint32_t *)j.unit.p + a;
    if (RleTimes::on && !*clock_started) {  // (behind the first segment's upload)
      if (!RleTimes::ref) { KU_TRY(ensure_event(RleTimes::ref, hipEventDefault)); HIP_TRY(hipEventRecord(RleTimes::ref, s)); }
      HIP_TRY(hipEventRecord(j.t_k0, s));
      *clock_started = true;
    }
    int st = ku_launch_classify_short(ctx->m.db, ctx->tax, ctx->cnt, (const uint8_t *)j.seqs.p, b.n_bytes, (const uint64_t *)j.off.p + a,
                                      (const uint32_t *)j.len.p + a, e - a, b.max_n, b.o.flags, (uint32_t *)j.calls.p + a, nullptr, nullptr,
                                      j.ws.p, j.ws.cap, ctx->n_cu, s, ctx->claim, &ro, sf);
    if (st != KU_OK) { (void)hipStreamSynchronize(ctx->h2d_stream); (void)hipStreamSynchronize(s); return fail(st, "fused kernel launch failed"); }
  }
  return KU_OK;
}

// The open unit's insert counts (sp.tail_row) travel from batch to batch through this small step behind the kernels: it
// reads what the batch before wrote behind ITS kernels on the other stream, and what it writes must not land before that
// batch has read -- so the step (not the kernels) waits for the whole of the batch before, in enqueue order.
static int queue_open_unit_step(ku_ctx *ctx, RleJob &j, hipStream_t s) {
  ku_ctx::Sparse &sp = ctx->sp;
  if (ctx->prev_kernels_done) HIP_TRY(hipStreamWaitEvent(s, ctx->prev_kernels_done, 0));
  // unit 0 continues the open unit: the inserts that unit had before this batch join its row
  if (j.cont_tail && j.n_units)
    KU_TRY(ku_launch_add_u32((uint32_t *)j.u_cnt.p, (const uint32_t *)sp.tail_row.p, ctx->tax.n_slots, s));
  KU_TRY(ku_launch_sparse_flag_units((const uint32_t *)j.u_cnt.p, (uint64_t)j.n_units * ctx->tax.n_slots, ctx->tax.n_slots, sp.dev.dense,
                                     (uint8_t *)j.u_flag.p, s));
  // the unit that stays open (tail form): its insert counts so far
  if (j.open_after && !(j.cont_carry && j.n_units == 1))
    HIP_TRY(hipMemcpyAsync(sp.tail_row.p, (const uint32_t *)j.u_cnt.p + (size_t)(j.n_units - 1) * ctx->tax.n_slots, (size_t)ctx->tax.n_slots * 4,
                           hipMemcpyDeviceToDevice, s));
  return KU_OK;
}

// ---- the copies back run on a stream of their own, behind this batch's kernels -- not in front of the next batch's
static int queue_copies_back(ku_ctx *ctx, RleJob &j, const RleBatch &b, uint64_t runs_cap, hipStream_t s) {
  unsigned long long *h_tot = (unsigned long long *)j.pin.p;
  const hipStream_t ds = ctx->d2h_stream;
  HIP_TRY(hipEventRecord(j.kernels_done, s));
  ctx->prev_kernels_done = j.kernels_done;  // (the jobs' events live as long as the context)
  HIP_TRY(hipStreamWaitEvent(ds, j.kernels_done, 0));
  HIP_TRY(hipMemcpyAsync(b.calls, j.calls.p, b.n_reads * 4, hipMemcpyDeviceToHost, ds));
  HIP_TRY(hipMemcpyAsync(b.run_off, j.roff.p, b.n_reads * 8, hipMemcpyDeviceToHost, ds));
  HIP_TRY(hipMemcpyAsync(b.run_cnt, j.rcnt.p, b.n_reads * 4, hipMemcpyDeviceToHost, ds));
  HIP_TRY(hipMemcpyAsync(&h_tot[0], j.d_counter, 8, hipMemcpyDeviceToHost, ds));
  // the runs themselves, when the caller said where they go: as much of the run array as its buffer holds (the extent in use
  // is only known behind the kernel; _finish tells whether it fitted -- else ku_fetch_runs, into a larger buffer)
  j.runs_copied = b.runs ? std::min<uint64_t>(b.runs_cap, runs_cap) : 0;
  if (j.runs_copied) HIP_TRY(hipMemcpyAsync(b.runs, j.runs.p, j.runs_copied * 8, hipMemcpyDeviceToHost, ds));
  if (j.sparse) {
    HIP_TRY(hipMemcpyAsync((uint8_t *)j.pin.p + 64, j.u_flag.p, std::max<uint32_t>(j.n_units, 1), hipMemcpyDeviceToHost, ds));
    HIP_TRY(hipMemcpyAsync(&h_tot[1], ctx->sp.dev.g_count, 8, hipMemcpyDeviceToHost, ds));
    HIP_TRY(hipMemcpyAsync(&h_tot[2], ctx->sp.dev.err, 4, hipMemcpyDeviceToHost, ds));
  }
  HIP_TRY(hipEventRecord(j.done, ds));
  return KU_OK;
}

// ---- the emulation's state behind this batch (what the next batch's plan starts from).  Host only.
static void advance_emulation_state(ku_ctx::Sparse &sp, RleJob &j, const RleBatch &b) {
  const bool whole_batch_one_open_unit = j.n_units == 1 && j.open_after;
  if (j.cont_tail && !whole_batch_one_open_unit) {  // unit 0 closes in this batch: its earlier reads go with the job
    j.tail_text.swap(sp.tail_text);
    j.tail_len.swap(sp.tail_len);
    sp.tail_text.clear();
    sp.tail_len.clear();
  }
  if (j.cont_carry && whole_batch_one_open_unit) {
    // (staged form, still open: stays in the carry buffers -- _finish writes them)
  } else if (j.open_after) {
    if (!(j.cont_tail && whole_batch_one_open_unit)) { sp.tail_text.clear(); sp.tail_len.clear(); }
    sparse_tail_append(sp, b.seqs, b.seq_off, b.seq_len, j.unit_first_read[j.n_units - 1], b.n_reads);
    sp.tail_open = true;
    sp.open = false;
  } else {
    sp.tail_open = false;
    sp.open = false;
    sp.tail_text.clear();
    sp.tail_len.clear();
  }
  sp.acc_nt = j.acc_after;
}

static int rle_job_enqueue(ku_ctx *ctx, RleJob &j, const RleBatch &b) {
  RleTimes::Lap lap_all{g_rle.t[1]};
  // the batch's kernels: consecutive batches take the two kernel streams in turn (never the context's own stream, ku_ctx.h)
  hipStream_t &ks = ctx->k_streams[(&j - &ctx->rle[0]) & 1];
  KU_TRY(ensure_stream(ks));
  KU_TRY(ensure_event(ctx->main_ev));
  const hipStream_t s = ks;
  const bool sparse = ctx->sp.on && !(b.o.flags & KU_F_NO_COUNTS);
  RlePlan p;
  KuSparseFast sf{};
  {
    RleTimes::Lap lap{g_rle.t[5]};
    p = rle_plan(ctx, b.n_bytes, b.n_reads, b.max_n, b.o.flags, b.monotonic ? b.seq_off : nullptr, /*test_hook=*/true);
    // (the work units come before the buffers: their number sizes the counters)
    KU_TRY(plan_work_units(ctx, j, b, sparse));
    // (the job's buffers are its own and its previous batch is through: growing them needs no synchronisation of ours)
    KU_TRY(j.reserve(b.n_bytes, b.n_reads, p.runs_cap, p.ws, p.n_seg(), sparse, j.n_units, ctx->tax.n_slots));
    KU_TRY(ensure_stream(ctx->h2d_stream));
    KU_TRY(ensure_stream(ctx->d2h_stream));
    if (sparse) {
      if (ctx->sp.tail_row.reserve((size_t)ctx->tax.n_slots * 4)) return fail(KU_ENOMEM, "device memory for the work-unit counters");
      KU_TRY(sparse_fast_view(ctx, j, &sf));
    }
  }
  bool clock_started = false;
  KU_TRY(queue_uploads_and_launches(ctx, j, b, p, s, sparse ? &sf : nullptr, &clock_started));
  {
    RleTimes::Lap lap{g_rle.t[8]};
    if (sparse) KU_TRY(queue_open_unit_step(ctx, j, s));
    if (clock_started) HIP_TRY(hipEventRecord(j.t_k1, s));
    KU_TRY(queue_copies_back(ctx, j, b, p.runs_cap, s));
  }
  if (sparse && j.n_units) advance_emulation_state(ctx->sp, j, b);
  j.b = b;
  j.runs_cap = p.runs_cap;
  j.settled = false;
  j.runs_in_ctx = false;
  j.busy = true;
  return KU_OK;
}

// ---- step two: wait for the batch (one event), settle what the emulation has to settle for it
static int rle_job_finish(ku_ctx *ctx, RleJob &j, uint64_t *n_runs, bool *classified) {
  hipStream_t s = ctx->stream;
  *classified = false;
  ctx->last_runs_copied = 0;
  if (j.settled) {
    j.busy = false;
    *n_runs = ctx->n_runs = j.n_runs;
    *classified = true;
    return KU_OK;
  }
  { RleTimes::Lap lap{g_rle.t[2]}; HIP_TRY(hipEventSynchronize(j.done)); }
  RleTimes::Lap lap_rest{g_rle.t[3]};
  g_rle.count_finish();
  if (RleTimes::on && j.t_k0 && j.b.n_reads) g_rle.add_kernels(j.t_k0, j.t_k1, j.b.n_reads);
  j.busy = false;
  ku_ctx::Sparse &sp = ctx->sp;
  const unsigned long long *h_tot = (const unsigned long long *)j.pin.p;
  const uint8_t *h_flag = (const uint8_t *)j.pin.p + 64;
  const unsigned long long total = h_tot[0];
  if (j.b.hits) memset(j.b.hits, 0, j.b.n_reads * 4);  // "Q:n" is quick mode only
  ctx->last_calls_dev = j.calls.p;
  if (total > j.runs_cap) {
    // the run array was too small for this batch (reads that change taxon every few k-mers): the per-k-mer codes once more
    // without any accounting, through the array parallel to the reads and its own run-length encoder (the context's buffers)
    if (ctx->b_taxa.reserve((j.b.n_bytes + 16) * 4) || ctx->b_runs.reserve((j.b.n_bytes + 1) * 8) || ctx->b_roff.reserve(j.b.n_reads * 8) ||
        ctx->b_rcnt.reserve(j.b.n_reads * 4) || ctx->b_calls.reserve(j.b.n_reads * 4))
      return fail(KU_ENOMEM, "device batch buffers");
    if (ctx->b_ws.reserve(rle_workspace_bytes(ctx, j.b.max_n, j.b.n_reads))) return fail(KU_ENOMEM, "device batch buffers");
    int st = ku_launch_classify_short(ctx->m.db, ctx->tax, ctx->cnt, (const uint8_t *)j.seqs.p, j.b.n_bytes, (const uint64_t *)j.off.p,
                                      (const uint32_t *)j.len.p, j.b.n_reads, j.b.max_n, j.b.o.flags | KU_F_NO_COUNTS, (uint32_t *)ctx->b_calls.p,
                                      (uint32_t *)ctx->b_taxa.p, nullptr, ctx->b_ws.p, ctx->b_ws.cap, ctx->n_cu, s, ctx->claim);
    if (st != KU_OK) return fail(st, "fused kernel launch failed");
    KU_TRY(rle_and_fetch(ctx, (const uint32_t *)ctx->b_taxa.p, (const uint64_t *)j.off.p, (const uint32_t *)j.len.p, j.b.n_reads, j.b.n_bytes + 1,
                         false, j.b.calls, nullptr, j.b.run_off, j.b.run_cnt, n_runs));
    j.runs_in_ctx = true;
  } else {
    *n_runs = ctx->n_runs = total;
    ctx->fetch_runs_src = j.runs.p;
    ctx->last_runs_copied = j.runs_copied;
  }
  *classified = true;  // what follows only concerns the emulation's state
  if (j.sparse && sp.on) {
    if ((uint32_t)h_tot[2]) return fail(KU_ENOMEM, "sparse-mode emulation: the run-wide set is full");
    sp.g_count = std::max<uint64_t>(sp.g_count, h_tot[1]);
    // Units the counting could not settle.  A unit that is still open behind the batch waits (tail form: it is looked at
    // when it closes, with everything it got); a unit in the staged form (it came from a staged batch) is always tracked.
    std::vector<uint32_t> flagged;
    std::vector<uint8_t> flag_all;
    const bool carry_stays_open = j.cont_carry && j.n_units == 1 && j.open_after;
    // The flags are from when the batch's kernels ran -- with several batches in flight, before the exact pass of a batch AHEAD
    // of this one turned dense the very sketch that flags these units (the first units of a run: taxon 0's; without this, every
    // unit of the two batches behind went through the exact evaluation for nothing, 25-75 ms per 10 M reads).  Sketches only ever
    // turn dense, so flagging once more with the state as it is now can only take flags away; the counts are complete (the
    // batch's event), the state is at rest (exact passes end synchronised), and a stream of its own does not queue behind the
    // kernels of the batches in flight.
    bool any_flag = false;
    for (uint32_t u = 0; u < j.n_units; ++u) any_flag |= !(u + 1 == j.n_units && j.open_after) && h_flag[u];
    {
      RleTimes::Lap lap{g_rle.x[0]};
      if (any_flag && !getenv("KU_NO_REFLAG")) {  // (test hook: the flags as the kernels left them)
        // (its own stream: d2h_stream holds the waits for the kernels and the copies back of the batches in flight)
        KU_TRY(ensure_stream(ctx->fetch_stream));
        hipStream_t fs = ctx->fetch_stream;
        const size_t fb = ((size_t)j.n_units + 3) & ~(size_t)3;
        HIP_TRY(hipMemsetAsync(j.u_flag.p, 0, fb, fs));
        KU_TRY(ku_launch_sparse_flag_units((const uint32_t *)j.u_cnt.p, (uint64_t)j.n_units * ctx->tax.n_slots, ctx->tax.n_slots, sp.dev.dense,
                                           (uint8_t *)j.u_flag.p, fs));
        HIP_TRY(hipMemcpyAsync((uint8_t *)j.pin.p + 64, j.u_flag.p, j.n_units, hipMemcpyDeviceToHost, fs));
        HIP_TRY(hipStreamSynchronize(fs));
      }
      for (uint32_t u = 0; u < j.n_units; ++u) {
        const bool open = u + 1 == j.n_units && j.open_after;
        if (u == 0 && j.cont_carry) { flagged.push_back(u); flag_all.push_back(1); }
        else if (!open && h_flag[u]) { flagged.push_back(u); flag_all.push_back(0); }
      }
    }
    if (!flagged.empty()) {
      RleTimes::Lap lap{g_rle.x[1]};
      // as on one stream, where they were queued in front of it: the kernels of the batches in flight come before the exact pass
      // (it closes work units -- sketches turn dense, entries join the run-wide set -- and those kernels read both)
      for (const RleJob &q : ctx->rle)
        if (q.busy && q.kernels_done) HIP_TRY(hipStreamWaitEvent(s, q.kernels_done, 0));
      KU_TRY(sparse_fast_exact(ctx, j, flagged, flag_all, carry_stays_open, s));
      uint64_t n_flagged_reads = 0;
      for (uint32_t u : flagged) n_flagged_reads += j.unit_first_read[u + 1] - j.unit_first_read[u];
      g_rle.count_exact_pass((double)flagged.size(), (double)n_flagged_reads);
    }
  }
  return KU_OK;
}

// every batch in flight is through its kernels AND its copies back (its `done` event): the copy of the run-wide set's size
// into the batch's totals is among those copies
int rle_drain_batches(ku_ctx *ctx) {
  for (RleJob &q : ctx->rle)
    if (q.busy && q.done) HIP_TRY(hipEventSynchronize(q.done));
  return KU_OK;
}

// which of the jobs takes the next batch (they take turns; rle_head is the oldest in flight)
static RleJob &rle_next_job(ku_ctx *ctx) {
  RleJob &j = ctx->rle[(ctx->rle_head + ctx->rle_in_flight) % KU_RLE_MAX_IN_FLIGHT];
  static const int counter_at[KU_RLE_MAX_IN_FLIGHT] = {26, 20, 22, 24};  // (dwords of the context's 32 scalars nobody else uses: dword 2 is
                                                                          // rle_and_fetch's counter, which an overflow redo launches on while batches are in flight)
  if (!j.d_counter) j.d_counter = (unsigned long long *)(ctx->d_scalar + counter_at[&j - &ctx->rle[0]]);
  return j;
}

static int rle_check_batch(RleBatch &b) {
  if ((b.n_bytes && !b.seqs) || (b.n_reads && (!b.seq_off || !b.seq_len || !b.calls || !b.run_off || !b.run_cnt)))
    return fail(KU_EINVAL, "ku_classify_batch_rle: null buffer");
  b.o.flags &= ~KU_F_KEEP_SLOTS;
  RleTimes::Lap lap{g_rle.t[0]};
  if (b.o.max_read_len == 0) for (uint64_t i = 0; i < b.n_reads; ++i) b.o.max_read_len = std::max(b.o.max_read_len, b.seq_len[i]);
  b.monotonic = true;
  for (uint64_t i = 0; i < b.n_reads; ++i) {
    if (b.seq_off[i] + b.seq_len[i] > b.n_bytes) return fail(KU_EINVAL, "read " + std::to_string(i) + " exceeds the sequence buffer");
    if (i && b.seq_off[i] < b.seq_off[i - 1] + b.seq_len[i - 1]) b.monotonic = false;
  }
  return KU_OK;
}

// the one-step paths (quick mode, several databases, sorted layout, shards, reads beyond 65535 k-mers, ...): through the
// context's own buffers, synchronously
static int rle_staged_batch(ku_ctx *ctx, const RleBatch &b, uint64_t *n_runs) {
  const uint64_t n_bytes = b.n_bytes, n_reads = b.n_reads;
  // a run needs at least one k-mer, so n_bytes bounds the number of runs: the device side cannot overflow
  const uint64_t runs_cap = n_bytes + 1;
  if (ctx->b_seqs.reserve(n_bytes + 16) || ctx->b_off.reserve(n_reads * 8) || ctx->b_len.reserve(n_reads * 4) ||
      ctx->b_calls.reserve(n_reads * 4) || ctx->b_taxa.reserve((n_bytes + 16) * 4) || ctx->b_hits.reserve(n_reads * 4) ||
      ctx->b_runs.reserve(runs_cap * 8) || ctx->b_roff.reserve(n_reads * 8) || ctx->b_rcnt.reserve(n_reads * 4))
    return fail(KU_ENOMEM, "device batch buffers");
  hipStream_t s = ctx->stream;
  HIP_TRY(hipMemcpyAsync(ctx->b_seqs.p, b.seqs, n_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ctx->b_off.p, b.seq_off, n_reads * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ctx->b_len.p, b.seq_len, n_reads * 4, hipMemcpyHostToDevice, s));
  KU_TRY(classify_device_impl(ctx, ctx->b_seqs.p, n_bytes, (const uint64_t *)ctx->b_off.p, (const uint32_t *)ctx->b_len.p,
                              n_reads, &b.o, (uint32_t *)ctx->b_calls.p, (uint32_t *)ctx->b_taxa.p,
                              (uint32_t *)ctx->b_hits.p, s, b.seq_off, b.seq_len));
  return rle_and_fetch(ctx, (const uint32_t *)ctx->b_taxa.p, (const uint64_t *)ctx->b_off.p, (const uint32_t *)ctx->b_len.p, n_reads,
                       runs_cap, (b.o.flags & KU_F_QUICK) != 0, b.calls, b.hits, b.run_off, b.run_cnt, n_runs);
}

// A dozen batches of the caller's size class through the whole path, count-less (no state changes), three in flight, from and
// into page-locked memory like the executable's.  What a run's first batches otherwise pay for, as the pipeline trace of
// `classify` showed it one by one (profiles/r05_e2e_sweep.log): the fused kernel's code object; the copy streams' queues (the
// first copy of some hundred KB from the device into page-locked memory on a stream: 23.5 ms -- 4-byte copies go another
// way); each job's events and scratch; scratch memory for the counting instances (they spill a few bytes per lane); and a
// 13 ms ioctl of the runtime's under the first enqueue that follows a finished batch.  Failure is harmless.
static void rle_warm_up(ku_ctx *ctx, uint64_t n_reads) {
  (void)ku_launch_warm_scratch(ctx->n_cu, ctx->stream);
  const RleTimes keep = g_rle;  // (KU_RLE_TIMES: the warm-up's batches are none of the caller's)
  const uint64_t wn = (std::min<uint64_t>(std::max<uint64_t>(n_reads, 1), 65536) + 1) & ~1ull, stride = 101;  // (even: the arrays behind stay 8-byte aligned)
  const size_t per_slot = (size_t)wn * (4 + 4 + 4 + 8) + (size_t)wn * 8 * 8;
  PinBuf w;
  if (w.reserve((size_t)wn * (stride + 12) + KU_RLE_MAX_IN_FLIGHT * per_slot + 4096) == 0) {
    memset(w.p, 0, w.cap);
    char *text = (char *)w.p;
    uint64_t *w_off = (uint64_t *)(text + ((wn * stride + 63) & ~63ull));
    uint32_t *w_len = (uint32_t *)(w_off + wn);
    char *slots = (char *)(w_len + wn);
    for (uint64_t r = 0; r < wn; ++r) {
      char *t = text + r * stride;
      for (int i = 0; i < 100; ++i) t[i] = "ACGTTGCAAGCTTCGA"[(i * 7 + i / 16 + r) & 15];
      t[100] = '\n';
      w_off[r] = r * stride;
      w_len[r] = 100;
    }
    const ku_opts wo = {KU_F_NO_COUNTS, 1, 100, 0};
    uint64_t w_runs = 0;
    int flying = 0;
    for (int rep = 0; rep < 12; ++rep) {
      if (flying == 3) { (void)ku_classify_batch_rle_finish(ctx, &w_runs); --flying; }
      char *sl = slots + (size_t)(rep % KU_RLE_MAX_IN_FLIGHT) * per_slot;
      uint64_t *roff = (uint64_t *)sl;
      uint32_t *calls = (uint32_t *)(roff + wn), *hits = calls + wn, *rcnt = hits + wn;
      ku_run *runs = (ku_run *)(rcnt + wn);
      if (ku_classify_batch_rle_enqueue(ctx, text, wn * stride, w_off, w_len, wn, &wo, calls, hits, roff, rcnt, runs, wn * 8) == KU_OK) ++flying;
    }
    while (flying-- > 0) (void)ku_classify_batch_rle_finish(ctx, &w_runs);
    if (ctx->fetch_stream) {  // (ku_fetch_runs' stream)
      (void)hipMemcpyAsync(w.p, ctx->rle[0].seqs.p, std::min<size_t>(ctx->rle[0].seqs.cap, 1u << 20), hipMemcpyDeviceToHost, ctx->fetch_stream);
      (void)hipStreamSynchronize(ctx->fetch_stream);
    }
    (void)hipDeviceSynchronize();
    w.release();
  }
  (void)hipGetLastError();
  g_rle = keep;
}

// The buffers of `n_jobs` batches of up to n_bytes / n_reads ahead of the first batch (device memory, page-locked scratch,
// streams, events): what _enqueue would otherwise set up inside the caller's timing window, a few milliseconds per job.
extern "C" int ku_classify_batch_rle_reserve(ku_ctx *ctx, uint64_t n_bytes, uint64_t n_reads, uint32_t max_read_len, uint32_t n_jobs) {
  KU_TRY(check_ready(ctx));
  KU_TRY(rle_idle(ctx, "ku_classify_batch_rle_reserve"));
  if (!ku_short_max_kmers(ctx->m.db)) return KU_OK;  // (the fused kernel does not apply: the one-step paths use the context's own buffers)
  KU_TRY(ensure_stream(ctx->h2d_stream));
  KU_TRY(ensure_stream(ctx->d2h_stream));
  KU_TRY(ensure_stream(ctx->fetch_stream));
  const RlePlan p = rle_plan_any_flags(ctx, n_bytes, n_reads, ku_max_kmers(ctx->m.db.k, max_read_len));
  const bool sparse = ctx->sp.on && ctx->sp.unit_nt;
  const uint64_t n_units = sparse ? n_bytes / ctx->sp.unit_nt + 2 : 0;
  for (uint32_t q = 0; q < std::min<uint32_t>(n_jobs, KU_RLE_MAX_IN_FLIGHT); ++q)
    KU_TRY(ctx->rle[q].reserve(n_bytes, n_reads, p.runs_cap, p.ws, 2, sparse, n_units, ctx->tax.n_slots));
  if (sparse && ctx->sp.tail_row.reserve((size_t)ctx->tax.n_slots * 4)) return fail(KU_ENOMEM, "device memory for the work-unit counters");
  if (!getenv("KU_NO_WARMUP")) rle_warm_up(ctx, n_reads);
  return KU_OK;
}

extern "C" int ku_classify_batch_rle_in_flight(const ku_ctx *ctx) { return ctx ? ctx->rle_in_flight : 0; }
extern "C" uint64_t ku_classify_batch_rle_copied(const ku_ctx *ctx) { return ctx ? ctx->last_runs_copied : 0; }

// The batch through the job: its first step (to_end = false: _finish does the second) or both.  No room for the emulation's
// tables: the classification itself does not depend on them (see classify_device_impl), so the emulation is given up and the
// batch goes once more, unless it was classified already; the run goes on with the dense registers alone.
static int rle_run_job(ku_ctx *ctx, RleJob &j, const RleBatch &b, bool to_end, uint64_t *n_runs) {
  for (int attempt = 0;; ++attempt) {
    bool classified = false;
    int st = rle_job_enqueue(ctx, j, b);
    if (to_end && st == KU_OK) st = rle_job_finish(ctx, j, n_runs, &classified);
    if (to_end) j.busy = false;
    if (st != KU_ENOMEM || attempt || !(ctx->sp.on && !(b.o.flags & KU_F_NO_COUNTS))) return st;
    sparse_give_up(ctx);
    if (classified) return KU_OK;
  }
}

extern "C" int ku_classify_batch_rle_enqueue(ku_ctx *ctx, const char *seqs, uint64_t n_bytes, const uint64_t *seq_off,
                                             const uint32_t *seq_len, uint64_t n_reads, const ku_opts *opts, uint32_t *calls,
                                             uint32_t *hits, uint64_t *run_off, uint32_t *run_cnt, ku_run *runs, uint64_t runs_cap) {
  KU_TRY(check_ready(ctx));
  if (ctx->rle_in_flight >= KU_RLE_MAX_IN_FLIGHT)
    return fail(KU_ESTATE, "ku_classify_batch_rle_enqueue: " + std::to_string(KU_RLE_MAX_IN_FLIGHT) + " batches are in flight (ku_classify_batch_rle_finish first)");
  RleBatch b{seqs, n_bytes, seq_off, seq_len, n_reads, opts ? *opts : ku_opts{0, 1, 0, 0}, 0, true, calls, hits, run_cnt, run_off, runs, runs_cap};
  KU_TRY(rle_check_batch(b));
  b.max_n = ku_max_kmers(ctx->m.db.k, b.o.max_read_len);
  RleJob &j = rle_next_job(ctx);
  const bool fused = n_reads && rle_fused_eligible(ctx, b.o.flags, b.max_n, n_bytes, n_reads, b.monotonic);
  // a unit in the staged form (carry buffers) is settled batch by batch, synchronously: such a batch goes in one step, too
  const bool in_steps = fused && !(ctx->sp.on && !(b.o.flags & KU_F_NO_COUNTS) && ctx->sp.open);
  if (in_steps) {
    KU_TRY(rle_run_job(ctx, j, b, /*to_end=*/false, nullptr));
    ++ctx->rle_in_flight;
    return KU_OK;
  }
  if (ctx->rle_in_flight) return fail(KU_ESTATE, "ku_classify_batch_rle_enqueue: this batch takes a path that cannot overlap with the batch in flight "
                                                 "(ku_classify_batch_rle_finish first, then enqueue it again)");
  // classified here and now; _finish hands the totals over
  uint64_t nr = 0;
  ctx->n_runs = 0;
  if (fused) KU_TRY(rle_run_job(ctx, j, b, /*to_end=*/true, &nr));  // (fused, but a unit in the staged form is open)
  else if (n_reads) {
    KU_TRY(rle_staged_batch(ctx, b, &nr));
    j.runs_in_ctx = true;
  }
  j.settled = true;
  j.busy = true;
  j.n_runs = nr;
  j.runs_copied = 0;
  ++ctx->rle_in_flight;
  return KU_OK;
}

extern "C" int ku_classify_batch_rle_finish(ku_ctx *ctx, uint64_t *n_runs) {
  if (!ctx || !n_runs) return fail(KU_EINVAL, "ku_classify_batch_rle_finish: null argument");
  *n_runs = 0;
  if (!ctx->rle_in_flight) return fail(KU_ESTATE, "ku_classify_batch_rle_finish: no batch is in flight");
  KU_TRY(ctx_activate(ctx));
  RleJob &j = ctx->rle[ctx->rle_head];
  ctx->rle_head = (ctx->rle_head + 1) % KU_RLE_MAX_IN_FLIGHT;
  --ctx->rle_in_flight;
  bool classified = false;
  int st = rle_job_finish(ctx, j, n_runs, &classified);
  j.busy = false;
  // the emulation ran out of room behind the classification: it is given up, the run goes on (ku_ctx_sparse_state says 2)
  if (st == KU_ENOMEM && classified && ctx->sp.on) st = sparse_give_up(ctx);
  return st;
}

extern "C" int ku_classify_batch_rle(ku_ctx *ctx, const char *seqs, uint64_t n_bytes, const uint64_t *seq_off,
                                     const uint32_t *seq_len, uint64_t n_reads, const ku_opts *opts, uint32_t *calls,
                                     uint32_t *hits, uint64_t *run_off, uint32_t *run_cnt, uint64_t *n_runs) {
  if (!n_runs) return fail(KU_EINVAL, "ku_classify_batch_rle: null buffer");
  *n_runs = 0;
  KU_TRY(check_ready(ctx));
  KU_TRY(rle_idle(ctx, "ku_classify_batch_rle"));
  KU_TRY(ku_classify_batch_rle_enqueue(ctx, seqs, n_bytes, seq_off, seq_len, n_reads, opts, calls, hits, run_off, run_cnt, nullptr, 0));
  return ku_classify_batch_rle_finish(ctx, n_runs);
}

extern "C" int ku_ctx_replace_calls(ku_ctx *ctx, const uint32_t *new_calls, uint64_t n_reads, uint64_t *n_dropped) {
  KU_TRY(check_ready(ctx));
  if (n_dropped) *n_dropped = 0;
  if (n_reads == 0) return KU_OK;
  if (!new_calls) return fail(KU_EINVAL, "ku_ctx_replace_calls: null argument");
  KU_TRY(rle_idle(ctx, "ku_ctx_replace_calls"));
  if (!ctx->last_calls_dev) return fail(KU_ESTATE, "ku_ctx_replace_calls: the context holds no batch");
  if (ctx->b_hits.reserve(n_reads * 4) != KU_OK) return fail(KU_ENOMEM, "device batch buffers");
  hipStream_t s = ctx->stream;
  unsigned long long *d_dropped = (unsigned long long *)(ctx->d_scalar + 16);
  HIP_TRY(hipMemsetAsync(d_dropped, 0, 8, s));
  HIP_TRY(hipMemcpyAsync(ctx->b_hits.p, new_calls, n_reads * 4, hipMemcpyHostToDevice, s));
  KU_TRY(ku_launch_replace_calls((const uint32_t *)ctx->last_calls_dev, (const uint32_t *)ctx->b_hits.p, n_reads, ctx->d_node_taxid, ctx->tax.n_nodes,
                                 ctx->cnt.n_reads, d_dropped, s));
  HIP_TRY(hipMemcpyAsync((void *)ctx->last_calls_dev, ctx->b_hits.p, n_reads * 4, hipMemcpyDeviceToDevice, s));  // a second replacement starts from these
  unsigned long long dropped = 0;
  HIP_TRY(hipMemcpyAsync(&dropped, d_dropped, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (n_dropped) *n_dropped = dropped;
  return KU_OK;
}

extern "C" int ku_fetch_runs(ku_ctx *ctx, ku_run *runs, uint64_t n_runs) {
  if (!ctx) return fail(KU_EINVAL, "ku_fetch_runs: null context");
  if (n_runs > ctx->n_runs) return fail(KU_EINVAL, "ku_fetch_runs: the last batch holds " + std::to_string(ctx->n_runs) + " runs");
  if (n_runs == 0) return KU_OK;
  if (!runs) return fail(KU_EINVAL, "ku_fetch_runs: null buffer");
  if (!ctx->fetch_runs_src) return fail(KU_ESTATE, "ku_fetch_runs: no batch was classified");
  // (a stream of its own: the copy queues neither behind the kernels of the batch in flight nor behind its copies back,
  // which wait for those kernels)
  KU_TRY(ctx_activate(ctx));
  if (!ctx->fetch_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->fetch_stream, hipStreamNonBlocking));
  HIP_TRY(hipMemcpyAsync(runs, ctx->fetch_runs_src, n_runs * 8, hipMemcpyDeviceToHost, ctx->fetch_stream));
  HIP_TRY(hipStreamSynchronize(ctx->fetch_stream));
  return KU_OK;
}
