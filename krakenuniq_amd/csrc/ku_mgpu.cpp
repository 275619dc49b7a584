// ku_mgpu.cpp -- the classify hot path over several GPUs: host C++ over the C ABI + RCCL (include/krakenuniq_amd.h,
// "several GPUs").  One host thread per rank; the database is sharded by minimizer-bin range (the reference's
// --preload-size partitioning, krakendb.cpp:430-526, laid out in space instead of in time).  Default exchange: OWNER
// ROUTING (RoutedStep) -- a rank scans its slice of the reads, runs of k-mers travel as 16-byte records to the rank
// that owns their bin, one slot per k-mer comes back.  Kept beside it: the position-wise exchange -- read batches are
// broadcast, per-k-mer slots are max-reduced ("non-zero wins", classify.cpp:445-452) and scattered over the read dimension.
// Either way every rank resolves its slice (classify.cpp:676-785), the per-taxon state is reduced at the end of the run.
//
// One translation unit in four files (the -DKU_TEST_HOOKS build of tests/rccl_shim compiles this file once more; both of
// its hooks live in the headers):
//   ku_mgpu_comm.h    the two exchange back ends: RCCL binding, the group (struct ku_mgpu), run_all, the primitives (comm_*)
//   ku_route_plan.h   where the routed step cuts a slice into rounds: plain host C++, checked without a device
//   ku_mgpu_route.h   the routed step (RoutedStep: the stages of a round, two streams)
//   ku_mgpu.cpp       the C ABI entry points, the position-wise step (rank_step_sharded), the host-batch call
//
// THE PROTOCOL of the same-process exchange (exchange() in ku_mgpu_comm.h is its only implementation): a step is a fixed
// sequence of collectives, and every rank makes every one of them whatever its own status -- a thread that returned early
// would leave the others in a barrier for ever.  So a primitive takes the rank's status and returns the status behind the
// exchange.  Inside, every rank passes the same barriers; a rank that has failed says so in the shared flag before a
// barrier; copies and merges run only on a rank that is well while no rank has said it failed; a phase that queued device
// work waits for its stream; behind the last barrier a rank that was well leaves with KU_ESTATE if any rank failed.  What
// one rank alone can find wrong beforehand (a null buffer of its own) is checked before run_all starts a thread.  Over RCCL
// the ranks of one process agree the same way in front of a collective (rccl_gate); ranks in several processes cannot.
#include <set>

#include "ku_mgpu_route.h"

// ---------------------------------------------------------------------------- life cycle
extern "C" int ku_mgpu_unique_id(uint8_t *id) {
  if (!id) return mfail(KU_EINVAL, "ku_mgpu_unique_id: null argument");
  M_TRY(rccl_ready());
  static_assert(sizeof(ncclUniqueId) == KU_MGPU_ID_BYTES, "RCCL unique id size");
  ncclUniqueId u;
  M_NCCL(g_rccl.GetUniqueId(&u));
  memcpy(id, &u, sizeof u);
  return KU_OK;
}

extern "C" void ku_mgpu_destroy(ku_mgpu *m) {
  if (!m) return;
  for (auto &r : m->ranks) {
    (void)hipSetDevice(r.device);
    if (r.ctx) (void)ku_ctx_synchronize(r.ctx);
    if (r.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(r.comm);
    r.release();
    if (r.ctx) ku_ctx_destroy(r.ctx);
  }
  if (m->sh.bar_init) pthread_barrier_destroy(&m->sh.bar);
  delete m;
}

extern "C" int ku_mgpu_create(const int *devices, uint32_t n_local, uint32_t first_rank, uint32_t world, const uint8_t *id,
                              uint32_t flags, ku_mgpu **out) {
  if (!out || !devices || n_local == 0 || world == 0 || first_rank + n_local > world)
    return mfail(KU_EINVAL, "ku_mgpu_create: bad rank layout");
  *out = nullptr;
  const bool all_here = first_rank == 0 && n_local == world;
  if (!all_here && !id) return mfail(KU_EINVAL, "ku_mgpu_create: a world that spans processes needs the unique id of rank 0");
  if (!all_here && n_local != 1) return mfail(KU_EUNSUP, "ku_mgpu_create: one rank per process, or all ranks in one process");
  ku_mgpu *m = new ku_mgpu();
  m->world = world;
  m->first_rank = first_rank;
  m->n_local = n_local;
  m->flags = flags;
  m->ranks.resize(n_local);
  for (auto *v : {&m->sh.ptr_a, &m->sh.ptr_b, &m->sh.ptr_c}) v->assign(n_local, nullptr);
  m->sh.vals.resize(n_local);
  m->sh.u64s.resize(n_local);
  m->sh.offs.assign(n_local, nullptr);
  m->sh.dev.assign(devices, devices + n_local);
  std::set<int> distinct(devices, devices + n_local);
  // KU_MGPU_FORCE_RCCL=1 takes the RCCL calls even for a world of one rank (a way to exercise them on a 1-GPU box)
  m->use_rccl = (world > 1 || getenv("KU_MGPU_FORCE_RCCL")) &&
                (!all_here || (distinct.size() == n_local && !(flags & KU_MGPU_NO_RCCL)));
  if (n_local > 1) {
    if (pthread_barrier_init(&m->sh.bar, nullptr, n_local) != 0) { delete m; return mfail(KU_ENOMEM, "pthread_barrier_init"); }
    m->sh.bar_init = true;
  }
  for (uint32_t i = 0; i < n_local; ++i) {
    auto &r = m->ranks[i];
    r.rank = first_rank + i;
    r.local = i;
    r.device = devices[i];
    int st = ku_ctx_create(devices[i], &r.ctx);
    if (st != KU_OK) { ku_mgpu_destroy(m); return st; }
  }
  if (m->use_rccl) {
    int st = rccl_ready();
    if (st != KU_OK) { ku_mgpu_destroy(m); return st; }
    if (all_here && !(id && n_local == 1)) {
      std::vector<ncclComm_t> comms(n_local);
      ncclResult_t e = g_rccl.CommInitAll(comms.data(), (int)n_local, devices);
      if (e != ncclSuccess) { ku_mgpu_destroy(m); return mfail(KU_EHIP, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(e)); }
      for (uint32_t i = 0; i < n_local; ++i) m->ranks[i].comm = comms[i];
    } else {
      ncclUniqueId u;
      memcpy(&u, id, sizeof u);
      if (hipSetDevice(devices[0]) != hipSuccess) { ku_mgpu_destroy(m); return mfail(KU_EHIP, "hipSetDevice failed"); }
      ncclResult_t e = g_rccl.CommInitRank(&m->ranks[0].comm, (int)world, u, (int)first_rank);
      if (e != ncclSuccess) { ku_mgpu_destroy(m); return mfail(KU_EHIP, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(e)); }
    }
  }
  *out = m;
  return KU_OK;
}

extern "C" ku_ctx *ku_mgpu_ctx(ku_mgpu *m, uint32_t local_index) {
  return (m && local_index < m->n_local) ? m->ranks[local_index].ctx : nullptr;
}
extern "C" int ku_mgpu_uses_rccl(const ku_mgpu *m) { return m && m->use_rccl ? 1 : 0; }
extern "C" int ku_mgpu_uses_routing(const ku_mgpu *m) { return m && m->route && !m->exact ? 1 : 0; }

extern "C" int ku_mgpu_set_timing(ku_mgpu *m, int on) {
  if (!m) return mfail(KU_EINVAL, "ku_mgpu_set_timing: null argument");
  m->timing = on != 0;
  return KU_OK;
}
extern "C" int ku_mgpu_step_times(ku_mgpu *m, uint32_t local_index, double *out) {
  if (!m || !out || local_index >= m->n_local) return mfail(KU_EINVAL, "ku_mgpu_step_times: bad argument");
  ku_mgpu::Rank &r = m->ranks[local_index];
  for (int i = 0; i < 6; ++i) out[i] = 0;
  if (hipSetDevice(r.device) != hipSuccess) return mfail(KU_EHIP, "hipSetDevice failed");
  for (auto &t : r.tev) {
    float ms = 0;
    if (hipEventSynchronize(t.second.second) != hipSuccess || hipEventElapsedTime(&ms, t.second.first, t.second.second) != hipSuccess)
      return mfail(KU_EHIP, "ku_mgpu_step_times: an event of the last step is not complete");
    if (t.first >= 0 && t.first < 3) out[t.first] += ms;
  }
  out[3] = r.t_rounds;
  out[4] = r.t_rec;
  out[5] = r.t_kmers;
  return KU_OK;
}

extern "C" int ku_mgpu_set_taxonomy(ku_mgpu *m, const ku_tax *tax) {
  if (!m || !tax) return mfail(KU_EINVAL, "ku_mgpu_set_taxonomy: null argument");
  M_TRY(ranks_idle(m, "ku_mgpu_set_taxonomy"));
  M_TRY(run_all(m, [&](ku_mgpu::Rank &r) -> int {
    uint64_t n = 0;
    int st = ku_ctx_db_values(r.ctx, nullptr, &n);
    std::vector<uint32_t> mine(st == KU_OK ? n : 0), all;
    if (st == KU_OK && n) st = ku_ctx_db_values(r.ctx, mine.data(), &n);
    st = comm_allgather_values(m, r, st, mine, all);
    if (st != KU_OK) return st;
    st = ku_ctx_set_taxonomy(r.ctx, tax, all.data(), all.size());
    // owner routing needs every rank's minimizer range and the probe table everywhere
    uint64_t info[4] = {0, 0, 0, 0};
    int is_hash = 0, single = 0;
    if (st == KU_OK) st = ku_ctx_route_info(r.ctx, &info[0], &info[1], &is_hash, &single);
    info[2] = (uint64_t)(is_hash && single);
    std::vector<uint64_t> allinfo;
    st = comm_allgather_u64(m, r, st, info, 4, allinfo, ku_ctx_stream_of(r.ctx));
    if (st == KU_OK && r.local == 0) {
      m->own_lo.assign(m->world, 0);
      m->own_hi.assign(m->world, 0);
      bool ok = true;
      for (uint32_t q = 0; q < m->world; ++q) { m->own_lo[q] = allinfo[4 * q]; m->own_hi[q] = allinfo[4 * q + 1]; ok = ok && allinfo[4 * q + 2]; }
      // the scan finds a bin's owner by bisection: the ranges must ascend with the rank (a shard plan's do) and not overlap
      for (uint32_t q = 0; q + 1 < m->world; ++q) ok = ok && m->own_lo[q] <= m->own_hi[q] && m->own_hi[q] <= m->own_lo[q + 1];
      if (std::getenv("KU_ROUTE_DEBUG")) {
        fprintf(stderr, "[ku_route] rank %u: hash+single everywhere / ascending ranges: %d;", r.rank, (int)ok);
        for (uint32_t q = 0; q < m->world; ++q) fprintf(stderr, " [%llu, %llu) flag %llu", (unsigned long long)m->own_lo[q], (unsigned long long)m->own_hi[q], (unsigned long long)allinfo[4 * q + 2]);
        fprintf(stderr, "\n");
      }
      const char *ex = getenv("KU_MGPU_EXCHANGE");
      // (KU_MGPU_FORCE_ROUTE=1: also a world of one rank takes the routed path -- scan, records, owner kernel, gather on one
      // stream, nothing on the wire: the device work of a routed step in one clean kernel trace)
      m->ring_reduce = ex && !strcmp(ex, "reduce");
      m->route = ok && (m->world > 1 || std::getenv("KU_MGPU_FORCE_ROUTE")) && m->world <= 64 && !(m->flags & KU_MGPU_REPLICAS) && !(ex && (!strcmp(ex, "slots") || m->ring_reduce));
    }
    return st;
  }));
  m->tax_set = true;
  return KU_OK;
}

extern "C" int ku_mgpu_load_dbs(ku_mgpu *m, const ku_db *const *dbs, uint32_t n_dbs, const ku_tax *tax) {
  if (!m || !dbs || !n_dbs || !tax) return mfail(KU_EINVAL, "ku_mgpu_load_dbs: null argument");
  M_TRY(ranks_idle(m, "ku_mgpu_load_dbs"));
  if (n_dbs == 1) return ku_mgpu_load(m, dbs[0], tax);
  // several databases are searched one after the other per k-mer, the first hit wins (classify.cpp:928-936): with the
  // first database cut into shards a later one could not tell whether another rank had found the k-mer already -- the
  // reference's own chunk mode only searches the first database (classify.cpp:639).  Replicas hold everything.
  if (!(m->flags & KU_MGPU_REPLICAS)) return mfail(KU_EUNSUP, "several databases on several GPUs need the replicas mode (KU_MGPU_REPLICAS)");
  ku_db_info info;
  M_TRY(ku_db_get_info(dbs[0], &info));
  M_TRY(run_all(m, [&](ku_mgpu::Rank &r) -> int {
    M_TRY(ku_ctx_load_db(r.ctx, dbs[0], 0, info.n_bins));
    for (uint32_t i = 1; i < n_dbs; ++i) M_TRY(ku_ctx_add_db(r.ctx, dbs[i]));
    return KU_OK;
  }));
  m->loaded = true;
  return ku_mgpu_set_taxonomy(m, tax);
}

extern "C" int ku_mgpu_load(ku_mgpu *m, const ku_db *db, const ku_tax *tax) {
  if (!m || !db || !tax) return mfail(KU_EINVAL, "ku_mgpu_load: null argument");
  M_TRY(ranks_idle(m, "ku_mgpu_load"));
  ku_db_info info;
  M_TRY(ku_db_get_info(db, &info));
  std::vector<uint64_t> bounds(m->world + 1);
  M_TRY(ku_db_shard_plan(db, m->world, bounds.data()));
  const bool replicas = (m->flags & KU_MGPU_REPLICAS) != 0;
  M_TRY(run_all(m, [&](ku_mgpu::Rank &r) -> int {
    return replicas ? ku_ctx_load_db(r.ctx, db, 0, info.n_bins) : ku_ctx_load_db(r.ctx, db, bounds[r.rank], bounds[r.rank + 1]);
  }));
  m->loaded = true;
  return ku_mgpu_set_taxonomy(m, tax);
}

// ---------------------------------------------------------------------------- report modes over the group
extern "C" int ku_mgpu_enable_sparse(ku_mgpu *m, uint64_t work_unit_nt, uint32_t global_log2) {
  if (!m) return mfail(KU_EINVAL, "ku_mgpu_enable_sparse: null argument");
  M_TRY(ranks_idle(m, "ku_mgpu_enable_sparse"));
  if (!m->tax_set) return mfail(KU_ESTATE, "ku_mgpu_enable_sparse: load the database and the taxonomy first");
  if (!single_process(m)) return mfail(KU_EUNSUP, "the sparse-mode emulation over several GPUs needs the group in one process");
  if (work_unit_nt == 0) return mfail(KU_EUNSUP, "ku_mgpu_enable_sparse: a work unit size is needed (the ranks take whole units)");
  M_TRY(run_all(m, [&](ku_mgpu::Rank &r) -> int { return ku_ctx_enable_sparse(r.ctx, work_unit_nt, global_log2); }));
  m->sparse = true;
  m->unit_nt = work_unit_nt;
  m->acc_nt = 0;
  m->open_rank = -1;
  return KU_OK;
}
extern "C" int ku_mgpu_sparse_close_unit(ku_mgpu *m) {
  if (!m) return mfail(KU_EINVAL, "ku_mgpu_sparse_close_unit: null argument");
  M_TRY(ranks_idle(m, "ku_mgpu_sparse_close_unit"));
  if (!m->sparse) return KU_OK;
  if (m->open_rank >= 0) {
    ku_mgpu::Rank &r = m->ranks[m->open_rank];
    if (hipSetDevice(r.device) != hipSuccess) return mfail(KU_EHIP, "hipSetDevice failed");
    M_TRY(ku_sparse_close_unit(r.ctx));
  }
  m->acc_nt = 0;
  m->open_rank = -1;
  return KU_OK;
}
extern "C" int ku_mgpu_sparse_state(const ku_mgpu *m) {
  if (!m) return 0;
  int worst = m->sparse_gave_up ? 2 : (m->sparse ? 1 : 0);
  for (const auto &r : m->ranks) {
    const int s = ku_ctx_sparse_state(r.ctx);
    if (s == 2) worst = 2;
  }
  return worst;
}
extern "C" int ku_mgpu_enable_exact(ku_mgpu *m, uint32_t capacity_log2) {
  if (!m) return mfail(KU_EINVAL, "ku_mgpu_enable_exact: null argument");
  M_TRY(ranks_idle(m, "ku_mgpu_enable_exact"));
  if (!m->tax_set) return mfail(KU_ESTATE, "ku_mgpu_enable_exact: load the database and the taxonomy first");
  // owner-computes: a k-mer is put into the set of the rank that owns its minimizer bin, so the ranks' sets are disjoint
  // and the distinct counts add up.  Replicas would see the same k-mer on several ranks.
  if (m->flags & KU_MGPU_REPLICAS) return mfail(KU_EUNSUP, "exact counting over several GPUs needs the sharded mode (the k-mer set is partitioned by owner)");
  M_TRY(run_all(m, [&](ku_mgpu::Rank &r) -> int { return ku_ctx_enable_exact(r.ctx, capacity_log2); }));
  m->exact = true;
  return KU_OK;
}

// ---------------------------------------------------------------------------- one batch
namespace {
// A rank ran out of memory for the emulation's tables and switched it off there: no rank's sets are the run's any more.
// The emulation is given up for the whole group, which goes on with the dense registers (no unit bookkeeping, no open unit
// to move -- ku_ctx_sparse_move_open_unit would refuse a context without tables and take the run down);
// ku_mgpu_sparse_state keeps saying 2, the report carries its estimates and says so.
int sparse_give_up_group(ku_mgpu *m) {
  for (auto &r : m->ranks) {
    if (hipSetDevice(r.device) != hipSuccess) return mfail(KU_EHIP, "hipSetDevice failed");
    if (ku_ctx_sparse_on(r.ctx)) M_TRY(ku_ctx_disable_sparse(r.ctx));
  }
  m->sparse = false;
  m->sparse_gave_up = true;
  m->open_rank = -1;
  m->acc_nt = 0;
  return KU_OK;
}

// the sharded batch on one rank, everything on stream s: broadcast, lookup of the owned k-mers, slot merge, resolve
int rank_step_sharded(ku_mgpu *m, ku_mgpu::Rank &r, int st, void *d_seqs, uint64_t *d_off, uint32_t *d_len, uint32_t *d_calls,
                      uint32_t *d_taxa, uint32_t *d_hits, uint64_t n_bytes, uint64_t n_reads, const uint64_t *rb,
                      const uint64_t *pos, const ku_opts &opts, hipStream_t s, const uint64_t *h_off = nullptr,
                      const uint32_t *h_len = nullptr) {
  st = comm_broadcast(m, r, st, d_seqs, n_bytes, s);
  st = comm_broadcast(m, r, st, d_off, n_reads * 8, s);
  st = comm_broadcast(m, r, st, d_len, n_reads * 4, s);
  ku_opts lo = opts;
  lo.flags = (opts.flags & ~KU_F_MERGE_CHUNK) | KU_F_KEEP_SLOTS;
  if (st == KU_OK && m->exact) {
    // classifyExact: the k-mers this rank OWNS go into its set.  The lookup runs as a chunk pass over an array preset with
    // a mark (positions of other owners keep it), the set takes what is not marked, the marks become 0 for the exchange
    st = ku_exact_owned_step(r.ctx, d_seqs, d_off, d_len, n_reads, n_bytes, &lo, d_taxa, s);
  } else if (st == KU_OK) st = ku_lookup_device(r.ctx, d_seqs, n_bytes, &lo, d_taxa, s);
  st = comm_reduce_slices_max(m, r, st, d_taxa, pos, s);
  if (st != KU_OK) return st;
  const uint64_t r0 = rb[r.rank], nr = rb[r.rank + 1] - r0;
  ku_opts ro = opts;
  ro.flags &= ~(KU_F_KEEP_SLOTS | KU_F_MERGE_CHUNK);
  if (nr == 0) return KU_OK;
  if (m->sparse && h_len && !(opts.flags & KU_F_NO_COUNTS))  // the rank's slice is whole work units: its merged slots feed the emulation
    M_TRY(ku_ctx_sparse_pass_slots(r.ctx, d_seqs, d_off + r0, d_len + r0, h_off + r0, h_len + r0, nr, n_bytes, d_taxa,
                                   (opts.flags & KU_F_QUICK) ? std::max(1u, opts.min_hits) : 0u, s));
  return ku_resolve_device(r.ctx, d_seqs, d_off + r0, d_len + r0, nr, &ro, d_calls + r0, d_taxa, d_hits ? d_hits + r0 : nullptr, s);
}
}  // namespace

extern "C" int ku_mgpu_step_device(ku_mgpu *m, const ku_mgpu_dev_batch *local, uint64_t n_bytes, uint64_t n_reads,
                                   const uint64_t *read_bounds, const uint64_t *pos_bounds, const ku_opts *opts) {
  if (!m || !local || !read_bounds || !pos_bounds) return mfail(KU_EINVAL, "ku_mgpu_step_device: null argument");
  M_TRY(ranks_idle(m, "ku_mgpu_step_device"));
  if (!m->tax_set) return mfail(KU_ESTATE, "ku_mgpu_step_device: load the database and the taxonomy first");
  if (m->flags & KU_MGPU_REPLICAS) return mfail(KU_EINVAL, "ku_mgpu_step_device is the sharded step; replicas classify through their own contexts");
  for (uint32_t i = 0; i < m->n_local; ++i)  // (in front of the threads: a rank that left alone would leave the others waiting)
    if (n_bytes && (!local[i].d_seqs || !local[i].d_taxa)) return mfail(KU_EINVAL, "ku_mgpu_step_device: null buffer");
  const ku_opts o = opts ? *opts : ku_opts{0, 1, 0, 0};
  m->reduced = false;
  return run_all(m, [&](ku_mgpu::Rank &r) -> int {
    const ku_mgpu_dev_batch &b = local[r.local];
    hipStream_t s = b.stream ? (hipStream_t)b.stream : ku_ctx_stream_of(r.ctx);
    if (m->route && !m->exact)
      return RoutedStep{m, r, KU_OK, b.d_seqs, b.d_seq_off, b.d_seq_len, b.d_calls, b.d_taxa, nullptr, n_bytes, read_bounds, pos_bounds, o, s, nullptr, nullptr}
          .run(false);
    return rank_step_sharded(m, r, KU_OK, b.d_seqs, b.d_seq_off, b.d_seq_len, b.d_calls, b.d_taxa, nullptr, n_bytes, n_reads,
                             read_bounds, pos_bounds, o, s);
  });
}

extern "C" int ku_mgpu_classify_batch_rle(ku_mgpu *m, const char *seqs, uint64_t n_bytes, const uint64_t *seq_off,
                                          const uint32_t *seq_len, uint64_t n_reads, const ku_opts *opts, uint32_t *calls,
                                          uint32_t *hits, uint64_t *run_off, uint32_t *run_cnt, uint64_t *n_runs) {
  if (!m || !n_runs || (n_bytes && !seqs) || (n_reads && (!seq_off || !seq_len || !calls || !run_off || !run_cnt)))
    return mfail(KU_EINVAL, "ku_mgpu_classify_batch_rle: null argument");
  M_TRY(ranks_idle(m, "ku_mgpu_classify_batch_rle"));
  if (!single_process(m)) return mfail(KU_EUNSUP, "host batches go through a single-process group");
  if (!m->tax_set) return mfail(KU_ESTATE, "ku_mgpu_classify_batch_rle: load the database and the taxonomy first");
  *n_runs = 0;
  for (auto &r : m->ranks) r.n_runs = r.run_base = 0;
  if (n_reads == 0) return KU_OK;
  m->reduced = false;
  ku_opts o = opts ? *opts : ku_opts{0, 1, 0, 0};
  o.flags &= ~(KU_F_KEEP_SLOTS | KU_F_MERGE_CHUNK);
  uint32_t max_len = 0;
  for (uint64_t i = 0; i < n_reads; ++i) {
    if (seq_off[i] + seq_len[i] > n_bytes) return mfail(KU_EINVAL, "read " + std::to_string(i) + " exceeds the sequence buffer");
    if (i && seq_off[i] < seq_off[i - 1]) return mfail(KU_EINVAL, "ku_mgpu_classify_batch_rle: reads must be in buffer order");
    max_len = std::max(max_len, seq_len[i]);
  }
  o.max_read_len = max_len;
  const bool replicas = (m->flags & KU_MGPU_REPLICAS) != 0, quick = (o.flags & KU_F_QUICK) != 0;
  // slices of the read dimension, balanced by bytes and cut at read boundaries -- with the sparse-mode emulation on, at
  // WORK UNIT boundaries (a unit closes behind the read that fills it, classify.cpp:510-521): every rank then runs the
  // emulation on whole units; the unit that is still open when the batch ends continues on rank 0 with the next batch
  const uint32_t W = m->world;
  std::vector<uint64_t> rb(W + 1), pos(W + 1);
  if (m->sparse && ku_mgpu_sparse_state(m) == 2) M_TRY(sparse_give_up_group(m));
  const bool sparse = m->sparse && !(o.flags & KU_F_NO_COUNTS);
  rb[0] = 0;
  if (sparse) {
    if (m->open_rank > 0) {  // the open unit's state moves to the rank that takes the first reads
      M_TRY(ku_ctx_sparse_move_open_unit(m->ranks[m->open_rank].ctx, m->ranks[0].ctx));
      m->open_rank = 0;
    }
    std::vector<uint64_t> unit_end;  // read indices behind which a unit closes
    uint64_t acc = m->acc_nt;
    for (uint64_t i = 0; i < n_reads; ++i) {
      acc += seq_len[i];
      if (acc >= m->unit_nt) { unit_end.push_back(i + 1); acc = 0; }
    }
    for (uint32_t q = 1; q < W; ++q) {
      const uint64_t target = n_bytes / W * q;
      // the first unit boundary at or behind the target byte (none: the rest of the batch is one rank's)
      auto it = std::lower_bound(unit_end.begin(), unit_end.end(), target, [&](uint64_t e, uint64_t t) { return (e < n_reads ? seq_off[e] : n_bytes) < t; });
      rb[q] = std::max<uint64_t>(rb[q - 1], it == unit_end.end() ? n_reads : *it);
    }
    m->acc_nt = acc;
  } else {
    for (uint32_t q = 1; q < W; ++q) {
      const uint64_t target = n_bytes / W * q;
      rb[q] = std::max<uint64_t>(rb[q - 1], (uint64_t)(std::lower_bound(seq_off, seq_off + n_reads, target) - seq_off));
    }
  }
  rb[W] = n_reads;
  for (uint32_t q = 0; q < W; ++q) pos[q] = rb[q] < n_reads ? seq_off[rb[q]] : n_bytes;
  pos[0] = 0;
  pos[W] = n_bytes;
  if (sparse) {  // where the open unit (if any) ends up: the last rank that got reads
    m->open_rank = -1;
    if (m->acc_nt > 0)
      for (uint32_t q = 0; q < W; ++q)
        if (rb[q + 1] > rb[q]) m->open_rank = (int)q;
  }
  std::vector<uint64_t> totals(W, 0);
  M_TRY(run_all(m, [&](ku_mgpu::Rank &r) -> int {
    hipStream_t s = ku_ctx_stream_of(r.ctx);
    const uint64_t r0 = rb[r.rank], nr = rb[r.rank + 1] - r0;
    // what this rank keeps resident: the whole batch (sharded: every rank scans everything) or its slice (replicas)
    const uint64_t b0 = replicas ? pos[r.rank] : 0, nb = replicas ? pos[r.rank + 1] - b0 : n_bytes;
    const uint64_t nq = replicas ? nr : n_reads;
    const uint64_t runs_cap = (replicas ? nb : pos[r.rank + 1] - pos[r.rank]) + 1;
    int st = KU_OK;
    if (!replicas && (r.seqs.reserve(nb + 16) || r.off.reserve(nq * 8 + 8) || r.len.reserve(nq * 4 + 4) || r.calls.reserve(nq * 4 + 4) ||
                      r.taxa.reserve((nb + 16) * 4) || r.hits.reserve(nq * 4 + 4) || r.runs.reserve(runs_cap * 8) ||
                      r.roff.reserve(nq * 8 + 8) || r.rcnt.reserve(nq * 4 + 4) || r.small.reserve(64)))
      st = mfail(KU_ENOMEM, "device memory for the batch");
    uint32_t *d_calls = (uint32_t *)r.calls.p, *d_hits = (uint32_t *)r.hits.p, *d_taxa = (uint32_t *)r.taxa.p;
    uint64_t *d_off = (uint64_t *)r.off.p;
    uint32_t *d_len = (uint32_t *)r.len.p;
    if (replicas) {
      // a replica is a whole single-GPU pipeline on its slice: the context's own host-buffer entry point (fused kernel with
      // run-length encoded output, the slice uploaded in segments under the kernels, the emulation's fast path)
      if (nr == 0) return KU_OK;
      std::vector<uint64_t> rel(nr);  // slice offsets are relative to the slice's first byte
      for (uint64_t i = 0; i < nr; ++i) rel[i] = seq_off[r0 + i] - b0;
      uint64_t nruns = 0;
      M_TRY(ku_classify_batch_rle(r.ctx, seqs + b0, nb, rel.data(), seq_len + r0, nr, &o, calls + r0, hits ? hits + r0 : nullptr, run_off + r0,
                                  run_cnt + r0, &nruns));
      totals[r.rank] = nruns;
      return KU_OK;
    } else if (m->route && !m->exact) {
      // owner routing: every rank takes its own slice of the host batch over its own PCIe link (no broadcast at all)
      const uint64_t p0 = pos[r.rank], pb = pos[r.rank + 1] - p0;
      if (st == KU_OK && ((pb && hipMemcpyAsync((char *)r.seqs.p + p0, seqs + p0, pb, hipMemcpyHostToDevice, s) != hipSuccess) ||
                          (nr && (hipMemcpyAsync(d_off + r0, seq_off + r0, nr * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
                                  hipMemcpyAsync(d_len + r0, seq_len + r0, nr * 4, hipMemcpyHostToDevice, s) != hipSuccess))))
        st = mfail(KU_EHIP, "upload of the batch failed");
      st = RoutedStep{m, r, st, r.seqs.p, d_off, d_len, d_calls, d_taxa, d_hits, n_bytes, rb.data(), pos.data(), o, s, seq_off, seq_len}.run(true);
    } else {
      if (st == KU_OK && r.rank == 0 &&
          (hipMemcpyAsync(r.seqs.p, seqs, n_bytes, hipMemcpyHostToDevice, s) != hipSuccess ||
           hipMemcpyAsync(d_off, seq_off, n_reads * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
           hipMemcpyAsync(d_len, seq_len, n_reads * 4, hipMemcpyHostToDevice, s) != hipSuccess))
        st = mfail(KU_EHIP, "upload of the batch failed");
      st = rank_step_sharded(m, r, st, r.seqs.p, d_off, d_len, d_calls, d_taxa, d_hits, n_bytes, n_reads, rb.data(),
                             pos.data(), o, s, seq_off, seq_len);
    }
    if (st != KU_OK) return st;
    if (nr == 0) return KU_OK;
    // run-length encoding of this rank's reads; (run_off, run_cnt) index the rank's own run array
    const uint64_t lq = replicas ? 0 : r0;  // index of the slice's first read in this rank's arrays
    unsigned long long *d_counter = (unsigned long long *)r.small.p;
    if (quick) {
      M_HIP(hipMemsetAsync(d_counter, 0, 8, s));
      M_HIP(hipMemsetAsync((uint64_t *)r.roff.p + lq, 0, nr * 8, s));
      M_HIP(hipMemsetAsync((uint32_t *)r.rcnt.p + lq, 0, nr * 4, s));
    } else {
      M_TRY(ku_launch_rle(d_taxa, ku_ctx_k_of(r.ctx), d_off + lq, d_len + lq, nr, runs_cap /* ~ bases */, r.runs.p, runs_cap, d_counter,
                          (uint64_t *)r.roff.p + lq, (uint32_t *)r.rcnt.p + lq, ku_ctx_cus_of(r.ctx), s));
    }
    unsigned long long total = 0;
    M_HIP(hipMemcpyAsync(&total, d_counter, 8, hipMemcpyDeviceToHost, s));
    M_HIP(hipMemcpyAsync(calls + r0, d_calls + lq, nr * 4, hipMemcpyDeviceToHost, s));
    if (hits) M_HIP(hipMemcpyAsync(hits + r0, d_hits + lq, nr * 4, hipMemcpyDeviceToHost, s));
    M_HIP(hipMemcpyAsync(run_off + r0, (uint64_t *)r.roff.p + lq, nr * 8, hipMemcpyDeviceToHost, s));
    M_HIP(hipMemcpyAsync(run_cnt + r0, (uint32_t *)r.rcnt.p + lq, nr * 4, hipMemcpyDeviceToHost, s));
    M_HIP(hipStreamSynchronize(s));
    if (total > runs_cap) return mfail(KU_EHIP, "run-length encoder overflowed its bound");
    totals[r.rank] = total;
    return KU_OK;
  }));
  // one run array for the caller: rank r's runs follow those of the ranks before it
  uint64_t base = 0;
  for (uint32_t q = 0; q < W; ++q) {
    m->ranks[q].run_base = base;
    m->ranks[q].n_runs = totals[q];
    if (base)
      for (uint64_t i = rb[q]; i < rb[q + 1]; ++i) run_off[i] += base;
    base += totals[q];
  }
  *n_runs = base;
  return KU_OK;
}

extern "C" int ku_mgpu_fetch_runs(ku_mgpu *m, ku_run *runs, uint64_t n_runs) {
  if (!m) return mfail(KU_EINVAL, "ku_mgpu_fetch_runs: null argument");
  uint64_t total = 0;
  for (auto &r : m->ranks) total += r.n_runs;
  if (n_runs > total) return mfail(KU_EINVAL, "ku_mgpu_fetch_runs: the last batch holds " + std::to_string(total) + " runs");
  if (n_runs == 0) return KU_OK;
  if (!runs) return mfail(KU_EINVAL, "ku_mgpu_fetch_runs: null buffer");
  return run_all(m, [&](ku_mgpu::Rank &r) -> int {
    if (r.run_base >= n_runs || r.n_runs == 0) return KU_OK;
    const uint64_t n = std::min(r.n_runs, n_runs - r.run_base);
    if (m->flags & KU_MGPU_REPLICAS) return ku_fetch_runs(r.ctx, runs + r.run_base, n);  // the runs lie in the rank's context
    hipStream_t s = ku_ctx_stream_of(r.ctx);
    M_HIP(hipMemcpyAsync(runs + r.run_base, r.runs.p, n * 8, hipMemcpyDeviceToHost, s));
    M_HIP(hipStreamSynchronize(s));
    return KU_OK;
  });
}

extern "C" int ku_mgpu_reduce_state(ku_mgpu *m, void *const *streams) {
  if (!m) return mfail(KU_EINVAL, "ku_mgpu_reduce_state: null argument");
  M_TRY(ranks_idle(m, "ku_mgpu_reduce_state"));
  if (!m->tax_set) return mfail(KU_ESTATE, "ku_mgpu_reduce_state: no taxonomy set");
  if (m->reduced) return mfail(KU_ESTATE, "ku_mgpu_reduce_state: the state is reduced already (another call would add the counters again)");
  M_TRY(run_all(m, [&](ku_mgpu::Rank &r) -> int {
    hipStream_t s = (streams && streams[r.local]) ? (hipStream_t)streams[r.local] : ku_ctx_stream_of(r.ctx);
    int st = comm_allreduce_state(m, r, s);
    return m->exact ? comm_allreduce_exact(m, r, st, s) : st;
  }));
  bool degraded = m->sparse && ku_mgpu_sparse_state(m) != 1;
  if (m->sparse && !degraded) {
    // the emulation's state of the whole run ends up in rank 0's context: the last unit closes where it is, a taxon is
    // dense if any rank found it dense, the sparse taxa's sets are the union of the ranks' sets (hyperloglogplus.cpp:586-665)
    const size_t ns = [&] { ku_counts_dims d{}; (void)ku_counts_dims_get(m->ranks[0].ctx, &d); return (size_t)d.n_slots; }();
    std::vector<uint32_t> dense(ns, 0), one(ns);
    int fs = KU_OK;
    for (auto &r : m->ranks) {
      if (hipSetDevice(r.device) != hipSuccess) return mfail(KU_EHIP, "hipSetDevice failed");
      fs = ku_ctx_sparse_finish(r.ctx, one.data());  // (the keys of the fast path's log join the rank's set here)
      if (fs != KU_OK) break;
      for (size_t i = 0; i < ns; ++i) dense[i] |= one[i];
    }
    for (auto &r : m->ranks) {
      if (fs != KU_OK) break;
      if (hipSetDevice(r.device) != hipSuccess) return mfail(KU_EHIP, "hipSetDevice failed");
      fs = ku_ctx_sparse_set_dense(r.ctx, dense.data());
    }
    for (uint32_t q = 1; q < m->n_local && fs == KU_OK; ++q) fs = ku_ctx_sparse_absorb(m->ranks[0].ctx, m->ranks[q].ctx);
    if (fs == KU_ENOMEM) degraded = true;  // no room for a rank's set (or the union): dense estimates, as below
    else if (fs != KU_OK) return fs;
    m->acc_nt = 0;
    m->open_rank = -1;
  }
  if (m->sparse && degraded) M_TRY(sparse_give_up_group(m));
  m->reduced = true;
  return KU_OK;
}

extern "C" int ku_mgpu_count_taxons(ku_mgpu *m, uint32_t *taxids, uint64_t *counts, uint64_t *n) {
  if (!m || !n) return mfail(KU_EINVAL, "ku_mgpu_count_taxons: null argument");
  if (!single_process(m)) return mfail(KU_EUNSUP, "ku_mgpu_count_taxons: single-process groups only");
  std::vector<std::pair<uint32_t, uint64_t>> acc;
  const uint32_t n_src = (m->flags & KU_MGPU_REPLICAS) ? 1 : m->n_local;
  for (uint32_t i = 0; i < n_src; ++i) {
    uint64_t c = 0;
    M_TRY(ku_ctx_count_taxons(m->ranks[i].ctx, nullptr, nullptr, &c));
    std::vector<uint32_t> t(c + 1);
    std::vector<uint64_t> v(c + 1);
    uint64_t cap = c;
    M_TRY(ku_ctx_count_taxons(m->ranks[i].ctx, t.data(), v.data(), &cap));
    for (uint64_t j = 0; j < cap; ++j) acc.emplace_back(t[j], v[j]);
  }
  std::sort(acc.begin(), acc.end());
  std::vector<std::pair<uint32_t, uint64_t>> out;
  for (auto &kv : acc) {
    if (!out.empty() && out.back().first == kv.first) out.back().second += kv.second;
    else out.push_back(kv);
  }
  if (taxids && counts) {
    if (*n < out.size()) return mfail(KU_EINVAL, "output arrays too small");
    for (size_t j = 0; j < out.size(); ++j) { taxids[j] = out[j].first; counts[j] = out[j].second; }
  }
  *n = out.size();
  return KU_OK;
}
