// ku_mgpu_route.h -- the routed step of the multi-GPU driver (part of the one translation unit ku_mgpu.cpp)
#pragma once
#include "ku_mgpu_comm.h"
#include "ku_route_plan.h"

namespace {
// The owner-routed sharded batch on one rank: the rank scans only ITS slice of the reads, every run of
// k-mers that share a minimizer occurrence travels as one 16-byte record to the rank that owns the bin, one slot per k-mer
// comes back.  The slice is taken in ROUNDS of whole reads (about KU_ROUTE_ROUND positions each; every rank runs the same
// number of rounds: it owns bins in all of them), and a round is four stages:
//   S  scan -> records in W queues, tickets in the per-k-mer array; prefix sum of the records' k-mer counts, per-queue totals
//   G  all-gather of {records, k-mers} per queue: the ONE host round trip of a round (a queue that overflowed: rescan)
//   X  all-to-all of the records (16 B each); prefix sum over what arrived; owner kernel: probe + HLL + n_kmers
//   Y  all-to-all of the slots (4 B per k-mer); tickets -> slots fused with the resolve stage of the round's reads
// The scan and the resolve stage are bound by instruction issue and latency, the owner kernel by the random line rate of the
// memory system.  Consecutive rounds alternate between two buffer sets on two streams, issued
// S(0) G(0) { X(r)  S(r+1)  G(r+1)  Y(r) }: the owner kernel of round r runs beside the scan of round r + 1 and the resolve
// of round r - 1, and the copies of one round's exchange under the kernels of the other.  Measured (one rank forced
// through this path, 10 M reads): two streams 41.2 ms against 43.0 on one -- whole kernels side by side hide each other far
// less than the stages inside the fused single-GPU kernel do -- and every round costs ~0.5-1 ms (padding of the queues,
// launches, the host round trip), so rounds are LARGE (256 M positions: a 10 M-read step over eight ranks is one round);
// what the rounds are for is bounded buffers, and a record index that fits a ticket, whatever the size of a slice.
//   have_slice: the rank's slice of seqs / off / len is in place already (host batches: every rank uploads its own part);
//   else rank 0 holds the whole batch and the slices are scattered first (device batches).
//
// One running status, `st`, and one exit rule: the step is a fixed sequence of collectives, and a rank makes every one of
// them whatever its status -- a stage whose status is bad skips its device work and hands the status to its collective,
// whose gates let everybody leave together.  Nothing returns between the first collective and the last.
struct RouteRound : RoutePlanRound {
  uint64_t cap = 0;
  uint32_t chunk = 0;
  std::vector<uint64_t> all, send_at, send_n, ret_at, ret_n, recv_at, recv_n, rk_at, rk_n;
  uint64_t n_recv = 0, k_recv = 0, k_send = 0;
};

// the read offsets of a slice in device memory as the planner's source: n copies, one synchronisation
struct RouteDeviceOffsets {
  const uint64_t *d_off;  // of the slice's first read
  hipStream_t s;
  int operator()(const uint64_t *idx, uint32_t n, uint64_t *out) const {
    for (uint32_t i = 0; i < n; ++i)
      if (hipMemcpyAsync(out + i, d_off + idx[i], 8, hipMemcpyDeviceToHost, s) != hipSuccess) return mfail(KU_EHIP, "read offsets copy failed");
    return hipStreamSynchronize(s) == hipSuccess ? KU_OK : mfail(KU_EHIP, "read offsets copy failed");
  }
};

struct RoutedStep {
  ku_mgpu *m;
  ku_mgpu::Rank &r;
  int st;  // the status the rank arrives with
  void *d_seqs;
  uint64_t *d_off;
  uint32_t *d_len, *d_calls, *d_taxa, *d_hits;
  uint64_t n_bytes;
  const uint64_t *rb, *pos;
  const ku_opts &opts;
  hipStream_t s;
  const uint64_t *h_off;
  const uint32_t *h_len;
  // what follows is derived in run()
  uint32_t W = 0, R = 0, n_info = 0;
  uint64_t r0 = 0, nr = 0, p0 = 0, nb = 0;
  bool counts = false, emulate = false, fused = false;
  bool resolved_before = false;  // a resolve kernel was queued: the next one (other stream) waits for it (they share the context's spill workspace)
  ku_opts ro{};
  std::vector<RouteRound> rd{};
  hipStream_t str[2] = {nullptr, nullptr};
  struct Tables { uint64_t *lo, *hi; unsigned long long *cursor, *info; } tb[2] = {};

  void fail(int code, const char *msg) { st = st == KU_OK ? mfail(code, msg) : st; }

  // ---- rounds: every rank takes part in every round, so their number follows from the largest slice
  void plan() {
    uint64_t round_pos = 256ull << 20;
    if (const char *e = std::getenv("KU_ROUTE_ROUND")) round_pos = std::max<uint64_t>(256, std::strtoull(e, nullptr, 10));
    uint64_t nb_max = 0;
    for (uint32_t q = 0; q < W; ++q) nb_max = std::max(nb_max, pos[q + 1] - pos[q]);
    R = (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(1, (nb_max + round_pos - 1) / round_pos));
    rd.assign(R, RouteRound{});
    if (st != KU_OK) return;
    st = h_off ? ku_route_plan(nr, nb, p0, R, round_pos, RouteHostOffsets{h_off + r0}, rd)
               : ku_route_plan(nr, nb, p0, R, round_pos, RouteDeviceOffsets{d_off + r0, s}, rd);
    if (st == KU_EINVAL) st = mfail(KU_EINVAL, "owner routing: the reads of a slice must be in buffer order");
  }
  // ---- the second set's stream follows the caller's up to here
  void fork() {
    str[0] = str[1] = s;
    // (with the stage timing on, everything stays on one stream: kernels side by side would stretch each other's event pairs.
    // Over RCCL too, unless KU_ROUTE_TWO_STREAMS=1: collectives of one communicator issued from two streams are ordered by the
    // library, but that path has never run on more than one physical GPU here, and what the second stream buys is ~4 %.)
    if (R > 1 && !std::getenv("KU_ROUTE_ONE_STREAM") && !m->timing && (!m->use_rccl || std::getenv("KU_ROUTE_TWO_STREAMS"))) {
      if (!r.aux && hipStreamCreateWithFlags(&r.aux, hipStreamNonBlocking) != hipSuccess) { r.aux = nullptr; fail(KU_EHIP, "stream creation failed"); }
      for (hipEvent_t *e : {&r.ev_a, &r.ev_b, &r.ev_r})
        if (!*e && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) { *e = nullptr; fail(KU_EHIP, "event creation failed"); }
      if (st == KU_OK) {
        if (hipEventRecord(r.ev_a, s) != hipSuccess || hipStreamWaitEvent(r.aux, r.ev_a, 0) != hipSuccess) st = mfail(KU_EHIP, "stream fork failed");
        str[1] = r.aux;
      }
    }
  }
  // the small device tables of both sets: the owners' ranges, the queues' cursors, what a round's all-gather sends
  void upload_tables() {
    for (int i = 0; i < 2; ++i) {
      auto &t = r.rs[i];
      if (st == KU_OK) st = t.rt_dev.reserve((2ull * W + (uint64_t)W * KU_ROUTE_CURSOR_STRIDE + n_info + 8) * 8);
      if (st != KU_OK) break;
      tb[i].lo = (uint64_t *)t.rt_dev.p;
      tb[i].hi = tb[i].lo + W;
      tb[i].cursor = (unsigned long long *)(tb[i].hi + W);
      tb[i].info = tb[i].cursor + (size_t)W * KU_ROUTE_CURSOR_STRIDE;
      if (hipMemcpyAsync(tb[i].lo, m->own_lo.data(), 8ull * W, hipMemcpyHostToDevice, str[i]) != hipSuccess ||
          hipMemcpyAsync(tb[i].hi, m->own_hi.data(), 8ull * W, hipMemcpyHostToDevice, str[i]) != hipSuccess)
        st = mfail(KU_EHIP, "routing tables upload failed");
    }
  }
  // the caller's stream takes over again
  void join() {
    if (str[1] == s || !r.ev_b) return;
    // (KU_TEST_DROP_STREAM_JOIN, test builds only (-DKU_TEST_HOOKS): the join is left out, i.e. the bug an asynchronous collective library exposes
    // and a synchronous stand-in hides; tests/test_gpu_rccl_shim.py checks that the stand-in of round 5 makes the step fail)
#ifdef KU_TEST_HOOKS
    static const bool drop_join = std::getenv("KU_TEST_DROP_STREAM_JOIN") != nullptr;
#else
    constexpr bool drop_join = false;
#endif
    if (hipEventRecord(r.ev_b, str[1]) != hipSuccess || (!drop_join && hipStreamWaitEvent(s, r.ev_b, 0) != hipSuccess)) fail(KU_EHIP, "stream join failed");
  }

  // ku_mgpu_set_timing: stage `tag` between two events on stream q
  void t_begin(int tag, hipStream_t q) {
    if (!m->timing || st != KU_OK) return;
    while (r.tev_pool.size() < r.tev_used + 2) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) return;
      r.tev_pool.push_back(e);
    }
    hipEvent_t e0 = r.tev_pool[r.tev_used], e1 = r.tev_pool[r.tev_used + 1];
    r.tev_used += 2;
    (void)hipEventRecord(e0, q);
    r.tev.push_back({tag, {e0, e1}});
  }
  void t_end(hipStream_t q) {
    if (m->timing && !r.tev.empty()) (void)hipEventRecord(r.tev.back().second.second, q);
  }

  // S: scan + prefix of round i on its set's stream (first attempt: the default room per queue)
  void scan_round(uint32_t i) {
    RouteRound &x = rd[i];
    auto &t = r.rs[i & 1];
    hipStream_t q = str[i & 1];
    const uint64_t n_q = (uint64_t)W * x.cap;
    if (st == KU_OK && n_q > KU_ROUTE_MAX_RECORDS) st = mfail(KU_EUNSUP, "owner routing: more records per rank and round than a ticket can number");
    if (st == KU_OK && (t.q_rec.reserve(n_q * 16) || t.q_kb.reserve((n_q + 1) * 4) || t.pfx_work.reserve(ku_route_prefix_work_bytes(n_q))))
      st = mfail(KU_ENOMEM, "device memory for the routing queues");
    if (st == KU_OK && hipMemsetAsync(tb[i & 1].cursor, 0, 8ull * W * KU_ROUTE_CURSOR_STRIDE, q) != hipSuccess) st = mfail(KU_EHIP, "routing cursors reset failed");
    if (st != KU_OK) return;
    t_begin(0, q);
    KuRouteDev rt{};
    rt.own_lo = tb[i & 1].lo; rt.own_hi = tb[i & 1].hi; rt.cursor = tb[i & 1].cursor;
    rt.q_rec = (uint4 *)t.q_rec.p;
    rt.cap = x.cap; rt.world = W; rt.chunk = x.chunk;
    if (x.sb) st = ku_ctx_route_scan(r.ctx, (const char *)d_seqs + p0 + x.a, x.sb, d_taxa + p0 + x.a, rt, q);
    if (st == KU_OK) {
      st = ku_launch_route_prefix(t.q_rec.p, n_q, x.cap, tb[i & 1].cursor, (uint32_t *)t.q_kb.p, tb[i & 1].info, t.pfx_work.p, q);
      if (st != KU_OK) st = mfail(st, "routing prefix kernels failed");
    }
    t_end(q);
  }
  void stage_S(uint32_t i) {
    RouteRound &x = rd[i];
    // One scanning pass: every owner's queue gets room for about 2.5 times its fair share of the records a slice of random
    // sequence makes (a record per ~10 positions; the shard bounds are quantiles of the database's k-mers, reads follow
    // the database -- but the owners of the high bins get up to twice the records per k-mer: a large minimizer does not
    // stay one for long), plus the chunk every block of the scan may leave partly used; the cursors come back as the
    // true totals.  A queue that did not hold its total (low-complexity reads, a batch from one corner of the minimizer
    // space) sends the rank through a second pass with queues of the size the first one counted -- the results do not
    // depend on which it was (KU_ROUTE_CAP: records per queue, for the tests).
    const unsigned grid = x.sb ? ku_route_scan_grid(x.sb, ku_ctx_cus_of(r.ctx)) : 1u;
    // (a block claims `chunk` records of a queue at a time: with few owners larger claims keep the adds on one cursor apart)
    x.chunk = KU_ROUTE_CHUNK * std::max(1u, 8u / W);
    x.cap = x.sb / (4ull * W) + ((uint64_t)grid + 1) * x.chunk;
    if (const char *e = std::getenv("KU_ROUTE_CAP")) x.cap = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    x.cap = (x.cap + x.chunk - 1) / x.chunk * x.chunk;
    scan_round(i);
  }
  // G: every rank learns how much it gets from whom (records and k-mers), and whether anybody's queues overflowed (then
  // the ranks concerned scan again and everybody gathers again: all see the same numbers, so all agree).  A rank can fail
  // here alone (no room for what it is to receive): it goes on to the exchanges like the others, with its status; the
  // segment tables start out as W empty segments, so they can be handed over whatever became of this stage.
  void stage_G(uint32_t i) {
    RouteRound &x = rd[i];
    auto &t = r.rs[i & 1];
    for (auto *v : {&x.send_at, &x.send_n, &x.ret_at, &x.ret_n, &x.recv_at, &x.recv_n, &x.rk_at, &x.rk_n}) v->assign(W, 0);
    x.n_recv = x.k_recv = x.k_send = 0;
    for (int attempt = 0;; ++attempt) {
      st = comm_allgather_u64_dev(m, r, st, tb[i & 1].info, n_info, x.all, str[i & 1]);
      if (st != KU_OK) return;
      if (std::getenv("KU_ROUTE_DEBUG") && r.rank == 0) {
        fprintf(stderr, "[ku_route] round %u/%u attempt %d: sb %llu reads %llu", i, R, attempt, (unsigned long long)x.sb, (unsigned long long)x.rn);
        for (uint32_t qq = 0; qq < W; ++qq) {
          fprintf(stderr, " | rank %u cap %llu:", qq, (unsigned long long)x.all[(size_t)qq * n_info + 2 * W]);
          for (uint32_t o = 0; o < W; ++o)
            fprintf(stderr, " %llu/%llu", (unsigned long long)x.all[(size_t)qq * n_info + 2 * o], (unsigned long long)x.all[(size_t)qq * n_info + 2 * o + 1]);
        }
        fprintf(stderr, "\n");
      }
      bool over_any = false, over_mine = false;
      uint64_t mine_max = 0;
      for (uint32_t qq = 0; qq < W; ++qq)
        for (uint32_t o = 0; o < W; ++o) {
          const bool ov = x.all[(size_t)qq * n_info + 2 * o] > x.all[(size_t)qq * n_info + 2 * W];
          over_any |= ov;
          if (qq == r.rank) { over_mine |= ov; mine_max = std::max(mine_max, x.all[(size_t)qq * n_info + 2 * o]); }
        }
      if (!over_any) break;
      if (attempt >= 1) { st = mfail(KU_ESTATE, "owner routing: a queue overflowed twice"); return; }
      if (over_mine) {
        x.cap = (mine_max + x.chunk - 1) / x.chunk * x.chunk;
        scan_round(i);
      }
    }
    // segment tables: what goes where (records / k-mers), what comes from whom
    const uint64_t *mine = x.all.data() + (size_t)r.rank * n_info;
    for (uint32_t qq = 0; qq < W; ++qq) {
      x.send_at[qq] = (uint64_t)qq * x.cap;
      x.send_n[qq] = mine[2 * qq];
      x.ret_at[qq] = x.k_send;
      x.ret_n[qq] = mine[2 * qq + 1];
      x.k_send += x.ret_n[qq];
      x.recv_at[qq] = x.n_recv;
      x.recv_n[qq] = x.all[(size_t)qq * n_info + 2 * r.rank];
      x.n_recv += x.recv_n[qq];
      x.rk_at[qq] = x.k_recv;
      x.rk_n[qq] = x.all[(size_t)qq * n_info + 2 * r.rank + 1];
      x.k_recv += x.rk_n[qq];
    }
    if (x.n_recv >= (1ull << 32) || x.k_recv >= (1ull << 32) || x.k_send >= (1ull << 32)) st = mfail(KU_EUNSUP, "owner routing: more than 2^32 k-mers per rank and round");
    if (st == KU_OK && (t.r_rec.reserve(std::max<uint64_t>(x.n_recv, 1) * 16) || t.r_kb.reserve((x.n_recv + 1) * 4) ||
                        t.pfx_work.reserve(ku_route_prefix_work_bytes(std::max(x.n_recv, (uint64_t)W * x.cap))) ||
                        t.r_slots.reserve(std::max<uint64_t>(x.k_recv, 1) * 4) || t.ret_slots.reserve(std::max<uint64_t>(x.k_send, 1) * 4)))
      st = mfail(KU_ENOMEM, "device memory for the routing queues");
  }
  // X: records to their owners (16 B per run of k-mers), probe + accounting there
  void stage_X(uint32_t i) {
    RouteRound &x = rd[i];
    auto &t = r.rs[i & 1];
    hipStream_t q = str[i & 1];
    st = comm_alltoallv(m, r, st, t.q_rec.p, x.send_at.data(), x.send_n.data(), t.r_rec.p, x.recv_at.data(), x.recv_n.data(), 16, q);
    t_begin(1, q);
    if (m->timing) { r.t_rec += (double)x.n_recv; r.t_kmers += (double)x.k_recv; }
    if (st == KU_OK) {
      st = ku_launch_route_prefix(t.r_rec.p, x.n_recv, 0, nullptr, (uint32_t *)t.r_kb.p, nullptr, t.pfx_work.p, q);
      if (st != KU_OK) st = mfail(st, "routing prefix kernels failed");
    }
    if (st == KU_OK) st = ku_ctx_route_owner(r.ctx, t.r_rec.p, x.n_recv, (const uint32_t *)t.r_kb.p, (uint32_t *)t.r_slots.p, counts, q);
    t_end(q);
  }
  // Y: slots back (4 B per k-mer), into place: resolve stage of the round's reads, or tickets -> slots
  void stage_Y(uint32_t i) {
    RouteRound &x = rd[i];
    auto &t = r.rs[i & 1];
    hipStream_t q = str[i & 1];
    st = comm_alltoallv(m, r, st, t.r_slots.p, x.rk_at.data(), x.rk_n.data(), t.ret_slots.p, x.ret_at.data(), x.ret_n.data(), 4, q);
    if (st != KU_OK) return;
    t_begin(2, q);
    if (fused && x.rn) {
      if (resolved_before && str[0] != str[1] && hipStreamWaitEvent(q, r.ev_r, 0) != hipSuccess) { st = mfail(KU_EHIP, "stream wait failed"); return; }
      const uint64_t f = r0 + x.ra;
      st = ku_ctx_route_resolve(r.ctx, d_off + f, d_len + f, x.rn, &ro, d_calls + f, d_taxa, d_hits ? d_hits + f : nullptr,
                                (const uint32_t *)t.q_kb.p, (const uint32_t *)t.ret_slots.p, q);
      if (st == KU_OK && str[0] != str[1] && hipEventRecord(r.ev_r, q) != hipSuccess) st = mfail(KU_EHIP, "event record failed");
      resolved_before = true;
    } else if (!fused && x.sb) {
      st = ku_launch_route_gather(d_taxa + p0 + x.a, x.sb, (const uint32_t *)t.q_kb.p, (const uint32_t *)t.ret_slots.p, q);
      if (st != KU_OK) st = mfail(st, "routing gather kernel failed");
    }
    t_end(q);
  }

  int run(bool have_slice) {
    W = m->world, n_info = 2 * W + 1;
    r0 = rb[r.rank], nr = rb[r.rank + 1] - r0, p0 = pos[r.rank], nb = pos[r.rank + 1] - p0;
    if (!have_slice) {
      st = comm_scatter_slices(m, r, st, d_seqs, pos, 1, s);
      st = comm_scatter_slices(m, r, st, d_off, rb, 8, s);
      st = comm_scatter_slices(m, r, st, d_len, rb, 4, s);
    }
    counts = !(opts.flags & (KU_F_NO_COUNTS | KU_F_QUICK));  // quick mode books the scanned prefix in the resolve stage
    emulate = m->sparse && h_len && !(opts.flags & KU_F_NO_COUNTS);
    ro = opts;
    ro.flags &= ~(KU_F_KEEP_SLOTS | KU_F_MERGE_CHUNK);
    // the resolve stage inside the rounds (the fused kernel's ROUTE instance: slot through the ticket, hit counts,
    // resolve_tree, call, taxids in place); quick mode, reads beyond 65535 k-mers and the sparse-sketch emulation (it wants the
    // slots in the array) turn the tickets into slots per round and resolve the slice behind the last one
    fused = !emulate && st == KU_OK && ku_ctx_route_resolve_prepare(r.ctx, &ro, s) == KU_OK;
    plan();
    fork();
    upload_tables();
    if (m->timing) { r.tev.clear(); r.tev_used = 0; r.t_rounds = R; r.t_rec = r.t_kmers = 0; }
    stage_S(0);
    stage_G(0);
    for (uint32_t i = 0; i < R; ++i) {
      stage_X(i);                       // ... ends with the owner kernel queued on this round's stream
      if (i + 1 < R) stage_S(i + 1);    // the next round's scan beside it, on the other stream
      if (i + 1 < R) stage_G(i + 1);    // (host: waits for that scan)
      stage_Y(i);                       // (host: waits for the owner kernel) slots back, resolve stage queued
    }
    join();
    if (st != KU_OK) return st;
    if (nr == 0 || fused) return KU_OK;
    if (emulate)
      M_TRY(ku_ctx_sparse_pass_slots(r.ctx, d_seqs, d_off + r0, d_len + r0, h_off + r0, h_len + r0, nr, n_bytes, d_taxa,
                                     (opts.flags & KU_F_QUICK) ? std::max(1u, opts.min_hits) : 0u, s));
    t_begin(2, s);
    st = ku_resolve_device(r.ctx, d_seqs, d_off + r0, d_len + r0, nr, &ro, d_calls + r0, d_taxa, d_hits ? d_hits + r0 : nullptr, s);
    t_end(s);
    return st;
  }
};
}  // namespace
