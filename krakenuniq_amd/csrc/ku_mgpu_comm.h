// ku_mgpu_comm.h -- the exchange layer of the multi-GPU driver (part of the one translation unit ku_mgpu.cpp): the group's
// state, one host thread per rank (run_all), and the exchange primitives (comm_*) over two back ends:
//   RCCL      ncclBroadcast / grouped ncclReduce (a reduce-scatter whose slices end on read boundaries) / ncclAllReduce /
//             ncclAllGather on the rank's stream.  librccl is bound with dlopen at the first use, so single-GPU users
//             of the library never load it and a process that already holds an RCCL (PyTorch ships one) shares it.
//   same-process copies + merge kernels, host barriers between the ranks' threads (exchange()): ranks that share a device
//             (RCCL admits one rank per device) -- the form the 1-GPU test box can run -- or KU_MGPU_NO_RCCL.
#pragma once
#include <dlfcn.h>
#include <pthread.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "ku_internal.h"

static int mfail(int code, const std::string &msg) {
  ku_set_error(msg);
  return code;
}
#define M_HIP(expr)                                                                                          \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess)                                                                                    \
      return mfail(e_ == hipErrorOutOfMemory ? KU_ENOMEM : KU_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define M_TRY(expr)             \
  do {                          \
    int s_ = (expr);            \
    if (s_ != KU_OK) return s_; \
  } while (0)

// ---------------------------------------------------------------------------- RCCL, bound at run time
namespace {
// every RCCL entry point the driver calls: a field of g_rccl each, bound by name in rccl_load
#define KU_RCCL_CALLS(X)                                                                                                   \
  X(GetUniqueId) X(CommInitRank) X(CommInitAll) X(CommDestroy) X(Broadcast) X(Reduce) X(Send) X(Recv) X(AllReduce) X(AllGather) \
  X(GroupStart) X(GroupEnd) X(GetErrorString)
struct Rccl {
  void *h = nullptr;
#define KU_FIELD(name) decltype(&nccl##name) name = nullptr;
  KU_RCCL_CALLS(KU_FIELD)
#undef KU_FIELD
};
Rccl g_rccl;
pthread_once_t g_rccl_once = PTHREAD_ONCE_INIT;
std::string g_rccl_err;

void rccl_load() {
#ifdef KU_TEST_HOOKS
  // Test builds only (tests/rccl_shim/Makefile links libkrakenuniq_amd_testhooks.so with -DKU_TEST_HOOKS; the product library does
  // not look at the variable): KU_RCCL_LIB=<path> binds that library instead -- the peer paths between processes on a 1-GPU box;
  // RTLD_LOCAL + the handle-first lookup of dlsym keep it apart from an RCCL the process already holds
  if (const char *over = getenv("KU_RCCL_LIB")) {
    g_rccl.h = dlopen(over, RTLD_NOW | RTLD_LOCAL);
    if (!g_rccl.h) {
      g_rccl_err = std::string("cannot load KU_RCCL_LIB=") + over + ": " + dlerror();
      return;
    }
  }
#endif
  for (const char *name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) {
    if (g_rccl.h) break;
    g_rccl.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
  }
  if (!g_rccl.h) {
    g_rccl_err = std::string("cannot load librccl: ") + dlerror();
    return;
  }
#define KU_SYM(name)                                                                        \
  g_rccl.name = reinterpret_cast<decltype(g_rccl.name)>(dlsym(g_rccl.h, "nccl" #name)); \
  if (!g_rccl.name) g_rccl_err = "librccl lacks nccl" #name;
  KU_RCCL_CALLS(KU_SYM)
#undef KU_SYM
}
int rccl_ready() {
  pthread_once(&g_rccl_once, rccl_load);
  return g_rccl_err.empty() ? KU_OK : mfail(KU_EHIP, g_rccl_err);
}
#define M_NCCL(expr)                                                                                     \
  do {                                                                                                   \
    ncclResult_t r_ = (expr);                                                                            \
    if (r_ != ncclSuccess) return mfail(KU_EHIP, std::string(#expr) + ": " + g_rccl.GetErrorString(r_)); \
  } while (0)
// a grouped exchange: `body` issues the calls of one group and returns the first result that is not ncclSuccess (`what`
// names the calls in the error text)
template <class Body>
int rccl_group(const char *what, Body &&body) {
  M_NCCL(g_rccl.GroupStart());
  const ncclResult_t e = body();
  if (e != ncclSuccess) {
    (void)g_rccl.GroupEnd();
    return mfail(KU_EHIP, std::string(what) + ": " + g_rccl.GetErrorString(e));
  }
  M_NCCL(g_rccl.GroupEnd());
  return KU_OK;
}

struct DBuf {
  void *p = nullptr;
  size_t cap = 0;
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  int reserve(size_t bytes) {
    if (bytes <= cap) return KU_OK;
    release();
    const size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(&p, want) != hipSuccess) {
      p = nullptr;
      return mfail(KU_ENOMEM, "device memory for a multi-GPU batch buffer");
    }
    cap = want;
    return KU_OK;
  }
};

// state the ranks of one process share for the same-process exchange
struct Shared {
  pthread_barrier_t bar;
  bool bar_init = false;
  std::vector<const void *> ptr_a, ptr_b, ptr_c;  // published per local rank
  std::vector<std::vector<uint32_t>> vals;
  std::vector<std::vector<uint64_t>> u64s;
  std::vector<const uint64_t *> offs;  // host offset tables published next to ptr_a
  std::vector<int> dev;
  std::atomic<int> failed{0};
};
}  // namespace

struct ku_mgpu {
  uint32_t world = 0, first_rank = 0, n_local = 0, flags = 0;
  bool use_rccl = false;
  struct Rank {
    uint32_t rank = 0, local = 0;
    int device = 0;
    ku_ctx *ctx = nullptr;
    ncclComm_t comm = nullptr;
    DBuf seqs, off, len, taxa, calls, hits, runs, roff, rcnt, scratch, small;
    // owner routing, two sets (the rounds of a step alternate between them, each set on a stream of its own): the send
    // queues (records) + their k-mer numbering, what this rank received + its numbering, the slots it found, the slots that
    // came back, scratch of the prefix sums, the small device tables of a round
    struct RouteSet {
      DBuf q_rec, q_kb, r_rec, r_kb, r_slots, ret_slots, pfx_work, rt_dev;
    } rs[2];
    // ku_mgpu_set_timing: event pairs of the last routed step, [stage 0 scan, 1 owner, 2 resolve], and what it received
    std::vector<hipEvent_t> tev_pool;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> tev;
    size_t tev_used = 0;
    double t_rounds = 0, t_rec = 0, t_kmers = 0;
    hipStream_t aux = nullptr;            // the second set's stream
    hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_r = nullptr;
    uint64_t n_runs = 0;   // runs of the last host batch still in `runs`
    uint64_t run_base = 0; // where they start in the caller's array
    // everything the rank holds on its device but the context and the communicator (the device is current)
    void release() {
      for (DBuf *b : {&seqs, &off, &len, &taxa, &calls, &hits, &runs, &roff, &rcnt, &scratch, &small}) b->release();
      for (auto &t : rs)
        for (DBuf *b : {&t.q_rec, &t.q_kb, &t.r_rec, &t.r_kb, &t.r_slots, &t.ret_slots, &t.pfx_work, &t.rt_dev}) b->release();
      if (aux) (void)hipStreamDestroy(aux);
      for (hipEvent_t e : tev_pool) (void)hipEventDestroy(e);
      for (hipEvent_t e : {ev_a, ev_b, ev_r})
        if (e) (void)hipEventDestroy(e);
    }
  };
  std::vector<Rank> ranks;
  Shared sh;
  bool loaded = false, tax_set = false;
  bool reduced = false;  // ku_mgpu_reduce_state ran and no batch was classified since: a second call would add the sums again
  // HyperLogLog++ sparse-mode emulation over the group (ku_mgpu_enable_sparse): every rank runs it on whole work units
  bool sparse = false;
  bool sparse_gave_up = false;       // the emulation was given up for the whole group (a rank ran out of memory)
  uint64_t unit_nt = 0, acc_nt = 0;  // -u, and the nt of the unit that is still open (classify.cpp:510-521)
  int open_rank = -1;                // the rank whose context holds that unit's state
  bool exact = false;                // classifyExact on the sharded group (ku_mgpu_enable_exact)
  // owner routing of the sharded path (set up with the taxonomy): every rank's minimizer range
  bool route = false;
  bool ring_reduce = false;  // KU_MGPU_EXCHANGE=reduce, read with the taxonomy like `route`
  std::vector<uint64_t> own_lo, own_hi;
  bool timing = false;
};

namespace {
// run fn(rank) on one host thread per local rank (inline for a single rank); the first failing status wins
int run_all(ku_mgpu *m, const std::function<int(ku_mgpu::Rank &)> &fn) {
  std::vector<int> st(m->n_local, KU_OK);
  std::vector<std::string> msg(m->n_local);
  auto body = [&](uint32_t i) {
    ku_mgpu::Rank &r = m->ranks[i];
    if (hipSetDevice(r.device) != hipSuccess) {
      st[i] = KU_EHIP;
      msg[i] = "hipSetDevice failed";
      m->sh.failed.store(1);
      return;
    }
    st[i] = fn(r);
    if (st[i] != KU_OK) {
      msg[i] = ku_last_error();
      m->sh.failed.store(1);
    }
  };
  m->sh.failed.store(0);
  if (m->n_local == 1) {
    body(0);
  } else {
    std::vector<std::thread> team;
    for (uint32_t i = 0; i < m->n_local; ++i) team.emplace_back(body, i);
    for (auto &t : team) t.join();
  }
  for (uint32_t i = 0; i < m->n_local; ++i)
    if (st[i] != KU_OK) return mfail(st[i], "rank " + std::to_string(m->ranks[i].rank) + ": " + msg[i]);
  return KU_OK;
}

// ---------------------------------------------------------------------------- the exchange primitives
// Each takes the rank's status so far and returns the status behind the exchange (the protocol: header of ku_mgpu.cpp).
void barrier(ku_mgpu *m) {
  if (m->n_local > 1) pthread_barrier_wait(&m->sh.bar);
}
// a rank that already failed says so before a barrier, everybody leaves with an error behind the last one
void gate_in(ku_mgpu *m, int st) {
  if (st != KU_OK) m->sh.failed.store(1);
}
int gate_out(ku_mgpu *m, int st) {
  if (st == KU_OK && m->sh.failed.load()) return mfail(KU_ESTATE, "another rank of the group failed");
  return st;
}
bool comm_noop(const ku_mgpu *m) { return m->world == 1 && !m->use_rccl; }
// RCCL path: a rank that failed before a collective must not leave the others waiting inside it.  The ranks of one
// process agree on skipping it through the shared flag (several processes cannot, short of another collective: there a
// failed rank ends its process and the launcher takes the job down).
int rccl_gate(ku_mgpu *m, int st) {
  if (m->n_local == 1) return st;
  gate_in(m, st);
  barrier(m);
  return gate_out(m, st);
}

// The same-process protocol (header of ku_mgpu.cpp), its one implementation.  `first_sync`: work queued on s wrote what
// gets published, s is waited for first (the text is the error's).  `publish` puts this rank's pointers into m->sh.  One
// or two phases follow; a phase with a `sync` text queues device work on s.  Behind the last barrier the peers may
// reuse what they published.
struct Phase { std::function<int()> body; const char *sync; };
int exchange(ku_mgpu *m, int st, hipStream_t s, const char *first_sync, const std::function<void()> &publish, std::initializer_list<Phase> phases) {
  if (first_sync && st == KU_OK && hipStreamSynchronize(s) != hipSuccess) st = mfail(KU_EHIP, first_sync);
  publish();
  for (const Phase &ph : phases) {
    gate_in(m, st);
    barrier(m);
    if (st != KU_OK || m->sh.failed.load()) continue;
    st = ph.body();
    if (st == KU_OK && ph.sync && hipStreamSynchronize(s) != hipSuccess) st = mfail(KU_EHIP, ph.sync);
  }
  gate_in(m, st);
  barrier(m);
  return gate_out(m, st);
}

int copy_from_peer(void *dst, const void *src, size_t bytes, hipStream_t s) {
  if (bytes) M_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, s));
  return KU_OK;
}
// p: `bytes` of local rank q's published buffer; made a pointer that a kernel on r's device may read -- p itself, or a copy
// staged at byte `at` of r.scratch (`room` bytes in all) when q sits on another device
int peer_readable(ku_mgpu *m, ku_mgpu::Rank &r, uint32_t q, const void *&p, size_t bytes, size_t at, size_t room, hipStream_t s) {
  if (m->sh.dev[q] == r.device) return KU_OK;
  M_TRY(r.scratch.reserve(room));
  void *staged = (char *)r.scratch.p + at;
  M_TRY(copy_from_peer(staged, p, bytes, s));
  p = staged;
  return KU_OK;
}

int comm_broadcast(ku_mgpu *m, ku_mgpu::Rank &r, int st, void *buf, size_t bytes, hipStream_t s) {
  if (comm_noop(m) || bytes == 0) return st;
  if (m->use_rccl) {
    M_TRY(rccl_gate(m, st));
    M_NCCL(g_rccl.Broadcast(buf, buf, bytes, ncclUint8, 0, r.comm, s));
    return KU_OK;
  }
  return exchange(m, st, s, "stream synchronisation failed", [&] { m->sh.ptr_a[r.local] = buf; },
                  {{[&] { return r.local ? copy_from_peer(buf, m->sh.ptr_a[0], bytes, s) : KU_OK; }, "broadcast copy failed"}});
}

// in place: afterwards rank r holds max over all ranks of taxa[pos[r] .. pos[r+1])
int comm_reduce_slices_max(ku_mgpu *m, ku_mgpu::Rank &r, int st, uint32_t *taxa, const uint64_t *pos, hipStream_t s) {
  if (comm_noop(m)) return st;
  const uint64_t lo = pos[r.rank], n = pos[r.rank + 1] - lo;
  if (m->use_rccl) {
    M_TRY(rccl_gate(m, st));
    if (m->ring_reduce)
      return rccl_group("ncclReduce", [&] {
        ncclResult_t e = ncclSuccess;
        for (uint32_t q = 0; q < m->world && e == ncclSuccess; ++q)
          if (const uint64_t n_q = pos[q + 1] - pos[q]) e = g_rccl.Reduce(taxa + pos[q], taxa + pos[q], n_q, ncclUint32, ncclMax, (int)q, r.comm, s);
        return e;
      });
    // all-to-all over the point-to-point xGMI links: every rank sends slice q of its array straight to rank q (each
    // pair of GPUs has its own link, so the world - 1 transfers of a rank run side by side) and folds the world - 1
    // slices it receives into its own with the merge kernel.  A ring / tree ncclReduce per slice would push every
    // slice through every link.
    const uint32_t peers = m->world - 1;
    M_TRY(r.scratch.reserve(std::max<uint64_t>(1, (uint64_t)peers * n) * 4));
    uint32_t *stage = (uint32_t *)r.scratch.p;
    M_TRY(rccl_group("ncclSend / ncclRecv", [&] {
      ncclResult_t e = ncclSuccess;
      uint32_t slot = 0;
      for (uint32_t q = 0; q < m->world && e == ncclSuccess; ++q) {
        if (q == r.rank) continue;
        const uint64_t n_q = pos[q + 1] - pos[q];
        if (n_q) e = g_rccl.Send(taxa + pos[q], n_q, ncclUint32, (int)q, r.comm, s);
        if (e == ncclSuccess && n) e = g_rccl.Recv(stage + (uint64_t)slot * n, n, ncclUint32, (int)q, r.comm, s);
        ++slot;
      }
      return e;
    }));
    for (uint32_t i = 0; i < peers && n; ++i) M_TRY(ku_launch_merge_max_u32(taxa + lo, stage + (uint64_t)i * n, n, s));
    return KU_OK;
  }
  auto merge = [&] {
    for (uint32_t q = 0; q < m->n_local && n; ++q) {
      if (q == r.local) continue;
      const void *src = (const uint32_t *)m->sh.ptr_a[q] + lo;
      M_TRY(peer_readable(m, r, q, src, n * 4, 0, n * 4, s));
      M_TRY(ku_launch_merge_max_u32(taxa + lo, (const uint32_t *)src, n, s));
    }
    return KU_OK;
  };
  return exchange(m, st, s, "lookup failed", [&] { m->sh.ptr_a[r.local] = taxa; }, {{merge, "slot merge failed"}});
}

int comm_allreduce_state(ku_mgpu *m, ku_mgpu::Rank &r, hipStream_t s) {
  if (comm_noop(m)) return KU_OK;
  uint8_t *regs = nullptr;
  uint64_t n_regs = 0, n_slots = 0, n_nodes = 0, *nk = nullptr, *nr = nullptr;
  int st = ku_counts_device_ptrs(r.ctx, &regs, &n_regs, &nk, &n_slots, &nr, &n_nodes);
  if (m->use_rccl) {
    M_TRY(rccl_gate(m, st));
    return rccl_group("ncclAllReduce of the per-taxon state", [&] {
      const ncclResult_t e1 = g_rccl.AllReduce(regs, regs, n_regs, ncclUint8, ncclMax, r.comm, s);
      const ncclResult_t e2 = g_rccl.AllReduce(nk, nk, n_slots, ncclUint64, ncclSum, r.comm, s);
      const ncclResult_t e3 = g_rccl.AllReduce(nr, nr, n_nodes, ncclUint64, ncclSum, r.comm, s);
      return e1 != ncclSuccess ? e1 : e2 != ncclSuccess ? e2 : e3;
    });
  }
  auto fold = [&] {  // everybody into the first rank ...
    for (uint32_t q = 1; q < m->n_local && r.local == 0; ++q) {
      const void *a = m->sh.ptr_a[q], *b = m->sh.ptr_b[q], *c = m->sh.ptr_c[q];
      const size_t room = n_regs + (n_slots + n_nodes) * 8;
      M_TRY(peer_readable(m, r, q, a, n_regs, 0, room, s));
      M_TRY(peer_readable(m, r, q, b, n_slots * 8, n_regs, room, s));
      M_TRY(peer_readable(m, r, q, c, n_nodes * 8, n_regs + n_slots * 8, room, s));
      M_TRY(ku_launch_merge_max_u8(regs, (const uint8_t *)a, n_regs, s));
      M_TRY(ku_launch_merge_add_u64((unsigned long long *)nk, (const unsigned long long *)b, n_slots, s));
      M_TRY(ku_launch_merge_add_u64((unsigned long long *)nr, (const unsigned long long *)c, n_nodes, s));
    }
    return KU_OK;
  };
  auto hand_back = [&] {  // ... and the result to everybody
    if (r.local == 0) return KU_OK;
    M_TRY(copy_from_peer(regs, m->sh.ptr_a[0], n_regs, s));
    M_TRY(copy_from_peer(nk, m->sh.ptr_b[0], n_slots * 8, s));
    return copy_from_peer(nr, m->sh.ptr_c[0], n_nodes * 8, s);
  };
  return exchange(m, st, s, "stream synchronisation failed", [&] { m->sh.ptr_a[r.local] = regs; m->sh.ptr_b[r.local] = nk; m->sh.ptr_c[r.local] = nr; },
                  {{fold, "state merge failed"}, {hand_back, "state copy failed"}});
}

// classifyExact over a sharded group: the ranks' k-mer sets are disjoint (a k-mer lives where its bin lives), the
// first-insertion counters per slot add up
int comm_allreduce_exact(ku_mgpu *m, ku_mgpu::Rank &r, int st, hipStream_t s) {
  if (comm_noop(m)) return st;
  unsigned long long *uq = ku_ctx_exact_unique_of(r.ctx);
  ku_counts_dims d{};
  if (st == KU_OK) st = uq ? ku_counts_dims_get(r.ctx, &d) : mfail(KU_ESTATE, "exact counting is not enabled on every rank");
  if (m->use_rccl) {
    M_TRY(rccl_gate(m, st));
    M_NCCL(g_rccl.AllReduce(uq, uq, d.n_slots, ncclUint64, ncclSum, r.comm, s));
    return KU_OK;
  }
  auto fold = [&] {
    for (uint32_t q = 1; q < m->n_local && r.local == 0; ++q) {
      const void *a = m->sh.ptr_a[q];
      M_TRY(peer_readable(m, r, q, a, d.n_slots * 8, 0, d.n_slots * 8, s));
      M_TRY(ku_launch_merge_add_u64(uq, (const unsigned long long *)a, d.n_slots, s));
    }
    return KU_OK;
  };
  return exchange(m, st, s, "stream synchronisation failed", [&] { m->sh.ptr_a[r.local] = uq; },
                  {{fold, "exact counter merge failed"},
                   {[&] { return r.local ? copy_from_peer(uq, m->sh.ptr_a[0], d.n_slots * 8, s) : KU_OK; }, "exact counter copy failed"}});
}

// union of every rank's ascending value list
int comm_allgather_values(ku_mgpu *m, ku_mgpu::Rank &r, int st, const std::vector<uint32_t> &mine, std::vector<uint32_t> &all) {
  all = mine;
  if (comm_noop(m)) return st;
  if (m->use_rccl) {
    M_TRY(rccl_gate(m, st));
    hipStream_t s = ku_ctx_stream_of(r.ctx);
    M_TRY(r.small.reserve(8ull * m->world + 8));
    unsigned long long mine_n = mine.size();
    unsigned long long *d_n = (unsigned long long *)r.small.p;
    M_HIP(hipMemcpyAsync(d_n + m->world, &mine_n, 8, hipMemcpyHostToDevice, s));
    M_NCCL(g_rccl.AllGather(d_n + m->world, d_n, 1, ncclUint64, r.comm, s));
    std::vector<unsigned long long> counts(m->world);
    M_HIP(hipMemcpyAsync(counts.data(), d_n, 8ull * m->world, hipMemcpyDeviceToHost, s));
    M_HIP(hipStreamSynchronize(s));
    const uint64_t mx = std::max<uint64_t>(1, *std::max_element(counts.begin(), counts.end()));
    M_TRY(r.scratch.reserve(4 * mx * (m->world + 1)));
    uint32_t *d_all = (uint32_t *)r.scratch.p, *d_mine = d_all + mx * m->world;
    M_HIP(hipMemsetAsync(d_mine, 0, 4 * mx, s));
    if (!mine.empty()) M_HIP(hipMemcpyAsync(d_mine, mine.data(), 4 * mine.size(), hipMemcpyHostToDevice, s));
    M_NCCL(g_rccl.AllGather(d_mine, d_all, mx, ncclUint32, r.comm, s));
    std::vector<uint32_t> buf(mx * m->world);
    M_HIP(hipMemcpyAsync(buf.data(), d_all, 4 * mx * m->world, hipMemcpyDeviceToHost, s));
    M_HIP(hipStreamSynchronize(s));
    all.clear();
    for (uint32_t q = 0; q < m->world; ++q) all.insert(all.end(), buf.begin() + q * mx, buf.begin() + q * mx + counts[q]);
  } else {
    auto collect = [&] {
      all.clear();
      for (const auto &v : m->sh.vals) all.insert(all.end(), v.begin(), v.end());
      return KU_OK;
    };
    st = exchange(m, st, nullptr, nullptr, [&] { m->sh.vals[r.local] = mine; }, {{collect, nullptr}});
  }
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
  return st;
}

// every rank's n numbers, published in m->sh.u64s, rank-major into `all` (the same-process half of the two all-gathers)
int gather_u64s(ku_mgpu *m, ku_mgpu::Rank &r, int st, const uint64_t *mine, uint32_t n, std::vector<uint64_t> &all) {
  auto collect = [&] {
    for (uint32_t q = 0; q < m->n_local; ++q) std::copy(m->sh.u64s[q].begin(), m->sh.u64s[q].end(), all.begin() + (size_t)q * n);
    return KU_OK;
  };
  return exchange(m, st, nullptr, nullptr, [&] { m->sh.u64s[r.local].assign(mine, mine + n); }, {{collect, nullptr}});
}

// every rank's `n` numbers, rank-major, on every rank
int comm_allgather_u64(ku_mgpu *m, ku_mgpu::Rank &r, int st, const uint64_t *mine, uint32_t n, std::vector<uint64_t> &all, hipStream_t s) {
  all.assign((size_t)m->world * n, 0);
  if (comm_noop(m)) { std::copy(mine, mine + n, all.begin()); return st; }
  if (m->use_rccl) {
    M_TRY(rccl_gate(m, st));
    M_TRY(r.small.reserve(8ull * n * (m->world + 1) + 64));
    unsigned long long *d_all = (unsigned long long *)r.small.p, *d_mine = d_all + (size_t)n * m->world;
    M_HIP(hipMemcpyAsync(d_mine, mine, 8ull * n, hipMemcpyHostToDevice, s));
    M_NCCL(g_rccl.AllGather(d_mine, d_all, n, ncclUint64, r.comm, s));
    M_HIP(hipMemcpyAsync(all.data(), d_all, 8ull * n * m->world, hipMemcpyDeviceToHost, s));
    M_HIP(hipStreamSynchronize(s));
    return KU_OK;
  }
  return gather_u64s(m, r, st, mine, n, all);
}

// the same for numbers that lie in DEVICE memory (written by work queued on s): ONE host round trip -- over RCCL the
// all-gather runs on the device and one copy brings everything back
int comm_allgather_u64_dev(ku_mgpu *m, ku_mgpu::Rank &r, int st, const unsigned long long *d_mine, uint32_t n, std::vector<uint64_t> &all, hipStream_t s) {
  all.assign((size_t)m->world * n, 0);
  if (m->use_rccl && !comm_noop(m)) {
    M_TRY(rccl_gate(m, st));
    M_TRY(r.small.reserve(8ull * n * m->world + 64));
    M_NCCL(g_rccl.AllGather(d_mine, r.small.p, n, ncclUint64, r.comm, s));
    M_HIP(hipMemcpyAsync(all.data(), r.small.p, 8ull * n * m->world, hipMemcpyDeviceToHost, s));
    M_HIP(hipStreamSynchronize(s));
    return KU_OK;
  }
  std::vector<uint64_t> mine(n, 0);
  if (st == KU_OK && (hipMemcpyAsync(mine.data(), d_mine, 8ull * n, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess))
    st = mfail(KU_EHIP, "routing counts copy failed");
  if (comm_noop(m)) { std::copy(mine.begin(), mine.end(), all.begin()); return st; }
  return gather_u64s(m, r, st, mine.data(), n, all);
}

// all-to-all of variable-size segments: rank r sends send[send_at[q] .. send_at[q] + send_n[q]) (elements of `elem` bytes) to
// rank q and receives rank p's segment for it at recv[recv_at[p] ..).  Over xGMI every pair of GPUs has its own link: the
// world - 1 transfers of a rank run side by side (grouped ncclSend / ncclRecv).
int comm_alltoallv(ku_mgpu *m, ku_mgpu::Rank &r, int st, const void *send, const uint64_t *send_at, const uint64_t *send_n, void *recv,
                   const uint64_t *recv_at, const uint64_t *recv_n, size_t elem, hipStream_t s) {
  if (comm_noop(m)) {
    if (st == KU_OK && send_n[0] &&
        hipMemcpyAsync((char *)recv + recv_at[0] * elem, (const char *)send + send_at[0] * elem, send_n[0] * elem, hipMemcpyDeviceToDevice, s) != hipSuccess)
      st = mfail(KU_EHIP, "local copy failed");
    return st;
  }
  if (m->use_rccl) {
    M_TRY(rccl_gate(m, st));
    return rccl_group("ncclSend / ncclRecv", [&] {
      ncclResult_t e = ncclSuccess;
      for (uint32_t q = 0; q < m->world && e == ncclSuccess; ++q) {
        if (send_n[q]) e = g_rccl.Send((const char *)send + send_at[q] * elem, send_n[q] * elem, ncclUint8, (int)q, r.comm, s);
        if (e == ncclSuccess && recv_n[q]) e = g_rccl.Recv((char *)recv + recv_at[q] * elem, recv_n[q] * elem, ncclUint8, (int)q, r.comm, s);
      }
      return e;
    });
  }
  auto pull = [&] {  // rank p's segment for this rank
    for (uint32_t p = 0; p < m->n_local; ++p)
      if (recv_n[p])
        M_TRY(copy_from_peer((char *)recv + recv_at[p] * elem, (const char *)m->sh.ptr_a[p] + m->sh.offs[p][r.rank] * elem, recv_n[p] * elem, s));
    return KU_OK;
  };
  return exchange(m, st, s, "stream synchronisation failed", [&] { m->sh.ptr_a[r.local] = send; m->sh.offs[r.local] = send_at; },
                  {{pull, "all-to-all copy failed"}});
}

// rank 0 holds buf[0 .. bounds[world]) (elements of `elem` bytes); rank q receives its slice [bounds[q], bounds[q + 1]) in place
int comm_scatter_slices(ku_mgpu *m, ku_mgpu::Rank &r, int st, void *buf, const uint64_t *bounds, size_t elem, hipStream_t s) {
  if (comm_noop(m)) return st;
  const uint64_t lo = bounds[r.rank], n = bounds[r.rank + 1] - lo;
  if (m->use_rccl) {
    M_TRY(rccl_gate(m, st));
    return rccl_group("ncclSend / ncclRecv", [&] {
      ncclResult_t e = ncclSuccess;
      if (r.rank == 0) {
        for (uint32_t q = 1; q < m->world && e == ncclSuccess; ++q)
          if (const uint64_t nq = bounds[q + 1] - bounds[q]) e = g_rccl.Send((const char *)buf + bounds[q] * elem, nq * elem, ncclUint8, (int)q, r.comm, s);
      } else if (n) e = g_rccl.Recv((char *)buf + lo * elem, n * elem, ncclUint8, 0, r.comm, s);
      return e;
    });
  }
  return exchange(m, st, s, "stream synchronisation failed", [&] { m->sh.ptr_a[r.local] = buf; },
                  {{[&] { return r.local ? copy_from_peer((char *)buf + lo * elem, (const char *)m->sh.ptr_a[0] + lo * elem, n * elem, s) : KU_OK; },
                    "scatter copy failed"}});
}

bool single_process(const ku_mgpu *m) { return m->first_rank == 0 && m->n_local == m->world; }

// A rank context (ku_mgpu_ctx) with batches of ku_classify_batch_rle_enqueue in flight: whatever classifies, reduces, loads or
// changes state over the group answers KU_ESTATE, before any rank starts (a collective must not begin on some ranks only)
int ranks_idle(const ku_mgpu *m, const char *who) {
  for (const auto &r : m->ranks)
    if (r.ctx && ku_classify_batch_rle_in_flight(r.ctx))
      return mfail(KU_ESTATE, std::string(who) + ": rank " + std::to_string(r.rank) + " has batches in flight (ku_classify_batch_rle_finish first)");
  return KU_OK;
}
}  // namespace
