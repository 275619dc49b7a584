"""-m gpu: the in-flight contract of tests/inflight_contract.py against the library.

While batches of ku_classify_batch_rle_enqueue are in flight on a context (their kernels on the two kernel streams, their
copies on the copy streams -- not on the context's own stream), every entry point that takes the context, or a group
holding it, either refuses (KU_ESTATE and no side effect), waits for all of the context's streams, or answers as on an idle
context.  Checked against the CPU oracle and the reference's files: a refused call must leave the run exactly as it was --
calls, Kraken text, per-taxon state, the sparse-sketch emulation's sets and the report all equal a run without it.

The outputs of the batches are page-locked: with pageable memory _enqueue serialises and nothing is really in flight."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from krakenuniq_amd import capi, synth
from oracle import ku_oracle as ko
import gpu_common as gc
import inflight_contract as ic
from test_gpu_sparse import assert_sparse_state_equals_oracle, rows, split_points
from test_gpu_two_step import batches_of, kraken_text, run_two_step

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F1 = os.path.join(ROOT, "tests", "golden", "f1")
COUNTS = [f"{F1}/database.kdb.counts"]
K = 31
KU_ESTATE = -6
SENTINEL = 0xFFFFFFFF
UNIT = 1000  # work units of the sparse cases: several close in every batch, one stays open behind most of them


def pinned(n, dtype, fill=0):
    """page-locked numpy array (the memory belongs to a pinned torch tensor the array keeps alive)"""
    import torch
    dt = np.dtype(dtype)
    a = torch.empty(max(int(n), 1) * dt.itemsize, dtype=torch.uint8).pin_memory().numpy().view(dt)
    a.fill(fill)
    return a


def pinned_batch(bb, bo, bl, fill=0):
    """a batch's inputs and result arrays in page-locked memory"""
    n = len(bo)
    arr = pinned(len(bb), np.uint8)
    arr[:] = np.frombuffer(bb, dtype=np.uint8) if isinstance(bb, (bytes, bytearray)) else bb
    off = pinned(n, np.uint64)
    off[:] = bo
    lens = pinned(n, np.uint32)
    lens[:] = bl
    out = {"calls": pinned(n, np.uint32, fill), "hits": pinned(n, np.uint32, fill), "run_off": pinned(n, np.uint64, fill),
           "run_cnt": pinned(n, np.uint32, fill), "runs": pinned(2 * (len(bb) // 6 + 4 * n + (1 << 20)), np.uint32, fill).reshape(-1, 2)}
    return arr, off, lens, out


_CACHE = {}


def f1():
    if "f1" not in _CACHE:
        ids, seqs = synth.read_seqfile(f"{F1}/reads.fq")
        buf, off, lens = ko.pack_reads(seqs)
        _CACHE["f1"] = (ids, seqs, buf, off, lens)
    return _CACHE["f1"]


def oracle_run(unit):
    key = ("run", unit)
    if key not in _CACHE:
        ids, seqs, buf, off, lens = f1()
        kw = {"work_unit_nt": unit} if unit else {}
        run = ko.Run(ko.Db(f"{F1}/database.kdb", f"{F1}/database.idx"), ko.Tax(f"{F1}/taxDB"), **kw)
        run.classify(seqs)
        _CACHE[key] = run
    return _CACHE[key]


def plain_report():
    """the dense-register report of an untouched context that ran the reads (there is no reference file for it)"""
    if "plain_report" not in _CACHE:
        ids, seqs, buf, off, lens = f1()
        ctx, cdb, ctax = gc.make_ctx(F1)
        ctx.classify_batch_rle(buf, off, lens)
        _CACHE["plain_report"] = ctx.report(ctax, COUNTS)
        ctx.close()
    return _CACHE["plain_report"]


def drain(ctx):
    """finishes whatever is still in flight: a failed assertion must not leave a context with running batches to the garbage
    collector (a library whose ku_ctx_destroy does not wait would free memory under them)"""
    n = ctypes.c_uint64()
    while ctx.h and ctx.rle_in_flight():
        capi.lib().ku_classify_batch_rle_finish(ctx.h, ctypes.byref(n))


def status_of(fn):
    with pytest.raises(capi.KuError) as e:
        fn()
    return e.value.status


# ---------------------------------------------------------------------------- refuse
class Env:
    """what the refused calls take: the context, its database and taxonomy, the reads, device copies of them, resident batches"""

    def __init__(self, ctx, cdb, ctax, buf, off, lens):
        self.ctx, self.cdb, self.ctax = ctx, cdb, ctax
        self.buf, self.off, self.lens = buf, off, lens
        self.n = len(lens)
        self._dev = None
        self.batches = []

    def dev(self):
        if self._dev is None:
            import torch
            d = "cuda:0"
            nb = len(self.buf)
            self._dev = {"seqs": torch.cat([torch.frombuffer(bytearray(self.buf), dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8)]).to(d),
                         "off": torch.from_numpy(self.off.astype(np.int64)).to(d), "len": torch.from_numpy(self.lens.astype(np.int32)).to(d),
                         "calls": torch.zeros(self.n, dtype=torch.int32, device=d), "taxa": torch.zeros(nb + 16, dtype=torch.int32, device=d),
                         "hits": torch.zeros(self.n, dtype=torch.int32, device=d), "runs": torch.zeros(2 * (nb + 1), dtype=torch.int32, device=d),
                         "roff": torch.zeros(self.n, dtype=torch.int64, device=d), "rcnt": torch.zeros(self.n, dtype=torch.int32, device=d),
                         "n_runs": torch.zeros(1, dtype=torch.int64, device=d), "pairs": torch.zeros(3, dtype=torch.int32, device=d),
                         "offsets": torch.zeros(2, dtype=torch.int64, device=d)}
            torch.cuda.synchronize()
        return self._dev

    def p(self, key):
        return self.dev()[key].data_ptr()


def _absorb(e):
    a, b = e.batches
    capi._chk(capi.lib().ku_batch_absorb(e.ctx.h, a.h, b.h), "ku_batch_absorb")


# row -> the call with valid arguments on the context that has batches in flight
REFUSE_CALLS = {
    "ku_ctx_load_db": lambda e: e.ctx.load_db(e.cdb),
    "ku_ctx_adopt_db": lambda e: e.ctx.adopt_db(e.p("pairs"), 0, e.p("offsets"), e.cdb.info.k, e.cdb.info.nt, 2, 0, 1),
    "ku_ctx_add_db": lambda e: e.ctx.add_db(e.cdb),
    "ku_ctx_set_taxonomy": lambda e: e.ctx.set_taxonomy(e.ctax),
    "ku_ctx_swap_shard": lambda e: e.ctx.swap_shard(e.cdb, 0, e.cdb.info.n_bins),
    "ku_ctx_prefetch_shard": lambda e: e.ctx.prefetch_shard(e.cdb, 0, e.cdb.info.n_bins),
    "ku_ctx_enable_exact": lambda e: e.ctx.enable_exact(20),
    "ku_counts_export_exact": lambda e: e.ctx.exact_counts(),
    "ku_ctx_reset_counts": lambda e: e.ctx.reset_counts(),
    "ku_counts_export": lambda e: e.ctx.counts(),
    "ku_ctx_merge_state": None,  # both sides: test_merge_state_is_refused_on_either_side
    "ku_ctx_report": lambda e: e.ctx.report(e.ctax, COUNTS),
    "ku_ctx_report_cols": lambda e: e.ctx.report(e.ctax, COUNTS, flags=1),
    "ku_ctx_replace_calls": lambda e: e.ctx.replace_calls(np.zeros(10, np.uint32)),
    "ku_ctx_enable_sparse": lambda e: e.ctx.enable_sparse(UNIT),
    "ku_ctx_disable_sparse": lambda e: e.ctx.disable_sparse(),
    "ku_sparse_close_unit": lambda e: e.ctx.sparse_close_unit(),
    "ku_sparse_export": lambda e: e.ctx.sparse_export(),
    "ku_classify_batch": lambda e: e.ctx.classify_batch(e.buf, e.off, e.lens),
    "ku_classify_batch_rle": lambda e: e.ctx.classify_batch_rle(e.buf, e.off, e.lens),
    "ku_classify_batch_rle_reserve": lambda e: e.ctx.rle_reserve(len(e.buf), e.n, int(e.lens.max()), 4),
    "ku_classify_batch_device": lambda e: e.ctx.classify_batch_device(e.p("seqs"), len(e.buf), e.p("off"), e.p("len"), e.n, e.p("calls"),
                                                                      e.p("taxa"), e.p("hits")),
    "ku_classify_batch_device_rle": lambda e: e.ctx.classify_batch_device_rle(e.p("seqs"), len(e.buf), e.p("off"), e.p("len"), e.n, e.p("calls"),
                                                                              e.p("runs"), len(e.buf) + 1, e.p("roff"), e.p("rcnt"), e.p("n_runs"),
                                                                              int(e.lens.max())),
    "ku_lookup_device": lambda e: e.ctx.lookup_device(e.p("seqs"), len(e.buf), e.p("taxa")),
    "ku_resolve_device": lambda e: e.ctx.resolve_device(e.p("seqs"), e.p("off"), e.p("len"), e.n, e.p("calls"), e.p("taxa"), e.p("hits")),
    "ku_lookup_stats_device": lambda e: e.ctx.lookup_stats_device(e.p("seqs"), len(e.buf)),
    "ku_batch_create": lambda e: e.ctx.batch(e.buf, e.off, e.lens),
    "ku_batch_lookup": lambda e: e.batches[0].lookup(),
    "ku_batch_finish": lambda e: e.batches[0].finish(),
    "ku_batch_absorb": _absorb,
}
DEVICE_ROWS = ("ku_ctx_adopt_db", "ku_classify_batch_device", "ku_classify_batch_device_rle", "ku_lookup_device", "ku_resolve_device",
               "ku_lookup_stats_device")
CTX_REFUSE = [r for r in ic.rows(ic.REFUSE) if not r.startswith("ku_mgpu_")]
MGPU_REFUSE = [r for r in ic.rows(ic.REFUSE) if r.startswith("ku_mgpu_")]


def test_every_refuse_row_is_probed():
    assert sorted(REFUSE_CALLS) == CTX_REFUSE
    assert sorted(MGPU_CALLS) == MGPU_REFUSE


def _check_run(ctx, ctax, cuts, results, mode):
    """the run after the refused call equals one without it: text, calls, state, the emulation's sets, the report"""
    ids, seqs, buf, off, lens = f1()
    run = oracle_run(UNIT if mode == "sparse" else 0)
    assert kraken_text(buf, off, lens, ids, cuts, results) == open(f"{F1}/out.tsv").read()
    text = ctx.report(ctax, COUNTS)
    if mode == "sparse":
        counts, flags, pairs, n_sparse, n_dense = assert_sparse_state_equals_oracle(ctx, run)
        gc.assert_same_counts(counts, run)
        assert rows(text) == rows(open(f"{F1}/report_u1000.tsv").read())
    elif mode == "exact":
        gc.assert_same_counts(ctx.counts(), run)
        assert rows(text) == rows(open(f"{F1}/report_exact.tsv").read())
    else:
        gc.assert_same_counts(ctx.counts(), run)
        assert text == plain_report()
    assert rows(ctx.report(ctax, COUNTS, flags=1)) == rows(open(f"{F1}/report_p0.tsv").read())


def _refuse_case(row, mode, call):
    ids, seqs, buf, off, lens = f1()
    cuts = split_points(len(seqs), 3, 41)
    ctx, cdb, ctax = gc.make_ctx(F1)
    if mode == "sparse":
        ctx.enable_sparse(UNIT)
    if mode == "exact":
        ctx.enable_exact(20)
    env = Env(ctx, cdb, ctax, buf, off, lens)
    if row in ("ku_batch_lookup", "ku_batch_finish", "ku_batch_absorb"):
        env.batches = [ctx.batch(buf, off, lens), ctx.batch(buf, off, lens)]  # (created while idle: an upload, no state)
    if row in DEVICE_ROWS:
        env.dev()  # (before the batches: torch's copies and its device-wide synchronisation must not wait for them)
    parts = list(batches_of(buf, off, lens, cuts))
    jobs, results = [], []
    # exact counting cannot overlap: one batch in flight (classified inside _enqueue), which must still be refused
    first = 1 if mode == "exact" else len(parts)
    pins = [pinned_batch(bb, bo, bl) for (a, b, bb, bo, bl) in parts]
    try:
        for arr, po, pl, out in pins[:first]:
            jobs.append(ctx.rle_enqueue(arr, po, pl, out=out))
        assert ctx.rle_in_flight() == first
        st = call(env)
        assert st == KU_ESTATE, (row, st)
        assert ctx.rle_in_flight() == first
        for j in jobs:
            results.append(ctx.rle_finish(j))
    finally:
        drain(ctx)
    for arr, po, pl, out in pins[first:]:
        results.append(ctx.rle_finish(ctx.rle_enqueue(arr, po, pl, out=out)))
    assert ctx.rle_in_flight() == 0
    _check_run(ctx, ctax, cuts, results, mode)
    if mode == "exact":
        ctx2, _, _ = gc.make_ctx(F1)
        ctx2.enable_exact(20)
        ctx2.classify_batch_rle(buf, off, lens)
        assert np.array_equal(ctx.exact_counts(), ctx2.exact_counts())
        ctx2.close()
    for b in env.batches:
        b.close()
    ctx.close()


@pytest.mark.parametrize("mode", ["plain", "sparse"])
@pytest.mark.parametrize("row", [r for r in CTX_REFUSE if r != "ku_ctx_merge_state"])
def test_refused_while_in_flight_and_nothing_changed(row, mode):
    _refuse_case(row, mode, lambda e: status_of(lambda: REFUSE_CALLS[row](e)))


def test_counts_export_exact_is_refused_with_its_one_batch_in_flight():
    _refuse_case("ku_counts_export_exact", "exact", lambda e: status_of(lambda: REFUSE_CALLS["ku_counts_export_exact"](e)))


@pytest.mark.parametrize("mode", ["plain", "sparse"])
@pytest.mark.parametrize("side", ["dst", "src"])
def test_merge_state_is_refused_on_either_side(side, mode):
    """dst has batches in flight (its counters are still written) or src has (a partial state would be merged, once)"""
    idle, _, _ = gc.make_ctx(F1)

    def call(e):
        return status_of(lambda: e.ctx.merge_state(idle) if side == "dst" else idle.merge_state(e.ctx))

    _refuse_case("ku_ctx_merge_state", mode, call)
    c = idle.counts()  # the idle side took nothing either
    assert not c["n_kmers"].any() and not c["n_reads"].any() and not c["registers"].any()
    idle.close()


# ---------------------------------------------------------------------------- allowed
def _allowed_answers(ctx):
    L = capi.lib()
    import ctypes as C
    d = capi.CountsDims()
    assert L.ku_counts_dims_get(ctx.h, C.byref(d)) == 0
    free, total = C.c_uint64(), C.c_uint64()
    assert L.ku_ctx_mem_info(ctx.h, C.byref(free), C.byref(total)) == 0
    t, c = ctx.count_taxons()
    t1, c1 = ctx.count_taxons(0)
    return {"dims": (d.n_slots, d.n_nodes), "layout": ctx.db_layout(), "values": ctx.db_values().tolist(), "count_taxons": (t.tolist(), c.tolist()),
            "count_taxons_db": (t1.tolist(), c1.tolist()), "mem_total": total.value, "sparse_state": ctx.sparse_state(),
            "device_ptrs": ctx.counts_device_ptrs(), "runs_cap": ctx.device_rle_runs_cap(150000, 1000, 151)}


@pytest.mark.parametrize("mode", ["plain", "sparse"])
def test_allowed_rows_answer_as_on_an_idle_context(mode):
    ids, seqs, buf, off, lens = f1()
    cuts = split_points(len(seqs), 4, 5)
    ctx, cdb, ctax = gc.make_ctx(F1)
    if mode == "sparse":
        ctx.enable_sparse(UNIT)
    idle = _allowed_answers(ctx)
    want_counts = dict(tuple(map(int, ln.split("\t"))) for ln in open(COUNTS[0]).read().split("\n") if ln)
    assert dict(zip(*idle["count_taxons"])) == want_counts
    pins = [pinned_batch(bb, bo, bl) for (a, b, bb, bo, bl) in batches_of(buf, off, lens, cuts)]
    try:
        jobs = [ctx.rle_enqueue(arr, po, pl, out=out) for arr, po, pl, out in pins]
        assert ctx.rle_in_flight() == 4
        assert _allowed_answers(ctx) == idle
        results = [ctx.rle_finish(jobs[0])]
        # ku_fetch_runs: the batch finished last, while the other three are still in flight
        n = len(results[0]["runs"])
        again = np.zeros((max(n, 1), 2), np.uint32)
        capi._chk(capi.lib().ku_fetch_runs(ctx.h, again.ctypes.data, n), "ku_fetch_runs")
        assert np.array_equal(again[:n], results[0]["runs"])
        assert ctx.rle_in_flight() == 3 and _allowed_answers(ctx) == idle
        results += [ctx.rle_finish(j) for j in jobs[1:]]
    finally:
        drain(ctx)
    _check_run(ctx, ctax, cuts, results, mode)
    ctx.close()


# ---------------------------------------------------------------------------- wait
BIG_READS = 131072  # per batch: four of them are still in flight well after the last _enqueue returns


def big_batches(n_batches=4):
    """reads of f1 repeated, each batch a different rotation of them"""
    ids, seqs, buf, off, lens = f1()
    reps = -(-BIG_READS // len(seqs))
    out = []
    for i in range(n_batches):
        s = (seqs[i * 97:] + seqs[:i * 97]) * reps
        bb, bo, bl = ko.pack_reads(s[:BIG_READS])
        out.append((bb, bo, bl))
    return out


def per_read_runs(r):
    """the runs of every read in read order (the run array's layout differs between launches: chunks are claimed by waves)"""
    cnt = r["run_cnt"].astype(np.int64)
    starts = np.repeat(r["run_off"].astype(np.int64), cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    return r["runs"][starts]


def test_synchronize_waits_for_the_batches_in_flight():
    """sentinels in the page-locked outputs: right after ku_ctx_synchronize every output array holds the batch's results --
    calls, per-read run offsets / counts and the runs themselves -- equal to the one-step call's; _finish then returns the same"""
    batches = big_batches()
    ref_ctx, _, _ = gc.make_ctx(F1)
    want = [ref_ctx.classify_batch_rle(bb, bo, bl) for bb, bo, bl in batches]
    ref_ctx.close()
    ctx, cdb, ctax = gc.make_ctx(F1)
    pins = [pinned_batch(bb, bo, bl, fill=SENTINEL) for bb, bo, bl in batches]
    try:
        jobs = [ctx.rle_enqueue(arr, po, pl, out=out) for arr, po, pl, out in pins]
        ctx.synchronize()
        # straight away, what the copies have delivered: the small arrays first, the batch enqueued last first (copying a
        # run buffer of tens of MB first would give the batches behind it the time to land on their own)
        snap = [{} for _ in pins]
        for i in reversed(range(len(pins))):
            for key in ("calls", "run_cnt", "run_off"):
                snap[i][key] = pins[i][3][key].copy()
        for i in reversed(range(len(pins))):
            snap[i]["runs"] = pins[i][3]["runs"].copy()
        assert ctx.rle_in_flight() == 4
        res = [ctx.rle_finish(j) for j in jobs]
    finally:
        drain(ctx)
    for i, (s, w) in enumerate(zip(snap, want)):
        n = len(w["calls"])
        for key in ("calls", "run_cnt"):
            assert not (s[key][:n] == SENTINEL).any(), (i, key, int((s[key][:n] == SENTINEL).sum()))
        assert not (s["run_off"][:n] == np.uint64(SENTINEL)).any(), (i, "run_off")
        assert int((s["run_off"][:n] + s["run_cnt"][:n]).max()) <= len(s["runs"]), i  # (the runs came with the calls)
        assert np.array_equal(s["calls"][:n], w["calls"]), i
        assert np.array_equal(s["run_cnt"][:n], w["run_cnt"]), i
        got = {"run_off": s["run_off"][:n], "run_cnt": s["run_cnt"][:n], "runs": s["runs"]}
        assert np.array_equal(per_read_runs(got), per_read_runs(w)), i
    assert ctx.rle_in_flight() == 0
    for r, w in zip(res, want):
        assert np.array_equal(r["calls"], w["calls"]) and np.array_equal(r["run_cnt"], w["run_cnt"])
        assert np.array_equal(per_read_runs(r), per_read_runs(w))
    ctx.close()


DESTROY_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
import gpu_common as gc
import test_gpu_inflight as t
batches = t.big_batches()
ref, _, _ = gc.make_ctx(t.F1)
want = [ref.classify_batch_rle(bb, bo, bl) for bb, bo, bl in batches]
ref.close()
ctx, cdb, ctax = gc.make_ctx(t.F1)
pins = [t.pinned_batch(bb, bo, bl, fill=t.SENTINEL) for bb, bo, bl in batches]
jobs = [ctx.rle_enqueue(arr, po, pl, out=out) for arr, po, pl, out in pins]
assert ctx.rle_in_flight() == 4
ctx.close()
for i, ((_, _, _, out), w) in enumerate(zip(pins, want)):
    n = len(w["calls"])
    assert np.array_equal(out["calls"][:n], w["calls"]), ("calls", i)
    assert np.array_equal(out["run_cnt"][:n], w["run_cnt"]), ("run_cnt", i)
    got = {"run_off": out["run_off"][:n], "run_cnt": out["run_cnt"][:n], "runs": out["runs"]}
    assert np.array_equal(t.per_read_runs(got), t.per_read_runs(w)), ("runs", i)
print("destroy-child-ok")
"""


def test_destroy_waits_for_the_batches_in_flight():
    """ku_ctx_destroy with four batches in flight, in a process of its own: their copies into the caller's page-locked buffers
    complete before anything is freed -- the buffers equal the one-step results and the process exits cleanly"""
    p = subprocess.Popen([sys.executable, "-c", DESTROY_CHILD, ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         cwd=ROOT)
    try:
        out = p.communicate(timeout=240)[0]
    except subprocess.TimeoutExpired:
        p.kill()
        out = p.communicate()[0]
        pytest.fail("the child did not finish in time:\n" + out[-4000:])
    assert p.returncode == 0 and "destroy-child-ok" in out, (p.returncode, out[-4000:])


# ---------------------------------------------------------------------------- growth of the run-wide set in flight
@pytest.mark.parametrize("unit,report", [(1000, "report_u1000.tsv"), (20000, None)])
def test_run_wide_set_grows_while_batches_are_in_flight(unit, report):
    """global_log2 = 10: the (slot, encoding) set starts at 1024 cells and is rehashed into larger tables while up to four
    batches are in flight (sparse_reserve_global waits for their copies back, the set's size among them)"""
    ids, seqs, buf, off, lens = f1()
    cuts = split_points(len(seqs), 13, 29)
    ctx, cdb, ctax = gc.make_ctx(F1)
    ctx.enable_sparse(unit, global_log2=10)
    res = run_two_step(ctx, buf, off, lens, cuts, depth=4)
    assert kraken_text(buf, off, lens, ids, cuts, res) == open(f"{F1}/out.tsv").read()
    run = oracle_run(unit)
    text = ctx.report(ctax, COUNTS)
    counts, flags, pairs, n_sparse, n_dense = assert_sparse_state_equals_oracle(ctx, run)
    gc.assert_same_counts(counts, run)
    assert len(pairs) > 1 << 9  # more than half of the first table's cells: the set did grow
    assert rows(text) == rows(capi.report_sparse(ctax, counts, flags, pairs, COUNTS))
    if report:
        assert rows(text) == rows(open(os.path.join(F1, report)).read())
    ctx.close()


# ---------------------------------------------------------------------------- group
def _step_args(mg, dev):
    W = mg.n_local
    N = dev["n"]
    rb = [N * r // W for r in range(W + 1)]
    pb = [int(dev["off_h"][x]) if x < N else dev["nb"] for x in rb]
    return [{"d_seqs": dev["seqs"].data_ptr(), "d_seq_off": dev["off"].data_ptr(), "d_seq_len": dev["len"].data_ptr(),
             "d_calls": dev["calls"].data_ptr(), "d_taxa": dev["taxa"].data_ptr()} for _ in range(W)], dev["nb"], N, rb, pb


MGPU_CALLS = {
    "ku_mgpu_load": lambda g: g.mg.load(g.cdb, g.ctax),
    "ku_mgpu_load_dbs": lambda g: g.mg.load_dbs([g.cdb, g.cdb], g.ctax),
    "ku_mgpu_set_taxonomy": lambda g: g.mg.set_taxonomy(g.ctax),
    "ku_mgpu_enable_sparse": lambda g: g.mg.enable_sparse(UNIT),
    "ku_mgpu_sparse_close_unit": lambda g: g.mg.sparse_close_unit(),
    "ku_mgpu_enable_exact": lambda g: g.mg.enable_exact(20),
    "ku_mgpu_classify_batch_rle": lambda g: g.mg.classify_batch_rle(g.buf, g.off, g.lens),
    "ku_mgpu_step_device": lambda g: g.mg.step_device(*_step_args(g.mg, g.dev), max_read_len=int(g.lens.max())),
    "ku_mgpu_reduce_state": lambda g: g.mg.reduce_state(),
}


@pytest.mark.parametrize("flags", [0, capi.KU_MGPU_REPLICAS])
def test_group_refuses_while_a_rank_context_has_batches_in_flight(flags):
    """batches (count-less) enqueued straight on a rank context (ku_mgpu_ctx): everything of the group that classifies,
    reduces, loads or changes state answers KU_ESTATE, its queries still answer; once they are finished the group's run
    equals the reference's output and the oracle's state"""
    import torch
    ids, seqs, buf, off, lens = f1()
    mg = capi.Mgpu([0, 0, 0], flags=flags)
    cdb = capi.Db(f"{F1}/database.kdb", f"{F1}/database.idx")
    ctax = capi.Tax(f"{F1}/taxDB")
    mg.load(cdb, ctax)
    want_counts = dict(tuple(map(int, ln.split("\t"))) for ln in open(COUNTS[0]).read().split("\n") if ln)
    t, c = mg.count_taxons()
    assert dict(zip(t.tolist(), c.tolist())) == want_counts
    queries = lambda: (mg.uses_rccl(), mg.uses_routing(), mg.sparse_state(), mg.ctx(1).h.value)
    idle_q = queries()

    class G:
        pass
    g = G()
    g.mg, g.cdb, g.ctax, g.buf, g.off, g.lens = mg, cdb, ctax, buf, off, lens
    d = "cuda:0"
    g.dev = {"seqs": torch.cat([torch.frombuffer(bytearray(buf), dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8)]).to(d),
             "off": torch.from_numpy(off.astype(np.int64)).to(d), "len": torch.from_numpy(lens.astype(np.int32)).to(d),
             "calls": torch.zeros(len(lens), dtype=torch.int32, device=d), "taxa": torch.zeros(len(buf) + 16, dtype=torch.int32, device=d),
             "n": len(lens), "nb": len(buf), "off_h": off}
    torch.cuda.synchronize()
    r0 = mg.ctx(0)
    # replicas: the rank holds the whole database and takes the fused two-step path (several batches really in flight);
    # a shard cannot overlap: its one batch is classified inside _enqueue and still counts as in flight until _finish
    cuts = split_points(len(seqs), 3, 11) if flags else [0, len(seqs)]
    pins = [pinned_batch(bb, bo, bl) for (a, b, bb, bo, bl) in batches_of(buf, off, lens, cuts)]
    try:
        jobs = [r0.rle_enqueue(arr, po, pl, flags=capi.KU_F_NO_COUNTS, out=out) for arr, po, pl, out in pins]
        assert r0.rle_in_flight() == len(jobs)
        for row in MGPU_REFUSE:
            st = status_of(lambda: MGPU_CALLS[row](g))
            assert st == KU_ESTATE, (row, st)
        t, c = mg.count_taxons()
        assert dict(zip(t.tolist(), c.tolist())) == want_counts
        assert queries() == idle_q
        assert r0.rle_in_flight() == len(jobs)
        res = [r0.rle_finish(j) for j in jobs]
    finally:
        drain(r0)
    if flags:  # the rank's own batches: the whole database, the reference's lines
        assert kraken_text(buf, off, lens, ids, cuts, res) == open(f"{F1}/out.tsv").read()
    # the group's run over the reads: as if nothing had been refused
    out = mg.classify_batch_rle(buf, off, lens)
    assert capi.format_kraken_rle(buf, off, lens, ids, K, out) == open(f"{F1}/out.tsv").read()
    mg.reduce_state()
    run = oracle_run(0)
    for i in range(3):
        gc.assert_same_counts(mg.ctx(i).counts(), run)
    mg.close()
