"""-m gpu: the HLL floors of the fused classify kernel (ku_short.hip; KuCountsDev::hll_floor) against the oracle.

The kernel drops a k-mer whose HLL rank does not exceed the floor of its slot -- a lower bound of the slot's 4096 registers that
the kernel itself raises by scanning a row every KU_HLL_FLOOR_EVERY reads of a wave -- before the register is looked at.  Wrong
would be: a floor above a register (inserts lost from then on), a floor that survives ku_ctx_reset_counts (the rank-1 inserts
of the next run lost), a filter that changes anything but the loads.  None of it shows on a state the filter never engages on,
so the database has one taxon T with a genome of 131 072 bases next to a few of 4 000: batch P tiles T's genome (and brings as
many random reads), after which the rows of T's slot and of slot 0 (the misses') hold no zero -- asserted on the oracle's
registers -- and their floors rise; the rare taxa's rows keep empty registers and their floors stay 0.  Batch Q then brings
substituted reads of T, reads of the rare taxa and random ones onto the raised floors.  Every case runs with
KU_SHORT_BLOCKS_PER_CU=1 (waves take several reads each) and KU_HLL_FLOOR_EVERY=1 (a scan after every read) unless it says
otherwise, and compares the whole per-taxon state bit for bit.

Shapes: `short` 150 bp (ITEMS = 2, one pass), `pairs` 2 x 150 joined by N (windowed), `long` 180 bp = 150 k-mers (ITEMS = 3)."""
import numpy as np
import pytest

from krakenuniq_amd import capi, synth
from oracle import ku_oracle as ko
import gpu_common as gc

pytestmark = pytest.mark.gpu
K, NT = 31, 13
GLEN, RARE_LEN, N_RARE = 131072, 4000, 3
UNIT = 200000  # work unit of the sparse-sketch emulation (nt)

_db = {}
_reads = {}
_oracle = {}
_ctx = []


def database():
    """T (the first species) with a long genome, N_RARE taxa with short ones; unrelated random sequences -- built once"""
    if not _db:
        rng = np.random.default_rng(4242)
        tax = synth.random_taxonomy(1 + N_RARE, rng, levels=(2, 3, 4, 5))
        genomes = {t: synth.procedural_genome(977 + i, i, GLEN if i == 0 else RARE_LEN) for i, t in enumerate(tax.species)}
        kmers, vals = synth.lca_database(genomes, tax, K)
        sk, sv, off = synth.sort_db(kmers, vals, K, NT)
        ids, par = tax.arrays()
        _db.update(raw=synth.pack_pairs(sk, sv).view(np.uint8), key_ct=len(sk), offsets=off, ids=ids, par=par, genomes=genomes,
                   T=tax.species[0], rare=list(tax.species[1:]))
    return _db


def _ascii(codes):
    return bytes(synth.codes_to_ascii(codes))


def _random_reads(rng, count, length):
    return [_ascii(rng.integers(0, 4, length).astype(np.uint8)) for _ in range(count)]


def _cut(genome, starts, length, rng, sub=0.0):
    out = []
    for s in starts:
        codes = genome[s:s + length]
        out.append(_ascii(synth.mutate(codes, sub, rng) if sub else codes))
    return out


def _pair_up(reads):
    return [a + b"N" + b for a, b in zip(reads[0::2], reads[1::2])]


def reads(shape):
    """{"P": ..., "Q": ...} of one shape -- built once, never changed"""
    if shape not in _reads:
        d = database()
        rng = np.random.default_rng({"short": 1, "pairs": 2, "long": 3}[shape])
        L = 180 if shape == "long" else 150
        g = d["genomes"][d["T"]]
        tiles = _cut(g, range(0, GLEN - L + 1, L - K + 1), L, rng)  # every k-mer of T but the last few
        tiles.append(_ascii(g[GLEN - L:]))
        p = tiles + _random_reads(rng, len(tiles) + (len(tiles) & 1), L)
        q = _cut(g, rng.integers(0, GLEN - L, 300).tolist(), L, rng, sub=0.03)
        for t in d["rare"]:
            q += _cut(d["genomes"][t], rng.integers(0, RARE_LEN - L, 40).tolist(), L, rng, sub=0.01)
        q += _random_reads(rng, 100, L)
        # reads of two taxa (the per-lane floor gather): half T, half a rare taxon
        for t in d["rare"]:
            for s in rng.integers(0, RARE_LEN - L, 10).tolist():
                q.append(_ascii(np.concatenate([g[s:s + L // 2], d["genomes"][t][s:s + L - L // 2]])))
        if shape == "pairs":
            if len(tiles) & 1:
                p = p[1:]  # (an even number of T's tiles: every pair is two reads of one kind)
            p, q = _pair_up(p), _pair_up(q)
        _reads[shape] = {"P": p, "Q": q}
    return _reads[shape]


def batch(shape, name):
    """`P`, `Q`, or a slice of one: `Q[0:3]`"""
    r = reads(shape)
    if "[" in name:
        a, b = name[2:-1].split(":")
        return r[name[0]][int(a):int(b)]
    return r[name]


def oracle(shape, seq, unit=None):
    """the oracle's run over the batches named in `seq`, in order: once per (shape, seq, work unit), never changed afterwards"""
    key = (shape, seq, unit)
    if key not in _oracle:
        d = database()
        odb = ko.Db(pairs=d["raw"], key_ct=d["key_ct"], k=K, offsets=d["offsets"], nt=NT)
        otax = ko.Tax(ids=d["ids"], parents=d["par"])
        run = ko.Run(odb, otax, **({} if unit is None else {"work_unit_nt": unit}))
        calls, codes = [], []
        for name in seq:
            res = run.classify(batch(shape, name))
            calls.append(res["calls"].copy())
            cc = []
            for i in range(len(res["calls"])):
                a, n = int(res["taxa_off"][i]), int(res["n_slots"][i])
                c = res["taxa"][a:a + n].copy()
                c[res["ambig"][a:a + n] != 0] = capi.KU_AMBIG
                cc.append(c)
            codes.append(cc)
        _oracle[key] = {"run": run, "calls": calls, "codes": codes, "keep": (odb, otax)}
    return _oracle[key]


def oracle_registers(run):
    return {t: c["sketch"].registers() for t, c in run.counts().items() if c["n_kmers"]}


def test_precondition_the_rows_of_t_and_of_the_misses_are_full_after_p():
    """(on the oracle alone) no case below passes vacuously: after P the two rows the floors are to rise on hold no zero, the
    rare taxa's rows -- not touched by P, and never full after Q either -- do"""
    d = database()
    for shape in ("short", "pairs", "long"):
        regs = oracle_registers(oracle(shape, ("P",))["run"])
        assert regs[0].min() >= 1 and regs[d["T"]].min() >= 1, shape
        assert set(regs) == {0, d["T"]}, shape
        regs = oracle_registers(oracle(shape, ("P", "P", "Q"))["run"])
        for t in d["rare"]:
            assert regs[t].max() >= 1 and regs[t].min() == 0, (shape, t)


def new_context():
    d = database()
    ctx, _, _ = gc.make_ctx(cdb=capi.Db(pairs=d["raw"], key_ct=d["key_ct"], k=K, offsets=d["offsets"], nt=NT),
                            ctax=capi.Tax(ids=d["ids"], parents=d["par"]))
    assert ctx.db_layout()["hash"]
    return ctx


@pytest.fixture
def ctx(monkeypatch):
    """the module's context with an empty state, under the environment of the cases"""
    monkeypatch.setenv("KU_SHORT_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("KU_HLL_FLOOR_EVERY", "1")
    if not _ctx:
        _ctx.append(new_context())
    _ctx[0].disable_sparse()
    _ctx[0].reset_counts()
    return _ctx[0]


@pytest.fixture(scope="module", autouse=True)
def release_everything():
    yield
    for c in _ctx:
        c.close()
    _ctx.clear()
    _oracle.clear()
    _reads.clear()
    _db.clear()


# ---- the three entry points, each returning (calls, per-read codes)
def _expand(runs, roff, rcnt, lens):
    out = []
    for i, l in enumerate(lens.tolist()):
        n = max(l - K + 1, 0)
        a, c = int(roff[i]), int(rcnt[i])
        rr = runs[a:a + c]
        assert (c == 0) == (n == 0), i
        out.append(np.repeat(rr[:, 0], np.diff(np.r_[rr[:, 1], n])) if c else np.zeros(0, dtype=np.uint32))
    return out


def launch_device(ctx, seqs):
    """ku_classify_batch_device: per-position codes (OUT = 0)"""
    import torch
    buf, off, lens = ko.pack_reads(seqs)
    n, nb = len(lens), len(buf)
    d_seqs = torch.cat([torch.frombuffer(bytearray(buf), dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8)]).cuda()
    d_off, d_len = torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
    calls = torch.zeros(n, dtype=torch.int32, device="cuda")
    taxa = torch.zeros(nb + 16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.classify_batch_device(d_seqs.data_ptr(), nb, d_off.data_ptr(), d_len.data_ptr(), n, calls.data_ptr(), taxa.data_ptr(),
                              max_read_len=int(lens.max()))
    ctx.synchronize()
    t = taxa.cpu().numpy().view(np.uint32)
    return calls.cpu().numpy().view(np.uint32), [t[int(o):int(o) + max(int(l) - K + 1, 0)] for o, l in zip(off.tolist(), lens.tolist())]


def launch_device_rle(ctx, seqs):
    """ku_classify_batch_device_rle: the kernel's own runs (OUT = 1)"""
    import torch
    buf, off, lens = ko.pack_reads(seqs)
    n, nb, L = len(lens), len(buf), int(lens.max())
    d_seqs = torch.cat([torch.frombuffer(bytearray(buf), dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8)]).cuda()
    d_off, d_len = torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
    cap = ctx.device_rle_runs_cap(nb, n, L)
    calls = torch.zeros(n, dtype=torch.int32, device="cuda")
    runs = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    roff, rcnt = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    nruns = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.classify_batch_device_rle(d_seqs.data_ptr(), nb, d_off.data_ptr(), d_len.data_ptr(), n, calls.data_ptr(), runs.data_ptr(), cap,
                                  roff.data_ptr(), rcnt.data_ptr(), nruns.data_ptr(), max_read_len=L)
    ctx.synchronize()
    assert int(nruns.item()) <= cap
    return calls.cpu().numpy().view(np.uint32), _expand(runs.cpu().numpy().view(np.uint32), roff.cpu().numpy(), rcnt.cpu().numpy(), lens)


def launch_host_rle(ctx, seqs):
    """ku_classify_batch_rle (OUT = 1; OUT = 2 behind enable_sparse)"""
    buf, off, lens = ko.pack_reads(seqs)
    rle = ctx.classify_batch_rle(buf, off, lens)
    return rle["calls"], _expand(rle["runs"], rle["run_off"], rle["run_cnt"], lens)


def run_and_check(ctx, launch, shape, seq, want, first=0):
    """the batches of `seq`, one launch each; calls and codes against the oracle's batches first, first + 1, ..."""
    for i, name in enumerate(seq):
        calls, codes = launch(ctx, batch(shape, name))
        assert np.array_equal(calls, want["calls"][first + i]), (name, np.nonzero(calls != want["calls"][first + i])[0][:10])
        for r, (c, w) in enumerate(zip(codes, want["codes"][first + i])):
            assert len(c) == len(w) and (c == w).all(), (name, r)


def row_minima(counts):
    return counts["registers"].min(axis=1).astype(np.uint32)


def slots_of(counts):
    d = database()
    slot = {int(t): s for s, t in enumerate(counts["slot_taxid"])}
    return slot[d["T"]], [slot[t] for t in d["rare"]]


# ---- 1. bit-exact state across the floor's rise
@pytest.mark.parametrize("shape,form", [("short", "device"), ("short", "device_rle"), ("short", "sparse"), ("pairs", "device"),
                                        ("long", "device")])
def test_state_is_exact_across_the_rise_of_the_floors(shape, form, ctx):
    """P, P, Q: the second P runs on rising floors, Q on raised ones"""
    seq = ("P", "P", "Q")
    want = oracle(shape, seq, UNIT if form == "sparse" else None)
    if form == "sparse":
        ctx.enable_sparse(UNIT)
    run_and_check(ctx, {"device": launch_device, "device_rle": launch_device_rle, "sparse": launch_host_rle}[form], shape, seq, want)
    counts = ctx.counts()
    gc.assert_same_counts(counts, want["run"])
    t_slot, _ = slots_of(counts)
    fl = ctx.hll_floors()
    assert fl[0] >= 1 and fl[t_slot] >= 1, (fl[0], fl[t_slot])  # (the filter was at work)
    assert (fl <= row_minima(counts)).all()


# ---- 2. the filter engaged, the invariant held
def test_floors_rise_where_rows_are_full_and_nowhere_else(ctx):
    want = oracle("short", ("P", "P", "Q"))
    run_and_check(ctx, launch_device, "short", ("P", "P"), want)
    counts = ctx.counts()
    t_slot, rare = slots_of(counts)
    fl = ctx.hll_floors()
    assert fl.shape == (len(counts["slot_taxid"]),) and fl.dtype == np.uint32
    assert fl[0] >= 1 and fl[t_slot] >= 1, (fl[0], fl[t_slot])
    assert (fl <= row_minima(counts)).all()
    assert not fl[rare].any()
    # Q: reads of T and random ones (floors up: a handful of k-mers survive) and reads of the rare taxa (floor 0: every k-mer
    # goes on to its register) in one launch
    run_and_check(ctx, launch_device, "short", ("Q",), want, first=2)
    counts = ctx.counts()
    fl2 = ctx.hll_floors()
    assert (fl2 >= fl).all() and (fl2 <= row_minima(counts)).all()
    assert not fl2[rare].any()
    gc.assert_same_counts(counts, want["run"])
    for s in rare:
        assert counts["n_kmers"][s] > 0 and counts["registers"][s].any()


# ---- 3. reset clears the floors
def test_reset_counts_clears_the_floors(ctx):
    run_and_check(ctx, launch_device, "short", ("P", "P", "Q"), oracle("short", ("P", "P", "Q")))
    assert ctx.hll_floors()[0] >= 1
    ctx.reset_counts()
    assert not ctx.hll_floors().any()
    want = oracle("short", ("Q[0:3]",))
    run_and_check(ctx, launch_device, "short", ("Q[0:3]",), want)  # (a floor left standing would drop their low-rank inserts)
    gc.assert_same_counts(ctx.counts(), want["run"])


# ---- 4. launches of one and of three reads on raised floors
def test_launches_of_one_and_three_reads_on_raised_floors(ctx):
    """one wave, then three, each with a handful of k-mers the floors let through (P twice: the first launch fills the rows,
    the second one's scans find them full)"""
    seq = ("P", "P", "Q[0:1]", "Q[1:4]")
    want = oracle("short", seq)
    run_and_check(ctx, launch_device, "short", seq[:2], want)
    fl = ctx.hll_floors()
    t_slot, _ = slots_of(ctx.counts())
    assert fl[0] >= 1 and fl[t_slot] >= 1
    run_and_check(ctx, launch_device, "short", seq[2:], want, first=2)
    got = ctx.counts()
    gc.assert_same_counts(got, want["run"])
    assert (ctx.hll_floors() <= row_minima(got)).all()


# ---- 5. the knob changes nothing but the loads
def test_every_setting_of_the_knob_gives_the_same_state(ctx, monkeypatch):
    want = oracle("short", ("P", "Q"))
    states = {}
    for every in ("0", "1", "7", "64"):
        monkeypatch.setenv("KU_HLL_FLOOR_EVERY", every)
        ctx.reset_counts()
        calls = [launch_device(ctx, batch("short", name))[0] for name in ("P", "Q")]
        states[every] = (ctx.counts(), calls, ctx.hll_floors())
    assert not states["0"][2].any()  # (0: no floors at all)
    assert states["1"][2][0] >= 1
    base = states["0"]
    gc.assert_same_counts(base[0], want["run"])
    for every, (counts, calls, _) in states.items():
        for key in ("registers", "n_kmers", "n_reads"):
            assert np.array_equal(counts[key], base[0][key]), (every, key)
        for a, b in zip(calls, base[1]):
            assert np.array_equal(a, b), every


# ---- 6. a merge keeps the invariant
def test_merge_state_keeps_the_floors_below_the_rows(ctx):
    """ku_ctx_merge_state (the out-of-core run's helper contexts): Q's state of a second context joins P + P's"""
    seq = ("P", "P", "Q", "Q")
    want = oracle("short", seq)
    run_and_check(ctx, launch_device, "short", seq[:2], want)
    if len(_ctx) < 2:
        _ctx.append(new_context())
    other = _ctx[1]
    other.reset_counts()
    run_and_check(other, launch_device, "short", ("Q",), want, first=2)
    ctx.merge_state(other)
    counts = ctx.counts()
    fl = ctx.hll_floors()
    assert fl[0] >= 1 and (fl <= row_minima(counts)).all()
    run_and_check(ctx, launch_device, "short", ("Q",), want, first=3)
    gc.assert_same_counts(ctx.counts(), want["run"])
    assert (ctx.hll_floors() <= row_minima(ctx.counts())).all()
