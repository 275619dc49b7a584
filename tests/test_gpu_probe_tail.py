"""-m gpu: the probe tail of the fused classify kernel (ku_short.hip, stage 4) against the oracle.

A lookup that its home line does not settle -- the first candidate entry is another k-mer's, or the bucket spilled into the
following line(s) -- is finished by the kernel's straggler pass; a lane that learns from the home header that it must go on
fetches the following line's header in the slot of the entry load.  At the default load factor of the probe table one lookup
in 120 takes that road; here the table is built at load 0.9 (chains over several lines, most buckets spilled) and 0.6 (mixed),
so that nearly every lookup does: whole genomes on both strands (every k-mer a hit, many of them lines away from home), reads
with substitutions (misses that walk to the end of a chain) and with `N`s, at the read lengths where the kernel changes its
shape -- 128 k-mers (both items of every lane live), 120, 70, 129 and 192 (three items per lane), ~400 and whole genomes
(windowed) --, in every output form: per-position codes, runs, the sparse-sketch emulation (SEEN marks in the line an entry
was FOUND in), and without accounting.  Databases of a few hundred k-mers at load 0.9 let a chain run past the table's last
line and wrap (not observable from outside: several seeds instead)."""
import numpy as np
import pytest

from krakenuniq_amd import capi, synth
from oracle import ku_oracle as ko
import gpu_common as gc

pytestmark = pytest.mark.gpu
K = 31
UNIT = 20000  # work unit of the sparse-sketch emulation (nt): several units per run

# name: (nt, KU_LOAD_FACTOR, genomes, genome length, seed)
TABLES = {
    "nt13_lf0.9": (13, "0.9", 8, 6000, 101),
    "nt15_lf0.9": (15, "0.9", 8, 5000, 102),
    "nt8_lf0.9": (8, "0.9", 8, 5500, 103),
    "nt13_lf0.6": (13, "0.6", 8, 5000, 104),
    "nt10_lf0.6": (10, "0.6", 8, 6000, 105),
    # a few hundred k-mers: a handful of lines, chains that run past the last one
    "tiny_nt13_s1": (13, "0.9", 3, 130, 201),
    "tiny_nt13_s2": (13, "0.9", 3, 140, 202),
    "tiny_nt13_s3": (13, "0.9", 2, 150, 203),
    "tiny_nt8_s4": (8, "0.9", 3, 125, 204),
    "tiny_nt13_s5": (13, "0.9", 4, 110, 205),
    "tiny_nt10_s6": (10, "0.9", 2, 135, 206),
}
BIG = [n for n in TABLES if not n.startswith("tiny")]
TINY = [n for n in TABLES if n.startswith("tiny")]

_tables = {}
_oracle = {}
_ctx = {}


def cut_reads(genomes, n_kmers, count, rng, sub=0.0, n_count=0):
    """`count` reads of exactly n_kmers k-mers cut from the genomes, either strand; substitutions at rate `sub`, n_count `N`s"""
    g = list(genomes.values())
    L = n_kmers + K - 1
    out = []
    for _ in range(count):
        src = g[int(rng.integers(0, len(g)))]
        if len(src) < L:  # (tiny databases: the genome itself, read round and round)
            src = np.tile(src, L // len(src) + 1)
        s = int(rng.integers(0, len(src) - L + 1))
        codes = src[s:s + L]
        if rng.random() < 0.5:
            codes = synth.revcomp_codes(codes)
        if sub:
            codes = synth.mutate(codes, sub, rng)
        text = bytearray(synth.codes_to_ascii(codes))
        for p in rng.integers(0, L, n_count).tolist():
            text[p] = ord("N")
        out.append(bytes(text))
    return out


def read_groups(genomes, rng, tiny):
    """three batches, one per shape of the kernel: up to 128 k-mers (two items per lane), up to 192 (three), beyond (windowed)"""
    c = (lambda n: max(2, n // 4)) if tiny else (lambda n: n)
    short = (cut_reads(genomes, 128, c(24), rng) + cut_reads(genomes, 128, c(16), rng, sub=0.025) +
             cut_reads(genomes, 120, c(12), rng, sub=0.03) + cut_reads(genomes, 70, c(12), rng, sub=0.02) +
             cut_reads(genomes, 128, c(8), rng, n_count=2) + cut_reads(genomes, 97, c(6), rng, sub=0.02, n_count=1) +
             [b"", b"ACGT" * 7, cut_reads(genomes, 1, 1, rng)[0]])
    mid = (cut_reads(genomes, 129, c(12), rng) + cut_reads(genomes, 192, c(16), rng) +
           cut_reads(genomes, 192, c(12), rng, sub=0.025) + cut_reads(genomes, 160, c(8), rng, sub=0.02, n_count=2))
    whole = [synth.codes_to_ascii(g) for g in genomes.values()]
    whole += [synth.codes_to_ascii(synth.revcomp_codes(g)) for g in genomes.values()]
    long_ = ([w for w in whole if len(w) >= K] + cut_reads(genomes, 400, c(8), rng) +
             cut_reads(genomes, 400, c(8), rng, sub=0.025) + cut_reads(genomes, 391, c(4), rng, sub=0.02, n_count=3))
    return [short, mid, long_]


def table(name):
    """database, reads and the packed batches of one table -- built once, never changed"""
    if name not in _tables:
        nt, lf, n_genomes, glen, seed = TABLES[name]
        rng = np.random.default_rng(seed)
        db = gc.random_db(rng, n_genomes=n_genomes, glen=glen, nt=nt)
        ids, par = db["tax"].arrays()
        groups = read_groups(db["genomes"], rng, name.startswith("tiny"))
        _tables[name] = {"nt": nt, "lf": lf, "raw": db["pairs"].view(np.uint8), "key_ct": len(db["kmers"]), "offsets": db["offsets"],
                         "ids": ids, "par": par, "groups": groups, "packed": [ko.pack_reads(g) for g in groups]}
    return _tables[name]


def oracle(name, unit=None):
    """the oracle's run over the table's reads, group after group (its state is the run's): once per (table, work unit)"""
    if (name, unit) not in _oracle:
        t = table(name)
        odb = ko.Db(pairs=t["raw"], key_ct=t["key_ct"], k=K, offsets=t["offsets"], nt=t["nt"])
        otax = ko.Tax(ids=t["ids"], parents=t["par"])
        run = ko.Run(odb, otax, **({} if unit is None else {"work_unit_nt": unit}))
        res = run.classify([r for g in t["groups"] for r in g])
        codes = []
        for i in range(len(res["calls"])):
            a, n = int(res["taxa_off"][i]), int(res["n_slots"][i])
            c = res["taxa"][a:a + n].copy()
            c[res["ambig"][a:a + n] != 0] = capi.KU_AMBIG
            codes.append(c)
        _oracle[(name, unit)] = {"run": run, "calls": res["calls"].copy(), "codes": codes, "keep": (odb, otax)}
    return _oracle[(name, unit)]


def context(name, monkeypatch):
    """the table's context, with nothing counted: one per table (the index of nt = 15 has 4^15 bins -- seconds to upload)"""
    if name not in _ctx:
        t = table(name)
        monkeypatch.setenv("KU_LOAD_FACTOR", t["lf"])  # (read when the context is created)
        ctx, _, ctax = gc.make_ctx(cdb=capi.Db(pairs=t["raw"], key_ct=t["key_ct"], k=K, offsets=t["offsets"], nt=t["nt"]),
                                   ctax=capi.Tax(ids=t["ids"], parents=t["par"]))
        assert ctx.db_layout()["hash"]
        _ctx[name] = (ctx, ctax)
    ctx, ctax = _ctx[name]
    ctx.disable_sparse()
    ctx.reset_counts()
    return ctx, ctax


@pytest.fixture(scope="module", autouse=True)
def release_everything():
    yield
    for ctx, _ in _ctx.values():
        ctx.close()
    _ctx.clear()
    _oracle.clear()
    _tables.clear()


def batches(name, sizes=None):
    """(first read, packed batch) of every group -- or, with `sizes`, the groups cut into batches of those sizes in turn"""
    t = table(name)
    first = 0
    for g, packed in zip(t["groups"], t["packed"]):
        if sizes is None:
            yield first, packed
        else:
            a, i = 0, 0
            while a < len(g):
                b = min(a + sizes[i % len(sizes)], len(g))
                yield first + a, ko.pack_reads(g[a:b])
                a, i = b, i + 1
        first += len(g)


def codes_of_taxa(gpu, off, lens):
    return [gpu["taxa"][int(o):int(o) + max(int(l) - K + 1, 0)] for o, l in zip(off.tolist(), lens.tolist())]


def codes_of_runs(rle, lens):
    out = []
    for i, l in enumerate(lens.tolist()):
        n = max(l - K + 1, 0)
        a, c = int(rle["run_off"][i]), int(rle["run_cnt"][i])
        rr = rle["runs"][a:a + c]
        assert (c == 0) == (n == 0), i
        if c:
            assert rr[0, 1] == 0 and np.all(np.diff(rr[:, 1].astype(np.int64)) > 0) and rr[-1, 1] < n, i
            assert np.all(rr[1:, 0] != rr[:-1, 0]), i  # maximal runs
            out.append(np.repeat(rr[:, 0], np.diff(np.r_[rr[:, 1], n])))
        else:
            out.append(np.zeros(0, dtype=np.uint32))
    return out


def assert_batch(want, first, calls, codes):
    n = len(calls)
    assert (calls == want["calls"][first:first + n]).all(), (first, np.nonzero(calls != want["calls"][first:first + n])[0][:10])
    for i, c in enumerate(codes):
        w = want["codes"][first + i]
        assert len(c) == len(w) and (c == w).all(), (first + i, len(w), np.nonzero(c != w)[0][:10])


def run_codes(ctx, name, want, sizes=None, flags=0):
    for first, (buf, off, lens) in batches(name, sizes):
        gpu = ctx.classify_batch(buf, off, lens, flags=flags)
        assert_batch(want, first, gpu["calls"], codes_of_taxa(gpu, off, lens))


def run_runs(ctx, name, want, sizes=None):
    for first, (buf, off, lens) in batches(name, sizes):
        rle = ctx.classify_batch_rle(buf, off, lens)
        assert_batch(want, first, rle["calls"], codes_of_runs(rle, lens))


def assert_sparse_state(ctx, run):
    """which sketches stayed sparse, and their sets of encoded hashes (the marked table entries + the run-wide set's misses)"""
    counts = ctx.counts()
    flags, pairs = ctx.sparse_export()
    slot_of = {int(t): s for s, t in enumerate(counts["slot_taxid"])}
    got = {}
    for p in pairs.tolist():
        got.setdefault(p >> 32, set()).add(p & 0xFFFFFFFF)
    n_sparse = 0
    for t, c in run.counts().items():
        if not c["n_kmers"]:
            continue
        s = slot_of[t]
        assert bool(flags[s]) == c["sparse"], (t, c["n_kmers"])
        if c["sparse"]:
            assert got.get(s, set()) == set(c["sketch"].sparse_list().tolist()), t
            n_sparse += 1
    return counts, n_sparse


@pytest.mark.parametrize("name", BIG + TINY)
def test_codes_calls_counts_and_registers(name, monkeypatch):
    """classify_batch: per-k-mer codes, calls, n_kmers / n_reads and the HLL registers, bit for bit"""
    want = oracle(name)
    ctx, _ = context(name, monkeypatch)
    run_codes(ctx, name, want)
    gc.assert_same_counts(ctx.counts(), want["run"])
    if name in BIG:  # every k-mer of the database was found (whole genomes, both strands): none is a miss, wherever it lies
        hits = sum(int(np.count_nonzero((c != 0) & (c != capi.KU_AMBIG))) for c in want["codes"])
        assert hits > 2 * table(name)["key_ct"]


@pytest.mark.parametrize("name", BIG + TINY)
def test_runs_expand_to_the_codes(name, monkeypatch):
    """classify_batch_rle: the kernel's runs, expanded, are the oracle's codes; the same state"""
    want = oracle(name)
    ctx, _ = context(name, monkeypatch)
    run_runs(ctx, name, want)
    gc.assert_same_counts(ctx.counts(), want["run"])


@pytest.mark.parametrize("name", BIG + TINY[:3])
def test_sparse_emulation_marks_the_entry_where_it_was_found(name, monkeypatch):
    """enable_sparse: a k-mer found lines away from home is booked by the SEEN byte of THAT line's entry -- the exported sets
    of (slot, encoded hash) equal the oracle's sparse sketches, and so does the report over them"""
    want = oracle(name, UNIT)
    ctx, ctax = context(name, monkeypatch)
    ctx.enable_sparse(UNIT)
    run_runs(ctx, name, want)
    counts, n_sparse = assert_sparse_state(ctx, want["run"])
    assert n_sparse > 0
    gc.assert_same_counts(counts, want["run"])
    flags, pairs = ctx.sparse_export()
    assert ctx.report(ctax, []) == capi.report_sparse(ctax, counts, flags, pairs, [])


@pytest.mark.parametrize("name", BIG[:1] + BIG[2:4] + TINY[:2])
def test_without_accounting(name, monkeypatch):
    """KU_F_NO_COUNTS: the same codes and calls, the per-taxon state untouched"""
    want = oracle(name)
    ctx, _ = context(name, monkeypatch)
    run_codes(ctx, name, want, flags=capi.KU_F_NO_COUNTS)
    c = ctx.counts()
    assert int(c["n_kmers"].sum()) == 0 and int(c["n_reads"].sum()) == 0 and not c["registers"].any()


@pytest.mark.parametrize("form", ["codes", "runs"])
@pytest.mark.parametrize("name", BIG[:1] + BIG[3:4] + TINY[:1])
def test_batches_of_one_and_three_reads(name, form, monkeypatch):
    """one wave, then three: launches smaller than a block"""
    want = oracle(name)
    ctx, _ = context(name, monkeypatch)
    (run_codes if form == "codes" else run_runs)(ctx, name, want, sizes=(1, 3))
    gc.assert_same_counts(ctx.counts(), want["run"])
