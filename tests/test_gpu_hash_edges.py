"""-m gpu: what the classify kernels derive from ku_fmix64(canonical k-mer), at hash values no genome reaches.

The dense HLL rank, the HyperLogLog++ sparse encoding with its rank flag, the per-slot floor filter, the sparse-to-dense switch
at 1024 entries and the report's clade unions all hang on bits of the hash that k-mers of random or procedural genomes set
alike: the golden f1 run reaches register value 17 of 53 and not one flagged encoding.  Here the k-mers are built from the
hashes (tests/built_kmers.py; its promises are checked on the oracle alone in tests/test_built_kmers.py): canonical 31-mers
with a chosen register and rank, a chosen encoding, or two of them with one encoding.  Reads are built k-mers joined by N, so a
read books exactly those; 4, 5 and 8 of them per read make 97, 129 and 225 windows -- the fused kernel's instances of two and of
three items per lane and the windowed ones (ku_launch_classify_short selects by the longest read: <= 128, <= 192, more).  Every
case compares the whole per-taxon state with the oracle's run bit for bit; nothing here has a tolerance.

One database serves the module -- synth.small_taxonomy() plus every built k-mer, about 5 300 of them -- with nt = 13 (the
specialised instances), and once more with nt = 9 (the generic ones); no batch has more than 1 100 reads.

  a. a ladder of one k-mer per rank 1 .. 53 under taxon 4, registers 0 and 4095 among them, and the same ladder of k-mers the
     database does not hold (booked under slot 0), through the three host entry points, the staged kernels and quick mode;
  b. floors at height: taxon 4's row filled to 21 .. 25 with one register at 20, the floor risen, then k-mers at, one above and
     far above the floor -- the filter's `rank > floor` at a floor of 20, not of 1;
  c. the 1024-entry edge by ENCODINGS and ORDER: 1023 k-mers and two more that share one encoding leave the taxon dense when the
     pair comes last and sparse with 1024 entries when it comes first;
  d. flagged encodings (add 1 .. 40) and encodings shared between sibling species and between species that meet at the root,
     through the report's clade unions in both forms, and the same registers (up to 53) through the dense roll-up and estimator.

A hash with add = 39 or 40 (rank 52, 53) is the only one of its encoding, so two species cannot share such an encoding: in (d)
they hold one of each with encodings of their own, and share the adds 1, 2, 3, 13, 26, 27.

Not covered: the routed multi-GPU step (ku_mgpu_step_device: its resolve stage books no HLL inserts of its own and takes two
ranks) and k other than 31 (the builders make 31-mers; the generic instances run here through nt = 9 only)."""
from itertools import zip_longest

import numpy as np
import pytest

from krakenuniq_amd import capi, synth
from oracle import ku_oracle as ko
import built_kmers as bk
import gpu_common as gc
from test_gpu_sparse import assert_sparse_state_equals_oracle, classify_in_batches_by_path, rows

pytestmark = pytest.mark.gpu
K = 31
UNIT = 500000  # work unit of the sparse-sketch emulation (nt): every case is one unit
F = 20  # (b) the lowest register of taxon 4's row after batch P
MINREG, OTHERS = 1234, (0, 2000, 4095)  # (b) the register that sits at F; three others for the k-mers at the floor

_world = {}
_ctx = {}
_oracle_ladder = {}


# --------------------------------------------------------------------------- the k-mers, the database, the contexts
def _ladder(rng, shift):
    """[(rank, register, k-mer)]: rank 1 at register 0, rank 41 at 4095, the others spread from `shift` on; 52 and 53 where a
    k-mer exists (one hash per register there: two ladders with one shift would hold the same k-mer)"""
    out, used = [], set()
    for rank in range(1, 54):
        idx = {1: 0, 41: 4095}.get(rank, (rank * 79 + shift) % 4096)
        while True:
            h, v, at = bk.first_dense(idx, rank, rng)
            if at not in used:
                break
            idx = at + 1
        used.add(at)
        out.append((rank, at, v))
    assert {0, 4095} <= used
    return out


def _twins(make, *args):
    """two different k-mers from the same builder call"""
    a = make(*args)
    for _ in range(64):
        b = make(*args)
        if b[1] != a[1]:
            assert b[0] != a[0]
            return a[1], b[1]
    raise AssertionError("no second k-mer")


def world():
    """every built k-mer of the module and the database over them -- built once, never changed"""
    if _world:
        return _world
    w = {}
    # a. the ladders
    w["in"], w["out"] = _ladder(np.random.default_rng(11), 5), _ladder(np.random.default_rng(12), 1005)
    # b. one k-mer per register: F + 1 + idx % 5, MINREG at F; then what batch Q picks from
    rng = np.random.default_rng(13)
    w["row"] = [bk.dense(i, F if i == MINREG else F + 1 + i % 5, rng)[1] for i in range(4096)]
    w["min_f"], w["min_f1"] = bk.dense(MINREG, F, rng)[1], bk.dense(MINREG, F + 1, rng)[1]
    w["at_rank"] = {(i, r): bk.dense(i, r, rng)[1] for i in OTHERS for r in range(1, F + 2)}  # (the floor is read at run time)
    top = [bk.first_dense(s, 53, rng) for s in (300, 3000)]
    w["top"] = [(at, v) for _, v, at in top]
    w["taxon5_b"] = bk.dense(77, 3, rng)[1]  # a k-mer of another taxon for the read of several taxa
    # c. 1024 distinct unflagged encodings and a twin of the last
    rng = np.random.default_rng(14)
    top25 = set()
    while len(top25) < 1024:
        t = int(rng.integers(0, 1 << 25))
        if t & 0x1FFF:
            top25.add(t)
    top25 = sorted(top25)
    rng.shuffle(top25)
    w["edge"] = [bk.plain(t, rng)[1] for t in top25[:-1]]
    last, twin = _twins(bk.plain, top25[-1], rng)
    w["edge"].append(last)
    w["twin"] = twin
    # d. flagged encodings shared by the siblings 4 and 5, their own at add 39 / 40, two more of 5's; unflagged ones over one
    # register shared by 4 and 6
    rng = np.random.default_rng(15)
    s4, s5, s6 = [], [], []
    for add in (1, 2, 3, 13, 26, 27):
        a, b = _twins(bk.flagged, 100 + add, add, rng)
        s4.append(a)
        s5.append(b)
    own = {}
    for sp, start in ((4, 500), (5, 2500)):
        for add in (39, 40):
            h, v, at = bk.first_flagged(start, add, rng)
            own[(sp, add)] = at
            (s4 if sp == 4 else s5).append(v)
    assert len(set(own.values())) == 4
    s5 += [bk.flagged(700, 5, rng)[1], bk.flagged(701, 20, rng)[1]]
    w["n_flagged"] = (len(s4), len(s5))
    for r in range(1, 14):
        low = (1 << (13 - r)) | (int(rng.integers(0, 1 << 13)) & ((1 << (13 - r)) - 1))
        a, b = _twins(bk.plain, (900 << 13) | low, rng)
        s4.append(a)
        s6.append(b)
    w["s4"], w["s5"], w["s6"] = s4, s5, s6
    # the database
    of = {4: [v for _, _, v in w["in"]] + w["row"] + [w["min_f"], w["min_f1"]] + list(w["at_rank"].values())
          + [v for _, v in w["top"]] + s4,
          5: [w["taxon5_b"]] + w["edge"] + [w["twin"]] + s5, 6: s6}
    kmers = np.array([v for t in of for v in of[t]], dtype=np.uint64)
    vals = np.array([t for t in of for _ in of[t]], dtype=np.uint32)
    assert len(np.unique(kmers)) == len(kmers) < 10000
    assert not set(kmers.tolist()) & {v for _, _, v in w["out"]}
    w["kmers"], w["vals"] = kmers, vals
    w["tax"] = synth.small_taxonomy()
    _world.update(w)
    return _world


def db_arrays(nt):
    w = world()
    if ("db", nt) not in w:
        sk, sv, off = synth.sort_db(w["kmers"], w["vals"], K, nt)
        w[("db", nt)] = {"raw": synth.pack_pairs(sk, sv).view(np.uint8).reshape(-1), "key_ct": len(sk), "offsets": off}
    return w[("db", nt)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the taxDB and the counts file of the reports"""
    d = tmp_path_factory.mktemp("hash_edges")
    w = world()
    w["tax"].write(str(d / "taxDB"))
    t, c = np.unique(w["vals"], return_counts=True)
    (d / "database.kdb.counts").write_text("".join(f"{a}\t{b}\n" for a, b in zip(t.tolist(), c.tolist())))
    return {"taxdb": str(d / "taxDB"), "counts": str(d / "database.kdb.counts")}


def oracle_db(nt=13):
    d = db_arrays(nt)
    ids, par = world()["tax"].arrays()
    return (ko.Db(pairs=d["raw"], key_ct=d["key_ct"], k=K, offsets=d["offsets"], nt=nt), ko.Tax(ids=ids, parents=par))


def context(files, nt=13, layout="hash"):
    """the module's context of that geometry and layout, its state empty"""
    key = (nt, layout)
    if key not in _ctx:
        d = db_arrays(nt)
        mp = pytest.MonkeyPatch()
        if layout == "sorted":
            mp.setenv("KU_LAYOUT", "sorted")
        try:
            ctx, _, ctax = gc.make_ctx(cdb=capi.Db(pairs=d["raw"], key_ct=d["key_ct"], k=K, offsets=d["offsets"], nt=nt),
                                       ctax=capi.Tax(files["taxdb"]))
        finally:
            mp.undo()
        assert ctx.db_layout()["hash"] == (layout == "hash")
        _ctx[key] = (ctx, ctax)
    ctx, ctax = _ctx[key]
    ctx.disable_sparse()
    ctx.reset_counts()
    return ctx, ctax


@pytest.fixture(scope="module", autouse=True)
def release_everything():
    yield
    for ctx, _ in _ctx.values():
        ctx.close()
    _ctx.clear()
    _oracle_ladder.clear()
    _world.clear()


def slot_of(counts, taxid):
    return {int(t): s for s, t in enumerate(counts["slot_taxid"])}[taxid]


# --------------------------------------------------------------------------- a. the rank ladder
def ladder_reads(per):
    """the ladder the database holds, the one it does not, and the two interleaved (reads of hits and misses)"""
    w = world()
    a, b = [v for _, _, v in w["in"]], [v for _, _, v in w["out"]]
    mixed = [v for pair in zip(a, b) for v in pair]
    return bk.reads_of(a, per) + bk.reads_of(b, per) + bk.reads_of(mixed, per)


def ladder_oracle(per, nt=13, quick=False):
    """the oracle's run over ladder_reads(per): once per case, never changed afterwards"""
    key = (per, nt, quick)
    if key not in _oracle_ladder:
        odb, otax = oracle_db(nt)
        run, res, buf, off, lens, taxa = gc.oracle_flat(odb, otax, ladder_reads(per), work_unit_nt=UNIT,
                                                        **({"quick": True, "min_hits": 1} if quick else {}))
        _oracle_ladder[key] = {"run": run, "res": res, "packed": (buf, off, lens), "taxa": taxa, "keep": (odb, otax)}
    return _oracle_ladder[key]


def test_precondition_the_oracle_holds_both_ladders():
    """(on the oracle alone) taxon 4's row and the misses' hold every rank 1 .. 53 once, at the registers they were built for"""
    w = world()
    for per, quick in ((4, False), (5, False), (8, False), (1, True)):
        c = ladder_oracle(per, quick=quick)["run"].counts()
        for t, ladder in ((4, w["in"]), (0, w["out"])):
            regs = c[t]["sketch"].registers()
            assert {int(i): int(regs[i]) for i in np.flatnonzero(regs)} == {at: rank for rank, at, _ in ladder}, (per, t)
            assert c[t]["n_kmers"] == 2 * 53
        assert sorted(int(x) for x in c[4]["sketch"].registers() if x) == list(range(1, 54))
    for per, length in ((4, 127), (5, 159), (8, 255)):  # 97, 129 and 225 windows: the three shapes of the fused kernel
        assert int(ladder_oracle(per)["packed"][2].max()) == length


def check_ladder(ctx, form, want):
    buf, off, lens = want["packed"]
    if form == "codes":
        gpu = ctx.classify_batch(buf, off, lens)
        gc.assert_same_classification(gpu, want["res"], want["taxa"], off, lens, K)
    else:
        if form == "sparse":
            ctx.enable_sparse(UNIT)
        rle = ctx.classify_batch_rle(buf, off, lens)
        assert np.array_equal(rle["calls"], want["res"]["calls"])
    if form == "sparse":
        counts, flags, pairs, n_sparse, n_dense = assert_sparse_state_equals_oracle(ctx, want["run"])
        assert n_sparse == 2 and n_dense == 0  # taxon 4 and the misses: 53 encodings each, flagged ones among them
        for t in (0, 4):
            assert sum(int(e) & 1 for e in want["run"].counts()[t]["sketch"].sparse_list()) == 40  # ranks 14 .. 53
    else:
        counts = ctx.counts()
    gc.assert_same_counts(counts, want["run"])
    assert counts["registers"][slot_of(counts, 4)].max() == 53 and counts["registers"][0].max() == 53


@pytest.mark.parametrize("form", ["codes", "runs", "sparse"])
@pytest.mark.parametrize("per", [4, 5, 8])
def test_rank_ladder_fused(files, per, form):
    ctx, _ = context(files)
    check_ladder(ctx, form, ladder_oracle(per))


@pytest.mark.parametrize("form", ["codes", "runs", "sparse"])
def test_rank_ladder_generic_instances(files, form):
    """nt = 9: the instances without a compiled-in geometry"""
    ctx, _ = context(files, nt=9)
    check_ladder(ctx, form, ladder_oracle(5, nt=9))


@pytest.mark.parametrize("form", ["codes", "runs", "sparse"])
def test_rank_ladder_staged(files, form):
    """KU_LAYOUT=sorted: no probe table, so the lookup, resolve and accounting kernels of ku_kernels.hip"""
    ctx, _ = context(files, layout="sorted")
    check_ladder(ctx, form, ladder_oracle(4))


def test_rank_ladder_quick_mode(files):
    """reads of one k-mer each, -q with min_hits 1: the scanned prefix is the whole read, every k-mer is booked"""
    want = ladder_oracle(1, quick=True)
    buf, off, lens = want["packed"]
    assert (lens == K).all()
    ctx, _ = context(files)
    gpu = ctx.classify_batch(buf, off, lens, flags=capi.KU_F_QUICK, min_hits=1)
    gc.assert_same_classification(gpu, want["res"], want["taxa"], off, lens, K, quick=True)
    counts = ctx.counts()
    gc.assert_same_counts(counts, want["run"])
    assert counts["registers"][slot_of(counts, 4)].max() == 53 and counts["registers"][0].max() == 53


# --------------------------------------------------------------------------- b. floors at height
def oracle_more(run, seqs):
    """a further batch on a run: (res, buf, off, lens, taxa laid out like the C ABI's)"""
    res = run.classify(seqs)
    buf, off, lens = ko.pack_reads(seqs)
    taxa = np.zeros(max(len(buf), 1), dtype=np.uint32)
    for i in range(len(seqs)):
        a, n = int(res["taxa_off"][i]), int(res["n_slots"][i])
        t = res["taxa"][a:a + n].copy()
        t[res["ambig"][a:a + n] != 0] = capi.KU_AMBIG
        taxa[int(off[i]):int(off[i]) + n] = t
    return res, buf, off, lens, taxa


def batch_q(floor):
    """on a floor of `floor` under taxon 4 (1 .. F): reads of four k-mers, and two with a stretch of random sequence -- more
    than 32 misses, which slot 0's floor of 0 lets through: more than half a queue in one pass, so the direct way -- next to
    k-mers of taxon 4 at and far above the floor, one of them with a k-mer of taxon 5 as well (floors gathered per lane)"""
    w = world()
    rng = np.random.default_rng(16)
    km = [w["min_f"], w["min_f1"]]
    for i in OTHERS:
        km += [w["at_rank"][(i, floor)], w["at_rank"][(i, floor + 1)]]
    km += [v for _, v in w["top"]]
    reads = bk.reads_of(km, 4)
    for extra in ([], [w["taxon5_b"]]):
        stretch = bytes(synth.codes_to_ascii(rng.integers(0, 4, 70).astype(np.uint8)))  # 40 k-mers no database holds
        parts = [bk.ascii_of(w["at_rank"][(0, floor)]), stretch, bk.ascii_of(w["top"][0][1], True)]
        parts += [bk.ascii_of(v) for v in extra]
        reads.append(b"N".join(parts))
    return reads


def test_precondition_batch_p_fills_the_row_to_f_and_q_raises_the_minimum():
    w = world()
    odb, otax = oracle_db()
    run = ko.Run(odb, otax)
    run.classify(bk.reads_of(w["row"], 4))
    regs = run.counts()[4]["sketch"].registers()
    assert regs.min() == F and regs.max() == F + 5 and int(np.argmin(regs)) == MINREG and (regs == F).sum() == 1
    assert set(run.counts()) == {4}  # no misses: slot 0 stays empty
    for floor in (1, F):
        q = batch_q(floor)
        run2 = ko.Run(odb, otax)
        run2.classify(bk.reads_of(w["row"], 4))
        res = run2.classify(q)
        c = run2.counts()
        r2 = c[4]["sketch"].registers()
        assert r2[MINREG] == F + 1 and r2.min() == F + 1 and [r2[at] for at, _ in w["top"]] == [53, 53]
        changed = np.flatnonzero(r2 != regs).tolist()
        assert sorted(changed) == sorted([MINREG] + [at for at, _ in w["top"]])  # the k-mers at the floor change nothing
        assert c[0]["n_kmers"] == 80 and max(len(x) for x in q) <= 192 + K - 1
        a = int(res["taxa_off"][-2])
        assert {4, 5} <= set(res["taxa"][a:].tolist())  # the last read meets taxa 4 and 5


def test_floors_at_height(files, monkeypatch):
    w = world()
    odb, otax = oracle_db()
    p = ko.pack_reads(bk.reads_of(w["row"], 4))
    assert len(p[2]) == 1024
    monkeypatch.setenv("KU_SHORT_BLOCKS_PER_CU", "1")
    states, floor = {}, None
    for every in ("1", "0"):
        monkeypatch.setenv("KU_HLL_FLOOR_EVERY", every)
        ctx, _ = context(files)
        run = ko.Run(odb, otax)
        for _ in range(2):
            res = run.classify_packed(*p)
            gpu = ctx.classify_batch(*p)
            assert np.array_equal(gpu["calls"], res["calls"])
        counts = ctx.counts()
        gc.assert_same_counts(counts, run)
        s4 = slot_of(counts, 4)
        fl = ctx.hll_floors()
        assert counts["registers"][s4].min() == F
        if every == "1":
            assert 0 < fl[s4] <= F, fl[s4]  # the floor has risen, and not past the row's minimum
            assert fl[0] == 0 and not np.delete(fl, s4).any()
            floor = int(fl[s4])
        else:
            assert not fl.any()
        q = batch_q(floor)  # (the same batch both times: the floor read under KU_HLL_FLOOR_EVERY=1)
        res, buf, off, lens, taxa = oracle_more(run, q)
        gpu = ctx.classify_batch(buf, off, lens)
        gc.assert_same_classification(gpu, res, taxa, off, lens, K)
        counts = ctx.counts()
        gc.assert_same_counts(counts, run)
        regs = counts["registers"][s4]
        assert regs[MINREG] == F + 1 and regs.min() == F + 1 and all(regs[at] == 53 for at, _ in w["top"])
        fl2 = ctx.hll_floors()
        assert (fl2 <= counts["registers"].min(axis=1)).all() and fl2[s4] >= fl[s4] and fl2[0] == 0
        states[every] = counts
    for key in ("slot_taxid", "registers", "n_kmers", "node_taxid", "n_reads"):
        assert np.array_equal(states["1"][key], states["0"][key]), key


# --------------------------------------------------------------------------- c. encodings at the 1024 edge
def edge_order(name):
    w = world()
    e, last, twin = w["edge"][:1023], w["edge"][1023], w["twin"]
    return {"1023_pair_last": e + [last, twin], "pair_first_1023": [last, twin] + e, "1024": e + [last],
            "1024_twin": [last] + e + [twin], "1022_pair": e[:1022] + [last, twin]}[name]


EDGE = {"1023_pair_last": (False, None), "pair_first_1023": (True, 1024), "1024": (True, 1024), "1024_twin": (False, None),
        "1022_pair": (True, 1023)}  # order -> (sparse, entries) of taxon 5 in the reference


@pytest.mark.parametrize("order", list(EDGE))
def test_precondition_the_oracle_switches_by_encodings_and_order(order):
    odb, otax = oracle_db()
    run = ko.Run(odb, otax, work_unit_nt=UNIT)
    reads = bk.reads_of(edge_order(order), 4)
    assert sum(len(r) for r in reads) < UNIT  # one work unit
    run.classify(reads)
    c = run.counts()
    assert set(c) == {5} and c[5]["n_kmers"] == len(edge_order(order))
    sparse, entries = EDGE[order]
    assert c[5]["sparse"] == sparse and (len(c[5]["sketch"].sparse_list()) == entries if sparse else True)
    e = world()["edge"]
    assert len({bk.encoding(int(ko.lib().ko_hash(v))) for v in e}) == 1024
    assert bk.encoding(int(ko.lib().ko_hash(world()["twin"]))) == bk.encoding(int(ko.lib().ko_hash(e[1023])))


@pytest.mark.parametrize("split", ["whole", "last_alone"])
@pytest.mark.parametrize("path", ["fast", "staged", "mixed"])
@pytest.mark.parametrize("order", list(EDGE))
def test_switch_to_dense_by_encodings_and_order(files, order, path, split, monkeypatch):
    """(1024_twin: the twin of the first k-mer comes last.)  One work unit; `last_alone`: the last read (for 1025 k-mers: the
    1025th alone) in a batch of its own, the unit carried over; `mixed` alternates the fast path and the staged emulation
    between the batches (`whole` then cuts in the middle)"""
    reads = bk.reads_of(edge_order(order), 4)
    n = len(reads)
    cuts = [0, n - 1, n] if split == "last_alone" else ([0, n // 2, n] if path == "mixed" else [0, n])
    odb, otax = oracle_db()
    run = ko.Run(odb, otax, work_unit_nt=UNIT)
    res = run.classify(reads)
    sparse, entries = EDGE[order]
    assert run.counts()[5]["sparse"] == sparse
    ctx, _ = context(files)
    ctx.enable_sparse(UNIT)
    buf, off, lens = ko.pack_reads(reads)
    rle = classify_in_batches_by_path(ctx, buf, off, lens, cuts, path, monkeypatch)
    assert np.array_equal(np.concatenate([r["calls"] for r in rle]), res["calls"])
    counts, flags, pairs, n_sparse, n_dense = assert_sparse_state_equals_oracle(ctx, run)
    assert (n_sparse, n_dense) == ((1, 0) if sparse else (0, 1))
    if sparse:
        assert len(pairs) == entries
    gc.assert_same_counts(counts, run)


# --------------------------------------------------------------------------- d. flagged encodings and clade unions in the report
@pytest.fixture(params=["tables", "bitmaps"])
def union_form(request, monkeypatch):
    """clade unions of the sparse sketches in ku_ctx_report: per-clade hash tables, or (test hook: for every clade with
    several members) bitmaps over the 2^25 indices, which send flagged entries through per-clade tables of their own"""
    if request.param == "bitmaps":
        monkeypatch.setenv("KU_ROLLUP_BITMAP_MIN", "1")
    return request.param


def report_reads():
    w = world()
    s4, s5, s6 = w["s4"], w["s5"], w["s6"]
    mixed = [v for trio in zip_longest(s4, s5, s6) for v in trio if v is not None]  # reads of two and of three taxa
    return bk.reads_of(s4 + s5 + s6, 4) + bk.reads_of(mixed, 5) + bk.reads_of(s6 + s5 + s4, 8)


def kmers_column(text):
    """taxID -> the report's `kmers` column (the clade's distinct k-mer estimate)"""
    out = {}
    for line in text.strip("\n").split("\n")[1:]:
        f = line.split("\t")
        out[int(f[6])] = int(f[3])
    return out


# encodings per clade: species 4 = 8 flagged + 13 unflagged, 5 = 10 flagged, 6 = the 13 unflagged ones of 4; genus 2 = 4 and 5
# with the six shared ones counted once; the root adds nothing to genus 2
N_ENC = {4: 21, 5: 10, 6: 13, 3: 13, 2: 21 + 10 - 6, 1: 25}


def test_precondition_the_oracle_counts_shared_encodings_once(files):
    w = world()
    assert w["n_flagged"] == (8, 10) and (len(w["s4"]), len(w["s5"]), len(w["s6"])) == (21, 10, 13)
    odb, otax = oracle_db()
    run = ko.Run(odb, otax, work_unit_nt=UNIT)
    run.classify(report_reads())
    c = run.counts()
    enc = {t: set(c[t]["sketch"].sparse_list().tolist()) for t in (4, 5, 6)}
    assert all(c[t]["sparse"] for t in enc) and {t: len(e) for t, e in enc.items()} == {4: 21, 5: 10, 6: 13}
    flagged = {t: {e for e in enc[t] if e & 1} for t in enc}
    assert {t: len(f) for t, f in flagged.items()} == {4: 8, 5: 10, 6: 0}
    assert sorted((e >> 1) & 0x3f for e in flagged[4]) == [1, 2, 3, 13, 26, 27, 39, 40]
    assert sorted((e >> 1) & 0x3f for e in flagged[5]) == [1, 2, 3, 5, 13, 20, 26, 27, 39, 40]
    assert len(enc[4] & enc[5]) == 6 and enc[6] < enc[4] and not enc[6] & enc[5]
    assert len({e >> 20 for e in enc[6]}) == 1 and sorted(c[6]["sketch"].registers()[900:901].tolist()) == [13]
    assert {t for t in c if c[t]["n_kmers"]} == {4, 5, 6} and all(c[t]["n_kmers"] == 3 * len(w[f"s{t}"]) for t in (4, 5, 6))
    # far fewer encodings than inserts, so the estimate is the number of encodings: a union that counted a shared one twice shows
    assert kmers_column(run.report(files["taxdb"], files["counts"])) == N_ENC


def test_report_unions_of_flagged_and_shared_encodings(files, union_form):
    reads = report_reads()
    odb, otax = oracle_db()
    run = ko.Run(odb, otax, work_unit_nt=UNIT)
    res = run.classify(reads)
    ctx, ctax = context(files)
    ctx.enable_sparse(UNIT)
    rle = ctx.classify_batch_rle(*ko.pack_reads(reads))
    assert np.array_equal(rle["calls"], res["calls"])
    paths = [files["counts"]]
    got = ctx.report(ctax, paths)
    counts, flags, pairs, n_sparse, n_dense = assert_sparse_state_equals_oracle(ctx, run)
    gc.assert_same_counts(counts, run)
    assert (n_sparse, n_dense) == (3, 0)
    assert got == capi.report_sparse(ctax, counts, flags, pairs, paths)
    want = run.report(files["taxdb"], files["counts"])
    assert rows(got) == rows(want)
    assert kmers_column(got) == N_ENC


def test_report_dense_rollup_with_registers_up_to_53(files):
    """without the emulation: registers only, the clade roll-up their byte-wise maximum, the host estimator over ranks up to 53"""
    reads = report_reads()
    odb, otax = oracle_db()
    ko.set_hll_sparse(False)
    try:
        run = ko.Run(odb, otax)
        res = run.classify(reads)
        want = run.report(files["taxdb"], files["counts"])
        assert not any(c["sparse"] for c in run.counts().values())
    finally:
        ko.set_hll_sparse(True)
    ctx, ctax = context(files)
    rle = ctx.classify_batch_rle(*ko.pack_reads(reads))
    assert np.array_equal(rle["calls"], res["calls"])
    counts = ctx.counts()
    gc.assert_same_counts(counts, run)
    assert counts["registers"][slot_of(counts, 4)].max() == 53 and counts["registers"][slot_of(counts, 5)].max() == 53
    paths = [files["counts"]]
    got = ctx.report(ctax, paths)
    assert got == capi.report(ctax, counts, paths)
    assert rows(got) == rows(want)
    for t, c in run.counts().items():  # the estimator alone, per taxon
        assert capi.hll_cardinality(c["sketch"].registers(), c["n_kmers"]) == c["cardinality"], t
