"""db_merge (ku_db_merge_files, bin/db_merge): the union of sorted databases on the GPU, the values of shared k-mers folded
with lca().  Every expected file comes from the numpy model below: it reads the inputs with synth.read_db, unions the k-mers,
folds the values left to right with the oracle's lca over the same taxDB, orders with synth.sort_db and writes with
synth.write_db.  The model itself is certified against the reference (oracle/_ref): merging the databases that the reference's
db_sort + set_lcas build from two libraries apart gives the files they build from both libraries together."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from krakenuniq_amd import capi, synth
from oracle import ku_oracle as ko
from test_kmer_db import _ref, _same_file, model_kmers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krakenuniq_amd", "bin")
DB_MERGE = os.path.join(BIN, "db_merge")
K = 31
SMALL = 4 << 20  # device budget of the kmer_db runs that build the inputs (the default, half of the free HBM, takes seconds to allocate)
ABSENT, ABSENT_BIG = 777, 3000000007  # values that the small taxonomy does not hold (the second one above 2^31)


# --------------------------------------------------------------------------- the model
def _read(pair):
    kdb, idx = pair
    assert os.path.dirname(kdb) == os.path.dirname(idx)
    return synth.read_db(os.path.dirname(kdb), kdb=os.path.basename(kdb), idx=os.path.basename(idx))


def model_merge(pairs, otax=None):
    """left fold over the inputs: {"kmers", "vals", "duplicates", "folded", "kinds"}; kinds counts the value pairs (a, b), a from
    the fold so far and b from the input being merged, of the k-mers both hold.  Two different non-zero values without a
    taxonomy: ValueError"""
    acc, k, nt = {}, None, None
    duplicates = folded = 0
    kinds = {}
    for n, pair in enumerate(pairs):
        kmers, vals, _, k_i, nt_i, idx_type = _read(pair)
        assert idx_type == 2 and (k, nt) in ((None, None), (k_i, nt_i))
        k, nt = k_i, nt_i
        assert len(np.unique(kmers)) == len(kmers)
        for km, v in zip(kmers.tolist(), vals.tolist()):
            if n and km in acc:
                a = acc[km]
                duplicates += 1
                kinds[(a, v)] = kinds.get((a, v), 0) + 1
                if a != v and a and v:
                    folded += 1
                    if otax is None:
                        raise ValueError("values differ")
                    acc[km] = otax.lca(a, v)
                else:
                    acc[km] = a or v
            else:
                acc[km] = v
    kmers = np.fromiter(acc.keys(), dtype=np.uint64, count=len(acc))
    vals = np.fromiter(acc.values(), dtype=np.uint32, count=len(acc))
    return {"kmers": kmers, "vals": vals, "k": k, "nt": nt, "duplicates": duplicates, "folded": folded, "kinds": kinds}


def write_model(m, dirname):
    sk, sv, off = synth.sort_db(m["kmers"], m["vals"], m["k"], m["nt"])
    synth.write_db(str(dirname), sk, sv, off, m["k"], m["nt"])
    return os.path.join(str(dirname), "database.kdb"), os.path.join(str(dirname), "database.idx")


def _same(got, want):
    return _same_file(got[0], want[0]) and _same_file(got[1], want[1])


def _merge(pairs, out_dir, tag, tax=None, device_bytes=SMALL):
    out = (os.path.join(str(out_dir), f"{tag}.kdb"), os.path.join(str(out_dir), f"{tag}.idx"))
    st = capi.db_merge_files([p[0] for p in pairs], [p[1] for p in pairs], out[0], out[1], tax=tax, device_bytes=device_bytes)
    return out, st


def plan(pairs, device_bytes):
    """the chunk plan restated: from its first bin a chunk takes the longest range of bins whose records, all inputs together,
    number at most `capacity` and whose bins number at most `max_bins`.  Returns (bounds, records per chunk and input)"""
    cap, max_bins = capi.db_merge_capacity(device_bytes)
    offs = [_read(p)[2].astype(np.int64) for p in pairs]
    tot = sum(offs)
    nb = len(tot) - 1
    bounds, lo = [0], 0
    while lo < nb:
        hi = min(lo + max_bins, nb, int(np.searchsorted(tot, tot[lo] + cap, side="right")) - 1)
        assert hi > lo, "a bin that does not fit"
        bounds.append(hi)
        lo = hi
    per_input = [[int(o[b1] - o[b0]) for o in offs] for b0, b1 in zip(bounds[:-1], bounds[1:])]
    return bounds, per_input


# --------------------------------------------------------------------------- libraries
def _genome(seed, length):
    return synth.codes_to_ascii(synth.procedural_genome(seed, 3, length))


def _libraries():
    """records (sequence, taxid) over synth.small_taxonomy(): root 1 -> genus 2 -> species 4, 5; genus 3 -> species 6 -> 1000000001.
    B carries pieces of A under other taxa, so that the k-mers both hold meet as siblings (4, 5), as a genus and its own
    species (2, 4), as equal taxa (5, 5) and as the sequence-level taxid and its species (1000000001, 6)"""
    g = {name: _genome(seed, 3000) for name, seed in (("a", 41), ("c", 42), ("e", 43), ("p", 44), ("b", 45), ("d", 46))}
    lib_a = [(g["a"], 4), (g["c"], 2), (g["e"], 5), (g["p"], 1000000001)]
    lib_b = [(g["b"] + g["a"][500:2500], 5), (g["c"][:1000], 4), (g["e"][1000:2000], 5), (g["p"][:1000], 6), (g["d"], 6)]
    lib_c = [(_genome(47, 3000) + g["a"][:800], 6), (g["b"][:900], 4), (g["d"][2000:], 1000000001)]
    return lib_a, lib_b, lib_c


def _write_library(d, name, lib):
    fa, mp = os.path.join(str(d), f"{name}.fa"), os.path.join(str(d), f"{name}.map")
    ids = [f"{name}{i}" for i in range(len(lib))]
    synth.write_fasta(fa, [s for s, _ in lib], ids=ids, width=60)
    with open(mp, "w") as f:
        f.write("".join(f"{i}\t{t}\n" for i, (_, t) in zip(ids, lib)))
    return fa, mp


def _patch_values(src, dst, vals):
    img = np.fromfile(src, dtype=np.uint8)
    hdr = 72 + 2 * (4 + 8 * int.from_bytes(img[8:16].tobytes(), "little"))
    pairs = img[hdr:hdr + 12 * len(vals)].view(synth.PAIR_DT)
    pairs["val"] = vals
    img.tofile(dst)


def _set_lcas(pair, lib, ctax, out_kdb):
    """the project's set_lcas over a database: the values folded, written next to the index"""
    sl = capi.SetLcas(capi.Db(*pair), ctax)
    for s, t in lib:
        sl.add(s, t)
    vals, missing = sl.finish()
    sl.close()
    assert missing == 0
    _patch_values(pair[0], out_kdb, vals)
    return out_kdb, pair[1]


# --------------------------------------------------------------------------- CPU: the command line
def _cli(args):
    return subprocess.run([DB_MERGE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)


def test_cli_usage_without_gpu(tmp_path):
    assert os.path.exists(DB_MERGE), "build with make -C krakenuniq_amd/csrc"
    r = _cli([])
    assert r.returncode == 64 and b"Usage: db_merge" in r.stderr
    r = _cli(["-h"])
    assert r.returncode == 0 and b"Usage: db_merge" in r.stderr
    out = ["-o", str(tmp_path / "out.kdb"), "-i", str(tmp_path / "out.idx")]
    assert _cli(out + ["a.kdb", "a.idx", "b.kdb"]).returncode == 64      # an odd count
    assert _cli(out + ["a.kdb", "a.idx"]).returncode == 64               # one pair
    assert _cli(["a.kdb", "a.idx", "b.kdb", "b.idx"]).returncode == 64   # no outputs
    assert _cli(out + ["-s", "lots", "a.kdb", "a.idx", "b.kdb", "b.idx"]).returncode == 64
    assert not os.path.exists(tmp_path / "out.kdb") and not os.path.exists(tmp_path / "out.idx")


def test_cli_missing_input_leaves_an_existing_database_alone(tmp_path):
    (tmp_path / "out.kdb").write_bytes(b"a database that took days")
    d = os.path.join(ROOT, "tests", "golden", "f1")
    r = _cli(["-o", str(tmp_path / "out.kdb"), "-i", str(tmp_path / "out.idx"), f"{d}/database.kdb", f"{d}/database.idx",
              str(tmp_path / "missing.kdb"), f"{d}/database.idx"])
    assert r.returncode == 66 and b"can't open" in r.stderr
    assert (tmp_path / "out.kdb").read_bytes() == b"a database that took days" and not os.path.exists(tmp_path / "out.idx")


# --------------------------------------------------------------------------- CPU: what the ABI checks before it looks for a device
def _hand_db(d, kmers, vals, nt, k=K):
    sk, sv, off = synth.sort_db(np.asarray(kmers, dtype=np.uint64), np.asarray(vals, dtype=np.uint32), k, nt)
    synth.write_db(str(d), sk, sv, off, k, nt)
    return os.path.join(str(d), "database.kdb"), os.path.join(str(d), "database.idx")


def test_abi_checks_without_a_device(tmp_path):
    rng = np.random.default_rng(1)
    a7 = _hand_db(tmp_path / "a7", rng.integers(0, 1 << 62, 50, dtype=np.uint64), np.zeros(50), 7)
    b7 = _hand_db(tmp_path / "b7", rng.integers(0, 1 << 62, 50, dtype=np.uint64), np.zeros(50), 7)
    b6 = _hand_db(tmp_path / "b6", rng.integers(0, 1 << 62, 50, dtype=np.uint64), np.zeros(50), 6)
    out = (str(tmp_path / "out.kdb"), str(tmp_path / "out.idx"))

    def refused(pairs, out=out, **kw):
        with pytest.raises(capi.KuError) as e:
            capi.db_merge_files([p[0] for p in pairs], [p[1] for p in pairs], *out, **kw)
        return e.value

    e = refused([a7, b6])  # minimizer lengths 7 and 6
    assert e.status == -1 and a7[0] in str(e) and b6[0] in str(e) and "db_sort -n" in str(e)
    assert refused([a7]).status == -1 and refused([a7] * 9).status == -1
    assert refused([a7, b7], device_bytes=capi.KU_DBMERGE_MIN_BYTES - 1).status == -1
    assert refused([a7, (str(tmp_path / "nope.kdb"), b7[1])]).status == -3
    os.symlink(b7[0], tmp_path / "link.kdb")  # the output is an input, under another name
    e = refused([a7, b7], out=(str(tmp_path / "link.kdb"), out[1]))
    assert e.status == -1 and "is the input" in str(e)
    e = refused([a7, b7], out=(out[0], a7[1]))
    assert e.status == -1
    assert not os.path.exists(out[0]) and not os.path.exists(out[1])
    assert os.path.getsize(b7[0]) == len(synth.kdb_header(K, 50)) + 50 * 12  # (untouched through the link)


def test_no_merge_without_a_device(tmp_path):
    if capi.lib().ku_device_count() > 0:
        pytest.skip("GPU present")
    rng = np.random.default_rng(2)
    a = _hand_db(tmp_path / "a", rng.integers(0, 1 << 62, 50, dtype=np.uint64), np.zeros(50), 7)
    b = _hand_db(tmp_path / "b", rng.integers(0, 1 << 62, 50, dtype=np.uint64), np.zeros(50), 7)
    (tmp_path / "out.idx").write_bytes(b"an index")
    with pytest.raises(capi.KuError) as e:
        capi.db_merge_files([a[0], b[0]], [a[1], b[1]], str(tmp_path / "out.kdb"), str(tmp_path / "out.idx"))
    assert e.value.status == -5  # KU_EHIP
    assert not os.path.exists(tmp_path / "out.kdb") and (tmp_path / "out.idx").read_bytes() == b"an index"


def test_budget_rule_of_the_binding():
    """db_merge_capacity restates include/krakenuniq_amd.h: an eighth of the budget for the bins at 24 bytes each (one closing
    entry per slice), the rest for the records at 56 bytes each"""
    assert capi.KU_DBMERGE_MIN_BYTES == 65536
    assert capi.db_merge_capacity(65536) == (1024, 340)
    assert capi.db_merge_capacity(3 << 20) == (49152, 16383)
    assert capi.db_merge_capacity(64 << 30) == ((56 << 30) // 56, (8 << 30) // 24 - 1)


# --------------------------------------------------------------------------- CPU: the model is the reference's
def test_the_model_is_the_reference(tmp_path):
    """the reference's db_sort + set_lcas over library A, over B and over both; the model's merge of the first two databases
    is the third, .kdb and .idx byte for byte"""
    lib_a, lib_b, _ = _libraries()
    tax = synth.small_taxonomy()
    tax.write(str(tmp_path / "taxDB"))
    built = {}
    for name, lib in (("a", lib_a), ("b", lib_b), ("ab", lib_a + lib_b)):
        fa, mp = _write_library(tmp_path, name, lib)
        kmers = model_kmers([s for s, _ in lib], K)
        perm = np.random.default_rng(3).permutation(len(kmers))
        synth.write_jdb(str(tmp_path / f"{name}.jdb"), kmers[perm], np.zeros(len(kmers), dtype=np.uint32), K)
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([_ref("db_sort"), "-t", "1", "-n", "7", "-d", str(tmp_path / f"{name}.jdb"), "-o", str(d / "zero.kdb"),
                            "-i", str(d / "database.idx")], stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()
        r = subprocess.run([_ref("set_lcas"), "-t", "1", "-d", str(d / "zero.kdb"), "-o", str(d / "database.kdb"), "-i", str(d / "database.idx"),
                            "-b", str(tmp_path / "taxDB"), "-m", mp, "-F", fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()
        built[name] = (str(d / "database.kdb"), str(d / "database.idx"))
    m = model_merge([built["a"], built["b"]], ko.Tax(str(tmp_path / "taxDB")))
    assert m["folded"] > 1000 and m["duplicates"] > m["folded"]
    assert _same(write_model(m, tmp_path / "model"), built["ab"])
    # ... and in the other order: the fold is commutative
    m = model_merge([built["b"], built["a"]], ko.Tax(str(tmp_path / "taxDB")))
    assert _same(write_model(m, tmp_path / "model_ba"), built["ab"])


# --------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """libraries A, B, C; for each its zero-valued database (kmer_db) and the same after set_lcas, nt = 7; A U B likewise"""
    d = tmp_path_factory.mktemp("db_merge")
    tax = synth.small_taxonomy()
    tax.write(str(d / "taxDB"))
    ctax, otax = capi.Tax(str(d / "taxDB")), ko.Tax(str(d / "taxDB"))
    libs = dict(zip("abc", _libraries()))
    libs["ab"] = libs["a"] + libs["b"]
    zero, lca = {}, {}
    for name, lib in libs.items():
        zero[name] = (str(d / f"{name}0.kdb"), str(d / f"{name}.idx"))
        capi.kmer_db_files([s for s, _ in lib], *zero[name], K, 7, device_bytes=SMALL)
        lca[name] = _set_lcas(zero[name], lib, ctax, str(d / f"{name}.kdb"))
    return {"dir": d, "libs": libs, "zero": zero, "lca": lca, "ctax": ctax, "otax": otax, "tax": tax}


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [7, 3, 10])
def test_zero_valued_union(tmp_path, nt):
    """db_merge(kmer_db(A), kmer_db(B)) == kmer_db(A U B); nt = 3: 64 big bins, nt = 10: a million bins, most of them empty"""
    a = [_genome(51, 4000), _genome(52, 4000)]
    b = [_genome(53, 4000) + a[0][1000:3000]]
    pairs = {}
    for name, recs in (("a", a), ("b", b), ("ab", a + b)):
        pairs[name] = (str(tmp_path / f"{name}.kdb"), str(tmp_path / f"{name}.idx"))
        capi.kmer_db_files(recs, *pairs[name], K, nt, device_bytes=SMALL)
    m = model_merge([pairs["a"], pairs["b"]])
    ka, kb = _read(pairs["a"])[0], _read(pairs["b"])[0]
    assert m["duplicates"] >= 1000 and len(ka) - m["duplicates"] >= 1000 and len(kb) - m["duplicates"] >= 1000
    got, st = _merge([pairs["a"], pairs["b"]], tmp_path, "got")
    assert _same(got, pairs["ab"])
    assert _same(got, write_model(m, tmp_path / "model"))
    n_chunks = len(plan([pairs["a"], pairs["b"]], SMALL)[0]) - 1  # (4 MiB: 21844 bins to a chunk)
    assert n_chunks == {7: 1, 3: 1, 10: 49}[nt]
    assert (st.key_ct, st.duplicates, st.folded, st.chunks) == (len(m["kmers"]), m["duplicates"], 0, n_chunks)
    assert st.capacity == capi.db_merge_capacity(SMALL)[0]


@pytest.mark.gpu
def test_lca_fold(case, tmp_path):
    """databases that went through set_lcas apart: siblings, a genus and its species, equal taxa, the sequence-level taxid"""
    pairs = [case["lca"]["a"], case["lca"]["b"]]
    m = model_merge(pairs, case["otax"])
    for kind in ((4, 5), (2, 4), (5, 5), (1000000001, 6)):
        assert m["kinds"].get(kind, 0) >= 100, kind
    got, st = _merge(pairs, tmp_path, "got", tax=case["ctax"])
    assert _same(got, write_model(m, tmp_path / "model"))
    assert _same(got, case["lca"]["ab"])  # == set_lcas(kmer_db(A U B), A U B)
    assert (st.key_ct, st.duplicates, st.folded) == (len(m["kmers"]), m["duplicates"], m["folded"]) and st.folded > 1000
    vals = _read(got)[1]
    assert {2, 4, 5, 6, 1000000001} <= set(vals.tolist())


@pytest.mark.gpu
def test_lca_fold_with_zeros_and_values_the_taxonomy_lacks(case, tmp_path):
    """one input zero-valued (a taxon and 0); values patched into the inputs that the taxDB does not hold, one above 2^31: they
    are nodes without a parent, so they stay where they meet themselves or 0 and fold to the root with anything else"""
    pairs = [case["lca"]["a"], case["zero"]["b"]]
    m = model_merge(pairs, case["otax"])
    assert m["kinds"].get((4, 0), 0) >= 100 and m["folded"] == 0
    for tax in (case["ctax"], None):  # nothing to fold: the taxonomy is not needed
        got, st = _merge(pairs, tmp_path, "zeros", tax=tax)
        assert _same(got, write_model(m, tmp_path / "model_zeros")) and st.folded == 0 and st.duplicates == m["duplicates"]
    # patched values
    ka, va = _read(case["lca"]["a"])[:2]
    kb, vb = _read(case["lca"]["b"])[:2]
    shared_b = np.flatnonzero(np.isin(kb, ka))
    shared_a = np.flatnonzero(np.isin(ka, kb))
    vb[shared_b[::5]] = ABSENT
    vb[shared_b[1::5]] = ABSENT_BIG
    vb[::9] = ABSENT_BIG                     # (also on k-mers that A lacks)
    va[shared_a[::4]] = ABSENT_BIG           # some of them meet ABSENT, some ABSENT_BIG, some a taxon
    pa, pb = (str(tmp_path / "pa.kdb"), str(tmp_path / "pa.idx")), (str(tmp_path / "pb.kdb"), str(tmp_path / "pb.idx"))
    shutil.copy(case["lca"]["a"][1], pa[1])
    shutil.copy(case["lca"]["b"][1], pb[1])
    _patch_values(case["lca"]["a"][0], pa[0], va)
    _patch_values(case["lca"]["b"][0], pb[0], vb)
    m = model_merge([pa, pb], case["otax"])
    kinds = m["kinds"]
    assert kinds.get((ABSENT_BIG, ABSENT_BIG), 0) and kinds.get((ABSENT_BIG, ABSENT), 0)
    assert any(a == ABSENT_BIG and b in (4, 5, 6) for a, b in kinds) and any(b == ABSENT and a in (2, 4, 5, 1000000001) for a, b in kinds)
    got, st = _merge([pa, pb], tmp_path, "patched", tax=case["ctax"])
    assert _same(got, write_model(m, tmp_path / "model_patched"))
    assert st.folded == m["folded"]
    vals = _read(got)[1]
    assert (vals == ABSENT_BIG).sum() > 100 and (vals == 1).sum() > 100


@pytest.mark.gpu
def test_incremental_recipe_through_the_programs(case, tmp_path):
    """kmer_db over the new library, db_merge without a taxonomy, set_lcas over the new library alone: the files of the full
    rebuild (kmer_db and set_lcas over both libraries)"""
    d = case["dir"]
    fa, mp = {}, {}
    for name in ("a", "b", "ab"):
        fa[name], mp[name] = _write_library(tmp_path, name, case["libs"][name])

    def run(tool, args):
        r = subprocess.run([os.path.join(BIN, tool)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, (tool, r.stderr.decode())
        return r

    def build(name):
        run("kmer_db", ["-n", "7", "-s", str(SMALL), "-o", str(tmp_path / f"{name}0.kdb"), "-i", str(tmp_path / f"{name}.idx"), fa[name]])

    def set_lcas(kdb, idx, out, name):
        run("set_lcas", ["-d", kdb, "-o", out, "-i", idx, "-b", str(d / "taxDB"), "-m", mp[name], "-F", fa[name]])

    for name in ("a", "b", "ab"):
        build(name)
    set_lcas(str(tmp_path / "ab0.kdb"), str(tmp_path / "ab.idx"), str(tmp_path / "ab.kdb"), "ab")  # the full rebuild
    set_lcas(str(tmp_path / "a0.kdb"), str(tmp_path / "a.idx"), str(tmp_path / "a.kdb"), "a")      # the database that exists
    r = run("db_merge", ["-v", "-s", "4M", "-o", str(tmp_path / "m0.kdb"), "-i", str(tmp_path / "m.idx"), str(tmp_path / "a.kdb"),
                         str(tmp_path / "a.idx"), str(tmp_path / "b0.kdb"), str(tmp_path / "b.idx")])
    assert b"records written" in r.stderr and b" 0 folded" in r.stderr
    set_lcas(str(tmp_path / "m0.kdb"), str(tmp_path / "m.idx"), str(tmp_path / "m.kdb"), "b")
    assert _same((str(tmp_path / "m.kdb"), str(tmp_path / "m.idx")), (str(tmp_path / "ab.kdb"), str(tmp_path / "ab.idx")))
    assert _same((str(tmp_path / "m.kdb"), str(tmp_path / "m.idx")), case["lca"]["ab"])
    # with -b the program folds two finished databases
    set_lcas(str(tmp_path / "b0.kdb"), str(tmp_path / "b.idx"), str(tmp_path / "b.kdb"), "b")
    run("db_merge", ["-b", str(d / "taxDB"), "-o", str(tmp_path / "f.kdb"), "-i", str(tmp_path / "f.idx"), str(tmp_path / "a.kdb"),
                     str(tmp_path / "a.idx"), str(tmp_path / "b.kdb"), str(tmp_path / "b.idx")])
    assert _same((str(tmp_path / "f.kdb"), str(tmp_path / "f.idx")), case["lca"]["ab"])


@pytest.mark.gpu
def test_chunk_boundaries(case, tmp_path):
    """the minimum budget and one that gives exactly two chunks: the files of the one-chunk run, the chunk count of the plan"""
    pairs = [case["lca"]["a"], case["lca"]["b"]]
    want, st = _merge(pairs, tmp_path, "one", tax=case["ctax"])
    assert st.chunks == 1 and _same(want, case["lca"]["ab"])
    budgets = [capi.KU_DBMERGE_MIN_BYTES]
    two = next(b for b in range(1 << 20, 16 << 20, 64 << 10) if len(plan(pairs, b)[0]) == 3)
    budgets.append(two)
    for n, budget in enumerate(budgets):
        bounds, per_input = plan(pairs, budget)
        if n == 0:
            assert len(bounds) - 1 >= 3 and any(0 in recs for recs in per_input)  # a chunk in which one input has no record
            assert max(sum(recs) for recs in per_input) > capi.db_merge_capacity(budget)[0] // 2  # cut by the records too
        got, st = _merge(pairs, tmp_path, f"b{n}", tax=case["ctax"], device_bytes=budget)
        assert st.chunks == len(bounds) - 1 and st.capacity == capi.db_merge_capacity(budget)[0]
        assert _same(got, want)
        assert st.key_ct == (os.path.getsize(want[0]) - len(synth.kdb_header(K, 0))) // 12
    # three inputs under the minimum budget: the intermediate result crosses every chunk
    trio = [case["lca"][n] for n in "abc"]
    m = model_merge(trio, case["otax"])
    got, st = _merge(trio, tmp_path, "trio", tax=case["ctax"], device_bytes=capi.KU_DBMERGE_MIN_BYTES)
    assert st.chunks == len(plan(trio, capi.KU_DBMERGE_MIN_BYTES)[0]) - 1 and _same(got, write_model(m, tmp_path / "model_trio"))


def _edge_cases():
    """hand-made inputs, nt = 3: name -> list of (kmers, vals)"""
    rng = np.random.default_rng(7)
    pick = np.array([0, 2, 4, 5, 6, 1000000001], dtype=np.uint32)
    s = np.unique(rng.integers(0, 1 << 62, 400, dtype=np.uint64))
    sk, _, off = synth.sort_db(s, np.zeros(len(s), dtype=np.uint32), K, 3)
    off = off.astype(np.int64)
    vals = lambda n: rng.choice(pick, n)
    lower = np.concatenate([sk[off[b]:off[b] + (off[b + 1] - off[b]) // 2] for b in range(64)])
    upper = np.setdiff1d(sk, lower)
    ends = np.unique(np.concatenate([sk[[off[b], off[b + 1] - 1]] for b in range(64) if off[b + 1] > off[b]]))
    assert sk[-1] in ends  # the last record of the file
    extra = rng.integers(0, 1 << 62, 60, dtype=np.uint64)
    filled = np.flatnonzero(np.diff(off))  # (the bin key is a minimum over 29 scrambled 3-mers: a few bins hold nearly everything)
    assert len(filled) >= 6
    in_bins = lambda which: np.concatenate([sk[off[b]:off[b + 1]] for b in which])
    even, odd = in_bins(filled[0::2]), in_bins(filled[1::2])
    assert len(even) > 50 and len(odd) > 50
    none = np.zeros(0, dtype=np.uint64)
    return {
        "equal": [(sk, vals(len(sk))), (sk, vals(len(sk)))],
        "b_below_a": [(upper, vals(len(upper))), (lower, vals(len(lower)))],
        "a_below_b": [(lower, vals(len(lower))), (upper, vals(len(upper)))],
        "bin_ends": [(sk, vals(len(sk))), (np.concatenate([ends, extra]), vals(len(ends) + 60))],
        "bin_ends_left": [(np.concatenate([ends, extra]), vals(len(ends) + 60)), (sk, vals(len(sk)))],
        "one_sided_bins": [(even, vals(len(even))), (np.concatenate([odd, even[:20]]), vals(len(odd) + 20))],
        "one_record": [(sk, vals(len(sk))), (sk[200:201], vals(1))],
        "one_record_left": [(extra[:1], vals(1)), (sk, vals(len(sk)))],
        "empty": [(sk, vals(len(sk))), (none, vals(0))],
        "empty_left": [(none, vals(0)), (sk, vals(len(sk)))],
        "both_empty": [(none, vals(0)), (none, vals(0))],
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["equal", "b_below_a", "a_below_b", "bin_ends", "bin_ends_left", "one_sided_bins", "one_record",
                                  "one_record_left", "empty", "empty_left", "both_empty"])
def test_edges_of_the_rank_arithmetic(case, tmp_path, name):
    sides = _edge_cases()[name]
    pairs = [_hand_db(tmp_path / f"in{i}", km, v, 3) for i, (km, v) in enumerate(sides)]
    m = model_merge(pairs, case["otax"])
    if name == "equal":
        assert m["duplicates"] == len(sides[0][0]) == len(m["kmers"])
    if name in ("b_below_a", "a_below_b"):
        assert m["duplicates"] == 0
    if name.startswith("empty"):
        assert _same(write_model(m, tmp_path / "model"), pairs[0 if name == "empty" else 1])
    got, st = _merge(pairs, tmp_path, "got", tax=case["ctax"])
    assert _same(got, write_model(m, tmp_path / "model"))
    assert (st.key_ct, st.duplicates, st.folded, st.chunks) == (len(m["kmers"]), m["duplicates"], m["folded"], 1)


@pytest.mark.gpu
def test_three_inputs(case, tmp_path):
    trio = [case["lca"][n] for n in "abc"]
    m = model_merge(trio, case["otax"])
    assert m["kinds"].get((2, 6), 0) >= 100  # C's taxon 6 meets the fold of A's 4 and B's 5: their genus
    got, st = _merge(trio, tmp_path, "abc", tax=case["ctax"])
    assert _same(got, write_model(m, tmp_path / "model"))
    assert (st.key_ct, st.duplicates, st.folded) == (len(m["kmers"]), m["duplicates"], m["folded"])
    ab, _ = _merge(trio[:2], tmp_path, "ab", tax=case["ctax"])
    ab_c, _ = _merge([ab, trio[2]], tmp_path, "ab_c", tax=case["ctax"])
    assert _same(got, ab_c)


@pytest.mark.gpu
def test_another_key_length(tmp_path):
    """k = 20: records of 5 + 4 bytes, read and written byte by byte"""
    a, b = [_genome(61, 3000)], [_genome(62, 3000) + _genome(61, 3000)[500:1500]]
    pairs = {}
    for name, recs in (("a", a), ("b", b), ("ab", a + b)):
        pairs[name] = (str(tmp_path / f"{name}.kdb"), str(tmp_path / f"{name}.idx"))
        capi.kmer_db_files(recs, *pairs[name], 20, 5, device_bytes=SMALL)
    got, st = _merge([pairs["a"], pairs["b"]], tmp_path, "got")
    assert _same(got, pairs["ab"]) and st.duplicates > 900
    assert capi.Db(*got).info.key_len == 5


@pytest.mark.gpu
def test_differing_values_are_refused_without_a_taxonomy(case, tmp_path):
    out = (str(tmp_path / "out.kdb"), str(tmp_path / "out.idx"))
    for budget in (SMALL, capi.KU_DBMERGE_MIN_BYTES):
        with pytest.raises(capi.KuError) as e:
            capi.db_merge_files([case["lca"]["a"][0], case["lca"]["b"][0]], [case["lca"]["a"][1], case["lca"]["b"][1]], *out,
                                device_bytes=budget)
        assert e.value.status == -2
        assert "values differ for a k-mer present in both inputs; a taxonomy is needed to fold them" in str(e.value)
        assert not os.path.exists(out[0]) and not os.path.exists(out[1])
    r = subprocess.run([DB_MERGE, "-o", out[0], "-i", out[1], *case["lca"]["a"], *case["lca"]["b"]], stderr=subprocess.PIPE)
    assert r.returncode == 65 and b"a taxonomy is needed" in r.stderr and not os.path.exists(out[0]) and not os.path.exists(out[1])


@pytest.mark.gpu
def test_device_index_out_of_range(case, tmp_path):
    out = (str(tmp_path / "out.kdb"), str(tmp_path / "out.idx"))
    for device in (-1, capi.lib().ku_device_count()):
        with pytest.raises(capi.KuError) as e:
            capi.db_merge_files([case["zero"]["a"][0], case["zero"]["b"][0]], [case["zero"]["a"][1], case["zero"]["b"][1]], *out,
                                device=device)
        assert e.value.status == -1 and "device index out of range" in str(e.value)
        assert os.listdir(tmp_path) == []
