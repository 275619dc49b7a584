"""kmer_db (ku_kmerdb_*, bin/kmer_db): library FASTA -> sorted database.kdb + database.idx on the GPU, in place of the
reference's Jellyfish 1 + db_sort -z (scripts/build_db.sh:140-146,201).  With zeroed values both files depend only on
the SET of the library's canonical k-mers, so the expected files are the reference's own db_sort -z (oracle/_ref) over a
shuffled Jellyfish-style list of the numpy model's distinct set; the reference's set_lcas without -x certifies that the set
is exactly the library's (no k-mer missing: exit 0; none too many: no value stays 0)."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from krakenuniq_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "krakenuniq_amd", "bin")
KMER_DB = os.path.join(BIN, "kmer_db")
REF = os.path.join(ROOT, "oracle", "_ref")
K = 31
SMALL = 4 << 20  # device budget of most runs here (258048 k-mers): half of the free HBM, the default, takes seconds to allocate


# --------------------------------------------------------------------------- CPU: the command line
def _cli(args, **kw):
    # (no device may be touched: a run that opened one would fail here on the GPU-less machine with EX_SOFTWARE, not 64)
    return subprocess.run([KMER_DB] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL, **kw)


def test_cli_usage_without_gpu():
    assert os.path.exists(KMER_DB), "build with make -C krakenuniq_amd/csrc"
    r = _cli([])
    assert r.returncode == 64 and b"Usage: kmer_db" in r.stderr
    r = _cli(["-h"])
    assert r.returncode == 0 and b"Usage: kmer_db" in r.stderr
    assert _cli(["-o", "a.kdb", "-i", "a.idx", "lib.fa"]).returncode == 64  # -n is mandatory


def test_cli_refuses_stdin_with_passes(tmp_path):
    out = ["-o", str(tmp_path / "a.kdb"), "-i", str(tmp_path / "a.idx")]
    for inputs in ([], ["-"]):
        r = _cli(["-n", "7", "-P", "2"] + out + inputs)
        assert r.returncode == 64 and b"once per pass" in r.stderr
    assert not os.path.exists(tmp_path / "a.kdb") and not os.path.exists(tmp_path / "a.idx")


def test_cli_argument_ranges(tmp_path):
    out = ["-o", str(tmp_path / "a.kdb"), "-i", str(tmp_path / "a.idx"), "lib.fa"]
    assert _cli(["-n", "16"] + out).returncode == 64
    assert _cli(["-n", "0"] + out).returncode == 64
    assert _cli(["-n", "7", "-k", "32"] + out).returncode == 64
    assert _cli(["-n", "7", "-k", "6"] + out).returncode == 64
    assert _cli(["-n", "2", "-P", "17"] + out).returncode == 64  # more passes than bins
    assert _cli(["-n", "7", "-s", "lots"] + out).returncode == 64
    assert _cli(["-n", "7", "-t", "0"] + out).returncode == 64
    assert not os.path.exists(tmp_path / "a.kdb") and not os.path.exists(tmp_path / "a.idx")


def test_cli_missing_input_leaves_an_existing_database_alone(tmp_path):
    """the outputs are created when the device handle opens; an input that is not there is found before that"""
    (tmp_path / "a.kdb").write_bytes(b"a database that took days")
    r = _cli(["-n", "7", "-o", str(tmp_path / "a.kdb"), "-i", str(tmp_path / "a.idx"), str(tmp_path / "missing.fa")])
    assert r.returncode == 66 and b"can't open" in r.stderr
    assert (tmp_path / "a.kdb").read_bytes() == b"a database that took days" and not os.path.exists(tmp_path / "a.idx")


def test_budget_rule_of_the_binding():
    """kmer_db_capacity restates the rule in include/krakenuniq_amd.h: segment = min(64 MiB, bytes / 64) rounded down to
    1 KiB, capacity = (bytes - segment) / 16"""
    assert capi.kmer_db_capacity(65536) == (4032, 1024)
    assert capi.kmer_db_capacity(128 << 10) == (8064, 2048)
    assert capi.kmer_db_capacity(3 << 20) == (193536, 49152)
    assert capi.kmer_db_capacity(64 << 30) == (((64 << 30) - (64 << 20)) // 16, 64 << 20)


# --------------------------------------------------------------------------- the model and the trial library
_VALID = np.zeros(256, dtype=bool)
_VALID[list(b"ACGTacgt")] = True


def model_kmers(seqs, k):
    """distinct canonical k-mers of the windows made of ACGTacgt only, never across two records (src/krakenutil.cpp:252-263)"""
    parts = [np.zeros(0, dtype=np.uint64)]
    for s in seqs:
        a = np.frombuffer(s, dtype=np.uint8)
        bad = np.flatnonzero(~_VALID[a])
        lo = 0
        for hi in list(bad) + [len(a)]:
            if hi - lo >= k:
                codes = synth.ascii_to_codes(bytes(s[lo:hi]).upper())
                parts.append(synth.canonical(synth.kmers_forward(codes, k), k))
            lo = hi + 1
    return np.unique(np.concatenate(parts))


def valid_windows(seqs, k):
    """windows of k bytes that hold none but ACGTacgt"""
    n = 0
    for s in seqs:
        bad = np.r_[0, np.cumsum(~_VALID[np.frombuffer(s, dtype=np.uint8)])]
        if len(s) >= k:
            n += int((bad[k:] == bad[:-k]).sum())
    return n


def passes_that_fit(kmers, k, nt, capacity):
    """the smallest power-of-two pass count at which the distinct set of every pass leaves 1/64 of the buffer free.  (The bin
    key is a minimum over k - nt + 1 scrambled m-mers, so the low ranges are by far the fullest.)"""
    bk = synth.bin_key(kmers, k, nt).astype(np.int64)
    p = 1
    while p <= 4 ** nt:
        per_pass = np.bincount(np.searchsorted([(i * 4 ** nt) // p for i in range(1, p)], bk, side="right"), minlength=p)
        if per_pass.max() <= capacity - capacity // 64:
            return p
        p *= 2
    raise AssertionError("no pass count fits")


def _trial_records():
    a = synth.codes_to_ascii
    g0, g1, g2 = (synth.procedural_genome(s, 3, 6000) for s in (11, 12, 13))
    rc = bytearray(a(synth.revcomp_codes(g2[2000:4000])))
    rc[700], rc[730] = ord("N"), ord("R")  # a run of 29 valid bases between two ambiguous letters: no window fits
    t0 = a(g0)
    recs = [t0,                                             # a genome
            a(g1) + a(g0[1000:3000]),                       # ... one carrying 2 kb of another
            a(g2) + b"NNNN" + bytes(rc),                    # ... one followed by the reverse complement of 2 kb of itself
            t0[:3000].lower() + t0[3000:],                  # ... the first genome again, its first half in lower case
            a(g1[:30]), a(g2[100:131]), b"N" * 40]          # no window, exactly one, none
    return recs


@pytest.fixture(scope="module")
def trial(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmer_db_trial")
    recs = _trial_records()
    assert len(recs) == 7 and sum(max(len(r) - K + 1, 0) for r in recs) == 27895
    fa = str(d / "library.fa")
    synth.write_fasta(fa, recs, ids=[f"seq{i}" for i in range(len(recs))], width=60)
    kmers = model_kmers(recs, K)
    assert len(kmers) == 17940  # three genomes' worth: the copies, the lower case and the strand add next to nothing
    jdb = str(d / "model.jdb")
    perm = np.random.default_rng(5).permutation(len(kmers))
    synth.write_jdb(jdb, kmers[perm], np.full(len(kmers), 7, dtype=np.uint32), K)  # (values db_sort -z has to zero)
    return {"dir": d, "recs": recs, "fa": fa, "kmers": kmers, "jdb": jdb, "want": {}}


def _ref(tool):
    p = os.path.join(REF, tool)
    assert os.path.exists(p), f"oracle/_ref/{tool} is built by oracle/Makefile (target ref) where the reference's sources are present"
    return p


def _want(trial, nt):
    """the reference's db_sort -z over the model's list, once per nt: (database.kdb, database.idx) paths"""
    if nt not in trial["want"]:
        kdb, idx = str(trial["dir"] / f"want{nt}.kdb"), str(trial["dir"] / f"want{nt}.idx")
        r = subprocess.run([_ref("db_sort"), "-z", "-t", "1", "-n", str(nt), "-d", trial["jdb"], "-o", kdb, "-i", idx], stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()
        trial["want"][nt] = (kdb, idx)
    return trial["want"][nt]


def _same_file(a, b):
    """byte equality without holding both files in memory (the index of nt = 15 has 8 GiB)"""
    if os.path.getsize(a) != os.path.getsize(b):
        return False
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(1 << 26), fb.read(1 << 26)
            if x != y:
                return False
            if not x:
                return True


def _kmer_db(args, fa, out_dir, tag="got", default_budget=False):
    kdb, idx = os.path.join(str(out_dir), f"{tag}.kdb"), os.path.join(str(out_dir), f"{tag}.idx")
    if "-s" not in args and not default_budget:
        args = ["-s", str(SMALL)] + args
    r = subprocess.run([KMER_DB, "-v", "-o", kdb, "-i", idx] + args + ([fa] if isinstance(fa, str) else fa), stderr=subprocess.PIPE)
    return r, kdb, idx


def _verbose(r, what):
    """per pass, the count that -v prints in front of `what`"""
    return [int(x) for x in re.findall(rf"(\d+) {what}", r.stderr.decode())]


# --------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 9, 15])
def test_trial_library_equals_the_reference_byte_for_byte(trial, tmp_path, nt):
    want_kdb, want_idx = _want(trial, nt)
    r, kdb, idx = _kmer_db(["-n", str(nt)], trial["fa"], tmp_path, default_budget=nt == 9)  # (-s left out once)
    assert r.returncode == 0, r.stderr.decode()
    assert _same_file(kdb, want_kdb) and _same_file(idx, want_idx)
    assert _verbose(r, "windows") == [27895] and _verbose(r, "distinct k-mers")[0] == len(trial["kmers"])
    if nt == 15:  # 16 GiB of index files: gone before the next test
        os.unlink(idx)
        os.unlink(want_idx)
        del trial["want"][nt]


@pytest.mark.gpu
def test_reference_set_lcas_certifies_the_set(trial, tmp_path):
    """set_lcas without -x exits 0 only if no library k-mer is missing (src/set_lcas.cpp:441-442); with every record under one
    taxon no value stays 0 only if the database holds no k-mer the library lacks"""
    r, kdb, idx = _kmer_db(["-n", "9"], trial["fa"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    (tmp_path / "seqid2taxid.map").write_text("".join(f"seq{i}\t4\n" for i in range(len(trial["recs"]))))
    r = subprocess.run([_ref("set_lcas"), "-t", "1", "-d", kdb, "-o", str(tmp_path / "lca.kdb"), "-i", idx, "-b", f"{G}/f1/taxDB",
                        "-m", str(tmp_path / "seqid2taxid.map"), "-F", trial["fa"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    kmers, vals, *_ = synth.read_db(str(tmp_path), kdb="lca.kdb", idx="got.idx")
    assert len(vals) == len(trial["kmers"]) and (vals == 4).all()
    assert np.array_equal(np.sort(kmers), trial["kmers"])
    db = capi.Db(kdb, idx)  # the classify path opens it
    assert db.info.key_ct == len(trial["kmers"]) and (db.info.k, db.info.nt, db.info.idx_type) == (K, 9, 2)


@pytest.mark.gpu
def test_binding_and_gzip_input_give_the_same_files(trial, tmp_path):
    want_kdb, want_idx = _want(trial, 9)
    key_ct, per_pass = capi.kmer_db_files(trial["recs"], str(tmp_path / "b.kdb"), str(tmp_path / "b.idx"), K, 9, device_bytes=SMALL)
    assert key_ct == len(trial["kmers"]) and len(per_pass) == 1
    assert (per_pass[0].windows, per_pass[0].distinct, per_pass[0].segments) == (27895, key_ct, 6)  # the record below k uploads nothing
    assert _same_file(str(tmp_path / "b.kdb"), want_kdb) and _same_file(str(tmp_path / "b.idx"), want_idx)
    gz = str(tmp_path / "library.fa.gz")
    with open(trial["fa"], "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    r, kdb, idx = _kmer_db(["-n", "9", "-t", "2"], gz, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert _same_file(kdb, want_kdb) and _same_file(idx, want_idx)


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 3, 7, 64])
def test_passes_give_identical_bytes(trial, tmp_path, passes):
    """nt = 3: 64 bins, so -P 64 has one bin per pass and most passes receive no k-mer at all"""
    want_kdb, want_idx = _want(trial, 3)
    r, kdb, idx = _kmer_db(["-n", "3", "-P", str(passes)], trial["fa"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert _same_file(kdb, want_kdb) and _same_file(idx, want_idx)
    distinct = _verbose(r, "distinct k-mers")
    assert len(distinct) == passes + 1 and sum(distinct[:-1]) == distinct[-1] == len(trial["kmers"])
    assert _verbose(r, "windows") == [27895] * passes
    if passes == 64:
        assert distinct[:-1].count(0) > 10  # passes whose bin range is empty
    if passes > 1:
        assert sum(_verbose(r, "candidates")) == valid_windows(trial["recs"], K)  # each lands in exactly one pass


def _budget_for(capacity):
    """the smallest device_bytes whose buffers hold `capacity` k-mers (the documented rule, inverted by search)"""
    b = capacity * 16
    while capi.kmer_db_capacity(b)[0] < capacity:
        b += 16
    return b


@pytest.mark.gpu
def test_many_flushes_do_not_change_the_files(trial, tmp_path):
    """a buffer that only just holds the distinct set (1/64 of it has to stay free): the candidates arrive in ever smaller
    batches, each sorted, made unique and merged into the set"""
    want_kdb, want_idx = _want(trial, 9)
    n = len(trial["kmers"])
    budget = _budget_for(n * 64 // 63 + 64)
    cap, seg = capi.kmer_db_capacity(budget)
    assert cap - cap // 64 >= n and seg < 6000  # the set fits; the records are cut as well
    r, kdb, idx = _kmer_db(["-n", "9", "-s", str(budget)], trial["fa"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert _verbose(r, "flushes")[0] >= 5, r.stderr.decode()
    # every flush but the first merges into the set, in pieces of at most capacity / 4 k-mers of either side (the way buffers of
    # more than 2^32 k-mers are merged, which rocprim::merge cannot take in one call): several calls per flush here
    assert _verbose(r, "merge calls")[0] >= 3 * (_verbose(r, "flushes")[0] - 1) // 2, r.stderr.decode()
    assert _verbose(r, "segments")[0] >= 8
    assert _same_file(kdb, want_kdb) and _same_file(idx, want_idx)
    # the K / M / G suffixes of -s: one flush at the end, same files
    r, kdb, idx = _kmer_db(["-n", "9", "-s", "1M"], trial["fa"], tmp_path, tag="one")
    assert r.returncode == 0 and _verbose(r, "flushes") == [1]
    assert _same_file(kdb, want_kdb) and _same_file(idx, want_idx)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
def test_buffer_filled_exactly_and_by_one_more(tmp_path, extra):
    """128 KiB: a buffer of 8064 k-mers, segments of 2 KiB.  Two records with 8064 windows between them, none ambiguous, fill
    it to the last place before the one flush at the end of the pass; one window more and the last launch no longer fits:
    the buffer is flushed before it.  (The second record repeats the first, so the distinct set stays well inside.)"""
    budget = 128 << 10
    cap, seg = capi.kmer_db_capacity(budget)
    assert (cap, seg) == (8064, 2048)
    g = synth.codes_to_ascii(synth.procedural_genome(21, 3, cap // 2 + K))
    recs = [g[:cap // 2 + K - 1], g[:cap // 2 + K - 1 + extra]]
    key_ct, per_pass = capi.kmer_db_files(recs, str(tmp_path / "database.kdb"), str(tmp_path / "database.idx"), K, 8,
                                          device_bytes=budget)
    st = per_pass[0]
    assert (st.capacity, st.segment_bytes) == (cap, seg)
    assert st.windows == st.candidates == cap + extra
    assert st.flushes == 1 + extra
    kmers = model_kmers(recs, K)
    assert key_ct == len(kmers) == cap // 2 + extra
    sk, sv, off = synth.sort_db(kmers, np.zeros(len(kmers), dtype=np.uint32), K, 8)
    synth.write_db(str(tmp_path / "want"), sk, sv, off, K, 8)
    for fn in ("database.kdb", "database.idx"):
        assert (tmp_path / fn).read_bytes() == (tmp_path / "want" / fn).read_bytes(), fn


@pytest.mark.gpu
def test_budget_errors(trial, tmp_path):
    out = (str(tmp_path / "o.kdb"), str(tmp_path / "o.idx"))
    with pytest.raises(capi.KuError) as e:  # below the documented minimum
        capi.KmerDb(*out, K, 9, device_bytes=capi.KU_KMERDB_MIN_BYTES - 1)
    assert e.value.status == -1 and not os.path.exists(out[0]) and not os.path.exists(out[1])
    with pytest.raises(capi.KuError) as e:  # the minimum itself holds 4032 k-mers: the trial library's set does not fit
        capi.kmer_db_files(trial["recs"], *out, K, 9, device_bytes=capi.KU_KMERDB_MIN_BYTES)
    assert e.value.status == -4 and "-P" in str(e.value)
    assert not os.path.exists(out[0]) and not os.path.exists(out[1])
    r, kdb, idx = _kmer_db(["-n", "9", "-s", "64K"], trial["fa"], tmp_path)
    assert r.returncode == 71 and b"-P" in r.stderr and not os.path.exists(kdb) and not os.path.exists(idx)
    # ... and with enough passes it does
    passes = passes_that_fit(trial["kmers"], K, 9, 4032)
    assert passes > 1
    r, kdb, idx = _kmer_db(["-n", "9", "-s", "64K", "-P", str(passes)], trial["fa"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert max(_verbose(r, "distinct k-mers")[:-1]) > 4032 // 2  # (the fullest pass does use the buffer)
    assert _same_file(kdb, _want(trial, 9)[0]) and _same_file(idx, _want(trial, 9)[1])


@pytest.mark.gpu
def test_segment_cuts_lose_and_repeat_nothing(tmp_path):
    """one record of 200 kb under 3 MiB: segments of 49152 bytes that overlap by k - 1, i.e. five of them, the windows of
    segment i starting at 49122 * i.  Ambiguous letters on the last byte of a segment, on the first window start behind a
    cut, and k - 1 bytes before one."""
    budget = 3 << 20
    cap, seg = capi.kmer_db_capacity(budget)
    step = seg - (K - 1)
    s = bytearray(synth.codes_to_ascii(synth.procedural_genome(31, 3, 200000)))
    assert seg == 49152 and len(s) > 4 * step + K
    s[seg - 1] = ord("N")            # the last byte segment 0 holds
    s[2 * step] = ord("R")           # the first byte of segment 2 = the first window start behind the cut
    s[3 * step - (K - 1)] = ord("n")  # k - 1 before the cut: the last window of segment 2 starts right behind it
    s[4 * step - 1] = ord("N")       # the last window start of segment 3
    recs = [bytes(s)]
    kmers = model_kmers(recs, K)
    # (a budget with segments this short holds 193536 k-mers, fewer than the record has: several passes)
    assert cap - cap // 64 < len(kmers)
    passes = passes_that_fit(kmers, K, 6, cap)
    key_ct, per_pass = capi.kmer_db_files(recs, str(tmp_path / "database.kdb"), str(tmp_path / "database.idx"), K, 6, passes=passes,
                                          device_bytes=budget)
    assert [p.segments for p in per_pass] == [5] * passes and [p.windows for p in per_pass] == [200000 - K + 1] * passes
    assert valid_windows(recs, K) == 200000 - K + 1 - 4 * K
    assert key_ct == len(kmers) and sum(p.candidates for p in per_pass) == valid_windows(recs, K)
    sk, sv, off = synth.sort_db(kmers, np.zeros(len(kmers), dtype=np.uint32), K, 6)
    synth.write_db(str(tmp_path / "want"), sk, sv, off, K, 6)
    for fn in ("database.kdb", "database.idx"):
        assert (tmp_path / fn).read_bytes() == (tmp_path / "want" / fn).read_bytes(), fn


@pytest.mark.gpu
def test_another_k(trial, tmp_path):
    k, nt = 29, 7
    kmers = model_kmers(trial["recs"], k)
    r, kdb, idx = _kmer_db(["-k", str(k), "-n", str(nt)], trial["fa"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    sk, sv, off = synth.sort_db(kmers, np.zeros(len(kmers), dtype=np.uint32), k, nt)
    synth.write_db(str(tmp_path / "want"), sk, sv, off, k, nt)
    assert _same_file(kdb, str(tmp_path / "want" / "database.kdb")) and _same_file(idx, str(tmp_path / "want" / "database.idx"))
    assert capi.Db(kdb, idx).info.k == k


@pytest.mark.gpu
def test_errors(trial, tmp_path):
    ok = (str(tmp_path / "o.kdb"), str(tmp_path / "o.idx"))
    # an output that cannot be written: KU_ENOINPUT, and neither file is left behind
    for kdb, idx in ((str(tmp_path / "no_such_dir" / "o.kdb"), ok[1]), (ok[0], str(tmp_path / "no_such_dir" / "o.idx"))):
        with pytest.raises(capi.KuError) as e:
            capi.KmerDb(kdb, idx, K, 9, device_bytes=SMALL)
        assert e.value.status == -3
        assert not os.path.exists(ok[0]) and not os.path.exists(ok[1])
    r, kdb, idx = _kmer_db(["-n", "9"], trial["fa"], tmp_path / "no_such_dir")
    assert r.returncode == 66
    # no window of k valid bases anywhere
    with pytest.raises(capi.KuError) as e:
        capi.kmer_db_files([b"ACGT" * 7, b"N" * 50, b"ACGTACGTACGTACGNACGTACGTACGTACGTACGT"], *ok, K, 9, device_bytes=SMALL)
    assert e.value.status == -2 and "no k-mers in the input" in str(e.value)
    assert not os.path.exists(ok[0]) and not os.path.exists(ok[1])
    (tmp_path / "empty.fa").write_text(">only\nACGTNNNN\n")
    r, kdb, idx = _kmer_db(["-n", "9"], str(tmp_path / "empty.fa"), tmp_path)
    assert r.returncode == 65 and b"no k-mers in the input" in r.stderr and not os.path.exists(idx)
    # arguments the library checks itself
    for k, nt, passes in ((31, 0, 1), (31, 16, 1), (32, 9, 1), (8, 9, 1), (31, 9, 0), (31, 2, 17)):
        with pytest.raises(capi.KuError) as e:
            capi.KmerDb(*ok, k, nt, passes, device_bytes=SMALL)
        assert e.value.status == -1, (k, nt, passes)
    # calls out of order
    with capi.KmerDb(*ok, K, 9, passes=2, device_bytes=SMALL) as b:
        b.add(trial["recs"][0])
        b.end_pass()
        with pytest.raises(capi.KuError) as e:  # the second pass has not been ended
            b.finish()
        assert e.value.status == -1
        b.add(trial["recs"][0])
        b.end_pass()
        with pytest.raises(capi.KuError) as e:  # a third pass
            b.end_pass()
        assert e.value.status == -1
        assert b.finish() == len(model_kmers(trial["recs"][:1], K))
        with pytest.raises(capi.KuError) as e:
            b.add(trial["recs"][0])
        assert e.value.status == -1
        with pytest.raises(capi.KuError) as e:
            b.finish()
        assert e.value.status == -1
    assert os.path.exists(ok[0]) and os.path.exists(ok[1])  # finished: the files stay


@pytest.mark.gpu
def test_a_corrupt_library_leaves_no_files(trial, tmp_path):
    """the input stage ends the program on a truncated gzip stream (exit 65), after the outputs were created: both are removed"""
    with open(trial["fa"], "rb") as f:
        gz = gzip.compress(f.read())
    (tmp_path / "cut.fa.gz").write_bytes(gz[:len(gz) // 2])
    r, kdb, idx = _kmer_db(["-n", "9", "-P", "2"], [trial["fa"], str(tmp_path / "cut.fa.gz")], tmp_path)
    assert r.returncode == 65 and b"gzip" in r.stderr, r.stderr.decode()
    assert not os.path.exists(kdb) and not os.path.exists(idx)


@pytest.mark.gpu
def test_the_build_end_to_end(tmp_path):
    """kmer_db -> set_lcas -> classify with this project's tools alone, against the reference's db_sort -z -> set_lcas over
    the model's k-mer list of the same library (tests/golden/f9), with the flags of tests/test_set_lcas.py"""
    lib, nt = f"{G}/f9/library.fa", 7
    _, seqs = synth.read_seqfile(lib)
    kmers = model_kmers(seqs, K)
    perm = np.random.default_rng(9).permutation(len(kmers))
    synth.write_jdb(str(tmp_path / "model.jdb"), kmers[perm], np.ones(len(kmers), dtype=np.uint32), K)

    def lcas(tool, kdb, idx, out):
        return subprocess.run([tool, "-M", "-x", "-t", "2", "-d", kdb, "-o", out, "-i", idx, "-b", f"{G}/f1/taxDB",
                               "-m", f"{G}/f9/seqid2taxid.map", "-F", lib], stdout=subprocess.PIPE, stderr=subprocess.PIPE)

    r = subprocess.run([_ref("db_sort"), "-z", "-t", "1", "-n", str(nt), "-d", str(tmp_path / "model.jdb"), "-o", str(tmp_path / "ref0.kdb"),
                        "-i", str(tmp_path / "ref.idx")], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    r = lcas(_ref("set_lcas"), str(tmp_path / "ref0.kdb"), str(tmp_path / "ref.idx"), str(tmp_path / "ref.kdb"))
    assert r.returncode == 0, r.stderr.decode()

    db = tmp_path / "db"
    db.mkdir()
    r, kdb0, idx = _kmer_db(["-n", str(nt)], lib, db, tag="database0")
    assert r.returncode == 0, r.stderr.decode()
    r = lcas(os.path.join(BIN, "set_lcas"), kdb0, idx, str(db / "database.kdb"))
    assert r.returncode == 0, r.stderr.decode()
    assert _same_file(str(db / "database.kdb"), str(tmp_path / "ref.kdb")) and _same_file(idx, str(tmp_path / "ref.idx"))
    vals = synth.read_db(str(db), idx="database0.idx")[1]
    assert len(vals) == len(kmers) and vals.any()

    shutil.copy(idx, db / "database.idx")
    r = subprocess.run([os.path.join(BIN, "classify"), "-d", str(db / "database.kdb"), "-i", str(db / "database.idx"), "-a", f"{G}/f1/taxDB",
                        "-o", str(tmp_path / "out.tsv"), f"{G}/f1/reads.fq"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    lines = (tmp_path / "out.tsv").read_text().splitlines()
    assert len(lines) == len(synth.read_seqfile(f"{G}/f1/reads.fq")[0]) and any(ln.startswith("C\t") for ln in lines)
