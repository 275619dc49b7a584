"""count_unique (ku_sketch_*, bin/count_unique) and kmer_db -P auto: HyperLogLog sketches of a library's k-mers on the GPU.

The reference's count_unique (src/count_unique.cpp) hashes every unambiguous FORWARD k-mer into dense registers and prints
min(windows observed, ertlCardinality(registers)).  The expected registers of a set of values are those of the oracle's dense
counter (oracle.ku_oracle.Hll(p, False)) after inserting every element, the expected estimate is
min(n_observed, ko_ertl_from_registers(registers, p, 1 << 62, 0)), and for the forward k-mers the reference's own binary
(oracle/_ref/count_unique) has to print the same number.  kmer_db -P auto sketches the canonical k-mers per range of the bin
keys and plans its passes from the estimates (ku_sketch_plan_passes); the rule is restated here with the oracle's estimator."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from krakenuniq_amd import capi, synth
from oracle import ku_oracle as ko
from built_kmers import unmix
from test_kmer_db import (_VALID, _kmer_db, _ref, _same_file, _trial_records, _want, model_kmers, passes_that_fit,
                          trial, valid_windows)  # noqa: F401  (trial: the module's fixture, with its reference files)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "krakenuniq_amd", "bin")
COUNT_UNIQUE = os.path.join(BIN, "count_unique")
KMER_DB = os.path.join(BIN, "kmer_db")
NAMES = ["ku_sketch_open", "ku_sketch_add", "ku_sketch_add_values", "ku_sketch_export", "ku_sketch_estimate", "ku_sketch_close",
         "ku_sketch_plan_passes"]
CANONICAL = 1
M64 = (1 << 64) - 1


# --------------------------------------------------------------------------- the models
def forward_kmers(seqs, k):
    """model_kmers without the canonical form: distinct forward k-mers of the windows made of ACGTacgt only"""
    parts = [np.zeros(0, dtype=np.uint64)]
    for s in seqs:
        a = np.frombuffer(s, dtype=np.uint8)
        bad = np.flatnonzero(~_VALID[a])
        lo = 0
        for hi in list(bad) + [len(a)]:
            if hi - lo >= k:
                parts.append(synth.kmers_forward(synth.ascii_to_codes(bytes(s[lo:hi]).upper()), k))
            lo = hi + 1
    return np.unique(np.concatenate(parts))


def oracle_registers(values, p):
    h = ko.Hll(p, False)
    for v in values.tolist():
        h.insert(v)
    return h.registers()


def ertl(registers, p):
    r = np.ascontiguousarray(registers, dtype=np.uint8)
    return int(ko.lib().ko_ertl_from_registers(ko._p(r, ko.u8p), p, 1 << 62, 0))


def expected_estimate(registers, p, n_observed):
    return min(n_observed, ertl(registers, p))


def plan_rule(registers, p, usable):
    """the rule of ku_sketch_plan_passes, restated: the smallest power of two P <= G with estimate * 11 <= usable * 10 for the
    max-merge of every pass's groups; None when P = G does not fit either"""
    g = registers.shape[0]
    n = 1
    while n <= g:
        fullest = max(ertl(registers[i * g // n:(i + 1) * g // n].max(axis=0), p) for i in range(n))
        if fullest * 11 <= usable * 10:
            return n
        n *= 2
    return None


def group_registers(canon, k, nt, n_groups, p):
    """oracle registers [n_groups, 2^p] of the canonical k-mers by the range of their bin key"""
    grp = (synth.bin_key(canon, k, nt).astype(np.uint64) * np.uint64(n_groups)) >> np.uint64(2 * nt)
    out = np.zeros((n_groups, 1 << p), dtype=np.uint8)
    for g in np.unique(grp):
        out[int(g)] = oracle_registers(canon[grp == g], p)
    return out


def ceil_11_10(e):
    """the smallest usable with e * 11 <= usable * 10"""
    return (e * 11 + 9) // 10


# --------------------------------------------------------------------------- CPU: command lines, names, planner
def _run(tool, args, **kw):
    kw.setdefault("stdin", subprocess.DEVNULL)
    return subprocess.run([tool] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)


def test_cli_usage_without_gpu():
    """(no device may be touched: a run that opened one would fail on a GPU-less machine with EX_SOFTWARE, not 64)"""
    assert os.path.exists(COUNT_UNIQUE), "build with make -C krakenuniq_amd/csrc"
    r = _run(COUNT_UNIQUE, ["-h"])
    assert r.returncode == 0 and b"Usage: count_unique" in r.stderr and r.stdout == b""
    for args in (["-k", "0"], ["-k", "32"], ["-p", "3"], ["-p", "19"], ["-t", "0"]):
        r = _run(COUNT_UNIQUE, args)
        assert r.returncode == 64 and r.stderr and r.stdout == b"", args
    assert b"k can't be <= 0" in _run(COUNT_UNIQUE, ["-k", "0"]).stderr  # the reference's messages
    assert b"k can't be > 31" in _run(COUNT_UNIQUE, ["-k", "32"]).stderr
    assert b"can't use nonpositive thread count" in _run(COUNT_UNIQUE, ["-t", "0"]).stderr


def test_kmer_db_auto_passes_need_files(tmp_path):
    out = ["-o", str(tmp_path / "a.kdb"), "-i", str(tmp_path / "a.idx")]
    for inputs in ([], ["-"]):
        r = _run(KMER_DB, ["-n", "7", "-P", "auto"] + out + inputs)
        assert r.returncode == 64 and b"once per pass" in r.stderr
    assert not os.path.exists(tmp_path / "a.kdb") and not os.path.exists(tmp_path / "a.idx")
    assert _run(KMER_DB, ["-n", "7", "-P", "some"] + out + ["lib.fa"]).returncode == 64  # still a number otherwise


def test_signatures_hold_the_sketch_names():
    assert [n for n in NAMES if n not in capi.SIGNATURES] == []
    L = capi.lib()
    assert all(hasattr(L, n) for n in NAMES)


@pytest.fixture(scope="module")
def four_groups():
    """G = 4, p = 12: groups of 3000 / 1000 / 300 / 100 distinct values"""
    rng = np.random.default_rng(17)
    vals = rng.integers(0, 1 << 63, 4400, dtype=np.uint64)
    assert len(np.unique(vals)) == 4400
    cuts = [0, 3000, 4000, 4300, 4400]
    return np.stack([oracle_registers(vals[a:b], 12) for a, b in zip(cuts, cuts[1:])])


def _plan(registers, usable):
    try:
        return capi.sketch_plan_passes(registers, usable)
    except capi.KuError as e:
        assert e.status == -4  # KU_ENOMEM
        return None, None


def test_planner_follows_the_restated_rule(four_groups):
    regs, p = four_groups, 12
    e1 = ertl(regs.max(axis=0), p)
    e2 = max(ertl(regs[:2].max(axis=0), p), ertl(regs[2:].max(axis=0), p))
    e4 = max(ertl(regs[g], p) for g in range(4))
    # (HLL at p = 12 is good to a few per cent: the estimates keep the order of the true counts 4400 > 4000 > 3000)
    assert abs(e1 - 4400) < 440 and abs(e2 - 4000) < 400 and abs(e4 - 3000) < 300 and e4 == ertl(regs[0], p)
    cases = [(10 * e1, 1, e1),                 # plenty of room
             (ceil_11_10(e1), 1, e1),          # exactly a tenth to spare ...
             (ceil_11_10(e1) - 1, 2, e2),      # ... and one k-mer less: the answer flips
             (ceil_11_10(e2), 2, e2),
             (ceil_11_10(e2) - 1, 4, e4),
             (ceil_11_10(e4), 4, e4),
             (ceil_11_10(e4) - 1, None, None)]  # the fullest single group does not fit: KU_ENOMEM
    for usable, want, fullest in cases:
        assert plan_rule(regs, p, usable) == want, usable
        assert _plan(regs, usable) == (want, fullest), usable
    with pytest.raises(capi.KuError) as e:
        capi.sketch_plan_passes(regs, ceil_11_10(e4) - 1)
    assert e.value.status == -4 and "budget" in str(e.value)


def test_planner_edges(four_groups):
    one = four_groups[:1]
    e = ertl(one[0], 12)
    assert _plan(one, ceil_11_10(e)) == (1, e) and _plan(one, ceil_11_10(e) - 1) == (None, None)  # G = 1: 1 or KU_ENOMEM
    for g, p in ((1, 4), (4, 12), (1024, 12), (2, 18)):
        assert _plan(np.zeros((g, 1 << p), dtype=np.uint8), 0) == (1, 0)  # all-zero registers: nothing to hold
    for shape in ((3, 4096), (2048, 16)):  # groups: a power of two up to 1024
        with pytest.raises(capi.KuError) as err:
            capi.sketch_plan_passes(np.zeros(shape, dtype=np.uint8), 100)
        assert err.value.status == -1
    for p in (3, 19):
        with pytest.raises(capi.KuError) as err:
            capi.sketch_plan_passes(np.zeros((1, 1 << p), dtype=np.uint8), 100)
        assert err.value.status == -1


# the two budgets of test_kmer_db_auto_passes (nt = 7, the trial library of tests/test_kmer_db.py: 17940 distinct k-mers), chosen
# with passes_that_fit, oracle registers and the restated rule: under 4 MiB the whole set fits one pass; 288 KiB hold 18176
# k-mers, the model needs 8 passes and the rule, with its tenth to spare, 16.  (The lowest range is by far the fullest, so a
# budget that one pass only just fits can cost more than one doubling: at 320 KiB the model needs 1 pass and the rule plans
# 8, since halving the ranges takes next to nothing off the fullest.  Such budgets are not used here.)
AUTO_BUDGETS = {4 << 20: (1, 1), 288 << 10: (8, 16)}  # device bytes -> (passes_that_fit of the model, passes the rule plans)


@pytest.fixture(scope="module")
def trial_groups():
    return group_registers(model_kmers(_trial_records(), 31), 31, 7, 1024, 12)


def test_budgets_of_the_auto_passes_test(trial_groups):
    """P below the model's would mean an estimate more than 10 % low; the margin can cost at most one doubling"""
    kmers = model_kmers(_trial_records(), 31)
    for budget, (p_model, p_rule) in AUTO_BUDGETS.items():
        cap = capi.kmer_db_capacity(budget)[0]
        assert passes_that_fit(kmers, 31, 7, cap) == p_model
        assert plan_rule(trial_groups, 12, cap - cap // 64) == p_rule and p_rule in (p_model, 2 * p_model)
        assert capi.sketch_plan_passes(trial_groups, cap - cap // 64)[0] == p_rule
    assert AUTO_BUDGETS[4 << 20][0] == 1 and AUTO_BUDGETS[288 << 10][0] >= 4


# --------------------------------------------------------------------------- GPU: the library against the oracle and the reference
PS = (4, 12, 14, 15, 18)


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """the trial library of tests/test_kmer_db.py plus a 120 kb record, an empty one and -- per k -- one of k - 1 bases"""
    g = synth.codes_to_ascii(synth.procedural_genome(21, 3, 40000))
    recs = _trial_records() + [g * 3, b""]
    return {"recs": recs, "dir": tmp_path_factory.mktemp("count_unique"), "short": g[500:530]}


def _records(library, k):
    return library["recs"] + [library["short"][:k - 1]]


def _reference_count(library, k, p):
    fa = str(library["dir"] / f"library_k{k}.fa")
    if not os.path.exists(fa):
        recs = _records(library, k)
        synth.write_fasta(fa, recs, ids=[f"seq{i}" for i in range(len(recs))], width=70)
    with open(fa, "rb") as f:
        r = subprocess.run([_ref("count_unique"), "-k", str(k), "-p", str(p)], stdin=f, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    return int(r.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, CANONICAL])
@pytest.mark.parametrize("k", [1, 12, 25, 31])
def test_trial_library_registers_and_estimates(library, k, flags):
    recs = _records(library, k)
    values = model_kmers(recs, k) if flags else forward_kmers(recs, k)
    windows = valid_windows(recs, k)
    assert len(values) == (4 if not flags else 2) if k == 1 else len(values) > 50000
    for p in PS:
        want = oracle_registers(values, p)
        with capi.Sketch(k, p, flags) as s:
            for r in recs:
                s.add(r)
            regs, n_observed = s.export()
            got = s.estimate()
        assert regs.shape == (1, 1 << p) and np.array_equal(regs[0], want), (k, p, flags)
        assert n_observed == windows
        assert got == expected_estimate(want, p, windows), (k, p, flags)
        if not flags:  # the forward k-mers: what the reference's binary counts
            assert got == _reference_count(library, k, p), (k, p)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 5])
def test_cuts_and_packing(k):
    """segments of 1 KiB: records that end one byte before the segment's end, on it, one byte behind it and k - 1 behind it,
    that span two and five segments, between records too short for a window, just long enough, and of one base"""
    g = synth.codes_to_ascii(synth.procedural_genome(33, 3, 12000))
    lens = [1023, k - 1, 1024, k, 1025, 1, 1024 + k - 1, k - 1, 2048, k, 5000, 1]
    recs, at = [], 0
    for n in lens:
        recs.append(g[at:at + n])
        at += n
    recs[4] = recs[4][:400] + b"N" + recs[4][401:].lower()  # (an ambiguous byte and lower case inside a record that is cut)
    p, half = 12, 6
    values = forward_kmers(recs, k)
    with capi.Sketch(k, p, segment_bytes=1024) as s:
        for r in recs[:half]:
            s.add(r)
        regs, n_observed = s.export()  # in the middle: what is staged is scanned
        assert n_observed == valid_windows(recs[:half], k) and np.array_equal(regs[0], oracle_registers(forward_kmers(recs[:half], k), p))
        for r in recs[half:]:
            s.add(r)
        regs, n_observed = s.export()
        assert s.export()[1] == n_observed  # (again: nothing is counted twice)
    assert n_observed == valid_windows(recs, k) and np.array_equal(regs[0], oracle_registers(values, p))
    with capi.Sketch(k, p) as s:  # the default segment
        for r in recs:
            s.add(r)
        regs0, n0 = s.export()
    assert n0 == n_observed and np.array_equal(regs0, regs)


def _built_hashes(p):
    m = 1 << p
    return [0, (m - 1) << (64 - p), ((5 % m) << (64 - p)) | 1, ((3 % m) << (64 - p)) | (1 << (63 - p))]


def test_unmix_inverts_the_hash():
    for p in PS:
        for h in _built_hashes(p):
            assert ko.lib().ko_hash(unmix(h)) == h


@pytest.mark.gpu
@pytest.mark.parametrize("p", PS)
def test_built_hashes_through_add_values(p):
    m = 1 << p
    values = np.array([unmix(h) for h in _built_hashes(p)], dtype=np.uint64)
    want = oracle_registers(values, p)
    # no bit behind the index: the saturated rank, at index 0 and at the last one; the lowest bit alone: one less; the first: 1
    assert {i: int(want[i]) for i in np.flatnonzero(want)} == {0: 64 - p + 1, m - 1: 64 - p + 1, 5 % m: 64 - p, 3 % m: 1}
    with capi.Sketch(31, p) as s:
        s.add_values(values)
        regs, n_observed = s.export()
        assert np.array_equal(regs[0], want) and n_observed == 4
        assert s.estimate() == expected_estimate(want, p, 4)
    with capi.Sketch(31, p, segment_bytes=1024) as s:  # one value 10 000 times: one register, every insert observed
        s.add_values(np.full(10000, 0x1234567, dtype=np.uint64))
        regs, n_observed = s.export()
        assert n_observed == 10000 and np.count_nonzero(regs) == 1
        assert np.array_equal(regs[0], oracle_registers(np.array([0x1234567], dtype=np.uint64), p))
    rnd = np.random.default_rng(p).integers(0, 1 << 64, 65536, dtype=np.uint64)
    with capi.Sketch(31, p) as s:
        s.add_values(rnd[:30000])
        s.add(b"ACGT" * 20)  # (sequence and values through the same staging segments)
        s.add_values(rnd[30000:])
        regs, n_observed = s.export()
    both = np.concatenate([rnd, forward_kmers([b"ACGT" * 20], 31)])
    assert n_observed == 65536 + 50 and np.array_equal(regs[0], oracle_registers(both, p))


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [7, 3])
def test_groups_follow_the_bin_key_ranges(nt):
    k, p, recs = 31, 12, _trial_records()
    n_groups = min(1024, 4 ** nt)
    canon = model_kmers(recs, k)
    want = group_registers(canon, k, nt, n_groups, p)
    with capi.Sketch(k, p, CANONICAL, nt, n_groups, segment_bytes=8192) as s:
        for r in recs:
            s.add(r)
        regs, n_observed = s.export()
        with pytest.raises(capi.KuError) as e:  # the estimate is the single sketch's
            s.estimate()
        assert e.value.status == -1
    assert regs.shape == (n_groups, 1 << p) and n_observed == valid_windows(recs, k)
    assert np.count_nonzero(want.any(axis=1)) >= 7  # (the low ranges are the fullest, and many stay empty: 7 of 64 for nt = 3)
    for g in range(n_groups):
        assert np.array_equal(regs[g], want[g]), g
    with capi.Sketch(k, p, CANONICAL) as s:
        for r in recs:
            s.add(r)
        one = s.export()[0]
    assert np.array_equal(regs.max(axis=0), one[0]) and np.array_equal(one[0], oracle_registers(canon, p))


@pytest.mark.gpu
def test_open_refuses_bad_arguments():
    for k, p, flags, nt, groups in ((0, 12, 0, 0, 1), (32, 12, 0, 0, 1), (31, 3, 0, 0, 1), (31, 19, 0, 0, 1), (31, 12, 2, 0, 1),
                                    (31, 12, 0, 7, 4), (31, 12, CANONICAL, 7, 3), (31, 12, CANONICAL, 7, 2048),
                                    (31, 12, CANONICAL, 2, 32), (31, 12, CANONICAL, 0, 4), (5, 12, CANONICAL, 7, 4),
                                    (31, 12, CANONICAL, 7, 0)):
        with pytest.raises(capi.KuError) as e:
            capi.Sketch(k, p, flags, nt, groups)
        assert e.value.status == -1, (k, p, flags, nt, groups)
    with capi.Sketch(31, 12, CANONICAL, 7, 4) as s:
        with pytest.raises(capi.KuError) as e:
            s.add_values(np.arange(4, dtype=np.uint64))
        assert e.value.status == -1


# --------------------------------------------------------------------------- GPU: the command lines
def _count(args, **kw):
    r = _run(COUNT_UNIQUE, args, **kw)
    assert r.returncode == 0, r.stderr.decode()
    return r


@pytest.mark.gpu
def test_cli_equals_the_reference(tmp_path):
    edge, lib = f"{G}/f2/edge.fa", f"{G}/f9/library.fa"
    with open(edge, "rb") as f:
        want = subprocess.run([_ref("count_unique"), "-k", "31", "-p", "12"], stdin=f, stdout=subprocess.PIPE).stdout
    assert want == open(f"{G}/count_unique_edge.txt", "rb").read() == b"294\n"
    with open(edge, "rb") as f:
        assert _count(["-p", "12"], stdin=f).stdout == want
    with open(lib, "rb") as f:
        want = subprocess.run([_ref("count_unique")], stdin=f, stdout=subprocess.PIPE).stdout
    assert int(want) > 1000
    with open(lib, "rb") as f:
        assert _count([], stdin=f).stdout == want  # standard input
    with open(lib, "rb") as f:
        assert _count(["-t", "4096", "-"], stdin=f).stdout == want  # ... by name; a thread count the reference would refuse
    r = _count(["-v", lib])  # a file
    assert r.stdout == want and re.search(rb"\d+ bytes, \d+ windows, [\d.]+ s, [\d.]+ MB/s", r.stderr)
    gz = str(tmp_path / "library.fa.gz")
    with open(lib, "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    assert _count([gz]).stdout == want
    ids, seqs = synth.read_seqfile(lib)
    assert len(seqs) >= 2
    half = len(seqs) // 2
    synth.write_fasta(str(tmp_path / "a.fa"), seqs[:half], ids=ids[:half], width=60)
    synth.write_fasta(str(tmp_path / "b.fa"), seqs[half:], ids=ids[half:], width=80)
    assert _count([str(tmp_path / "a.fa"), str(tmp_path / "b.fa")]).stdout == want
    _, lib_seqs = synth.read_seqfile(lib)  # -C: the canonical k-mers, against the oracle
    canon = model_kmers(lib_seqs, 31)
    assert int(_count(["-C", lib]).stdout) == expected_estimate(oracle_registers(canon, 14), 14, valid_windows(lib_seqs, 31))
    (tmp_path / "empty.fa").write_bytes(b"")
    r = _count([str(tmp_path / "empty.fa")])
    assert r.stdout == b"0\n" and r.stderr
    assert _run(COUNT_UNIQUE, [str(tmp_path / "missing.fa")]).returncode == 66


@pytest.mark.gpu
@pytest.mark.parametrize("budget", sorted(AUTO_BUDGETS))
def test_kmer_db_auto_passes(trial, trial_groups, tmp_path, budget):
    p_model, p_rule = AUTO_BUDGETS[budget]
    cap = capi.kmer_db_capacity(budget)[0]
    usable = cap - cap // 64
    r, kdb, idx = _kmer_db(["-n", "7", "-P", "auto", "-s", str(budget)], trial["fa"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    m = re.search(r"planned passes: (\d+) \(fullest range ≈ (\d+) k-mers of (\d+)\)", r.stderr.decode())
    assert m, r.stderr.decode()
    assert int(m.group(1)) == plan_rule(trial_groups, 12, usable) == p_rule and int(m.group(3)) == usable
    assert int(m.group(1)) in (p_model, 2 * p_model)
    assert len(re.findall(r"pass \d+/%d:" % p_rule, r.stderr.decode())) == p_rule
    want_kdb, want_idx = _want(trial, 7)
    assert _same_file(kdb, want_kdb) and _same_file(idx, want_idx)


@pytest.mark.gpu
def test_kmer_db_auto_passes_without_a_fit(trial, tmp_path):
    """nt = 1: four ranges at the most, and the fullest holds far more than the minimum budget: EX_SOFTWARE, -s named, no files"""
    r, kdb, idx = _kmer_db(["-n", "1", "-P", "auto", "-s", "64K"], trial["fa"], tmp_path)
    assert r.returncode == 70 and b"-s" in r.stderr, r.stderr.decode()
    assert not os.path.exists(kdb) and not os.path.exists(idx)
