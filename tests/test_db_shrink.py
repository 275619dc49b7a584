"""db_shrink on the GPU (ku_db_shrink_files, bin/db_shrink).  Every comparison is byte equality with the reference's files
(tests/golden/db_shrink) or with the numpy model that tests/test_db_shrink_host.py certifies against them
(tests/db_shrink_model.py); where oracle/_ref/db_sort is present the database mode is also held to the reference's db_sort over
the shrunk list."""
import os
import subprocess

import numpy as np
import pytest

import db_shrink_model as model
from krakenuniq_amd import capi, synth
from oracle import ku_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "db_shrink")
F1 = os.path.join(ROOT, "tests", "golden", "f1")
DB_SHRINK = os.path.join(ROOT, "krakenuniq_amd", "bin", "db_shrink")
REF_DB_SORT = os.path.join(ROOT, "oracle", "_ref", "db_sort")
SMALL = 4 << 20  # device budget of most runs (the default, half of the free HBM, takes seconds to allocate)
KEY_CT = 5000


def _cli(args):
    return subprocess.run([DB_SHRINK] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def dbs(tmp_path_factory):
    """one set of 5000 k-mers, values up to 2^32 - 1, as a sorted database for nt = 1, 3 and 9: nt -> (kdb, idx)"""
    rng = np.random.default_rng(21)
    kmers = np.unique(rng.integers(0, 1 << 62, KEY_CT, dtype=np.uint64))
    assert len(kmers) == KEY_CT
    vals = rng.integers(1, 1 << 32, KEY_CT, dtype=np.uint64).astype(np.uint32)
    assert (vals > 1 << 31).sum() > 1000
    out = {}
    for nt in (1, 3, 9):
        d = tmp_path_factory.mktemp(f"db_shrink_nt{nt}")
        synth.write_db(str(d), *synth.sort_db(kmers, vals, 31, nt), 31, nt)
        out[nt] = (str(d / "database.kdb"), str(d / "database.idx"))
    return out


# --------------------------------------------------------------------------- list mode: the reference's files
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(model.FIXTURES))
def test_list_mode_equals_the_golden_files(name, tmp_path):
    """through the executable and through the binding; list37_k27 has records of 7 + 4 bytes"""
    src = os.path.join(GOLD, name + ".jdb")
    for n, O in model.FIXTURES[name][2]:
        want = _bytes(os.path.join(GOLD, f"{name}_n{n}_O{O}.jdb"))
        out = str(tmp_path / f"cli_{n}_{O}.jdb")
        r = _cli(["-d", src, "-o", out, "-n", str(n), "-O", str(O), "-s", "4M"])
        assert r.returncode == 0, r.stderr.decode()
        assert _bytes(out) == want, (n, O)
        out = str(tmp_path / f"api_{n}_{O}.jdb")
        st = capi.db_shrink_files(src, out, n, O, device_bytes=SMALL)
        assert _bytes(out) == want, (n, O)
        key_ct = model.FIXTURES[name][1]
        assert (st.key_ct_in, st.key_ct_out, st.block_size, st.odd_blocks, st.chunks) == (key_ct, n, key_ct // n, key_ct % n, 1)
    r = _cli(["-d", src, "-o", str(tmp_path / "default_O.jdb"), "-n", "5", "-v", "-s", "4M"])  # -O defaults to 1
    assert r.returncode == 0 and b"5 of " in r.stderr and b"records written" in r.stderr
    assert _bytes(tmp_path / "default_O.jdb") == model.shrink_list_bytes(src, 5, 1)


# --------------------------------------------------------------------------- database mode: the model's files
def _cases(nt):
    """(n, O) over 5000 records"""
    cases = [(1000, 5), (1000, 1),      # key_ct % n == 0: the last and the first record of every block
             (1700, 2),                 # bs = 2, 1600 blocks of 3: O == bs while odd blocks exist
             (1700, 1), (7, 1), (7, 714),
             (KEY_CT, 1),               # every record
             (1, KEY_CT), (1, 1),       # one record: the first and the last of the input
             (3, 700)]                  # three records: most bins of nt = 9 become empty, the first and the last filled ones too
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 3, 9])
def test_database_mode_equals_the_model(dbs, tmp_path, nt):
    kdb, idx = dbs[nt]
    for n, O in _cases(nt):
        assert model.rule_ok(KEY_CT, n, O)
        want = model.write_model(kdb, idx, n, O, str(tmp_path / "want.kdb"), str(tmp_path / "want.idx"))
        got = (str(tmp_path / "got.kdb"), str(tmp_path / "got.idx"))
        st = capi.db_shrink_files(kdb, got[0], n, O, in_idx=idx, out_idx=got[1], device_bytes=SMALL)
        assert _bytes(got[0]) == _bytes(want[0]), (n, O)
        assert _bytes(got[1]) == _bytes(want[1]), (n, O)
        assert (st.key_ct_in, st.key_ct_out, st.block_size, st.odd_blocks) == (KEY_CT, n, KEY_CT // n, KEY_CT % n)
        info = capi.Db(*got).info
        assert (info.key_ct, info.nt, info.idx_type, info.k) == (n, nt, 2, 31)
        if (n, O) == (3, 700) and nt == 9:  # bins that held records and hold none now, the first and the last filled one among them
            old, new = synth.read_db(os.path.dirname(kdb))[2].astype(np.int64), synth.read_db(str(tmp_path), "got.kdb", "got.idx")[2].astype(np.int64)
            filled, still = np.flatnonzero(np.diff(old)), np.flatnonzero(np.diff(new))
            assert len(still) <= 3 and filled[0] not in still and filled[-1] not in still
        if os.path.exists(REF_DB_SORT):  # the recipe of scripts/shrink_db.sh: the list, then db_sort over it
            lst = str(tmp_path / "list.jdb")
            capi.db_shrink_files(kdb, lst, n, O, device_bytes=SMALL)
            assert _bytes(lst) == _bytes(want[0])
            r = subprocess.run([REF_DB_SORT, "-t", "1", "-n", str(nt), "-d", lst, "-o", str(tmp_path / "ref.kdb"), "-i", str(tmp_path / "ref.idx")],
                               stderr=subprocess.PIPE)
            assert r.returncode == 0, r.stderr.decode()
            assert _bytes(got[0]) == _bytes(tmp_path / "ref.kdb") and _bytes(got[1]) == _bytes(tmp_path / "ref.idx"), (n, O)


@pytest.mark.gpu
def test_database_mode_through_the_program(dbs, tmp_path):
    kdb, idx = dbs[3]
    got = (str(tmp_path / "got.kdb"), str(tmp_path / "got.idx"))
    r = _cli(["-d", kdb, "-i", idx, "-o", got[0], "-I", got[1], "-n", "1700", "-O", "2", "-s", "64K", "-v"])
    assert r.returncode == 0, r.stderr.decode()
    assert b"1700 of 5000 records written" in r.stderr and b"3 chunks" in r.stderr
    want = model.write_model(kdb, idx, 1700, 2, str(tmp_path / "want.kdb"), str(tmp_path / "want.idx"))
    assert _bytes(got[0]) == _bytes(want[0]) and _bytes(got[1]) == _bytes(want[1])


@pytest.mark.gpu
def test_database_mode_at_key_len_7(tmp_path):
    """k = 27: records of 7 + 4 bytes, read and written byte by byte, chunk cuts at record boundaries that no dword shares"""
    rng = np.random.default_rng(23)
    kmers = np.unique(rng.integers(0, 1 << 54, 6000, dtype=np.uint64))
    vals = rng.integers(1, 1 << 32, len(kmers), dtype=np.uint64).astype(np.uint32)
    sk, sv, off = synth.sort_db(kmers, vals, 27, 4)
    kdb, idx = str(tmp_path / "in.kdb"), str(tmp_path / "in.idx")
    model.write_list(kdb, sk, sv, 27)
    with open(idx, "wb") as f:
        f.write(b"KRAKIX2\x04" + off.astype("<u8").tobytes())
    for n, O, budget in ((777, 3, capi.KU_DBSHRINK_MIN_BYTES), (len(kmers), 1, capi.KU_DBSHRINK_MIN_BYTES), (2, 1, SMALL)):
        want = model.write_model(kdb, idx, n, O, str(tmp_path / "want.kdb"), str(tmp_path / "want.idx"))
        got = (str(tmp_path / "got.kdb"), str(tmp_path / "got.idx"))
        st = capi.db_shrink_files(kdb, got[0], n, O, in_idx=idx, out_idx=got[1], device_bytes=budget)
        assert _bytes(got[0]) == _bytes(want[0]) and _bytes(got[1]) == _bytes(want[1]), (n, O)
        assert st.chunks == -(-len(kmers) // capi.db_shrink_capacity(budget)[0])
    assert capi.Db(*got).info.key_len == 7


# --------------------------------------------------------------------------- the result loads and classifies
@pytest.mark.gpu
def test_the_shrunk_database_classifies(tmp_path):
    """tests/golden/f1 shrunk to a third: one batch of its reads through a context equals the CPU oracle on the same files"""
    key_ct = capi.Db(f"{F1}/database.kdb", f"{F1}/database.idx").info.key_ct
    kdb, idx = str(tmp_path / "database.kdb"), str(tmp_path / "database.idx")
    capi.db_shrink_files(f"{F1}/database.kdb", kdb, key_ct // 3, 2, in_idx=f"{F1}/database.idx", out_idx=idx, device_bytes=SMALL)
    want = model.write_model(f"{F1}/database.kdb", f"{F1}/database.idx", key_ct // 3, 2, str(tmp_path / "want.kdb"), str(tmp_path / "want.idx"))
    assert _bytes(kdb) == _bytes(want[0]) and _bytes(idx) == _bytes(want[1])
    ids, seqs = synth.read_seqfile(f"{F1}/reads.fq")
    buf, off, lens = ko.pack_reads(seqs)
    ctx = capi.Ctx(0)
    cdb, ctax = capi.Db(kdb, idx), capi.Tax(f"{F1}/taxDB")
    ctx.load_db(cdb)
    ctx.set_taxonomy(ctax)
    gpu = ctx.classify_batch(buf, off, lens)
    run = ko.Run(ko.Db(kdb, idx), ko.Tax(f"{F1}/taxDB"))
    res = run.classify(seqs)
    assert (gpu["calls"] == res["calls"]).all()
    assert (res["calls"] != 0).sum() > 100
    text = capi.format_kraken(buf, off, lens, ids, 31, gpu["calls"], taxa=gpu["taxa"])
    taxa = np.zeros(len(buf), dtype=np.uint32)
    for i in range(len(seqs)):
        a, n = int(res["taxa_off"][i]), int(res["n_slots"][i])
        t = res["taxa"][a:a + n].copy()
        t[res["ambig"][a:a + n] != 0] = capi.KU_AMBIG
        taxa[int(off[i]):int(off[i]) + n] = t
    assert text == capi.format_kraken(buf, off, lens, ids, 31, res["calls"], taxa=taxa)  # per-k-mer hits too
    assert text != _bytes(f"{F1}/out.tsv").decode()  # (a third of the k-mers: not the full database's hits)


# --------------------------------------------------------------------------- budgets
def _chunks(key_ct, budget):
    return -(-key_ct // capi.db_shrink_capacity(budget)[0])


@pytest.mark.gpu
def test_every_budget_gives_the_same_files(dbs, tmp_path):
    """the minimum (chunks of 2389 records: cuts at 2389 and 4778), a budget whose three chunks are cut elsewhere, and the default"""
    kdb, idx = dbs[3]
    three = 68000
    assert capi.db_shrink_capacity(capi.KU_DBSHRINK_MIN_BYTES)[0] == 2389 and capi.db_shrink_capacity(three)[0] == 2479
    assert _chunks(KEY_CT, capi.KU_DBSHRINK_MIN_BYTES) == 3 and _chunks(KEY_CT, three) == 3
    # (1000, 5): blocks of 5, the cut at 2389 falls inside one; (1700, 2): blocks of 3 then of 2; (2, 1): blocks of 2500, the
    # first chunk selects nothing; (1, 1): the block is larger than a chunk, the first two select nothing
    for n, O in ((1000, 5), (1000, 1), (1700, 2), (2, 1), (1, 1), (1, KEY_CT), (KEY_CT, 1)):
        want = model.write_model(kdb, idx, n, O, str(tmp_path / "want.kdb"), str(tmp_path / "want.idx"))
        for budget in (capi.KU_DBSHRINK_MIN_BYTES, three) + ((0,) if (n, O) == (1700, 2) else ()):
            got = (str(tmp_path / "got.kdb"), str(tmp_path / "got.idx"))
            st = capi.db_shrink_files(kdb, got[0], n, O, in_idx=idx, out_idx=got[1], device_bytes=budget)
            assert _bytes(got[0]) == _bytes(want[0]) and _bytes(got[1]) == _bytes(want[1]), (n, O, budget)
            if budget:
                assert (st.chunks, st.chunk_records) == (3, capi.db_shrink_capacity(budget)[0])
            else:
                assert st.chunks == 1 and st.chunk_records > KEY_CT
    # the index in slices: nt = 9 has 262144 offsets, the minimum budget maps 1024 at a time
    kdb, idx = dbs[9]
    assert capi.db_shrink_capacity(capi.KU_DBSHRINK_MIN_BYTES)[1] == 1024
    want = model.write_model(kdb, idx, 1700, 2, str(tmp_path / "want.kdb"), str(tmp_path / "want.idx"))
    got = (str(tmp_path / "got9.kdb"), str(tmp_path / "got9.idx"))
    capi.db_shrink_files(kdb, got[0], 1700, 2, in_idx=idx, out_idx=got[1], device_bytes=capi.KU_DBSHRINK_MIN_BYTES)
    assert _bytes(got[0]) == _bytes(want[0]) and _bytes(got[1]) == _bytes(want[1])


@pytest.mark.gpu
def test_chunk_cuts_on_block_ends_and_chunks_that_select_nothing(tmp_path):
    """a list of 5 * 2389 records at the minimum budget: with n = 5 every chunk is one block (O = 1: its last record, O = 2389:
    its first); with n = 2389 every cut is a block end as well; with n = 2 the blocks are larger than a chunk, and three of the
    five chunks select nothing"""
    cap = capi.db_shrink_capacity(capi.KU_DBSHRINK_MIN_BYTES)[0]
    key_ct = 5 * cap
    rng = np.random.default_rng(29)
    src = str(tmp_path / "in.jdb")
    synth.write_jdb(src, rng.integers(0, 1 << 62, key_ct, dtype=np.uint64), rng.integers(0, 1 << 32, key_ct, dtype=np.uint64).astype(np.uint32), 31)
    for n, O in ((5, 1), (5, cap), (5, 1000), (cap, 1), (cap, 5), (2, 1), (2, 5972), (key_ct - 1, 1)):
        assert model.rule_ok(key_ct, n, O)
        bounds = [model.S(key_ct, n, O, c * cap) for c in range(6)]
        if n == 2:
            assert sum(a == b for a, b in zip(bounds[:-1], bounds[1:])) == 3
        out = str(tmp_path / "out.jdb")
        st = capi.db_shrink_files(src, out, n, O, device_bytes=capi.KU_DBSHRINK_MIN_BYTES)
        assert _bytes(out) == model.shrink_list_bytes(src, n, O), (n, O)
        assert (st.chunks, st.chunk_records) == (5, cap)


# --------------------------------------------------------------------------- errors: the status, and nothing left behind
@pytest.mark.gpu
def test_errors_leave_no_output(dbs, tmp_path):
    kdb, idx = dbs[3]
    lst = os.path.join(GOLD, "list1000.jdb")
    work = tmp_path / "work"
    work.mkdir()
    out, out_idx = str(work / "out.kdb"), str(work / "out.idx")
    img, ix = _bytes(lst), _bytes(idx)
    (tmp_path / "type1.idx").write_bytes(b"KRAKIDX" + ix[7:])
    (tmp_path / "short.jdb").write_bytes(img[:-5])
    (tmp_path / "magic.jdb").write_bytes(b"JFLISTDX" + img[8:])
    os.symlink(lst, tmp_path / "link.jdb")
    db = ["-d", kdb, "-i", idx, "-o", out, "-I", out_idx]
    cases = [  # (arguments, exit code, status of the binding or None where the binding cannot express it, text)
        (["-d", lst, "-o", out, "-n", "1001"], 65, -2, "larger than old key count"),
        (["-d", lst, "-o", out, "-n", "300", "-O", "4"], 65, -2, "larger than block size"),
        (db + ["-n", "5001"], 65, -2, "larger than old key count"),
        (db + ["-n", "1700", "-O", "3"], 65, -2, "larger than block size"),
        (["-d", lst, "-o", out, "-n", "0"], 64, -1, "positive"),
        (["-d", lst, "-o", out, "-n", "7", "-O", "0"], 64, -1, ""),
        (["-d", lst, "-n", "7"], 64, None, "Usage: db_shrink"),
        (["-d", kdb, "-o", out, "-I", out_idx, "-n", "7"], 64, -1, ""),
        (["-d", kdb, "-i", str(tmp_path / "type1.idx"), "-o", out, "-I", out_idx, "-n", "7"], 64, -1, "db_sort"),
        (["-d", lst, "-i", idx, "-o", out, "-I", out_idx, "-n", "7"], 65, -2, "not the index of this database"),
        (["-d", str(tmp_path / "short.jdb"), "-o", out, "-n", "7"], 65, -2, "truncated"),
        (["-d", str(tmp_path / "magic.jdb"), "-o", out, "-n", "7"], 65, -2, "not Jellyfish v1 database"),
        (["-d", lst, "-o", str(tmp_path / "link.jdb"), "-n", "7"], 64, -1, "is the input"),
        (["-d", lst, "-o", out, "-n", "7", "-s", "65535"], 64, -1, "below the minimum"),
    ]
    codes = dict(ln.split() for ln in open(os.path.join(GOLD, "reference_exit_codes.txt")))
    assert [int(codes[n]) for n in ("n_above_key_ct", "O_above_block_size", "n_0", "O_0", "missing_o")] == [cases[i][1] for i in (0, 1, 4, 5, 6)]
    for args, code, status, text in cases:
        r = _cli(args)
        assert r.returncode == code and text.encode() in r.stderr, (args, r.returncode, r.stderr)
        assert os.listdir(work) == [], args
        if status is None:
            continue
        opt = {args[i]: args[i + 1] for i in range(0, len(args), 2)}
        with pytest.raises(capi.KuError) as e:
            capi.db_shrink_files(opt["-d"], opt["-o"], int(opt["-n"]), int(opt.get("-O", 1)), in_idx=opt.get("-i"), out_idx=opt.get("-I"),
                                 device_bytes=int(opt.get("-s", SMALL)))
        assert e.value.status == status and text in str(e.value), args
        assert os.listdir(work) == [], args
    assert _bytes(lst) == img and _bytes(idx) == ix
    r = _cli(["-h"])
    assert r.returncode == 0 and r.stderr.startswith(b"Usage: db_shrink")
    # an index whose offsets leave the database is found on the device: the outputs it had created are gone
    bad = np.frombuffer(ix[8:], dtype="<u8").copy()
    bad[5] = KEY_CT + 1
    (tmp_path / "bad.idx").write_bytes(ix[:8] + bad.tobytes())
    with pytest.raises(capi.KuError) as e:
        capi.db_shrink_files(kdb, out, 7, 1, in_idx=str(tmp_path / "bad.idx"), out_idx=out_idx, device_bytes=SMALL)
    assert e.value.status == -2 and os.listdir(work) == []


@pytest.mark.gpu
def test_device_index_out_of_range(tmp_path):
    for device in (-1, capi.lib().ku_device_count()):
        with pytest.raises(capi.KuError) as e:
            capi.db_shrink_files(os.path.join(GOLD, "list1000.jdb"), str(tmp_path / "out.jdb"), 7, device=device)
        assert e.value.status == -1 and "device index out of range" in str(e.value)
        assert os.listdir(tmp_path) == []
