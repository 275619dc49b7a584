"""db_sort and set_lcas on records that are not three dwords: k = 21, key_len 6, so the record codec (ku_rec_load / ku_rec_store,
csrc/ku_kmerdb.h) goes byte by byte.  The expected files are the reference's own db_sort and set_lcas (oracle/_ref) over the
same shuffled Jellyfish-format list; database.kdb and database.idx byte for byte, with and without -z."""
import os
import subprocess

import numpy as np
import pytest

from krakenuniq_amd import synth
from test_kmer_db import _ref, _same_file, model_kmers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krakenuniq_amd", "bin")
K, NT, KEY_LEN = 21, 5, 6


def _run(args, **kw):
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)
    assert r.returncode == 0, " ".join(args) + "\n" + r.stderr.decode()


@pytest.mark.gpu
def test_db_sort_and_set_lcas_at_key_len_6(tmp_path):
    # two genomes of 2 000 bases under the sibling species 4 and 5 (genus 2); bases 600..1100 of the second are the first's,
    # so the k-mers of that stretch fold to the genus
    a = synth.procedural_genome(21, 4, 2000)
    b = synth.procedural_genome(21, 5, 2000)
    b[600:1100] = a[600:1100]
    recs = [synth.codes_to_ascii(a), synth.codes_to_ascii(b)]
    synth.write_fasta(str(tmp_path / "library.fa"), recs, ids=["seqA", "seqB"], width=60)
    (tmp_path / "seqid2taxid.map").write_text("seqA\t4\nseqB\t5\n")
    synth.small_taxonomy().write(str(tmp_path / "taxDB"))
    kmers = model_kmers(recs, K)
    n = len(kmers)
    assert (2 * K + 7) // 8 == KEY_LEN and 3400 < n < 3960
    # the list, written here: header, then per record six little-endian key bytes and four value bytes.  Every fifth value
    # is pre-set to species 6 (it takes part in the fold, and -z has something to zero)
    vals = np.zeros(n, dtype=np.uint32)
    vals[::5] = 6
    perm = np.random.default_rng(21).permutation(n)
    raw = np.concatenate([kmers[perm].astype("<u8").view(np.uint8).reshape(n, 8)[:, :KEY_LEN],
                          vals[perm].astype("<u4").view(np.uint8).reshape(n, 4)], axis=1)
    jdb = str(tmp_path / "in.jdb")
    with open(jdb, "wb") as f:
        f.write(synth.kdb_header(K, n))
        f.write(raw.tobytes())

    def p(name):
        return str(tmp_path / name)

    # (-M: without it the reference's set_lcas folds into the file -d names and copies that to -o)
    lcas = ["-M", "-x", "-t", "1", "-b", p("taxDB"), "-m", p("seqid2taxid.map"), "-F", p("library.fa")]
    for who, db_sort, set_lcas in (("ref", _ref("db_sort"), _ref("set_lcas")),
                                   ("got", os.path.join(BIN, "db_sort"), os.path.join(BIN, "set_lcas"))):
        _run([db_sort, "-t", "1", "-n", str(NT), "-d", jdb, "-o", p(f"{who}0.kdb"), "-i", p(f"{who}.idx")])
        _run([db_sort, "-z", "-t", "1", "-n", str(NT), "-d", jdb, "-o", p(f"{who}z.kdb"), "-i", p(f"{who}z.idx")])
        _run([set_lcas, "-d", p(f"{who}0.kdb"), "-i", p(f"{who}.idx"), "-o", p(f"{who}.kdb")] + lcas)
    for fn in ("0.kdb", ".idx", "z.kdb", "z.idx", ".kdb"):
        assert _same_file(p("got" + fn), p("ref" + fn)), fn
    # the case is what it claims to be: records of ten bytes; pre-set (lca(4 or 5, 6) = 1), folded (2) and plain values all
    # occur -- the shared stretch has 480 windows, four fifths of them not pre-set --; -z zeroed them
    hdr = len(synth.kdb_header(K, n))
    out = np.fromfile(p("got.kdb"), dtype=np.uint8)[hdr:].reshape(n, KEY_LEN + 4)
    got_vals = out[:, KEY_LEN:].copy().view("<u4").ravel()
    assert {1, 2, 4, 5} <= set(np.unique(got_vals).tolist()) and (got_vals == 2).sum() > 300
    assert not np.fromfile(p("gotz.kdb"), dtype=np.uint8)[hdr:].reshape(n, KEY_LEN + 4)[:, KEY_LEN:].any()
    assert np.fromfile(p("got0.kdb"), dtype=np.uint8)[hdr:].reshape(n, KEY_LEN + 4)[:, KEY_LEN:].any()
