"""The one writer of a database.kdb + database.idx pair (csrc/ku_dbfiles.h) without a device: bin/dbfiles_check runs its
cases -- a complete run, an abandoned one, an index path that is a directory, a write that fails, finish() after that --
inside a directory of the test's and prints one line per case; the complete run's files are compared with the model's."""
import os
import subprocess

import numpy as np

from krakenuniq_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krakenuniq_amd", "bin", "dbfiles_check")
CASES = ["complete", "abandoned", "index_is_a_directory", "write_fails", "finish_after_failure"]


def test_the_writer_cases(tmp_path):
    assert os.path.exists(BIN), "build with make -C krakenuniq_amd/csrc"
    d = tmp_path / "out"
    d.mkdir()
    r = subprocess.run([BIN, str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.stdout.decode().splitlines() == [f"{c} ok" for c in CASES], r.stdout.decode() + r.stderr.decode()
    assert r.returncode == 0
    # what is left: the complete run's pair, and the directory that stood in the index's way
    assert sorted(os.listdir(d)) == ["complete.idx", "complete.kdb", "is_a_directory.idx"] and os.path.isdir(d / "is_a_directory.idx")
    # the complete run, byte for byte: nt = 2, k = 31, thirteen records, one in each of the first thirteen bins
    k, nt, n = 31, 2, 13
    kmers = (np.uint64(0x0123456789ABCDEF) * np.arange(1, n + 1, dtype=np.uint64)) & np.uint64((1 << 2 * k) - 1)
    vals = np.arange(100, 100 + n, dtype=np.uint32)
    offsets = np.minimum(np.arange(4 ** nt + 1), n).astype(np.uint64)
    synth.write_db(str(tmp_path / "want"), kmers, vals, offsets, k, nt)
    for got, want in (("complete.kdb", "database.kdb"), ("complete.idx", "database.idx")):
        assert (d / got).read_bytes() == (tmp_path / "want" / want).read_bytes(), got


def test_usage_and_a_missing_directory(tmp_path):
    assert subprocess.run([BIN], stderr=subprocess.PIPE).returncode == 64
    r = subprocess.run([BIN, str(tmp_path / "no_such_dir")], stderr=subprocess.PIPE)
    assert r.returncode == 66 and not os.path.exists(tmp_path / "no_such_dir")
