"""The numpy model of db_shrink that tests/test_db_shrink_host.py certifies against the reference's files
(tests/golden/db_shrink) and tests/test_db_shrink.py holds the GPU tool to: the rule as Python integers (src, S), the list
writer and reader for any key length, the shrunk list and the shrunk database's index, and the inputs of the golden files."""
import numpy as np

FIXTURES = {  # name -> (k, records, the (n, O) pairs the reference was run with)
    "list1000": (31, 1000, [(7, 1), (7, 3), (1000, 1), (1, 1000), (300, 2)]),
    "list37_k27": (27, 37, [(5, 1), (5, 7), (37, 1)]),
}


# --------------------------------------------------------------------------- the rule
def rule_ok(key_ct, n, O):
    return 1 <= n <= key_ct and 1 <= O <= key_ct // n


def src(key_ct, n, O, j):
    """the input record that output record j is: blocks of bs records, the first `odd` of them one longer, the record O places
    before the end of block j"""
    bs, odd = divmod(key_ct, n)
    return (j + 1) * bs + min(j + 1, odd) - O


def S(key_ct, n, O, x):
    """#{ j : src(j) < x }, in closed form"""
    bs, odd = divmod(key_ct, n)
    t = x + O - 1
    return min(odd, t // (bs + 1)) + (min(max((t - odd) // bs - odd, 0), n - odd) if t >= odd else 0)


def all_src(key_ct, n, O):
    bs, odd = divmod(key_ct, n)
    m = np.arange(1, n + 1, dtype=np.int64)
    return m * bs + np.minimum(m, odd) - O


def S_of(key_ct, n, O, x):
    """S over an array of indices, by counting: independent of the closed form"""
    return np.searchsorted(all_src(key_ct, n, O), np.asarray(x, dtype=np.int64), side="left")


# --------------------------------------------------------------------------- lists of any key length
def header_size(k):
    return 72 + 2 * (4 + 8 * 2 * k)


def list_header(k, key_ct):
    h = bytearray(header_size(k))
    h[0:8] = b"JFLISTDN"
    h[8:16] = (2 * k).to_bytes(8, "little")
    h[16:24] = (4).to_bytes(8, "little")
    h[48:56] = int(key_ct).to_bytes(8, "little")
    return bytes(h)


def pack_records(kmers, vals, k):
    """key_len = ceil(2k / 8) little-endian key bytes + 4 value bytes per record"""
    key_len = (2 * k + 7) // 8
    rec = np.zeros((len(kmers), key_len + 4), dtype=np.uint8)
    rec[:, :key_len] = np.asarray(kmers, dtype="<u8").view(np.uint8).reshape(-1, 8)[:, :key_len]
    rec[:, key_len:] = np.asarray(vals, dtype="<u4").view(np.uint8).reshape(-1, 4)
    return rec


def write_list(path, kmers, vals, k):
    with open(path, "wb") as f:
        f.write(list_header(k, len(kmers)))
        f.write(pack_records(kmers, vals, k).tobytes())


def read_list(path):
    """(header bytes, records as a (key_ct, key_len + 4) byte array)"""
    raw = np.fromfile(path, dtype=np.uint8)
    assert raw[:8].tobytes() == b"JFLISTDN"
    key_bits = int.from_bytes(raw[8:16].tobytes(), "little")
    key_ct = int.from_bytes(raw[48:56].tobytes(), "little")
    hdr, ps = 72 + 2 * (4 + 8 * key_bits), (key_bits + 7) // 8 + 4
    return raw[:hdr].tobytes(), raw[hdr:hdr + key_ct * ps].reshape(key_ct, ps)


# --------------------------------------------------------------------------- the model
def shrink_list_bytes(path, n, O):
    """the file db_shrink -n n -O O writes from the list at `path`: its header with n at byte 48, the records src(0 .. n - 1)"""
    hdr, rec = read_list(path)
    assert rule_ok(len(rec), n, O)
    return hdr[:48] + int(n).to_bytes(8, "little") + hdr[56:] + rec[all_src(len(rec), n, O)].tobytes()


def shrink_index_bytes(idx_path, key_ct, n, O):
    """the index of the shrunk database: new_off[b] = S(old_off[b]), the closing offset n"""
    raw = np.fromfile(idx_path, dtype=np.uint8)
    assert raw[:7].tobytes() == b"KRAKIX2"
    off = raw[8:].view("<u8")
    assert int(off[-1]) == key_ct
    new = S_of(key_ct, n, O, off.astype(np.int64)).astype("<u8")
    assert int(new[-1]) == n
    return raw[:8].tobytes() + new.tobytes()


def write_model(kdb, idx, n, O, out_kdb, out_idx=None):
    """the model's files: the shrunk list, and with out_idx the shrunk database's index next to it"""
    with open(out_kdb, "wb") as f:
        f.write(shrink_list_bytes(kdb, n, O))
    if out_idx is not None:
        with open(out_idx, "wb") as f:
            f.write(shrink_index_bytes(idx, len(read_list(kdb)[1]), n, O))
    return (out_kdb, out_idx) if out_idx is not None else out_kdb


# --------------------------------------------------------------------------- the inputs of the golden files
def fixture_input(name):
    """(kmers, vals, k) of a golden input list: unsorted k-mers below 4^k, values up to 2^32 - 1"""
    k, n, _ = FIXTURES[name]
    rng = np.random.default_rng({"list1000": 1000, "list37_k27": 37}[name])
    kmers = rng.integers(0, 1 << (2 * k), n, dtype=np.uint64)
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return kmers, vals, k
