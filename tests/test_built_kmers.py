"""tests/built_kmers.py against the oracle alone (no GPU): what the builders promise is what tests/test_gpu_hash_edges.py
relies on, so none of its cases passes for a k-mer that is not the one it was meant to be.

Where a rank leaves one hash per register (53, 52: see built_kmers) not every register has a canonical 31-mer: of the registers
{0, 7, 4095} x ranks {52, 53} only (7, 53) and (4095, 52) do.  The others are not skipped: the test goes through every hash
the case allows and asserts, with the oracle's own revcomp, that none is a canonical 31-mer's, and then takes the rank at the
next register that has one."""
import numpy as np
import pytest

import built_kmers as bk
from oracle import ku_oracle as ko

K = 31
RANKS = (1, 13, 14, 40, 41, 52, 53)
INDICES = (0, 7, 4095)
ADDS = (1, 2, 13, 26, 27, 39, 40)


def oracle_is_canonical_kmer(v):
    return v < 4 ** K and ko.lib().ko_canonical(v, K) == v and v <= ko.lib().ko_revcomp(v, K)


def check_kmer(h, v):
    assert ko.lib().ko_hash(v) == h and oracle_is_canonical_kmer(v), (hex(h), hex(v))
    # ... and it is the k-mer the oracle's scanner makes of the text, on either strand
    for flip in (False, True):
        text = bk.ascii_of(v, flip)
        fwd, amb = ko.scan(text, K)
        assert len(text) == K and not amb.any() and ko.lib().ko_canonical(int(fwd[0]), K) == v


def hashes_of_rank(idx, rank):
    """every hash with register idx and the rank: 2^(52 - rank) of them (rank 53: one)"""
    if rank == 53:
        return [idx << 52]
    return [(idx << 52) | (1 << (52 - rank)) | low for low in range(1 << (52 - rank))]


def hashes_of_add(top12, add):
    if add == 40:
        return [top12 << 52]
    return [(top12 << 52) | (1 << (39 - add)) | low for low in range(1 << (39 - add))]


def test_unmix_and_the_python_restatements():
    rng = np.random.default_rng(1)
    for h in [0, bk.M64, 1, 1 << 63] + rng.integers(0, 1 << 64, 200, dtype=np.uint64).tolist():
        v = bk.unmix(h)
        assert ko.lib().ko_hash(v) == h
        assert bk.revcomp(v >> 2) == ko.lib().ko_revcomp(v >> 2, K)
        d, s = ko.Hll(12, False), ko.Hll(12, True)
        d.insert(v)
        s.insert(v)
        assert int(d.registers()[h >> 52]) == bk.dense_rank(h) and s.sparse_list().tolist() == [bk.encoding(h)]


def test_build_honours_the_mask_and_says_when_there_is_no_kmer():
    rng = np.random.default_rng(2)
    mask, val = 0xF0F0F0F0F0F0F0F0, 0xA050A050A050A050
    seen = set()
    for _ in range(50):
        h, v = bk.build(mask, val, rng)
        assert h & mask == val
        check_kmer(h, v)
        seen.add(h)
    assert len(seen) == 50  # (the free bits are drawn)
    with pytest.raises(bk.NoKmer):  # hash 0 is the hash of 2^64 - 1
        bk.build(bk.M64, 0, rng)
    h, v = bk.build(bk.M64, 7 << 52, rng)
    assert h == 7 << 52
    check_kmer(h, v)


@pytest.mark.parametrize("idx", INDICES)
def test_dense_registers_hold_the_requested_rank(idx):
    rng = np.random.default_rng(100 + idx)
    for rank in RANKS:
        try:
            h, v = bk.dense(idx, rank, rng)
            at = idx
        except bk.NoKmer:
            assert rank >= 52, (idx, rank)  # (from 2 hashes per register on a register without any is chance, not arithmetic)
            assert not any(oracle_is_canonical_kmer(bk.unmix(x)) for x in hashes_of_rank(idx, rank))
            h, v, at = bk.first_dense(idx, rank, rng)
            assert at != idx
        check_kmer(h, v)
        assert h >> 52 == at and bk.dense_rank(h) == rank
        sk = ko.Hll(12, False)
        sk.insert(v)
        regs = sk.registers()
        assert int(regs[at]) == rank and np.count_nonzero(regs) == 1, (idx, rank)


def test_every_rank_is_held_at_one_of_the_indices_itself():
    """(what the NoKmer branch above leaves: ranks 52 and 53 are reached at 4095 and at 7)"""
    rng = np.random.default_rng(3)
    for rank in RANKS:
        held = []
        for idx in INDICES:
            try:
                bk.dense(idx, rank, rng)
                held.append(idx)
            except bk.NoKmer:
                pass
        assert held if rank >= 52 else held == list(INDICES), rank
    assert bk.dense(7, 53, rng)[0] == 7 << 52 and bk.dense(4095, 52, rng)[0] == (4095 << 52) | 1


@pytest.mark.parametrize("top12", INDICES)
def test_flagged_encodings_hold_the_flag_and_add(top12):
    rng = np.random.default_rng(200 + top12)
    for add in ADDS:
        try:
            h, v = bk.flagged(top12, add, rng)
            at = top12
        except bk.NoKmer:
            assert add >= 39, (top12, add)
            assert not any(oracle_is_canonical_kmer(bk.unmix(x)) for x in hashes_of_add(top12, add))
            h, v, at = bk.first_flagged(top12, add, rng)
            assert at != top12
        check_kmer(h, v)
        sk = ko.Hll(12, True)
        sk.insert(v)
        assert sk.is_sparse
        enc = sk.sparse_list().tolist()
        assert enc == [(at << 20) | (add << 1) | 1] == [bk.encoding(h)], (top12, add)
        regs = sk.registers()  # the dense view of the same k-mer
        assert int(regs[at]) == 13 + add and np.count_nonzero(regs) == 1
        dn = ko.Hll(12, False)
        dn.insert(v)
        assert np.array_equal(dn.registers(), regs)


def test_plain_encodings_twins_and_their_ranks():
    rng = np.random.default_rng(4)
    for top12 in INDICES:
        for r in (1, 2, 12, 13):  # rank of the 13 index bits behind top12
            low13 = (1 << (13 - r)) | (int(rng.integers(0, 1 << 13)) & ((1 << (13 - r)) - 1))
            top25 = (top12 << 13) | low13
            (h1, v1), (h2, v2) = bk.plain(top25, rng), bk.plain(top25, rng)
            assert v1 != v2 and h1 >> 39 == h2 >> 39 == top25
            check_kmer(h1, v1)
            check_kmer(h2, v2)
            sk = ko.Hll(12, True)
            sk.insert(v1)
            sk.insert(v2)
            assert sk.sparse_list().tolist() == [top25 << 7] and sk.n_observed == 2  # two k-mers, one encoding, no flag
            assert int(sk.registers()[top12]) == r
    with pytest.raises(AssertionError):
        bk.plain(5 << 13, rng)  # (13 zeros behind the register index: that encoding is a flagged one)


def test_reads_book_exactly_their_kmers():
    rng = np.random.default_rng(5)
    kmers = [bk.dense(int(rng.integers(0, 4096)), 1 + i % 40, rng)[1] for i in range(19)]
    for per, length in ((1, 31), (4, 127), (5, 159), (8, 255)):
        reads = bk.reads_of(kmers, per)
        assert len(reads) == -(-len(kmers) // per) and all(len(r) == length for r in reads[:-1])
        got = []
        for r in reads:
            fwd, amb = ko.scan(r, K)
            assert int((amb == 0).sum()) == (len(r) + 1) // 32
            got += [ko.lib().ko_canonical(int(x), K) for x in fwd[amb == 0]]
        assert got == kmers  # in order, either strand
        assert reads[0][:K] == bk.ascii_of(kmers[0]) and (per == 1 or reads[0][K + 1:2 * K + 1] == bk.ascii_of(kmers[1], True))
