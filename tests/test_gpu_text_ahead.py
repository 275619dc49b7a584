"""-m gpu: a wave's successive reads in the fused classify kernel (ku_short.hip) against the oracle.

The one-pass instance with two k-mers per lane requests the text of a wave's NEXT read -- two aligned dwords per lane --
inside the current read, behind the last loads that read waits for, and stage 1 of the next iteration takes it from
registers.  Whether a read's text was requested ahead is decided twice by the same scalar test (it has a k-mer, and it and the
dwords around it lie inside the buffer): once with the next read's length and offset, once with its own.  What that code owns
shows only where a wave runs several reads, so every batch here has 3 * n_waves + 3 reads at one block per CU
(KU_SHORT_BLOCKS_PER_CU=1): every wave runs three reads, three waves a fourth, and read r is followed on its wave by read
r + n_waves.  Each test first checks on the host that its batch really puts the pairs it names next to each other.
  lengths     0, k - 1 (no k-mer: nothing requested, nothing stale consumed), k, 140, 141 (the first length with the tail round
              of m-mer positions), 150, 158 (128 k-mers): every ordered pair of them on some wave, with short -> long -> short
              and a read without k-mers between two normal ones
  alignment   offsets of a read and of its successor at every combination mod 4 (separators of 1 .. 4 bytes)
  batch end   the buffer ends exactly behind the last read; the last one, two, three reads of the batch are the next read of a
              wave, and the last one with k-mers is not inside the buffer by the kernel's test: it is loaded in place, byte-wise
  N           in the first four bases, in the last four, in both: around the first dword of the successor's text
  222 bases   the same mix at three k-mers per lane, the instance that loads its text in place
Every batch goes through ku_classify_batch_device (codes) and ku_classify_batch_device_rle (runs); calls, per-k-mer codes,
n_kmers, n_reads and the HLL registers are the oracle's."""
import numpy as np
import pytest

from krakenuniq_amd import capi
import gpu_common as gc
import test_gpu_read_edges as edges

pytestmark = pytest.mark.gpu
K = edges.K
LENGTHS = (0, K - 1, K, 140, 141, 150, 158)


@pytest.fixture(scope="module", autouse=True)
def one_block_per_cu_and_release():
    mp = pytest.MonkeyPatch()
    mp.setenv("KU_SHORT_BLOCKS_PER_CU", "1")
    yield
    mp.undo()
    if edges._w:
        edges._w["ctx"].close()
    edges._w.clear()


def n_waves():
    return edges.world()["n_cu"] * 4  # one block of four waves per CU


def pack(reads, seps, tail=0, lead=0):
    """this file's buffer: `lead` 'N's, then every read followed by seps[i] 'N's (the last one by `tail`); n_bytes is the end
    of that -- the device allocation is exactly as long (edges.upload: torch.from_numpy(buf).to(dev))"""
    parts, off, pos = [b"N" * lead], [], lead
    for i, r in enumerate(reads):
        off.append(pos)
        gap = tail if i == len(reads) - 1 else int(seps[i])
        parts += [r, b"N" * gap]
        pos += len(r) + gap
    buf = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    assert len(buf) == pos
    return buf, np.array(off, dtype=np.uint64), np.array([len(r) for r in reads], dtype=np.uint32)


def text_inside(off, lens, n_bytes):
    """the kernel's test for "requested ahead / fetched as two dwords per lane": the read and the aligned dwords around it"""
    return off.astype(np.int64) + lens.astype(np.int64) + 6 < n_bytes


def successors(values):
    """(value of read r, value of the read behind it on its wave) for every read that has one"""
    s = n_waves()
    return set(zip(values[:-s], values[s:]))


def check(batches):
    ctx = edges.world()["ctx"]
    ctx.disable_sparse()
    for buf, off, lens in batches:
        assert len(lens) > 3 * n_waves()
        run, want_calls, want_codes = edges.oracle_batch(buf, off, lens)
        for form in (edges.device_codes, edges.device_runs):
            ctx.reset_counts()
            calls, codes = form(buf, off, lens)
            edges.assert_reads(calls, codes, want_calls, want_codes)
            gc.assert_same_counts(ctx.counts(), run)
    ctx.reset_counts()


def pool(rng, lengths, each=8):
    """a few reads of every length: whole fragments (one taxon) and ones with a substitution (misses among the hits)"""
    return {l: [edges.frag(rng, l, sub=bool(i & 1)) for i in range(each)] for l in lengths}


def mixed_lengths(rng, lengths):
    """wave i runs lengths a, b, a (, a) for the i-th ordered pair (a, b): every ordered pair is a (read, successor)"""
    s, p = n_waves(), pool(rng, lengths)
    m = len(lengths)
    assert s >= m * m
    lens = []
    for r in range(3 * s + 3):
        a, b = divmod((r % s) % (m * m), m)
        lens.append(lengths[b] if r // s == 1 else lengths[a])
    reads = [p[l][r % len(p[l])] for r, l in enumerate(lens)]
    got = successors(lens)
    assert got >= {(a, b) for a in lengths for b in lengths}, "a pair of lengths is next to each other on no wave"
    triples = set(zip(lens[:-2 * s], lens[s:-s], lens[2 * s:]))
    return reads, triples


def test_every_pair_of_lengths_on_one_wave():
    rng = np.random.default_rng(71)
    reads, triples = mixed_lengths(rng, LENGTHS)
    assert (K, 158, K) in triples and (140, 158, 140) in triples  # short -> long -> short
    assert (150, K - 1, 150) in triples and (158, 0, 158) in triples  # no k-mer between two normal reads
    check([pack(reads, rng.integers(1, 5, len(reads)), tail=1), pack(reads[::-1], np.ones(len(reads)), tail=0)])


def test_offsets_of_a_read_and_its_successor_at_every_alignment():
    rng = np.random.default_rng(72)
    n = 3 * n_waves() + 3
    p = pool(rng, (97, 98, 99, 100, 141, 150))
    lens = rng.choice(list(p), n)
    reads = [p[int(l)][r % 8] for r, l in enumerate(lens)]
    buf, off, ln = pack(reads, rng.integers(1, 5, n), tail=3)
    assert successors((off % 4).tolist()) == {(a, b) for a in range(4) for b in range(4)}
    assert text_inside(off, ln, len(buf))[:-1].all()
    check([(buf, off, ln)])


@pytest.mark.parametrize("outside", [1, 2, 3])
def test_the_last_reads_of_the_batch_are_a_waves_next_read(outside):
    """`outside` reads at the buffer's end fail the kernel's inside test: the last one that has k-mers, and behind it an empty
    read and a one-base read (outside = 2, 3); every alignment of that read with k-mers"""
    rng = np.random.default_rng(73)
    s = n_waves()
    n = 3 * s + 3
    p = pool(rng, (100, 150))
    batches = []
    for mod4 in range(4):
        reads = [p[(100, 150)[r & 1]][r % 8] for r in range(n)]
        for i, t in enumerate((b"", b"A")[:outside - 1]):
            reads[n - 1 - i] = t
        last = n - outside  # the last read with k-mers
        buf, off, ln = pack(reads, np.ones(n), tail=0)
        buf, off, ln = pack(reads, np.ones(n), tail=0, lead=(mod4 - int(off[last])) % 4)
        assert int(off[last]) % 4 == mod4 and int(off[-1]) + int(ln[-1]) == len(buf)
        inside = text_inside(off, ln, len(buf))
        assert inside[:last].all() and not inside[last:].any() and ln[last] >= K
        assert last >= 3 * s and last - s >= 0  # it is the fourth read of a wave whose third one lies inside the buffer
        batches.append((buf, off, ln))
    check(batches)


def test_ambiguous_bases_at_both_ends_of_the_text():
    rng = np.random.default_rng(74)
    n = 3 * n_waves() + 3
    p = pool(rng, (100, 141, 150))

    def with_n(text, where):
        t = bytearray(text)
        for q in where:
            t[q] = ord("N")
        return bytes(t)

    marks = [(), (0,), (1,), (2,), (3,), (-1,), (-2,), (-3,), (-4,), (0, -1), (3, -4), (0, 1, 2, 3), (-4, -3, -2, -1)]
    kinds = [i % len(marks) for i in range(n)]
    kinds[n_waves():2 * n_waves()] = [(i * 5 + 3) % len(marks) for i in range(n_waves())]  # (another kind behind each kind)
    reads = [with_n(p[(100, 141, 150)[r % 3]][r % 8], marks[kd]) for r, kd in enumerate(kinds)]
    assert len(successors(kinds)) >= 2 * len(marks) and {a for a, _ in successors(kinds)} == set(range(len(marks)))
    check([pack(reads, rng.integers(1, 5, n), tail=2)])


def test_the_same_mix_at_three_kmers_per_lane():
    rng = np.random.default_rng(75)
    reads, _ = mixed_lengths(rng, LENGTHS + (222,))
    assert max(len(r) for r in reads) == 222
    check([pack(reads, rng.integers(1, 5, len(reads)), tail=0)])
