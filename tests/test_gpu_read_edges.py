"""-m gpu: the read-level edges of the fused classify kernel (ku_short.hip) against the oracle.

Stage 1 of the kernel decides once per read, in scalar code, whether the read and the two aligned dwords that cover any
four of its bytes lie inside the sequence buffer; every read but the batch's last few then fetches two dwords per lane from
the read's aligned base, and the ones at the buffer's end go byte by byte.  Every lane stores its quad's code word, and
every lane a sentinel behind the read's last m-mer.  The edges that code owns, at the smallest shapes that reach them:
  buffer end    the last read ends 0 .. 8 bytes in front of n_bytes, at each alignment of its offset mod 4 -- a read of
                100 bases, one shorter than k, an empty one, one of exactly k bases
  word count    read lengths on, one in front of and one behind a 16-base word boundary; 158 bases (the longest read of the
                two-items instance) and 222 (of the three-items instance); a windowed read whose last window is one k-mer
  sentinels     reads of exactly 128 and 192 k-mers (the m-mer array at its fullest); a low-complexity read, which takes
                the exact scan of the tie path, behind a plain one in the same wave, and the other way round
  launch shape  1 read, 3 reads, one read more than the grid has waves: waves with none, one and two reads
Every batch goes through ku_classify_batch_device (codes, with accounting), ku_classify_batch_device_rle (runs) and, with the
sparse-sketch emulation on, ku_classify_batch_rle; calls, per-k-mer codes (or the expanded runs) and the per-taxon state are
the oracle's.  The database is the g13 geometry of tests/kernel_instances.py: k = 31, nt = 13, twelve random genomes."""
import numpy as np
import pytest

from krakenuniq_amd import capi, synth
from oracle import ku_oracle as ko
import gpu_common as gc
from test_gpu_sparse import assert_sparse_state_equals_oracle

pytestmark = pytest.mark.gpu
K, NT = 31, 13
UNIT = 20000  # work unit of the sparse-sketch emulation (nt)

_w = {}


def world():
    """database, context and oracle handles: built once, never changed"""
    if not _w:
        import torch
        rng = np.random.default_rng(1313)
        db = gc.random_db(rng, n_genomes=12, glen=6000, k=K, nt=NT)
        ids, par = db["tax"].arrays()
        raw = db["pairs"].view(np.uint8)
        ctx, _, _ = gc.make_ctx(cdb=capi.Db(pairs=raw, key_ct=len(db["kmers"]), k=K, offsets=db["offsets"], nt=NT),
                                ctax=capi.Tax(ids=ids, parents=par))
        assert ctx.db_layout()["hash"]
        _w.update(torch=torch, dev=torch.device("cuda:0"), ctx=ctx, raw=raw,
                  odb=ko.Db(pairs=raw, key_ct=len(db["kmers"]), k=K, offsets=db["offsets"], nt=NT), otax=ko.Tax(ids=ids, parents=par),
                  genomes=[synth.codes_to_ascii(g) for g in db["genomes"].values()],
                  n_cu=torch.cuda.get_device_properties(0).multi_processor_count)
    return _w


@pytest.fixture(scope="module", autouse=True)
def release_everything():
    yield
    if _w:
        _w["ctx"].close()
    _w.clear()


# ---- reads
def frag(rng, length, sub=False):
    """`length` bases of a genome; sub: one substitution in the middle (the k-mers over it miss, the others hit)"""
    g = world()["genomes"]
    src = g[int(rng.integers(0, len(g)))]
    s = int(rng.integers(0, len(src) - length + 1))
    text = bytearray(src[s:s + length])
    if sub and length:
        p = length // 2
        text[p] = ord("ACGT"[("ACGT".index(chr(text[p])) + 1 + int(rng.integers(0, 3))) % 4])
    return bytes(text)


def low_complexity(rng, length):
    """a short motif over and over: equal m-mers at several positions of every window, the kernel's tie path"""
    motif = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(2, 8))))
    return (motif * (length // len(motif) + 1))[:length]


def layout(reads, last_mod4=None, tail=1):
    """the batch's buffer: one 'N' behind every read but the last, `tail` of them behind that one (n_bytes = its end + tail),
    and its offset moved to last_mod4 (mod 4) by further 'N's in front of it"""
    parts, off, pos = [], [], 0
    for i, r in enumerate(reads):
        if i == len(reads) - 1 and last_mod4 is not None:
            pad = (last_mod4 - pos) % 4
            parts.append(b"N" * pad)
            pos += pad
        off.append(pos)
        parts.append(r)
        pos += len(r)
        if i < len(reads) - 1:
            parts.append(b"N")
            pos += 1
    parts.append(b"N" * tail)
    buf = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    off = np.array(off, dtype=np.uint64)
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    assert len(buf) == int(off[-1]) + int(lens[-1]) + tail and (last_mod4 is None or int(off[-1]) % 4 == last_mod4)
    return buf, off, lens


# ---- the oracle's side
def oracle_batch(buf, off, lens, unit=None):
    w = world()
    run = ko.Run(w["odb"], w["otax"], **({} if unit is None else {"work_unit_nt": unit}))
    res = run.classify_packed(buf, off, lens)
    codes = []
    for i in range(len(lens)):
        a, n = int(res["taxa_off"][i]), int(res["n_slots"][i])
        assert n == max(int(lens[i]) - K + 1, 0)
        c = res["taxa"][a:a + n].copy()
        c[res["ambig"][a:a + n] != 0] = capi.KU_AMBIG
        codes.append(c)
    # no batch passes vacuously: the oracle saw a k-mer of the database and one that is not in it
    flat = np.concatenate(codes)
    assert np.any((flat != 0) & (flat != capi.KU_AMBIG)) and np.any(flat == 0), "the batch needs a hit and a miss"
    return run, res["calls"].copy(), codes


def assert_reads(calls, codes, want_calls, want_codes):
    assert (calls == want_calls).all(), np.nonzero(calls != want_calls)[0][:10]
    for i, (c, wc) in enumerate(zip(codes, want_codes)):
        assert len(c) == len(wc) and (c == wc).all(), (i, len(wc), np.nonzero(c != wc)[0][:10])


def expand_runs(runs, run_off, run_cnt, lens):
    out = []
    for i, l in enumerate(lens.tolist()):
        n = max(l - K + 1, 0)
        a, c = int(run_off[i]), int(run_cnt[i])
        rr = runs[a:a + c]
        assert (c == 0) == (n == 0), i
        if c:
            assert rr[0, 1] == 0 and np.all(np.diff(rr[:, 1].astype(np.int64)) > 0) and rr[-1, 1] < n, i
            assert np.all(rr[1:, 0] != rr[:-1, 0]), i  # maximal runs
            out.append(np.repeat(rr[:, 0], np.diff(np.r_[rr[:, 1], n])))
        else:
            out.append(np.zeros(0, dtype=np.uint32))
    return out


# ---- the device's side
def upload(buf, off, lens):
    w = world()
    torch, dev = w["torch"], w["dev"]
    return (torch.from_numpy(buf).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
            torch.from_numpy(lens.astype(np.int32)).to(dev))


def device_codes(buf, off, lens):
    w = world()
    torch, dev, ctx = w["torch"], w["dev"], w["ctx"]
    d_seqs, d_off, d_len = upload(buf, off, lens)
    n = len(lens)
    taxa = torch.zeros(len(buf), dtype=torch.int32, device=dev)
    calls = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (torch works on its stream, the library on the context's own)
    ctx.classify_batch_device(d_seqs.data_ptr(), len(buf), d_off.data_ptr(), d_len.data_ptr(), n, calls.data_ptr(), taxa.data_ptr(),
                              max_read_len=int(lens.max()))
    ctx.synchronize()
    taxa = taxa.cpu().numpy().view(np.uint32)
    return calls.cpu().numpy().view(np.uint32), [taxa[int(o):int(o) + max(int(l) - K + 1, 0)] for o, l in zip(off.tolist(), lens.tolist())]


def device_runs(buf, off, lens):
    w = world()
    torch, dev, ctx = w["torch"], w["dev"], w["ctx"]
    d_seqs, d_off, d_len = upload(buf, off, lens)
    n, longest = len(lens), int(lens.max())
    cap = ctx.device_rle_runs_cap(len(buf), n, longest)
    runs = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
    roff = torch.zeros(n, dtype=torch.int64, device=dev)
    rcnt = torch.zeros(n, dtype=torch.int32, device=dev)
    nruns = torch.zeros(1, dtype=torch.int64, device=dev)
    calls = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.classify_batch_device_rle(d_seqs.data_ptr(), len(buf), d_off.data_ptr(), d_len.data_ptr(), n, calls.data_ptr(), runs.data_ptr(), cap,
                                  roff.data_ptr(), rcnt.data_ptr(), nruns.data_ptr(), max_read_len=longest)
    ctx.synchronize()
    assert int(nruns.item()) <= cap
    return calls.cpu().numpy().view(np.uint32), expand_runs(runs.cpu().numpy().view(np.uint32), roff.cpu().numpy(), rcnt.cpu().numpy(), lens)


def check(batches):
    """every batch (buf, off, lens) in the three forms; the context's state is the one batch's each time"""
    ctx = world()["ctx"]
    ctx.disable_sparse()
    for buf, off, lens in batches:
        run, want_calls, want_codes = oracle_batch(buf, off, lens)
        for form in (device_codes, device_runs):
            ctx.reset_counts()
            calls, codes = form(buf, off, lens)
            assert_reads(calls, codes, want_calls, want_codes)
            gc.assert_same_counts(ctx.counts(), run)
    ctx.enable_sparse(UNIT, 20)
    try:
        for buf, off, lens in batches:
            run, want_calls, want_codes = oracle_batch(buf, off, lens, UNIT)
            ctx.reset_counts()
            rle = ctx.classify_batch_rle(buf, off, lens)
            assert_reads(rle["calls"], expand_runs(rle["runs"], rle["run_off"], rle["run_cnt"], lens), want_calls, want_codes)
            counts, *_ = assert_sparse_state_equals_oracle(ctx, run)
            gc.assert_same_counts(counts, run)
    finally:
        ctx.disable_sparse()
        ctx.reset_counts()


# ---- buffer end
LAST = {"plain": lambda rng: frag(rng, 100, sub=True), "shorter_than_k": lambda rng: frag(rng, 17), "empty": lambda rng: b"",
        "exactly_k": lambda rng: frag(rng, K)}


@pytest.mark.parametrize("last", list(LAST))
def test_last_read_at_the_end_of_the_buffer(last):
    """the last read ends 0 .. 8 bytes in front of n_bytes, its offset at every alignment mod 4"""
    rng = np.random.default_rng(41)
    batches = []
    for tail in range(9):
        for mod4 in range(4):
            reads = [frag(rng, 100, sub=True), frag(rng, int(rng.integers(K, 150))), LAST[last](rng)]
            batches.append(layout(reads, last_mod4=mod4, tail=tail))
    check(batches)


# ---- stage 1's word count, the fullest m-mer array
def test_read_lengths_around_the_word_boundaries_two_items():
    """lengths 16 w - 1, 16 w, 16 w + 1, and 158 bases = 128 k-mers, the longest read of the two-items instance"""
    rng = np.random.default_rng(42)
    lengths = [l for w in (2, 3, 4, 5, 6, 7, 8, 9) for l in (16 * w - 1, 16 * w, 16 * w + 1)] + [157, 158]
    assert max(lengths) - K + 1 == 128
    reads = [frag(rng, 100, sub=True)] + [frag(rng, l, sub=bool(i & 1)) for i, l in enumerate(lengths)]
    check([layout(reads), layout(reads[::-1], tail=0)])


def test_read_lengths_around_the_word_boundaries_three_items():
    """the same up to 222 bases = 192 k-mers, the longest read of the three-items instance"""
    rng = np.random.default_rng(43)
    lengths = [l for w in (10, 11, 12, 13) for l in (16 * w - 1, 16 * w, 16 * w + 1)] + [159, 221, 222]
    assert max(lengths) - K + 1 == 192
    reads = [frag(rng, 100, sub=True)] + [frag(rng, l, sub=bool(i & 1)) for i, l in enumerate(lengths)]
    check([layout(reads), layout(reads[::-1], tail=0)])


def test_windowed_read_whose_last_window_is_one_kmer():
    """2 x 128 + 1 k-mers: two full windows and one of a single k-mer (31 bases, the buffer's last)"""
    rng = np.random.default_rng(44)
    reads = [frag(rng, 100, sub=True), frag(rng, 2 * 128 + 1 + K - 1, sub=True)]
    check([layout(reads, tail=t) for t in (0, 1, 5)])


# ---- sentinels and the tie path
def test_plain_and_low_complexity_reads_alternate_in_a_wave():
    """two reads per wave: a low-complexity one (exact scan of the tie path) behind a plain one in the even waves, the other way
    round in the odd ones; reads of 128 k-mers among them"""
    w = world()
    rng = np.random.default_rng(45)
    n_waves = w["n_cu"] * 6 * 4  # (ku_short_grid_waves: two k-mers per lane, < 500 k reads: 6 blocks of 4 waves per CU)
    plain = [frag(rng, l, sub=True) for l in (158, 100, 64, 150)]
    lowc = [low_complexity(rng, l) for l in (158, 100, 65, 150)] + [frag(rng, 60) + low_complexity(rng, 98)]
    reads = []
    for r in range(2 * n_waves):
        tie_turn = ((r % n_waves) & 1) == (r // n_waves)
        reads.append(lowc[r % len(lowc)] if tie_turn else plain[r % len(plain)])
    check([layout(reads)])


def test_low_complexity_reads_of_the_three_items_instance():
    """reads of 192 k-mers, plain and low-complexity, in both orders"""
    rng = np.random.default_rng(46)
    reads = [frag(rng, 222, sub=True), low_complexity(rng, 222), frag(rng, 222), frag(rng, 100) + low_complexity(rng, 122)]
    check([layout(reads), layout(reads[::-1])])


# ---- launch shape
@pytest.mark.parametrize("shape", ["one", "three", "grid_plus_one"])
def test_waves_with_none_one_and_two_reads(shape):
    w = world()
    rng = np.random.default_rng(47)
    n = {"one": 1, "three": 3, "grid_plus_one": w["n_cu"] * 6 * 4 + 1}[shape]
    reads = [frag(rng, int(rng.integers(K + 40, 159)), sub=True) for _ in range(min(n, 64))]
    reads = [reads[i % len(reads)] for i in range(n)]
    check([layout(reads, tail=0), layout(reads, last_mod4=3, tail=2)])
