"""-m gpu: the fused classify kernel (ku_short.hip) with its waves claiming their reads from a counter of the launch.

KU_SHORT_CLAIM=<chunk> makes every wave take `chunk` consecutive reads at a time: its first chunk is [w * chunk, (w + 1) * chunk),
every later one comes from an atomic add on the launch's cell, and a claim at or behind n_reads ends the wave's read loop.  Which
wave classifies a read enters no result, so every batch here must give, bit for bit, what the CPU oracle gives AND what the same
batch gives with KU_SHORT_CLAIM=0 (the static stride): calls, per-k-mer codes (as the array parallel to the reads and as runs,
expanded), n_kmers, n_reads and the HLL registers.  `calls` starts as 0xFFFFFFFF everywhere and holds none of it afterwards,
and n_reads sums to the number of reads: every read was classified exactly once.

All batches run at one block per CU (KU_SHORT_BLOCKS_PER_CU=1 beside the claim knob, which wins): about a thousand waves, so a
few thousand reads already give every wave several chunks.
  chunks and counts   chunk 1, 2, 3, 16; n below n_waves * chunk (the last waves' first chunk partial or empty), exactly that
                      (every later claim comes back past the end), one more, and several chunks per wave with a ragged end
  the batch's end     the last read ends on the buffer's final bytes (the text path that loads in place), once in the middle of
                      a chunk and once as a chunk's first read -- a plain read, one shorter than k, one that is all N, one
                      with N at both ends; the same kinds are spread over the batch as well
  instance families   tests/claim_child.py under the launch recorder of test_gpu_instances: OUT 0 / 1 / 2, KU_F_NO_COUNTS,
                      nt 13 / 15 and a generic (k, nt), three k-mers per lane, windows (2 x 150 + N, 1 kbp), each with the
                      instance it must have launched
  the cell            more launches than the ring has cells, back to back, alternating between two streams and through the
                      host-batch call two deep; a context asked to launch on more streams than the ring has cells refuses
The instances that have no room for the claim (ks_claim_instance) run the static stride whatever the knob says; they are
compared all the same."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from krakenuniq_amd import capi
import gpu_common as gc
import test_gpu_read_edges as edges
from test_gpu_text_ahead import pack

pytestmark = pytest.mark.gpu
K = edges.K
FILL = 0xFFFFFFFF
HERE = os.path.dirname(os.path.abspath(__file__))
CLAIM_CELLS = 32  # KU_CLAIM_CELLS, ku_internal.h


@pytest.fixture(scope="module", autouse=True)
def one_block_per_cu_and_release():
    mp = pytest.MonkeyPatch()
    mp.setenv("KU_SHORT_BLOCKS_PER_CU", "1")
    yield
    mp.undo()
    os.environ.pop("KU_SHORT_CLAIM", None)
    if edges._w:
        edges._w["ctx"].close()
    edges._w.clear()


def n_waves():
    return edges.world()["n_cu"] * 4  # one block of four waves per CU


# ---- the device's side: as test_gpu_read_edges, with `calls` pre-filled and an optional stream
def device_codes(ctx, buf, off, lens, flags=0, stream=None, wait=True):
    w = edges.world()
    torch, dev = w["torch"], w["dev"]
    d_seqs, d_off, d_len = edges.upload(buf, off, lens)
    n = len(lens)
    taxa = torch.zeros(len(buf), dtype=torch.int32, device=dev)
    calls = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.classify_batch_device(d_seqs.data_ptr(), len(buf), d_off.data_ptr(), d_len.data_ptr(), n, calls.data_ptr(), taxa.data_ptr(),
                              max_read_len=int(lens.max()), flags=flags, stream=stream)

    def fetch():
        t = taxa.cpu().numpy().view(np.uint32)
        return calls.cpu().numpy().view(np.uint32), [t[int(o):int(o) + max(int(l) - K + 1, 0)] for o, l in zip(off.tolist(), lens.tolist())]
    if not wait:
        return fetch, (d_seqs, d_off, d_len)
    ctx.synchronize()
    torch.cuda.synchronize()  # (a caller's stream is not the context's)
    return fetch()


def device_runs(ctx, buf, off, lens, flags=0):
    w = edges.world()
    torch, dev = w["torch"], w["dev"]
    d_seqs, d_off, d_len = edges.upload(buf, off, lens)
    n, longest = len(lens), int(lens.max())
    cap = ctx.device_rle_runs_cap(len(buf), n, longest)
    runs = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
    roff = torch.zeros(n, dtype=torch.int64, device=dev)
    rcnt = torch.zeros(n, dtype=torch.int32, device=dev)
    nruns = torch.zeros(1, dtype=torch.int64, device=dev)
    calls = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.classify_batch_device_rle(d_seqs.data_ptr(), len(buf), d_off.data_ptr(), d_len.data_ptr(), n, calls.data_ptr(), runs.data_ptr(), cap,
                                  roff.data_ptr(), rcnt.data_ptr(), nruns.data_ptr(), max_read_len=longest, flags=flags)
    ctx.synchronize()
    assert int(nruns.item()) <= cap
    return calls.cpu().numpy().view(np.uint32), edges.expand_runs(runs.cpu().numpy().view(np.uint32), roff.cpu().numpy(), rcnt.cpu().numpy(), lens)


def one_run(form, buf, off, lens, chunk):
    ctx = edges.world()["ctx"]
    os.environ["KU_SHORT_CLAIM"] = str(chunk)
    try:
        ctx.reset_counts()
        calls, codes = form(ctx, buf, off, lens)
        return calls, codes, ctx.counts()
    finally:
        os.environ.pop("KU_SHORT_CLAIM", None)


def check(buf, off, lens, chunks):
    """the batch in both output forms at every chunk size, against the oracle and against the static stride"""
    edges.world()["ctx"].disable_sparse()
    run, want_calls, want_codes = edges.oracle_batch(buf, off, lens)
    for form in (device_codes, device_runs):
        s_calls, s_codes, s_counts = one_run(form, buf, off, lens, 0)
        edges.assert_reads(s_calls, s_codes, want_calls, want_codes)
        gc.assert_same_counts(s_counts, run)
        for chunk in chunks:
            calls, codes, counts = one_run(form, buf, off, lens, chunk)
            assert not (calls == FILL).any(), ("reads nobody classified", chunk, np.nonzero(calls == FILL)[0][:10])
            edges.assert_reads(calls, codes, want_calls, want_codes)
            edges.assert_reads(calls, codes, s_calls, s_codes)
            gc.assert_same_counts(counts, run)
            assert int(counts["n_reads"].sum()) == len(lens), (chunk, int(counts["n_reads"].sum()), len(lens))
            for key in ("n_kmers", "n_reads", "registers"):
                assert (counts[key] == s_counts[key]).all(), (chunk, key)
    edges.world()["ctx"].reset_counts()


def mixed_reads(rng, n):
    """reads of 31 .. 110 bases, every other one with a substitution; now and then one without k-mers, all N, N at both ends"""
    lens = rng.integers(K, 111, n)
    reads = [edges.frag(rng, int(l), sub=bool(i & 1)) for i, l in enumerate(lens)]
    for i in range(7, n, 97):
        reads[i] = special("shorter_than_k", rng)
    for i in range(11, n, 101):
        reads[i] = special("all_n", rng)
    for i in range(13, n, 103):
        reads[i] = special("n_at_both_ends", rng)
    return reads


def special(kind, rng):
    if kind == "plain":
        return edges.frag(rng, 100, sub=True)
    if kind == "shorter_than_k":
        return edges.frag(rng, K - 1)
    if kind == "all_n":
        return b"N" * 64
    t = bytearray(edges.frag(rng, 100, sub=True))
    t[0] = t[1] = t[-1] = t[-3] = ord("N")
    return bytes(t)


@pytest.mark.parametrize("chunk", [1, 2, 3, 16])
def test_read_counts_around_the_first_chunks(chunk):
    rng = np.random.default_rng(900 + chunk)
    first = n_waves() * chunk  # reads the waves own without a claim
    counts = [first - chunk - 1, first, first + 1, first + 3001 + chunk]
    assert counts[0] > 0 and (chunk == 1 or counts[3] % chunk != 0)
    reads = mixed_reads(rng, max(counts))
    for n in counts:
        check(*pack(reads[:n], rng.integers(1, 5, n), tail=1), chunks=[chunk])


@pytest.mark.parametrize("place", ["mid_chunk", "chunk_first"])
@pytest.mark.parametrize("kind", ["plain", "shorter_than_k", "all_n", "n_at_both_ends"])
def test_the_batchs_last_read_on_the_buffers_final_bytes(kind, place):
    """chunks of three reads start at multiples of 3, wave-owned and claimed ones alike: read n - 1 is a chunk's first read when
    n - 1 is a multiple of 3 and its middle one when n - 1 = 1 (mod 3).  The read in front of it is a plain one that lies inside
    the buffer, so the text of the last one is asked for ahead -- at the dummy address -- and loaded in place."""
    rng = np.random.default_rng(950)
    chunk = 3
    n = 4 * n_waves() * chunk + 1 + (place == "mid_chunk")
    assert (n - 1) % chunk == (1 if place == "mid_chunk" else 0)
    reads = mixed_reads(rng, n)
    reads[n - 2] = special("plain", rng)
    reads[n - 1] = special(kind, rng)
    buf, off, lens = pack(reads, rng.integers(1, 5, n), tail=0)
    assert int(off[-1]) + int(lens[-1]) == len(buf)
    check(buf, off, lens, chunks=[chunk])


def test_instance_families_under_the_launch_recorder(tmp_path):
    """one batch per instance family in a child process that records its kernel launches (tests/claim_child.py): every cell
    matched the oracle with the claim and with the static stride, and launched the one instance it names"""
    rec = os.path.join(HERE, "rccl_shim", "libku_launch_recorder.so")
    assert os.path.exists(rec), "build the test libraries first (__graft_entry__.build())"
    out = tmp_path / "claim.json"
    env = {**os.environ, "LD_PRELOAD": rec + (":" + os.environ["LD_PRELOAD"] if os.environ.get("LD_PRELOAD") else "")}
    env.pop("KU_SHORT_BLOCKS_PER_CU", None)  # (the child sets the knobs cell by cell)
    p = subprocess.run([sys.executable, os.path.join(HERE, "claim_child.py"), str(out)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=240)
    print(p.stdout[-8000:])
    assert p.returncode == 0, p.stdout[-4000:]
    res = json.loads(out.read_text())
    assert res["rec_total"] > 0, "the recorder saw no launch"
    import claim_child
    seen = {c["cell"]: c for c in res["cells"]}
    bad = []
    for name, want in claim_child.CELLS.items():
        for mode in ("claim", "static"):
            c = seen.get(f"{name}/{mode}")
            if c is None:
                bad.append(f"{name}/{mode}: did not run")
            elif c["error"]:
                bad.append(f"{name}/{mode}:\n{c['error']}")
            elif c["launched"] != [want]:
                bad.append(f"{name}/{mode}: launched {c['launched']}, not {want}")
    assert not bad, "\n".join(bad)


# ---- the cell
def small_batches(rng, how_many, n):
    out = []
    for _ in range(how_many):
        reads = mixed_reads(rng, n)
        out.append(pack(reads, rng.integers(1, 5, n), tail=2))
    return out


def test_more_launches_than_cells_back_to_back_on_two_streams(monkeypatch):
    """2 x CLAIM_CELLS + 3 launches of about two reads per wave, none waited for, on two streams in turn: each launch finds its
    stream's cell clean (a launch sets it back itself) and classifies every read once"""
    w = edges.world()
    torch, ctx = w["torch"], w["ctx"]
    ctx.disable_sparse()
    monkeypatch.setenv("KU_SHORT_CLAIM", "2")
    rng = np.random.default_rng(970)
    batches = small_batches(rng, 3, 2 * n_waves() + 5)
    want = [edges.oracle_batch(*b)[1:] for b in batches]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ctx.reset_counts()
    pending = []
    n_launch = 2 * CLAIM_CELLS + 3
    for i in range(n_launch):
        b = batches[i % 3]
        pending.append(device_codes(ctx, *b, stream=streams[i & 1].cuda_stream, wait=False))
    for s in streams:
        s.synchronize()
    ctx.synchronize()
    for i, (fetch, _keep) in enumerate(pending):
        calls, codes = fetch()
        assert not (calls == FILL).any(), i
        edges.assert_reads(calls, codes, *want[i % 3])
    # the state of all launches together: the oracle over the same sequence of batches
    run = edges.oracle_batch(*batches[0])[0]
    for i in range(1, n_launch):
        run.classify_packed(*batches[i % 3])
    counts = ctx.counts()
    gc.assert_same_counts(counts, run)
    assert int(counts["n_reads"].sum()) == sum(len(batches[i % 3][2]) for i in range(n_launch))
    ctx.reset_counts()


def test_more_batches_than_cells_through_the_host_batch_call_two_deep(monkeypatch):
    """batches of about 2 k reads of 160 .. 222 bases (three k-mers per lane: the instance that claims with run output and
    accounting), two in flight at any time, their kernels on the context's two kernel streams in turn"""
    ctx = edges.world()["ctx"]
    ctx.disable_sparse()
    monkeypatch.setenv("KU_SHORT_CLAIM", "2")
    rng = np.random.default_rng(971)
    n = 2 * n_waves() + 7
    batches = []
    for _ in range(3):
        reads = [edges.frag(rng, int(l), sub=bool(i & 1)) for i, l in enumerate(rng.integers(160, 223, n))]
        batches.append(pack(reads, rng.integers(1, 5, n), tail=1))
    want = [edges.oracle_batch(*b)[1:] for b in batches]
    ctx.reset_counts()
    n_batch = CLAIM_CELLS + 5
    jobs, done = [], 0
    for i in range(n_batch + 1):
        if i < n_batch:
            jobs.append(ctx.rle_enqueue(*batches[i % 3]))
        if len(jobs) == 2 or (i == n_batch and jobs):
            while len(jobs) > (1 if i < n_batch else 0):
                rle = ctx.rle_finish(jobs.pop(0))
                lens = batches[done % 3][2]
                edges.assert_reads(rle["calls"], edges.expand_runs(rle["runs"], rle["run_off"], rle["run_cnt"], lens), *want[done % 3])
                done += 1
    assert done == n_batch
    run = edges.oracle_batch(*batches[0])[0]
    for i in range(1, n_batch):
        run.classify_packed(*batches[i % 3])
    counts = ctx.counts()
    gc.assert_same_counts(counts, run)
    assert int(counts["n_reads"].sum()) == n_batch * n
    ctx.reset_counts()


def test_one_stream_more_than_the_ring_has_cells_is_refused(monkeypatch):
    """a context of its own: CLAIM_CELLS streams bind the ring's cells one by one, the next one finds no cell that is known to be
    idle and the launch is refused (KU_EINVAL) -- and a stream that has its cell still launches"""
    w = edges.world()
    torch = w["torch"]
    monkeypatch.setenv("KU_SHORT_CLAIM", "2")
    rng = np.random.default_rng(972)
    buf, off, lens = small_batches(rng, 1, n_waves() + 3)[0]
    want = edges.oracle_batch(buf, off, lens)[1:]
    streams, seen = [], set()
    for prio in (0, -1):
        for _ in range(64):
            s = torch.cuda.Stream(priority=prio)
            if s.cuda_stream not in seen and s.cuda_stream != 0:
                seen.add(s.cuda_stream)
                streams.append(s)
    assert len(streams) > CLAIM_CELLS, f"only {len(streams)} distinct streams to be had"
    ctx = second_context()
    try:
        for s in streams[:CLAIM_CELLS]:
            calls, codes = device_codes(ctx, buf, off, lens, stream=s.cuda_stream)
            edges.assert_reads(calls, codes, *want)
        with pytest.raises(capi.KuError) as e:
            device_codes(ctx, buf, off, lens, stream=streams[CLAIM_CELLS].cuda_stream)
        assert e.value.status == -1  # KU_EINVAL
        calls, codes = device_codes(ctx, buf, off, lens, stream=streams[3].cuda_stream)
        edges.assert_reads(calls, codes, *want)
    finally:
        ctx.close()


def second_context():
    """the world's database once more, in a context whose ring this test may fill"""
    rng = np.random.default_rng(1313)
    db = gc.random_db(rng, n_genomes=12, glen=6000, k=K, nt=edges.NT)
    ids, par = db["tax"].arrays()
    ctx, _, _ = gc.make_ctx(cdb=capi.Db(pairs=db["pairs"].view(np.uint8), key_ct=len(db["kmers"]), k=K, offsets=db["offsets"], nt=edges.NT),
                            ctax=capi.Tax(ids=ids, parents=par))
    return ctx
