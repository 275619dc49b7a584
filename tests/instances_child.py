"""Child process of tests/test_gpu_instances.py: runs the matrix cells of one database geometry (kernel_instances.MATRIX[group])
under the launch recorder (LD_PRELOAD=libku_launch_recorder.so, set by the parent for this process only), compares every cell
with the oracle and writes, cell by cell, {cell, launched, error} to a JSON file.

    python tests/instances_child.py <group> <out.json>

Not a test module: the parent starts it with a time limit, reads the file and asserts.
"""
import ctypes
import json
import os
import sys
import tempfile
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import numpy as np  # noqa: E402

import kernel_instances as ki  # noqa: E402

REC_LIB = os.path.join(HERE, "rccl_shim", "libku_launch_recorder.so")
GOLDEN = os.path.join(HERE, "golden")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


class Recorder:
    """the recorder's list, read through its C entry points (the library is already in the process: LD_PRELOAD)"""

    def __init__(self):
        self.L = ctypes.CDLL(REC_LIB)
        for f in ("ku_rec_total", "ku_rec_count"):
            getattr(self.L, f).restype = ctypes.c_uint64
        self.L.ku_rec_get.restype = ctypes.c_uint64
        self.L.ku_rec_get.argtypes = [ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64]

    def clear(self):
        self.L.ku_rec_clear()

    def names(self):
        buf = ctypes.create_string_buffer(512)
        return [buf.value.decode() for i in range(self.L.ku_rec_count()) if self.L.ku_rec_get(i, buf, 512)]

    def total(self):
        return int(self.L.ku_rec_total())


class Out:
    def __init__(self, path, rec):
        self.path, self.rec, self.cells = path, rec, []

    def window(self, cell, fn):
        """run fn() with the recorder cleared before and read after: the family instances it launched belong to `cell`"""
        self.rec.clear()
        r = fn()
        got = sorted({n for n in self.rec.names() if ki.in_families(n)})
        self.cells.append({"cell": cell, "launched": got, "error": None})
        self.flush()
        return r

    def fail(self, cell, err):
        hit = [c for c in self.cells if c["cell"] == cell]
        if hit:
            hit[-1]["error"] = err
        else:
            self.cells.append({"cell": cell, "launched": [], "error": err})
        self.flush()

    def flush(self):
        with open(self.path + ".tmp", "w") as f:
            json.dump({"cells": self.cells, "rec_total": self.rec.total()}, f)
        os.replace(self.path + ".tmp", self.path)


# ---- reads
def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGTN", b"TGCAN"))


def frag(rng, genomes, n):
    g = genomes[int(rng.integers(len(genomes)))]
    if len(g) < n:
        g = (g * (n // len(g) + 1))
    a = int(rng.integers(0, len(g) - n + 1))
    s = g[a:a + n]
    return revcomp(s) if rng.random() < 0.5 else s


def edge_reads(rng, genomes, k, lmax):
    """the reads every batch carries: empty, k - 1 / k / k + 1 bases, all N, N at k-mer edges, low complexity (minimizer
    ties), reverse complements, chimeras of many taxa, a mate pair joined by N"""
    g0 = genomes[0]
    out = [b"", g0[:k - 1], g0[:k], g0[:k + 1], b"N" * (k + 9)]
    s = bytearray(frag(rng, genomes, min(lmax, k + 40)))
    for p in (0, k - 1, k, len(s) - k, len(s) - 1):
        t = bytearray(s)
        if 0 <= p < len(t):
            t[p] = ord("N")
        out.append(bytes(t))
    for u in (b"A", b"AT", b"ACG", b"AACC", b"GATTACA"):
        out.append((u * (lmax // len(u) + 1))[:min(lmax, 90)])
    f = frag(rng, genomes, min(lmax, 100))
    out += [revcomp(f), f]
    chim = b"".join(genomes[i % len(genomes)][50 * i:50 * i + k + 3] for i in range(64))
    out.append(chim[:lmax])
    if lmax >= 2 * 60 + 1:
        h = min(150, (lmax - 1) // 2)
        out.append(frag(rng, genomes, h) + b"N" + frag(rng, genomes, h))
    return [r for r in out if len(r) <= lmax]


def shape_batch(rng, genomes, k, n_kmers, n_bulk):
    """a batch whose longest read has exactly n_kmers k-mers"""
    lmax = n_kmers + k - 1
    reads = edge_reads(rng, genomes, k, lmax)
    for _ in range(n_bulk):
        n = int(rng.integers(k, lmax + 1))
        r = bytearray(frag(rng, genomes, n))
        for p in rng.integers(0, n, size=int(rng.poisson(n * 0.002))):
            r[p] = ord("N")
        reads.append(bytes(r))
    reads.append(frag(rng, genomes, lmax))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def pack(reads):
    from oracle import ku_oracle as ko
    return ko.pack_reads(reads)


# ---- comparisons
def rows(text):
    return sorted(text.strip("\n").split("\n"))


def want_codes(res, lens, k):
    t = res["taxa"].copy()
    t[res["ambig"][:len(t)] != 0] = 0xFFFFFFFF
    return t


def expand(rle, lens, k):
    """runs -> per-k-mer codes, read after read"""
    nk = np.maximum(lens.astype(np.int64) - k + 1, 0)
    out = np.zeros(int(nk.sum()), dtype=np.uint32)
    pos = 0
    runs = rle["runs"]
    for i in range(len(lens)):
        a, c, n = int(rle["run_off"][i]), int(rle["run_cnt"][i]), int(nk[i])
        if n:
            rr = runs[a:a + c]
            assert c > 0 and rr[0, 1] == 0, (i, c)
            starts = rr[:, 1].astype(np.int64)
            reps = np.diff(np.append(starts, n))
            assert (reps > 0).all(), i
            out[pos:pos + n] = np.repeat(rr[:, 0], reps)
        else:
            assert c == 0, i
        pos += n
    return out


def gpu_codes(gpu_taxa, off, lens, k):
    parts = [gpu_taxa[int(o):int(o) + max(int(l) - k + 1, 0)] for o, l in zip(off, lens)]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint32)


def assert_zero_state(ctx):
    c = ctx.counts()
    assert not c["n_kmers"].any() and not c["n_reads"].any() and not c["registers"].any(), "counting off left per-taxon state"


class Geo:
    """one database geometry: a context, the oracle's database and taxonomy, host genomes to cut reads from"""

    def __init__(self, ctx, ctax, odb, otax, taxpath, genomes, k, cores, bench=None):
        self.ctx, self.ctax, self.odb, self.otax, self.taxpath = ctx, ctax, odb, otax, taxpath
        self.genomes, self.k, self.cores, self.bench = genomes, k, cores, bench


def run_cell(out, geo, cell, buf, off, lens, quick=False):
    from krakenuniq_amd import capi
    from oracle import ku_oracle as ko
    import gpu_common as gc
    from test_gpu_sparse import assert_sparse_state_equals_oracle
    parts = cell.split("/")
    form, cnt = parts[2], parts[3]
    k, ctx = geo.k, geo.ctx
    flags = (capi.KU_F_NO_COUNTS if cnt == "off" else 0) | (capi.KU_F_QUICK if quick else 0)
    min_hits = 2 if quick else 1
    if form == "sparse":
        ctx.enable_sparse()
    ctx.reset_counts()
    try:
        if form == "codes":
            gpu = out.window(cell, lambda: ctx.classify_batch(buf, off, lens, flags=flags, min_hits=min_hits))
        else:
            gpu = out.window(cell, lambda: ctx.classify_batch_rle(buf, off, lens, flags=flags, min_hits=min_hits))
        run = ko.Run(geo.odb, geo.otax, threads=geo.cores, quick=quick, min_hits=min_hits)
        res = run.classify_packed(buf, off, lens)
        bad = np.nonzero(gpu["calls"] != res["calls"])[0]
        assert len(bad) == 0, ("calls differ", len(bad), bad[:8].tolist())
        if quick:
            assert (gpu["hits"] == res["hits"]).all(), "quick hit counts differ"
        else:
            want = want_codes(res, lens, k)
            got = gpu_codes(gpu["taxa"], off, lens, k) if form == "codes" else expand(gpu, lens, k)
            bad = np.nonzero(got != want[:len(got)])[0]
            assert len(got) == int(res["taxa_off"][-1]) and len(bad) == 0, ("per-k-mer codes differ", len(bad), bad[:8].tolist())
        if cnt == "off":
            assert_zero_state(ctx)
        elif form == "sparse":
            export_cell = cell + "/export" if cell + "/export" in ki.all_cells() else None
            if export_cell:
                # the open work unit closes first, unrecorded (its tail may go through the lookup kernel again,
                # ku_api_rle.cpp sparse_tail_insert); then sparse_export inside the window (it harvests the SEEN marks); the comparison below exports again
                ctx.sparse_close_unit()
                out.window(export_cell, lambda: ctx.sparse_export())
            counts, flags_s, pairs, n_sparse, n_dense = assert_sparse_state_equals_oracle(ctx, run)
            gc.assert_same_counts(counts, run)
            assert rows(ctx.report(geo.ctax)) == rows(run.report(geo.taxpath)), "report differs from the oracle's"
            if cell + "/reset" in ki.all_cells():
                out.window(cell + "/reset", lambda: ctx.reset_counts())
        else:
            gc.assert_same_counts(ctx.counts(), run)
    finally:
        if form == "sparse":
            ctx.disable_sparse()
    return res


def fused_cells(out, geo, group, rng):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    k = geo.k
    for cell in ki.MATRIX[group]:
        parts = cell.split("/")
        if len(parts) > 4 or parts[0] != group:
            continue
        try:
            shape = parts[1]
            if shape in ki.SHAPES:
                nk = ki.SHAPES[shape]
                reads = shape_batch(rng, geo.genomes, k, nk, 300 if shape == "win" else 1500)
            elif shape in ki.TINY:
                n = ki.TINY[shape] or n_cu * 6 * 4 + 1  # (ku_short_grid_waves: two k-mers per lane, < 500 k reads: 6 blocks of 4 per CU)
                reads = [frag(rng, geo.genomes, int(rng.integers(k + 20, k + 127))) for _ in range(n)]
            elif shape in ("w65535", "w65536"):
                nk = int(shape[1:])
                reads = edge_reads(rng, geo.genomes, k, 300) + [frag(rng, geo.genomes, 2000)]
                big = b"".join(geo.genomes)
                while len(big) < nk + k - 1:
                    big += big
                reads += [big[:nk + k - 1], revcomp(big[-(nk + k - 1):])]
            elif shape == "quick":
                reads = shape_batch(rng, geo.genomes, k, 120, 1500)
            buf, off, lens = pack(reads)
            run_cell(out, geo, cell, buf, off, lens, quick=shape == "quick")
        except Exception:
            out.fail(cell, traceback.format_exc(limit=6))


# ---- databases
def host_geo(k, nt, seed, tmp):
    from krakenuniq_amd import capi
    from oracle import ku_oracle as ko
    from gpu_common import random_db
    from test_gpu_fullsize import host_cores
    rng = np.random.default_rng(seed)
    db = random_db(rng, n_genomes=12, glen=6000, k=k, nt=nt)
    kl = (2 * k + 7) // 8
    raw = np.zeros(len(db["kmers"]) * (kl + 4), dtype=np.uint8)
    rec = raw.reshape(-1, kl + 4)
    rec[:, :kl] = db["kmers"].astype("<u8").view(np.uint8).reshape(-1, 8)[:, :kl]
    rec[:, kl:] = db["vals"].astype("<u4").view(np.uint8).reshape(-1, 4)
    taxpath = os.path.join(tmp, f"taxDB_{k}_{nt}")
    db["tax"].write(taxpath)
    odb = ko.Db(pairs=raw, key_ct=len(db["kmers"]), k=k, offsets=db["offsets"], nt=nt)
    cdb = capi.Db(pairs=raw, key_ct=len(db["kmers"]), k=k, offsets=db["offsets"], nt=nt)
    ctax, otax = capi.Tax(taxpath), ko.Tax(taxpath)
    ctx = capi.Ctx(0)
    ctx.load_db(cdb)
    ctx.set_taxonomy(ctax)
    ctx._keep += [cdb, ctax, raw]
    genomes = [ACGT[np.asarray(g)].tobytes() for g in db["genomes"].values()]  # (2-bit codes)
    return Geo(ctx, ctax, odb, otax, taxpath, genomes, k, host_cores())


def bench_geo(nt, n_species, genome_len, seed, tmp):
    import torch
    from krakenuniq_amd import capi, synth_torch
    from oracle import ku_oracle as ko
    from test_gpu_fullsize import host_cores, oracle_db_from_device
    dev = torch.device("cuda:0")
    db = synth_torch.BenchDb(dev, n_species=n_species, genome_len=genome_len, k=31, nt=nt, seed=seed)
    taxpath = os.path.join(tmp, f"taxDB_bench_{nt}")
    db.tax.write(taxpath)
    odb, keep = oracle_db_from_device(torch, db.kmers, db.vals, db.offsets, 31, nt)
    db.kmers = db.vals = None
    ctax, otax = capi.Tax(taxpath), ko.Tax(taxpath)
    ctx = capi.Ctx(0)
    ctx.adopt_db(db.pairs.data_ptr(), db.n_pairs, db.offsets.data_ptr(), 31, nt, 2, keep=db)
    ctx.set_taxonomy(ctax)
    ctx._keep += [ctax, keep]
    codes = db.genomes[:256].cpu().numpy()
    genomes = [ACGT[row].tobytes() for row in codes]
    return Geo(ctx, ctax, odb, otax, taxpath, genomes, 31, host_cores(), bench=db)


# ---- the routed step and the staged kernels
def route_cells(out, tmp):
    import torch
    from krakenuniq_amd import capi, synth_torch
    from oracle import ku_oracle as ko
    import gpu_common as gc
    from test_gpu_fullsize import host_cores, oracle_db_from_device
    dev = torch.device("cuda:0")
    NT, W, K = 11, 2, 31
    db = synth_torch.BenchDb(dev, n_species=100, genome_len=60_000, k=K, nt=NT, seed=3)
    ids, par = db.tax.arrays()
    ctax, otax = capi.Tax(ids=ids, parents=par), ko.Tax(ids=ids, parents=par)
    odb, keep = oracle_db_from_device(torch, db.kmers, db.vals, db.offsets, K, NT)
    offs = db.offsets
    bounds = [0] + [int(torch.searchsorted(offs, offs[-1] * q // W).item()) for q in range(1, W)] + [4 ** NT]
    for cell in ki.MATRIX["route"]:
        group, shape, cnt = cell.split("/")[0], cell.split("/")[1], cell.split("/")[3]
        if group != "route":
            route_geometry_cell(out, cell, int(group[5:]), cnt)
            continue
        try:
            if shape == "s128":
                N, L = 20_000, 150
                seqs, off, lens, _ = db.sample_reads(N, L, seed=5, n_rate=0.003)
            else:
                N, L = 6_000, 301
                seqs, off, lens = db.sample_pairs(N, 150, seed=9, n_rate=0.003)
            seqs = seqs.reshape(-1)
            nb = seqs.numel()
            mg = capi.Mgpu([0] * W)
            shards = []
            for r in range(W):
                sh = synth_torch.BenchDb(dev, n_species=100, genome_len=60_000, k=K, nt=NT, seed=3, bin_lo=bounds[r], bin_hi=bounds[r + 1])
                mg.ctx(r).adopt_db(sh.pairs.data_ptr(), sh.n_pairs, sh.offsets.data_ptr(), K, NT, 2, bounds[r], bounds[r + 1])
                shards.append(sh)
            mg.set_taxonomy(ctax)
            assert mg.uses_routing()
            rb = [N * r // W for r in range(W + 1)]
            stride = nb // N
            pb = [x * stride for x in rb]
            bufs = []
            for r in range(W):
                bufs.append({"seqs": seqs if r == 0 else torch.zeros(nb + 16, dtype=torch.uint8, device=dev),
                             "off": off if r == 0 else torch.zeros(N, dtype=torch.int64, device=dev),
                             "len": lens if r == 0 else torch.zeros(N, dtype=torch.int32, device=dev),
                             "calls": torch.zeros(N, dtype=torch.int32, device=dev),
                             "taxa": torch.zeros(nb + 16, dtype=torch.int32, device=dev)})
            torch.cuda.synchronize()
            flags = capi.KU_F_NO_COUNTS if cnt == "off" else 0

            def step():
                mg.step_device([{"d_seqs": b["seqs"].data_ptr(), "d_seq_off": b["off"].data_ptr(), "d_seq_len": b["len"].data_ptr(),
                                 "d_calls": b["calls"].data_ptr(), "d_taxa": b["taxa"].data_ptr()} for b in bufs],
                               nb, N, rb, pb, flags=flags, max_read_len=L)
                for r in range(W):
                    mg.ctx(r).synchronize()
            out.window(cell, step)
            run = ko.Run(odb, otax, threads=host_cores())
            h_seqs = seqs.cpu().numpy()
            h_off, h_len = off.cpu().numpy().astype(np.uint64), lens.cpu().numpy().astype(np.uint32)
            res = run.classify_packed(h_seqs, h_off, h_len)
            want = want_codes(res, h_len, K)
            for r in range(W):
                lo, hi = rb[r], rb[r + 1]
                calls = bufs[r]["calls"].cpu().numpy().view(np.uint32)[lo:hi]
                assert np.array_equal(calls, res["calls"][lo:hi]), ("calls differ on rank", r)
                got = gpu_codes(bufs[r]["taxa"].cpu().numpy().view(np.uint32), h_off[lo:hi], h_len[lo:hi], K)
                a, b = int(res["taxa_off"][lo]), int(res["taxa_off"][hi])
                assert np.array_equal(got, want[a:b]), ("per-k-mer codes differ on rank", r)
            mg.reduce_state()
            if cnt == "off":
                assert_zero_state(mg.ctx(0))
            else:
                gc.assert_same_counts(mg.ctx(0).counts(), run)
            mg.close()
            del shards, bufs
            torch.cuda.empty_cache()
        except Exception:
            out.fail(cell, traceback.format_exc(limit=6))


_route_worlds = {}


def route_geometry_cell(out, cell, nt, cnt):
    """route13 / route15: the routed step at k = 31, nt = 13 / 15 over two narrow bin ranges (route_geometry.py)"""
    from krakenuniq_amd import capi
    import route_geometry as rg
    try:
        if nt not in _route_worlds:
            w = rg.World(31, nt)
            reads = rg.make_reads(w, "short", 1)
            _route_worlds[nt] = (w, reads, rg.Reference(w, reads))
        w, reads, ref = _route_worlds[nt]
        flags = capi.KU_F_NO_COUNTS if cnt == "off" else 0
        routed = rg.Routed(w)
        try:
            up = routed.upload(reads)
            out.window(cell, lambda: routed.step(up, flags=flags))
            rg.assert_step(routed, up, ref)
            counts = routed.counts()
            if cnt == "off":
                rg.assert_zero_state(counts)
            else:
                rg.assert_counts(counts, ref)
        finally:
            routed.close()
    except Exception:
        out.fail(cell, traceback.format_exc(limit=6))


def staged_cells(out, tmp):
    import torch
    from krakenuniq_amd import capi, synth
    from oracle import ku_oracle as ko
    import gpu_common as gc
    from gpu_common import make_ctx, oracle_flat
    dev = torch.device("cuda:0")
    f1, f8 = os.path.join(GOLDEN, "f1"), os.path.join(GOLDEN, "f8")
    K = 31
    _, seqs1 = synth.read_seqfile(f"{f1}/reads.fq")
    _, seqs8 = synth.read_seqfile(f"{f8}/reads.fq")
    odb1 = ko.Db(f"{f1}/database.kdb", f"{f1}/database.idx")
    odb8 = ko.Db(f"{f8}/database.kdb", f"{f8}/database.idx")
    otax = ko.Tax(f"{f1}/taxDB")

    def classify_cell(cell, ctx, seqs, extra=()):
        cnt = cell.split("/")[3]
        flags = capi.KU_F_NO_COUNTS if cnt == "off" else 0
        run, res, buf, off, lens, taxa = oracle_flat(odb1, otax, seqs, extra_dbs=extra)
        ctx.reset_counts()
        gpu = out.window(cell, lambda: ctx.classify_batch(buf, off, lens, flags=flags))
        gc.assert_same_classification(gpu, res, taxa, off, lens, K)
        if cnt == "off":
            assert_zero_state(ctx)
        else:
            gc.assert_same_counts(ctx.counts(), run)

    for cell in ki.MATRIX["staged"]:
        what = cell.split("/")[1]
        try:
            if what in ("sorted", "prior", "prior_sorted"):
                if what != "prior":
                    os.environ["KU_LAYOUT"] = "sorted"
                try:
                    ctx = capi.Ctx(0)
                    cdb1 = capi.Db(f"{f1}/database.kdb", f"{f1}/database.idx")
                    ctx.load_db(cdb1)
                    ctx._keep.append(cdb1)
                    if what != "sorted":
                        cdb8 = capi.Db(f"{f8}/database.kdb", f"{f8}/database.idx")
                        ctx.add_db(cdb8)
                        ctx._keep.append(cdb8)
                    ctax = capi.Tax(f"{f1}/taxDB")
                    ctx.set_taxonomy(ctax)
                    ctx._keep.append(ctax)
                finally:
                    os.environ.pop("KU_LAYOUT", None)
                assert ctx.db_layout()["hash"] == (what == "prior")
                classify_cell(cell, ctx, seqs1 if what == "sorted" else seqs8, () if what == "sorted" else (odb8,))
                ctx.close()
            elif what == "shard":
                form, cnt = cell.split("/")[2], cell.split("/")[3]
                if form == "resolve":
                    continue  # (run inside the codes/on cell below)
                base, cdb, ctax = make_ctx(f1)
                bounds = cdb.shard_plan(2)
                all_values = base.db_values()
                run, res, buf, off, lens, taxa = oracle_flat(odb1, otax, seqs1)
                t_seq = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
                t_off = torch.from_numpy(off.astype(np.int64)).to(dev)
                t_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
                flags = capi.KU_F_NO_COUNTS if cnt == "off" else 0
                ctxs, slots = [], []
                for s in range(2):
                    c, _, _ = make_ctx(cdb=cdb, ctax=ctax, shard=(int(bounds[s]), int(bounds[s + 1])), all_values=all_values)
                    ctxs.append(c)
                    slots.append(torch.zeros(len(buf), dtype=torch.int32, device=dev))

                def lookups():
                    for c, t in zip(ctxs, slots):
                        c.lookup_device(t_seq.data_ptr(), len(buf), t.data_ptr(), flags=capi.KU_F_KEEP_SLOTS | flags)
                        c.synchronize()
                out.window(cell, lookups)
                merged = torch.maximum(slots[0], slots[1])
                t_calls = torch.zeros(len(lens), dtype=torch.int32, device=dev)

                def resolve():
                    ctxs[0].resolve_device(t_seq.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), len(lens), t_calls.data_ptr(),
                                           merged.data_ptr(), flags=flags, max_read_len=int(lens.max()))
                    ctxs[0].synchronize()
                if cnt == "on":
                    out.window("staged/shard/resolve/on", resolve)
                else:
                    resolve()
                gpu = {"calls": t_calls.cpu().numpy().view(np.uint32), "taxa": merged.cpu().numpy().view(np.uint32)}
                gc.assert_same_classification(gpu, res, taxa, off, lens, K)
                cs = [c.counts() for c in ctxs]
                if cnt == "off":
                    for c in ctxs:
                        assert_zero_state(c)
                else:
                    tot = dict(cs[0])
                    tot["registers"] = np.maximum.reduce([c["registers"] for c in cs])
                    tot["n_kmers"] = np.sum([c["n_kmers"] for c in cs], axis=0)
                    tot["n_reads"] = np.sum([c["n_reads"] for c in cs], axis=0)
                    gc.assert_same_counts(tot, run)
                for c in ctxs + [base]:
                    c.close()
            elif what == "stats":
                ctx, cdb, ctax = make_ctx(f1)
                run, res, buf, off, lens, taxa = oracle_flat(odb1, otax, seqs1)
                t_seq = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
                torch.cuda.synchronize()
                st = out.window(cell, lambda: ctx.lookup_stats_device(t_seq.data_ptr(), len(buf)))
                # one query per unambiguous k-mer of the buffer (k-mers across a read separator are ambiguous)
                n_ok = int((res["ambig"][:int(res["taxa_off"][-1])] == 0).sum())
                assert st["lookups"] == n_ok, (st, n_ok)
                assert 0 < st["nonempty"] <= st["lookups"] and st["sum_nb"] >= st["nonempty"], st
                ctx.close()
        except Exception:
            out.fail(cell, traceback.format_exc(limit=6))


def main():
    group, path = sys.argv[1], sys.argv[2]
    assert "libku_launch_recorder" in os.environ.get("LD_PRELOAD", ""), "run me with the recorder preloaded"
    import torch  # noqa: F401  (before the library: one HIP runtime, torch's)
    from krakenuniq_amd import capi
    rec = Recorder()
    capi.lib()
    out = Out(path, rec)
    out.flush()
    rng = np.random.default_rng({"g13": 13, "g15": 15, "g10": 10, "e25": 25}.get(group, 1))
    with tempfile.TemporaryDirectory() as tmp:
        if group == "g13":
            fused_cells(out, host_geo(31, 13, 1313, tmp), "g13", rng)
            p = bench_geo(13, 2000, 4000, 1301, tmp)
            fused_cells_pressure(out, p, "p13")
        elif group == "g15":
            geo = bench_geo(15, 2000, 4000, 1501, tmp)
            fused_cells(out, geo, "g15", rng)
            fused_cells_pressure(out, geo, "p15")
        elif group == "g10":
            fused_cells(out, host_geo(31, 10, 1010, tmp), "g10", rng)
        elif group == "e25":
            fused_cells(out, host_geo(25, 13, 2513, tmp), "e25", rng)
        elif group == "route":
            route_cells(out, tmp)
        elif group == "staged":
            staged_cells(out, tmp)
        else:
            raise SystemExit(f"unknown group {group}")
    out.flush()
    for c in out.cells:
        print(f"{c['cell']:32s} -> {', '.join(c['launched']) or '(none)'}{'   FAILED' if c['error'] else ''}")
    print("launches recorded:", rec.total())


def fused_cells_pressure(out, geo, prefix):
    group = "g13" if prefix == "p13" else "g15"
    for cell in ki.MATRIX[group]:
        if not cell.startswith(prefix + "/"):
            continue
        try:
            os.environ["KU_SHORT_BLOCKS_PER_CU"] = "1"  # fewer waves: each meets more reads (and taxa) than its LDS tables hold
            if cell.split("/")[1] == "win":
                s, o, l_ = geo.bench.sample_pairs(20_000, 150, seed=5, n_rate=0.002)
            else:
                s, o, l_, _ = geo.bench.sample_reads(300_000, 150, seed=6, n_rate=0.002)
            buf = s.reshape(-1).cpu().numpy()
            off, lens = o.cpu().numpy().astype(np.uint64), l_.cpu().numpy().astype(np.uint32)
            run_cell(out, geo, cell, buf, off, lens)
        except Exception:
            out.fail(cell, traceback.format_exc(limit=6))
        finally:
            os.environ.pop("KU_SHORT_BLOCKS_PER_CU", None)


if __name__ == "__main__":
    main()
