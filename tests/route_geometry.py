"""A small owner-routed world at any (k, nt), for tests/test_route_geometry_model.py (CPU), tests/test_gpu_route_geometry.py and the
`route13` / `route15` cells of tests/instances_child.py.  Not a test module.

The owner kernel (ku_route.hip) has instances of its own for k = 31 with nt = 13 and nt = 15, and a world tiled over all
4^nt bins needs 4^nt + 1 offsets on some rank (8.6 GB at nt = 15).  ku_mgpu_set_taxonomy only asks that the ranks' ranges ascend
and do not overlap, and ku_ctx_adopt_db takes bin_hi - bin_lo + 1 offsets, so two NARROW shards do: with S = 4^nt,

    rank 0 owns [0, S/w)      nobody owns [S/w, S/w + S/g)      rank 1 owns [S/w + S/g, 2 S/w + S/g)      nobody owns the rest

which also puts k-mers into bins that nobody owns (KU_ROUTE_MISS: slot 0, not booked) in front of the scan, the fused ROUTE
resolve and ku_route_gather_kernel.  Nothing here holds 4^nt entries of anything.

The reference is the oracle over the OWNED k-mers only, indexed at nt = 9: what a k-mer classifies as does not depend on the
index's bin-key length (the model test holds the oracle to that), and a k-mer of a gap is then simply absent -- slot 0.  One
thing differs: the oracle books every miss under taxon 0, the routed step only the misses an owner saw.  Taxon 0's n_kmers and
registers are therefore rebuilt here from the reads: unambiguous k-mers, not in the owned set, bin in an owned range.
"""
import numpy as np

from krakenuniq_amd import synth
from oracle import ku_oracle as ko

# (k, nt) -> (w, g): a rank owns S / w bins, the gap between the ranks is S / g wide
GEOMETRIES = {(31, 15): (32, 256), (31, 13): (16, 64), (25, 13): (16, 64)}
N_SPECIES, GENOME_LEN, ORACLE_NT = 6, 20_000, 9
_BASES = b"ACGT"


def route_maxn(k, nt):
    """k-mers per record (ku_route_maxn, ku_internal.h): the window, cut so that the record's bases fit 56"""
    return min(k - nt + 1, 57 - k, 31)


class World:
    """database, taxonomy and the two ranks' shards of one geometry (host side; `Routed` puts it on the device)"""

    def __init__(self, k, nt, seed=None):
        w, g = GEOMETRIES[(k, nt)]
        S = 4 ** nt
        self.k, self.nt = k, nt
        self.ranges = [(0, S // w), (S // w + S // g, 2 * (S // w) + S // g)]
        rng = np.random.default_rng(1000 * k + nt if seed is None else seed)
        # three genera of two species: siblings are mutated copies of one sequence, so they share k-mers (LCA = the genus)
        self.tax = synth.random_taxonomy(N_SPECIES, rng, levels=(1, 2, 3, 3))
        base, self.genomes = {}, {}
        for i, tid in enumerate(self.tax.species):
            par = self.tax.parent[tid]
            if par not in base:
                base[par] = synth.procedural_genome(int(rng.integers(1, 1 << 30)), i, GENOME_LEN)
            self.genomes[tid] = synth.mutate(base[par], 0.03, rng)
        self.ascii = [synth.codes_to_ascii(g_) for g_ in self.genomes.values()]
        kmers, vals = synth.lca_database(self.genomes, self.tax, k)
        bins = synth.bin_key(kmers, k, nt)
        order = np.lexsort((kmers, bins))
        # the global database: offsets are indices into THIS order
        self.kmers, self.vals, self.bins = kmers[order], vals[order], bins[order]
        self.cut = [(int(np.searchsorted(self.bins, lo)), int(np.searchsorted(self.bins, hi))) for lo, hi in self.ranges]
        self.owned_kmers = np.sort(np.concatenate([self.kmers[a:b] for a, b in self.cut]))
        self.ids, self.parents = self.tax.arrays()
        self._shards, self._odb = {}, {}

    def owner_of(self, bins):
        """rank that owns each bin, -1: nobody (-1 below the second range = the gap, above it = the unowned top)"""
        out = np.full(bins.shape, -1, dtype=np.int64)
        for r, (lo, hi) in enumerate(self.ranges):
            out[(bins >= np.uint64(lo)) & (bins < np.uint64(hi))] = r
        return out

    def shard(self, r):
        """rank r's 12-byte pairs and its hi - lo + 1 offsets (global pair indices, closing entry included)"""
        if r not in self._shards:
            (lo, hi), (a, b) = self.ranges[r], self.cut[r]
            per_bin = np.bincount((self.bins[a:b] - np.uint64(lo)).astype(np.int64), minlength=hi - lo)
            offsets = np.empty(hi - lo + 1, dtype=np.uint64)
            offsets[0] = a
            np.cumsum(per_bin, out=offsets[1:])
            offsets[1:] += np.uint64(a)
            assert int(offsets[-1]) == b
            self._shards[r] = {"pairs": synth.pack_pairs(self.kmers[a:b], self.vals[a:b]), "offsets": offsets, "lo": lo, "hi": hi,
                               "n_pairs": b - a}
        return self._shards[r]

    def oracle_db(self, nt=ORACLE_NT, ranks=(0, 1)):
        """ko.Db over the k-mers the given ranks own, indexed at `nt`"""
        key = (nt, tuple(ranks))
        if key not in self._odb:
            km = np.concatenate([self.kmers[self.cut[r][0]:self.cut[r][1]] for r in ranks])
            va = np.concatenate([self.vals[self.cut[r][0]:self.cut[r][1]] for r in ranks])
            sk, sv, off = synth.sort_db(km, va, self.k, nt)
            kl = (2 * self.k + 7) // 8
            raw = np.zeros(len(sk) * (kl + 4), dtype=np.uint8)
            rec = raw.reshape(-1, kl + 4)
            rec[:, :kl] = sk.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :kl]
            rec[:, kl:] = sv.astype("<u4").view(np.uint8).reshape(-1, 4)
            self._odb[key] = ko.Db(pairs=raw, key_ct=len(sk), k=self.k, offsets=off, nt=nt)
        return self._odb[key]

    def oracle_tax(self):
        return ko.Tax(ids=self.ids, parents=self.parents)


# ---- reads
def _noisy(rng, s):
    """3 % substitutions and a few N"""
    r = bytearray(s)
    n = len(r)
    for p in np.nonzero(rng.random(n) < 0.03)[0]:
        r[p] = _BASES[(_BASES.index(r[p]) + int(rng.integers(1, 4))) & 3] if r[p] in _BASES else r[p]
    for p in rng.integers(0, max(n, 1), size=int(rng.poisson(n * 0.002))):
        r[p] = ord("N")
    return bytes(r)


def _random_seq(rng, n):
    return np.frombuffer(_BASES, dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def make_reads(world, shape, seed):
    """`short`: ~4 000 reads, the longest of exactly 128 k-mers (one pass of the ROUTE resolve; enough records that every lane of
    an owner group is busy and a group's k-mers exceed one round of 128); `win`: ~1 000 mate pairs 150 + N + 150 and ~40
    reads of 3 kbp (the windowed ROUTE instance).  Genome fragments (either strand) with substitutions and N, a tenth pure
    random sequence, and the edge reads every batch of the instance matrix carries."""
    import instances_child as ic
    rng = np.random.default_rng(seed)
    k, g = world.k, world.ascii
    if shape == "short":
        lmax = 128 + k - 1
        reads = ic.edge_reads(rng, g, k, lmax)
        for _ in range(4000):
            n = lmax if rng.random() < 0.5 else int(rng.integers(k, lmax + 1))
            reads.append(_random_seq(rng, n) if rng.random() < 0.1 else _noisy(rng, ic.frag(rng, g, n)))
        reads.append(ic.frag(rng, g, lmax))
    else:
        lmax = 3000
        reads = ic.edge_reads(rng, g, k, lmax)
        for _ in range(1000):
            if rng.random() < 0.1:
                reads.append(_random_seq(rng, 150) + b"N" + _random_seq(rng, 150))
            else:
                reads.append(_noisy(rng, ic.frag(rng, g, 150)) + b"N" + _noisy(rng, ic.frag(rng, g, 150)))
        for i in range(40):
            reads.append(_random_seq(rng, lmax) if i % 10 == 9 else _noisy(rng, ic.frag(rng, g, lmax)))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def read_kmers(reads, k):
    """canonical k-mers and ambiguity flags of all reads, read after read (the layout of the oracle's per-k-mer arrays)"""
    fw, am = [], []
    for s in reads:
        f, a = ko.scan(s, k)
        fw.append(f)
        am.append(a)
    return synth.canonical(np.concatenate(fw), k), np.concatenate(am)


# ---- reference
class Reference:
    """the oracle's run over `reads`, with taxon 0's state as the routed step books it"""

    def __init__(self, world, reads, quick=False, min_hits=1, ranks=(0, 1), oracle_nt=ORACLE_NT, threads=4):
        self.world, self.reads = world, reads
        self.buf, self.off, self.lens = ko.pack_reads(reads)
        self.tax = world.oracle_tax()
        run = ko.Run(world.oracle_db(oracle_nt, ranks), self.tax, quick=quick, min_hits=min_hits, threads=threads)
        res = run.classify_packed(self.buf, self.off, self.lens)
        self.calls, self.hits, self.taxa_off = res["calls"], res["hits"], res["taxa_off"].astype(np.int64)
        n = int(self.taxa_off[-1])
        self.ambig = res["ambig"][:n]
        self.codes = res["taxa"][:n].copy()
        self.codes[self.ambig != 0] = 0xFFFFFFFF
        self.n_reads, self.n_kmers, self.registers = {}, {}, {}
        for t, c in run.counts().items():
            if c["n_reads"]:
                self.n_reads[t] = c["n_reads"]
            if c["n_kmers"]:
                self.n_kmers[t] = c["n_kmers"]
                self.registers[t] = c["sketch"].registers()
        self.oracle_zero = self.n_kmers.get(0, 0)
        if quick:
            # quick mode books the scanned prefix of a read in the resolve stage of the rank that read it, misses under
            # slot 0 whoever owns their bin (or nobody): the oracle's own taxon 0
            return
        # taxon 0 of the routed step: the misses whose bin somebody owns
        self.canon, amb = read_kmers(reads, world.k)
        assert np.array_equal(amb != 0, self.ambig != 0)
        self.bins = synth.bin_key(self.canon, world.k, world.nt)
        own = world.owner_of(self.bins)
        self.owner = np.where(np.isin(own, ranks), own, -1)
        in_db = np.isin(self.canon, np.sort(np.concatenate([world.kmers[world.cut[r][0]:world.cut[r][1]] for r in ranks])))
        booked = (self.ambig == 0) & ~in_db & (self.owner >= 0)
        self.n_kmers.pop(0, None)
        self.registers.pop(0, None)
        if booked.any():
            h = ko.Hll(12, False)
            for x in self.canon[booked].tolist():
                h.insert(x)
            self.n_kmers[0] = int(booked.sum())
            self.registers[0] = h.registers()

    def slice(self, a, b):
        """reads [a, b) as a batch of their own: (reads, calls, codes)"""
        return self.reads[a:b], self.calls[a:b], self.codes[int(self.taxa_off[a]):int(self.taxa_off[b])]


def assert_counts(ctx_counts, ref):
    """n_reads, n_kmers and the HLL registers per taxon, bit for bit (gpu_common.assert_same_counts against `ref`)"""
    got_k = {int(t): (int(n), r) for t, n, r in zip(ctx_counts["slot_taxid"], ctx_counts["n_kmers"], ctx_counts["registers"]) if n}
    got_r = {int(t): int(n) for t, n in zip(ctx_counts["node_taxid"], ctx_counts["n_reads"]) if n}
    assert got_r == ref.n_reads, "n_reads differ"
    assert {t: v[0] for t, v in got_k.items()} == ref.n_kmers, ("n_kmers differ", {t: v[0] for t, v in got_k.items()}.get(0), ref.n_kmers.get(0))
    for t, (n, regs) in got_k.items():
        assert (regs == ref.registers[t]).all(), ("registers differ", t)
    for n, r in zip(ctx_counts["n_kmers"], ctx_counts["registers"]):
        if n == 0:
            assert not r.any()


def assert_zero_state(ctx_counts):
    assert not ctx_counts["n_kmers"].any() and not ctx_counts["n_reads"].any() and not ctx_counts["registers"].any(), \
        "counting off left per-taxon state"


# ---- the device side
class Routed:
    """the world on device 0: one ku_mgpu group whose ranks share the device; rank r adopts shard r.  `n_ranks` = 1 is the world
    of one (KU_MGPU_FORCE_ROUTE=1, read by set_taxonomy: set it before): rank 0's range is owned, everything else is not"""

    def __init__(self, world, n_ranks=2):
        import torch
        from krakenuniq_amd import capi
        self.torch, self.capi, self.world, self.W = torch, capi, world, n_ranks
        self.dev = torch.device("cuda:0")
        self.mg = capi.Mgpu([0] * n_ranks)
        self.keep = []
        for r in range(n_ranks):
            sh = world.shard(r)
            pairs = torch.from_numpy(sh["pairs"].view(np.uint8).copy()).to(self.dev)  # (the context rewrites values as slots in place)
            offsets = torch.from_numpy(sh["offsets"].view(np.int64)).to(self.dev)
            self.mg.ctx(r).adopt_db(pairs.data_ptr(), sh["n_pairs"], offsets.data_ptr(), world.k, world.nt, 2, sh["lo"], sh["hi"])
            self.keep += [pairs, offsets]
        self.ctax = capi.Tax(ids=world.ids, parents=world.parents)
        self.mg.set_taxonomy(self.ctax)
        assert self.mg.uses_routing()

    def upload(self, reads):
        """the batch on rank 0, empty buffers of the same size on the others (the step scatters the slices)"""
        torch, dev, W = self.torch, self.dev, self.W
        buf, off, lens = ko.pack_reads(reads)
        N, nb = len(lens), len(buf)
        rb = [N * r // W for r in range(W + 1)]
        pb = [int(off[x]) if x < N else nb for x in rb]
        h = {"seqs": np.frombuffer(buf, dtype=np.uint8), "off": off.astype(np.int64), "len": lens.astype(np.int32)}
        bufs = []
        for r in range(W):
            b = {"seqs": torch.zeros(nb + 16, dtype=torch.uint8, device=dev), "off": torch.zeros(N, dtype=torch.int64, device=dev),
                 "len": torch.zeros(N, dtype=torch.int32, device=dev), "calls": torch.zeros(N, dtype=torch.int32, device=dev),
                 "taxa": torch.zeros(nb + 16, dtype=torch.int32, device=dev)}
            if r == 0:
                b["seqs"][:nb] = torch.from_numpy(h["seqs"].copy()).to(dev)
                b["off"][:] = torch.from_numpy(h["off"]).to(dev)
                b["len"][:] = torch.from_numpy(h["len"]).to(dev)
            bufs.append(b)
        torch.cuda.synchronize()
        return {"bufs": bufs, "N": N, "nb": nb, "rb": rb, "pb": pb, "off": off, "lens": lens}

    def step(self, up, flags=0, min_hits=1, max_read_len=None):
        """one ku_mgpu_step_device; returns per rank (first read, last read, calls, per-k-mer codes at the valid positions)"""
        L = int(up["lens"].max()) if max_read_len is None else max_read_len
        self.mg.step_device([{"d_seqs": b["seqs"].data_ptr(), "d_seq_off": b["off"].data_ptr(), "d_seq_len": b["len"].data_ptr(),
                              "d_calls": b["calls"].data_ptr(), "d_taxa": b["taxa"].data_ptr()} for b in up["bufs"]],
                            up["nb"], up["N"], up["rb"], up["pb"], flags=flags, min_hits=min_hits, max_read_len=L)
        for r in range(self.W):
            self.mg.ctx(r).synchronize()

    def results(self, up):
        k, out = self.world.k, []
        for r in range(self.W):
            lo, hi = up["rb"][r], up["rb"][r + 1]
            calls = up["bufs"][r]["calls"].cpu().numpy().view(np.uint32)[lo:hi]
            taxa = up["bufs"][r]["taxa"].cpu().numpy().view(np.uint32)
            parts = [taxa[int(o):int(o) + max(int(n) - k + 1, 0)] for o, n in zip(up["off"][lo:hi], up["lens"][lo:hi])]
            out.append((lo, hi, calls, np.concatenate(parts) if parts else np.zeros(0, np.uint32)))
        return out

    def counts(self):
        self.mg.reduce_state()
        return self.mg.ctx(0).counts()

    def close(self):
        self.mg.close()
        self.keep = []
        self.torch.cuda.empty_cache()


def assert_step(routed, up, ref, first_read=0, codes=True):
    """calls per rank slice, and the per-k-mer codes at the valid positions, against reads [first_read, first_read + N) of `ref`"""
    for r, (lo, hi, calls, got) in enumerate(routed.results(up)):
        _, want_calls, want_codes = ref.slice(first_read + lo, first_read + hi)
        bad = np.nonzero(calls != want_calls)[0]
        assert len(bad) == 0, ("calls differ on rank", r, len(bad), (bad[:8] + lo).tolist())
        if codes:
            assert len(got) == len(want_codes), ("per-k-mer layout differs on rank", r)
            bad = np.nonzero(got != want_codes)[0]
            assert len(bad) == 0, ("per-k-mer codes differ on rank", r, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want_codes[bad[:8]].tolist())
