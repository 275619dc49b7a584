"""CPU: the reference of tests/test_gpu_route_geometry.py (tests/route_geometry.py) held to its own conditions, so that the
GPU test cannot pass vacuously: the narrow ranges own enough of the reads' k-mers, the gap and the unowned top are populated,
taxon 0's expected state is neither empty nor the oracle's own, reads are called and left uncalled, records of maximal
length occur, nothing of 4^nt entries is allocated, and the oracle does not care at which nt its database is indexed."""
import numpy as np
import pytest

import route_geometry as rg
from krakenuniq_amd import synth

_cache = {}


def world_and_ref(k, nt):
    if (k, nt) not in _cache:
        w = rg.World(k, nt)
        _cache[(k, nt)] = (w, rg.Reference(w, rg.make_reads(w, "short", 1)))
    return _cache[(k, nt)]


@pytest.mark.parametrize("k,nt", list(rg.GEOMETRIES))
def test_ranges_are_narrow_and_every_region_is_populated(k, nt):
    w, ref = world_and_ref(k, nt)
    S = 4 ** nt
    wd, g = rg.GEOMETRIES[(k, nt)]
    assert w.ranges == [(0, S // wd), (S // wd + S // g, 2 * S // wd + S // g)]
    assert w.ranges[0][1] < w.ranges[1][0] and w.ranges[1][1] < S  # a gap between the ranks, unowned bins above them
    for r in range(2):
        sh = w.shard(r)
        assert len(sh["offsets"]) == S // wd + 1 and len(sh["pairs"]) == sh["n_pairs"] > 1000
        assert int(sh["offsets"][0]) == w.cut[r][0] and int(sh["offsets"][-1]) == w.cut[r][1]
        assert (np.diff(sh["offsets"].astype(np.int64)) >= 0).all()
        # a bin's pairs are where its offsets say: the first and the last pair of the shard lie in their bins
        b = synth.bin_key(w.kmers[[w.cut[r][0], w.cut[r][1] - 1]], k, nt).astype(np.int64) - sh["lo"]
        assert sh["offsets"][b[0]] == w.cut[r][0] and sh["offsets"][b[1] + 1] == w.cut[r][1]
    assert max(len(w.kmers), len(w.owned_kmers)) < 200_000  # (no 4^nt anywhere)
    # the reads' distinct unambiguous k-mers by region
    canon, idx = np.unique(ref.canon[ref.ambig == 0], return_index=True)
    bins = ref.bins[ref.ambig == 0][idx]
    own = w.owner_of(bins)
    n = len(canon)
    frac = {"rank0": (own == 0).sum() / n, "rank1": (own == 1).sum() / n,
            "gap": ((own < 0) & (bins < np.uint64(w.ranges[1][0]))).sum() / n, "top": (bins >= np.uint64(w.ranges[1][1])).sum() / n}
    print(k, nt, n, frac)
    assert frac["rank0"] >= 0.10 and frac["rank1"] >= 0.10 and frac["gap"] >= 0.02 and frac["top"] >= 0.20, frac


@pytest.mark.parametrize("k,nt", list(rg.GEOMETRIES))
def test_reference_calls_and_taxon_zero_are_not_vacuous(k, nt):
    w, ref = world_and_ref(k, nt)
    # taxon 0: booked misses exist, and they are fewer than the oracle's (which books the unowned ones too)
    assert 0 < ref.n_kmers[0] < ref.oracle_zero, (ref.n_kmers.get(0), ref.oracle_zero)
    assert ref.registers[0].any()
    # "not in the owned set" is what the oracle calls a miss
    miss = (ref.ambig == 0) & ~np.isin(ref.canon, w.owned_kmers)
    assert np.array_equal(miss, (ref.ambig == 0) & (ref.codes == 0))
    assert int(miss.sum()) == ref.oracle_zero
    # hits exist on both ranks, and k-mers of the whole database that nobody owns are misses here
    hit = (ref.ambig == 0) & (ref.codes != 0)
    assert (ref.owner[hit] >= 0).all() and (ref.owner[hit] == 0).any() and (ref.owner[hit] == 1).any()
    assert (np.isin(ref.canon, w.kmers) & miss).any()
    n = len(ref.calls)
    unclassified = int((ref.calls == 0).sum())
    assert unclassified >= 0.05 * n and n - unclassified >= 0.50 * n, (unclassified, n)
    called = set(ref.calls[ref.calls != 0].tolist())
    inner = called - set(w.tax.species)
    print(k, nt, "called", sorted(called), "inner", sorted(inner), "unclassified", unclassified, "of", n)
    assert len(called) >= 3 and inner


@pytest.mark.parametrize("k,nt", list(rg.GEOMETRIES))
def test_records_of_maximal_length_occur(k, nt):
    """a run of ku_route_maxn(k, nt) consecutive unambiguous k-mers of one read that share their (owned) bin: the scan cuts
    such a run into a record with the largest n the format holds"""
    w, ref = world_and_ref(k, nt)
    maxn = rg.route_maxn(k, nt)
    assert maxn == {(31, 15): 17, (31, 13): 19, (25, 13): 13}[(k, nt)]
    assert int(ref.lens.max()) - k + 1 == 128
    found = 0
    for i in range(len(ref.lens)):
        a, b = int(ref.taxa_off[i]), int(ref.taxa_off[i + 1])
        if b - a < maxn:
            continue
        ok = (ref.ambig[a:b] == 0) & (ref.owner[a:b] >= 0)
        same = ok[1:] & ok[:-1] & (ref.bins[a + 1:b] == ref.bins[a:b - 1])
        run = 0
        for s in same.tolist():
            run = run + 1 if s else 0
            if run >= maxn - 1:
                found += 1
                break
    print(k, nt, "reads with a run of", maxn, ":", found)
    assert found > 0


def test_windowed_shape_is_windowed():
    w, _ = world_and_ref(31, 13)
    reads = rg.make_reads(w, "win", 2)
    lens = np.array([len(r) for r in reads])
    assert lens.max() == 3000 and (lens == 301).sum() >= 900 and (lens == 3000).sum() >= 40


def test_classification_does_not_depend_on_the_index_nt():
    """the justification of the reference: the same k-mer set indexed at nt = 9 and at nt = 11 gives identical calls, codes,
    hit counts and per-taxon state"""
    w, ref9 = world_and_ref(31, 15)
    ref11 = rg.Reference(w, ref9.reads, oracle_nt=11)
    assert np.array_equal(ref9.calls, ref11.calls) and np.array_equal(ref9.codes, ref11.codes) and np.array_equal(ref9.hits, ref11.hits)
    assert ref9.n_reads == ref11.n_reads and ref9.n_kmers == ref11.n_kmers and ref9.oracle_zero == ref11.oracle_zero
    assert ref9.registers.keys() == ref11.registers.keys()
    for t in ref9.registers:
        assert np.array_equal(ref9.registers[t], ref11.registers[t]), t
    # ... and the quick run likewise
    q9, q11 = rg.Reference(w, ref9.reads, quick=True, min_hits=2), rg.Reference(w, ref9.reads, quick=True, min_hits=2, oracle_nt=11)
    assert np.array_equal(q9.calls, q11.calls) and np.array_equal(q9.hits, q11.hits) and q9.n_kmers == q11.n_kmers


def test_world_of_one_reference_owns_rank_zero_only():
    w, ref = world_and_ref(31, 13)
    one = rg.Reference(w, ref.reads, ranks=(0,))
    assert (one.owner <= 0).all() and (one.owner == 0).any()
    hit = (one.ambig == 0) & (one.codes != 0)
    assert hit.any() and (one.owner[hit] == 0).all()
    assert 0 < one.n_kmers[0] < ref.n_kmers[0] and not np.array_equal(one.calls, ref.calls)
