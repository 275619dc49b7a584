"""-m gpu: the owner-routed step (ku_mgpu_step_device) at the geometries its owner kernel has instances for, with bins that
nobody owns, against the oracle (tests/route_geometry.py; tests/test_route_geometry_model.py holds that reference to its
conditions).  Two ranks share device 0; every cell compares the calls per rank slice, the per-k-mer codes at the valid
positions and, after ku_mgpu_reduce_state, n_reads / n_kmers / HLL registers bit for bit (all zero under KU_F_NO_COUNTS).

  a  (31,15), (31,13), (25,13) x counting on / off: ku_route_owner_kernel<true|false, 31,15 | 31,13 | 0,0>; at (31,15) two steps
     with different batches on one group (queues, cursors and the owners' counters reused)
  b  the windowed ROUTE resolve (mate pairs 150 + N + 150, reads of 3 kbp)
  c  the unfused return, ku_route_gather_kernel + resolve: KU_NO_FUSED=1, an unknown read length, quick mode
  d  a world of one rank under KU_MGPU_FORCE_ROUTE=1 (what bench.py's single-rank route profile runs)
  e  KU_ROUTE_CAP: queues that overflow into the second pass, caps that are no multiple of the prefix kernels' 1024-record
     tile, and a queue buffer of more than 4096 tiles, nearly all of them unused
"""
import pytest

import route_geometry as rg
from krakenuniq_amd import capi

pytestmark = pytest.mark.gpu

_worlds, _reads, _refs = {}, {}, {}


def world(k, nt):
    if (k, nt) not in _worlds:
        _worlds[(k, nt)] = rg.World(k, nt)
    return _worlds[(k, nt)]


def reads(k, nt, shape, seed=1):
    key = (k, nt, shape, seed)
    if key not in _reads:
        _reads[key] = rg.make_reads(world(k, nt), shape, seed)
    return _reads[key]


def reference(k, nt, shape, seeds=(1,), **kw):
    """the oracle over the batches `seeds` of a shape, one after the other in one run (computed once, shared)"""
    key = (k, nt, shape, seeds, tuple(sorted(kw.items())))
    if key not in _refs:
        _refs[key] = rg.Reference(world(k, nt), [r for s in seeds for r in reads(k, nt, shape, s)], **kw)
    return _refs[key]


def run_cell(k, nt, shape, flags=0, min_hits=1, max_read_len=None, n_ranks=2, seeds=(1,), codes=True, **ref_kw):
    if ref_kw.get("quick"):
        ref_kw["min_hits"] = min_hits
    ref = reference(k, nt, shape, seeds, **ref_kw)
    routed = rg.Routed(world(k, nt), n_ranks)
    try:
        first = 0
        for s in seeds:
            up = routed.upload(reads(k, nt, shape, s))
            routed.step(up, flags=flags, min_hits=min_hits, max_read_len=max_read_len)
            rg.assert_step(routed, up, ref, first, codes=codes)
            first += up["N"]
        counts = routed.counts()
        if flags & capi.KU_F_NO_COUNTS:
            rg.assert_zero_state(counts)
        else:
            rg.assert_counts(counts, ref)
    finally:
        routed.close()


@pytest.mark.parametrize("counting", ["on", "off"])
@pytest.mark.parametrize("k,nt", list(rg.GEOMETRIES))
def test_owner_instances_with_unowned_bins(k, nt, counting):
    """a: the six owner instances; (31,15) counting runs two different batches through one group"""
    seeds = (1, 2) if (k, nt, counting) == (31, 15, "on") else (1,)
    run_cell(k, nt, "short", flags=0 if counting == "on" else capi.KU_F_NO_COUNTS, seeds=seeds)


@pytest.mark.parametrize("k,nt", [(31, 15), (31, 13)])
def test_windowed_route_resolve_with_unowned_bins(k, nt):
    """b"""
    run_cell(k, nt, "win")


@pytest.mark.parametrize("how", ["no_fused", "unknown_len", "quick"])
def test_unfused_return_with_unowned_bins(how, monkeypatch):
    """c: tickets -> slots by ku_route_gather_kernel (KU_ROUTE_MISS -> slot 0), the resolve kernels behind the last round.
    Quick mode: the oracle's quick run; the step has no hit-count output, so calls and the per-taxon state are compared (quick
    mode books a read's scanned prefix where the read is resolved, misses under taxon 0 whoever owns them: the oracle's taxon 0)"""
    if how == "no_fused":
        monkeypatch.setenv("KU_NO_FUSED", "1")
        run_cell(31, 15, "short")
    elif how == "unknown_len":
        run_cell(31, 15, "short", max_read_len=0)
    else:
        run_cell(31, 15, "short", flags=capi.KU_F_QUICK, min_hits=2, codes=False, quick=True)


def test_world_of_one_forced_through_the_routed_step(monkeypatch):
    """d: one owned range, every other bin unowned"""
    monkeypatch.setenv("KU_MGPU_FORCE_ROUTE", "1")
    run_cell(31, 13, "short", n_ranks=1, ranks=(0,))


@pytest.mark.parametrize("cap", [256, 768, 1280, 2200064])
def test_queue_capacities(cap, monkeypatch):
    """e: two ranks claim 256 records at a time.  256, 768, 1280 overflow (second pass with queues of the counted size); 768 and
    1280 are no multiple of the 1024-record prefix tile; 2 x 2200064 records are 4297 tiles (> 4096: the second trip of
    ku_route_prefix_blocks_kernel, whose carry the grand total in kb[n_rec] needs), almost all wholly unused.  (The second
    queue starts in tile 2148 there, so every record that is read lies in front of tile 4096: the carry reaches the result
    through the total only, not through a record's number.)"""
    assert cap % 256 == 0 and (2 * 2200064 + 1023) // 1024 == 4297
    monkeypatch.setenv("KU_ROUTE_CAP", str(cap))
    run_cell(31, 13, "short")
