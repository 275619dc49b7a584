"""Every gfx950 instance of the five classify kernel families, as data.

`ku_classify_short_kernel<ITEMS, DO_COUNTS, KK, MM, WIN, OUT, ROUTE>` (ku_short.hip), `ku_lookup_kernel<MODE, LAYOUT, SHARDED,
PRIOR, ITEMS>` (ku_kernels.hip), `ku_resolve_kernel<MODE>` (ku_kernels.hip), `ku_seen_kernel<WHAT>` (ku_sparse.hip) and
`ku_route_owner_kernel<DO_COUNTS, KK, MM>` (ku_route.hip) are
compiled once per template argument list, and the launchers pick one at run time.  A bug in one instance passes every test
that launches its neighbours, so:
  - tests/test_kernel_instances.py (CPU) holds this table to the `.kd` symbols of the built library's gfx950 code objects;
  - tests/test_gpu_instances.py (-m gpu) runs every cell of MATRIX in a child process that records each kernel launch,
    asserts that a cell launches exactly the rows that name it, compares the cell's results with the oracle, and checks
    that every row not marked "not driven" was reached.

A row: the instance (demangled, as the compiler emitted it), the entry point and inputs that select it, the matrix cells
(fnmatch patterns over MATRIX) that drive it, and -- only for a row no cell drives -- the reason.

Cell names: `<group>/<shape>/<output>/<counting>` for the fused kernel, where
  group   g13: k = 31, nt = 13 (host random_db)   g15: k = 31, nt = 15 (device BenchDb, 2 000 species)
          g10: k = 31, nt = 10 (generic)          e25: k = 25, nt = 13 (selection edge: generic instance)
          p13 / p15: taxon pressure (BenchDb, >= 2 000 taxa, waves that meet > 256 slots and > 64 calls)
  shape   s128 / s129 / s192 / s193: longest read of exactly that many k-mers; win: ~3 000 k-mers (windowed);
          w65535 / w65536: the windowed limit and one past it (staged lookup + resolve);
          tiny1 / tiny3 / tiny5: batches of 1, 3, 5 reads; tinygrid: one read more than the grid has waves
  output  codes: ku_classify_batch; runs: ku_classify_batch_rle; sparse: ku_classify_batch_rle after ku_ctx_enable_sparse
          (OUT = 2 when counting); .../export and .../reset: ku_sparse_export and ku_ctx_reset_counts behind a sparse cell
  counting on, or off (KU_F_NO_COUNTS)
and `quick/...` (KU_F_QUICK, min_hits 2), `route/...` (routed ku_mgpu_step_device on two ranks of device 0, k = 31, nt = 11),
`route13/...` / `route15/...` (the same at nt = 13 / 15 over two narrow bin ranges, tests/route_geometry.py), `staged/...`
(golden f1 / f8: sorted layout, shards of the bin range, two databases, ku_lookup_stats_device).
"""
import fnmatch

GROUPS = ("g13", "g15", "g10", "e25")          # one database geometry each (p13 / p15 ride in the g13 / g15 children)
SHAPES = {"s128": 128, "s129": 129, "s192": 192, "s193": 193, "win": 3000}
OUTPUTS = ("codes", "runs", "sparse")
TINY = {"tiny1": 1, "tiny3": 3, "tiny5": 5, "tinygrid": None}  # None: the grid's wave count + 1


def _matrix():
    cells = {}
    for g in GROUPS:
        cl = []
        for s in SHAPES:
            for o in OUTPUTS:
                for c in ("on", "off"):
                    cl.append(f"{g}/{s}/{o}/{c}")
        for t in TINY:
            for o in OUTPUTS:
                cl.append(f"{g}/{t}/{o}/on")
            cl.append(f"{g}/{t}/codes/off")
        for s in ("s128", "win"):
            cl += [f"{g}/{s}/sparse/on/export", f"{g}/{s}/sparse/on/reset"]
        cells[g] = cl
    cells["g13"] += ["p13/s128/codes/on", "p13/s128/runs/on", "p13/s128/sparse/on", "g13/w65535/codes/on",
                     "g13/w65536/codes/on", "g13/w65536/codes/off", "g13/quick/codes/on", "g13/quick/codes/off"]
    cells["g15"] += ["p15/s128/codes/on", "p15/s128/runs/on", "p15/s128/sparse/on", "p15/win/codes/on"]
    cells["route"] = ["route/s128/codes/on", "route/s128/codes/off", "route/win/codes/on", "route/win/codes/off",
                      "route13/s128/codes/on", "route13/s128/codes/off", "route15/s128/codes/on", "route15/s128/codes/off"]
    cells["staged"] = ["staged/sorted/codes/on", "staged/sorted/codes/off", "staged/shard/codes/on", "staged/shard/codes/off",
                       "staged/shard/resolve/on", "staged/prior/codes/on", "staged/prior/codes/off",
                       "staged/prior_sorted/codes/on", "staged/prior_sorted/codes/off", "staged/stats"]
    return cells


# child process (one database geometry each) -> its cells, in the order they run
MATRIX = _matrix()

_S = "ku_classify_short_kernel"
_NOT_ROUTED_RUNS = ("no entry point passes run output to ku_launch_route_resolve: the routed step's resolve stage writes per-k-mer "
                    "codes (ku_ctx_route_resolve), and its runs come from ku_rle_kernel afterwards")

# (instance, entry point + what selects it, cells, reason when not driven)
ROWS = [
    # ---- one pass, <= 128 k-mers (ITEMS = 2)
    (f"{_S}<2, true, 31, 13, false, 0, false>", "classify_batch; k31 nt13; longest <= 128 k-mers; counting",
     ("g13/s128/codes/on", "g13/tiny*/codes/on", "p13/s128/codes/on"), None),
    (f"{_S}<2, true, 31, 13, false, 1, false>", "classify_batch_rle; k31 nt13; <= 128; counting",
     ("g13/s128/runs/on", "g13/tiny*/runs/on", "p13/s128/runs/on"), None),
    (f"{_S}<2, true, 31, 13, false, 2, false>", "classify_batch_rle + enable_sparse; k31 nt13; <= 128; counting",
     ("g13/s128/sparse/on", "g13/tiny*/sparse/on", "p13/s128/sparse/on"), None),
    (f"{_S}<2, true, 31, 15, false, 0, false>", "classify_batch; k31 nt15; <= 128; counting",
     ("g15/s128/codes/on", "g15/tiny*/codes/on", "p15/s128/codes/on"), None),
    (f"{_S}<2, true, 31, 15, false, 1, false>", "classify_batch_rle; k31 nt15; <= 128; counting",
     ("g15/s128/runs/on", "g15/tiny*/runs/on", "p15/s128/runs/on"), None),
    (f"{_S}<2, true, 31, 15, false, 2, false>", "classify_batch_rle + enable_sparse; k31 nt15; <= 128; counting",
     ("g15/s128/sparse/on", "g15/tiny*/sparse/on", "p15/s128/sparse/on"), None),
    (f"{_S}<2, true, 0, 0, false, 0, false>", "classify_batch; any other geometry; <= 128; counting",
     ("g10/s128/codes/on", "e25/s128/codes/on", "g10/tiny*/codes/on", "e25/tiny*/codes/on"), None),
    (f"{_S}<2, true, 0, 0, false, 1, false>", "classify_batch_rle; other geometry; <= 128; counting",
     ("g10/s128/runs/on", "e25/s128/runs/on", "g10/tiny*/runs/on", "e25/tiny*/runs/on"), None),
    (f"{_S}<2, true, 0, 0, false, 2, false>", "classify_batch_rle + enable_sparse; other geometry; <= 128; counting",
     ("g10/s128/sparse/on", "e25/s128/sparse/on", "g10/tiny*/sparse/on", "e25/tiny*/sparse/on"), None),
    (f"{_S}<2, false, 0, 0, false, 0, false>", "classify_batch; any geometry; <= 128; KU_F_NO_COUNTS",
     ("[gep]*/s128/codes/off", "[gep]*/tiny*/codes/off"), None),
    (f"{_S}<2, false, 0, 0, false, 1, false>", "classify_batch_rle (sparse or not); any geometry; <= 128; KU_F_NO_COUNTS",
     ("[gep]*/s128/runs/off", "[gep]*/s128/sparse/off"), None),
    # ---- one pass, 129-192 k-mers (ITEMS = 3)
    (f"{_S}<3, true, 31, 13, false, 0, false>", "classify_batch; k31 nt13; longest 129-192 k-mers; counting",
     ("g13/s129/codes/on", "g13/s192/codes/on"), None),
    (f"{_S}<3, true, 31, 13, false, 1, false>", "classify_batch_rle; k31 nt13; 129-192; counting",
     ("g13/s129/runs/on", "g13/s192/runs/on"), None),
    (f"{_S}<3, true, 31, 13, false, 2, false>", "classify_batch_rle + enable_sparse; k31 nt13; 129-192; counting",
     ("g13/s129/sparse/on", "g13/s192/sparse/on"), None),
    (f"{_S}<3, true, 31, 15, false, 0, false>", "classify_batch; k31 nt15; 129-192; counting",
     ("g15/s129/codes/on", "g15/s192/codes/on"), None),
    (f"{_S}<3, true, 31, 15, false, 1, false>", "classify_batch_rle; k31 nt15; 129-192; counting",
     ("g15/s129/runs/on", "g15/s192/runs/on"), None),
    (f"{_S}<3, true, 31, 15, false, 2, false>", "classify_batch_rle + enable_sparse; k31 nt15; 129-192; counting",
     ("g15/s129/sparse/on", "g15/s192/sparse/on"), None),
    (f"{_S}<3, true, 0, 0, false, 0, false>", "classify_batch; other geometry; 129-192; counting",
     ("g10/s129/codes/on", "g10/s192/codes/on", "e25/s129/codes/on", "e25/s192/codes/on"), None),
    (f"{_S}<3, true, 0, 0, false, 1, false>", "classify_batch_rle; other geometry; 129-192; counting",
     ("g10/s129/runs/on", "g10/s192/runs/on", "e25/s129/runs/on", "e25/s192/runs/on"), None),
    (f"{_S}<3, true, 0, 0, false, 2, false>", "classify_batch_rle + enable_sparse; other geometry; 129-192; counting",
     ("g10/s129/sparse/on", "g10/s192/sparse/on", "e25/s129/sparse/on", "e25/s192/sparse/on"), None),
    (f"{_S}<3, false, 0, 0, false, 0, false>", "classify_batch; any geometry; 129-192; KU_F_NO_COUNTS",
     ("[gep]*/s129/codes/off", "[gep]*/s192/codes/off"), None),
    (f"{_S}<3, false, 0, 0, false, 1, false>", "classify_batch_rle (sparse or not); any geometry; 129-192; KU_F_NO_COUNTS",
     ("[gep]*/s129/runs/off", "[gep]*/s192/runs/off", "[gep]*/s129/sparse/off", "[gep]*/s192/sparse/off"), None),
    # ---- windowed, 193-65535 k-mers (ITEMS = 2, WIN)
    (f"{_S}<2, true, 31, 13, true, 0, false>", "classify_batch; k31 nt13; longest 193-65535 k-mers; counting",
     ("g13/s193/codes/on", "g13/win/codes/on", "g13/w65535/codes/on"), None),
    (f"{_S}<2, true, 31, 13, true, 1, false>", "classify_batch_rle; k31 nt13; windowed; counting",
     ("g13/s193/runs/on", "g13/win/runs/on"), None),
    (f"{_S}<2, true, 31, 13, true, 2, false>", "classify_batch_rle + enable_sparse; k31 nt13; windowed; counting",
     ("g13/s193/sparse/on", "g13/win/sparse/on"), None),
    (f"{_S}<2, true, 31, 15, true, 0, false>", "classify_batch; k31 nt15; windowed; counting",
     ("g15/s193/codes/on", "g15/win/codes/on", "p15/win/codes/on"), None),
    (f"{_S}<2, true, 31, 15, true, 1, false>", "classify_batch_rle; k31 nt15; windowed; counting",
     ("g15/s193/runs/on", "g15/win/runs/on"), None),
    (f"{_S}<2, true, 31, 15, true, 2, false>", "classify_batch_rle + enable_sparse; k31 nt15; windowed; counting",
     ("g15/s193/sparse/on", "g15/win/sparse/on"), None),
    (f"{_S}<2, true, 0, 0, true, 0, false>", "classify_batch; other geometry; windowed; counting",
     ("g10/s193/codes/on", "g10/win/codes/on", "e25/s193/codes/on", "e25/win/codes/on"), None),
    (f"{_S}<2, true, 0, 0, true, 1, false>", "classify_batch_rle; other geometry; windowed; counting",
     ("g10/s193/runs/on", "g10/win/runs/on", "e25/s193/runs/on", "e25/win/runs/on"), None),
    (f"{_S}<2, true, 0, 0, true, 2, false>", "classify_batch_rle + enable_sparse; other geometry; windowed; counting",
     ("g10/s193/sparse/on", "g10/win/sparse/on", "e25/s193/sparse/on", "e25/win/sparse/on"), None),
    (f"{_S}<2, false, 0, 0, true, 0, false>", "classify_batch; any geometry; windowed; KU_F_NO_COUNTS",
     ("[gep]*/s193/codes/off", "[gep]*/win/codes/off"), None),
    (f"{_S}<2, false, 0, 0, true, 1, false>", "classify_batch_rle (sparse or not); any geometry; windowed; KU_F_NO_COUNTS",
     ("[gep]*/s193/runs/off", "[gep]*/win/runs/off", "[gep]*/s193/sparse/off", "[gep]*/win/sparse/off"), None),
    # ---- resolve stage of the owner-routed step (ROUTE): ku_mgpu_step_device, KU_MGPU_EXCHANGE=route
    (f"{_S}<2, true, 0, 0, false, 0, true>", "routed step; longest <= 128 k-mers; counting",
     ("route/s128/codes/on", "route1[35]/s128/codes/on"), None),
    (f"{_S}<2, false, 0, 0, false, 0, true>", "routed step; <= 128; KU_F_NO_COUNTS",
     ("route/s128/codes/off", "route1[35]/s128/codes/off"), None),
    (f"{_S}<2, true, 0, 0, true, 0, true>", "routed step; 129-65535 k-mers; counting", ("route/win/codes/on",), None),
    (f"{_S}<2, false, 0, 0, true, 0, true>", "routed step; 129-65535; KU_F_NO_COUNTS", ("route/win/codes/off",), None),
    (f"{_S}<2, true, 0, 0, false, 1, true>", "ku_launch_route_resolve with runs_out; <= 128; counting", (), _NOT_ROUTED_RUNS),
    (f"{_S}<2, false, 0, 0, false, 1, true>", "ku_launch_route_resolve with runs_out; <= 128; no counts", (), _NOT_ROUTED_RUNS),
    (f"{_S}<2, true, 0, 0, true, 1, true>", "ku_launch_route_resolve with runs_out; windowed; counting", (), _NOT_ROUTED_RUNS),
    (f"{_S}<2, false, 0, 0, true, 1, true>", "ku_launch_route_resolve with runs_out; windowed; no counts", (), _NOT_ROUTED_RUNS),
    # ---- staged lookup (MODE 0: slots, 1: slots + counting, 2: probe statistics, 3: route scan; LAYOUT 1 = hash table)
    ("ku_lookup_kernel<1, 1, false, false, 1>", "staged path, hash layout, whole bin range, counting: reads past 65535 k-mers",
     ("g13/w65536/codes/on",), None),
    ("ku_lookup_kernel<0, 1, false, false, 1>", "as above without counting: KU_F_NO_COUNTS, quick mode (counted in its resolve "
     "stage), the first database of two (the last one counts)",
     ("g13/quick/codes/*", "g13/w65536/codes/off", "staged/prior/codes/*"), None),
    ("ku_lookup_kernel<1, 1, true, false, 1>", "hash layout, a shard of the bin range, counting", ("staged/shard/codes/on",), None),
    ("ku_lookup_kernel<0, 1, true, false, 1>", "hash layout, shard, KU_F_NO_COUNTS", ("staged/shard/codes/off",), None),
    ("ku_lookup_kernel<1, 0, true, false, 1>", "KU_LAYOUT=sorted, counting", ("staged/sorted/codes/on",), None),
    ("ku_lookup_kernel<0, 0, true, false, 1>", "KU_LAYOUT=sorted, KU_F_NO_COUNTS, or the first database of two",
     ("staged/sorted/codes/off", "staged/prior_sorted/codes/*"), None),
    ("ku_lookup_kernel<1, 1, false, true, 1>", "second database (prior), hash layout, counting", ("staged/prior/codes/on",), None),
    ("ku_lookup_kernel<0, 1, false, true, 1>", "second database, hash layout, KU_F_NO_COUNTS", ("staged/prior/codes/off",), None),
    ("ku_lookup_kernel<1, 0, true, true, 1>", "second database, sorted layout, counting", ("staged/prior_sorted/codes/on",), None),
    ("ku_lookup_kernel<0, 0, true, true, 1>", "second database, sorted layout, KU_F_NO_COUNTS",
     ("staged/prior_sorted/codes/off",), None),
    ("ku_lookup_kernel<2, 0, true, false, 1>", "ku_lookup_stats_device (bench.py's probe statistics)", ("staged/stats",), None),
    ("ku_lookup_kernel<3, 1, true, false, 2>", "route scan of the routed step", ("route/*", "route1[35]/*"), None),
    # ---- staged resolve (MODE 0: <= 384 k-mers, 1: <= 12 288, 2: longer); the quick path has a kernel of its own
    ("ku_resolve_kernel<0>", "staged path, every read up to 384 k-mers",
     ("g13/w65536/codes/*", "staged/sorted/codes/*", "staged/shard/resolve/on", "staged/prior*/codes/*"), None),
    ("ku_resolve_kernel<1>", "staged path, reads of 385-12 288 k-mers", ("g13/w65536/codes/*",), None),
    ("ku_resolve_kernel<2>", "staged path, reads past 12 288 k-mers", ("g13/w65536/codes/*",), None),
    # ---- the owner of the routed step (DO_COUNTS, KK, MM; 0, 0 = any other geometry)
    ("ku_route_owner_kernel<true, 31, 13>", "routed step; k31 nt13; counting", ("route13/s128/codes/on",), None),
    ("ku_route_owner_kernel<false, 31, 13>", "routed step; k31 nt13; KU_F_NO_COUNTS", ("route13/s128/codes/off",), None),
    ("ku_route_owner_kernel<true, 31, 15>", "routed step; k31 nt15; counting", ("route15/s128/codes/on",), None),
    ("ku_route_owner_kernel<false, 31, 15>", "routed step; k31 nt15; KU_F_NO_COUNTS", ("route15/s128/codes/off",), None),
    ("ku_route_owner_kernel<true, 0, 0>", "routed step; any other geometry; counting", ("route/*/codes/on",), None),
    ("ku_route_owner_kernel<false, 0, 0>", "routed step; other geometry; KU_F_NO_COUNTS (quick mode too: it counts in its resolve stage)",
     ("route/*/codes/off",), None),
    # ---- SEEN marks of the probe table (sparse fast path)
    ("ku_seen_kernel<0>", "ku_sparse_export after an OUT = 2 batch: count the marks", ("*/sparse/on/export",), None),
    ("ku_seen_kernel<1>", "ku_sparse_export after an OUT = 2 batch: insert the marks into the run-wide set",
     ("*/sparse/on/export",), None),
    ("ku_seen_kernel<2>", "ku_ctx_reset_counts after an OUT = 2 batch: clear the marks", ("*/sparse/on/reset",), None),
]

FAMILIES = ("ku_classify_short_kernel<", "ku_lookup_kernel<", "ku_resolve_kernel<", "ku_seen_kernel<", "ku_route_owner_kernel<")


def all_cells():
    return [c for cl in MATRIX.values() for c in cl]


def expected(cell):
    """the instances a cell must launch: every row with a pattern that matches it"""
    return {r[0] for r in ROWS if any(fnmatch.fnmatchcase(cell, p) for p in r[2])}


def driven():
    return {r[0] for r in ROWS if r[3] is None}


def in_families(name):
    return name.startswith(FAMILIES)
