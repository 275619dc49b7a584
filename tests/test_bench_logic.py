"""bench.py's host-side planning, without a GPU: the probe table the library will lay out (the load-factor chain of
ku_ctx_set_taxonomy) and where a routed step's counter traffic comes from (profiles/route_traffic.json) -- the
one-GPU configuration lines as profiled, and the 8-GPU line of the plain `--gpus 8` flow, which no box of the pool can run."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("ku_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_planned_table_follows_the_load_factor_chain():
    b = load_bench()
    free = 280e9
    tb, lf = b.planned_table_bytes(610_000_000, free)  # configs[1]: 80 B per pair fit 40 % of the free memory
    assert lf == 0.2 and abs(tb - 610_000_000 / 1.6 * 128) < 1e6
    tb, lf = b.planned_table_bytes(3_720_000_000, free - 45e9)  # one shard of configs[2]: 0.2 does not, 0.3 does
    assert lf == 0.3 and tb < 0.85 * (free - 45e9)
    tb, lf = b.planned_table_bytes(6_000_000_000, 200e9)  # 72 GB of pairs beside 200 GB of free memory: a dense table
    assert lf == 0.6 and tb == int(6_000_000_000 / 4.8) * 128
    tb, lf = b.planned_table_bytes(24_000_000_000, 10e9)  # nothing fits: the sorted layout
    assert lf is None and tb == 24_000_000_000 * 12


def test_routed_traffic_of_the_profiled_and_of_the_full_world(tmp_path):
    b = load_bench()
    path = os.path.join(ROOT, "profiles", "route_traffic.json")
    tj = json.load(open(path))
    rev = tj["kernel_rev"]
    ent = tj["workloads"]["nt15_species96000_shards8_ws1_reads10000000_len150"]["hbm_bytes_per_step"]
    # as profiled: one rank of eight shards doing everybody's scan and resolve -- the line models the rank's share (1 / 8)
    t, note = b.routed_traffic(path, rev, 15, 96000, 8, 1, 10_000_000, 150, 1 / 8)
    assert abs(t - ((ent["scan"] + ent["resolve"]) / 8 + ent["owner"])) < 1 and "r06_config2" in note
    # the world of eight holds the layout: the same bytes, taken from the one-rank profile
    t8, note8 = b.routed_traffic(path, rev, 15, 96000, 8, 8, 10_000_000, 150, 1.0)
    assert abs(t8 - t) < 1 and "1 / 8" in note8
    # other worlds, other workloads, other kernel sources: nothing is made up
    assert b.routed_traffic(path, rev, 15, 48000, 4, 4, 10_000_000, 150, 1.0)[0] is None
    assert b.routed_traffic(path, rev, 15, 96000, 8, 2, 10_000_000, 150, 0.25)[0] is None
    t, note = b.routed_traffic(path, "000000000000", 15, 96000, 8, 8, 10_000_000, 150, 1.0)
    assert t is None and "refused" in note
    assert b.routed_traffic(str(tmp_path / "missing.json"), rev, 15, 96000, 8, 8, 10_000_000, 150, 1.0)[0] is None


def test_dump_outputs_is_a_seeded_sample_of_what_the_step_returned(tmp_path):
    """--dump-outputs on host tensors: the sampled calls and per-k-mer codes are the step's own, the per-position array and
    the kernel's runs give the same files, and two dumps of one step are identical"""
    import numpy as np
    import torch
    b = load_bench()
    k, n, L = 31, 3000, 45
    stride, nk = L + 1, L - k + 1
    g = torch.Generator().manual_seed(3)
    d_calls = torch.randint(0, 1 << 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    d_off = torch.arange(n, dtype=torch.int64) * stride
    d_len = torch.full((n,), L, dtype=torch.int32)
    per_kmer = torch.randint(-3, 3, (n, nk), generator=g, dtype=torch.int32).cumsum(1).div(4, rounding_mode="floor").to(torch.int32)  # runs of equal codes
    d_taxa = torch.zeros(n * stride, dtype=torch.int32)
    d_taxa.view(n, stride)[:, :nk] = per_kmer
    runs, roff, rcnt = [], [], []
    for r in per_kmer.tolist():
        roff.append(len(runs))
        for j, c in enumerate(r):
            if j == 0 or c != r[j - 1]:
                runs.append((c, j))
        rcnt.append(len(runs) - roff[-1])
    runs_t = (torch.tensor(runs, dtype=torch.int32), torch.tensor(roff, dtype=torch.int64), torch.tensor(rcnt, dtype=torch.int32))
    rng = np.random.default_rng(5)
    counts = {"slot_taxid": np.arange(7, dtype=np.uint32), "n_kmers": rng.integers(0, 1 << 40, 7).astype(np.uint64),
              "registers": rng.integers(0, 40, (7, 4096)).astype(np.uint8), "node_taxid": np.arange(9, dtype=np.uint32),
              "n_reads": rng.integers(0, 1000, 9).astype(np.uint64)}
    dirs = [tmp_path / "a", tmp_path / "b", tmp_path / "c"]
    b.dump_outputs(str(dirs[0]), k, d_calls, d_off, d_len, 0, n, counts, d_taxa=d_taxa)
    b.dump_outputs(str(dirs[1]), k, d_calls, d_off, d_len, 0, n, counts, d_taxa=d_taxa)
    b.dump_outputs(str(dirs[2]), k, d_calls, d_off, d_len, 0, n, counts, runs=runs_t)
    names = sorted(p.name for p in dirs[0].iterdir())
    assert names == sorted(f"{x}.npy" for x in ("read_index", "calls", "codes", "slot_taxid", "n_kmers", "node_taxid", "n_reads", "registers"))
    total = 0
    for name in names:
        x = np.load(dirs[0] / name)
        assert x.dtype in (np.float32, np.float64), name
        total += x.nbytes
        for d in dirs[1:]:
            assert np.array_equal(x, np.load(d / name)), name
    assert total <= 64 << 20
    sel = np.load(dirs[0] / "read_index.npy").astype(np.int64)
    assert len(sel) == n and (np.diff(sel) > 0).all()
    assert np.array_equal(np.load(dirs[0] / "calls.npy"), d_calls.numpy()[sel].view(np.uint32).astype(np.float64))
    assert np.array_equal(np.load(dirs[0] / "codes.npy"), per_kmer.numpy()[sel].reshape(-1).view(np.uint32).astype(np.float64))
    assert np.array_equal(np.load(dirs[0] / "n_kmers.npy"), counts["n_kmers"].astype(np.float64))
    assert np.load(dirs[0] / "registers.npy").shape == (7, 4096)
