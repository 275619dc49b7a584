"""Child process of tests/test_gpu_claim.py: one batch per instance family of the fused classify kernel, each with the waves claiming
their reads (KU_SHORT_CLAIM=3) and with the static stride (KU_SHORT_CLAIM=0), at one block per CU, under the launch recorder
(LD_PRELOAD=libku_launch_recorder.so, set by the parent for this process only).  Every run is compared with the oracle by
instances_child.run_cell -- calls, per-k-mer codes or expanded runs, n_kmers, n_reads, HLL registers, the sparse state and the
report for OUT = 2, all-zero state without counting -- so the two runs of a cell agree with each other bit for bit as well; with
counting, n_reads sums to the number of reads.  Written cell by cell to a JSON file: {cell, launched, error}.

    python tests/claim_child.py <out.json>

Not a test module: the parent starts it with a time limit, reads the file and asserts.
"""
import os
import sys
import tempfile
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import numpy as np  # noqa: E402

import instances_child as ic  # noqa: E402

_S = "ku_classify_short_kernel"
# cell -> the instance it must launch.  Cell names as in tests/kernel_instances.py: <geometry>/<shape>/<output>/<counting>
CELLS = {
    "g13/s128/codes/on": f"{_S}<2, true, 31, 13, false, 0, false>",
    "g13/s128/runs/on": f"{_S}<2, true, 31, 13, false, 1, false>",
    "g13/s128/sparse/on": f"{_S}<2, true, 31, 13, false, 2, false>",
    "g13/s128/codes/off": f"{_S}<2, false, 0, 0, false, 0, false>",
    "g13/s128/runs/off": f"{_S}<2, false, 0, 0, false, 1, false>",
    "g13/s192/codes/on": f"{_S}<3, true, 31, 13, false, 0, false>",
    "g13/s192/runs/on": f"{_S}<3, true, 31, 13, false, 1, false>",
    "g13/s192/sparse/on": f"{_S}<3, true, 31, 13, false, 2, false>",
    "g13/pairs/codes/on": f"{_S}<2, true, 31, 13, true, 0, false>",
    "g13/pairs/codes/off": f"{_S}<2, false, 0, 0, true, 0, false>",
    "g13/kbp/runs/on": f"{_S}<2, true, 31, 13, true, 1, false>",
    "g13/kbp/runs/off": f"{_S}<2, false, 0, 0, true, 1, false>",
    "e25/s128/codes/on": f"{_S}<2, true, 0, 0, false, 0, false>",
    "g15/s128/codes/on": f"{_S}<2, true, 31, 15, false, 0, false>",
}


def batch(rng, geo, shape, n):
    k = geo.k
    if shape == "s128":
        reads = [ic.frag(rng, geo.genomes, int(l)) for l in rng.integers(k, k + 128, n)]
    elif shape == "s192":
        reads = [ic.frag(rng, geo.genomes, int(l)) for l in rng.integers(160, 223, n)]
    elif shape == "pairs":
        reads = [ic.frag(rng, geo.genomes, 150) + b"N" + ic.frag(rng, geo.genomes, 150) for _ in range(n)]
    else:
        reads = [ic.frag(rng, geo.genomes, 1000) for _ in range(n)]
    for i in range(0, n, 5):  # misses among the hits
        t = bytearray(reads[i])
        t[len(t) // 2] = ord("ACGT"["ACGT".index(chr(t[len(t) // 2])) ^ 1]) if chr(t[len(t) // 2]) in "ACGT" else ord("A")
        reads[i] = bytes(t)
    reads += ic.edge_reads(rng, geo.genomes, k, max(len(r) for r in reads))
    order = rng.permutation(len(reads))
    return ic.pack([reads[i] for i in order])


def main():
    path = sys.argv[1]
    assert "libku_launch_recorder" in os.environ.get("LD_PRELOAD", ""), "run me with the recorder preloaded"
    import torch  # (before the library: one HIP runtime, torch's)
    from krakenuniq_amd import capi
    rec = ic.Recorder()
    capi.lib()
    out = ic.Out(path, rec)
    out.flush()
    n_waves = torch.cuda.get_device_properties(0).multi_processor_count * 4
    os.environ["KU_SHORT_BLOCKS_PER_CU"] = "1"
    rng = np.random.default_rng(77)
    with tempfile.TemporaryDirectory() as tmp:
        geos = {}
        for cell in CELLS:
            g, shape, _, cnt = cell.split("/")
            try:
                if g not in geos:
                    geos[g] = {"g13": lambda: ic.host_geo(31, 13, 1313, tmp), "e25": lambda: ic.host_geo(25, 13, 2513, tmp),
                               "g15": lambda: ic.bench_geo(15, 2000, 4000, 1501, tmp)}[g]()
                geo = geos[g]
                # several chunks of three per wave, a ragged end (long reads: fewer, they take windows)
                n = {"pairs": 4, "kbp": 3}.get(shape, 10) * n_waves + 2
                buf, off, lens = batch(rng, geo, shape, n)
                for mode, chunk in (("claim", "3"), ("static", "0")):
                    os.environ["KU_SHORT_CLAIM"] = chunk
                    name = f"{cell}/{mode}"
                    try:
                        ic.run_cell(out, geo, name, buf, off, lens)
                        if cnt == "on":
                            # (run_cell leaves the run's state in the context, the sparse form's too)
                            total = int(geo.ctx.counts()["n_reads"].sum())
                            assert total == len(lens), ("n_reads sums to", total, "reads", len(lens))
                    except Exception:
                        out.fail(name, traceback.format_exc(limit=6))
            except Exception:
                out.fail(cell + "/claim", traceback.format_exc(limit=6))
    out.flush()
    for c in out.cells:
        print(f"{c['cell']:32s} -> {', '.join(c['launched']) or '(none)'}{'   FAILED' if c['error'] else ''}")
    print("launches recorded:", rec.total())


if __name__ == "__main__":
    main()
