"""-m gpu: every instance of the classify kernel families against the oracle, with proof of which instance each cell reached.

The cells of tests/kernel_instances.MATRIX run in child processes, one per database geometry, one after another
(tests/instances_child.py).  Each child preloads the launch recorder (tests/rccl_shim/libku_launch_recorder.so: hipLaunchKernel
noted by name, then forwarded), so a cell knows the kernel instances it launched.  Here:
  - every cell compared with the oracle without error (calls, per-k-mer codes or runs, quick hit counts, per-taxon n_kmers /
    n_reads / HLL registers, the sparse state and report for OUT = 2, all-zero state without counting);
  - every cell launched exactly the instances whose rows name it;
  - the union over all cells covers every row not marked "not driven".
A child that ends on a signal or its time limit fails its test, and no further child is started.
"""
import json
import os
import subprocess
import sys

import pytest

import kernel_instances as ki

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REC = os.path.join(HERE, "rccl_shim", "libku_launch_recorder.so")
LIMITS = {"g13": 240, "g15": 300, "g10": 150, "e25": 150, "route": 150, "staged": 120}  # seconds per child
_state = {"stop": None, "reached": {}}


def run_child(group, tmp_path):
    if _state["stop"]:
        pytest.fail(f"not started: the child of {_state['stop']} ended abnormally")
    assert os.path.exists(REC), "build the test libraries first (__graft_entry__.build())"
    out = tmp_path / f"{group}.json"
    env = {**os.environ, "LD_PRELOAD": REC + (":" + os.environ["LD_PRELOAD"] if os.environ.get("LD_PRELOAD") else "")}
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "instances_child.py"), group, str(out)], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LIMITS[group])
    except subprocess.TimeoutExpired as e:
        _state["stop"] = group
        pytest.fail(f"child {group} exceeded {LIMITS[group]} s:\n{(e.stdout or '')[-3000:] if isinstance(e.stdout, str) else ''}")
    print(p.stdout[-20000:])
    if p.returncode < 0:
        _state["stop"] = group
        pytest.fail(f"child {group} ended on signal {-p.returncode}")
    assert p.returncode == 0, p.stdout[-4000:]
    res = json.loads(out.read_text())
    errs = [c for c in res["cells"] if c["error"]]
    if errs:
        print(f"first failing cell {errs[0]['cell']}:\n{errs[0]['error']}")
    assert res["rec_total"] > 0, "the recorder saw no launch: hipLaunchKernel was not interposed"
    return res["cells"]


@pytest.mark.parametrize("group", list(ki.MATRIX))
def test_cells_reach_their_instances_and_match_the_oracle(group, tmp_path):
    cells = run_child(group, tmp_path)
    seen = {c["cell"]: c for c in cells}
    errors, wrong = [], []
    for name in ki.MATRIX[group]:
        c = seen.get(name)
        if c is None:
            errors.append(f"{name}: did not run")
            continue
        if c["error"]:
            errors.append(f"{name}:\n{c['error']}")
        want = ki.expected(name)
        if set(c["launched"]) != want:
            wrong.append(f"{name}: launched {sorted(c['launched'])}, its rows are {sorted(want)}")
        _state["reached"].update({n: name for n in c["launched"]})
    assert not wrong and not errors, "\n".join(wrong + errors)


def test_every_driven_row_was_reached():
    if set(_state["reached"]) == set() or _state["stop"]:
        pytest.fail("the matrix did not run to the end in this session")
    missing = ki.driven() - set(_state["reached"])
    assert not missing, sorted(missing)
    for r in ki.ROWS:
        if r[3] is not None:
            print(f"not driven: {r[0]}: {r[3]}")
