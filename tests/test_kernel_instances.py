"""CPU: the instance table (tests/kernel_instances.py) equals what the compiler emitted.

The `.kd` (kernel descriptor) symbols of the built library's gfx950 code objects name every kernel instance; the five classify
families among them must be exactly the table's rows.  An instance added to the source or removed from it fails here until
its row exists (or is gone), so the GPU matrix cannot silently miss a new one.
"""
import fnmatch
import os
import shutil
import subprocess

import pytest

import kernel_instances as ki

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "krakenuniq_amd", "libkrakenuniq_amd.so")


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name)
    if p is None:
        pytest.fail(f"{name} not found: it comes with ROCm's LLVM, which builds the library")
    return p


def compiled_instances(lib, tmp):
    """demangled names of the five families' kernels in the gfx950 code objects of `lib`"""
    # llvm-objdump --offloading writes the extracted bundles next to its input: work on a copy
    copy = os.path.join(tmp, os.path.basename(lib))
    shutil.copyfile(lib, copy)
    subprocess.run([_tool("llvm-objdump"), "--offloading", copy], check=True, stdout=subprocess.DEVNULL, cwd=tmp)
    objs = [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if f.endswith("gfx950")]
    assert objs, "no gfx950 code object in the library"
    mangled = set()
    for o in objs:
        out = subprocess.run([_tool("llvm-readelf"), "-s", "--wide", o], check=True, stdout=subprocess.PIPE, text=True).stdout
        for line in out.splitlines():
            f = line.split()
            if len(f) >= 8 and f[7].endswith(".kd"):
                mangled.add(f[7][:-3])
    cxxfilt = shutil.which("c++filt") or _tool("llvm-cxxfilt")
    dem = subprocess.run([cxxfilt], input="\n".join(sorted(mangled)) + "\n", check=True, stdout=subprocess.PIPE,
                         text=True).stdout.splitlines()
    names = set()
    for d in dem:
        if d.startswith("void "):
            d = d[5:]
        d = d[:d.rfind("(")] if "(" in d else d
        if ki.in_families(d):
            names.add(d)
    return names


def test_instance_table_equals_the_compiled_code_objects(tmp_path):
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    got = compiled_instances(LIB, str(tmp_path))
    table = [r[0] for r in ki.ROWS]
    assert len(table) == len(set(table)), "a row is listed twice"
    missing, extra = set(table) - got, got - set(table)
    for fam in ki.FAMILIES:
        print(f"{fam[:-1]}: {sum(n.startswith(fam) for n in got)} instances compiled")
    for n in sorted(missing):
        print("table row not in the code objects:", n)
    for n in sorted(extra):
        print("compiled instance without a table row:", n)
    assert not missing and not extra


def test_every_row_is_driven_or_says_why():
    cells = ki.all_cells()
    assert len(cells) == len(set(cells))
    for inst, entry, pats, reason in ki.ROWS:
        assert entry, inst
        if reason is None:
            assert pats, f"{inst}: no cell drives it and no reason is given"
        else:
            assert not pats and len(reason) > 20, inst
        for p in pats:
            assert any(fnmatch.fnmatchcase(c, p) for c in cells), f"{inst}: pattern {p!r} matches no cell of the matrix"


def test_every_cell_expects_some_instance():
    for c in ki.all_cells():
        assert ki.expected(c), c
