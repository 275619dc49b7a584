"""The README table "Environment knobs" is the index of the KU_* environment variables: every variable the sources read has a
row there, every row names a variable that something still reads, and the A/B switches that were retired stay retired."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krakenuniq_amd", "csrc")

# retired: the default they switched away from is the only behaviour now
RETIRED = ("KU_RLE_KERNEL_STREAMS", "KU_RLE_D2H_STREAM", "KU_RLE_SEG_MB", "KU_RLE_DEPTH", "KU_NO_POPULATE", "KU_POPULATE_MB",
           "KU_PARSE_TEAM_GZ", "KU_TOP_PAD_MB", "KU_NO_PREFETCH", "KU_NO_BGZF", "KU_SEQIO_GENERAL", "KU_MGPU_NO_RCCL")
# (the last one lives on as a flag of ku_mgpu_create, in the public header and the binding: only the variable is gone)
STILL_A_FLAG = ("KU_MGPU_NO_RCCL",)


def text_of(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def read_by_sources():
    names = set()
    for ext in ("cpp", "h", "hip"):
        for path in glob.glob(os.path.join(CSRC, "*." + ext)):
            names.update(re.findall(r'getenv\("(K[SU]_[A-Z0-9_]+)"\)', text_of(path)))
    capi = text_of(os.path.join(ROOT, "krakenuniq_amd", "capi.py"))
    names.update(re.findall(r'os\.environ(?:\.get\(|\[)"(KU_[A-Z0-9_]+)"', capi))
    names.update(re.findall(r'"(KU_[A-Z0-9_]+)" in os\.environ', capi))
    return names


def knob_table():
    """the lines of the section from its heading to the end of its table"""
    lines = text_of(os.path.join(ROOT, "README.md")).split("\n")
    at = lines.index("## Environment knobs")
    while not lines[at].startswith("|"):
        at += 1
    end = at
    while end < len(lines) and lines[end].startswith("|"):
        end += 1
    return lines[at:end]


def test_every_variable_that_is_read_is_documented():
    read = read_by_sources()
    assert len(read) > 40 and "KU_LIB" in read and "KU_HW_QUEUES" in read and "KU_DEVICE" in read, sorted(read)
    section = "\n".join(knob_table())
    missing = sorted(n for n in read if not re.search(r"(?<![A-Z0-9_])" + n + r"(?![A-Z0-9_])", section))
    assert not missing, missing


def test_every_documented_variable_is_read():
    documented = set()
    for row in knob_table()[2:]:  # (behind the header and its rule)
        documented.update(re.findall(r"`(KU_[A-Z0-9_]+)[=`]", row.split("|")[1]))
    assert len(documented) > 40, sorted(documented)
    me = os.path.abspath(__file__)
    others = [text_of(os.path.join(ROOT, "bench.py"))]
    for d, _, files in os.walk(os.path.join(ROOT, "tests")):
        others += [text_of(os.path.join(d, f)) for f in files if f.endswith((".py", ".cpp", ".h", ".hip", ".sh")) or f == "Makefile"
                   if os.path.join(d, f) != me]
    read = read_by_sources()
    stale = sorted(n for n in documented - read if not any(re.search(r"(?<![A-Z0-9_])" + n + r"(?![A-Z0-9_])", t) for t in others))
    assert not stale, stale


def test_the_retired_names_are_gone():
    found = []
    for top in ("krakenuniq_amd", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                with open(os.path.join(d, f), "rb") as fh:
                    data = fh.read()
                for n in RETIRED:
                    # a name that is still a flag may stand in the code, but not as the string an environment read would pass
                    pat = b'"' + n.encode() + b'"' if n in STILL_A_FLAG else b"(?<![A-Z0-9_])" + n.encode() + b"(?![A-Z0-9_])"
                    if re.search(pat, data):
                        found.append((os.path.relpath(os.path.join(d, f), ROOT), n))
    assert not found, found
