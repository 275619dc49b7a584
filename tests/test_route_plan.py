"""The round planner of the owner-routed multi-GPU step (csrc/ku_route_plan.h) without a device: bin/route_plan_check plans
the rounds of one slice from the read offsets on its standard input, once over a host array and once through a batched
source that counts its fetches (what a device array costs in round trips); both are compared with the rule restated here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krakenuniq_amd", "bin", "route_plan_check")
KU_EINVAL = -1
U64 = 1 << 64


def rule(off, p0, nb, R, round_pos):
    """(status, rounds [(a, sb, ra, rn)], whether the rounds were cut by position): the rule, independent of the C++ (linear
    searches, one pass)"""
    nr = len(off)

    def cuts_of(rc):  # a round starts at its first read; one that starts behind the last read is empty
        cut = [0] + [(off[rc[i]] - p0) % U64 if rc[i] < nr else nb for i in range(1, R)] + [nb]
        return cut if all(cut[i - 1] <= cut[i] <= nb for i in range(1, R)) else None

    rc = [nr * i // R for i in range(R + 1)]
    cut = [0] + [nb] * R
    by_position = False
    if R > 1 and nr:
        cut = cuts_of(rc)
        if cut is None:
            return KU_EINVAL, [], False
        if max(cut[i + 1] - cut[i] for i in range(R)) > round_pos + round_pos // 2:
            by_position = True
            lo = [0] * R
            for i in range(1, R):
                target = p0 + nb // R * i
                first = next((j for j in range(nr) if off[j] >= target), nr)
                lo[i] = max(first, lo[i - 1])
            rc = lo + [nr]
            cut = cuts_of(rc)
            if cut is None:
                return KU_EINVAL, [], True
    return 0, [(cut[i], cut[i + 1] - cut[i], rc[i], rc[i + 1] - rc[i]) for i in range(R)], by_position


def offsets(lens, p0=0):
    out, at = [], p0
    for n in lens:
        out.append(at)
        at += n
    return out, at - p0


def run_tool(off, p0, nb, R, round_pos):
    assert os.path.exists(BIN), "build with make -C krakenuniq_amd/csrc"
    r = subprocess.run([BIN, str(p0), str(nb), str(R), str(round_pos)], input=" ".join(map(str, off)).encode(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    got, lines = {}, r.stdout.decode().splitlines()
    while lines:
        name, _, st, _, fetches = lines.pop(0).split()
        n = R if int(st) == 0 else 0
        got[name] = (int(st), [tuple(map(int, ln.split())) for ln in lines[:n]], int(fetches))
        lines = lines[n:]
    assert sorted(got) == ["batched", "host"], r.stdout.decode()
    return got


SKEWED = [150] * 25 + [100_000] + [150] * 25
CASES = {
    # name: (read lengths, p0, R, round_pos, cut by position?)
    "ten_reads_three_rounds": ([100] * 10, 0, 3, 400, False),
    "a_slice_in_mid_buffer": ([100] * 10, 123_456, 3, 400, False),
    "contig_among_short_reads": (SKEWED, 0, 6, 20_000, True),
    "contig_among_short_reads_mid_buffer": (SKEWED, 777, 6, 20_000, True),
    "target_on_a_read_offset": ([100, 400, 400, 100], 0, 2, 100, True),  # target 500 == offset of read 2
    "more_rounds_than_reads": ([100] * 3, 0, 8, 1000, False),
    "more_rounds_than_reads_by_position": ([100] * 3, 40, 8, 50, True),
    "one_long_read": ([100_000], 0, 4, 25_000, True),
    "no_reads": ([], 0, 3, 256, False),
    "one_round": ([100] * 10, 0, 1, 256, False),
    "one_round_too_wide": ([100] * 10, 0, 1, 4, False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_sources_follow_the_rule(name):
    lens, p0, R, round_pos, by_position = CASES[name]
    off, nb = offsets(lens, p0)
    st, want, took_position = rule(off, p0, nb, R, round_pos)
    assert st == 0 and took_position == by_position
    assert sum(x[1] for x in want) == nb and sum(x[3] for x in want) == len(off)  # (the restatement itself: the rounds tile the slice)
    got = run_tool(off, p0, nb, R, round_pos)
    assert got["host"][:2] == (0, want)
    assert got["batched"][:2] == (0, want)
    # one fetch for the equal-reads cuts, one per bisection step over [0, nr], one for the offsets of the reads found
    nr = len(off)
    assert got["batched"][2] <= 2 + nr.bit_length()  # ceil(log2(nr + 1))
    assert got["batched"][2] == 0 if (R == 1 or nr == 0) else got["batched"][2] >= (2 if by_position else 1)


def test_the_skewed_slice_is_cut_by_position():
    """the case the position cut is for: by reads, one round would hold the contig and eight short reads beside it"""
    off, nb = offsets(SKEWED)
    _, want, _ = rule(off, 0, nb, 6, 20_000)
    assert [x[2] for x in want] == [0, 26, 26, 26, 26, 26] and [x[2] for x in want] != [51 * i // 6 for i in range(6)]
    assert run_tool(off, 0, nb, 6, 20_000)["batched"][1] == want


def test_positions_without_reads_go_to_the_first_round():
    got = run_tool([], 0, 40, 3, 256)
    assert got["host"][1] == got["batched"][1] == [(0, 40, 0, 0), (40, 0, 0, 0), (40, 0, 0, 0)] == rule([], 0, 40, 3, 256)[1]


@pytest.mark.parametrize("off,p0,nb,R,round_pos", [
    ([0, 100, 200, 300, 400, 500, 250, 700, 800, 900], 0, 1000, 3, 400),  # read 6 lies in front of read 3
    ([0, 100, 200, 300, 400, 500, 250, 700, 800, 900], 0, 1000, 3, 100),  # (the same where the position cut would apply)
    ([100, 200, 300, 400], 100, 150, 2, 1000),                            # a cut beyond the slice's end
    ([100, 200, 300, 400], 350, 150, 2, 1000),                            # a read in front of the slice's first position
])
def test_reads_out_of_buffer_order_are_refused(off, p0, nb, R, round_pos):
    assert rule(off, p0, nb, R, round_pos)[0] == KU_EINVAL
    got = run_tool(off, p0, nb, R, round_pos)
    assert got["host"][:2] == (KU_EINVAL, []) and got["batched"][:2] == (KU_EINVAL, [])


def test_usage():
    assert subprocess.run([BIN], stderr=subprocess.PIPE).returncode == 64
    assert subprocess.run([BIN, "0", "10", "0", "5"], stdin=subprocess.DEVNULL, stderr=subprocess.PIPE).returncode == 64
