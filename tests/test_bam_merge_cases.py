"""The yardstick of the lra_bam_merger tests, checked on the CPU: every crafted run (tests/bam_merge_cases.py) inflates to a non-descending key sequence,
a heap merge by (key, run, ordinal) -- the tie rule: run order, then file order -- is Python's stable sort of the runs' concatenation, and a case that
is meant to stream has runs of at least ten windows of compressed bytes.  No GPU: this fails only if the cases are wrong."""
import heapq
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_text as bt                                                             # noqa: E402
import bam_merge_cases as mc                                                      # noqa: E402
import bam_text                                                                   # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return mc.cases()


def device_key(rec):
    """the merger's 64-bit key, as include/lra_hip.h states it"""
    ref, pos = struct.unpack_from("<ii", rec, 4)
    (flag,) = struct.unpack_from("<H", rec, 18)
    return ((ref & 0x7fffffff) << 33) | (((pos + 1) & 0xffffffff) << 1) | ((flag >> 4) & 1)


def split_records(raw):
    out, at = [], 0
    while at < len(raw):
        (bs,) = struct.unpack_from("<I", raw, at)
        out.append(raw[at:at + 4 + bs])
        at += 4 + bs
    assert at == len(raw)
    return out


@pytest.mark.parametrize("name", ["consecutive_1", "consecutive_2", "consecutive_3", "consecutive_5", "streaming", "one_key", "straddle", "larger", "shapes", "small"])
def test_case(cases, name):
    c = cases[name]
    head = mc.header_bytes()
    files = [mc.run_bytes(run, c["level"]) for run in c["runs"]]
    for run, f in zip(c["runs"], files):
        raw = bam_text.inflate(f)
        assert raw[:len(head)] == head
        recs = split_records(raw[len(head):])
        assert recs == run
        keys = [device_key(r) for r in recs]
        assert keys == sorted(keys), "a run descends"
        assert [bt.sort_key(r) for r in recs] == sorted(bt.sort_key(r) for r in recs)
        if c["stream"]:
            assert len(f) >= 10 * c["window"], (name, len(f))
    heap = heapq.merge(*[[(device_key(r), i, j, r) for j, r in enumerate(run)] for i, run in enumerate(c["runs"])])
    assert [t[3] for t in heap] == mc.merged(c["runs"])


def test_the_consecutive_slices_merge_into_one_sort(cases):
    recs = mc.fixture_records()
    want = sorted(recs, key=bt.sort_key)
    for k in (1, 2, 3, 5):
        runs = cases["consecutive_%d" % k]["runs"]
        assert len(runs) == k and [len(r) for r in runs[:-1]] == [0, 1, 64, 65][:k - 1]
        assert mc.merged(runs) == want


def test_the_tie_cases_are_ties(cases):
    assert len({device_key(r) for run in cases["one_key"]["runs"] for r in run}) == 1
    assert len({r for run in cases["one_key"]["runs"] for r in run}) == 6000, "distinct names"
    for run in cases["straddle"]["runs"]:
        same = [r for r in run if bt.sort_key(r) == (0, 100_000, 0)]
        assert sum(len(r) for r in same) > 4 * mc.WINDOW
