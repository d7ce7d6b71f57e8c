"""The crafted runs of the lra_bam_merger tests: what test_bam_merge_cases.py checks on the CPU and test_bam_merge_device.py merges on the device.

A run file is a BAM header (its own BGZF member unless the case says otherwise), BGZF members of a coordinate-sorted record list, and the EOF member.
A case is a list of runs (each a list of raw records, already in key order) with the window it is merged under; a case that is meant to stream has
runs whose compressed size is at least ten windows, so the merger needs at least ten rounds whatever it does."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_text as bt                                                             # noqa: E402

REF_LEN = [400_000, 300_000, 250_000]
WINDOW = 65536                                                                    # the smallest window the merger takes: compressed bytes per refill
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def fixture_records():
    """the sorter test's 5000 records: refID -1, 0, 1, 2 with many ties, names of 1 .. 254 bytes, every start alignment; behind them the 65535-op record,
    the 70000-op CG:B:I record of about 280 KB, the records above 4096 and above 65280 bytes"""
    rng = np.random.default_rng(42)
    recs = bt.random_records(rng, 4994, REF_LEN)
    recs.append(bt.make_record(0, 77, 0, b"x", [(3 << 4) | (7 if k % 3 else 2) for k in range(65535)], 100))
    recs.append(bt.cg_record(1, 500, 16, b"cgform", [(2 << 4) | (7 if k % 2 else 1) for k in range(70000)], 70000))
    recs.append(bt.make_record(2, 10, 0, b"n" * 254, [(100 << 4) | 0], 4000))
    recs.append(bt.make_record(2, 10, 16, b"m", [(100 << 4) | 0], 50_000))
    recs.append(bt.make_record(-1, -1, 4, b"u", [], 3000))
    recs.append(bt.make_record(0, 0, 0, b"z", [], 0))
    assert len(recs) == 5000
    return recs


def header_bytes(ref_len=REF_LEN, text=b"@HD\tVN:1.6\tSO:coordinate\n"):
    o = [b"BAM\x01", struct.pack("<I", len(text)), text, struct.pack("<I", len(ref_len))]
    for i, n in enumerate(ref_len):
        name = b"chr%d\0" % (i + 1)
        o += [struct.pack("<I", len(name)), name, struct.pack("<I", n)]
    return b"".join(o)


def run_bytes(recs, level=1, ref_len=REF_LEN, eof=True, cuts=None, header_member=True):
    """the bytes of a run file.  cuts: where the record stream is cut into members (default: every 65280 bytes); header_member=False: header and
    records are one stream, so the first records lie in the header's member"""
    from lra_amd import bgzf
    head, body = header_bytes(ref_len), b"".join(recs)
    if header_member:
        return bgzf.bgzf_compress(head, 6, eof=False) + (bgzf.bgzf_compress(body, level, cuts=cuts, eof=False) if body else b"") + (EOF_BLOCK if eof else b"")
    return bgzf.bgzf_compress(head + body, level, cuts=cuts, eof=eof)


def slices(recs, sizes):
    """consecutive slices of recs of the given sizes and the rest, each stable-sorted by the key: the runs a sorter makes from successive batches"""
    out, at = [], 0
    for n in list(sizes) + [len(recs) - sum(sizes)]:
        out.append(sorted(recs[at:at + n], key=bt.sort_key))
        at += n
    return out


def consecutive(recs, k):
    """k runs: slices of 0, 1, 64, 65 records (as many of them as k - 1 allows) and the rest"""
    return slices(recs, [0, 1, 64, 65][:k - 1])


def thirds(recs, k=3):
    n = len(recs) // k
    return slices(recs, [n] * (k - 1))


def one_key_runs():
    """three runs of 2000 unmapped records each: one key, distinct names"""
    return [[bt.make_record(-1, -1, 4, b"r%d_%04d" % (r, i), [], 300 + (i % 7)) for i in range(2000)] for r in range(3)]


def straddle_runs():
    """three runs in which the key (refID 0, pos 100000, forward) fills more than four windows, between records in front of it and behind it"""
    runs = []
    for r in range(3):
        a = [bt.make_record(0, 10 * i + r, 0, b"a%d_%04d" % (r, i), [(50 << 4) | 0], 300) for i in range(400)]
        b = [bt.make_record(0, 100_000, 0, b"b%d_%04d" % (r, i), [(50 << 4) | 0], 300 + (i % 5)) for i in range(700)]
        c = [bt.make_record(0, 100_001 + 10 * i, 16 if i % 2 else 0, b"c%d_%04d" % (r, i), [(50 << 4) | 0], 300) for i in range(400)]
        runs.append(a + b + c)
    return runs


def cases():
    """name -> dict(runs, window, level, stream)"""
    recs = fixture_records()
    c = {}
    for k in (1, 2, 3, 5):
        c["consecutive_%d" % k] = dict(runs=consecutive(recs, k), window=0, level=1, stream=False)
    c["streaming"] = dict(runs=thirds(recs), window=WINDOW, level=0, stream=True)
    c["one_key"] = dict(runs=one_key_runs(), window=WINDOW, level=0, stream=True)
    c["straddle"] = dict(runs=straddle_runs(), window=WINDOW, level=0, stream=True)
    c["larger"] = dict(runs=slices(recs[4000:], [500]), window=WINDOW, level=0, stream=False)      # the records of 4 and more windows are in the second run
    a, b, d, e = slices(recs[:1500], [400, 300, 500])
    c["shapes"] = dict(runs=[a, [], b, d, e], window=0, level=1, stream=False)                     # written in five shapes of file, an empty run among them
    c["small"] = dict(runs=slices(recs[:300], [120]), window=0, level=1, stream=False)             # the merge that must work after a refusal
    return c


def merged(runs):
    """the yardstick: Python's stable sort of the runs' concatenation"""
    return sorted([r for run in runs for r in run], key=bt.sort_key)
