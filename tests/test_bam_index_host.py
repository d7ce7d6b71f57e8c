"""lra_bam_index_host (no GPU): the .bai bytes of crafted coordinate-sorted BAM record streams, byte for byte against tests/bai_text.py's builder, and
region queries through the index against the brute-force overlap set.  The rules are in include/lra_hip.h and restated in bai_text's docstring."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_text as bt                                                             # noqa: E402

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from lra_amd._lib import load_library
    return load_library()


def host_index(lib, raw, ref_len, member_off, first):
    from lra_amd.bam import index_host
    return index_host(raw, ref_len, member_off, first, lib=lib)


def sized(total, ref, pos, flag, name, ops):
    """a record of exactly `total` bytes: l_seq takes (l + 1) // 2 + l bytes, which is never 1 mod 3 -- the name grows by a byte then"""
    k = total - len(bt.make_record(ref, pos, flag, name, ops, 0))
    if k % 3 == 1:
        name, k = name + b"x", k - 1
    rec = bt.make_record(ref, pos, flag, name, ops, 2 * (k // 3) + (1 if k % 3 else 0))
    assert len(rec) == total
    return rec


def both(lib, recs, ref_len, rng=None, queries=0):
    """the sorted stream of recs -> its .bai, equal from the library and from the builder; optionally the region queries"""
    raw = b"".join(sorted(recs, key=bt.sort_key))
    head, _ = bt.gzip_members(b"H" * 100)
    body, off = bt.gzip_members(raw)
    first = len(head)
    bai = host_index(lib, raw, ref_len, off, first)
    assert bai == bt.build(raw, len(ref_len), off, first)
    if queries:
        hit = bt.check_queries(rng, head + body + EOF_BLOCK, bai, raw, ref_len, queries)
        assert hit > queries // 8, "the regions must find records"
    return raw, bai


def test_zero_records(lib):
    raw, bai = both(lib, [], [1000, 2000])
    assert bai == b"BAI\x01" + (2).to_bytes(4, "little") + b"\0" * 16 + b"\0" * 8


def test_no_references_no_records(lib):
    both(lib, [], [])


def test_random_stream_and_queries(lib):
    rng = np.random.default_rng(5)
    ref_len = [3_000_000, 50_000, 1_000_000]                                      # (reference 1 may stay without records in other seeds; here all have some)
    recs = bt.random_records(rng, 1500, ref_len)
    raw, bai = both(lib, recs, ref_len, rng, 200)
    refs, n_no_coor = bt.parse(bai)
    assert n_no_coor == sum(1 for r in bt.walk(raw) if r["ref"] < 0) > 0
    assert len(raw) > 3 * bt.MEMBER


def test_reference_without_records(lib):
    rng = np.random.default_rng(6)
    recs = [r for r in bt.random_records(rng, 300, [200_000, 100_000, 300_000]) if bt.sort_key(r)[0] != 1]
    raw, bai = both(lib, recs, [200_000, 100_000, 300_000], rng, 200)
    refs, _ = bt.parse(bai)
    assert refs[1] == dict(bins={}, lin=[], meta=None) and refs[0]["meta"] and refs[2]["meta"]


def test_only_unplaced_records(lib):
    rng = np.random.default_rng(7)
    recs = bt.random_records(rng, 40, [100_000], p_unmapped=1.0)
    raw, bai = both(lib, recs, [100_000])
    refs, n = bt.parse(bai)
    assert n == 40 and refs[0]["meta"] is None


def test_record_ends_exactly_on_a_cut(lib):
    rng = np.random.default_rng(8)
    a = bt.make_record(0, 0, 0, b"first", [(100 << 4) | 0], 1000)
    b = sized(bt.MEMBER - len(a), 0, 5, 0, b"second", [(50 << 4) | 0])
    rest = [bt.make_record(0, 100 + 10 * k, 16 * (k & 1), b"r%d" % k, [(30 << 4) | 7], 50) for k in range(50)]
    recs = [a, b] + rest
    raw, bai = both(lib, recs, [100_000], rng, 200)
    assert bt.walk(raw)[1]["next"] == bt.MEMBER
    refs, _ = bt.parse(bai)
    # one bin, one run: the chunk starts at the file's first member and the record behind the cut starts at (second member, 0)
    assert all(v & 0xffff < bt.MEMBER for ch in refs[0]["bins"].values() for c in ch for v in c)


def test_record_spans_three_members(lib):
    rng = np.random.default_rng(9)
    big = bt.make_record(0, 1000, 0, b"big", [(5000 << 4) | 0], 93_000)
    assert len(big) > 2 * bt.MEMBER
    recs = [bt.make_record(0, 10 * k, 0, b"s%d" % k, [(20 << 4) | 0], 30) for k in range(60)] + [big] + \
           [bt.make_record(0, 2000 + 10 * k, 16, b"t%d" % k, [(20 << 4) | 0], 30) for k in range(60)]
    raw, bai = both(lib, recs, [100_000], rng, 200)
    w = [r for r in bt.walk(raw) if r["next"] - r["at"] == len(big)][0]
    assert w["at"] // bt.MEMBER + 2 <= (w["next"] - 1) // bt.MEMBER


def test_record_in_bin_zero(lib):
    rng = np.random.default_rng(10)
    ref_len = [1 << 27]
    across = bt.make_record(0, (1 << 26) - 10, 0, b"across", [(100 << 4) | 0], 10)
    assert bt.core(across, 0)["bin"] == 0
    recs = bt.random_records(rng, 200, ref_len, p_unmapped=0.0) + [across]
    raw, bai = both(lib, recs, ref_len, rng, 200)
    refs, _ = bt.parse(bai)
    assert 0 in refs[0]["bins"]
    rd = bt.Reader(b"".join([bt.gzip_members(b"H" * 100)[0], bt.gzip_members(raw)[0], EOF_BLOCK]), bai)
    assert across in rd.query(0, 1 << 26, (1 << 26) + 1)


def test_long_span_record_and_cg_form(lib):
    """a record of 65535 ops (the most n_cigar_op holds) and the CG:B:I form of one with 70000 ops: the span of the second is its N op's"""
    rng = np.random.default_rng(11)
    ops = [(3 << 4) | (7 if k % 3 else 2) for k in range(65535)]
    ops70 = [(2 << 4) | (7 if k % 2 else 1) for k in range(70000)]
    cg = bt.cg_record(1, 500, 16, b"cgform", ops70, 70000)
    assert bt.core(cg, 0)["end"] == 500 + 2 * 35000
    recs = [bt.make_record(0, 77, 0, b"many", ops, 100), cg] + bt.random_records(rng, 100, [400_000, 300_000])
    both(lib, recs, [400_000, 300_000], rng, 200)


def test_reference_too_long_for_bai(lib):
    rec = bt.make_record(0, 10, 0, b"x", [(10 << 4) | 0], 4)
    _, off = bt.gzip_members(rec)
    from lra_amd.bam import index_host
    index_host(rec, [1 << 29], off, 0, lib=lib)                                   # 2^29 itself is addressable
    with pytest.raises(ValueError):
        index_host(rec, [(1 << 29) + 1], off, 0, lib=lib)


def test_malformed_streams_are_refused(lib):
    from lra_amd.bam import index_host
    rec = bt.make_record(0, 10, 0, b"x", [(10 << 4) | 0], 4)
    _, off = bt.gzip_members(rec)
    with pytest.raises(ValueError):
        index_host(rec[:-1], [1000], off, 0, lib=lib)                             # cut short
    with pytest.raises(ValueError):
        index_host(rec, [], off, 0, lib=lib)                                      # refID outside the table
    with pytest.raises(ValueError):
        index_host(rec, [1000], [0, 5, 9], 0, lib=lib)                            # a member table of another stream
