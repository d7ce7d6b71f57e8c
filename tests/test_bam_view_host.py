"""lra_bai_query_host (no GPU): the chunk plan of a region from the bytes of a .bai index, against a Python restatement of the planner's rules and against
the records a brute-force walk finds; the edges of the rules; every index the reader refuses, whole and cut at every field boundary."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_text as bt                                                             # noqa: E402

REF_LEN = [400_000, 300_000, 250_000]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from lra_amd._lib import load_library
    return load_library()


def query(lib, bai, n_ref, ref, beg, end):
    from lra_amd.bam import bai_query
    return bai_query(bai, n_ref, ref, beg, end, lib=lib)


def refused(lib, bai, n_ref=-1, ref=0, beg=0, end=1):
    try:
        query(lib, bai, n_ref, ref, beg, end)
    except ValueError:
        return True
    return False


def indexed(recs, n_ref):
    recs = sorted(recs, key=bt.sort_key)
    raw = b"".join(recs)
    _, moff = bt.gzip_members(raw)
    return raw, moff, bt.build(raw, n_ref, moff)


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(7)
    raw, moff, bai = indexed(bt.random_records(rng, 5000, REF_LEN), 3)
    return dict(raw=raw, moff=moff, bai=bai, recs=bt.walk(raw), refs=bt.parse(bai)[0])


def plan_py(refs, ref, beg, end):
    """the planner's rules: reg2bins' bins; min_off = lin[beg >> 14], empty behind the last window; starts clipped, emptied chunks dropped; sorted and merged"""
    R = refs[ref]
    if beg >= end or (beg >> 14) >= len(R["lin"]):
        return []
    min_off = R["lin"][beg >> 14]
    ch = sorted((max(cb, min_off), ce) for b in bt.reg2bins(beg, end) for cb, ce in R["bins"].get(b, ()) if max(cb, min_off) < ce)
    out = []
    for b, e in ch:
        if out and b <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([b, e])
    return [tuple(c) for c in out]


def check_plan(lib, D, n_ref, ref, beg, end):
    plan = query(lib, D["bai"], n_ref, ref, beg, end)
    assert all(b < e for b, e in plan) and all(plan[i][1] < plan[i + 1][0] for i in range(len(plan) - 1)), (ref, beg, end, plan)
    lin = D["refs"][ref]["lin"]
    if plan:
        assert all(b >= lin[beg >> 14] for b, _ in plan)
    assert plan == plan_py(D["refs"], ref, beg, end), (ref, beg, end)
    hits = 0
    for r in D["recs"]:
        if r["ref"] == ref and r["pos"] < end and r["end"] > beg:
            v = bt.voff(r["at"], D["moff"], 0)
            assert any(b <= v < e for b, e in plan), (ref, beg, end, r)
            hits += 1
    return hits


def regions(rng, recs, ref_len, n=200):
    """as bai_text.check_queries chooses them: half around a record, half anywhere"""
    for k in range(n):
        ref = int(rng.integers(0, len(ref_len)))
        beg = int(rng.integers(0, ref_len[ref]))
        if k % 2 and recs:
            r = recs[int(rng.integers(0, len(recs)))]
            if r["ref"] >= 0:
                ref = r["ref"]
                beg = max(0, r["pos"] - int(rng.integers(0, 20000)))
        end = min(ref_len[ref], beg + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 22)))))
        yield ref, beg, end


def test_random_regions(lib, big):
    rng = np.random.default_rng(11)
    hit = sum(bool(check_plan(lib, big, 3, ref, beg, end)) for ref, beg, end in regions(rng, big["recs"], REF_LEN))
    assert hit >= 50


def test_edges_of_the_region(lib, big):
    for ref, n in enumerate(REF_LEN):
        assert check_plan(lib, big, 3, ref, 0, n) > 0
        check_plan(lib, big, 3, ref, 0, 1)
        check_plan(lib, big, 3, ref, n - 1, n)
        for p in (0, 16384, n // 2, n):
            assert query(lib, big["bai"], 3, ref, p, p) == []                     # beg == end: nothing overlaps
    n_intv = len(big["refs"][0]["lin"])
    assert query(lib, big["bai"], 3, 0, n_intv << 14, (n_intv << 14) + 100) == []   # a window behind the last touched one
    assert query(lib, big["bai"], 3, 0, (n_intv << 14) - 1, (n_intv << 14) + 100) == plan_py(big["refs"], 0, (n_intv << 14) - 1, (n_intv << 14) + 100)
    assert query(lib, big["bai"], -1, 0, 0, 1000) == query(lib, big["bai"], 3, 0, 0, 1000)   # n_ref < 0: not compared
    for bad in ((3, 0, 10), (-1, 0, 10), (0, 10, 9), (0, -1, 5)):
        assert refused(lib, big["bai"], 3, *bad), bad
    assert refused(lib, big["bai"], 2) and refused(lib, big["bai"], 4)            # the index of another reference table


def test_reference_without_records(lib):
    rng = np.random.default_rng(3)
    recs = [r for r in bt.random_records(rng, 300, REF_LEN) if struct.unpack_from("<i", r, 4)[0] != 1]
    raw, moff, bai = indexed(recs, 3)
    D = dict(raw=raw, moff=moff, bai=bai, recs=bt.walk(raw), refs=bt.parse(bai)[0])
    assert D["refs"][1]["bins"] == {} and D["refs"][1]["lin"] == []
    assert query(lib, bai, 3, 1, 0, REF_LEN[1]) == []
    assert check_plan(lib, D, 3, 0, 0, REF_LEN[0]) > 0


def test_bin_zero_and_chunks_that_merge(lib):
    ref_len = [1 << 28]
    cross = (1 << 26) - 500
    recs = [bt.make_record(0, 100 + 7 * i, 0, b"a%d" % i, [(50 << 4) | 0], 20) for i in range(30)]
    recs += [bt.make_record(0, cross, 0, b"cross", [(1000 << 4) | 0], 30)]      # crosses 2^26: bin 0
    recs += [bt.make_record(0, cross + 100 + i, 16, b"b%d" % i, [(40 << 4) | 0], 20) for i in range(30)]
    # a record of a wider bin between records of the narrowest one: three runs whose chunks touch end to start
    recs += [bt.make_record(0, (1 << 27) + 16000, 0, b"n1", [(100 << 4) | 0], 10), bt.make_record(0, (1 << 27) + 16300, 0, b"wide", [(200 << 4) | 0], 10),
             bt.make_record(0, (1 << 27) + 16400, 0, b"n2", [(100 << 4) | 0], 10)]
    raw, moff, bai = indexed(recs, 1)
    D = dict(raw=raw, moff=moff, bai=bai, recs=bt.walk(raw), refs=bt.parse(bai)[0])
    assert 0 in D["refs"][0]["bins"]
    assert check_plan(lib, D, 1, 0, (1 << 26) - 10, (1 << 26) + 10) >= 1          # found through bin 0
    assert check_plan(lib, D, 1, 0, (1 << 26) + 400, (1 << 26) + 401) >= 1
    a, b = (1 << 27) + 16000, (1 << 27) + 16600
    raw_chunks = [c for bn in bt.reg2bins(a, b) for c in D["refs"][0]["bins"].get(bn, ())]
    plan = query(lib, bai, 1, 0, a, b)
    assert len(raw_chunks) >= 3 and len(plan) == 1, (raw_chunks, plan)           # two bins' chunks, touching, are one chunk of the plan
    assert check_plan(lib, D, 1, 0, a, b) == 3
    check_plan(lib, D, 1, 0, 0, 1 << 28)
    assert query(lib, bai, 1, 0, 0, 1 << 40) == query(lib, bai, 1, 0, 0, 1 << 29)   # end above what the bins address


def boundaries(bai):
    """the offsets at which a field of the index starts or ends (a count that is negative ends the walk)"""
    at, out = 8, [0, 4, 8]
    (n_ref,) = struct.unpack_from("<i", bai, 4)
    for _ in range(max(n_ref, 0)):
        if at + 4 > len(bai):
            return out
        (n_bin,) = struct.unpack_from("<i", bai, at); at += 4; out.append(at)
        for _ in range(max(n_bin, 0)):
            if at + 8 > len(bai):
                return out
            _, n_chunk = struct.unpack_from("<Ii", bai, at); out += [at + 4, at + 8]; at += 8
            for _ in range(max(n_chunk, 0)):
                if at + 16 > len(bai):
                    return out
                out += [at + 8, at + 16]; at += 16
        if n_bin < 0 or at + 4 > len(bai):
            return out
        (n_intv,) = struct.unpack_from("<i", bai, at); at += 4; out.append(at)
        for _ in range(max(n_intv, 0)):
            if at + 8 > len(bai):
                return out
            at += 8; out.append(at)
        if n_intv < 0:
            return out
    if at + 8 <= len(bai):
        out.append(at + 8)
    return sorted(set(o for o in out if o <= len(bai)))


def small_index():
    rng = np.random.default_rng(5)
    return indexed(bt.random_records(rng, 40, REF_LEN, max_ops=5), 3)[2]


def test_truncated_index_is_refused(lib):
    good = small_index()
    assert not refused(lib, good, 3)
    assert not refused(lib, good[:-8], 3)                                         # n_no_coor is optional (SAM specification 5.2)
    cuts = [c for c in boundaries(good) if c < len(good) - 8]
    assert len(cuts) > 50
    for c in cuts:
        assert refused(lib, good[:c], 3), c
    for c in range(len(good) - 7, len(good)):                                     # inside n_no_coor
        assert refused(lib, good[:c], 3), c
    assert refused(lib, b"", 3) and refused(lib, b"BAM\x01" + good[4:], 3)


def malformed():
    good = small_index()
    refs, _ = bt.parse(good)
    out = {}
    # where reference 0's fields lie
    at = 8
    (n_bin,) = struct.unpack_from("<i", good, at)
    assert n_bin >= 2
    first_bin = at + 4
    _, n_chunk = struct.unpack_from("<Ii", good, first_bin)
    first_chunk = first_bin + 8
    p = first_bin
    for _ in range(n_bin):
        _, k = struct.unpack_from("<Ii", good, p)
        p += 8 + 16 * k
    n_intv_at = p
    put = lambda b, o, fmt, *v: b[:o] + struct.pack(fmt, *v) + b[o + struct.calcsize(fmt):]
    out["negative n_bin"] = put(good, at, "<i", -1)
    out["negative n_chunk"] = put(good, first_bin + 4, "<i", -2)
    out["negative n_intv"] = put(good, n_intv_at, "<i", -1)
    cb, ce = struct.unpack_from("<QQ", good, first_chunk)
    out["chunk end < beg"] = put(good, first_chunk, "<QQ", ce + 1, cb)
    out["n_bin beyond the bytes"] = put(good, at, "<i", 1 << 28)
    out["n_chunk beyond the bytes"] = put(good, first_bin + 4, "<i", 1 << 27)
    out["n_intv beyond the bytes"] = put(good, n_intv_at, "<i", 1 << 28)
    out["negative n_ref"] = put(good, 4, "<i", -3)
    out["bytes behind n_no_coor"] = good + b"\0"
    out["pseudo-bin with one chunk"] = None
    # the pseudo-bin is the last bin of reference 0: give it one chunk (the bytes behind then parse as something else or run out)
    pseudo = n_intv_at - 40
    assert struct.unpack_from("<Ii", good, pseudo) == (bt.PSEUDO, 2)
    out["pseudo-bin with one chunk"] = put(good, pseudo + 4, "<i", 1)
    return good, out


def test_malformed_index_is_refused(lib):
    good, bad = malformed()
    valid = {good, good[:-8]}
    for name, b in bad.items():
        assert refused(lib, b, 3), name
        for c in boundaries(b):
            if c < len(b) and b[:c] not in valid:
                assert refused(lib, b[:c], 3), (name, c)
    assert refused(lib, good, 2), "an n_ref other than the BAM header's"
    assert not refused(lib, good, 3)
