"""The contained-alignment filter (bam_contained.h) through lra_bam_vcf's drop_contained, on crafted BAM files whose records carry a TLEN: the records the
filter drops are the ones tests/svcalls_ref.py's walk drops -- the reference's ParseAlignment.py -- at every run length around the scan's wave, block and tile
sizes, across windows, across a window that is run again in front of a refused record, and by region; with the filter off the bytes are today's."""
import json
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svcalls_cases as sc                                                        # noqa: E402
import svcalls_ref as sr                                                          # noqa: E402

pytestmark = pytest.mark.gpu
CIGAR = "12M1I10M2D9M"                                                            # every walked record yields two lines: who was dropped shows in the text
SPAN = 33


@pytest.fixture(scope="module")
def vctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from lra_amd.context import Context
    c = Context(0)
    yield c
    c.close()


def collect(ctx, path, bai=None, region=None, **kw):
    from lra_amd.bam import BamVcf
    from lra_amd._lib import LraError
    d = BamVcf(ctx, path, bai, values=True, **kw)
    text, vals, err = [], [], None
    try:
        for n, v, t in d.fetch(*(region or ())):
            vals += [(int(x["ref_id"]), int(x["pos"]), int(x["qstart"]), int(x["svlen"]), int(x["kind"]), int(x["strand"]), int(x["record"])) for x in v]
            text.append(t)
    except LraError as e:
        err = str(e)
    st = d.stats()
    d.close()
    return b"".join(text), vals, st, err


def check(ctx, tmp_path, recs, genome, name="c.bam", level=1, **kw):
    path = sc.plain_file(tmp_path, name, recs, [len(g) for g in genome], level=level)
    want, wvals, wst = sc.vcf_want(recs, genome)
    text, vals, st, err = collect(ctx, path, drop_contained=True, **kw)
    assert err is None, err
    assert text == want and vals == wvals
    assert (st["records_read"], st["records_contained"], st["records_walked"], st["records_filtered"]) == (len(recs), wst["contained"], wst["walked"], wst["filtered"])
    return path, st


def run_of(ref, n, pattern, rng, tag):
    """n records of one reference: "kept": every end above the ends before; "dropped": all behind the first lie inside it; "alt": every other one"""
    out = []
    for k in range(n):
        pos = 10 + 3 * k
        e = {"kept": pos + 100 + k, "dropped": 10 + 100_000 if k == 0 else pos + 50 + (k % 7), "alt": 20_000 + 10 * (k - k % 2)}[pattern]             # (alt: an odd record's end equals the even one's in front of it)
        out.append(sc.rec(ref, pos, e - pos - 1, name=b"%s_%d" % (tag, k), ops=CIGAR, rng=rng))
    return out


def test_run_lengths(vctx, tmp_path):
    """runs of 1, 2, 63 - 65, 255 - 257 and 1025 records (the scan's wave is 64 lanes, a lane folds 8 records, a tile holds 2048), one behind the other with the
    reference alternating, so that every run's first record stands behind a run with larger ends"""
    rng = np.random.default_rng(1)
    genome = sc.genome_of([5000, 5000])
    sc.load(vctx, genome)
    recs, ref = [], 0
    for pattern in ("kept", "dropped", "alt"):
        for n in (1, 2, 63, 64, 65, 255, 256, 257, 1025):
            recs += run_of(ref, n, pattern, rng, b"%s%d" % (pattern.encode(), n))
            ref ^= 1
    drop = sr.contained([sr.core_of(r) for r in recs])
    assert sum(drop) > 2000 and drop.count(False) > 2500
    check(vctx, tmp_path, recs, genome)


def test_ends(vctx, tmp_path):
    """equal ends drop; pos + 1 + tlen above 2^31 is compared in 64 bits; TLEN may be negative; the reference's own cases (ParseAlignment.py's goldens)"""
    rng = np.random.default_rng(2)
    genome = sc.genome_of([4000, 4000, 4000])
    sc.load(vctx, genome)
    big = 2 ** 31 - 1
    cases = {"wide": [(0, 10, big), (0, 11, big - 1), (0, 12, big - 1), (0, 13, big), (0, 14, -5), (0, 15, big), (1, 5, big), (1, 6, 7)],
             "negative": [(0, 100, -50), (0, 100, -60), (0, 100, -40), (0, 101, -41), (0, 200, -200), (0, 300, -2 ** 31), (1, 0, -2 ** 31), (1, 0, -2 ** 31), (1, 1, -2 ** 31 + 1)]}
    assert [d for d in sr.contained(cases["wide"])] == [False, True, False, False, True, False, False, True]   # ends 2^31 + 10, + 10, + 11, + 13, 10, + 15
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svcalls_scripts_golden.json")))
    for case in gold["parse"]:
        if max(p for _, p, _ in case["lines"]) + SPAN <= 4000:
            ids = {}
            cases[case["name"]] = [(ids.setdefault(c, len(ids)), p - 1, t) for c, p, t in case["lines"]]
            assert [i for i, d in enumerate(sr.contained(cases[case["name"]])) if not d] == case["kept"]
    assert len(cases) >= 20
    for name, cores in cases.items():
        recs = [sc.rec(r, p, t, name=b"%s%d" % (name.encode()[:8], k), ops=CIGAR, rng=rng) for k, (r, p, t) in enumerate(cores)]
        check(vctx, tmp_path, recs, genome, name=name + ".bam")


def windows_file(rng, n=4000):
    """records of about 100 bytes for windows of 65536: a stretch whose reference changes with every record (whatever record a window begins or ends with is a
    run's first), a stretch of pairs, then one reference whose first record's end stands until a record three windows on exceeds it, then unmapped records"""
    recs = [sc.rec(k % 2, 10 + k, 500 - k % 3, name=b"a%04d" % k, ops=CIGAR, rng=rng) for k in range(1500)]
    recs += [sc.rec((k // 2) % 2, 2000 + k, 40 + (5 if k % 4 < 2 else -5) * (k % 2), name=b"p%04d" % k, ops=CIGAR, rng=rng) for k in range(1500)]
    recs.append(sc.rec(2, 0, 9000, name=b"top", ops=CIGAR, rng=rng))               # end 9001
    recs += [sc.rec(2, 1 + k, 8999 - k + (1 if k % 1000 == 999 else 0), name=b"u%04d" % k, ops=CIGAR, rng=rng) for k in range(n)]   # ends 9001, and 9002 at every 1000th
    recs += [sc.rec(-1, -1, 0, flag=4, name=b"un%d" % k, seq=b"ACGT") for k in range(5)]
    return recs


def test_windows_and_the_carry(vctx, tmp_path):
    rng = np.random.default_rng(3)
    genome = sc.genome_of([6000, 6000, 6000])
    sc.load(vctx, genome)
    recs = windows_file(rng)
    drop = sr.contained([sr.core_of(r) for r in recs])
    assert not any(drop[:1500]) and drop[3001:7001].count(False) == 1              # behind `top`, only the first record with end 9002 is kept
    path, st = check(vctx, tmp_path, recs, genome, level=0, window_bytes=65536)
    assert st["windows"] >= 8
    check(vctx, tmp_path, recs, genome, level=0)                                   # one window
    # with the filter off, and through the field's old name's value 0, today's bytes
    want, wvals, _ = sc.vcf_want(recs, genome, drop_contained=False)
    text, vals, st, err = collect(vctx, path, window_bytes=65536)
    assert err is None and text == want and vals == wvals and st["records_contained"] == 0
    assert collect(vctx, path, drop_contained=False)[0] == want


def test_a_window_run_again(vctx, tmp_path):
    """a refused record in the middle of a later window: the records in front of it are run again with the carry as it was, and delivered; the next call refuses"""
    rng = np.random.default_rng(4)
    genome = sc.genome_of([60_000])
    sc.load(vctx, genome)
    recs = [sc.rec(0, 10 * k, 100 + (k % 3) * 20 - (35 if k % 5 == 0 else 0), name=b"w%04d" % k, ops=CIGAR, rng=rng) for k in range(3000)]
    bad = 2201                                                                     # (a record the filter keeps: a dropped one is not walked, so not refused)
    assert not sr.contained([sr.core_of(r) for r in recs])[bad]
    l_name = recs[bad][12]
    recs[bad] = recs[bad][:36 + l_name] + struct.pack("<I", (12 << 4) | 9) + recs[bad][40 + l_name:]
    drop = sr.contained([sr.core_of(r) for r in recs[:bad]])
    assert 500 < sum(drop) < 1700
    path = sc.plain_file(tmp_path, "again.bam", recs, [60_000], level=0)
    want, wvals, wst = sc.vcf_want(recs[:bad], genome)
    for kw in (dict(window_bytes=65536), {}):
        text, vals, st, err = collect(vctx, path, drop_contained=True, **kw)
        assert err and "op code above 8" in err and "record %d" % bad in err, err
        assert text == want and vals == wvals and st["records_contained"] == wst["contained"]


def test_regions(vctx, tmp_path):
    from lra_amd.bam import BamVcf
    from lra_amd._lib import LraError
    rng = np.random.default_rng(5)
    ref_len = [50_000, 3000, 50_000]
    genome = sc.genome_of(ref_len)
    sc.load(vctx, genome)
    recs = []
    for ref in (0, 2):
        recs += [sc.rec(ref, 20 * k, 300 + (k % 4) * 15 - (100 if k % 3 == 0 else 0), name=b"g%d_%04d" % (ref, k), ops=CIGAR, rng=rng) for k in range(1200)]
    recs.insert(1200, sc.rec(1, 5, 40, name=b"mid", ops=CIGAR, rng=rng))
    recs.insert(1201, sc.rec(1, 6, 39, name=b"mid_in", ops=CIGAR, rng=rng))
    bam, bai = sc.indexed_file(tmp_path, "r.bam", recs, ref_len)
    for ref in range(3):                                                           # a whole reference: the whole pass's lines of it
        want, wvals, wst = sc.vcf_want(recs, genome, region=(ref, 0, ref_len[ref]))
        text, vals, st, err = collect(vctx, bam, bai, region=(ref, 0, None), drop_contained=True)
        assert err is None and text == want and [v[:6] for v in vals] == [v[:6] for v in wvals] and st["records_contained"] == wst["contained"] > 0
    want = sc.vcf_want(recs, genome, region=(2, 0, 9000))[0]                       # beg == 0 and an end inside: the records in front of the end, in order
    text, _, _, err = collect(vctx, bam, bai, region=(2, 0, 9000), drop_contained=True)
    assert err is None and text == want and want
    text, _, _, err = collect(vctx, bam, bai, region=(2, 1, 9000), drop_contained=True)
    assert text == b"" and err and "drop_contained" in err and "begins at 0" in err
    o = BamVcf(vctx, bam, bai, drop_contained=True)
    try:
        with pytest.raises(LraError, match="drop_contained"):
            list(o.fetch(0, 100, 200))
        assert b"".join(p[2] for p in o.fetch()) == sc.vcf_want(recs, genome)[0]    # the object takes another pass
    finally:
        o.close()
    assert collect(vctx, bam, bai, region=(2, 1, 9000))[0] == sc.vcf_want(recs, genome, drop_contained=False, region=(2, 1, 9000))[0]   # off: any region
