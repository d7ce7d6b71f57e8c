"""tests/svcombine_ref.py, the oracle of the two-haplotype combination, pinned on the CPU: (a) its column rule against what the reference's own awk programs
-- the rules Homcalls and Hetcalls of both snakefiles -- printed for crafted rows (tests/golden/svcombine_awk_golden.json, written by
tools/make_golden_svcombine.py); (b) the interval rule of bedtools intersect -f F -r, which no script of the reference holds, worked by hand below; (c) the
classes and the delivery order of combineHet's cat."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svcombine_ref as cr                                                        # noqa: E402

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svcombine_awk_golden.json")))


# ---- (a) the columns -------------------------------------------------------------------------------------------------------------------------------------------
def test_columns_equal_the_awk():
    rows = [r.encode() for r in GOLD["rows"]]
    assert len(GOLD["cases"]) == 6 and any(b"=0001;x;" in r for r in rows)          # an INFO with ; and = of its own
    for case in GOLD["cases"]:
        got = [cr.columns(r, filter_pass=case["snakefile"] == "combinehapSV.snakefile") for r in rows]
        assert got == [x.encode() for x in case["printed"]], (case["snakefile"], case["rule"], case["program"])
    first = cr.columns(rows[0]).split(b"\t")
    assert len(first) == 10 and first[6] == first[7] == rows[0].split(b"\t")[8] and first[8:] == [b"GT", b"1/1"]
    assert cr.columns(rows[0], True).split(b"\t")[6:8] == [b"PASS", first[7]]


# ---- (b) the intervals -------------------------------------------------------------------------------------------------------------------------------------------
def test_partner_by_hand():
    a = (0, 100, 110)
    # b = [107, 117): ov = 110 - 107 = 3; 10 * 3 = 30 >= 3 * 10 = 30 for both rows of length 10: partners at equality
    assert cr.partner(a, (0, 107, 117)) and cr.partner((0, 107, 117), a)
    # b = [108, 118): ov 2; 20 < 30
    assert not cr.partner(a, (0, 108, 118)) and not cr.partner((0, 108, 118), a)
    # b of length 11 with ov 3, [107, 118): 30 >= 30 for a, 30 < 33 for b: the fraction is needed of both rows (-r)
    assert not cr.partner(a, (0, 107, 118)) and not cr.partner((0, 107, 118), a)
    # touching: ov 0; one base: ov 1, 10 < 30
    assert not cr.partner(a, (0, 110, 120)) and not cr.partner(a, (0, 90, 100)) and not cr.partner(a, (0, 109, 119))
    # a inside b: ov = 10; b of 33 bases: 100 >= 99 partners; 34 bases: 100 < 102 -- more than 10 / 3 as long
    assert cr.partner(a, (0, 90, 123)) and not cr.partner(a, (0, 90, 124))
    # insertions at one anchor: [s, s + 40) and [s, s + 100): ov 40, 400 >= 300; and [s, s + 140): 400 < 420
    assert cr.partner((0, 500, 540), (0, 500, 600)) and not cr.partner((0, 500, 540), (0, 500, 640))
    # another reference
    assert not cr.partner(a, (1, 100, 110))
    # 1 / 10, combinehapSV.snakefile's: ov 1 of 10 and 10
    assert cr.partner(a, (0, 109, 119), 1, 10) and not cr.partner(a, (0, 109, 120), 1, 10)
    # symmetric, for every pair of a small grid
    iv = [(0, s, s + n) for s in range(0, 30, 3) for n in (1, 2, 7, 10, 33, 34)]
    assert all(cr.partner(x, y) == cr.partner(y, x) for x in iv for y in iv)
    assert all(cr.partner(x, x) for x in iv)


def test_float_form_on_a_grid():
    """the single-precision test bedtools makes, (float)ov / (float)len >= 0.3f, against the integers, for every ov <= len <= 600 (the stand-alone program
    tools/micro/bam_svcombine_host_check.cpp goes further); numpy's float32 division is IEEE's"""
    import numpy as np
    n = np.arange(1, 601, dtype=np.int64)
    ov, ln = np.meshgrid(n, n)
    ok = ov <= ln
    for num, den, lit in ((3, 10, np.float32(0.3)), (1, 10, np.float32(0.1))):
        f = (ov.astype(np.float32) / ln.astype(np.float32)) >= lit
        assert np.array_equal(f[ok], (den * ov >= num * ln)[ok])


# ---- (c) the classes and the order -----------------------------------------------------------------------------------------------------------------------------
def table(rows, hap, kind):
    """svcalls_ref.calls()' (text, rows) of one kind from (ref, start, end): NR in the order given"""
    text, out = [], []
    for nr, (ref, s, e) in enumerate(rows, 1):
        svlen = (e - s) * (-1 if kind == "DEL" else 1)
        info = b"SVTYPE=%s;SVLEN=%d;QNAME=q%d;QSTART=5;QSTRAND=+" % (kind.encode(), svlen, nr)
        text.append(b"\t".join([b"chr%d" % (ref + 1), b"%d" % s, b"%d" % e, b"aligner.%s.%s.%d" % (kind.encode(), hap, nr), b"A", b"C", b"60", b"PASS", info, b"GT", b"1/1"]) + b"\n")
        out.append((ref, s, e, nr, svlen, 5, 1 if kind == "DEL" else 0, 0, nr - 1))
    return b"".join(text), out


def calls(ins, dele, hap):
    return {"INS": table(ins, hap, "INS"), "DEL": table(dele, hap, "DEL")}


def test_classes_and_delivery_order():
    m = calls([(0, 500, 540), (0, 900, 950)], [(0, 100, 110), (1, 100, 110), (0, 300, 400)], b"maternal")
    p = calls([(0, 500, 600), (0, 2000, 2040)], [(0, 107, 117), (0, 300, 400), (0, 301, 399), (0, 310, 410), (2, 5, 50)], b"paternal")
    got, st = cr.combine(m, p)
    assert [(g[0], g[1], g[2]) for g in got] == list(cr.ORDER)
    by = {(g[0], g[1], g[2]): g for g in got}
    ids = lambda g: [ln.split(b"\t")[2] for ln in g[3].split(b"\n")[:-1]]
    assert ids(by["maternal", "INS", "hom"]) == [b"aligner.INS.maternal.1"] and ids(by["maternal", "INS", "het"]) == [b"aligner.INS.maternal.2"]
    assert ids(by["paternal", "INS", "het"]) == [b"aligner.INS.paternal.2"]
    # the maternal DEL [300, 400) has three partners and is printed once, with its maternal ID; the same interval on chr2 is het; the paternal partners are nowhere
    assert ids(by["maternal", "DEL", "hom"]) == [b"aligner.DEL.maternal.1", b"aligner.DEL.maternal.3"] and ids(by["maternal", "DEL", "het"]) == [b"aligner.DEL.maternal.2"]
    assert ids(by["paternal", "DEL", "het"]) == [b"aligner.DEL.paternal.5"] and st["partnered_p"] == [1, 4]
    assert all(r[-2:] == (0, 1) for r in by["maternal", "DEL", "hom"][4]) and all(r[-2:] == (1, 0) for r in by["paternal", "DEL", "het"][4])
    line = by["maternal", "INS", "hom"][3].split(b"\t")
    assert line[:3] == [b"chr1", b"500", b"aligner.INS.maternal.1"] and line[6] == line[7] and line[6].startswith(b"SVTYPE=INS") and line[8:] == [b"GT", b"1/1\n"]
    # an INS and a DEL over the same bases never meet; a class without rows has no piece; PASS and + 1
    got, st = cr.combine(calls([(0, 100, 140)], [], b"maternal"), calls([], [(0, 100, 140)], b"paternal"), filter_pass=True, one_based=True)
    assert [(g[0], g[1], g[2]) for g in got] == [("maternal", "INS", "het"), ("paternal", "DEL", "het")]
    assert got[0][3].split(b"\t")[1] == b"101" and got[0][3].split(b"\t")[6] == b"PASS"
    assert cr.combine(calls([], [], b"maternal"), calls([], [], b"paternal"))[0] == []
    # 1 / 10 makes partners of what 3 / 10 leaves apart
    m, p = calls([], [(0, 100, 110)], b"maternal"), calls([], [(0, 109, 119)], b"paternal")
    assert [g[2] for g in cr.combine(m, p)[0]] == ["het", "het"] and [g[2] for g in cr.combine(m, p, 1, 10)[0]] == ["hom"]
