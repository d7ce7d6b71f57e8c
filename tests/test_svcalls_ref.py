"""tests/svcalls_ref.py, the oracle of the assembly-SV calls, pinned on the CPU: against what the reference's own ParseAlignment.py and mergeSV.py did with
crafted inputs (tests/golden/svcalls_scripts_golden.json, written by tools/make_golden_svcalls.py), and the interval rules that no script of the reference
holds -- bedtools' and awk's -- one by one, worked by hand in the text below."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svcalls_ref as sr                                                          # noqa: E402
import vcf_ref as vr                                                              # noqa: E402

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svcalls_scripts_golden.json")))
CODE = {c: k for k, c in enumerate("MIDNSHP=X")}


def ops(text):
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n) << 4) | CODE[ch])
            n = ""
    return out


def cores_of(lines):
    """the golden's SAM lines (chrom, POS 1-based, TLEN) -> (refID, pos 0-based, tlen), a refID per name in order of appearance"""
    ids = {}
    return [(ids.setdefault(c, len(ids)), p - 1, t) for c, p, t in lines]


# ---- the contained filter ---------------------------------------------------------------------------------------------------------------------------------
def test_contained_equals_the_script():
    assert len(GOLD["parse"]) >= 20
    for case in GOLD["parse"]:
        cores = cores_of(case["lines"])
        kept = [i for i, d in enumerate(sr.contained(cores)) if not d]
        assert kept == case["kept"], case["name"]
        assert sr.contained_script(cores) == sr.contained(cores), case["name"]      # current_end is the running maximum


def test_contained_cases():
    by = {c["name"]: c for c in GOLD["parse"]}
    # the example: ends 601 451 601 602 711 -- the 3rd equals the maximum and drops, the 4th exceeds it by one; then (5,10) twice, (6,8), (6,20): ends 16 16 15 27
    assert by["issue_example"]["kept"] == [0, 3, 4, 5, 8]
    assert by["equal_ends"]["kept"] == [0] and by["one_record"]["kept"] == [0]
    assert by["first_of_a_run"]["kept"] == [0, 1, 2, 4]                             # a run's first record is kept whatever stood before, c1's second run included
    assert by["reference_change"]["kept"] == [0, 2, 4, 5]
    assert by["dropped_does_not_lower"]["kept"] == [0, 4]                          # ends 101 12 53 101 102 102
    assert by["negative_tlen"]["kept"] == [0, 2, 3] and by["large"]["kept"] == [0, 2]
    # records with refID < 0 take no part: never dropped, and the run goes on behind them
    assert sr.contained([(0, 0, 100), (-1, -1, 0), (0, 5, 10), (-1, -1, 0), (-1, -1, 0)]) == [False, False, True, False, False]


# ---- the merge ----------------------------------------------------------------------------------------------------------------------------------------------
def test_merge_equals_the_script():
    assert len(GOLD["merge"]) >= 20
    for case in GOLD["merge"]:
        rows = [tuple(r) for r in case["rows"]]
        ids = ["aligner.DEL.maternal.%d" % (i + 1) for i in range(len(rows))]
        col = [",".join(ids[j] for j, b in enumerate(rows) if b[0] == a[0] and sr.related(a[1:], b[1:])) for a in rows]
        assert col == case["intersect"], case["name"]                              # the script's input was built with this `related`
        assert all(ids[i] in col[i].split(",") for i in range(len(rows)))          # -wao pairs a row with itself: ov = len, both quotients 1
        assert [i for i, k in enumerate(sr.merge(rows)) if k] == case["kept"], case["name"]


def test_merge_cases():
    by = {c["name"]: c["kept"] for c in GOLD["merge"]}
    assert by["chain_A_B_C"] == [0, 2]                                             # B is dropped and spreads nothing: C stays
    assert by["disjoint"] == [0, 2] and by["touching"] == [0, 1]
    assert by["one_way_kept"] == [0, 1] and by["one_way_dropped"] == [0]           # a pair related one way only (test_overlap_rule works it)
    assert by["nr_not_start_order"] == [0, 1, 4] and by["two_references"] == [0, 1, 3]
    assert by["all_related"] == [0] and by["long_chain"] == list(range(0, 21, 2))


# ---- the interval rules, one by one ---------------------------------------------------------------------------------------------------------------------------
def test_mask_rule():
    """bedtools intersect -v drops a row that shares at least one base with a mask interval: [s, e) and [b, f) share a base when s < f and b < e."""
    row = (0, 100, 140)
    assert not sr.masked(*row, [(0, 140, 200)]) and not sr.masked(*row, [(0, 50, 100)])          # touching END, touching START: no shared base
    assert sr.masked(*row, [(0, 139, 200)]) and sr.masked(*row, [(0, 50, 101)])                  # one shared base at either end
    assert not sr.masked(*row, [(1, 0, 1000)]) and not sr.masked(*row, [])                       # another reference; an empty mask
    assert sr.masked(*row, [(0, 500, 600), (0, 90, 95), (0, 0, 1000), (0, 120, 121)])            # any order, overlapping one another
    assert sr.masked(*row, [(0, 110, 111)]) and sr.masked(*row, [(0, 0, 1000)])                  # inside the row; around it


def test_overlap_rule():
    """R(a, b) for the first row a and the second b: ov = min(END) - max(START) > 0, 10 ov >= len_a, 10 ov > len_b."""
    assert not sr.related((0, 50), (50, 100)) and not sr.related((50, 100), (0, 50))             # touching: ov = 0
    assert sr.related((0, 50), (49, 59)) is False                                                # ov 1: 10 >= 50 fails
    # 10 ov == len on the FIRST row keeps the relation: a = [0, 100), b = [90, 140): ov 10, 100 >= 100, 100 > 50
    assert sr.related((0, 100), (90, 140))
    # ... on the SECOND row it does not: the same pair the other way round: 100 >= 50 holds, 100 > 100 fails
    assert not sr.related((90, 140), (0, 100))
    assert sr.related((0, 100), (89, 139)) and sr.related((89, 139), (0, 100))                   # ov 11: both ways
    assert not sr.related((0, 101), (91, 141))                                                   # ov 10, len_a 101: 100 >= 101 fails
    # so the order of the two rows decides: the 50-base row behind the 100-base row is dropped, in front of it both stay
    assert sr.merge([("c1", 0, 100), ("c1", 90, 140)]) == [True, False] and sr.merge([("c1", 90, 140), ("c1", 0, 100)]) == [True, True]
    # rows [0,100) [95,145) [0,50) [45,145).  R(0,1): ov 5, 50 >= 100 fails.  R(0,2): ov 50, 500 >= 100, 500 > 50.  R(0,3): ov 55, 550 >= 100, 550 > 100.
    assert sr.merge([("c1", 0, 100), ("c1", 95, 145), ("c1", 0, 50), ("c1", 45, 145)]) == [True, True, False, False]


def test_nr_order_is_not_start_order():
    """a long record's late variant has a lower NR than the next record's early one: the earlier NR wins, wherever it starts"""
    rows = [("c1", 500, 600), ("c1", 100, 200), ("c1", 520, 620), ("c1", 110, 210), ("c1", 0, 50)]
    assert sr.merge(rows) == [True, True, False, False, True]
    assert sr.merge(rows[::-1]) == [True, True, True, False, False]                              # the same intervals numbered the other way: the others go


# ---- rows, numbering and the text ------------------------------------------------------------------------------------------------------------------------------
def test_calls():
    import numpy as np
    rng = np.random.default_rng(1)
    genome = [bytes(rng.choice(list(b"ACGT"), 400).astype(np.uint8)), bytes(rng.choice(list(b"ACGT"), 300).astype(np.uint8))]
    names = [b"chr1", b"chr2"]
    seq = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    recs = [(0, 10, 0, 60, ops("20M3D10M2I10M4I5M"), seq(51), b"a"),              # DEL 3 at 29, INS 2 at 42 (too small at min_size 3), INS 4 at 52
            (0, 12, 16, 60, ops("18M3D30M"), seq(48), b"nested"),                # inside a: the same DEL, dropped with its record
            (0, 40, 0, 60, ops("10M3I10M"), seq(23), b"b"),                      # INS 3 at 49: [49, 52) and a's [52, 56) touch: both stay
            (1, 5, 0, 60, ops("10M5D10M5I10M"), seq(35), b"c")]                  # the second reference: NR runs on
    cores = [(0, 10, 48), (0, 12, 51 - 5), (0, 40, 20), (1, 5, 35)]
    out = sr.calls(recs, cores, names, genome, min_size=3)
    assert out["stats"]["contained"] == 1 and out["stats"]["walked"] == 3 and out["stats"]["small"] == [1, 0]
    assert [r[:4] + r[8:] for r in out["DEL"][1]] == [(0, 29, 32, 1, 0), (1, 14, 19, 2, 3)]
    assert [r[:4] + r[8:] for r in out["INS"][1]] == [(0, 52, 56, 1, 0), (0, 49, 52, 2, 2), (1, 29, 34, 3, 3)]
    first = out["DEL"][0].split(b"\n")[0].split(b"\t")
    plain = vr.line(names, recs[0], vr.variants(recs[0], genome, 3)[0]).rstrip(b"\n").split(b"\t")
    assert first[:4] == [b"chr1", b"29", b"32", b"aligner.DEL.maternal.1"] and first[4:] == plain[3:] and len(first) == 11
    assert sr.calls(recs, cores, names, genome, min_size=3, drop_contained=False)["stats"]["merged"] == [0, 1]   # the nested record's DEL is merged away instead
    masked = sr.calls(recs, cores, names, genome, min_size=3, mask=[(0, 31, 40), (1, 0, 14)])
    assert [r[:4] for r in masked["DEL"][1]] == [(1, 14, 19, 1)] and masked["stats"]["masked"] == [0, 1]   # NR counts the survivors of the mask
    only = sr.calls(recs, cores, names, genome, min_size=3, region=1, aligner=b"lra", hap=b"paternal")
    assert only["INS"][0].split(b"\t")[3] == b"lra.INS.paternal.1" and [r[3] for r in only["DEL"][1]] == [1]
