"""lra_bam_svcalls on crafted BAM files: the pieces' text and values equal tests/svcalls_ref.py's tables -- the rows at the size threshold, the mask at its
edges, the numbering across references, the merge at its equalities, along chains, in cliques and against the START order -- and what it refuses it refuses
with the finished references' pieces delivered first and another pass possible."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svcalls_cases as sc                                                        # noqa: E402
import svcalls_ref as sr                                                          # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = sc.NAMES


@pytest.fixture(scope="module")
def vctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from lra_amd.context import Context
    c = Context(0)
    yield c
    c.close()


def rec_with(ref, rows, name, rng, tlen=None, flag=0, lead=5):
    """a record whose variants are `rows` [(START, length, "I" / "D")], ascending and apart: it begins `lead` bases in front of the first anchor and ends 5 bases
    behind the last variant.  tlen None: its reference span"""
    pos = rows[0][0] + 1 - lead
    assert pos >= 0
    cur, cigar = pos, ""
    for start, n, kind in rows:
        assert start + 1 - cur >= (1 if not cigar else 0)                          # (0: a run of the other kind at the same anchor)
        cigar += ("%dM" % (start + 1 - cur) if start + 1 > cur else "") + "%d%s" % (n, kind)
        cur = start + 1 + (n if kind == "D" else 0)
    cigar += "5M"
    span = cur + 5 - pos
    return sc.rec(ref, pos, span if tlen is None else tlen, flag=flag, name=name, ops=cigar, rng=rng)


def collect(ctx, path, bai=None, ref=None, mask=None, obj=None, **kw):
    """one pass -> the pieces [(ref_id, kind, rows as the oracle's tuples, text)], the stats, the error; every value's text_off is where its line begins"""
    from lra_amd.bam import BamSvCalls
    from lra_amd._lib import LraError
    d = obj or BamSvCalls(ctx, path, bai, values=True, **kw)
    pieces, err = [], None
    try:
        if mask is not None:
            d.set_mask(mask)
        for r, kind, n, v, t in d.fetch(ref):
            assert v is not None and len(v) == n and n > 0
            lines = t.split(b"\n")[:-1]
            assert len(lines) == n and t.endswith(b"\n")
            assert np.array_equal(v["text_off"], np.concatenate([[0], np.cumsum([len(x) + 1 for x in lines])])[:-1])
            assert all(int(x["ref_id"]) == r and int(x["kind"]) == (1 if kind == "DEL" else 0) for x in v)
            rows = [(int(x["ref_id"]), int(x["start"]), int(x["end"]), int(x["nr"]), int(x["svlen"]), int(x["qstart"]), int(x["kind"]), int(x["strand"]), int(x["record"])) for x in v]
            pieces.append((r, kind, rows, t))
    except LraError as e:
        err = str(e)
    st = d.stats()
    if obj is None:
        d.close()
    return pieces, st, err


def tables(pieces):
    return {k: (b"".join(p[3] for p in pieces if p[1] == k), [r for p in pieces if p[1] == k for r in p[2]]) for k in ("DEL", "INS")}


def check(ctx, tmp_path, recs, genome, name="s.bam", level=1, load_it=True, mask=None, **kw):
    """the whole file against the oracle: both tables' text and values, the order of the pieces, the counts"""
    if load_it:
        sc.load(ctx, genome)
    path = sc.plain_file(tmp_path, name, recs, [len(g) for g in genome], level=level)
    okw = {k: kw[k] for k in ("require", "exclude", "min_mapq", "min_size", "drop_contained", "aligner", "hap") if k in kw}
    for k in ("aligner", "hap"):
        if k in okw:
            okw[k] = okw[k].encode()
    want = sr.calls([sc.parse(r) for r in recs], [sr.core_of(r) for r in recs], NAMES, genome, mask=mask or (), **okw)
    pieces, st, err = collect(ctx, path, mask=mask, **kw)
    assert err is None, err
    got = tables(pieces)
    for k in ("DEL", "INS"):
        assert got[k][0] == want[k][0], (k, got[k][0][:300], want[k][0][:300])
        assert got[k][1] == want[k][1], k
    order = [(p[0], p[1]) for p in pieces]
    assert order == sorted(order, key=lambda x: (x[0], x[1] != "DEL")) and len(set(order)) == len(order)   # by reference, DEL in front of INS, one piece each
    ws = want["stats"]
    assert (st["records_read"], st["records_contained"], st["records_walked"]) == (len(recs), ws["contained"], ws["walked"])
    assert [st["small_ins"], st["small_del"]] == ws["small"] and [st["masked_ins"], st["masked_del"]] == ws["masked"]
    assert [st["merged_ins"], st["merged_del"]] == ws["merged"] and [st["kept_ins"], st["kept_del"]] == ws["kept"]
    assert st["bytes_text"] == len(want["DEL"][0]) + len(want["INS"][0])
    return path, want, st


# ---- rows and the mask -----------------------------------------------------------------------------------------------------------------------------------------
def test_rows_at_the_threshold(vctx, tmp_path):
    rng = np.random.default_rng(1)
    genome = sc.genome_of([3000])
    recs = [rec_with(0, [(100 * k + 50, n, c)], b"t%d" % k, rng) for k, (n, c) in enumerate((n, c) for c in "ID" for n in (1, 2, 3, 4))]
    recs.append(rec_with(0, [(1000, 2, "I"), (1000, 3, "D")], b"both", rng))       # an INS and a DEL at one anchor
    recs.append(rec_with(0, [(1100, 3, "I"), (1120, 1, "D"), (1140, 2, "D"), (1150, 1, "I")], b"four", rng, flag=16))
    for size, kept in ((1, 14), (2, 10), (3, 6), (0, 14), (5, 0)):
        _, want, st = check(vctx, tmp_path, recs, genome, min_size=size)
        assert st["kept_ins"] + st["kept_del"] == kept and st["small_ins"] + st["small_del"] == 14 - kept
    worked = want                                                                  # (min_size 5: nothing)
    assert worked["DEL"][0] == b"" and worked["INS"][0] == b""
    _, want, _ = check(vctx, tmp_path, recs, genome, min_size=3, load_it=False)
    first = want["DEL"][0].split(b"\n")[0].split(b"\t")
    assert first[:4] == [b"chr1", b"650", b"653", b"aligner.DEL.maternal.1"] and len(first[4]) == 4 and len(first[5]) == 1 and first[6:8] == [b"60", b"PASS"]
    assert b"QSTRAND=-" in want["INS"][0] and [r[:4] for r in want["DEL"][1]][-1] == (0, 1000, 1003, 3)


def test_mask(vctx, tmp_path):
    rng = np.random.default_rng(2)
    genome = sc.genome_of([3000, 3000])
    recs = [rec_with(0, [(100, 40, "D")], b"d", rng), rec_with(0, [(300, 40, "I")], b"i", rng), rec_with(1, [(100, 40, "D"), (300, 40, "I")], b"other", rng)]
    sc.load(vctx, genome)
    n = {}
    for key, mask in (("none", None), ("empty", []), ("touch_start", [(0, 60, 100), (0, 250, 300)]), ("touch_end", [(0, 140, 150), (0, 340, 350)]),
                      ("base_at_start", [(0, 60, 101), (0, 250, 301)]), ("base_at_end", [(0, 139, 150), (0, 339, 350)]), ("other_ref", [(1, 0, 3000)]),
                      ("inside", [(0, 120, 121)]), ("around", [(0, 0, 3000)]), ("empty_interval_inside", [(0, 120, 120)]),
                      ("unsorted_overlapping", [(0, 2000, 2100), (0, 330, 2050), (1, 5, 50), (0, 0, 50), (0, 10, 20), (1, 20, 101), (0, 40, 90)])):
        _, want, st = check(vctx, tmp_path, recs, genome, mask=mask, min_size=40, load_it=False)
        n[key] = (st["kept_del"], st["kept_ins"])
    assert n == {"none": (2, 2), "empty": (2, 2), "touch_start": (2, 2), "touch_end": (2, 2), "base_at_start": (1, 1), "base_at_end": (1, 1), "other_ref": (1, 1),
                 "inside": (1, 2), "around": (1, 1), "empty_interval_inside": (1, 2), "unsorted_overlapping": (1, 1)}
    # NR counts the survivors of the mask: with all of chr1 masked, chr2's rows are number 1
    _, want, _ = check(vctx, tmp_path, recs, genome, mask=[(0, 0, 3000)], min_size=40, load_it=False)
    assert want["DEL"][0].split(b"\t")[3] == b"aligner.DEL.maternal.1" and want["DEL"][0].startswith(b"chr2\t")
    from lra_amd.bam import BamSvCalls
    from lra_amd._lib import LraError
    d = BamSvCalls(vctx, sc.plain_file(tmp_path, "m.bam", recs, [3000, 3000]))
    try:
        for bad in ([(2, 0, 10)], [(-1, 0, 10)], [(0, 10, 9)], [(0, -1, 9)]):
            with pytest.raises(LraError, match="set_mask"):
                d.set_mask(bad)
        d.set_mask([(0, 0, 3000)])
        assert b"".join(p[4] for p in d.fetch()).count(b"\n") == 2
        d.set_mask([])                                                             # taken away again
        assert b"".join(p[4] for p in d.fetch()).count(b"\n") == 4
    finally:
        d.close()


# ---- the merge ---------------------------------------------------------------------------------------------------------------------------------------------------
def ins_rows(intervals, rng, ref=0, tag=b"m"):
    """one record per row, an insertion each: START and length free of one another.  TLEN ascends with START, so that the contained filter keeps every record"""
    return [rec_with(ref, [(s, e - s, "I")], b"%s%d" % (tag, k), rng, tlen=1_000_000 + s) for k, (s, e) in enumerate(intervals)]


def test_merge_equalities(vctx, tmp_path):
    """10 ov == len on the first row relates the pair, on the second it does not (tests/test_svcalls_ref.py works the numbers): [1000, 1100) then [1090, 1140)
    drops the second; [3090, 3140) numbered in front of [3000, 3100) -- a long record's late variant, then the next record's -- keeps both.  Touching rows"""
    rng = np.random.default_rng(3)
    genome = sc.genome_of([6000])
    recs = ins_rows([(1000, 1100), (1090, 1140)], rng)
    recs.append(rec_with(0, [(2000, 3, "I"), (3090, 50, "I")], b"late", rng, tlen=1_000_000 + 2000))
    recs += ins_rows([(3000, 3100)], rng, tag=b"early")
    recs += ins_rows([(4000, 4050), (4050, 4100), (4200, 4310), (4299, 4350)], rng, tag=b"touch")   # ov 0; then ov 11 of 110 and 51: both ways
    recs = sorted(recs, key=lambda r: sr.core_of(r)[1])
    _, want, st = check(vctx, tmp_path, recs, genome, min_size=40)
    assert [r[1] for r in want["INS"][1]] == [1000, 3090, 3000, 4000, 4050, 4200] and st["merged_ins"] == 2
    _, want, _ = check(vctx, tmp_path, recs, genome, min_size=40, drop_contained=False, load_it=False)   # (nothing is contained here: the same rows)
    assert [r[1] for r in want["INS"][1]] == [1000, 3090, 3000, 4000, 4050, 4200]


def test_merge_chain(vctx, tmp_path):
    """200 rows, each related only to its successor: every other one is kept, and every decision waits for the one in front of it"""
    rng = np.random.default_rng(4)
    genome = sc.genome_of([60_000])
    recs = ins_rows([(80 * k + 10, 80 * k + 110) for k in range(200)], rng)
    _, want, st = check(vctx, tmp_path, recs, genome, min_size=40)
    assert [r[3] for r in want["INS"][1]] == list(range(1, 201, 2)) and st["merge_rounds"] >= 100
    # deletions overlap on the reference too; 700 of them are three of the pair search's tiles of 256 rows, most of which a row passes over
    recs = [rec_with(0, [(80 * k + 10, 100, "D")], b"d%d" % k, rng, tlen=1_000_000 + k) for k in range(700)]
    recs.append(rec_with(0, [(59_000, 60, "D")], b"far", rng, tlen=2_000_000))
    recs.insert(0, rec_with(0, [(6, 58_000, "D")], b"wide", rng, tlen=100))        # number 1, related to none (a tenth of it is 5800 bases) but met by every tile
    _, want, st = check(vctx, tmp_path, recs, genome, min_size=40, load_it=False)
    assert [r[3] for r in want["DEL"][1]] == [1] + list(range(2, 702, 2)) + [702] and st["merge_rounds"] >= 700


def test_merge_cliques(vctx, tmp_path):
    rng = np.random.default_rng(5)
    genome = sc.genome_of([10_000, 10_000])
    recs = ins_rows([(10 + k, 1010 + k) for k in range(65)], rng) + ins_rows([(10 + k, 1010 + k) for k in range(257)], rng, ref=1, tag=b"n")
    _, want, st = check(vctx, tmp_path, recs, genome, min_size=40)
    assert [r[:4] for r in want["INS"][1]] == [(0, 10, 1010, 1), (1, 10, 1010, 66)] and st["merged_ins"] == 320


def test_nr_order_against_start_order(vctx, tmp_path):
    """record k begins at k and holds one insertion at 6000 - 100 k: NR ascends while START descends; neighbours share 50 of 150 bases"""
    rng = np.random.default_rng(6)
    genome = sc.genome_of([8000])
    recs = [rec_with(0, [(6000 - 100 * k, 150, "I")], b"z%d" % k, rng, tlen=1_000_000 + k, lead=6000 - 100 * k + 1 - k) for k in range(40)]
    _, want, st = check(vctx, tmp_path, recs, genome, min_size=40)
    assert [r[3] for r in want["INS"][1]] == list(range(1, 41, 2)) and [r[1] for r in want["INS"][1]][:2] == [6000, 5800]


K, REF_LEN = 100, [21_000, 21_000, 500, 21_000]                                 # records of 300 bytes, 3 K to a reference: some windows of 65536 each


def two_reference_file(rng):
    recs = []
    for ref in (0, 1, 3):                                                          # (reference 2 has no record)
        for k in range(K):
            recs.append(rec_with(ref, [(200 * k + 20, 45 + k % 3, "D"), (200 * k + 120, 50 + k % 5, "I")], b"r%d_%d" % (ref, k), rng))
            recs.append(rec_with(ref, [(200 * k + 22, 45, "D")], b"in%d_%d" % (ref, k), rng))                                   # nested: the contained filter's
            recs.append(rec_with(ref, [(200 * k + 25, 44, "D"), (200 * k + 130, 48, "I")], b"s%d_%d" % (ref, k), rng, tlen=260))   # its own calls again, shifted: merged away
    recs += [sc.rec(-1, -1, 0, flag=4, name=b"un%d" % k, seq=b"ACGT") for k in range(3)]
    return recs


def test_references_pieces_and_numbering(vctx, tmp_path):
    rng = np.random.default_rng(7)
    ref_len = REF_LEN
    genome = sc.genome_of(ref_len)
    recs = two_reference_file(rng)
    path, want, st = check(vctx, tmp_path, recs, genome, min_size=40, level=0)
    assert st["records_contained"] == 3 * K and st["merged_del"] == 3 * K and st["kept_del"] == 3 * K and st["kept_ins"] == 3 * K
    assert [r[3] for r in want["DEL"][1]] == list(range(1, 6 * K + 1, 2))              # NR runs on across the references
    pieces, st, err = collect(vctx, path, min_size=40, window_bytes=65536)          # many windows: a reference's rows gather over them
    assert err is None and st["windows"] >= 3 and tables(pieces)["DEL"] == want["DEL"] and tables(pieces)["INS"] == want["INS"]
    assert [(p[0], p[1]) for p in pieces] == [(0, "DEL"), (0, "INS"), (1, "DEL"), (1, "INS"), (3, "DEL"), (3, "INS")]
    check(vctx, tmp_path, recs, genome, min_size=40, drop_contained=False, load_it=False)   # the nested records' calls are merged away instead
    check(vctx, tmp_path, recs, genome, min_size=40, aligner="lra", hap="paternal", exclude=0x14, load_it=False)
    # a whole reference: NR restarts at 1
    bam, bai = sc.indexed_file(tmp_path, "i.bam", recs, ref_len)
    P, cores = [sc.parse(r) for r in recs], [sr.core_of(r) for r in recs]
    from lra_amd.bam import BamSvCalls
    from lra_amd._lib import LraError
    d = BamSvCalls(vctx, bam, bai, values=True, min_size=40)
    try:
        for ref in (1, 3, b"chr1", 2):
            r = NAMES.index(ref) if isinstance(ref, bytes) else ref
            w = sr.calls(P, cores, NAMES, genome, min_size=40, region=r)
            pieces, _, err = collect(vctx, None, obj=d, ref=ref)
            got = tables(pieces)
            cut = lambda t: (t[0], [x[:8] for x in t[1]])                          # (`record` counts the records the pass has read: a region's begin at its first chunk)
            assert err is None and cut(got["DEL"]) == cut(w["DEL"]) and cut(got["INS"]) == cut(w["INS"])
            assert [x[3] for x in got["DEL"][1]] == list(range(1, 2 * K + 1, 2))[:len(got["DEL"][1])] and (r == 2) == (not pieces)
        for beg, end in ((1, 21_000), (0, 20_999), (10, 20)):                          # narrower than the reference
            assert vctx.lib.lra_bam_svcalls_region(d.h, ctypes.c_int32(1), ctypes.c_int64(beg), ctypes.c_int64(end)) != 0
            with pytest.raises(LraError, match="not the whole of reference 1"):
                vctx.check(-2)
        assert vctx.lib.lra_bam_svcalls_region(d.h, ctypes.c_int32(1), ctypes.c_int64(0), ctypes.c_int64(10 ** 12)) == 0   # beyond the end is the whole
        pieces, _, err = collect(vctx, None, obj=d)                                # and a whole pass behind them
        assert err is None and tables(pieces)["INS"] == want["INS"]
    finally:
        d.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(vctx, tmp_path):
    rng = np.random.default_rng(8)
    ref_len = REF_LEN
    genome = sc.genome_of(ref_len)
    sc.load(vctx, genome)
    good = two_reference_file(rng)[:-3]
    at = 6 * K + 60                                                                     # a record of the last reference, behind others of it
    assert sr.core_of(good[at])[0] == 3 and sr.core_of(good[at - 20])[0] == 3
    l_name = good[at][12]
    bad_op = good[at][:36 + l_name] + struct.pack("<I", (25 << 4) | 9) + good[at][40 + l_name:]
    unsorted = rec_with(3, [(100, 50, "D")], b"early", rng)
    from lra_amd.bam import BamSvCalls
    for bad, why in ((bad_op, "op code above 8"), (unsorted, "not coordinate-sorted at record %d" % at)):
        recs = good[:at] + [bad] + good[at + 1:]
        path = sc.plain_file(tmp_path, "bad.bam", recs, ref_len, level=0)
        w = sr.calls([sc.parse(r) for r in recs[:6 * K]], [sr.core_of(r) for r in recs[:6 * K]], NAMES, genome, min_size=40)   # references 0 and 1 are finished
        for kw in ({}, dict(window_bytes=65536)):
            d = BamSvCalls(vctx, path, values=True, min_size=40, **kw)
            try:
                for _ in range(2):                                                 # the second pass says the same
                    pieces, _, err = collect(vctx, None, obj=d)
                    assert err and why in err and "record %d" % at in err and path in err and "lra_bam_svcalls" in err, err
                    assert [(p[0], p[1]) for p in pieces] == [(0, "DEL"), (0, "INS"), (1, "DEL"), (1, "INS")]
                    assert tables(pieces)["DEL"] == w["DEL"] and tables(pieces)["INS"] == w["INS"]
                    from lra_amd.bam import SvCallsPiece
                    p = SvCallsPiece()
                    assert vctx.lib.lra_bam_svcalls_next(d.h, ctypes.byref(p)) == 0 and not p.n_rows and not p.text_len   # the pass is over
            finally:
                d.close()
    with pytest.raises(Exception):
        BamSvCalls(vctx, path, text=False, values=False)
    with pytest.raises(Exception, match="printable"):
        BamSvCalls(vctx, path, aligner="a b")
