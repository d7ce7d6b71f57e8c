"""lra_sv_combine on crafted pairs of BAM files: the pieces' text and values equal tests/svcombine_ref.py's classes over tests/svcalls_ref.py's tables -- the
partner test at its equalities, touching and contained rows, rows of other references and kinds, several partners, a partner merged away in its own pass, the
tiles' boundaries and a long early row, several references over many windows, empty haplotypes, the options -- and what it refuses it refuses with the
haplotype named and nothing delivered."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_merge_cases as mc                                                      # noqa: E402
import svcalls_cases as sc                                                        # noqa: E402
import svcalls_ref as sr                                                          # noqa: E402
import svcombine_ref as cr                                                        # noqa: E402

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


def hap_records(spec, rng, tag):
    """spec: [(ref, [(START, length, "I" / "D"), ...])], a record each, its variants ascending and apart -> the records sorted by (ref, first START), stable,
    each beginning 5 bases in front of its first anchor; TLEN ascends with the file's order, so that the contained filter keeps every record"""
    order = sorted(range(len(spec)), key=lambda i: (spec[i][0], spec[i][1][0][0]))
    recs = []
    for n, i in enumerate(order):
        ref, rows = spec[i]
        pos = rows[0][0] + 1 - 5
        assert pos >= 0
        cur, cigar = pos, ""
        for start, ln, kind in rows:
            assert start + 1 > cur
            cigar += "%dM%d%s" % (start + 1 - cur, ln, kind)
            cur = start + 1 + (ln if kind == "D" else 0)
        recs.append(sc.rec(ref, pos, 1_000_000 + 10 * n, name=b"%s%d" % (tag, i), ops=cigar + "5M", rng=rng))
    return recs


def single(rows, ref=0):
    """a record per row (START, length, kind)"""
    return [(ref, [r]) for r in rows]


def collect(ctx, path_m, path_p, bai_m=None, bai_p=None, ref=None, mask=None, **kw):
    """one run -> the pieces [(hap, kind, cls, text, rows as the oracle's tuples)], the stats, the error; every value's text_off is where its line begins"""
    from lra_amd.bam import SvCombine
    from lra_amd._lib import LraError
    d = SvCombine(ctx, path_m, path_p, bai_m, bai_p, values=True, **kw)
    pieces, err = [], None
    try:
        if mask is not None:
            d.set_mask(mask)
        for hap, kind, cls, n, v, t in d.fetch(ref):
            assert v is not None and len(v) == n and n > 0
            lines = t.split(b"\n")[:-1]
            assert len(lines) == n and t.endswith(b"\n")
            assert np.array_equal(v["text_off"], np.concatenate([[0], np.cumsum([len(x) + 1 for x in lines])])[:-1])
            assert all(int(x["kind"]) == (1 if kind == "DEL" else 0) for x in v)
            rows = [(int(x["ref_id"]), int(x["start"]), int(x["end"]), int(x["nr"]), int(x["svlen"]), int(x["qstart"]), int(x["kind"]), int(x["strand"]), int(x["record"]),
                     int(x["hap"]), int(x["cls"])) for x in v]
            pieces.append((hap, kind, cls, t, rows))
    except LraError as e:
        err = str(e)
        pieces_at_error = list(pieces)
        assert not pieces_at_error, "a refused run delivered pieces"
    st = d.stats()
    d.close()
    return pieces, st, err


def check(ctx, tmp_path, spec_m, spec_p, genome, rng, load_it=True, level=1, frac=None, filter_pass=False, pos_one_based=False, **kw):
    """the two files against the oracle: every piece's text and values, the delivery order, the counts -> (the oracle's pieces and stats, the object's stats)"""
    if load_it:
        sc.load(ctx, genome)
    ref_len = [len(g) for g in genome]
    recs = {"m": hap_records(spec_m, rng, b"m"), "p": hap_records(spec_p, rng, b"p")}
    path = {h: sc.plain_file(tmp_path, h + ".bam", recs[h], ref_len, level=level) for h in "mp"}
    okw = {k: kw[k] for k in ("min_size", "drop_contained") if k in kw}
    num, den = frac or (3, 10)
    want, wst, wm, wp = cr.run([sc.parse(r) for r in recs["m"]], [sr.core_of(r) for r in recs["m"]], [sc.parse(r) for r in recs["p"]], [sr.core_of(r) for r in recs["p"]],
                               NAMES, genome, num, den, filter_pass, pos_one_based, **okw)
    got, st, err = collect(ctx, path["m"], path["p"], frac=frac, filter_pass=filter_pass, pos_one_based=pos_one_based, **kw)
    assert err is None, err
    assert [g[:3] for g in got] == [w[:3] for w in want]
    for g, w in zip(got, want):
        assert g[3] == w[3], (g[:3], g[3][:300], w[3][:300])
        assert g[4] == w[4], g[:3]
    assert [st["het_m_ins"], st["het_m_del"], st["het_p_ins"], st["het_p_del"], st["hom_ins"], st["hom_del"]] == \
           [wst["m_INS_het"], wst["m_DEL_het"], wst["p_INS_het"], wst["p_DEL_het"], wst["m_INS_hom"], wst["m_DEL_hom"]]
    assert [st["partnered_p_ins"], st["partnered_p_del"]] == wst["partnered_p"] and st["runs"] == 1
    assert st["bytes_text"] == sum(len(w[3]) for w in want)
    for h, w in ((0, wm), (1, wp)):                                                # the two passes' own stats are reachable: their tables are the merged ones
        assert [st["passes"][h]["kept_ins"], st["passes"][h]["kept_del"]] == w["stats"]["kept"] and st["passes"][h]["bytes_text"] == 0
        assert [st["passes"][h]["merged_ins"], st["passes"][h]["merged_del"]] == w["stats"]["merged"]
    return want, wst, st


def ids(want, key):
    return [ln.split(b"\t")[2] for w in want if w[:3] == key for ln in w[3].split(b"\n")[:-1]]


# ---- the partner test ------------------------------------------------------------------------------------------------------------------------------------------
A_ROWS = [(100, 10, "D"), (300, 10, "D"), (500, 10, "D"), (700, 10, "D"), (900, 10, "D"), (1100, 10, "D"), (2000, 40, "I"), (2500, 40, "I"), (3000, 50, "I")]
B_ROWS = [(107, 10, "D"),                                                          # ov 3: 30 >= 30 both ways: hom
          (308, 10, "D"),                                                          # ov 2: both het
          (507, 11, "D"),                                                          # ov 3 of 10 and 11: 30 >= 30 but 30 < 33: both het
          (710, 10, "D"),                                                          # touching: both het
          (890, 34, "D"),                                                          # a inside a b more than 10 / 3 as long: 100 < 102: both het
          (1090, 33, "D"),                                                         # inside a b of 33: 100 >= 99: hom
          (2000, 100, "I"),                                                        # one anchor, 40 and 100: ov 40, 400 >= 300: hom
          (2500, 140, "I"),                                                        # 40 and 140: 400 < 420: both het
          (3000, 50, "D")]                                                         # an INS and a DEL over the same bases: both het


@pytest.mark.parametrize("swapped", [False, True])
def test_equalities_touching_containment_and_kinds(vctx, tmp_path, swapped):
    rng = np.random.default_rng(1)
    genome = sc.genome_of([6000, 6000])
    a = single(A_ROWS) + single([(100, 10, "D")], ref=1)                           # the same interval as b's first row, on another reference: het
    b = single(B_ROWS)
    m, p = (b, a) if swapped else (a, b)
    want, wst, st = check(vctx, tmp_path, m, p, genome, rng, min_size=1)
    hom = {s for w in want if w[2] == "hom" for s in (r[1] for r in w[4])}
    assert hom == ({107, 1090, 2000} if swapped else {100, 1100, 2000})
    assert (st["hom_ins"], st["hom_del"], st["partnered_p_ins"], st["partnered_p_del"]) == (1, 2, 1, 2)
    assert st["het_m_ins"] + st["het_m_del"] + st["het_p_ins"] + st["het_p_del"] == 19 - 6
    assert [w[:3] for w in want] == list(cr.ORDER)
    line = [w for w in want if w[:3] == ("maternal", "DEL", "hom")][0][3].split(b"\n")[0].split(b"\t")
    assert len(line) == 10 and line[2] == b"aligner.DEL.maternal.1" and line[5] == b"60" and line[6] == line[7] and line[6].startswith(b"SVTYPE=DEL;SVLEN=-10;QNAME=")
    assert line[8:] == [b"GT", b"1/1"]


def test_several_partners_and_a_partner_merged_away(vctx, tmp_path):
    """the maternal [1000, 1100) has three paternal partners -- [930, 1030), [1035, 1065), [1070, 1170), no two of them related in their own merge -- and is
    printed once; they are printed nowhere.  The paternal [3050, 3150) would be the maternal [3100, 3150)'s partner, but its own pass merges it into
    [3000, 3100), which only touches the maternal row: het"""
    rng = np.random.default_rng(2)
    genome = sc.genome_of([6000])
    m = single([(1000, 100, "I"), (3100, 50, "I")])
    p = single([(930, 100, "I"), (1035, 30, "I"), (1070, 100, "I"), (3000, 100, "I"), (3050, 100, "I")])
    want, wst, st = check(vctx, tmp_path, m, p, genome, rng, min_size=30)
    assert ids(want, ("maternal", "INS", "hom")) == [b"aligner.INS.maternal.1"] and ids(want, ("maternal", "INS", "het")) == [b"aligner.INS.maternal.2"]
    assert ids(want, ("paternal", "INS", "het")) == [b"aligner.INS.paternal.4"] and st["partnered_p_ins"] == 3 and st["passes"][1]["merged_ins"] == 1
    assert cr.partner((0, 3100, 3150), (0, 3050, 3150))                             # (it would have been one)


# ---- the tiles -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_tile_boundaries(vctx, tmp_path, n):
    """a paternal table of n rows on one reference, 150 bases apart, behind one long row that spans every later START; maternal tables of one row -- the
    partner of the first small row, of the last, of the first row of the last tile, of the long row alone -- and of 513 rows"""
    rng = np.random.default_rng(3)
    genome = sc.genome_of([90_000])
    sc.load(vctx, genome)
    small = [(150 * k + 200, 40, "D") for k in range(n)]
    p = single([(60, 80_000, "D")] + small)                                        # NR 1: the long row; the small rows are rows 1 .. n of the table
    last_tile = 256 * (n // 256)                                                   # the table's row that begins its last tile (the table has n + 1 rows)
    for k in sorted({0, n - 1, max(last_tile - 1, 0)}):
        s = small[k][0]
        want, wst, st = check(vctx, tmp_path, single([(s + 5, 40, "D")]), p, genome, rng, load_it=False)
        assert st["hom_del"] == 1 and st["partnered_p_del"] == 1 and st["het_p_del"] == n
        assert [r[1] for w in want if w[:3] == ("paternal", "DEL", "het") for r in w[4]] == [60] + [x[0] for x in small if x[0] != s]
    want, wst, st = check(vctx, tmp_path, single([(25_000, 55_000, "D")]), p, genome, rng, load_it=False)   # far along: only the long row, row 0, is its partner
    assert st["hom_del"] == 1 and st["partnered_p_del"] == 1 and st["het_p_del"] == n
    m = single([(150 * k + 205, 40, "D") for k in range(513) if k % 7])            # 513 rows less every seventh
    want, wst, st = check(vctx, tmp_path, m, p, genome, rng, load_it=False)
    assert st["hom_del"] == len([k for k in range(min(n, 513)) if k % 7]) and st["het_m_del"] == len(m) - st["hom_del"] and st["partnered_p_del"] == st["hom_del"]


# ---- several references ------------------------------------------------------------------------------------------------------------------------------------------
def test_references_windows_and_empty_haplotypes(vctx, tmp_path):
    rng = np.random.default_rng(4)
    genome = sc.genome_of([40_000, 30_000, 500, 30_000])
    K = 180
    m, p = [], []
    for ref in (0, 1, 3):
        for k in range(K):
            m.append((ref, [(150 * k + 10, 45 + k % 3, "D"), (150 * k + 90, 50 + k % 5, "I")]))
            if ref != 1:                                                           # reference 1 has rows in the maternal haplotype only
                # every fourth deletion shares 10 .. 12 bases of 45 with the maternal one (too few), the others 30 .. 32; the insertions share an anchor and
                # every third is up to four times as long
                p.append((ref, [(150 * k + 45, 40, "D") if k % 4 == 0 else (150 * k + 25, 45, "D"), (150 * k + 90, 50 + (k % 5) * (40 if k % 3 == 0 else 1), "I")]))
    want, wst, st = check(vctx, tmp_path, m, p, genome, rng, level=0, window_bytes=65536)
    assert st["passes"][0]["windows"] >= 2 and st["passes"][1]["windows"] >= 2   # the tables are appended to across windows
    assert st["hom_del"] == 2 * (K - K // 4) and st["het_m_del"] == K + 2 * (K // 4) and st["het_p_del"] == 2 * (K // 4) and st["hom_ins"] > 0 and st["het_p_ins"] > 0
    assert not any(r[0] == 1 for w in want if w[2] == "hom" for r in w[4])
    # one haplotype without rows: everything is het of the other; both: no pieces
    want, wst, st = check(vctx, tmp_path, m[:40], [], genome, rng, load_it=False)
    assert [w[:3] for w in want] == [("maternal", "INS", "het"), ("maternal", "DEL", "het")] and st["het_m_ins"] == 40
    want, wst, st = check(vctx, tmp_path, [], p[:40], genome, rng, load_it=False)
    assert [w[:3] for w in want] == [("paternal", "INS", "het"), ("paternal", "DEL", "het")] and st["het_p_del"] == 40
    want, wst, st = check(vctx, tmp_path, [], [], genome, rng, load_it=False)
    assert want == [] and st["bytes_text"] == 0


# ---- the options -----------------------------------------------------------------------------------------------------------------------------------------------
def test_options(vctx, tmp_path):
    from lra_amd.bam import BamSvCalls, SvCombine
    from lra_amd._lib import LraError
    rng = np.random.default_rng(5)
    genome = sc.genome_of([6000, 6000])
    ref_len = [6000, 6000]
    a = single(A_ROWS) + single([(100, 10, "D"), (2000, 40, "I")], ref=1)
    b = single(B_ROWS) + single([(109, 10, "D"), (2000, 45, "I")], ref=1)
    # 1 / 10 and PASS: combinehapSV.snakefile's.  [100, 110) and [109, 119) on chr2 are partners now
    want, wst, st = check(vctx, tmp_path, a, b, genome, rng, min_size=1, frac=(1, 10), filter_pass=True)
    assert (1, 100) in {(r[0], r[1]) for w in want if w[2] == "hom" for r in w[4]} and st["hom_del"] == 6 and st["hom_ins"] == 3
    # ... and every line is the line lra_bam_svcalls prints for the row with vcf_columns
    recs = {"maternal": hap_records(a, np.random.default_rng(5), b"m"), "paternal": hap_records(b, np.random.default_rng(5), b"p")}
    lines = {}
    for hap in recs:
        d = BamSvCalls(vctx, sc.plain_file(tmp_path, hap + "1.bam", recs[hap], ref_len), min_size=1, hap=hap, vcf_columns=True)
        lines[hap] = set(b"".join(x[4] for x in d.fetch()).split(b"\n")[:-1])
        d.close()
    got, _, err = collect(vctx, sc.plain_file(tmp_path, "m1.bam", recs["maternal"], ref_len), sc.plain_file(tmp_path, "p1.bam", recs["paternal"], ref_len), min_size=1,
                          frac=(1, 10), filter_pass=True)
    assert err is None and len(got) == 5                                            # (no paternal insertion is left without a partner)
    for hap, kind, cls, text, rows in got:
        assert set(text.split(b"\n")[:-1]) <= lines[hap] and b"\tPASS\t" in text
    assert sum(len(g[4]) for g in got) + st["partnered_p_ins"] + st["partnered_p_del"] == len(lines["maternal"]) + len(lines["paternal"])
    # START + 1
    want1, _, _ = check(vctx, tmp_path, a, b, genome, rng, min_size=1, pos_one_based=True, load_it=False)
    want0, _, _ = check(vctx, tmp_path, a, b, genome, rng, min_size=1, load_it=False)
    assert [int(ln.split(b"\t")[1]) for w in want1 for ln in w[3].split(b"\n")[:-1]] == [int(ln.split(b"\t")[1]) + 1 for w in want0 for ln in w[3].split(b"\n")[:-1]]
    assert [w[4] for w in want1] == [w[4] for w in want0]                          # (the values never)
    # one reference, through the indexes: numbered from 1, as lra_bam_svcalls does
    P = {h: [sc.parse(r) for r in recs[h]] for h in recs}
    cores = {h: [sr.core_of(r) for r in recs[h]] for h in recs}
    files = {h: sc.indexed_file(tmp_path, h + "i.bam", recs[h], ref_len) for h in recs}
    for ref in (1, b"chr1"):
        r = NAMES.index(ref) if isinstance(ref, bytes) else ref
        w, wst, _, _ = cr.run(P["maternal"], cores["maternal"], P["paternal"], cores["paternal"], NAMES, genome, min_size=1, region=r)
        got, st, err = collect(vctx, files["maternal"][0], files["paternal"][0], files["maternal"][1], files["paternal"][1], ref=ref, min_size=1)
        cut = lambda t: [(x[:3], x[3], [y[:8] + y[9:] for y in x[4]]) for x in t]     # (`record` counts the records the pass has read: a region's begin at its first chunk)
        assert err is None and cut(got) == cut(w) and got and all(y[0] == r for x in got for y in x[4])
    with pytest.raises(LraError, match="not the whole of reference"):
        d = SvCombine(vctx, files["maternal"][0], files["paternal"][0], files["maternal"][1], files["paternal"][1])
        try:
            vctx.check(vctx.lib.lra_sv_combine_region(d.h, 1, 5, 6000))
        finally:
            d.close()
    # a mask goes to both passes
    mask = [(0, 0, 1000), (1, 0, 6000)]
    wm = sr.calls(P["maternal"], cores["maternal"], NAMES, genome, hap=b"maternal", min_size=1, mask=mask)
    wp = sr.calls(P["paternal"], cores["paternal"], NAMES, genome, hap=b"paternal", min_size=1, mask=mask)
    got, st, err = collect(vctx, files["maternal"][0], files["paternal"][0], mask=mask, min_size=1)
    assert err is None and [(g[:4], g[4]) for g in got] == [(w[:4], w[4]) for w in cr.combine(wm, wp)[0]] and st["passes"][0]["masked_del"] == 6
    # fractions that are none
    for frac in ((0, 7), (4, 3), (1, 0)):
        with pytest.raises(LraError, match="fraction"):
            SvCombine(vctx, files["maternal"][0], files["paternal"][0], frac=frac)
    with pytest.raises(LraError, match="neither text nor values"):
        SvCombine(vctx, files["maternal"][0], files["paternal"][0], text=False, values=False)
    # values alone: no text, the same rows
    d = SvCombine(vctx, files["maternal"][0], files["paternal"][0], text=False, values=True, min_size=1)
    got = [(hap, kind, cls, t, [int(x) for x in v["nr"]]) for hap, kind, cls, n, v, t in d.fetch()]
    d.close()
    assert [(g[:3], g[4]) for g in got] == [(w[:3], [r[3] for r in w[4]]) for w in want0] and all(g[3] == b"" for g in got)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(vctx, tmp_path):
    from lra_amd import bgzf
    from lra_amd.bam import SvCombine
    from lra_amd._lib import LraError
    rng = np.random.default_rng(6)
    genome = sc.genome_of([6000, 6000])
    ref_len = [6000, 6000]
    sc.load(vctx, genome)
    m = hap_records(single(A_ROWS) + single([(100, 50, "D")], ref=1), rng, b"m")
    p = hap_records(single(B_ROWS) + single([(120, 50, "D")], ref=1), rng, b"p")
    good_m, good_p = sc.plain_file(tmp_path, "gm.bam", m, ref_len), sc.plain_file(tmp_path, "gp.bam", p, ref_len)
    # two reference tables that differ from each other (and not in what the context compares: the lengths)
    head = mc.header_bytes(ref_len).replace(b"chr2\0", b"chrX\0")
    renamed = sc.write(tmp_path, "renamed.bam", bgzf.bgzf_compress(head, 6, eof=False) + bgzf.bgzf_compress(b"".join(p), 1, eof=False) + mc.EOF_BLOCK)
    with pytest.raises(LraError, match=r"lra_sv_combine_create: .*renamed.bam: reference 1 is named chrX, in .*gm.bam it is chr2"):
        SvCombine(vctx, good_m, renamed)
    with pytest.raises(LraError, match="lra_bam_svcalls_create"):                  # a length: the pass's own test against the context's genome
        SvCombine(vctx, sc.plain_file(tmp_path, "short.bam", m, [6000, 5000]), good_p)
    # an unsorted paternal file: the run is refused with the haplotype named, nothing is delivered -- not even the maternal rows or chr1's -- and a run on good files succeeds
    bad_p = sc.plain_file(tmp_path, "bp.bam", p[:-1] + [p[0]], ref_len)
    for kw in ({}, dict(window_bytes=65536)):
        pieces, st, err = collect(vctx, good_m, bad_p, min_size=1, **kw)
        assert err and "the paternal pass" in err and "not coordinate-sorted at record %d" % (len(p) - 1) in err and bad_p in err and not pieces, err
        assert st["runs"] == 0 and st["bytes_text"] == 0
    pieces, st, err = collect(vctx, bad_p, good_p, min_size=1)
    assert err and "the maternal pass" in err and not pieces
    d = SvCombine(vctx, good_m, bad_p, min_size=1)                                  # the same object refuses the same way twice: it took another run
    for _ in range(2):
        with pytest.raises(LraError, match="the paternal pass"):
            list(d.fetch())
    d.close()
    pieces, st, err = collect(vctx, good_m, good_p, min_size=1)
    assert err is None and len(pieces) >= 4 and st["runs"] == 1
