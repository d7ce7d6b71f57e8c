"""lra_bam_vcf on crafted BAM files: text and values equal tests/vcf_ref.py's walk -- every op kind, merged runs, the edges of the CIGAR, min_length, long
REF / ALT at the emitter's chunk size and at either nibble parity, the CG:B:I form, the digits, window sizes, regions through the .bai, the filters --
and what it refuses it refuses with the earlier records' lines delivered first and another pass possible."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_text as bt                                                             # noqa: E402
import bam_merge_cases as mc                                                      # noqa: E402
import bam_text                                                                   # noqa: E402
import vcf_ref as vr                                                              # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [b"chr%d" % (i + 1) for i in range(8)]
CODE = {c: k for k, c in enumerate("MIDNSHP=X")}
CHUNK = 4096                                                                      # the emitter's tile: bam_vcf.hip cuts the text into chunks of this many bytes
Q_OPS, R_OPS = {0, 1, 4, 7, 8}, {0, 2, 3, 7, 8}


def op(n, code):
    return (n << 4) | (CODE[code] if isinstance(code, str) else code)


def cig(text):
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(op(int(n), ch))
            n = ""
    return out


def bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def rec(ref=0, pos=100, flag=0, name=b"r", ops=(), seq=None, tags=b"", mapq=60, rng=None, core=None):
    """a record with a real SEQ: seq None: random bases for the ops' query length; core: the ops stored in the core CIGAR when they are not `ops` (the CG form)"""
    ops = list(ops)
    if seq is None:
        seq = bases(rng or np.random.default_rng(len(name) + pos), sum(o >> 4 for o in ops if (o & 15) in Q_OPS))
    span = sum(o >> 4 for o in ops if (o & 15) in R_OPS)
    stored = ops if core is None else core
    bin_ = 4680 if ref < 0 else bt.reg2bin(pos, pos + max(span, 1))
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, mapq, bin_, len(stored), flag, len(seq), -1, -1, 0) + name + b"\0"
    body += struct.pack("<%dI" % len(stored), *stored) + vr.pack_seq(seq) + b"\xff" * len(seq) + tags
    return struct.pack("<I", len(body)) + body


def cg_rec(ref, pos, flag, name, ops, rng, before=b"", behind=b""):
    """the CG:B:I form: CIGAR <l_seq>S<span>N, the ops in the tag, other tags in front of it and behind it"""
    l_seq = sum(o >> 4 for o in ops if (o & 15) in Q_OPS)
    span = sum(o >> 4 for o in ops if (o & 15) in R_OPS)
    tag = b"CGBI" + struct.pack("<I%dI" % len(ops), len(ops), *ops)
    return rec(ref, pos, flag, name, ops, rng=rng, tags=before + tag + behind, core=[op(l_seq, "S"), op(span, "N")])


def parse(r):
    return vr.parse_record(r, bam_text._tags)


def write(tmp_path, name, data):
    p = os.path.join(str(tmp_path), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


@pytest.fixture(scope="module")
def vctx():
    """a context of this module's own: every test loads its genome into it"""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from lra_amd.context import Context
    c = Context(0)
    yield c
    c.close()


def load(ctx, genome):
    from lra_amd.index import load_genome
    load_genome(ctx, np.frombuffer(b"".join(genome), np.uint8))
    pos = np.concatenate([[0], np.cumsum([len(g) for g in genome])]).astype(np.uint64)
    ctx.check(ctx.lib.lra_ctx_load_chromosomes(ctx.h, (ctypes.c_uint64 * len(pos))(*[int(x) for x in pos]), len(genome)))


def genome_of(ref_len, seed=3):
    rng = np.random.default_rng(seed)
    return [bases(rng, n) for n in ref_len]


def collect(ctx, path, bai=None, region=None, obj=None, **kw):
    """one pass -> the text, the values as the oracle's tuples, the stats, the error; every value's text_off is where its line begins"""
    from lra_amd.bam import BamVcf
    from lra_amd._lib import LraError
    d = obj or BamVcf(ctx, path, bai, values=True, **kw)
    text, vals, err = [], [], None
    try:
        for n, v, t in d.fetch(*(region or ())):
            assert v is not None and len(v) == n and n > 0
            lines = t.split(b"\n")[:-1]
            assert len(lines) == n and t.endswith(b"\n")
            at = np.concatenate([[0], np.cumsum([len(x) + 1 for x in lines])])[:-1]
            assert np.array_equal(v["text_off"], at)
            vals += [(int(x["ref_id"]), int(x["pos"]), int(x["qstart"]), int(x["svlen"]), int(x["kind"]), int(x["strand"]), int(x["record"])) for x in v]
            text.append(t)
    except LraError as e:
        err = str(e)
    st = d.stats()
    if obj is None:
        d.close()
    return b"".join(text), vals, st, err


def check(ctx, tmp_path, recs, genome, name="x.bam", level=1, load_it=True, **kw):
    """the whole file against the oracle: text, values, the counts of walked and skipped records"""
    if load_it:
        load(ctx, genome)
    ref_len = [len(g) for g in genome]
    path = write(tmp_path, name, mc.run_bytes(recs, level=level, ref_len=ref_len))
    okw = {k: kw[k] for k in ("require", "exclude", "min_mapq", "min_length", "pos_one_based") if k in kw and kw[k] is not None}
    want, wvals, wst = vr.call([parse(r) for r in recs], NAMES, genome, **okw)
    text, vals, st, err = collect(ctx, path, **kw)
    assert err is None, err
    assert text == want, (text[:300], want[:300])
    assert vals == wvals
    from lra_amd.bam import BamVcf
    o = BamVcf(ctx, path, **kw)                                                    # text alone, a fresh object's stats
    try:
        assert b"".join(p[2] for p in o.fetch()) == want
        s1 = o.stats()
    finally:
        o.close()
    assert (s1["records_read"], s1["records_walked"], s1["records_skipped"], s1["records_filtered"]) == (len(recs), wst["walked"], wst["skipped"], wst["filtered"])
    assert s1["n_ins"] == sum(1 for v in wvals if v[4] == 0) and s1["n_del"] == sum(1 for v in wvals if v[4] == 1) and s1["bytes_text"] == len(want)
    return path, want, wvals


# ---- the worked example ---------------------------------------------------------------------------------------------------------------------------------
WORKED = (b"chr1\t4\t.\tT\tTCA\t60\tPASS\tSVTYPE=INS;SVLEN=2;QNAME=r1;QSTART=5;QSTRAND=+\tGT\t1/1\n"
          b"chr1\t6\t.\tCAAG\tA\t60\tPASS\tSVTYPE=DEL;SVLEN=-3;QNAME=r1;QSTART=9;QSTRAND=+\tGT\t1/1\n")


def test_worked_example(vctx, tmp_path):
    genome = [b"ACGTTGCAAGCTTAGGCATC"]
    r = lambda flag: rec(pos=2, flag=flag, name=b"r1", ops=cig("2S3M2I2M3D4M1S"), seq=b"TTGTTCAGACTTAG")
    _, want, vals = check(vctx, tmp_path, [r(0)], genome)
    assert want == WORKED and vals == [(0, 4, 5, 2, 0, 0, 0), (0, 6, 9, -3, 1, 0, 0)]
    _, want, _ = check(vctx, tmp_path, [r(0)], genome, pos_one_based=True)
    assert want == WORKED.replace(b"chr1\t4\t", b"chr1\t5\t").replace(b"chr1\t6\t", b"chr1\t7\t")
    _, want, vals = check(vctx, tmp_path, [r(16)], genome)
    assert want == WORKED.replace(b"QSTRAND=+", b"QSTRAND=-") and [v[5] for v in vals] == [1, 1]


# ---- ops and the edges of the CIGAR ----------------------------------------------------------------------------------------------------------------------
def test_ops_and_edges(vctx, tmp_path):
    rng = np.random.default_rng(1)
    cigars = ["5=%d%s4=" % (3 + c, "MIDNSHP=X"[c]) for c in range(9)]                 # every op code between two match runs
    cigars += ["3M0I2M", "3M2I0M2I4M", "3M2I3I2M", "3M1I2P2I3M", "4M1D2N3D2M", "3M0D2M", "2M1I1P2I1H2M"]
    cigars += ["4M3D2I5M", "4M2I3D5M", "3M1I1D1I1D1I1D2M", "3M2D1I2D1I4M", "3X2I2=1D1X"]   # D then I, I then D, alternating runs
    cigars += ["3S2I4M2I3M", "3D4M1D3M", "2H3S4M", "4M2I", "4M3D", "4M3S", "4M2I2S", "4M2D2S", "4M2I3D", "4M2S1H"]   # leading and trailing ops
    recs = [rec(pos=10 + 37 * k, name=b"c%d" % k, ops=cig(c), rng=rng) for k, c in enumerate(cigars)]
    recs.append(rec(pos=5, name=b"only_si", ops=cig("3S4I"), rng=rng))
    recs.append(rec(pos=5, name=b"no_ops", ops=[], seq=b"ACGT"))
    recs.append(rec(pos=5, name=b"no_seq", ops=cig("3M2I3M"), seq=b""))
    recs.append(rec(pos=5, name=b"only_dn", ops=cig("3D4N"), seq=b"A"))
    recs.append(rec(ref=-1, pos=-1, flag=4, name=b"unmapped", seq=b"ACGT"))
    _, want, vals = check(vctx, tmp_path, recs, genome_of([3000]))
    names = [ln.split(b"QNAME=")[1].split(b";")[0] for ln in want.split(b"\n")[:-1]]
    count = [names.count(b"c%d" % k) for k in range(len(cigars))]
    assert count[:9] == [0, 1, 1, 1, 1, 0, 0, 0, 0] and count[9:16] == [0, 1, 1, 1, 1, 0, 1] and count[16:21] == [2, 2, 6, 4, 2]
    assert count[21:] == [1, 1, 0, 0, 0, 0, 0, 1, 1, 0]       # a run in front of trailing S is followed by an entry: it is printed; the S run is not
    assert not any(n in names for n in (b"only_si", b"no_ops", b"no_seq", b"only_dn"))


def test_threshold(vctx, tmp_path):
    rng = np.random.default_rng(2)
    recs = [rec(pos=50 * k, name=b"t%d" % k, ops=cig("6M%d%s6M" % (n, c)), rng=rng) for k, (n, c) in enumerate((n, c) for c in "ID" for n in (3, 4, 5, 6, 7))]
    genome = genome_of([1000])
    for L, kept in ((5, 6), (6, 4), (4, 8), (1, 10), (0, 10)):
        _, _, vals = check(vctx, tmp_path, recs, genome, min_length=L)
        assert len(vals) == kept and all(abs(v[3]) >= max(L, 1) for v in vals)


# ---- long REF and ALT ------------------------------------------------------------------------------------------------------------------------------------
def test_long_variants(vctx, tmp_path):
    rng = np.random.default_rng(4)
    genome = genome_of([400_000])
    recs = [rec(pos=1000, name=b"big_ins", ops=cig("20M100000I20M"), rng=rng), rec(pos=2000, name=b"big_del", ops=cig("20M100000D20M"), rng=rng)]
    for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1):
        recs.append(rec(pos=3000 + n, name=b"i%d" % n, ops=cig("7M%dI5M" % n), rng=rng))
        recs.append(rec(pos=120_000 + 3 * n, name=b"d%d" % n, ops=cig("7M%dD5M" % n), rng=rng))
    for lead in (10, 11):                                                          # the anchor at an odd and at an even SEQ index: ALT starts at either nibble
        recs.append(rec(pos=5000 + lead, name=b"par%d" % lead, ops=cig("%dM9000I4M" % lead), rng=rng))
    small = "".join("3=1D3=1I" for _ in range(500))
    recs.append(rec(pos=200_000, name=b"amid", ops=cig(small + "3=100000I" + small + "3="), rng=rng))
    path, want, vals = check(vctx, tmp_path, recs, genome, level=0)
    amid = [v for v in vals if v[6] == len(recs) - 1]
    assert len(amid) == 2001 and max(v[3] for v in amid) == 100000 and max(v[3] for v in vals) == 100000 and min(v[3] for v in vals) == -100000
    text, _, st, err = collect(vctx, path, window_bytes=65536)                     # records larger than the window
    assert err is None and text == want and st["windows"] > 3


def test_cg_form(vctx, tmp_path):
    rng = np.random.default_rng(5)
    genome = genome_of([50_000, 1000])
    ops = [op(1, "=" if k % 2 == 0 else "I") for k in range(70000)]
    xa, xb = b"XAC\x07", b"XBZok\0"
    recs = [cg_rec(0, 500, 16, b"first", ops, rng, behind=xa + xb), cg_rec(0, 600, 0, b"last", ops[:2001], rng, before=xa + xb),
            rec(pos=700, name=b"notag", ops=[], seq=bases(rng, 4), core=cig("4S6N")),                    # no tag: S N are the ops, no M = X base
            rec(pos=800, name=b"notform", ops=cig("4S6N2M"), rng=rng, tags=b"CGBI" + struct.pack("<II", 1, op(9, "M")))]
    _, want, vals = check(vctx, tmp_path, recs, genome)
    assert sum(1 for v in vals if v[6] == 0) == 34999 and sum(1 for v in vals if v[6] == 1) == 1000 and not any(v[6] >= 2 for v in vals)


def test_ops_without_a_class_between_runs(vctx, tmp_path):
    """200 000 ops of length 0, H and P inside one insertion run and inside one deletion run: one variant each, and no lane walks them"""
    rng = np.random.default_rng(12)
    none = [op(0, "MIDNS=X"[k % 7]) if k % 3 else op(5, "HP"[k % 2]) for k in range(100_000)]
    ops = cig("3M2I") + none + cig("2I3M2D") + none + cig("3N4M") + none + cig("1I") + none
    recs = [cg_rec(0, 100, 0, b"none", ops, rng), rec(pos=300, name=b"after", ops=cig("3M1D3M"), rng=rng)]
    _, want, vals = check(vctx, tmp_path, recs, genome_of([2000]))
    assert [(v[3], v[6]) for v in vals] == [(4, 0), (-5, 0), (-1, 1)]


def test_digits(vctx, tmp_path):
    rng = np.random.default_rng(6)
    genome = genome_of([350_000])
    recs = [rec(pos=0, name=b"L%d" % L, ops=cig("%dM2I3M" % L), rng=rng) for L in (1, 9, 10, 11, 99, 100, 101, 99999, 100000, 100001)]   # POS and QSTART
    recs += [rec(pos=1000 + k, name=b"I%d" % n, ops=cig("4M%dI3M" % n), rng=rng) for k, n in enumerate((9, 10, 11, 99, 100, 101, 99999, 100000, 100001))]
    recs += [rec(pos=2000 + k, name=b"D%d" % n, ops=cig("4M%dD3M" % n), rng=rng) for k, n in enumerate((9, 10, 11, 99, 100, 101, 99999, 100000, 100001))]
    for one in (False, True):
        _, want, vals = check(vctx, tmp_path, recs, genome, pos_one_based=one, level=0)
        pos = {int(ln.split(b"\t")[1]) for ln in want.split(b"\n")[:-1]}
        assert {9, 10, 99, 100, 99999, 100000} <= pos and (0 in pos) == (not one)
    assert {9, 10, 99, 100, 99999, 100000} <= {v[2] for v in vals} and {9, 10, 99, 100, 99999, 100000} <= {v[3] for v in vals}
    assert {-9, -10, -99, -100, -99999, -100000} <= {v[3] for v in vals} and vals[0][1] == 0


# ---- windows ---------------------------------------------------------------------------------------------------------------------------------------------
def many(n=900, ref=0, rng=None):
    rng = rng or np.random.default_rng(7)
    return [rec(ref=ref, pos=100 * i, name=b"g%04d" % i, ops=cig("30M3I20M%dD40=" % (1 + i % 7)), rng=rng) for i in range(n)]


def test_windows(vctx, tmp_path):
    genome = genome_of([400_000])
    recs = many(3000)
    path, want, _ = check(vctx, tmp_path, recs, genome, level=0)
    text, _, st, err = collect(vctx, path, window_bytes=65536)
    assert err is None and text == want and st["windows"] >= 5                       # (600 KB of records: they straddle every edge of a 64 KiB window)
    text, _, st, err = collect(vctx, path, window_bytes=1)                         # raised to 65536
    assert err is None and text == want


# ---- regions ---------------------------------------------------------------------------------------------------------------------------------------------
def indexed_file(tmp_path, name, recs, ref_len, level=1):
    from lra_amd import bgzf
    recs = sorted(recs, key=bt.sort_key)
    raw = b"".join(recs)
    head = bgzf.bgzf_compress(mc.header_bytes(ref_len), 6, eof=False)
    members = [bgzf.bgzf_compress(raw[a:a + bt.MEMBER], level, eof=False) for a in range(0, len(raw), bt.MEMBER)]
    moff = bt.member_table(len(raw), [len(m) for m in members])
    bam = write(tmp_path, name, head + b"".join(members) + mc.EOF_BLOCK)
    bai = write(tmp_path, name + ".bai", bt.build(raw, len(ref_len), moff, len(head)))
    return bam, bai, recs


def test_regions(vctx, tmp_path):
    from lra_amd.bam import BamVcf
    from lra_amd._lib import LraError
    rng = np.random.default_rng(8)
    ref_len = [200_000, 5000, 90_000]
    genome = genome_of(ref_len)
    load(vctx, genome)
    recs = many(1500, 0, rng) + many(600, 2, rng) + [rec(ref=1, pos=7, name=b"mid", ops=cig("5M2I5M"), rng=rng)]
    recs.append(rec(ref=0, pos=160_000, name=b"wide", ops=cig("10M2I30000M5D10M1I10M"), rng=rng))   # anchors at 160 009, 190 009 and 190 024
    bam, bai, recs = indexed_file(tmp_path, "s.bam", recs, ref_len)
    P = [parse(r) for r in recs]
    whole = vr.call(P, NAMES, genome)[0]
    o = BamVcf(vctx, bam, bai, values=True)
    try:
        assert collect(vctx, None, obj=o)[0] == whole
        for ref in range(3):                                                       # a whole reference: the whole pass filtered to it
            text, vals, _, err = collect(vctx, None, obj=o, region=(ref, 0, None))
            assert err is None and text == b"".join(ln + b"\n" for ln in whole.split(b"\n")[:-1] if ln.startswith(NAMES[ref] + b"\t"))
        a = 100 * 700 + 29                                                         # the insertion anchor of record g0700; its deletion's is at + 20
        for beg, end in ((a, a + 21), (a + 1, a + 20), (a - 5, a + 1), (a, a + 1), (a + 20, a + 21), (a, a), (0, 30), (160_009, 160_010), (170_000, 180_000),
                         (190_009, 190_025), (190_010, 190_024), (199_000, 10 ** 12)):
            text, vals, _, err = collect(vctx, None, obj=o, region=(0, beg, end))
            want, wv, _ = vr.call(P, NAMES, genome, region=(0, beg, end))
            assert err is None and text == want and [v[:6] for v in vals] == [v[:6] for v in wv], (beg, end)
        got = lambda b, e: {v[1] for v in collect(vctx, None, obj=o, region=(0, b, e))[1]}
        assert got(a, a + 21) == {a, a + 20} and got(a + 1, a + 20) == set() and got(a, a) == set()   # anchors at beg and end - 1 stay, at beg - 1 and end go
        assert got(170_000, 180_000) == set() and got(190_009, 190_025) == {190_009, 190_024}         # the wide record overlaps: its anchors lie outside
        for bad in (-1, 3):
            with pytest.raises(LraError):
                list(o.fetch(bad, 0, 10))
        assert collect(vctx, None, obj=o)[0] == whole                               # a whole pass behind region passes
    finally:
        o.close()
    o = BamVcf(vctx, bam)
    try:
        with pytest.raises(LraError, match="without an index"):
            list(o.fetch(0, 0, 100))
    finally:
        o.close()


# ---- filters ---------------------------------------------------------------------------------------------------------------------------------------------
def test_filters(vctx, tmp_path):
    rng = np.random.default_rng(9)
    genome = genome_of([2000])
    recs = [rec(pos=20 * k, flag=f, mapq=q, name=b"f%d" % k, ops=cig("5M2I5M"), rng=rng) for k, (f, q) in enumerate(
        [(0, 60), (16, 20), (0, 19), (4, 60), (256, 60), (512, 60), (1024, 60), (2048, 60), (1, 60), (3, 21), (0x100 | 16, 60)])]
    n = {}
    for key, kw in (("default", {}), ("q20", dict(min_mapq=20)), ("q21", dict(min_mapq=21)), ("f1", dict(require=1)), ("f3q21", dict(require=3, min_mapq=21)),
                    ("F0", dict(exclude=0)), ("F704", dict(exclude=0x704)), ("F10", dict(exclude=0x10))):
        n[key] = len(check(vctx, tmp_path, recs, genome, **kw)[2])
    assert n == {"default": 10, "q20": 9, "q21": 8, "f1": 2, "f3q21": 1, "F0": 11, "F704": 6, "F10": 9}   # the default drops flag 4 only


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_no_genome_and_other_genomes(tmp_path):
    from lra_amd.bam import BamVcf
    from lra_amd._lib import LraError
    from lra_amd.context import Context
    ref_len = [3000, 2000]
    genome = genome_of(ref_len)
    path = write(tmp_path, "g.bam", mc.run_bytes(many(20), ref_len=ref_len))
    c = Context(0)
    try:
        with pytest.raises(LraError, match="no genome"):
            BamVcf(c, path)
        load(c, genome[:1])
        with pytest.raises(LraError, match="2 references and the genome 1 chromosomes"):
            BamVcf(c, path)
        load(c, [genome[0], genome[1][:-1]])
        with pytest.raises(LraError, match=r"reference 1 \(chr2\): has 2000 bases in the BAM header and 1999 in the genome"):
            BamVcf(c, path)
        load(c, genome)
        o = BamVcf(c, path)
        want = vr.call([parse(r) for r in many(20)], NAMES, genome)[0]
        assert b"".join(p[2] for p in o.fetch()) == want
        load(c, [genome[0][:-5], genome[1]])                                       # another genome behind the object's back: the next pass refuses
        with pytest.raises(LraError, match=r"reference 0 \(chr1\)"):
            list(o.fetch())
        load(c, genome)
        assert b"".join(p[2] for p in o.fetch()) == want
        o.close()
    finally:
        c.close()


def test_bad_records_are_refused(vctx, tmp_path):
    from lra_amd.bam import BamVcf, VcfPiece
    ref_len = [12_000, 500]
    genome = genome_of(ref_len)
    load(vctx, genome)
    good = many(100)
    rng = np.random.default_rng(10)
    l_name = good[70][12]
    put = lambda r, at, b: r[:at] + b + r[at + len(b):]
    cases = [(put(good[70], 36 + l_name, struct.pack("<I", op(30, 9))), "op code above 8"),
             (rec(pos=7000, name=b"g0070", ops=cig("30M3I20M2D40="), seq=bases(rng, 92)), "do not sum to its l_seq"),
             (rec(pos=11_990, name=b"g0070", ops=cig("5M2I6M"), rng=rng), "beyond its reference"),
             (rec(ref=1, pos=400, name=b"g0070", ops=cig("50M2I40M20D11M"), rng=rng), "beyond its reference")]
    for bad, why in cases:
        bam, bai, recs = indexed_file(tmp_path, "bad.bam", good[:70] + [bad] + good[71:], ref_len, level=0)
        at = recs.index(bad)                                                       # (the file is sorted: where the bad record stands)
        P = [parse(r) for r in recs[:at]]
        want = vr.call(P, NAMES, genome)[0]
        o = BamVcf(vctx, bam, bai, values=True)
        try:
            for _ in range(2):                                                     # the second pass says the same
                text, vals, _, err = collect(vctx, None, obj=o)
                assert text == want and err and why in err and "record %d" % at in err and bam in err and "lra_bam_vcf" in err, err
                p = VcfPiece()
                assert vctx.lib.lra_bam_vcf_next(o.h, ctypes.byref(p)) == 0 and not p.n_variants and not p.text_len   # the pass is over
                text, vals, _, err = collect(vctx, None, obj=o, region=(0, 0, 3000))   # a fresh pass in front of the bad record runs to its end
                assert err is None and text == vr.call(P, NAMES, genome, region=(0, 0, 3000))[0] and len(vals) == 60
        finally:
            o.close()
    recs = list(good)
    recs[70] = rec(pos=11_989, name=b"fits", ops=cig("5M2I6M"), rng=rng)            # ends with the reference's last base: taken
    check(vctx, tmp_path, recs, genome, load_it=False)
    recs[70] = rec(pos=7000, flag=4, name=b"filtered", ops=cig("30M3I"), seq=b"ACGT")   # not walked: its sums are nobody's business
    check(vctx, tmp_path, recs, genome, load_it=False)


def test_lifetime(vctx, tmp_path):
    from lra_amd.bam import BamVcf
    genome = genome_of([400_000])
    load(vctx, genome)
    recs = many(3000)
    path = write(tmp_path, "l.bam", mc.run_bytes(recs, level=0, ref_len=[400_000]))
    want = vr.call([parse(r) for r in recs], NAMES, genome)[0]
    o = BamVcf(vctx, path, window_bytes=65536)
    it = o.fetch()
    next(it)
    assert b"".join(p[2] for p in o.fetch()) == want                                  # a new pass over one that was left
    it = o.fetch()
    next(it)
    o.close()                                                                       # destroyed mid-pass
    with pytest.raises(Exception):
        BamVcf(vctx, path, text=False, values=False)
