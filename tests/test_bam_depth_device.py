"""lra_bam_depth on crafted BAM files: values and text, per base and binned, equal tests/depth_ref.py's loop -- every op kind, the CG:B:I form, the
position window at its edges (a record ending at and beyond it, growth, prefixes, slides, the jump), bins that cut pieces, regions through the .bai,
the filters -- and what it refuses it refuses with final pieces delivered first and another pass possible."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_text as bt                                                             # noqa: E402
import bam_merge_cases as mc                                                      # noqa: E402
import bam_text                                                                   # noqa: E402
import depth_ref as dr                                                            # noqa: E402

pytestmark = pytest.mark.gpu

REF_LEN = mc.REF_LEN
NAMES = [b"chr%d" % (i + 1) for i in range(8)]
SPAN = 65536


def op(n, code):
    return (n << 4) | code


def rec(ref=0, pos=100, flag=0, name=b"r", ops=(), l_seq=0, tags=b"", mapq=60):
    """a record with the fields depth reads chosen (the view test's builder, without SEQ / QUAL / mate choices)"""
    span = sum(o >> 4 for o in ops if (o & 15) in bt.CONSUMES_REF)
    bin_ = 4680 if ref < 0 else bt.reg2bin(pos, pos + max(span, 1))
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, mapq, bin_, len(ops), flag, l_seq, -1, -1, 0) + name + b"\0"
    body += struct.pack("<%dI" % len(ops), *ops) + bytes((l_seq + 1) // 2) + b"\xff" * l_seq + tags
    return struct.pack("<I", len(body)) + body


def parse(r):
    """a record's bytes -> the oracle's (ref, pos, flag, mapq, ops)"""
    ref, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", r, 4)
    at = 36 + l_name
    ops = list(struct.unpack_from("<%dI" % n_cig, r, at))
    if n_cig == 2 and ops[0] == (l_seq << 4 | 4) and (ops[1] & 15) == 3:
        for t in bam_text._tags(r[at + 8 + (l_seq + 1) // 2 + l_seq:]):
            if t[0] == "CG" and t[1] == "B" and t[2].startswith("I"):
                ops = [int(v) for v in t[3]]
                break
    return ref, pos, flag, mapq, ops


def write(tmp_path, name, data):
    p = os.path.join(str(tmp_path), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def collect(ctx, path, ref_len, bai=None, region=None, keep=False, **kw):
    """one pass -> (per-base: one uint32 array per reference and a mask of the delivered positions; bins: {ref: [sums]}), the text, the stats, the error"""
    from lra_amd.bam import BamDepth
    from lra_amd._lib import LraError
    d = kw.pop("obj", None) or BamDepth(ctx, path, bai, values=True, **kw)
    bin_ = d.bin
    vals = [np.zeros(n, np.uint32) for n in ref_len]
    seen = [np.zeros(n, bool) for n in ref_len]
    sums, nxt, text, err = {}, {}, [], None
    try:
        for ref, first, count, v, t in d.fetch(*(region or ())):
            text.append(t)
            assert v is not None and len(v) == count
            if bin_:
                assert first == nxt.get(ref, first), "bins come once and in order"
                sums.setdefault(ref, []).extend(int(x) for x in v)
                nxt[ref] = first + count * bin_
            else:
                assert not seen[ref][first:first + count].any(), "a position came twice"
                vals[ref][first:first + count] = v
                seen[ref][first:first + count] = True
    except LraError as e:
        err = str(e)
    st = d.stats()
    if not keep:
        d.close()
    return (sums if bin_ else (vals, seen)), b"".join(text), st, err


def whole_text(d, ref_len, bin_=0, all_positions=False):
    if bin_:
        return b"".join(dr.bin_text(NAMES[r], d[r], 0, n, bin_) for r, n in enumerate(ref_len))
    return b"".join(dr.base_text(NAMES[r], d[r], 0, n, all_positions) for r, n in enumerate(ref_len))


def check(ctx, tmp_path, recs, ref_len=REF_LEN, bins=(7,), modes=(False, True), name="x.bam", level=1, oracle_kw=None, **kw):
    """the whole file: per base (without and with -a) and binned, values and text, against the oracle"""
    path = write(tmp_path, name, mc.run_bytes(recs, level=level, ref_len=ref_len))
    okw = dict(oracle_kw or {})
    for k in ("require", "exclude", "min_mapq", "count_deletions"):
        if k in kw and kw[k] is not None:
            okw[k] = kw[k]
    d = dr.depth([parse(r) for r in recs], ref_len, **okw)
    st = None
    for a in modes:
        (vals, seen), text, st, err = collect(ctx, path, ref_len, all_positions=a, **kw)
        assert err is None, err
        for r in range(len(ref_len)):
            assert np.array_equal(vals[r], d[r]), (a, r, np.nonzero(vals[r] != d[r])[0][:10])
            assert seen[r].all() if a else seen[r][d[r] > 0].all()
        assert text == whole_text(d, ref_len, 0, a), a
    for b in bins:
        sums, text, st, err = collect(ctx, path, ref_len, bin=b, **kw)
        assert err is None, err
        for r, n in enumerate(ref_len):
            assert sums.get(r, []) == dr.bin_sums(d[r], 0, n, b), (b, r)
        assert text == whole_text(d, ref_len, b), b
    return path, d, st


# ---- ops -----------------------------------------------------------------------------------------------------------------------------------------------
def op_records():
    r = [rec(pos=10 + 40 * c, name=b"k%d" % c, ops=[op(5, 7), op(3 + c, c), op(4, 7)]) for c in range(9)]          # every op kind between two = runs
    r.append(rec(pos=400, name=b"clips", ops=[op(3, 5), op(4, 4), op(10, 0), op(2, 4), op(1, 5)], l_seq=16))
    r.append(rec(pos=420, name=b"eie", ops=[op(5, 7), op(2, 1), op(5, 7), op(1, 6), op(3, 8)]))
    r.append(rec(pos=440, name=b"ede", ops=[op(5, 7), op(2, 2), op(5, 7), op(1, 1), op(3, 2), op(2, 1), op(4, 8)]))
    r.append(rec(pos=470, name=b"cut", ops=[op(6, 7), op(1, 8), op(30, 3), op(2, 7), op(1, 1), op(30, 3), op(5, 0)]))
    r.append(rec(pos=600, name=b"none", ops=[]))
    r.append(rec(pos=600, name=b"d_first", ops=[op(3, 2), op(4, 7), op(2, 2)]))
    r += [rec(pos=700, name=b"twin%d" % k, ops=[op(20, 7)]) for k in range(2)]
    r.append(rec(pos=720, name=b"touch", ops=[op(20, 7)]))                          # begins where the twins end: + 1 and - 1 in one cell
    return r


@pytest.mark.parametrize("dels", [False, True])
def test_every_op_kind(ctx, tmp_path, dels):
    _, d, _ = check(ctx, tmp_path, op_records(), ref_len=[2000], bins=(1, 7, 1000, 5000), count_deletions=dels)
    assert d[0][10 + 80 + 5] == (1 if dels else 0) and d[0][719] == 2 and d[0][720] == 1


def test_contention_and_digits(ctx, tmp_path):
    """5000 records on one pos and CIGAR, and records stacked so that the depth's text crosses 9 -> 10, 99 -> 100 and 999 -> 1000"""
    recs = [rec(pos=50, name=b"s%d" % k, ops=[op(1200 - k, 7)]) for k in range(1100)]
    recs += [rec(pos=3000, name=b"c%d" % k, ops=[op(30, 7), op(5, 2), op(30, 8)]) for k in range(5000)]
    _, d, st = check(ctx, tmp_path, recs, ref_len=[5000], bins=(1000,))
    assert d[0][3000] == 5000 and d[0][3032] == 0 and {9, 10, 99, 100, 999, 1000} <= set(int(x) for x in d[0][50:1300])
    assert st["depth_max"] == 5000


def test_cg_form(ctx, tmp_path):
    ops = [op(2, 7 if k % 2 else 1) for k in range(70000)]
    a = bt.cg_record(1, 500, 16, b"cgform", ops, 70000)
    b = rec(pos=900, name=b"kept", ops=[op(4, 4), op(6, 3)], l_seq=5, tags=b"CGBI" + struct.pack("<II", 1, op(9, 0)), ref=1)   # <l_seq>S<n>N it is not: the core ops count
    c = rec(pos=1000, name=b"second", ops=[op(4, 4), op(6, 3)], l_seq=4, tags=b"XAC\x07" + b"CGBI" + struct.pack("<III", 2, op(4, 0), op(2, 2)) + b"XBZok\0", ref=1)
    e = rec(pos=1100, name=b"notag", ops=[op(4, 4), op(6, 3)], l_seq=4, ref=1)
    _, d, _ = check(ctx, tmp_path, [a, b, c, e], bins=(1000,), modes=(False,))
    assert d[1][70499] == 1 and d[1][70500] == 0 and d[1][900] == 1 and d[1][1000] == 2 and d[1][1004] == 1 and d[1][1100] == 1


# ---- the position window --------------------------------------------------------------------------------------------------------------------------------
def test_window_edges_and_growth(ctx, tmp_path):
    recs = [rec(pos=1000, name=b"at", ops=[op(SPAN, 7)]), rec(pos=1000, name=b"beyond", ops=[op(SPAN + 1, 7)]),
            rec(pos=1000 + SPAN, name=b"next", ops=[op(10, 7)]),
            rec(pos=150000, name=b"long", ops=[op(100000, 7), op(7, 2), op(99993, 8)]), rec(pos=150010, name=b"in", ops=[op(5, 0)])]
    _, d, st = check(ctx, tmp_path, recs, bins=(1000, 7), span_bases=SPAN)
    assert d[0][1000 + SPAN] == 2 and d[0][349999] == 1 and d[0][350000] == 0


def test_prefixes_and_slides(ctx, tmp_path):
    """3000 short records 200 bases apart: a window's records span more than the span, and several windows follow"""
    recs = [rec(pos=200 * i, name=b"p%04d" % i, ops=[op(150, 7), op(20, 2), op(150, 8)], l_seq=40) for i in range(3000)]
    path, d, st = check(ctx, tmp_path, recs, ref_len=[700000, 1000], bins=(1000,), level=0, span_bases=SPAN, window_bytes=65536)
    assert 5 <= st["windows"] <= 8 and st["slides"] > st["windows"]              # (a window's 500 records reach over 100 000 positions)


def test_far_record_jumps(ctx, tmp_path):
    """one record at 500 000 000 of a 2^29-base reference: the base jumps, nothing in between is scanned"""
    ref_len = [1 << 29, 1000]
    at = 500_000_000
    recs = [rec(pos=at, name=b"far", ops=[op(30, 7), op(4, 2), op(10, 8)]), rec(ref=1, pos=5, name=b"b", ops=[op(3, 0)])]
    path = write(tmp_path, "far.bam", mc.run_bytes(recs, ref_len=ref_len))
    d = dr.depth([(0, 1000, 0, 60, parse(recs[0])[4]), parse(recs[1])], [2000, 1000])
    from lra_amd.bam import BamDepth
    o = BamDepth(ctx, path, values=True, span_bases=SPAN)
    try:
        pieces = [(ref, first, v.copy(), t) for ref, first, _, v, t in o.fetch()]
        st = o.stats()
    finally:
        o.close()
    want = b"".join(b"chr1\t%d\t%d\n" % (at - 1000 + p + 1, d[0][p]) for p in range(2000) if d[0][p]) + dr.base_text(b"chr2", d[1], 0, 1000)
    assert b"".join(p[3] for p in pieces) == want
    got = np.zeros(2000, np.uint32)
    for ref, first, v, _ in pieces:
        if ref == 0:
            assert at - 1000 <= first and first + len(v) <= at + 1000
            got[first - (at - 1000):first - (at - 1000) + len(v)] = v
    assert np.array_equal(got, d[0]) and sum(len(p[2]) for p in pieces) < 2 * SPAN
    assert st["slides"] <= st["windows"] + len(ref_len) + 4


def test_bins_and_empty_reference(ctx, tmp_path):
    """an empty reference between two used ones; a bin larger than the range; ragged last bins (123 457 is a multiple of neither 7 nor 1000)"""
    recs = [rec(ref=0, pos=399_000, name=b"a", ops=[op(1000, 7)]), rec(ref=0, pos=399_990, name=b"tail", ops=[op(10, 0)]),
            rec(ref=2, pos=0, name=b"c", ops=[op(3333, 7)]), rec(ref=2, pos=249_999, name=b"last", ops=[op(1, 8)])]
    ref_len = [400_000, 123_457, 250_000]
    _, d, _ = check(ctx, tmp_path, recs, ref_len=ref_len, bins=(1, 7, 1000, 1 << 20), span_bases=SPAN)
    assert d[1].sum() == 0 and ref_len[1] % 7 and ref_len[1] % 1000


# ---- invariance -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_sorted():
    recs = sorted(mc.fixture_records(), key=bt.sort_key)
    d = dr.depth([parse(r) for r in recs], REF_LEN)
    return recs, d, whole_text(d, REF_LEN), whole_text(d, REF_LEN, 1000)


def test_invariance(ctx, tmp_path, fixture_sorted):
    recs, d, text, btext = fixture_sorted
    path = write(tmp_path, "f.bam", mc.run_bytes(recs, level=0))
    for window in (65536, 0):
        for span in (65536, 1 << 20, 0):
            (vals, _), got, st, err = collect(ctx, path, REF_LEN, window_bytes=window, span_bases=span)
            assert err is None, err
            assert all(np.array_equal(vals[r], d[r]) for r in range(3)) and got == text, (window, span)
            _, got, _, err = collect(ctx, path, REF_LEN, bin=1000, window_bytes=window, span_bases=span)
            assert err is None and got == btext, (window, span)
    assert st["records_read"] == 5000 and st["records_counted"] + st["records_filtered"] == 5000 and st["covered"] == sum(int((x > 0).sum()) for x in d)
    assert st["depth_sum"] == sum(int(x.sum()) for x in d) and st["depth_max"] == max(int(x.max()) for x in d)


# ---- regions ----------------------------------------------------------------------------------------------------------------------------------------------
def indexed_file(tmp_path, name, recs, level=1, ref_len=REF_LEN):
    from lra_amd import bgzf
    recs = sorted(recs, key=bt.sort_key)
    raw = b"".join(recs)
    head = bgzf.bgzf_compress(mc.header_bytes(ref_len), 6, eof=False)
    members = [bgzf.bgzf_compress(raw[a:a + bt.MEMBER], level, eof=False) for a in range(0, len(raw), bt.MEMBER)]
    moff = bt.member_table(len(raw), [len(m) for m in members])
    bam = write(tmp_path, name, head + b"".join(members) + mc.EOF_BLOCK)
    bai = write(tmp_path, name + ".bai", bt.build(raw, len(ref_len), moff, len(head)))
    return bam, bai


def region_check(ctx, objs, d, ref, beg, end):
    end_c = min(end, len(d[ref]))
    (vals, seen), text, _, err = collect(ctx, None, [len(x) for x in d], region=(ref, beg, end), obj=objs[0], keep=True)
    assert err is None, err
    assert np.array_equal(vals[ref][beg:end_c], d[ref][beg:end_c]) and not seen[ref][:beg].any() and not seen[ref][end_c:].any(), (ref, beg, end)
    assert text == dr.base_text(NAMES[ref], d[ref], beg, end_c), (ref, beg, end)
    sums, text, _, err = collect(ctx, None, [len(x) for x in d], region=(ref, beg, end), obj=objs[1], keep=True)
    assert err is None and sums.get(ref, []) == dr.bin_sums(d[ref], beg, end_c, 500) and text == dr.bin_text(NAMES[ref], d[ref], beg, end_c, 500), (ref, beg, end)


def test_regions_random(ctx, tmp_path, fixture_sorted):
    from lra_amd.bam import BamDepth
    recs, d, _, _ = fixture_sorted
    bam, bai = indexed_file(tmp_path, "s.bam", recs)
    objs = [BamDepth(ctx, bam, bai, values=True), BamDepth(ctx, bam, bai, values=True, bin=500)]
    rng = np.random.default_rng(11)
    try:
        for k in range(200):
            ref = int(rng.integers(0, 3))
            beg = int(rng.integers(0, REF_LEN[ref]))
            end = min(REF_LEN[ref], beg + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 18)))))
            region_check(ctx, objs, d, ref, beg, end)
        region_check(ctx, objs, d, 2, REF_LEN[2] - 10, 10 ** 12)                  # end is clamped
        region_check(ctx, objs, d, 0, 0, REF_LEN[0])
        (vals, seen), text, _, err = collect(ctx, None, REF_LEN, obj=objs[0], keep=True)   # a whole pass behind region passes
        assert err is None and all(np.array_equal(vals[r], d[r]) for r in range(3))
    finally:
        for o in objs:
            o.close()


def test_regions_crafted(ctx, tmp_path):
    from lra_amd.bam import BamDepth
    from lra_amd._lib import LraError
    ref_len = [200_000, 5000, 5000]
    recs = [rec(pos=9_990, name=b"a", ops=[op(30, 7), op(10, 2), op(30, 7)]), rec(pos=99_990, name=b"b", ops=[op(40, 7)]), rec(pos=150_000, name=b"l", ops=[op(10, 0)]),
            rec(ref=2, pos=7, name=b"c", ops=[op(5, 0)])]
    bam, bai = indexed_file(tmp_path, "c.bam", recs, ref_len=ref_len)
    d = dr.depth([parse(r) for r in recs], ref_len)
    objs = [BamDepth(ctx, bam, bai, values=True, all_positions=True), BamDepth(ctx, bam, bai, values=True, bin=500)]
    try:
        for ref, beg, end in ((0, 10_000, 10_010), (0, 10_025, 10_035), (0, 9_990, 9_991), (0, 10_059, 10_060), (0, 10_060, 10_061), (0, 5, 5), (0, 160_000, 170_000),
                              (1, 0, 5000), (0, 9_995, 10_005), (0, 99_995, 100_005), (2, 0, 5000)):
            end_c = min(end, ref_len[ref])
            (vals, seen), text, _, err = collect(ctx, None, ref_len, region=(ref, beg, end), obj=objs[0], keep=True)
            assert err is None and np.array_equal(vals[ref][beg:end_c], d[ref][beg:end_c]) and seen[ref].sum() == end_c - beg, (ref, beg, end)
            assert text == dr.base_text(NAMES[ref], d[ref], beg, end_c, True), (ref, beg, end)
            sums, text, _, err = collect(ctx, None, ref_len, region=(ref, beg, end), obj=objs[1], keep=True)
            assert err is None and text == dr.bin_text(NAMES[ref], d[ref], beg, end_c, 500), (ref, beg, end)
        assert b"\t9999\t1\nchr1\t10000\t1\n" in dr.base_text(NAMES[0], d[0], 9_995, 10_005) and b"\t99999\t1\nchr1\t100000\t1\n" in dr.base_text(NAMES[0], d[0], 99_995, 100_005)
    finally:
        for o in objs:
            o.close()
    o = BamDepth(ctx, bam)
    try:
        with pytest.raises(LraError, match="without an index"):
            list(o.fetch(0, 0, 100))
        assert b"".join(p[4] for p in o.fetch()) == whole_text(d, ref_len)
    finally:
        o.close()


# ---- filters ----------------------------------------------------------------------------------------------------------------------------------------------
def test_filters(ctx, tmp_path):
    recs = [rec(pos=10 * k, flag=f, mapq=q, name=b"f%d" % k, ops=[op(25, 7)]) for k, (f, q) in enumerate(
        [(0, 60), (16, 20), (0, 19), (4, 60), (256, 60), (512, 60), (1024, 60), (2048, 60), (1, 60), (3, 21), (0x100 | 16, 60)])]
    recs += [rec(ref=-1, pos=-1, flag=4, name=b"u%d" % k, l_seq=10) for k in range(5)]
    for kw in (dict(), dict(min_mapq=20), dict(min_mapq=21), dict(require=1), dict(require=3, min_mapq=21), dict(exclude=0), dict(exclude=0x4), dict(exclude=0x700)):
        check(ctx, tmp_path, recs, ref_len=[1000], bins=(), modes=(False,), **kw)
    P = [parse(r) for r in recs]
    tot = lambda **k: int(dr.depth(P, [1000], **k)[0].sum())
    assert tot(min_mapq=20) - tot(min_mapq=21) == 25 and tot() - tot(min_mapq=20) == 25                     # mapq == min_mapq is kept, one below is dropped
    assert tot(exclude=0) - tot() == 5 * 25 and tot(exclude=0x4) - tot(exclude=0) == -25 and tot(exclude=0x700) - tot() == 25 and tot(require=1) == 50


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def refusal(ctx, tmp_path, recs, bad_at, text, data=None, good=None, **kw):
    """the file is refused naming `text`; what came first is the oracle's values of all the good records at the delivered positions; a second pass says the same"""
    import ctypes
    from lra_amd.bam import BamDepth, DepthPiece
    path = write(tmp_path, "bad.bam", data if data is not None else mc.run_bytes(recs, level=0))
    good = [r for k, r in enumerate(recs) if k != bad_at] if good is None else good
    d = dr.depth([parse(r) for r in good], REF_LEN)
    o = BamDepth(ctx, path, values=True, **kw)
    try:
        for _ in range(2):
            (vals, seen), got, _, err = collect(ctx, None, REF_LEN, obj=o, keep=True)
            assert err and all(t in err for t in text.split("|")) and path in err, err
            for r in range(3):
                assert np.array_equal(vals[r][seen[r]], d[r][seen[r]])
            lines = got.split(b"\n")[:-1]
            assert all(ln == b"%s\t%d\t%d" % (NAMES[0], int(ln.split(b"\t")[1]), d[0][int(ln.split(b"\t")[1]) - 1]) for ln in lines)
            p = DepthPiece()
            assert ctx.lib.lra_bam_depth_next(o.h, ctypes.byref(p)) == 0 and not p.count and not p.text_len   # the pass is over
        return seen
    finally:
        o.close()


def many(n=900):
    return [rec(pos=100 * i, name=b"g%04d" % i, ops=[op(60, 7), op(3, 1), op(70, 8)], l_seq=133) for i in range(n)]


def test_unsorted_is_refused(ctx, tmp_path):
    recs = many()
    recs[70], recs[71] = recs[71], recs[70]
    seen = refusal(ctx, tmp_path, recs, None, "not coordinate-sorted at record 71", good=recs[:71])
    assert seen[0][:6900].all()
    # across a window edge: the swap is wherever the second window begins
    from lra_amd.bam import BamDepth
    recs = many(3000)
    path = write(tmp_path, "probe.bam", mc.run_bytes(recs, level=0))
    o = BamDepth(ctx, path, window_bytes=65536)
    list(o.fetch())
    assert o.stats()["windows"] >= 3
    o.close()
    per = len(recs[0])
    k = (65536 - 200) // per                                                       # about the first record behind the first window
    hit = 0
    for j in range(k - 3, k + 4):
        r2 = list(recs)
        r2[j - 1], r2[j] = r2[j], r2[j - 1]
        refusal(ctx, tmp_path, r2, None, "not coordinate-sorted at record %d" % j, good=r2[:j], window_bytes=65536)
        hit += 1
    assert hit == 7


def test_bad_records_are_refused(ctx, tmp_path):
    recs = many(100)
    put = lambda r, at, b: r[:at] + b + r[at + len(b):]
    l_name = recs[70][12]
    for bad, text in ((put(recs[70], 36 + l_name, struct.pack("<I", op(5, 9))), "op code above 8"),
                      (put(recs[70], 20, struct.pack("<I", 40000)), "shorter than its fields")):
        r2 = list(recs)
        r2[70] = bad
        seen = refusal(ctx, tmp_path, r2, 70, text + "|record 70")
        assert seen[0][:6900].all()


def test_file_faults(ctx, tmp_path):
    from lra_amd import bgzf
    recs = many(2000)
    good = mc.run_bytes(recs, level=0)
    head = len(bgzf.bgzf_compress(mc.header_bytes(), 6, eof=False))
    sizes, at = [], head
    while at < len(good):
        n = struct.unpack_from("<H", good, at + 16)[0] + 1
        sizes.append((at, n)); at += n
    refusal(ctx, tmp_path, recs, None, "cut by the end of the file", data=good[:sizes[3][0]], good=recs)   # (the third member ends inside a record)
    m_at, m_len = sizes[2]
    hurt = bytearray(good); hurt[m_at + m_len // 2] ^= 0x55
    refusal(ctx, tmp_path, recs, None, "CRC", data=bytes(hurt), good=recs)


# ---- lifetime ---------------------------------------------------------------------------------------------------------------------------------------------
def test_lifetime(ctx, tmp_path, fixture_sorted):
    from lra_amd.bam import BamDepth
    recs, d, text, _ = fixture_sorted
    big = write(tmp_path, "big.bam", mc.run_bytes(recs))
    small_recs = [rec(pos=5, name=b"s", ops=[op(3, 0)])]
    small = write(tmp_path, "small.bam", mc.run_bytes(small_recs))
    o = BamDepth(ctx, big)
    assert b"".join(p[4] for p in o.fetch()) == text and b"".join(p[4] for p in o.fetch()) == text   # two passes on one object
    it = o.fetch()
    next(it)
    o.close()                                                                       # destroyed mid-pass
    o = BamDepth(ctx, small)
    assert b"".join(p[4] for p in o.fetch()) == b"chr1\t6\t1\nchr1\t7\t1\nchr1\t8\t1\n"
    o.close()
    o = BamDepth(ctx, big, span_bases=SPAN)
    it = o.fetch()
    next(it)
    assert b"".join(p[4] for p in o.fetch()) == text                                  # a new pass over one that was left
    o.close()
