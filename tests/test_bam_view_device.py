"""lra_bam_view on crafted BAM files: the text it prints equals tests/bam_text.py's lines byte for byte -- whole files of every shape, every CIGAR, SEQ, QUAL
and aux form, small windows, flag filters -- region passes through the .bai equal the brute-force overlap set in file order, and what the view refuses
it refuses with the records in front delivered and another pass possible."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_text as bt                                                             # noqa: E402
import bam_merge_cases as mc                                                      # noqa: E402
import bam_text                                                                   # noqa: E402

pytestmark = pytest.mark.gpu

REF_LEN = mc.REF_LEN
REFS = [(b"chr%d" % (i + 1), n) for i, n in enumerate(REF_LEN)]


def even_tail(rec):
    """make_record's filler leaves bits in the unused nibble behind an odd l_seq, which bam_text refuses: clear it"""
    l_name, n_cig, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    if l_seq % 2 == 0:
        return rec
    at = 36 + l_name + 4 * n_cig + l_seq // 2
    return rec[:at] + bytes([rec[at] & 0xf0]) + rec[at + 1:]


def rec(ref=0, pos=100, flag=0, name=b"r", ops=(), l_seq=0, qual=None, tags=b"", nref=-1, npos=-1, tlen=0, mapq=60, seq=None):
    """a record with every field chosen; qual None: 0xff bytes"""
    span = sum(o >> 4 for o in ops if (o & 15) in bt.CONSUMES_REF)
    bin_ = 4680 if ref < 0 else bt.reg2bin(pos, pos + max(span, 1))
    if seq is None:
        seq = bytes((37 * k + 11 * l_seq) & 255 for k in range((l_seq + 1) // 2))
        if l_seq % 2:
            seq = seq[:-1] + bytes([seq[-1] & 0xf0])
    q = b"\xff" * l_seq if qual is None else bytes(qual)
    assert len(q) == l_seq and len(seq) == (l_seq + 1) // 2
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, mapq, bin_, len(ops), flag, l_seq, nref, npos, tlen) + name + b"\0"
    body += struct.pack("<%dI" % len(ops), *ops) + seq + q + tags
    return struct.pack("<I", len(body)) + body


def lines_of(recs):
    raw = b"".join(recs)
    return [ln + b"\n" for _, _, ln in bam_text.records(raw, REFS)]


def write(tmp_path, name, data):
    p = os.path.join(str(tmp_path), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def view_all(ctx, path, window=0, flags=None, bai=None):
    from lra_amd.bam import BamView
    v = BamView(ctx, path, bai, window)
    try:
        if flags:
            v.set_flags(*flags)
        return b"".join(v.fetch())
    finally:
        v.close()


def check_whole(ctx, tmp_path, recs, name="x.bam", window=0, **kw):
    path = write(tmp_path, name, mc.run_bytes(recs, **kw))
    got = view_all(ctx, path, window)
    want = b"".join(lines_of(recs))
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        k = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
        raise AssertionError("line %d of %d / %d:\n got %r\nwant %r" % (k, len(g), len(w), g[k][:300] if k < len(g) else None, w[k][:300] if k < len(w) else None))
    return path


@pytest.fixture(scope="module")
def fixture_records():
    return [even_tail(r) for r in mc.fixture_records()]


@pytest.fixture(scope="module")
def fixture_lines(fixture_records):
    return lines_of(fixture_records)


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_whole_file_small(ctx, tmp_path, fixture_records, n):
    check_whole(ctx, tmp_path, fixture_records[:n])


def test_whole_file_5000(ctx, tmp_path, fixture_records, fixture_lines):
    """with the 65535-op record, the 70000-op CG:B:I record (restored, its tag dropped), records above 4096 and above 65280 bytes"""
    path = write(tmp_path, "f.bam", mc.run_bytes(fixture_records))
    from lra_amd.bam import BamView
    v = BamView(ctx, path)
    try:
        got = b"".join(v.fetch())
        assert v.last_records == 5000
        text, names, lens = v.header()
        assert text == b"@HD\tVN:1.6\tSO:coordinate\n" and names == [n for n, _ in REFS] and lens == REF_LEN
        s = v.stats()
        assert s["records"] == 5000 and s["bytes_text"] == len(got) and s["bytes_read"] == os.path.getsize(path)
    finally:
        v.close()
    assert got == b"".join(fixture_lines)
    cg = [ln for ln in fixture_lines if ln.startswith(b"cgform\t")][0]
    assert b"CG:B" not in cg and cg.split(b"\t")[5].count(b"=") == 35000


def test_small_window_streams(ctx, tmp_path, fixture_records, fixture_lines):
    """65536 compressed bytes per step over a stored file of many windows; the 280 KB record is larger than four of them"""
    data = mc.run_bytes(fixture_records, level=0)
    assert len(data) >= 10 * 65536 and max(len(r) for r in fixture_records) > 280_000
    path = write(tmp_path, "w.bam", data)
    from lra_amd.bam import BamView
    v = BamView(ctx, path, None, 1)                                               # (raised to 65536)
    try:
        pieces = list(v.fetch())
        assert v.stats()["windows"] >= 10 and len(pieces) >= 10
        assert all(p.endswith(b"\n") for p in pieces)
    finally:
        v.close()
    assert b"".join(pieces) == b"".join(fixture_lines)


def test_file_shapes(ctx, tmp_path, fixture_records):
    recs = fixture_records[:300]
    n = len(mc.header_bytes()) + len(b"".join(recs))

    def cuts(first, steps):                                                       # members of these sizes, over and over, behind the first cuts
        out = list(first)
        while out[-1] < n:
            out.append(out[-1] + steps[len(out) % len(steps)])
        return out
    check_whole(ctx, tmp_path, recs, "a.bam", header_member=False)                # records in the header's member
    check_whole(ctx, tmp_path, recs, "b.bam", eof=False)                          # no EOF member
    check_whole(ctx, tmp_path, recs, "c.bam", cuts=cuts([1, 5, 37, 4000, 4001], [65536, 1000, 30001, 1, 65280]))   # uneven members
    check_whole(ctx, tmp_path, recs, "d.bam", header_member=False, eof=False, cuts=cuts([100], [65536, 7, 50000]), window=65536)


def op(n, code):
    return (n << 4) | code


def test_cigars(ctx, tmp_path):
    recs = [rec(name=b"none", ops=[]), rec(name=b"one", ops=[op(1, 0)]),
            rec(name=b"lens", ops=[op(n, 0) for n in (1, 9, 10, 99, 100, 99999999, 268435455)], ref=2, pos=0),
            rec(name=b"codes", ops=[op(3 + c, c) for c in range(9)], l_seq=9),
            rec(name=b"max", ops=[op(1 + k % 12, (0, 1, 2, 7, 8)[k % 5]) for k in range(65535)], l_seq=5),
            rec(name=b"after", ops=[op(7, 4), op(20, 0)], l_seq=27)]
    check_whole(ctx, tmp_path, recs)


def test_op_count_above_a_scan_tile(ctx, tmp_path):
    """4097 CIGAR ops in the window: one more than scan.h's tile, in one record and spread over many"""
    check_whole(ctx, tmp_path, [rec(name=b"t", ops=[op(1 + k % 30, k % 3) for k in range(4097)])], "a.bam")
    many = [rec(name=b"m%d" % i, pos=i, ops=[op(1 + (i + k) % 11, k % 2) for k in range(17)]) for i in range(241)]
    assert sum(struct.unpack_from("<H", r, 16)[0] for r in many) == 4097
    check_whole(ctx, tmp_path, many, "b.bam")


def test_cg_form(ctx, tmp_path):
    ops = [op(2, 7 if k % 2 else 1) for k in range(70000)]
    a = bt.cg_record(1, 500, 16, b"cgform", ops, 70000)
    b = rec(name=b"kept", ops=[op(4, 4), op(6, 3)], l_seq=5, tags=b"CGBI" + struct.pack("<II", 1, op(9, 0)))   # <l_seq>S<n>N it is not: the tag stays
    c = rec(name=b"first", ops=[op(4, 4), op(6, 3)], l_seq=4, tags=b"XAC\x07" + b"CGBI" + struct.pack("<III", 2, op(4, 0), op(2, 2)) + b"XBZok\0")
    lines = lines_of([a, b])
    assert lines[0].split(b"\t")[5].endswith(b"2I2=") and b"CG:B" not in lines[0] and b"CG:B:I,144" in lines[1]
    path = write(tmp_path, "x.bam", mc.run_bytes([a, b, c]))
    got = view_all(ctx, path).split(b"\n")
    assert got[0] + b"\n" == lines[0] and got[1] + b"\n" == lines[1]
    f = got[2].split(b"\t")                                                       # (bam_text wants the tag last; the view takes it wherever it stands)
    assert f[5] == b"4M2D" and f[11:] == [b"XA:i:7", b"XB:Z:ok"]


def test_seq_and_qual(ctx, tmp_path):
    rng = np.random.default_rng(1)
    recs = []
    for n in (0, 1, 2, 7, 8, 9, 255, 256, 1000, 4099):
        q = rng.integers(0, 94, n, dtype=np.uint8).tobytes()
        s = rng.integers(0, 256, (n + 1) // 2, dtype=np.uint8).tobytes()
        if n % 2:
            s = s[:-1] + bytes([s[-1] & 0xf0])
        recs.append(rec(name=b"q%d" % n, l_seq=n, qual=q, seq=s, ops=[op(n, 0)] if n else []))
        recs.append(rec(name=b"noq%d" % n, l_seq=n, seq=s))                        # QUAL all 0xff
    recs.append(rec(name=b"", l_seq=3, qual=b"\0\x01\x5d"))                         # a name of one byte (the NUL alone)
    recs.append(rec(name=b"n" * 254, l_seq=3, qual=b"\x5d\0\x01"))
    recs.append(rec(name=b"x" * 253, l_seq=0))
    check_whole(ctx, tmp_path, recs)


def seq_end_case(target, kind, rng):
    """the first record of a file whose SEQ (kind 0) or QUAL (kind 1) ends at byte `target` of the text"""
    for pad in range(4):
        name = b"edge" + b"_" * pad
        prefix = len(lines_of([rec(name=name, l_seq=2, qual=b"!!", ops=[op(5, 0)])])[0]) - len(b"\n") - 2 - 1 - 2   # the bytes in front of SEQ
        n = target - prefix if kind == 0 else target - prefix - 1
        if kind == 1:
            if n % 2:
                continue
            n //= 2
        r = rec(name=name, l_seq=n, qual=rng.integers(0, 94, n, dtype=np.uint8).tobytes(), ops=[op(5, 0)],
                seq=rng.integers(0, 256, (n + 1) // 2, dtype=np.uint8).tobytes() if n % 2 == 0 else None)
        line = lines_of([r])[0]
        f = line.split(b"\t")
        end = len(b"\t".join(f[:10])) if kind == 0 else len(line) - 1
        assert end == target, (end, target)
        return r
    raise AssertionError("no record for %d" % target)


def test_seq_and_qual_ends_at_chunk_edges(ctx, tmp_path):
    rng = np.random.default_rng(2)
    for k, (target, kind) in enumerate((t, c) for t in (4095, 4096, 4097, 8191, 8192, 8193) for c in (0, 1)):
        recs = [seq_end_case(target, kind, rng), rec(name=b"behind", l_seq=70, qual=bytes(range(70)))]
        check_whole(ctx, tmp_path, recs, "e%d.bam" % k)


def aux_records():
    f32 = lambda *v: struct.pack("<%df" % len(v), *v)
    t = []
    t.append(b"XAAq" + b"Xbc" + struct.pack("<b", -128) + b"XcC" + struct.pack("<B", 255) + b"Xss" + struct.pack("<h", -32768) +
             b"XSS" + struct.pack("<H", 65535) + b"Xii" + struct.pack("<i", -2 ** 31) + b"XII" + struct.pack("<I", 2 ** 32 - 1) + b"Xzi" + struct.pack("<i", 0))
    t.append(b"".join(b"F%df" % k + f32(v) for k, v in enumerate((0.0, -0.0, 1e-5, 123456.7, 3.4e38, -2.5, 1e10, 0.1, 1234567.0, 7e-39))))
    t.append(b"ZeZ\0" + b"ZsZhello world\0" + b"HxH1AE301\0" + b"ZlZ" + b"y" * 5000 + b"\0")
    for st, fmt, vals in (("c", "b", (-128, 0, 127)), ("C", "B", (0, 9, 255)), ("s", "h", (-32768, -1, 32767)), ("S", "H", (0, 10, 65535)),
                          ("i", "i", (-2 ** 31, -9, 2 ** 31 - 1)), ("I", "I", (0, 99, 2 ** 32 - 1)), ("f", "f", (0.0, -0.0, 1e-5, 123456.7, 3.4e38))):
        t.append(b"B" + st.encode() + b"B" + st.encode() + struct.pack("<I%d%s" % (len(vals), fmt), len(vals), *vals) +
                 b"E" + st.encode() + b"B" + st.encode() + struct.pack("<I", 0))    # and one of 0 elements
    rng = np.random.default_rng(4)
    big = rng.integers(-2 ** 31, 2 ** 31, 10000, dtype=np.int64).astype("<i4")
    bigf = (rng.standard_normal(10000) * 10.0 ** rng.integers(-8, 9, 10000)).astype("<f4")
    t.append(b"BIBi" + struct.pack("<I", 10000) + big.tobytes() + b"NVf" + f32(0.875) + b"BFBf" + struct.pack("<I", 10000) + bigf.tobytes() + b"ENAz")
    return [rec(name=b"aux%d" % k, pos=10 * k, l_seq=k % 3, tags=tg, ops=[op(5, 0)]) for k, tg in enumerate(t)]


def test_aux_types(ctx, tmp_path):
    recs = aux_records()
    lines = lines_of(recs)
    assert b"Xi:i:-2147483648" in lines[0] and b"XI:i:4294967295" in lines[0] and b"XA:A:q" in lines[0]
    assert lines[1].rstrip(b"\n").split(b"\t")[11:16] == [b"F0:f:0", b"F1:f:-0", b"F2:f:1e-05", b"F3:f:123457", b"F4:f:3.4e+38"]
    assert b"\tZe:Z:\t" in lines[2] and b"\tEc:B:c\n" in lines[3]
    check_whole(ctx, tmp_path, recs)


def test_flag_filters(ctx, tmp_path, fixture_records, fixture_lines):
    recs, lines = fixture_records[:600], fixture_lines[:600]
    path = write(tmp_path, "x.bam", mc.run_bytes(recs))
    flag = [struct.unpack_from("<H", r, 18)[0] for r in recs]
    for req, excl in ((0, 0), (16, 0), (0, 4), (16, 2048), (256 | 16, 0), (0, 0xffff), (4, 16)):
        want = b"".join(ln for ln, f in zip(lines, flag) if (f & req) == req and (f & excl) == 0)
        assert view_all(ctx, path, flags=(req, excl)) == want, (req, excl)
    assert len({f & 0x914 for f in flag}) >= 6


# ---- regions -----------------------------------------------------------------------------------------------------------------------------------------
def indexed_file(tmp_path, name, recs, level=1, n_ref=3):
    """a sorted file with its .bai -> (bam path, bai path, raw stream)"""
    from lra_amd import bgzf
    recs = sorted(recs, key=bt.sort_key)
    raw = b"".join(recs)
    head = bgzf.bgzf_compress(mc.header_bytes(), 6, eof=False)
    members = [bgzf.bgzf_compress(raw[a:a + bt.MEMBER], level, eof=False) for a in range(0, len(raw), bt.MEMBER)]
    moff = bt.member_table(len(raw), [len(m) for m in members])
    bam = write(tmp_path, name, head + b"".join(members) + mc.EOF_BLOCK)
    bai = write(tmp_path, name + ".bai", bt.build(raw, n_ref, moff, len(head)))
    return bam, bai, raw


def brute_lines(raw, ref, beg, end):
    return b"".join(bam_text.record_line(r[4:], REFS) + b"\n" for r in bt.brute(raw, ref, beg, end))


def test_regions(ctx, tmp_path, fixture_records):
    from lra_amd.bam import BamView
    bam, bai, raw = indexed_file(tmp_path, "s.bam", fixture_records)
    rng = np.random.default_rng(9)
    recs = bt.walk(raw)
    line = [bam_text.record_line(raw[r["at"] + 4:r["next"]], REFS) + b"\n" for r in recs]

    def brute_lines(_raw, ref, beg, end):                                         # bai_text.brute's rule over the records walked once
        return b"".join(ln for r, ln in zip(recs, line) if r["ref"] == ref and r["pos"] < end and r["end"] > beg)
    v = BamView(ctx, bam, bai)
    try:
        hit = 0
        for k in range(200):
            ref = int(rng.integers(0, 3))
            beg = int(rng.integers(0, REF_LEN[ref]))
            if k % 2:
                r = recs[int(rng.integers(0, len(recs)))]
                if r["ref"] >= 0:
                    ref, beg = r["ref"], max(0, r["pos"] - int(rng.integers(0, 20000)))
            end = min(REF_LEN[ref], beg + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 22)))))
            want = brute_lines(raw, ref, beg, end)
            got = b"".join(v.fetch(ref, beg, end))
            assert got == want, (ref, beg, end, got.count(b"\n"), want.count(b"\n"))
            hit += bool(want)
        assert hit >= 50
        # by name, to the reference's end, and again: two passes on one view give the same
        a = b"".join(v.fetch("chr2"))
        assert a == brute_lines(raw, 1, 0, REF_LEN[1]) and a == b"".join(v.fetch(b"chr2", 0, None)) and a.count(b"\n") == v.last_records
        assert b"".join(v.fetch(2, REF_LEN[2] - 1, 10 ** 12)) == brute_lines(raw, 2, REF_LEN[2] - 1, REF_LEN[2])   # end is clamped
        assert b"".join(v.fetch(0, 5, 5)) == b""
        v.set_flags(16, 0)
        want = b"".join(ln for r, ln in zip(recs, line) if r["ref"] == 0 and r["pos"] < 50000 and r["end"] > 0 and r["flag"] & 16)
        assert want and b"".join(v.fetch(0, 0, 50000)) == want
        v.set_flags(0, 0)
        assert b"".join(v.fetch()) == b"".join(line)                                # a whole pass behind region passes
    finally:
        v.close()


def test_regions_small_window_and_crafted(ctx, tmp_path):
    """a region inside one 60 kb record, placed records with flag 4, an empty result; chunks longer than the window"""
    from lra_amd.bam import BamView
    recs = [rec(0, 1000, 0, b"long", [op(60000, 0)], 50), rec(0, 1200, 4, b"placed_unmapped", [], 30, qual=bytes(range(30))),
            rec(0, 30000, 16, b"inside", [op(100, 0)], 100), rec(0, 70000, 0, b"behind", [op(10, 0)], 10), rec(1, 5, 4, b"placed2", [], 0),
            rec(-1, -1, 4, b"unplaced", [], 20)]
    recs += [rec(0, 100000 + 3 * i, 16 * (i % 2), b"d%05d" % i, [op(50, 0)], 120, qual=bytes((i + k) % 90 for k in range(120)), tags=b"NVf" + struct.pack("<f", i / 8)) for i in range(3000)]
    bam, bai, raw = indexed_file(tmp_path, "c.bam", recs, level=0)
    assert os.path.getsize(bam) > 6 * 65536
    for window in (0, 65536):
        v = BamView(ctx, bam, bai, window)
        try:
            for ref, beg, end in ((0, 40000, 40010), (0, 1200, 1201), (0, 1100, 1300), (0, 61000, 69000), (0, 61000, 70001), (1, 0, 100), (1, 6, 100), (2, 0, 1000),
                                  (0, 100000, 109000), (0, 104000, 104001), (0, 0, REF_LEN[0])):
                want = brute_lines(raw, ref, beg, end)
                assert b"".join(v.fetch(ref, beg, end)) == want, (window, ref, beg, end)
            assert brute_lines(raw, 0, 40000, 40010).startswith(b"long\t") and brute_lines(raw, 0, 61000, 69000) == b"" and brute_lines(raw, 0, 1200, 1201).count(b"\n") == 2
        finally:
            v.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def pieces_then_error(v, *region):
    from lra_amd._lib import LraError
    got = []
    try:
        for p in v.fetch(*region):
            got.append(p)
    except LraError as e:
        return b"".join(got), str(e)
    return b"".join(got), None


def bad_record_cases():
    good = rec(name=b"good", ops=[op(5, 0)], l_seq=4, qual=b"\1\2\3\4", tags=b"XAi" + struct.pack("<i", 5))
    put = lambda r, at, b: r[:at] + b + r[at + len(b):]
    c = {}
    c["l_read_name 0"] = (put(good, 12, b"\0"), "shorter than its fields")
    c["no NUL"] = (put(good, 36 + 4, b"x"), "shorter than its fields")
    c["fields beyond block_size"] = (put(good, 20, struct.pack("<I", 4000)), "shorter than its fields")
    c["refID outside"] = (put(good, 4, struct.pack("<i", 3)), "outside [-1, 3)")
    c["refID -2"] = (put(good, 4, struct.pack("<i", -2)), "outside [-1, 3)")
    c["op code 9"] = (put(good, 36 + 5, struct.pack("<I", op(5, 9))), "op code above 8")
    tail = lambda t: rec(name=b"good", ops=[op(5, 0)], l_seq=4, qual=b"\1\2\3\4", tags=t)
    c["aux ends inside a tag header"] = (tail(b"XAi" + struct.pack("<i", 5) + b"XB"), "aux block")
    c["aux ends inside a value"] = (tail(b"XAi\1\2"), "aux block")
    c["Z without NUL"] = (tail(b"XAZabc"), "aux block")
    c["B longer than the record"] = (tail(b"XABi" + struct.pack("<I", 3) + b"\0" * 8), "aux block")
    c["unknown type"] = (tail(b"XAQ\0\0\0\0"), "aux block")
    c["unknown B subtype"] = (tail(b"XABZ" + struct.pack("<I", 0)), "aux block")
    c["block_size below 32"] = (struct.pack("<I", 8) + b"\0" * 8, "block_size 8")
    return c


@pytest.mark.parametrize("case", sorted(bad_record_cases()))
def test_bad_record_is_refused(ctx, tmp_path, case):
    from lra_amd.bam import BamView
    bad, text = bad_record_cases()[case]
    front = [rec(name=b"f%d" % i, pos=i, ops=[op(3, 0)], l_seq=3, qual=b"\5\6\7") for i in range(70)]
    path = write(tmp_path, "x.bam", mc.run_bytes(front + [bad] + front[:5]))
    v = BamView(ctx, path)
    try:
        for _ in range(2):                                                        # the view takes another pass, and says the same
            got, err = pieces_then_error(v)
            assert got == b"".join(lines_of(front)), case
            assert err and text in err and "record 70" in err and path in err, err
    finally:
        v.close()


def test_file_faults(ctx, tmp_path, fixture_records):
    from lra_amd.bam import BamView
    from lra_amd._lib import LraError
    recs = fixture_records[:400]
    good = mc.run_bytes(recs, level=0)
    ok = write(tmp_path, "ok.bam", good)
    want = b"".join(lines_of(recs))
    with pytest.raises(LraError, match="not a BAM file"):
        BamView(ctx, write(tmp_path, "no.bam", b"@HD\tVN:1.6\nr1\t4\t*\t0\t0\t*\t*\t0\t0\tA\t!\n"))
    assert view_all(ctx, ok) == want
    # a member with a damaged byte: the records of the members in front come first
    from lra_amd import bgzf
    head = len(bgzf.bgzf_compress(mc.header_bytes(), 6, eof=False))
    sizes, at = [], head
    while at < len(good):
        n = struct.unpack_from("<H", good, at + 16)[0] + 1
        sizes.append((at, n)); at += n
    assert len(sizes) >= 4
    m_at, m_len = sizes[2]
    hurt = bytearray(good); hurt[m_at + m_len // 2] ^= 0x55
    raw, lines = b"".join(recs), lines_of(recs)
    whole, off = 0, 0
    for r in recs:                                                                # the records that end inside the first two members
        off += len(r)
        if off <= 2 * bt.MEMBER:
            whole += 1
    v = BamView(ctx, write(tmp_path, "hurt.bam", bytes(hurt)))
    try:
        got, err = pieces_then_error(v)
        assert got == b"".join(lines[:whole]) and err and "compressed offset %d" % m_at in err and "CRC" in err, err
    finally:
        v.close()
    v = BamView(ctx, write(tmp_path, "cut.bam", good[:sizes[3][0]]))            # the file ends inside a record
    try:
        got, err = pieces_then_error(v)
        assert err and "cut by the end of the file" in err and got and want.startswith(got), err
    finally:
        v.close()
    # the index: of another reference table, damaged, absent
    bam, bai, _ = indexed_file(tmp_path, "s.bam", recs)
    b = open(bai, "rb").read()
    with pytest.raises(LraError, match="references"):
        BamView(ctx, bam, write(tmp_path, "two.bai", b[:4] + struct.pack("<i", 2) + b[8:]))
    with pytest.raises(LraError, match="n_bin"):
        BamView(ctx, bam, write(tmp_path, "neg.bai", b[:8] + struct.pack("<i", -1) + b[12:]))
    with pytest.raises(LraError, match="index"):
        BamView(ctx, bam, write(tmp_path, "short.bai", b[:len(b) // 2]))
    v = BamView(ctx, bam)
    try:
        with pytest.raises(LraError, match="without an index"):
            list(v.fetch(0, 0, 100))
        assert b"".join(v.fetch()) == b"".join(lines_of(sorted(recs, key=bt.sort_key)))
    finally:
        v.close()
    v = BamView(ctx, bam, bai)
    try:
        for bad in ((3, 0, 10), (-1, 0, 10), (0, 10, 9)):
            with pytest.raises(LraError):
                list(v.fetch(*bad))
        assert b"".join(v.fetch(0, 0, 1000)) == brute_lines(b"".join(sorted(recs, key=bt.sort_key)), 0, 0, 1000)
    finally:
        v.close()
