"""A small BAM-to-SAM decoder (SAM/BAM specification 4.2), independent of the project's readers and writers: members are inflated with Python's zlib, records
are taken apart with struct / numpy, and every record prints as one SAM line.  Integers of any type print as decimal, 'f' as "%.6g" of the float32 (what
ostream << float prints), 'B' arrays and 'Z' as text; a kSmN CIGAR with a CG:B:I tag is restored and the tag dropped, as htslib does on reading; a QUAL of
0xff bytes prints as '*'."""
import struct
import zlib

import numpy as np

NT16 = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
_NP = {"c": np.int8, "C": np.uint8, "s": "<i2", "S": "<u2", "i": "<i4", "I": "<u4", "f": "<f4"}


def inflate(data):
    """BGZF / gzip members back to back -> their data, through zlib alone; every member's CRC and length are zlib's to check"""
    out = []
    while data:
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        assert d.eof, "a member that does not end"
        data = d.unused_data
    return b"".join(out)


def parse_header(raw):
    """-> (header text, [(name, length)], the offset of the first record)"""
    assert raw[:4] == b"BAM\x01", raw[:4]
    (l_text,) = struct.unpack_from("<I", raw, 4)
    text = raw[8:8 + l_text]
    at = 8 + l_text
    (n_ref,) = struct.unpack_from("<I", raw, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<I", raw, at)
        name = raw[at + 4:at + 4 + l_name]
        assert name.endswith(b"\0") and b"\0" not in name[:-1]
        (l_ref,) = struct.unpack_from("<I", raw, at + 4 + l_name)
        refs.append((name[:-1], l_ref))
        at += 8 + l_name
    return text, refs, at


def _tags(b):
    out = []
    at = 0
    while at < len(b):
        tag, t = b[at:at + 2].decode(), chr(b[at + 2])
        at += 3
        if t == "A":
            out.append((tag, "A", chr(b[at]))); at += 1
        elif t in _INT:
            n = struct.calcsize(_INT[t])
            out.append((tag, "i", str(struct.unpack_from(_INT[t], b, at)[0]))); at += n
        elif t == "f":
            out.append((tag, "f", "%.6g" % np.frombuffer(b, "<f4", 1, at)[0])); at += 4
        elif t in "ZH":
            e = b.index(b"\0", at)
            out.append((tag, t, b[at:e].decode())); at = e + 1
        elif t == "B":
            st = chr(b[at])
            (n,) = struct.unpack_from("<I", b, at + 1)
            a = np.frombuffer(b, _NP[st], n, at + 5)
            out.append((tag, "B", st + "".join(("," + ("%.6g" % v if st == "f" else str(int(v)))) for v in a), a))
            at += 5 + n * a.itemsize
        else:
            raise AssertionError("aux type %r" % t)
    assert at == len(b)
    return out


def _cigar(ops):
    return "".join("%d%s" % (int(o) >> 4, CIGAR_OPS[int(o) & 15]) for o in ops)


def record_line(rec, refs):
    """one record's bytes behind its block_size -> its SAM line (bytes, without the newline)"""
    ref_id, pos, l_name, mapq, _bin, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHIiii", rec, 0)
    at = 32
    name = rec[at:at + l_name]
    assert name.endswith(b"\0") and b"\0" not in name[:-1], name
    at += l_name
    ops = np.frombuffer(rec, "<u4", n_cig, at)
    at += 4 * n_cig
    packed = np.frombuffer(rec, np.uint8, (l_seq + 1) // 2, at)
    at += (l_seq + 1) // 2
    qual = rec[at:at + l_seq]
    assert len(qual) == l_seq
    at += l_seq
    tags = _tags(rec[at:])
    nib = np.stack([packed >> 4, packed & 15], 1).reshape(-1)
    assert l_seq % 2 == 0 or nib[-1] == 0, "the odd tail's low nibble"
    seq = "".join(NT16[v] for v in nib[:l_seq]) if l_seq else "*"
    if n_cig == 2 and int(ops[0]) == (l_seq << 4 | 4) and (int(ops[1]) & 15) == 3:      # the real CIGAR is in CG:B:I
        cg = [t for t in tags if t[0] == "CG" and t[1] == "B" and t[2].startswith("I")]
        if cg:
            assert tags[-1] is cg[0], "CG:B:I is the last tag"
            ops = cg[0][3]
            tags = [t for t in tags if t is not cg[0]]
    q = "*" if not l_seq or qual == b"\xff" * l_seq else bytes(v + 33 for v in qual).decode("latin-1")
    rname = lambda i: "*" if i < 0 else refs[i][0].decode()
    f = [name[:-1].decode(), str(flag), rname(ref_id), str(pos + 1), str(mapq), _cigar(ops) if len(ops) else "*",
         "*" if nref < 0 else ("=" if nref == ref_id else rname(nref)), str(npos + 1), str(tlen), seq, q]
    f += ["%s:%s:%s" % t[:3] for t in tags]
    return "\t".join(f).encode("latin-1")


def records(raw, refs, at=0):
    """the record stream raw[at:] -> [(offset of the record's block_size, block_size, SAM line)]"""
    out = []
    while at < len(raw):
        (bs,) = struct.unpack_from("<I", raw, at)
        assert bs >= 32 and at + 4 + bs <= len(raw), (at, bs, len(raw))
        out.append((at, bs, record_line(raw[at + 4:at + 4 + bs], refs)))
        at += 4 + bs
    return out


def reg2bin(beg, end):
    end -= 1
    for sh, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == end >> sh:
            return base + (beg >> sh)
    return 0
