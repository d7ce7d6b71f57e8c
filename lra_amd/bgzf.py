"""BGZF, BAM and SAM writers for tests and tools (the SAM/BAM specification, sections 1 and 4), built on Python's zlib.

bgzf_compress   BGZF members at any level and strategy, cut where the caller says, with or without the 28-byte EOF member
gzip_compress   plain (non-BGZF) gzip of one or more members, with optional FNAME / FEXTRA / FHCRC header fields
bam_bytes       an unaligned BAM (header + records with typed aux fields of every kind), uncompressed; write_bam compresses it
sam_text        the same records as SAM text; write_sam writes it plain or BGZF-compressed

A record is a dict: name (bytes), seq (bytes of "=ACMGRSVTWYHKDBN" letters; b"" for '*'), qual (bytes of Phred+33 characters, or None for '*'), flag (int),
aux (list of (tag, type, value): type in "AcCsSiIfZHB"; B values are (subtype, [values]))."""
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
NT16 = b"=ACMGRSVTWYHKDBN"
_NT16_CODE = {c: i for i, c in enumerate(NT16)}


def member(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    """one BGZF member of data (at most 65536 bytes)"""
    assert len(data) <= 65536
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    cdata = c.compress(data) + c.flush()
    bsize = 12 + 6 + len(cdata) + 8 - 1
    assert bsize < 65536, "a member larger than 64 KiB: cut the data smaller"
    head = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize)
    return head + cdata + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))


def bgzf_compress(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, cuts=None, block=65280, eof=True) -> bytes:
    """data cut into members: at the offsets `cuts` (sorted), else every `block` bytes (65280: htslib's size, whose members never exceed 64 KiB)"""
    if cuts is None:
        cuts = list(range(block, len(data), block))
    bounds = [0] + [c for c in cuts if 0 < c < len(data)] + [len(data)]
    out = [member(data[a:b], level, strategy) for a, b in zip(bounds, bounds[1:]) if b > a or len(data) == 0]
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def gzip_member(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, fname=None, fextra=None, fhcrc=False) -> bytes:
    """one RFC 1952 member of data (any size) without a BGZF 'BC' field; fname (bytes), fextra (bytes, must not hold a BC subfield) and fhcrc set the
    header's FNAME / FEXTRA / FHCRC fields"""
    flg = (4 if fextra is not None else 0) | (8 if fname is not None else 0) | (2 if fhcrc else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0" + b"\0\xff"
    if fextra is not None:
        head += struct.pack("<H", len(fextra)) + fextra
    if fname is not None:
        head += fname + b"\0"
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return head + c.compress(data) + c.flush() + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data) & 0xffffffff)


def gzip_compress(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, cuts=(), **fields) -> bytes:
    """data as concatenated gzip members cut at the offsets `cuts` (none: one member); fields: gzip_member's fname / fextra / fhcrc, on every member"""
    bounds = [0] + [c for c in cuts if 0 < c < len(data)] + [len(data)]
    return b"".join(gzip_member(data[a:b], level, strategy, **fields) for a, b in zip(bounds, bounds[1:]))


def blocks(data: bytes):
    """the members of a BGZF file -> (in_off[n + 1], out_off[n + 1]) as lists: where each member lies and where its data goes"""
    in_off, out_off = [0], [0]
    p = 0
    while p < len(data):
        xlen = struct.unpack_from("<H", data, p + 10)[0]
        x, bsize = 0, None
        while x + 4 <= xlen:
            si, slen = data[p + 12 + x:p + 14 + x], struct.unpack_from("<H", data, p + 14 + x)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", data, p + 16 + x)[0]
            x += 4 + slen
        p += bsize + 1
        in_off.append(p)
        out_off.append(out_off[-1] + struct.unpack_from("<I", data, p - 4)[0])
    return in_off, out_off


def _aux_bin(aux):
    out = b""
    for tag, t, v in aux:
        out += tag.encode() if isinstance(tag, str) else tag
        if t == "A":
            out += b"A" + (v.encode() if isinstance(v, str) else v)
        elif t in "cCsSiI":
            out += t.encode() + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[t], v)
        elif t == "f":
            out += b"f" + struct.pack("<f", v)
        elif t in "ZH":
            out += t.encode() + (v.encode() if isinstance(v, str) else v) + b"\0"
        elif t == "B":
            st, vals = v
            fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[st]
            out += b"B" + st.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack("<" + fmt, x) for x in vals)
        else:
            raise ValueError(t)
    return out


def bam_record(r) -> bytes:
    name = r["name"] + b"\0"
    seq = r.get("seq", b"")
    qual = r.get("qual")
    n = len(seq)
    codes = [_NT16_CODE[c] for c in seq.upper()]
    packed = bytes(((codes[i] << 4) | (codes[i + 1] if i + 1 < n else 0)) for i in range(0, n, 2))
    q = b"\xff" * n if qual is None else bytes(c - 33 for c in qual)
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 255, 4680, 0, r.get("flag", 4), n, -1, -1, 0) + name + packed + q + _aux_bin(r.get("aux", []))
    return struct.pack("<I", len(body)) + body


def bam_bytes(records, header_text=b"@HD\tVN:1.6\tSO:unknown\n", refs=()) -> bytes:
    head = b"BAM\1" + struct.pack("<i", len(header_text)) + header_text + struct.pack("<i", len(refs))
    for nm, ln in refs:
        head += struct.pack("<i", len(nm) + 1) + nm + b"\0" + struct.pack("<i", ln)
    return head + b"".join(bam_record(r) for r in records)


def write_bam(path, records, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, cuts=None, block=65280, eof=True, **kw):
    raw = bam_bytes(records, **kw)
    with open(path, "wb") as f:
        f.write(bgzf_compress(raw, level, strategy, cuts, block, eof))
    return raw


def _aux_text(aux):
    out = []
    for tag, t, v in aux:
        tag = tag.decode() if isinstance(tag, bytes) else tag
        if t in "cCsSiI":
            out.append("%s:i:%d" % (tag, v))
        elif t == "f":
            out.append("%s:f:%g" % (tag, v))
        elif t == "B":
            st, vals = v
            out.append("%s:B:%s" % (tag, st) + "".join(("," + ("%g" % x if st == "f" else "%d" % x)) for x in vals))
        else:
            out.append("%s:%s:%s" % (tag, t, v.decode() if isinstance(v, bytes) else v))
    return out


def sam_line(r) -> bytes:
    f = [r["name"].decode(), str(r.get("flag", 4)), "*", "0", "0", "*", "*", "0", "0", (r.get("seq") or b"*").decode(),
         "*" if r.get("qual") is None else r["qual"].decode()] + r.get("aux_text", _aux_text(r.get("aux", [])))
    return "\t".join(f).encode() + b"\n"


def sam_text(records, header=b"@HD\tVN:1.6\tSO:unknown\n@PG\tID:x\tPN:x\n") -> bytes:
    return header + b"".join(sam_line(r) for r in records)


def write_sam(path, records, bgzf=False, level=6, cuts=None, eof=True, header=b"@HD\tVN:1.6\tSO:unknown\n@PG\tID:x\tPN:x\n", text=None):
    raw = sam_text(records, header) if text is None else text
    with open(path, "wb") as f:
        f.write(bgzf_compress(raw, level, cuts=cuts, eof=eof) if bgzf else raw)
    return raw
