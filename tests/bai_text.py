"""The .bai index (SAM specification 5.2) in Python, independent of the library: a builder from a sorted raw BAM record stream, by the rules
include/lra_hip.h states, and a reader that answers region queries by the specification's reg2bins, the linear index and zlib.

The rules.  Only records with refID >= 0 are indexed, under the bin of their own core field.  A run is a maximal sequence of consecutive records in
file order with the same (refID, bin); each run is one chunk [voff(start of its first), voff(end of its last)); a bin's chunks are in file order; no further
merging.  Bins ascend by number; a reference with records also gets the pseudo-bin 37450, last and counted in n_bin, with the chunks (voff of its
first record, voff end of its last) and (n_mapped, n_unmapped by flag & 4).  Window w (16384 bases) of the linear index holds the smallest start offset of
a record with pos >> 14 <= w <= (end - 1) >> 14, end = pos + max(1, the reference bases its CIGAR consumes); n_intv = the last touched window + 1; an
untouched window takes the value of the next touched one behind it.  A reference without records has n_bin = n_intv = 0.  The trailing n_no_coor counts
the records with refID = -1.  Byte u of the stream has the virtual offset ((first + member_off[u // 65280]) << 16) | (u % 65280)."""
import struct
import zlib

MEMBER = 65280
PSEUDO = 37450
CONSUMES_REF = {0, 2, 3, 7, 8}                                                    # M D N = X


def core(raw, at):
    """the fields of the record at raw[at:] the index needs -> dict"""
    bs, ref, pos, l_name, _mapq, bin_, n_cig, flag = struct.unpack_from("<IiiBBHHH", raw, at)
    ops = struct.unpack_from("<%dI" % n_cig, raw, at + 36 + l_name)
    span = sum(o >> 4 for o in ops if (o & 15) in CONSUMES_REF)
    return dict(at=at, next=at + 4 + bs, ref=ref, pos=pos, end=pos + max(span, 1), bin=bin_, flag=flag)


def walk(raw):
    out, at = [], 0
    while at < len(raw):
        out.append(core(raw, at))
        at = out[-1]["next"]
    assert at == len(raw)
    return out


def member_table(n_bytes, member_len):
    """member_off[n_members + 1] from the members' compressed lengths"""
    off = [0]
    for n in member_len:
        off.append(off[-1] + n)
    assert len(off) - 1 == (n_bytes + MEMBER - 1) // MEMBER
    return off


def voff(u, member_off, first):
    return ((first + member_off[u // MEMBER]) << 16) | (u % MEMBER)


def build(raw, n_ref, member_off, first=0):
    """the .bai bytes of the sorted raw stream"""
    recs = walk(raw)
    refs = [dict(bins={}, lin={}, first=None, last=None, mapped=0, unmapped=0) for _ in range(n_ref)]
    n_no_coor = 0
    prev = None
    for r in recs:
        if r["ref"] < 0:
            n_no_coor += 1
            prev = None
            continue
        R = refs[r["ref"]]
        vb, ve = voff(r["at"], member_off, first), voff(r["next"], member_off, first)
        chunks = R["bins"].setdefault(r["bin"], [])
        if prev == (r["ref"], r["bin"]):
            chunks[-1][1] = ve
        else:
            chunks.append([vb, ve])
        prev = (r["ref"], r["bin"])
        if R["first"] is None:
            R["first"] = vb
        R["last"] = ve
        R["unmapped" if r["flag"] & 4 else "mapped"] += 1
        for w in range(r["pos"] >> 14, ((r["end"] - 1) >> 14) + 1):
            R["lin"][w] = min(R["lin"].get(w, vb), vb)
    o = [b"BAI\x01", struct.pack("<i", n_ref)]
    for R in refs:
        o.append(struct.pack("<i", len(R["bins"]) + (1 if R["bins"] else 0)))
        for b in sorted(R["bins"]):
            o.append(struct.pack("<Ii", b, len(R["bins"][b])))
            for c in R["bins"][b]:
                o.append(struct.pack("<QQ", *c))
        if R["bins"]:
            o.append(struct.pack("<IiQQQQ", PSEUDO, 2, R["first"], R["last"], R["mapped"], R["unmapped"]))
        n_intv = max(R["lin"]) + 1 if R["lin"] else 0
        o.append(struct.pack("<i", n_intv))
        vals, nxt = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):
            nxt = R["lin"].get(w, nxt)
            vals[w] = nxt
        o.append(struct.pack("<%dQ" % n_intv, *vals))
    o.append(struct.pack("<Q", n_no_coor))
    return b"".join(o)


def parse(bai):
    """-> ([{"bins": {bin: [(beg, end)]}, "lin": [..], "meta": (first, last, mapped, unmapped) or None}], n_no_coor)"""
    assert bai[:4] == b"BAI\x01"
    (n_ref,) = struct.unpack_from("<i", bai, 4)
    at = 8
    refs = []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", bai, at); at += 4
        bins, meta, last_bin = {}, None, -1
        for k in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at); at += 8
            ch = [struct.unpack_from("<QQ", bai, at + 16 * i) for i in range(n_chunk)]
            at += 16 * n_chunk
            if b == PSEUDO:
                assert k == n_bin - 1 and n_chunk == 2, "the pseudo-bin comes last, with two chunks"
                meta = ch[0] + ch[1]
            else:
                assert b > last_bin and b < PSEUDO, "bins ascend"
                last_bin = b
                bins[b] = ch
        (n_intv,) = struct.unpack_from("<i", bai, at); at += 4
        lin = list(struct.unpack_from("<%dQ" % n_intv, bai, at)); at += 8 * n_intv
        refs.append(dict(bins=bins, lin=lin, meta=meta))
    (n_no_coor,) = struct.unpack_from("<Q", bai, at)
    assert at + 8 == len(bai)
    return refs, n_no_coor


def reg2bins(beg, end):
    """the bins that may hold a record overlapping [beg, end) (SAM specification 5.3)"""
    end -= 1
    out = [0]
    for sh, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(base + (beg >> sh), base + (end >> sh) + 1))
    return out


class Reader:
    """Region queries on a BGZF file of BAM records (bytes) through its .bai: members are inflated with zlib from the compressed offset a virtual offset
    names, records read from the offset inside."""

    def __init__(self, file_bytes, bai):
        self.f = file_bytes
        self.refs, self.n_no_coor = parse(bai)
        self.cache = {}

    def member(self, coff):
        if coff not in self.cache:
            d = zlib.decompressobj(31)
            data = d.decompress(self.f[coff:])
            assert d.eof
            self.cache[coff] = (data, coff + len(self.f) - coff - len(d.unused_data))
        return self.cache[coff]

    def read(self, v, n):
        """n bytes from virtual offset v -> (bytes, the virtual offset behind them)"""
        coff, u = v >> 16, v & 0xffff
        out = b""
        while n:
            data, nxt = self.member(coff)
            if u >= len(data):
                coff, u = nxt, 0
                continue
            take = data[u:u + n]
            out += take; n -= len(take); u += len(take)
        data, nxt = self.member(coff)
        if u >= len(data):
            coff, u = nxt, 0
        return out, (coff << 16) | u

    def query(self, ref, beg, end):
        """the records (their bytes, block_size included) that overlap [beg, end) of reference ref, in file order, found through the index alone: the
        chunks of reg2bins' bins, each read from the larger of its start and the linear index's offset of beg's window, filtered by overlap"""
        R = self.refs[ref]
        w = beg >> 14
        if w >= len(R["lin"]):                                                    # behind the last touched window: no record reaches beg or starts behind it
            return []
        min_off = R["lin"][w]
        found = {}
        for b in reg2bins(beg, end):
            for cb, ce in R["bins"].get(b, ()):
                v = max(cb, min_off)
                while v < ce:
                    head, _ = self.read(v, 4)
                    (bs,) = struct.unpack("<I", head)
                    rec, nv = self.read(v, 4 + bs)
                    c = core(rec, 0)
                    if c["ref"] == ref and c["pos"] < end and c["end"] > beg:
                        found[v] = rec
                    v = nv
        return [found[v] for v in sorted(found)]


def brute(raw, ref, beg, end):
    return [raw[r["at"]:r["next"]] for r in walk(raw) if r["ref"] == ref and r["pos"] < end and r["end"] > beg]


# ---- crafted records ----------------------------------------------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    end -= 1
    for sh, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == end >> sh:
            return base + (beg >> sh)
    return 0


def make_record(ref, pos, flag, name, ops, l_seq=0, tags=b"", mapq=60):
    """one BAM alignment record (block_size included); ops: the CIGAR as uint32 values (at most 65535: n_cigar_op has 16 bits); the bin is reg2bin of
    the span the ops (or, in the CG:B:I form, the N op) give; SEQ / QUAL are filler bytes"""
    span = sum(o >> 4 for o in ops if (o & 15) in CONSUMES_REF)
    bin_ = 4680 if ref < 0 else reg2bin(pos, pos + max(span, 1))
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, mapq, bin_, len(ops), flag, l_seq, -1, -1, 0) + name + b"\0"
    body += struct.pack("<%dI" % len(ops), *ops) + bytes((7 * k + len(name)) & 255 for k in range((l_seq + 1) // 2)) + b"\xff" * l_seq + tags
    return struct.pack("<I", len(body)) + body


def cg_record(ref, pos, flag, name, ops, l_seq):
    """the CG:B:I form of a record whose ops do not fit n_cigar_op: CIGAR <l_seq>S<span>N, the ops in the tag"""
    span = sum(o >> 4 for o in ops if (o & 15) in CONSUMES_REF)
    tag = b"CGBI" + struct.pack("<I%dI" % len(ops), len(ops), *ops)
    return make_record(ref, pos, flag, name, [(l_seq << 4) | 4, (span << 4) | 3], l_seq, tag)


def random_records(rng, n, ref_len, max_ops=300, max_span=60000, p_unmapped=0.1):
    """n records on the references ref_len (and refID -1) with many ties: positions come from a small set"""
    out = []
    spots = [int(rng.integers(0, 1 << 30)) for _ in range(max(2, n // 4))]
    for i in range(n):
        name = bytes(rng.integers(65, 91, int(rng.integers(1, 255)), dtype="uint8"))
        if rng.random() < p_unmapped or not ref_len:
            out.append(make_record(-1, -1, 4, name, [], int(rng.integers(0, 200))))
            continue
        ref = int(rng.integers(0, len(ref_len)))
        n_ops = int(rng.integers(0, max_ops + 1))
        per = max(1, max_span // max(n_ops, 1))
        ops = [(int(rng.integers(1, per + 1)) << 4) | int(rng.choice([0, 1, 2, 3, 4, 7, 8])) for _ in range(n_ops)]
        span = max(1, sum(o >> 4 for o in ops if (o & 15) in CONSUMES_REF))
        pos = spots[int(rng.integers(0, len(spots)))] % max(1, ref_len[ref] - span)
        flag = int(rng.choice([0, 16, 256, 272, 2048, 2064])) | (4 if rng.random() < 0.05 else 0)
        out.append(make_record(ref, pos, flag, name, ops, int(rng.integers(0, 400))))
    return out


def sort_key(rec):
    ref, pos = struct.unpack_from("<ii", rec, 4)
    (flag,) = struct.unpack_from("<H", rec, 18)
    return (ref & 0xffffffff, pos, flag & 16)


def gzip_members(raw):
    """raw cut every 65280 bytes, each part one gzip member -> (the members back to back, member_off[n + 1])"""
    parts, off = [], [0]
    for a in range(0, len(raw), MEMBER):
        c = zlib.compressobj(1, zlib.DEFLATED, 31)
        parts.append(c.compress(raw[a:a + MEMBER]) + c.flush())
        off.append(off[-1] + len(parts[-1]))
    return b"".join(parts), off


def check_queries(rng, file_bytes, bai, raw, ref_len, n=200):
    """n random regions: what the index reaches, filtered by overlap, is the brute-force overlap set"""
    rd = Reader(file_bytes, bai)
    recs = walk(raw)
    hit = 0
    for k in range(n):
        ref = int(rng.integers(0, len(ref_len)))
        if k % 2 and recs:                                                       # half of the regions lie around a record
            r = recs[int(rng.integers(0, len(recs)))]
            if r["ref"] >= 0:
                ref = r["ref"]
                beg = max(0, r["pos"] - int(rng.integers(0, 20000)))
            else:
                beg = int(rng.integers(0, ref_len[ref]))
        else:
            beg = int(rng.integers(0, ref_len[ref]))
        end = min(ref_len[ref], beg + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 22)))))
        want = [raw[r["at"]:r["next"]] for r in recs if r["ref"] == ref and r["pos"] < end and r["end"] > beg]
        got = rd.query(ref, beg, end)
        assert got == want, (ref, beg, end, len(got), len(want))
        hit += bool(want)
    return hit
