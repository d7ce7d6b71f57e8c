"""SAM and BAM read files (lra_amd/csrc/input.hip, input_bam.hip, input_device.hip): BGZF inflate against zlib, corrupt streams, both reader forms against
a plain-Python restatement of GetNext's HTS branch (Input.h:296-393) with the port's decisions (an error where the reference stops without a word),
flagRemove, passthrough tags, SAM against BAM, file sequences, and mapping BAM input against the same reads as FASTQ."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from lra_amd import bgzf, synth
from test_input import IStream, _token, _write_files, ref_batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IUPAC = b"=ACMGRSVTWYHKDBN"


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _members(data):
    """BGZF members with Python's zlib -> (decompressed bytes up to the first bad member, ok)"""
    out, p = [], 0
    while p < len(data):
        if len(data) - p < 18 or data[p:p + 4] != b"\x1f\x8b\x08\x04":
            return b"".join(out), False
        xlen = struct.unpack_from("<H", data, p + 10)[0]
        bsize = None
        x = 0
        while x + 4 <= xlen:
            slen = struct.unpack_from("<H", data, p + 14 + x)[0]
            if data[p + 12 + x:p + 14 + x] == b"BC":
                bsize = struct.unpack_from("<H", data, p + 16 + x)[0]
            x += 4 + slen
        if bsize is None or p + bsize + 1 > len(data):
            return b"".join(out), False
        m = data[p:p + bsize + 1]
        crc, isize = struct.unpack_from("<II", m, len(m) - 8)
        try:
            d = zlib.decompress(m[12 + xlen:-8], -15)
        except zlib.error:
            return b"".join(out), False
        if len(d) != isize or zlib.crc32(d) & 0xffffffff != crc:
            return b"".join(out), False
        out.append(d)
        p += bsize + 1
    return b"".join(out), True


def _fmt_aux(a):
    out, p = [], 0
    size = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    code = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}
    def val(t, at):
        v = struct.unpack_from("<" + code[t], a, at)[0]
        return ("%g" % v) if t == "f" else "%d" % v
    while p + 3 <= len(a):
        tag, t = a[p:p + 2].decode(), chr(a[p + 2])
        p += 3
        if t == "A":
            out.append("%s:A:%s" % (tag, chr(a[p]))); p += 1
        elif t in "cCsSiI":
            out.append("%s:i:%s" % (tag, val(t, p))); p += size[t]
        elif t == "f":
            out.append("%s:f:%s" % (tag, val(t, p))); p += 4
        elif t in "ZH":
            e = a.index(b"\0", p)
            out.append("%s:%s:%s" % (tag, t, a[p:e].decode())); p = e + 1
        elif t == "B":
            st, n = chr(a[p]), struct.unpack_from("<I", a, p + 1)[0]
            p += 5
            out.append("%s:B:%s" % (tag, st) + "".join("," + val(st, p + i * size[st]) for i in range(n))); p += n * size[st]
    return "\t".join(out).encode() if out else None


def _bam_recs(raw):
    """records of a decompressed BAM -> list of (flag, name, seq, qual, tags), ok"""
    recs = []
    lt = struct.unpack_from("<i", raw, 4)[0]
    p = 8 + lt
    nref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    for _ in range(nref):
        p += 8 + struct.unpack_from("<i", raw, p)[0]
    while p < len(raw):
        if p + 4 > len(raw):
            return recs, False
        bs = struct.unpack_from("<I", raw, p)[0]
        if bs < 32 or p + 4 + bs > len(raw):
            return recs, False
        r = raw[p + 4:p + 4 + bs]
        ln, nc, flag, ls = r[8], struct.unpack_from("<H", r, 12)[0], struct.unpack_from("<H", r, 14)[0], struct.unpack_from("<i", r, 16)[0]
        if ln < 1 or 32 + ln + 4 * nc + (ls + 1) // 2 + ls > bs or r[32 + ln - 1] != 0:
            return recs, False
        name = r[32:32 + ln - 1]
        sq = r[32 + ln + 4 * nc:]
        seq = bytes(IUPAC[(sq[i >> 1] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(ls))
        q = sq[(ls + 1) // 2:]
        qual = None if ls == 0 or q[0] == 0xff else bytes((x + 33) & 0xff for x in q[:ls])
        recs.append((flag, name, seq, qual, _fmt_aux(q[ls:bs - 32 - ln - 4 * nc - (ls + 1) // 2])))
        p += 4 + bs
    return recs, True


def _nt16(c):
    c = chr(c).upper()
    c = "T" if c == "U" else c
    return ord(c) if c.encode() in IUPAC else ord("N")


def _sam_aux(f):
    tag, t, v = f[:2], f[3], f[5:]
    if t == "i":
        return "%s:i:%d" % (tag, int(v))
    if t == "f":
        return "%s:f:%g" % (tag, float(v))
    if t == "B" and v[0] == "f":
        return "%s:B:f" % tag + "".join(",%g" % float(x) for x in v.split(",")[1:])
    if t == "B":
        return "%s:B:%s" % (tag, v[0]) + "".join(",%d" % int(x) for x in v.split(",")[1:])
    return f


def _sam_recs(text):
    recs = []
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    i = 0
    while i < len(lines) and lines[i].startswith(b"@"):
        i += 1
    for l in lines[i:]:
        f = l.split(b"\t")
        seq = b"" if f[9] == b"*" else bytes(_nt16(c) for c in f[9])
        if f[10] != b"*" and len(f[10]) != len(seq):
            return recs, False
        qual = None if f[10] == b"*" or not seq else f[10]
        aux = [_sam_aux(x.decode()) for x in f[11:]]
        recs.append((int(f[1]), f[0], seq, qual, "\t".join(aux).encode() if aux else None))
    return recs, True


def hts_records(path):
    data = open(path, "rb").read()
    if data[:2] == b"\x1f\x8b":
        raw, ok = _members(data)
        recs, ok2 = _bam_recs(raw) if raw[:4] == b"BAM\1" else _sam_recs(raw)
        return recs, ok and ok2
    return _sam_recs(data)


def _is_hts(path):
    d = open(path, "rb").read(4)
    return d[:2] == b"\x1f\x8b" or (d[:1] != b">" and d[:1] != b"@") or d[:3] == b"@HD"


def ref_hts_batches(files, max_bases, flag_remove=0, passthrough=False):
    """Input::Initialize + GetNext + BufferedRead over FASTA / FASTQ / SAM / BAM files with the port's decisions -> (batches of (name, seq, qual[, tags]),
    error or not).  FASTA / FASTQ only: test_input.ref_batches."""
    if not any(_is_hts(f) for f in files):
        return ref_batches(files, max_bases), None
    st = dict(cur=0, ok=True, err=False, unread=False)

    def init():
        d = open(files[st["cur"]], "rb").read()
        s = IStream(d)
        if s.peek() == ord(">"):
            st.update(s=s, type=0); return
        if s.peek() == ord("@"):
            t = IStream(d); t.getline(); t.getline()
            if t.peek() == ord("+"):
                st.update(s=s, type=1); return
        recs, ok = hts_records(files[st["cur"]])
        st.update(type=2, recs=iter(recs), rec_ok=ok)
    init()

    def rec(name, seq, qual, tags=None):
        return (name, seq, qual, tags) if passthrough else (name, seq, qual)

    def get_next():
        if not st["ok"]:
            return None
        if st["type"] == 0 and st["s"].eof:
            st["cur"] += 1
            if st["cur"] >= len(files):
                st["ok"] = False; return None
            init()
        if st["type"] == 2:
            for flag, name, seq, qual, tags in st["recs"]:
                st["unread"] = False
                if flag & flag_remove:
                    continue
                return rec(name, seq, qual, tags)
            st["ok"] = False
            st["err"] = not st["rec_ok"] or st["cur"] + 1 < len(files)
            return None
        s = st["s"]
        if s.eof:
            return None
        if st["type"] == 0:
            name = _token(s.getline())
            seq = b""
            c = s.peek()
            while c != -1 and c != ord(">"):
                seq += s.getline().replace(b" ", b"").upper()
                c = s.peek()
            if c == -1:
                s.get()
            return rec(name, seq, None)
        h, q, sep, ql = s.getline(), s.getline(), s.getline(), s.getline()
        if not (h and q and sep and ql):
            st["cur"] += 1
            if st["cur"] >= len(files):
                st["ok"] = False; return None
            init()
            if st["type"] == 2:
                st["unread"] = True; return None
            s = st["s"]
            if st["type"] == 1:
                h, q, sep, ql = s.getline(), s.getline(), s.getline(), s.getline()
        if not (h and q and sep and ql):
            return None
        return rec(_token(h), q.replace(b" ", b"").upper(), ql.replace(b" ", b""))
    out = []
    while True:
        batch, total = [], 0
        while total < max_bases:
            r = get_next()
            if r is None:
                break
            batch.append(r); total += len(r[1])
        if not batch and st["unread"] and not st["err"]:
            st["err"] = True; st["ok"] = False
        if batch:
            out.append(batch)
        if not batch or st["err"]:
            return out, st["err"]


# ---------------------------------------------------------------------------------------------------------------- corpora
def _rand_recs(rng, n, max_len=600, aux=True, prefix="b"):
    recs = []
    for i in range(n):
        L = 0 if i % 17 == 5 else int(rng.integers(1, max_len))
        seq = bytes(np.frombuffer(b"ACGTACGTACGTN=MRWSYKVHDB", np.uint8)[rng.integers(0, 24, L)])
        qual = None if (i % 7 == 3 or L == 0) else bytes(rng.integers(33, 75, L).astype(np.uint8))
        nl = 254 if i == 2 else 1 if i == 3 else int(rng.integers(2, 40))
        name = ("%s%d_" % (prefix, i)).encode()
        name = (name + b"x" * nl)[:nl]
        a = []
        if aux and i % 3:
            a = [("RG", "Z", "grp%d" % (i % 4)), ("np", "C", i % 200), ("sN", "s", -300 - i), ("iI", "I", 70000 + i), ("XA", "A", "z"),
                 ("rq", "f", 0.5 + i / 8), ("zz", "B", ("C", [1, 2, i % 250]))]
            if i % 5 == 0:
                a += [("Bc", "B", ("c", [-1, 5])), ("Bs", "B", ("s", [-300])), ("BS", "B", ("S", [40000, 1])), ("Bi", "B", ("i", [-70000])),
                      ("BI", "B", ("I", [3000000000])), ("Bf", "B", ("f", [0.125, -2.5, 1e-3])), ("HH", "H", "1AE3"), ("cc", "c", -7),
                      ("SS", "S", 60000), ("ii", "i", -100000)]
        recs.append(dict(name=name, seq=seq, qual=qual, flag=int([4, 4, 4, 0x104, 0x804, 0x204, 4][i % 7]), aux=a))
    return recs


def _cuts(rng, n):
    cuts, p = [], 0
    while True:
        p += int(rng.integers(40, 6000))
        if p >= n:
            return cuts
        cuts.append(p)


def _corpus(tmp_path, seed=1, n=60):
    """a BAM with random block cuts and its EOF block, the same without the EOF block, the same records as SAM and BGZF SAM"""
    rng = np.random.default_rng(seed)
    recs = _rand_recs(rng, n)
    raw = bgzf.bam_bytes(recs)
    paths = {}
    for key, eof in (("bam", True), ("bam_noeof", False)):
        p = tmp_path / ("%s_%d.bam" % (key, seed))
        p.write_bytes(bgzf.bgzf_compress(raw, 6, cuts=_cuts(rng, len(raw)), eof=eof))
        paths[key] = str(p)
    paths["sam"] = str(tmp_path / ("s_%d.sam" % seed)); bgzf.write_sam(paths["sam"], recs)
    paths["samgz"] = str(tmp_path / ("s_%d.sam.gz" % seed)); bgzf.write_sam(paths["samgz"], recs, bgzf=True, cuts=_cuts(rng, 10 ** 6))
    return recs, paths


def _read_all(files, max_bases, ctx=None, chunk=None, flag_remove=0, passthrough=False):
    from lra_amd import reads_io
    rf = reads_io.ReadsFile(files, ctx=ctx, chunk=chunk, flag_remove=flag_remove, passthrough=passthrough)
    got, failed = [], None

    def rows(b):
        if passthrough:
            return list(zip(b["names"], b["seqs"], b["quals"], b["tags"]))
        assert all(t is None for t in b["tags"])
        return list(zip(b["names"], b["seqs"], b["quals"]))
    try:
        while True:
            try:
                b = rf.next_batch(max_bases)
            except IOError as e:
                failed = str(e).split(": ", 1)[1]
                if e.partial is not None:
                    got.append(rows(e.partial))
                    if ctx is not None:
                        _check_device_arrays(ctx, e.partial)
                with pytest.raises(IOError):
                    rf.next_batch(max_bases)
                break
            if b is None:
                break
            if ctx is not None:
                _check_device_arrays(ctx, b)
            got.append(rows(b))
    finally:
        rf.close()
    return got, failed


def _check_device_arrays(ctx, b):
    n, tot = b["n"], b["total_bases"]
    seq = ctx.to_host(b["d_seq"], tot + 64, np.uint8).tobytes()
    assert seq == b"".join(b["seqs"]) + bytes(64)
    assert np.array_equal(ctx.to_host(b["d_off"], n + 1, np.uint64), b["off"]) and b["off"][0] == 0


def _check_host(files, max_bases, **kw):
    exp, exp_err = ref_hts_batches(files, max_bases, kw.get("flag_remove", 0), kw.get("passthrough", False))
    got, err = _read_all(files, max_bases, **kw)
    assert len(got) == len(exp), (len(got), len(exp), err)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (i, [x[0] for x in g][:4], [x[0] for x in e][:4])
    assert (err is not None) == bool(exp_err), (err, exp_err)
    return got, err


# ---------------------------------------------------------------------------------------------------------------- inflate
def _inflate(lib, data, ctx=None):
    io_, oo = bgzf.blocks(data)
    n = len(io_) - 1
    out = np.zeros(oo[-1] + 1, np.uint8)
    st = np.full(n, -1, np.int32)
    a_io, a_oo, buf = np.array(io_, np.uint64), np.array(oo, np.uint64), np.frombuffer(data, np.uint8).copy()
    if ctx is None:
        assert lib.lra_bgzf_inflate_host(n, buf.ctypes.data, a_io.ctypes.data, a_oo.ctypes.data, out.ctypes.data, st.ctypes.data) == 0
    else:
        import torch
        dev = lambda a: torch.from_numpy(a.view(np.uint8)).cuda()
        t_buf, t_io, t_oo, t_out, t_st = dev(buf), dev(a_io), dev(a_oo), dev(out), dev(st)
        assert lib.lra_bgzf_inflate_batch(ctx.h, n, t_buf.data_ptr(), t_io.data_ptr(), t_oo.data_ptr(), t_out.data_ptr(), t_st.data_ptr()) == 0
        out, st = t_out.cpu().numpy(), t_st.cpu().numpy().view(np.int32)
    return out[:oo[-1]].tobytes(), st


def _inflate_corpora():
    rng = np.random.default_rng(3)
    rnd = bytes(rng.integers(0, 256, 150_000).astype(np.uint8))
    dna = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 300_000)])
    runs = b"A" * 70_000 + b"AC" * 40_000 + b"\0" * 65_536
    out = []
    for level in (0, 1, 6, 9):
        out.append(("rnd%d" % level, rnd, level, zlib.Z_DEFAULT_STRATEGY, [0, 0, 1] + list(range(60_000, 150_000, 60_000))))
        out.append(("dna%d" % level, dna, level, zlib.Z_DEFAULT_STRATEGY, list(range(65_536, 300_000, 65_536)) if level else list(range(60_000, 300_000, 60_000))))
    for strat in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
        out.append(("runs%d" % strat, runs, 6, strat, [65_536, 65_537, 70_000, 135_536, 150_000]))
        out.append(("dna_s%d" % strat, dna, 9, strat, None))
    return out


def test_inflate_host_matches_zlib():
    from lra_amd._lib import load_library
    lib = load_library()
    for name, data, level, strat, cuts in _inflate_corpora():
        f = bgzf.bgzf_compress(data, level, strat, cuts=cuts)
        got, st = _inflate(lib, f)
        assert (st == 0).all() and got == data, name
    got, st = _inflate(lib, bgzf.bgzf_compress(b""))                   # an empty member and the EOF member
    assert got == b"" and (st == 0).all() and len(st) == 2


def _corrupt_cases():
    rng = np.random.default_rng(9)
    data = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 50_000)])
    good = bgzf.member(data, 6)
    cases = []
    # (name, member, ISIZE the block table gives it, the status: bgzf.h's LRA_BGZF_ERR_*)
    b = bytearray(good); b[40] ^= 0x10; cases.append(("flipped payload bit", bytes(b), len(data), FLIPPED))
    b = bytearray(good); b[-6] ^= 1; cases.append(("bad crc", bytes(b), len(data), 8))
    cases.append(("isize mismatch", good, len(data) - 1, 9))
    b = bytearray(good); b[-1] ^= 1; cases.append(("isize field", bytes(b), len(data), 9))
    cases.append(("truncated", good[:len(good) // 2], len(data), 1))
    b = bytearray(good); struct.pack_into("<H", b, 16, len(good) + 50); cases.append(("bsize past the end", bytes(b), len(data), 1))
    cases.append(("deflate data cut", _wrap(good[18:18 + (len(good) - 26) // 2], len(data)), len(data), 2))
    # a dynamic block (BFINAL 0, BTYPE 2 least significant bit first) whose code-length code is over-subscribed: HLIT / HDIST / HCLEN, 19 lengths of 1
    bits = [0, 0, 1] + [0] * 5 + [0] * 5 + [1, 1, 1, 1] + [1, 0, 0] * 19
    raw = bytes(sum(bit << k for k, bit in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8)) + b"\0" * 4
    cases.append(("invalid code lengths", _wrap(raw, 10), 10, 4))
    # a fixed block: literal 'A' then a match of length 3 at distance 2 (before the block's start)
    bw = _Bits(); bw.put(1, 1); bw.put(1, 2); bw.code(0x30 + ord("A"), 8); bw.code(1, 7); bw.code(1, 5); bw.code(0, 7)
    cases.append(("distance before the start", _wrap(bw.bytes(), 4), 4, 5))
    bw = _Bits(); bw.put(1, 1); bw.put(3, 2)                           # block type 3
    cases.append(("bad block type", _wrap(bw.bytes(), 1), 1, 4))
    bw = _Bits(); bw.put(1, 1); bw.put(0, 2); bw.put(0, 5); bw.put(0x0005, 16); bw.put(0xfff0, 16)   # a stored block, NLEN not ~LEN
    cases.append(("stored LEN / NLEN", _wrap(bw.bytes(), 5), 5, 6))
    bw = _Bits(); bw.put(1, 1); bw.put(1, 2); bw.code(0x30 + ord("A"), 8); bw.code(0, 7)              # one literal, ISIZE 4
    cases.append(("less data than ISIZE", _wrap(bw.bytes(), 4), 4, 7))
    cases.append(("more data than ISIZE", _wrap(bw.bytes(), 0), 0, 3))
    return cases


FLIPPED = 4    # the flipped bit of "flipped payload bit" lands in the dynamic block's code lengths


class _Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, x, k):                                                # LSB first
        self.v |= x << self.n; self.n += k

    def code(self, x, k):                                               # Huffman codes MSB first
        for i in range(k - 1, -1, -1):
            self.put((x >> i) & 1, 1)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8 + 2, "little")


def _wrap(cdata, isize):
    bsize = 12 + 6 + len(cdata) + 8 - 1
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize) + cdata +
            struct.pack("<II", 0, isize))


def test_inflate_host_corrupt_streams():
    """CPU only: every corrupt member gives an error status, nothing outside the member's ranges is touched"""
    from lra_amd._lib import load_library
    lib = load_library()
    for name, m, isize, status in _corrupt_cases():
        buf = np.frombuffer(m, np.uint8).copy()
        out = np.full(isize + 64, 0xab, np.uint8)
        st = np.full(1, -1, np.int32)
        io_ = np.array([0, len(m)], np.uint64); oo = np.array([0, isize], np.uint64)
        assert lib.lra_bgzf_inflate_host(1, buf.ctypes.data, io_.ctypes.data, oo.ctypes.data, out.ctypes.data, st.ctypes.data) == 0
        assert st[0] == status, (name, st[0])
        assert (out[isize:] == 0xab).all(), name


# ---------------------------------------------------------------------------------------------------------------- the host reader
ORDERS = [1, 7, 1000, 10 ** 9]


@pytest.mark.parametrize("max_bases", ORDERS)
def test_host_reader_bam_and_sam(tmp_path, max_bases):
    recs, p = _corpus(tmp_path)
    first = None
    for key in ("bam", "bam_noeof", "sam", "samgz"):
        got, err = _check_host([p[key]], max_bases)
        assert err is None
        flat = [x for b in got for x in b]
        if first is None:
            first = flat
            assert len(flat) == len(recs)
            assert any(q is None for _, _, q in flat) and any(s == b"" for _, s, _ in flat) and any(b"=" in s for _, s, _ in flat)
            assert {len(n) for n, _, _ in flat} >= {1, 254}
        assert flat == first, key                                       # SAM, BGZF SAM and BAM of the same records: the same reads


def test_host_reader_flag_remove_and_passthrough(tmp_path):
    recs, p = _corpus(tmp_path, seed=2)
    for mask in (0, 0x100, 0x904, 0xffff):
        for key in ("bam", "sam"):
            got, err = _check_host([p[key]], 500, flag_remove=mask, passthrough=mask == 0x100)
            n = sum(len(b) for b in got)
            assert n == sum(1 for r in recs if not r["flag"] & mask), (mask, key)
    got, _ = _check_host([p["bam"]], 10 ** 9, passthrough=True)
    tags = [t for b in got for _, _, _, t in b]
    assert any(t is None for t in tags) and any(t and b"Bf:B:f,0.125,-2.5,0.001" in t for t in tags)
    g2, _ = _check_host([p["samgz"]], 10 ** 9, passthrough=True)
    assert g2 == got
    files = _write_files(tmp_path)
    got, _ = _read_all([files[0], p["bam"]], 10 ** 9, passthrough=True)
    tags = [t for b in got for _, _, _, t in b]
    assert tags[:8] == [None] * 8 and any(tags[8:])                     # FASTA reads: no tags


def test_sam_normalisation_and_errors(tmp_path):
    body = (b"@HD\tVN:1.6\n@SQ\tSN:c\tLN:9\n"
            b"q1\t4\t*\t0\t0\t*\t*\t0\t0\tacgUx\tIIIII\tXX:i:+05\tYY:f:1.50\tZZ:B:i,+3,-4\n"
            b"q2\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"
            b"q3\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\tAA:Z:x y\n")
    sam = tmp_path / "n.sam"; sam.write_bytes(body)
    got, err = _read_all([str(sam)], 10 ** 9, passthrough=True)
    assert err is None
    assert got == [[(b"q1", b"ACGTN", b"IIIII", b"XX:i:5\tYY:f:1.5\tZZ:B:i,3,-4"), (b"q2", b"", None, None), (b"q3", b"ACGT", None, b"AA:Z:x y")]]
    bad = tmp_path / "bad.sam"; bad.write_bytes(body + b"q4\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIII\n" + b"q5\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    for mb in (1, 10 ** 9):
        got, err = _check_host([str(bad)], mb)
        assert err and "record 3" in err and "bad.sam" in err, err
        assert [x[0] for b in got for x in b] == [b"q1", b"q2", b"q3"]


def test_file_sequences(tmp_path):
    recs, p = _corpus(tmp_path, seed=4, n=20)
    files = _write_files(tmp_path)                                      # a.fa b.fa c.fq d.fastq e.fq
    fa, fq = files[0], files[2]
    got, err = _check_host([fa, p["bam"]], 1000)                        # FASTA then BAM: both read
    assert err is None and sum(len(b) for b in got) == 8 + 20
    for seq in ([p["bam"], fa], [p["bam"], p["sam"]], [p["sam"], p["bam"]]):
        for mb in (1, 500, 10 ** 9):
            got, err = _check_host(seq, mb)
            assert err and "not read" in err and os.path.basename(seq[1]) in err, err
    for mb in (1, 300, 10 ** 9):
        got, err = _check_host([fq, p["bam"]], mb)                     # the BAM is read by the next batch, if the one that ended the FASTQ file is not empty
        if err:
            assert "not read" in err and os.path.basename(p["bam"]) in err
    # truncated, bad CRC, a bad record
    raw = bgzf.bam_bytes(recs)
    data = bgzf.bgzf_compress(raw, 6, cuts=list(range(300, len(raw), 300)), eof=False)
    io_, _ = bgzf.blocks(data)
    tr = tmp_path / "trunc.bam"; tr.write_bytes(data[:io_[4] + 30])
    b = bytearray(data); b[io_[5] - 7] ^= 0xff; crc = tmp_path / "crc.bam"; crc.write_bytes(bytes(b))
    cut = tmp_path / "cut.bam"; cut.write_bytes(bgzf.bgzf_compress(raw[:-5]))
    badrec, badbs = _bad_record_files(tmp_path, raw)
    for f, what in ((tr, "compressed offset %d" % io_[4]), (crc, "compressed offset %d" % io_[4]), (cut, "record"), (badrec, "record 1 "),
                    (badbs, "record 2 ")):
        for mb in (1, 10 ** 9):
            got, err = _check_host([str(f)], mb)
            assert err and what in err and f.name in err, (f, err)
    # refused at open: CRAM-like, gzip that is not BGZF, fastq.gz
    from lra_amd import reads_io
    cram = tmp_path / "x.cram"; cram.write_bytes(b"CRAM\3\0" + bytes(100))
    gz = tmp_path / "x.bam.gz"; gz.write_bytes(gzip.compress(raw))
    fqgz = tmp_path / "x.fq.gz"; fqgz.write_bytes(bgzf.bgzf_compress(open(fq, "rb").read()))
    for f in (cram, gz, fqgz):
        with pytest.raises(IOError):
            reads_io.ReadsFile([str(f)])


def _bad_record_files(tmp_path, raw):
    """the BAM bytes raw with record 1's l_read_name = 0, and with record 2's block_size = 20 (below 32)"""
    hl = len(bgzf.bam_bytes([]))
    starts = [hl]
    for _ in range(2):
        starts.append(starts[-1] + 4 + struct.unpack_from("<I", raw, starts[-1])[0])
    r1 = bytearray(raw); r1[starts[1] + 4 + 8] = 0
    r2 = bytearray(raw); struct.pack_into("<I", r2, starts[2], 20)
    a = tmp_path / "badrec.bam"; a.write_bytes(bgzf.bgzf_compress(bytes(r1), cuts=list(range(900, len(raw), 900))))
    b = tmp_path / "badbs.bam"; b.write_bytes(bgzf.bgzf_compress(bytes(r2), cuts=list(range(900, len(raw), 900))))
    return a, b


def test_set_flag_and_passthrough_only_before_the_first_batch(tmp_path):
    from lra_amd import reads_io
    _, p = _corpus(tmp_path, seed=5, n=10)
    rf = reads_io.ReadsFile([p["bam"]])
    assert rf.lib.lra_reads_set_flag_remove(rf.h, 4) == 0 and rf.lib.lra_reads_set_passthrough(rf.h, 1) == 0
    assert rf.lib.lra_reads_set_passthrough(rf.h, 2) != 0
    rf.next_batch(10)
    assert rf.lib.lra_reads_set_flag_remove(rf.h, 0) != 0 and rf.lib.lra_reads_set_passthrough(rf.h, 0) != 0
    rf.close()


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_inflate_device_matches_zlib(ctx):
    from lra_amd._lib import load_library
    lib = load_library()
    for name, data, level, strat, cuts in _inflate_corpora():
        f = bgzf.bgzf_compress(data, level, strat, cuts=cuts)
        got, st = _inflate(lib, f, ctx)
        assert (st == 0).all() and got == data, name
    rng = np.random.default_rng(11)
    big = bytes(np.frombuffer(b"ACGTTTGA", np.uint8)[rng.integers(0, 8, 4000 * 3000)])
    f = bgzf.bgzf_compress(big, 6, cuts=list(range(3000, len(big), 3000)))   # 4000 members in one call
    got, st = _inflate(lib, f, ctx)
    assert len(st) == 4001 and (st == 0).all() and got == big
    io_, _ = bgzf.blocks(f)
    b = bytearray(f); b[io_[7] - 8] ^= 1                                 # a CRC mismatch over valid DEFLATE
    got, st = _inflate(lib, bytes(b), ctx)
    assert st[6] == 8 and (np.delete(st, 6) == 0).all()


def _same_dev_host(ctx, files, max_bases, chunk, **kw):
    host, herr = _check_host(files, max_bases, **kw)
    dev, derr = _read_all(files, max_bases, ctx=ctx, chunk=chunk, **kw)
    assert derr == herr, (derr, herr)
    assert dev == host
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 4096, 4099, 6007])
def test_device_reader_matches_host(ctx, tmp_path, chunk):
    recs, p = _corpus(tmp_path, seed=6, n=80)
    files = _write_files(tmp_path)
    for mb in (1, 1000, 10 ** 9):
        for key in ("bam", "bam_noeof", "sam", "samgz"):
            _same_dev_host(ctx, [p[key]], mb, chunk)
        _same_dev_host(ctx, [p["bam"]], mb, chunk, flag_remove=0x904, passthrough=True)
        _same_dev_host(ctx, [files[0], p["bam"]], mb, chunk, passthrough=True)
        _same_dev_host(ctx, [files[0], p["samgz"]], mb, chunk)
        _same_dev_host(ctx, [p["bam"], files[0]], mb, chunk)
        _same_dev_host(ctx, [files[2], p["bam"]], mb, chunk)
    # a record longer than a step: random bases and qualities, so that its members hold far more compressed bytes than a step of 4096 / 4099 / 6007
    # bytes reads -- the steps in front of it hold no whole record and read on
    rng = np.random.default_rng(12)
    lrec = dict(name=b"long", seq=bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 36000)]), qual=bytes(rng.integers(33, 75, 36000).astype(np.uint8)),
                flag=4, aux=[("RG", "Z", "g")])
    short = _rand_recs(np.random.default_rng(1), 6)
    lraw = bgzf.bam_bytes(short[:3] + [lrec] + short[3:])
    lp = tmp_path / "long.bam"; lp.write_bytes(bgzf.bgzf_compress(lraw, 6, cuts=list(range(5000, len(lraw), 5000))))
    hl = len(bgzf.bam_bytes(short[:3]))
    io_, oo = bgzf.blocks(lp.read_bytes())
    in_long = [i for i in range(len(io_) - 1) if oo[i + 1] > hl and oo[i] < hl + 36000 * 1.5]
    assert io_[in_long[-1]] - io_[in_long[0] + 1] > 4 * 6007                # the members wholly inside the record: several steps' worth
    for mb in (1, 10 ** 9):
        got = _same_dev_host(ctx, [str(lp)], mb, chunk, passthrough=True)
        assert max(len(x[1]) for b in got for x in b) == 36000
    raw = bgzf.bam_bytes(recs)
    data = bgzf.bgzf_compress(raw, 6, cuts=list(range(700, len(raw), 700)), eof=False)
    io_, _ = bgzf.blocks(data)
    tr = tmp_path / "trunc.bam"; tr.write_bytes(data[:io_[9] + 30])
    b = bytearray(data); b[io_[12] - 7] ^= 0xff; crc = tmp_path / "crc.bam"; crc.write_bytes(bytes(b))
    badrec, badbs = _bad_record_files(tmp_path, raw)
    for f in (tr, crc, badrec, badbs):
        for mb in (1, 10 ** 9):
            _same_dev_host(ctx, [str(f)], mb, chunk)


def _genome_and_reads(tmp_path, err, seed):
    genome = synth.make_genome(400_000, seed=9, repeat_frac=0.2, n_families=3)
    CH = [0, 150_000, len(genome)]
    reads, _ = synth.simulate_reads(genome, 24, 6000, 1500, err, seed=seed)
    rng = np.random.default_rng(seed)
    recs = [dict(name=b"r%d" % i, seq=r.tobytes(), qual=None if i % 5 == 2 else bytes(rng.integers(35, 70, len(r)).astype(np.uint8)), flag=4,
                 aux=[] if i % 4 == 1 else [("RG", "Z", "run%d" % i), ("np", "C", i), ("rq", "f", 0.99)]) for i, r in enumerate(reads)]
    recs.append(dict(name=b"unmappable", seq=bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 3000)]), qual=None, flag=4, aux=[("XX", "i", 1)]))
    bam = tmp_path / "reads.bam"; bgzf.write_bam(str(bam), recs)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (r["name"], r["seq"], r["qual"] or b"I" * len(r["seq"])) for r in recs))
    return genome, CH, recs, str(bam), str(fq)


def _map_records(ctx, mapper, files, passthrough=False):
    from lra_amd import reads_io
    out = []
    rf = reads_io.ReadsFile(files, ctx=ctx, chunk=64 << 10, passthrough=passthrough)
    while True:
        b = rf.next_batch(60_000)
        if b is None:
            break
        res = reads_io.map_reads_device(mapper, b)
        out += mapper.records(res, b["names"], b["seqs"], quals=b["quals"], passthrough=b["tags"] if passthrough else None)
    rf.close()
    return out


def _check_mapping(ctx, mapper, recs, bam, fq):
    fq_text = _map_records(ctx, mapper, [fq])
    bam_text = _map_records(ctx, mapper, [bam])
    assert len(bam_text) == len(recs)
    noq = {r["name"] for r in recs if r["qual"] is None}
    for r, t_fq, t_bam in zip(recs, fq_text, bam_text):
        if r["name"] in noq:                                            # no qualities: '*' where the FASTQ's were
            lines = t_bam.split(b"\n")[:-1]
            assert all(l.split(b"\t")[10] == b"*" for l in lines), r["name"]
            assert [l.split(b"\t")[:10] for l in lines] == [l.split(b"\t")[:10] for l in t_fq.split(b"\n")[:-1]]
        else:
            assert t_bam == t_fq, r["name"]
    pt = _map_records(ctx, mapper, [bam], passthrough=True)
    for r, t, tp in zip(recs, bam_text, pt):
        tags = _fmt_aux(bgzf._aux_bin(r["aux"]))
        exp = b"".join(l + (b"\t" + tags if tags else b"") + b"\n" for l in t.split(b"\n")[:-1])
        assert tp == exp, r["name"]
    assert any(b"\t*\t0\t0\t" in t for t in pt[-1:]) and pt[-1].endswith(b"\tXX:i:1\n")
    assert sum(b"\t*\t0\t0\t" not in t for t in bam_text) >= 20


@pytest.mark.gpu
def test_map_bam_ont(ctx, tmp_path):
    from lra_amd import mapread
    genome, CH, recs, bam, fq = _genome_and_reads(tmp_path, 0.10, 4)
    o = mapread.LowAccOptions()
    ik, ip = synth.build_global_index(genome, o.globalK, o.globalW, 100)
    mapper = mapread.LowAccMapper(ctx, genome, ik, ip, [b"chrA", b"chrB"], CH, o)
    _check_mapping(ctx, mapper, recs, bam, fq)


@pytest.mark.gpu
def test_map_bam_ccs(ctx, tmp_path):
    from lra_amd import mapread
    genome, CH, recs, bam, fq = _genome_and_reads(tmp_path, 0.01, 6)
    mapper = mapread.HighAccMapper(ctx, genome, None, None, [b"chrA", b"chrB"], CH, preset="ccs")
    _check_mapping(ctx, mapper, recs, bam, fq)


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["-ONT", "-CCS"])
def test_map_files_tool_bam(tmp_path, preset):
    genome = synth.make_genome(300_000, seed=3, repeat_frac=0.2, n_families=2)
    g = tmp_path / "genome.fa"
    s = genome.tobytes()
    g.write_bytes(b">chr1\n" + b"\n".join(s[x:x + 70] for x in range(0, len(s), 70)) + b"\n")
    reads, _ = synth.simulate_reads(genome, 30, 5000, 1500, 0.08 if preset == "-ONT" else 0.01, seed=11)
    recs = [dict(name=b"m%d" % i, seq=r.tobytes(), qual=b"5" * len(r), flag=4 if i % 6 else 0x904, aux=[("RG", "Z", "x%d" % i)]) for i, r in enumerate(reads)]
    bam = tmp_path / "r.bam"; bgzf.write_bam(str(bam), recs)
    fq = tmp_path / "r.fq"; fq.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (r["name"], r["seq"], r["qual"]) for r in recs))
    fq_kept = tmp_path / "k.fq"; fq_kept.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (r["name"], r["seq"], r["qual"]) for r in recs if not r["flag"] & 0x900))

    def run(reads, *extra):
        o = tmp_path / "out.sam"
        cmd = [sys.executable, os.path.join(ROOT, "tools", "map_files.py"), preset, str(g), str(reads), "-o", str(o), "--batch-bases", "40000", *extra]
        p = subprocess.run(cmd, capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return [l for l in o.read_bytes().split(b"\n") if l and not l.startswith(b"@")]
    assert run(bam) == run(fq)
    assert run(bam, "-Flag", "2304") == run(fq_kept)
    pt = run(bam, "--passthrough")
    assert len(pt) == len(run(fq)) and all(l.split(b"\t")[-1] == b"RG:Z:x" + l.split(b"\t")[0][1:] for l in pt)
