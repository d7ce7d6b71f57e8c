"""The inputs of the BGZF deflate tests (test_bgzf_deflate.py on the host form, test_bgzf_deflate_device.py on the kernel): one batch of edge members,
three seeded texts, the checks every member has to pass, and a small DEFLATE reader that lists a member's blocks and tokens."""
import functools
import heapq
import struct
import zlib

import numpy as np

from lra_amd import bgzf
from lra_amd._lib import load_library

IN_MAX, SLOT = 65280, 65536
EDGE_LENGTHS = [0, 1, 2, 3, 4, 257, 258, 259, 260, 32767, 32768, 32769, 65279, 65280]
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


@functools.lru_cache(None)
def sam_like():
    """about 1 MB: names, random ACGT of 500, 3000 and 30000 bases, skewed qualities, =XID CIGARs, tags"""
    rng = np.random.default_rng(11)
    out = []
    qual_p = np.array([0.5 ** (1 + i / 3) for i in range(40)]); qual_p /= qual_p.sum()
    for i in range(15 * 3):
        n = [500, 3000, 30000][i % 3]
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
        qual = bytes((73 - rng.choice(40, n, p=qual_p)).astype(np.uint8))
        ops, left = [], n
        while left:
            k = min(left, int(rng.integers(1, 200)))
            op = "=XID"[int(rng.choice(4, p=[0.7, 0.1, 0.1, 0.1]))]
            ops.append("%d%s" % (k, op))
            if op != "D":
                left -= k
        f = ["m64011_190830_220126/%d/ccs" % rng.integers(1, 10 ** 7), str(int(rng.choice([0, 16, 2048, 2064]))), "chr%d" % rng.integers(1, 23),
             str(int(rng.integers(1, 2 * 10 ** 8))), str(int(rng.integers(0, 61))), "".join(ops), "*", "0", "0", seq.decode(), qual.decode(),
             "NM:i:%d" % rng.integers(0, n // 8 + 1), "AS:i:%d" % rng.integers(0, 2 * n), "TP:A:P", "NV:f:%.2f" % rng.random()]
        out.append("\t".join(f) + "\n")
    return "".join(out).encode()


@functools.lru_cache(None)
def paf_like():
    """about 0.5 MB of PAF lines"""
    rng = np.random.default_rng(12)
    out = []
    for i in range(4300):
        ql = int(rng.integers(1000, 40000)); qs = int(rng.integers(0, 200)); qe = ql - int(rng.integers(0, 200))
        ts = int(rng.integers(1, 2 * 10 ** 8)); al = qe - qs + int(rng.integers(-50, 50))
        out.append("\t".join(["m64011_190830_220126/%d/ccs" % rng.integers(1, 10 ** 7), str(ql), str(qs), str(qe), "+-"[int(rng.integers(2))],
                              "chr%d" % rng.integers(1, 23), str(int(rng.integers(5 * 10 ** 7, 25 * 10 ** 7))), str(ts), str(ts + al),
                              str(al - int(rng.integers(0, al // 10 + 1))), str(al), str(int(rng.integers(0, 61))), "NM:i:%d" % rng.integers(0, 4000),
                              "AO:i:%d" % rng.integers(1, 5), "tp:A:P"]) + "\n")
    return "".join(out).encode()


@functools.lru_cache(None)
def repetitive():
    """one 71-byte line, 3000 times"""
    return (b"@SQ\tSN:chr1_KI270706v1_random\tLN:175055\tM5:62def1a794b3e18192863d187af956e6"[:70] + b"\n") * 3000


def cut(text):
    return [text[a:a + IN_MAX] for a in range(0, len(text), IN_MAX)]


FIB_COUNTS = [1, 1, 3, 4, 7, 11, 18, 29, 47, 76, 123, 199, 322, 521, 843, 1364]


@functools.lru_cache(None)
def fibonacci_counts():
    """16 byte values with the counts FIB_COUNTS, 3569 bytes inside one deflate block.  With the end-of-block symbol's 1 in front, every count from the
    fourth on is the sum of all but the last before it plus one, so a Huffman tree over them is a chain 16 deep however ties are broken.  The order has to
    leave the encoder no match (a match takes literals out of the counts): a seeded shuffle, then, as long as the host encoder finds matches, one byte
    under each match is swapped with a byte somewhere else and the encoder runs again.  The counts never change; the order follows the encoder's hash and
    match rule, whatever they are."""
    rng = np.random.default_rng(5)
    f = np.frombuffer(b"".join(bytes([33 + s]) * c for s, c in enumerate(FIB_COUNTS)), np.uint8).copy()
    rng.shuffle(f)
    for _ in range(400):
        out, out_len, status = run_host([f.tobytes()])
        blocks = deflate_blocks(members_of(out, out_len, status)[0])
        pos, found = 0, []
        for b in blocks:
            for t in b["tokens"]:
                if isinstance(t, tuple):
                    found.append((pos, t[0]))
                    pos += t[0]
                else:
                    pos += 1
        if not found:
            return f.tobytes()
        assert all(b["type"] == 2 for b in blocks)
        for p, n in found:
            i, j = p + int(rng.integers(min(n, 6))), int(rng.integers(len(f)))
            f[i], f[j] = f[j], f[i]
    raise AssertionError("no order without a match found")


@functools.lru_cache(None)
def edge_members():
    """[(name, data)]: the batch both forms run.  Data of 65281 bytes is the one member that must be refused."""
    rng = np.random.default_rng(13)
    rnd = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))
    sam = sam_like()
    items = [("len%d" % n, sam[1000:1000 + n]) for n in EDGE_LENGTHS]
    items.append(("too_long", sam[:IN_MAX + 1]))
    items.append(("one_byte_value", b"A" * 5000))
    items.append(("period3", b"abc" * 2000))
    p258 = rnd(258)
    items.append(("period258", p258 * 40))
    x = rnd(300)
    items.append(("dist32768", x + bytes(32768 - 300) + x))
    items.append(("dist32769", x + bytes(32769 - 300) + x))
    items.append(("all_bytes", bytes(range(256)) * 8))
    items.append(("one_symbol", b"A" * 60))                   # inside one group of 64: no match is looked for, and 60 literals of one value beat a stored block
    items.append(("one_distance", rnd(2048) * 8))
    items.append(("fibonacci", fibonacci_counts()))
    items.append(("random", rnd(IN_MAX)))
    return items


def run_host(datas):
    """lra_bgzf_deflate_host over the batch into a buffer of 0xab -> (out, out_len, status), 64 sentinel bytes in front of and behind the slots"""
    lib = load_library()
    n = len(datas)
    buf = np.frombuffer(b"".join(datas), np.uint8).copy()
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in datas], dtype=np.uint64)
    out, out_len, status = np.full(64 + n * SLOT + 64, 0xab, np.uint8), np.full(n, 0xffffffff, np.uint32), np.full(n, -1, np.int32)
    assert lib.lra_bgzf_deflate_host(n, buf.ctypes.data, off.ctypes.data, out.ctypes.data + 64, out_len.ctypes.data, status.ctypes.data) == 0
    assert (out[:64] == 0xab).all() and (out[-64:] == 0xab).all()
    return out[64:-64], out_len, status


def members_of(out, out_len, status):
    return [out[i * SLOT:i * SLOT + int(out_len[i])].tobytes() if status[i] == 0 else None for i in range(len(status))]


def check_member(m, data):
    """framing, raw inflate by zlib, CRC-32 and ISIZE"""
    assert 28 <= len(m) <= SLOT
    assert m[:16] == bytes.fromhex("1f8b08040000000000ff060042430200"), m[:18].hex()
    assert struct.unpack_from("<H", m, 16)[0] == len(m) - 1
    d = zlib.decompressobj(-15)
    got = d.decompress(m[18:-8]) + d.flush()
    assert d.eof and d.unused_data == b""
    assert got == data
    assert struct.unpack_from("<II", m, len(m) - 8) == (zlib.crc32(data) & 0xffffffff, len(data))


def check_sentinels(out, out_len, status):
    """every byte of a slot behind its member (the whole slot of a refused one) still holds the sentinel"""
    for i in range(len(status)):
        n = int(out_len[i]) if status[i] == 0 else 0
        assert (out[i * SLOT + n:(i + 1) * SLOT] == 0xab).all(), i


def inflate_host(members, datas):
    """lra_bgzf_inflate_host over the members packed back to back -> status 0 everywhere and the data"""
    lib = load_library()
    n = len(members)
    comp = np.frombuffer(b"".join(members), np.uint8).copy()
    io_ = np.zeros(n + 1, np.uint64); io_[1:] = np.cumsum([len(m) for m in members], dtype=np.uint64)
    oo = np.zeros(n + 1, np.uint64); oo[1:] = np.cumsum([len(d) for d in datas], dtype=np.uint64)
    out, st = np.zeros(int(oo[-1]) + 1, np.uint8), np.full(n, -1, np.int32)
    assert lib.lra_bgzf_inflate_host(n, comp.ctypes.data, io_.ctypes.data, oo.ctypes.data, out.ctypes.data, st.ctypes.data) == 0
    assert (st == 0).all(), st
    assert out[:-1].tobytes() == b"".join(datas)


class _Reader:
    def __init__(self, b):
        self.b, self.p = b, 0

    def bits(self, n):
        v = 0
        for i in range(n):
            v |= ((self.b[self.p >> 3] >> (self.p & 7)) & 1) << i
            self.p += 1
        return v

    def sym(self, table):
        code, n = 0, 0
        while True:
            code = (code << 1) | self.bits(1); n += 1
            if (n, code) in table:
                return table[(n, code)]
            assert n < 16


def _table(lengths):
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    t = {}
    for s, n in enumerate(lengths):
        if n:
            t[(n, nxt[n])] = s
            nxt[n] += 1
    return t


def deflate_blocks(m):
    """a member's DEFLATE blocks -> [dict(type, lit_lengths, dist_lengths, cl_symbols, tokens)]; a token is a literal's value or (length, distance)"""
    r, out = _Reader(m[18:-8]), []
    while True:
        last, typ = r.bits(1), r.bits(2)
        blk = dict(type=typ, tokens=[], lit_lengths=[], dist_lengths=[], cl_symbols=[])
        if typ == 0:
            r.p = (r.p + 7) & ~7
            n, nn = r.bits(16), r.bits(16)
            assert n == (~nn & 0xffff)
            blk["stored"] = n
            r.p += 8 * n
        else:
            assert typ == 2
            hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
            cl = [0] * 19
            for i in range(hclen):
                cl[CL_ORDER[i]] = r.bits(3)
            ct, lens = _table(cl), []
            while len(lens) < hlit + hdist:
                s = r.sym(ct)
                blk["cl_symbols"].append(s)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + r.bits(2))
                elif s == 17:
                    lens += [0] * (3 + r.bits(3))
                else:
                    lens += [0] * (11 + r.bits(7))
            assert len(lens) == hlit + hdist
            blk["lit_lengths"], blk["dist_lengths"] = lens[:hlit], lens[hlit:]
            lt, dt = _table(lens[:hlit]), _table(lens[hlit:])
            while True:
                s = r.sym(lt)
                if s < 256:
                    blk["tokens"].append(s)
                elif s == 256:
                    break
                else:
                    ln = LBASE[s - 257] + r.bits(LEXT[s - 257])
                    ds = r.sym(dt)
                    blk["tokens"].append((ln, DBASE[ds] + r.bits(DEXT[ds])))
        out.append(blk)
        if last:
            assert (r.p + 7) >> 3 == len(r.b)
            return out


def bgzf_size(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    return len(bgzf.bgzf_compress(text, level, strategy, eof=False))


def huffman_depth(counts):
    """the depth of an unrestricted Huffman tree over the counts (the deepest choice at a tie)"""
    h = [(c, -0, i) for i, c in enumerate(counts)]
    heapq.heapify(h)
    k = len(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], min(a[1], b[1]) - 1, k))
        k += 1
    return -h[0][1]
