"""lra_bgzf_inflate_lut_batch (inflate_lut.hip, the table-driven kernel) against lra_bgzf_inflate_host (the shared decoder): byte for byte and status for status
over one batch of members, with a sentinel in every byte no member owns."""
import struct
import zlib

import numpy as np
import pytest

from lra_amd import bgzf
from test_input_bam import _Bits, _corrupt_cases, _wrap

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _canonical(lengths):
    """code of every symbol with a length (RFC 1951 3.2.2)"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = {}
    for s, n in enumerate(lengths):
        if n:
            codes[s] = nxt[n]
            nxt[n] += 1
    return codes


def _len_sym(n):
    s = max(i for i in range(29) if LBASE[i] <= n) if n < 258 else 28
    return s, n - LBASE[s]


def _dist_sym(d):
    s = max(i for i in range(30) if DBASE[i] <= d)
    return s, d - DBASE[s]


def _hand_dynamic():
    """One final dynamic block.  Literal/length code: 11 symbols with the lengths 1..11 and the literals 'a'..'p' with 15 bits each (2^-11 shared by 16
    codes); distance code: the chain 1, 2, .. 14, 15, 15 over the symbols 0..15.  So both codes reach 15 bits and the symbols behind the lookup tables'
    10 and 8 bits take the fall-back walk.  The code-length code spells the 316 lengths with 16 (the run of 15s), 17 and 18 (the zero runs)."""
    lit = [0] * 286
    for n, s in enumerate([65, 67, 71, 84, 10, 256, 257, 264, 265, 285, 78]):      # A C G T \n EOB len3 len10 len11-12 len258 N
        lit[s] = n + 1
    for s in range(97, 113):
        lit[s] = 15
    dist = [0] * 30
    for s in range(14):
        dist[s] = s + 1
    dist[14] = dist[15] = 15
    cl = [0] * 19
    for s in [0, 17, 18, 16, 15, 1, 2, 3, 4, 5, 6, 7, 8]:
        cl[s] = 4
    for s in range(9, 15):
        cl[s] = 5
    lc, dc, cc = _canonical(lit), _canonical(dist), _canonical(cl)
    bw = _Bits()
    bw.put(1, 1); bw.put(2, 2); bw.put(286 - 257, 5); bw.put(30 - 1, 5); bw.put(19 - 4, 4)
    for s in CL_ORDER:
        bw.put(cl[s], 3)
    seq, i, used = lit + dist, 0, set()
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 11:
            k = min(run, 138); bw.code(cc[18], cl[18]); bw.put(k - 11, 7); used.add(18)
        elif v == 0 and run >= 3:
            k = min(run, 10); bw.code(cc[17], cl[17]); bw.put(k - 3, 3); used.add(17)
        elif v and run >= 4:
            bw.code(cc[v], cl[v]); k = 1
            left = run - 1
            while left >= 3:
                r = min(left, 6); bw.code(cc[16], cl[16]); bw.put(r - 3, 2); used.add(16); left -= r; k += r
        else:
            k = 1; bw.code(cc[v], cl[v])
        i += k
    assert used == {16, 17, 18}
    out = bytearray()

    def literal(c):
        bw.code(lc[c], lit[c]); out.append(c)

    def match(n, d):
        s, e = _len_sym(n)
        bw.code(lc[257 + s], lit[257 + s]); bw.put(e, LEXT[s])
        s, e = _dist_sym(d)
        bw.code(dc[s], dist[s]); bw.put(e, DEXT[s])
        for _ in range(n):
            out.append(out[-d])

    rng = np.random.default_rng(5)
    for c in rng.choice(np.frombuffer(b"ACGTN\nabcdefghijklmnop", np.uint8), 400):
        literal(int(c))
    for n, d in [(3, 1), (10, 17 + 5), (12, 193 + 40), (258, 129 + 63), (258, 2), (11, 200), (258, 1), (3, 4), (10, 7), (12, 97 + 31), (258, 256)]:
        match(n, d)
        literal(97 + (n + d) % 16)
    bw.code(lc[256], lit[256])
    raw, data = bw.bytes(), bytes(out)
    assert zlib.decompress(raw, -15) == data                                   # the hand-made stream is valid DEFLATE
    return _member_of(raw, data)


def _member_of(raw, data):
    m = bytearray(_wrap(raw, len(data)))
    struct.pack_into("<I", m, len(m) - 8, zlib.crc32(data) & 0xffffffff)
    return bytes(m)


def _hand_far_match(rng):
    """a stored block of 32768 bytes, then a fixed block: a match of length 258 at distance 32768"""
    head = bytes(rng.integers(0, 256, 32768).astype(np.uint8))
    bw = _Bits()
    bw.put(0, 1); bw.put(0, 2); bw.put(0, 5); bw.put(32768, 16); bw.put(32768 ^ 0xffff, 16); bw.put(int.from_bytes(head, "little"), 8 * 32768)
    bw.put(1, 1); bw.put(1, 2); bw.code(0xc0 + 5, 8); bw.code(29, 5); bw.put(32768 - 24577, 13); bw.code(0, 7)
    data = head + head[:258]
    raw = bw.bytes()
    assert zlib.decompress(raw, -15) == data
    return _member_of(raw, data)


def _fastq_like(rng, n):
    out = bytearray()
    k = 0
    while len(out) < n:
        ln = int(rng.integers(50, 3000))
        out += b"@read%d/ccs\n" % k + bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)]) + b"\n+\n" + bytes((33 + rng.integers(0, 42, ln)).astype(np.uint8)) + b"\n"
        k += 1
    return bytes(out[:n])


def _batch():
    """(member, the ISIZE its table entry gives it, the status bgzf.h defines for it) in batch order: a bad member after every few good ones"""
    rng = np.random.default_rng(17)
    text, rnd, ones = _fastq_like(rng, 65536), bytes(rng.integers(0, 256, 60000).astype(np.uint8)), b"\x07" * 65536
    good = []
    for level, strat in [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)]:
        for kind, data in (("text", text), ("rnd", rnd), ("ones", ones)):
            sizes = [0, 1, 2, 3, 255, 256, 1000, 4093, 20001, 30011, 60000 if kind == "rnd" or level == 0 else 65536]
            for n in sizes:
                good.append(bgzf.member(data[:n], level, strat))
    good.append(_hand_dynamic())
    good.append(_hand_far_match(rng))
    far = text[:300] + rnd[:32000] + text[:300]                                 # zlib's own farthest matches (level 9: distances up to 32506)
    good.append(bgzf.member(far, 9))
    bad = [(m, isize, st) for _, m, isize, st in _corrupt_cases()]
    assert {st for _, _, st in bad} == set(range(1, 10))
    items, step = [], len(good) // len(bad)
    for i, m in enumerate(good):
        items.append((m, struct.unpack_from("<I", m, len(m) - 4)[0], 0))
        if i % step == step - 1 and bad:
            items.append(bad.pop())
    assert not bad
    return items


@pytest.mark.gpu
def test_inflate_lut_matches_host(ctx):
    import torch
    lib = ctx.lib
    items = _batch()
    n = len(items)
    assert 120 <= n <= 260
    # a member table is contiguous (out_off[i + 1] ends member i), so the batch goes in two launches into one buffer: 7 sentinel bytes in front, 13
    # between the two halves' ranges (odd numbers: unaligned starts), 64 behind
    half, gap = n // 2, 13
    comp = b"".join(m for m, _, _ in items)
    in_off = [0]
    for m, _, _ in items:
        in_off.append(in_off[-1] + len(m))
    lo = [7]
    for _, isize, _ in items[:half]:
        lo.append(lo[-1] + isize)
    hi = [lo[-1] + gap]
    for _, isize, _ in items[half:]:
        hi.append(hi[-1] + isize)
    total = hi[-1] + 64
    a_in = np.frombuffer(comp, np.uint8).copy()
    parts = [(0, half, np.array(in_off[:half + 1], np.uint64), np.array(lo, np.uint64)), (half, n, np.array(in_off[half:], np.uint64), np.array(hi, np.uint64))]
    rng_of = lambda i: (lo[i], lo[i + 1]) if i < half else (hi[i - half], hi[i - half + 1])
    h_out, h_st = np.full(total, 0xab, np.uint8), np.full(n, -1, np.int32)
    for a, b, io_, oo in parts:
        assert lib.lra_bgzf_inflate_host(b - a, a_in.ctypes.data, io_.ctypes.data, oo.ctypes.data, h_out.ctypes.data, h_st[a:].ctypes.data) == 0
    for i, (_, _, st) in enumerate(items):
        assert h_st[i] == st, (i, h_st[i], st)
    dev = lambda a: torch.from_numpy(a.view(np.uint8)).cuda()
    t_in, t_out, t_st = dev(a_in), dev(np.full(total, 0xab, np.uint8)), dev(np.full(n, -1, np.int32))
    for a, b, io_, oo in parts:
        t_io, t_oo = dev(io_), dev(oo)
        assert lib.lra_bgzf_inflate_lut_batch(ctx.h, b - a, t_in.data_ptr(), t_io.data_ptr(), t_oo.data_ptr(), t_out.data_ptr(), t_st.data_ptr() + 4 * a) == 0
    d_out, d_st = t_out.cpu().numpy(), t_st.cpu().numpy().view(np.int32)
    assert np.array_equal(d_st, h_st), np.nonzero(d_st != h_st)[0][:8]
    for a, b in [(0, lo[0]), (lo[-1], hi[0]), (hi[-1], total)]:                              # the padding in front, between and behind
        assert (d_out[a:b] == 0xab).all() and (h_out[a:b] == 0xab).all()
    for i in range(n):
        a, b = rng_of(i)
        if h_st[i] == 0:
            assert np.array_equal(d_out[a:b], h_out[a:b]), i                                # a good member: byte for byte (its neighbours may be bad)
    # a bad member sets only its own status (checked above) and writes only inside its own range: the buffers differ, if at all, inside bad ranges
    diff = np.nonzero(d_out != h_out)[0]
    bad_ranges = [rng_of(i) for i in range(n) if h_st[i]]
    assert all(any(a <= p < b for a, b in bad_ranges) for p in diff)


@pytest.mark.gpu
def test_inflate_lut_unaligned_single_members(ctx):
    """every start alignment of input and output, sentinels on both sides of one member"""
    import torch
    lib = ctx.lib
    rng = np.random.default_rng(2)
    data = _fastq_like(rng, 9001)
    m = bgzf.member(data, 6)
    for shift_in in range(4):
        for shift_out in range(4):
            comp = np.frombuffer(bytes(shift_in) + m + bytes(5), np.uint8).copy()
            a_io = np.array([shift_in, shift_in + len(m)], np.uint64)
            a_oo = np.array([shift_out, shift_out + len(data)], np.uint64)
            dev = lambda a: torch.from_numpy(a.view(np.uint8)).cuda()
            t_in, t_io, t_oo, t_out, t_st = dev(comp), dev(a_io), dev(a_oo), dev(np.full(len(data) + 16, 0xab, np.uint8)), dev(np.full(1, -1, np.int32))
            assert lib.lra_bgzf_inflate_lut_batch(ctx.h, 1, t_in.data_ptr(), t_io.data_ptr(), t_oo.data_ptr(), t_out.data_ptr(), t_st.data_ptr()) == 0
            out = t_out.cpu().numpy()
            assert t_st.cpu().numpy().view(np.int32)[0] == 0
            assert out[shift_out:shift_out + len(data)].tobytes() == data
            assert (out[:shift_out] == 0xab).all() and (out[shift_out + len(data):] == 0xab).all()
