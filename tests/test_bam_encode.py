"""The device primitives of BAM output -- lra_bam_cigar_batch, lra_bam_pack_seq_batch, lra_bam_phred_batch -- against numpy on crafted inputs, with guard
bytes on both sides of every result."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 0xA5
NG = 48                                  # guard bytes on either side
LENGTHS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 8191, 8192, 8193, 20000]
NT16 = "=ACMGRSVTWYHKDBN"
TAB = np.full(256, 15, np.uint8)
for _k, _c in enumerate(NT16):
    TAB[ord(_c)] = _k
    TAB[ord(_c.lower())] = _k


def _dev(ctx, a, view):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return None
    return torch.from_numpy(a.view(view).copy()).to(ctx.device)


def _guarded(ctx, call, data_of, n_bytes_of):
    """Run `call` once to size the context's buffers, lay guards in front of and behind the result's data, run it again -> (result, the data's bytes)."""
    import torch
    r0 = call()
    nb, p = int(n_bytes_of(r0)), int(data_of(r0))
    guard = torch.full((NG,), GUARD, dtype=torch.uint8, device=ctx.device)
    for at in (p - NG, p + nb):
        ctx.check(ctx.lib.lra_copy_device(ctx.h, C.c_void_p(at), C.c_void_p(guard.data_ptr()), C.c_uint64(NG)))
    torch.cuda.synchronize()
    res = call()
    assert int(n_bytes_of(res)) == nb and int(data_of(res)) == p
    raw = ctx.to_host(p - NG, nb + 2 * NG, np.uint8).tobytes()
    assert raw[:NG] == bytes([GUARD]) * NG, "bytes in front of the result were written"
    assert raw[NG + nb:] == bytes([GUARD]) * NG, "bytes behind the result were written"
    return res, raw[NG:NG + nb]


# ---- CIGAR ------------------------------------------------------------------------------------------------------------------------------------------------
def _cigar_expect(runs, pre, suf, op):
    runs = np.asarray(runs, np.uint32)
    ops = (runs & ~np.uint32(15)) | np.asarray([7, 8, 1, 2], np.uint32)[runs & 3]
    c = 5 if op == "H" else 4
    head = [(pre << 4) | c] if pre > 0 else []
    tail = [(suf << 4) | c] if suf > 0 else []
    return np.concatenate([np.asarray(head, np.uint32), ops, np.asarray(tail, np.uint32)]).astype(np.uint32)


def _cigar_run(ctx, lists, pre=None, suf=None, op=None):
    from lra_amd import bam
    n = len(lists)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, np.uint32) for x in lists]) if off[-1] else np.zeros(0, np.uint32)
    args = (_dev(ctx, flat, np.int32), _dev(ctx, off, np.int64), None if pre is None else _dev(ctx, np.asarray(pre, np.int32), np.int32),
            None if suf is None else _dev(ctx, np.asarray(suf, np.int32), np.int32), None if op is None else _dev(ctx, np.frombuffer(op.encode(), np.uint8), np.uint8))
    res, raw = _guarded(ctx, lambda: bam.bam_cigar_batch(ctx, *args, raw=True), lambda r: r.d_ops, lambda r: 4 * int(r.n_ops))
    assert int(res.n_aln) == n
    o = ctx.to_host(res.d_off, n + 1, np.uint64)
    assert int(o[0]) == 0 and int(o[-1]) == int(res.n_ops)
    ops = np.frombuffer(raw, np.uint32)
    got = [ops[int(o[i]):int(o[i + 1])] for i in range(n)]
    zero = [0] * n
    exp = [_cigar_expect(x, (pre or zero)[i], (suf or zero)[i], (op or "S" * n)[i]) for i, x in enumerate(lists)]
    for i, (g, e) in enumerate(zip(got, exp)):
        assert np.array_equal(g, e), (i, len(g), len(e))
    return got


def _runs(rng, n):
    ln = rng.choice(np.asarray([1, 2, 3, 15, 16, 255, 4096, (1 << 28) - 1], np.int64), n)
    return ((ln << 4) | rng.integers(0, 4, n)).astype(np.uint32)


def test_cigar_every_op_and_the_length_edges(ctx):
    edge = [1, (1 << 28) - 1]
    got = _cigar_run(ctx, [[(v << 4) | k for v in edge] for k in range(4)] + [[(v << 4) | k] for k in range(4) for v in edge])
    assert [int(x) for x in got[0]] == [(1 << 4) | 7, 0xfffffff7] and [int(x) & 15 for x in np.concatenate(got[:4])] == [7, 7, 8, 8, 1, 1, 2, 2]


@pytest.mark.parametrize("clips", [False, True])
def test_cigar_alignment_sizes(ctx, clips):
    rng = np.random.default_rng(11)
    sizes = [0, 1, 63, 64, 65, 4097, 0, 1, 255, 256, 257, 0]
    lists = [_runs(rng, n) for n in sizes]
    if not clips:
        _cigar_run(ctx, lists)
        return
    n = len(lists)
    pre = [int(x) for x in rng.choice([0, -3, 7, (1 << 27) + 5], n)]
    suf = [int(x) for x in rng.choice([0, -1, 9, 100_000], n)]
    for op in (None, "S" * n, "H" * n, ("SH" * n)[:n]):
        got = _cigar_run(ctx, lists, pre, suf, op)
        assert sum(len(g) for g in got) == sum(sizes) + sum(p > 0 for p in pre) + sum(s > 0 for s in suf)
    _cigar_run(ctx, lists, pre, None, None)
    _cigar_run(ctx, lists, None, suf, "H" * n)
    _cigar_run(ctx, lists, [0] * n, [-5] * n, None)                            # clips <= 0: no op
    assert [list(x) for x in _cigar_run(ctx, [[], [], []], [5, 0, 0], [0, 0, 12], "HSH")] == [[(5 << 4) | 5], [], [(12 << 4) | 5]]


def test_cigar_empty_batch(ctx):
    assert _cigar_run(ctx, []) == []
    assert [len(x) for x in _cigar_run(ctx, [[]])] == [0]


# ---- SEQ --------------------------------------------------------------------------------------------------------------------------------------------------
def _pack_expect(src, off, ln):
    if off + ln > len(src):
        c = np.full(ln, 15, np.uint8)
    else:
        c = TAB[src[off:off + ln]]
    if ln & 1:
        c = np.concatenate([c, np.zeros(1, np.uint8)])
    return ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes()


def _pack_run(ctx, src, ranges):
    from lra_amd import bam
    n = len(ranges)
    d_src = _dev(ctx, src, np.uint8)
    d_rng = _dev(ctx, np.asarray(ranges, np.uint64).reshape(-1, 2), np.int64)
    res, raw = _guarded(ctx, lambda: bam.bam_pack_seq_batch(ctx, d_rng, d_src, raw=True), lambda r: r.d_data, lambda r: r.n_bytes)
    assert int(res.n) == n
    o = ctx.to_host(res.d_off, n + 1, np.uint64)
    exp = [_pack_expect(src, a, ln) for a, ln in ranges]
    assert [int(x) for x in o] == [0] + [int(x) for x in np.cumsum([len(e) for e in exp])]
    for i, e in enumerate(exp):
        g = raw[int(o[i]):int(o[i + 1])]
        if g != e:
            at = next(k for k in range(len(e)) if g[k] != e[k])
            raise AssertionError("range %d %r: byte %d of %d is %02x, not %02x" % (i, ranges[i], at, len(e), g[at], e[at]))
    return raw


def _bases(rng, n):
    src = np.frombuffer(b"ACGTNacgtn", np.uint8)[rng.integers(0, 10, n)].copy()
    k = rng.integers(0, n, n // 16)
    src[k] = rng.integers(0, 256, len(k))                                       # any byte, here and there
    return src


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_pack_seq_every_misalignment_and_length(ctx, shift):
    """Each of the 8 source misalignments with every length; `shift` 1-base ranges in front move every range's output offset by that many bytes, so each
    length starts at an odd and an even byte and at each place inside an output dword."""
    rng = np.random.default_rng(40 + shift)
    src = _bases(rng, 8 * 80 * len(LENGTHS) + 8 * sum(LENGTHS))
    ranges = [(3, 1)] * shift
    at = 0
    for mis in range(8):
        for ln in LENGTHS:
            at = (at + 63) // 64 * 64 + mis
            ranges.append((at, ln))
            at += ln
    assert at <= len(src)
    raw = _pack_run(ctx, src, ranges)
    assert len(raw) == shift + 8 * sum((ln + 1) // 2 for ln in LENGTHS)


def test_pack_seq_all_byte_values_and_small_ranges(ctx):
    rng = np.random.default_rng(5)
    src = np.concatenate([np.arange(256, dtype=np.uint8), np.arange(255, -1, -1, dtype=np.uint8), _bases(rng, 4000)])
    raw = _pack_run(ctx, src, [(0, 256), (256, 256), (1, 255), (0, 512)])
    assert raw[:128] == bytes((int(TAB[2 * i]) << 4) | int(TAB[2 * i + 1]) for i in range(128))
    codes = {c: raw[ord(c) // 2] >> 4 if ord(c) % 2 == 0 else raw[ord(c) // 2] & 15 for c in NT16 + NT16.lower() + "U0@\n"}
    assert [codes[c] for c in NT16] == list(range(16)) and [codes[c] for c in NT16.lower()] == list(range(16)) and [codes[c] for c in "U0@\n"] == [15] * 4
    # n = 0 and 1, runs of empty ranges, a thousand 1- and 2-base ranges
    assert _pack_run(ctx, src, []) == b""
    assert len(_pack_run(ctx, src, [(700, 5)])) == 3
    assert _pack_run(ctx, src, [(9, 0)] * 70) == b""
    _pack_run(ctx, src, [(5, 0)] * 3 + [(600, 9)] + [(0, 0)] * 130 + [(601, 8), (2, 0)])
    small = [(512 + int(a), 1 + int(k)) for a, k in zip(rng.integers(0, 3990, 1000), rng.integers(0, 2, 1000))]
    assert len(_pack_run(ctx, src, small)) == 1000
    # a range that leaves the array is not read: its bases are N
    assert _pack_run(ctx, src, [(len(src) - 3, 4), (len(src) - 3, 3), (1 << 40, 5)])[:2] == b"\xff\xff"


# ---- QUAL -------------------------------------------------------------------------------------------------------------------------------------------------
def _phred_expect(quals, read, pos, ln):
    q = quals[read] if read < len(quals) else None
    if q is None or q == b"*" or pos + ln > len(q):
        return b"\xff" * ln
    return bytes(v - 33 for v in q[pos:pos + ln])


def _phred_run(ctx, quals, reqs, no_quals=False):
    from lra_amd import bam
    n = len(reqs)
    off = np.zeros(len(quals) + 1, np.int64)
    off[1:] = np.cumsum([len(q) if q is not None else 0 for q in quals])
    flat = np.frombuffer(b"".join(q for q in quals if q is not None) + b"\0" * 64, np.uint8)
    d_q, d_off = (None, None) if no_quals else (_dev(ctx, flat, np.uint8), _dev(ctx, off, np.int64))
    d_req = _dev(ctx, np.asarray([(r, p, ln, 0) for r, p, ln in reqs], np.uint32).reshape(-1, 4), np.int32)
    res, raw = _guarded(ctx, lambda: bam.bam_phred_batch(ctx, d_req, len(quals), d_q, d_off, raw=True), lambda r: r.d_data, lambda r: r.n_bytes)
    o = ctx.to_host(res.d_off, n + 1, np.uint64)
    exp = [_phred_expect([None] * len(quals) if no_quals else quals, *r) for r in reqs]
    assert [int(x) for x in o] == [0] + [int(x) for x in np.cumsum([len(e) for e in exp])]
    for i, e in enumerate(exp):
        assert raw[int(o[i]):int(o[i + 1])] == e, (i, reqs[i])
    return raw


def test_phred_lengths_and_places(ctx):
    rng = np.random.default_rng(8)
    quals = [bytes(rng.integers(33, 127, ln + 3 * (i & 3)).astype(np.uint8)) for i, ln in enumerate(LENGTHS)]
    quals += [b"", b"*", None, b"!" * 70, b"~" * 70, b"*" + bytes(rng.integers(33, 127, 40).astype(np.uint8))]
    nq = len(quals)
    reqs = []
    for i, ln in enumerate(LENGTHS):                                            # inside the string at every source misalignment, at its end, one byte past it, wholly outside
        L = len(quals[i])
        reqs += [(i, 0, ln), (i, L - ln, ln), (i, L - ln + 1, ln), (i, L + 5, ln), (i, 0, L), (i, 0, L + 1)]
        reqs += [(i, k, max(ln - k, 0)) for k in range(1, 4)]
    e, s, none, lo, hi, lead = range(len(LENGTHS), nq)
    reqs += [(e, 0, 0), (e, 0, 4), (s, 0, 1), (s, 0, 9), (none, 0, 6), (lo, 0, 70), (hi, 3, 67), (lead, 0, 41), (lead, 0, 1), (nq, 0, 5), (0xffffffff, 0, 12)]
    raw = _phred_run(ctx, quals, reqs)
    assert b"\x00" * 70 in raw and bytes([93]) * 67 in raw                      # the values 33 and 126
    for shift in (1, 2, 3):                                                     # every request at each place inside an output dword
        _phred_run(ctx, quals, [(lo, 0, 1)] * shift + reqs)
    assert set(_phred_run(ctx, quals, reqs, no_quals=True)) <= {0xff}


def test_phred_small_batches(ctx):
    quals = [b"5" * 100, b"I" * 3]
    assert _phred_run(ctx, quals, []) == b""
    assert _phred_run(ctx, quals, [(1, 1, 2)]) == bytes([40, 40])
    assert _phred_run(ctx, quals, [(0, 0, 0)] * 70) == b""
    rng = np.random.default_rng(2)
    _phred_run(ctx, quals, [(0, int(p), 1 + int(k)) for p, k in zip(rng.integers(0, 99, 1000), rng.integers(0, 2, 1000))])
