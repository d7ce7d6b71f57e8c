"""lra_cigar_text_batch: the CIGAR kernel on crafted runs, against strings formatted here from the same arrays."""
import numpy as np
import pytest

OPS = "=XID"
EDGES = [1, 9, 10, 99, 100, 999, 1000, 9999, 10_000, 99_999, 100_000, 999_999, 1_000_000, 9_999_999, 10_000_000, 99_999_999, 100_000_000, (1 << 28) - 1]
GUARD = 0xA5


def _expect(runs, pre, suf, op):
    s = ("%d%s" % (pre, op) if pre > 0 else "") + "".join("%d%s" % (int(r) >> 4, OPS[int(r) & 15]) for r in runs) + ("%d%s" % (suf, op) if suf > 0 else "")
    return s.encode()


def _run(ctx, lists, pre=None, suf=None, op=None):
    """-> (texts, raw result, the bytes behind the text) with a guard pattern laid behind the result's text before the call."""
    import torch
    from lra_amd import refine
    n = len(lists)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, np.uint32) for x in lists]) if off[-1] else np.zeros(0, np.uint32)
    dev = ctx.device
    t = lambda a, dt: None if a is None else torch.from_numpy(np.asarray(a, dt)).to(dev)
    d_runs = torch.from_numpy(flat.view(np.int32).copy()).to(dev) if len(flat) else None
    d_off = torch.from_numpy(off).to(dev)
    args = (d_runs, d_off, t(pre, np.int32), t(suf, np.int32), t(None if op is None else [ord(c) for c in op], np.uint8))
    r0 = refine.cigar_text_batch(ctx, *args, raw=True)                    # sizes the context's buffers; then the guard goes behind the text
    nb = int(r0.n_bytes)
    guard = torch.full((48,), GUARD, dtype=torch.uint8, device=dev)
    import ctypes as C
    ctx.check(ctx.lib.lra_copy_device(ctx.h, C.c_void_p(r0.d_text + nb), C.c_void_p(guard.data_ptr()), C.c_uint64(48)))
    torch.cuda.synchronize()
    res = refine.cigar_text_batch(ctx, *args, raw=True)
    assert int(res.n_bytes) == nb and int(res.n_aln) == n and res.d_text == r0.d_text
    o = ctx.to_host(res.d_off, n + 1, np.uint64) if n else np.zeros(1, np.uint64)
    raw = ctx.to_host(res.d_text, nb + 48, np.uint8).tobytes()
    assert raw[nb:] == bytes([GUARD]) * 48, "bytes behind the last offset were written"
    assert int(o[0]) == 0 and int(o[-1]) == nb
    return [raw[int(o[i]):int(o[i + 1])] for i in range(n)]


def _runs(rng, n):
    ln = rng.choice(np.asarray(EDGES + [2, 3, 5, 12, 47], np.int64), n)
    return ((ln << 4) | rng.integers(0, 4, n)).astype(np.uint32)


@pytest.mark.gpu
def test_every_decimal_width_and_op(ctx):
    lists = [[(v << 4) | k for v in EDGES] for k in range(4)] + [[(v << 4) | (i & 3)] for i, v in enumerate(EDGES)]
    got = _run(ctx, lists)
    assert got == [_expect(x, 0, 0, "S") for x in lists]
    assert got[0].startswith(b"1=9=10=99=100=") and got[3].endswith(b"100000000D268435455D")


@pytest.mark.gpu
@pytest.mark.parametrize("shuffled", [False, True])
def test_alignment_sizes_in_one_batch(ctx, shuffled):
    """0, 1, 63, 64, 65, 4095, 4096, 4097 runs, and around the launch's 256 lanes per workgroup (the runs are cut one per lane: 255, 256, 257)."""
    rng = np.random.default_rng(5)
    sizes = [0, 1, 63, 64, 65, 4095, 4096, 4097, 255, 256, 257, 0]
    if shuffled:
        sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    lists = [_runs(rng, n) for n in sizes]
    assert _run(ctx, lists) == [_expect(x, 0, 0, "S") for x in lists]
    pre = [int(x) for x in rng.choice([0, 7, 10, 12345], len(sizes))]
    suf = [int(x) for x in rng.choice([0, 9, 100, 99999], len(sizes))]
    op = "".join(rng.choice(["S", "H"], len(sizes)))
    assert _run(ctx, lists, pre, suf, op) == [_expect(x, p, s, c) for x, p, s, c in zip(lists, pre, suf, op)]


@pytest.mark.gpu
def test_clips(ctx):
    rng = np.random.default_rng(9)
    edge = [1, 9, 10, 99, 100, 999, 1000, 99_999, 100_000, 999_999_999, 1_000_000_000, 2_147_483_647]
    lists = [_runs(rng, 1 + i % 5) for i in range(len(edge))]
    n = len(lists)
    zero = [0] * n
    for pre, suf in ((edge, None), (None, edge), (edge, edge[::-1]), (zero, zero), (edge, zero), ([-3] * n, edge)):
        for op in (None, "S" * n, "H" * n, ("SH" * n)[:n]):
            got = _run(ctx, lists, pre, suf, op)
            exp = [_expect(x, (pre or zero)[i], (suf or zero)[i], (op or "S" * n)[i]) for i, x in enumerate(lists)]
            assert got == exp, (pre, suf, op)
    # clips around alignments without runs
    assert _run(ctx, [[], [], []], [5, 0, 0], [0, 0, 12], "HSH") == [b"5H", b"", b"12H"]


@pytest.mark.gpu
def test_empty_batch(ctx):
    assert _run(ctx, []) == []
    assert _run(ctx, [[]]) == [b""]
