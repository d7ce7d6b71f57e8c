"""lra_pack_strings_batch against a numpy gather: strings that lie anywhere in a source buffer (a NUL behind each, as the device readers' c_qual has),
packed back to back into a destination that sits inside a larger buffer of guard bytes."""
import ctypes as C

import numpy as np
import pytest

GUARD = 0xA5
PAD = 64                                # guard bytes on either side of d_dst


def _pack(ctx, lens, src_mis=0, dst_mis=0, shuffle=False, seed=0):
    """Lay the strings out (source order shuffled or not), run the primitive, check the output and the guards; -> the packed bytes."""
    import torch
    rng = np.random.default_rng(seed)
    n = len(lens)
    lens = np.asarray(lens, np.int64)
    order = rng.permutation(n) if shuffle else np.arange(n)
    pos = np.zeros(n, np.uint64)
    parts, at = [bytes(src_mis)], src_mis
    strings = [None] * n
    for i in order:                                                       # string i, then its NUL slot
        s = rng.integers(1, 256, int(lens[i])).astype(np.uint8).tobytes()
        strings[i] = s
        pos[i] = at
        parts.append(s + b"\0")
        at += len(s) + 1
    src = np.frombuffer(b"".join(parts) + bytes(8), np.uint8).copy()
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    total = int(off[n])
    exp = b"".join(strings)
    assert len(exp) == total and b"\0" not in exp
    d_src = torch.from_numpy(src).to(ctx.device)
    d_pos = torch.from_numpy(pos.view(np.int64)).to(ctx.device)
    d_off = torch.from_numpy(off.view(np.int64)).to(ctx.device)
    buf = torch.full((PAD + dst_mis + total + PAD,), GUARD, dtype=torch.uint8, device=ctx.device)
    assert buf.data_ptr() % 4 == 0 and d_src.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    ctx.check(ctx.lib.lra_pack_strings_batch(ctx.h, C.c_uint64(n), C.c_void_p(d_src.data_ptr()), C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_off.data_ptr()),
                                             C.c_void_p(buf.data_ptr() + PAD + dst_mis)))
    out = buf.cpu().numpy()
    lo = PAD + dst_mis
    assert (out[:lo] == GUARD).all(), "bytes in front of d_dst were written"
    assert (out[lo + total:] == GUARD).all(), "bytes behind d_dst[d_dst_off[n]) were written"
    got = out[lo:lo + total].tobytes()
    if got != exp:
        k = next(i for i in range(total) if got[i] != exp[i])
        raise AssertionError("first difference at byte %d of %d (string %d): %r / %r" % (k, total, int(np.searchsorted(off, k, "right")) - 1, got[k:k + 16], exp[k:k + 16]))
    assert b"\0" not in got                                               # no NUL slot reaches the output
    return got


def _edge_lengths():
    from lra_amd.reads_io import PACK_CHUNK
    return list(range(10)) + [63, 64, 65, 255, 256, 257, PACK_CHUNK - 1, PACK_CHUNK, PACK_CHUNK + 1, 3 * PACK_CHUNK + 123]


@pytest.mark.gpu
@pytest.mark.parametrize("src_mis", range(4))
@pytest.mark.parametrize("dst_mis", range(4))
def test_every_length_class_at_every_misalignment(ctx, src_mis, dst_mis):
    lens = _edge_lengths()
    _pack(ctx, lens, src_mis, dst_mis, seed=4 * src_mis + dst_mis)
    _pack(ctx, lens[::-1], src_mis, dst_mis, shuffle=True, seed=16 + 4 * src_mis + dst_mis)   # the source in another order than the output
    for L in (1, 2, 3, 5, 64, 4097):                                       # one string: its own misalignments are exactly these
        _pack(ctx, [L], src_mis, dst_mis, seed=L)


@pytest.mark.gpu
def test_runs_of_empty_strings(ctx):
    from lra_amd.reads_io import PACK_CHUNK
    _pack(ctx, [0] * 5 + [7, 300] + [0] * 9 + [PACK_CHUNK + 904, 1] + [0] * 4, 1, 3)
    _pack(ctx, [0] * 70 + [PACK_CHUNK] + [0] * 70 + [PACK_CHUNK] + [0] * 70, 2, 0)   # empties exactly at chunk borders
    _pack(ctx, [0, 0, 0])                                                  # nothing to write at all
    _pack(ctx, [0])
    _pack(ctx, [0, 1, 0], 3, 1)


@pytest.mark.gpu
def test_n_zero_and_n_one(ctx):
    import torch
    ctx.check(ctx.lib.lra_pack_strings_batch(ctx.h, C.c_uint64(0), None, None, None, None))
    buf = torch.full((128,), GUARD, dtype=torch.uint8, device=ctx.device)
    ctx.check(ctx.lib.lra_pack_strings_batch(ctx.h, C.c_uint64(0), C.c_void_p(buf.data_ptr()), None, None, C.c_void_p(buf.data_ptr() + 64)))
    assert (buf.cpu().numpy() == GUARD).all()
    for L in (0, 1, 4, 4096, 10_000):
        _pack(ctx, [L], 1, 2, seed=L)


@pytest.mark.gpu
def test_thousands_of_one_byte_strings_share_chunks(ctx):
    got = _pack(ctx, [1] * 6000, 1, 1, seed=9)
    assert len(got) == 6000
    rng = np.random.default_rng(5)
    _pack(ctx, rng.integers(0, 3, 9000).tolist(), 0, 3, shuffle=True, seed=10)   # 0, 1 and 2 bytes, scattered in the source


@pytest.mark.gpu
def test_first_offset_must_be_zero(ctx):
    import torch
    off = torch.tensor([4, 8], dtype=torch.int64, device=ctx.device)
    pos = torch.tensor([0], dtype=torch.int64, device=ctx.device)
    buf = torch.full((128,), GUARD, dtype=torch.uint8, device=ctx.device)
    rc = ctx.lib.lra_pack_strings_batch(ctx.h, C.c_uint64(1), C.c_void_p(buf.data_ptr()), C.c_void_p(pos.data_ptr()), C.c_void_p(off.data_ptr()), C.c_void_p(buf.data_ptr() + 64))
    assert rc != 0 and (buf.cpu().numpy() == GUARD).all()
