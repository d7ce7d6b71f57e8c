"""lra_bgzf_deflate_batch (deflate.hip's kernel) against lra_bgzf_deflate_host: the same batch of edge members byte for byte, whatever the members' order and
the input's alignment; the two inflate kernels read the members back; lra_bgzf_compress_device over texts of several rounds."""
import gzip

import numpy as np
import pytest

from lra_amd import bgzf
from lra_amd.deflate import compress_device
import bgzf_deflate_cases as K

pytestmark = pytest.mark.gpu


def _run_device(ctx, datas, shift=0, order=None):
    """the batch in `order` with the input `shift` bytes into a buffer of 0xab -> (out, out_len, status) in the order of `datas`, sentinels checked"""
    import torch
    n = len(datas)
    order = list(range(n)) if order is None else order
    body = b"".join(datas[i] for i in order)
    buf = np.full(256 + shift + len(body) + 64, 0xab, np.uint8)
    buf[256 + shift:256 + shift + len(body)] = np.frombuffer(body, np.uint8)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(datas[i]) for i in order], dtype=np.uint64)
    dev = lambda a: torch.from_numpy(a.view(np.uint8)).cuda()
    t_in, t_off = dev(buf), dev(off)
    t_out, t_len, t_st = dev(np.full(64 + n * K.SLOT + 64, 0xab, np.uint8)), dev(np.full(n, 0xffffffff, np.uint32)), dev(np.full(n, -1, np.int32))
    ctx.check(ctx.lib.lra_bgzf_deflate_batch(ctx.h, n, t_in.data_ptr() + 256 + shift, t_off.data_ptr(), t_out.data_ptr() + 64, t_len.data_ptr(), t_st.data_ptr()))
    out, ln, st = t_out.cpu().numpy(), t_len.cpu().numpy().view(np.uint32), t_st.cpu().numpy().view(np.int32)
    assert np.array_equal(t_in.cpu().numpy(), buf)
    assert (out[:64] == 0xab).all() and (out[-64:] == 0xab).all()
    out = out[64:-64]
    K.check_sentinels(out, ln, st)
    members = K.members_of(out, ln, st)
    back = [None] * n
    for k, i in enumerate(order):
        back[i] = (members[k], int(ln[k]), int(st[k]))
    return back


@pytest.fixture(scope="module")
def host_edge():
    items = K.edge_members()
    out, out_len, status = K.run_host([d for _, d in items])
    return items, [(m, int(l), int(s)) for m, l, s in zip(K.members_of(out, out_len, status), out_len, status)]


def _same(items, got, want, what):
    for (name, _), g, w in zip(items, got, want):
        assert g[2] == w[2], (what, name, g[2], w[2])
        if w[2] == 0:
            assert g[1] == w[1] and g[0] == w[0], (what, name, g[1], w[1])
        else:
            assert g[0] is None


def test_batch_equals_host(ctx, host_edge):
    items, want = host_edge
    assert sum(1 for _, _, s in want if s != 0) == 1
    _same(items, _run_device(ctx, [d for _, d in items]), want, "as is")


def test_order_and_alignment_do_not_change_a_member(ctx, host_edge):
    items, want = host_edge
    datas = [d for _, d in items]
    n = len(datas)
    _same(items, _run_device(ctx, datas, 0, list(range(n))[::-1]), want, "reversed")
    for shift in range(1, 16):                               # every misalignment of the input, the whole batch, in alternating order
        order = list(range(n)) if shift & 1 else list(range(n))[::-1]
        _same(items, _run_device(ctx, datas, shift, order), want, "shift %d" % shift)


def test_inflate_kernels_read_the_members_back(ctx, host_edge):
    import torch
    items, _ = host_edge
    good = [(name, d) for name, d in items if len(d) <= K.IN_MAX]
    got = _run_device(ctx, [d for _, d in good])
    members = [m for m, _, _ in got]
    n = len(members)
    comp = np.frombuffer(b"".join(members), np.uint8).copy()
    io_ = np.zeros(n + 1, np.uint64); io_[1:] = np.cumsum([len(m) for m in members], dtype=np.uint64)
    oo = np.zeros(n + 1, np.uint64); oo[1:] = np.cumsum([len(d) for _, d in good], dtype=np.uint64)
    dev = lambda a: torch.from_numpy(a.view(np.uint8)).cuda()
    t_in, t_io, t_oo = dev(np.concatenate([comp, np.zeros(64, np.uint8)])), dev(io_), dev(oo)
    for fn in (ctx.lib.lra_bgzf_inflate_batch, ctx.lib.lra_bgzf_inflate_lut_batch):
        t_out, t_st = torch.zeros(int(oo[-1]) + 64, dtype=torch.uint8, device="cuda"), dev(np.full(n, -1, np.int32))
        ctx.check(fn(ctx.h, n, t_in.data_ptr(), t_io.data_ptr(), t_oo.data_ptr(), t_out.data_ptr(), t_st.data_ptr()))
        assert (t_st.cpu().numpy().view(np.int32) == 0).all()
        assert t_out.cpu().numpy()[:int(oo[-1])].tobytes() == b"".join(d for _, d in good)


def _check_stream(text, data, off):
    n = (len(text) + K.IN_MAX - 1) // K.IN_MAX
    assert len(off) == n + 1 and off[0] == 0 and off[-1] == len(data)
    in_off, out_off = bgzf.blocks(data)
    assert in_off == [int(x) for x in off]
    assert out_off == [min(len(text), i * K.IN_MAX) for i in range(n + 1)]
    assert gzip.decompress(data + bgzf.EOF_BLOCK) == text


def test_compress_device_texts_equal_host_members(ctx):
    for text in (K.sam_like(), K.paf_like(), K.repetitive()):
        data, off = compress_device(ctx, text, round_members=0)
        _check_stream(text, data, off)
        o, ln, st = K.run_host(K.cut(text))
        assert data == b"".join(K.members_of(o, ln, st))


def test_compress_device_lengths(ctx):
    sam = K.sam_like()
    for n in (0, 1, 65280, 65281, 3 * 65280):
        data, off = compress_device(ctx, sam[:n], round_members=0)
        _check_stream(sam[:n], data, off)
    data, off = compress_device(ctx, sam[:3 * 65280], round_members=2)          # a round of two and a round of one
    _check_stream(sam[:3 * 65280], data, off)


def test_compress_device_several_rounds(ctx):
    text = (K.sam_like() + K.paf_like() + K.repetitive()) * 8                    # 14 MB, 217 members, in rounds of 50
    whole, off0 = compress_device(ctx, text, round_members=0)
    data, off = compress_device(ctx, text, round_members=50)
    assert len(off) - 1 > 200 and data == whole and np.array_equal(off, off0)
    _check_stream(text, data, off)
    compress_device(ctx, b"", round_members=0)                                  # the default again for whoever uses the context next
