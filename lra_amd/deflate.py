"""BGZF deflate (deflate.hip): members from lra_bgzf_deflate_host / lra_bgzf_deflate_batch and the stream stage lra_bgzf_compress_device."""
import ctypes as C

import numpy as np

from ._lib import load_library

IN_MAX = 65280          # LRA_BGZF_IN_MAX: bytes of data per member
SLOT = 65536            # LRA_BGZF_SLOT: bytes a member may take


def member_table(datas):
    """list of bytes -> (the data back to back as uint8, in_off[n + 1] as uint64)"""
    off = np.zeros(len(datas) + 1, np.uint64)
    if datas:
        off[1:] = np.cumsum([len(d) for d in datas], dtype=np.uint64)
    return np.frombuffer(b"".join(datas), np.uint8).copy(), off


def deflate_members(datas, ctx=None):
    """One BGZF member per item of `datas` (bytes, at most IN_MAX each) -> (members, status): members[i] is the member's bytes, None where status[i] != 0.
    ctx None: lra_bgzf_deflate_host; a Context: lra_bgzf_deflate_batch on its device.  Both give the same bytes."""
    lib = load_library()
    n = len(datas)
    buf, off = member_table(datas)
    if ctx is None:
        out, out_len, status = np.zeros(max(n, 1) * SLOT, np.uint8), np.zeros(max(n, 1), np.uint32), np.full(max(n, 1), -1, np.int32)
        rc = lib.lra_bgzf_deflate_host(n, buf.ctypes.data, off.ctypes.data, out.ctypes.data, out_len.ctypes.data, status.ctypes.data)
        if rc != 0:
            raise ValueError("lra_bgzf_deflate_host: %d" % rc)
    else:
        import torch
        dev = lambda a: torch.from_numpy(a.view(np.uint8)).to(ctx.device)
        t_in, t_off = dev(np.concatenate([buf, np.zeros(1, np.uint8)])), dev(off)
        t_out = torch.zeros(max(n, 1) * SLOT, dtype=torch.uint8, device=ctx.device)
        t_len, t_st = dev(np.zeros(max(n, 1), np.uint32)), dev(np.full(max(n, 1), -1, np.int32))
        ctx.check(lib.lra_bgzf_deflate_batch(ctx.h, n, t_in.data_ptr(), t_off.data_ptr(), t_out.data_ptr(), t_len.data_ptr(), t_st.data_ptr()))
        out, out_len, status = t_out.cpu().numpy(), t_len.cpu().numpy().view(np.uint32), t_st.cpu().numpy().view(np.int32)
    members = [out[i * SLOT:i * SLOT + int(out_len[i])].tobytes() if status[i] == 0 else None for i in range(n)]
    return members, status[:n].copy()


def compress_result(lib, ctx, rc, data, data_len, moff, n_members):
    """the context-owned result of a compress call -> (bytes, member_off as uint64[n_members + 1]), copied"""
    ctx.check(rc)
    n = int(n_members.value)
    off = np.ctypeslib.as_array(C.cast(moff, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
    return (C.string_at(data, int(data_len.value)) if data_len.value else b""), off


def compress_device(ctx, text, length=None, round_members=None):
    """lra_bgzf_compress_device: text -- bytes, a uint8 numpy array (uploaded) or a uint8 tensor on ctx's device, or a raw device address with `length` --
    cut every IN_MAX bytes -> (the members back to back as bytes, member_off[n_members + 1]).  No EOF member is appended.
    round_members: members per round of the stage (None: leave as it is; 0: the default)."""
    import torch
    lib = ctx.lib
    if isinstance(text, (bytes, bytearray, memoryview)):
        text = np.frombuffer(bytes(text), np.uint8)
    if isinstance(text, np.ndarray):
        text = torch.from_numpy(np.concatenate([text.view(np.uint8), np.zeros(1, np.uint8)])).to(ctx.device)[:-1]
    if isinstance(text, torch.Tensor):
        keep, addr, length = text, text.data_ptr(), text.numel()
    else:
        keep, addr = None, int(text)
    if round_members is not None:
        ctx.check(lib.lra_bgzf_compress_set_round(ctx.h, int(round_members)))
    data, data_len, moff, n_members = C.c_void_p(), C.c_uint64(0), C.c_void_p(), C.c_uint64(0)
    rc = lib.lra_bgzf_compress_device(ctx.h, C.c_void_p(addr), C.c_uint64(length), C.byref(data), C.byref(data_len), C.byref(moff), C.byref(n_members))
    del keep
    return compress_result(lib, ctx, rc, data, data_len, moff, n_members)


def compress_stats(ctx):
    """(wall ms, output bytes) of the context's last compress call"""
    ms, nb = C.c_double(0), C.c_uint64(0)
    ctx.check(ctx.lib.lra_bgzf_compress_stats(ctx.h, C.byref(ms), C.byref(nb)))
    return ms.value, int(nb.value)
