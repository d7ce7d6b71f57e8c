"""The device primitives behind BAM output (bam_encode.hip): an alignment's CIGAR as BAM ops, ranges of bases as 4-bit codes, ranges of quality strings
as phred bytes.  Inputs are device tensors; results are copied to numpy."""
import ctypes as C

import numpy as np

from .context import Context

NT16 = "=ACMGRSVTWYHKDBN"


class BamCigarResult(C.Structure):
    """lra_bam_cigar_result (include/lra_hip.h)"""
    _fields_ = [("n_aln", C.c_int32), ("n_ops", C.c_uint64), ("d_off", C.c_void_p), ("d_ops", C.c_void_p)]


class BamBytesResult(C.Structure):
    """lra_bam_bytes_result (include/lra_hip.h)"""
    _fields_ = [("n", C.c_uint64), ("n_bytes", C.c_uint64), ("d_off", C.c_void_p), ("d_data", C.c_void_p)]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def bam_cigar_batch(ctx: Context, runs, run_off, pre_clip=None, suf_clip=None, clip_op=None, raw=False):
    """lra_bam_cigar_batch: arguments as refine.cigar_text_batch -> one uint32 array of BAM ops per alignment; raw=True: the BamCigarResult."""
    n = int(run_off.numel()) - 1
    res = BamCigarResult()
    q = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ctx.check(ctx.lib.lra_bam_cigar_batch(ctx.h, n, _p(runs), q(run_off), q(pre_clip), q(suf_clip), q(clip_op), C.byref(res)))
    if raw:
        return res
    off = ctx.to_host(res.d_off, n + 1, np.uint64) if n else np.zeros(1, np.uint64)
    ops = ctx.to_host(res.d_ops, int(res.n_ops), np.uint32) if int(res.n_ops) else np.zeros(0, np.uint32)
    return [ops[int(off[i]):int(off[i + 1])] for i in range(n)]


def _split(ctx, res, n):
    off = ctx.to_host(res.d_off, n + 1, np.uint64) if n else np.zeros(1, np.uint64)
    data = ctx.to_host(res.d_data, int(res.n_bytes), np.uint8).tobytes() if int(res.n_bytes) else b""
    return [data[int(off[i]):int(off[i + 1])] for i in range(n)]


def bam_pack_seq_batch(ctx: Context, ranges, src, raw=False):
    """lra_bam_pack_seq_batch: ranges = uint64 tensor [n, 2] of (offset, length) into the uint8 tensor src -> the packed bytes of every range."""
    n = int(ranges.shape[0]) if ranges is not None else 0
    res = BamBytesResult()
    ctx.check(ctx.lib.lra_bam_pack_seq_batch(ctx.h, C.c_uint64(n), _p(ranges), _p(src), C.c_uint64(int(src.numel()) if src is not None else 0), C.byref(res)))
    return res if raw else _split(ctx, res, n)


def bam_phred_batch(ctx: Context, reqs, n_reads, qual, qual_off, raw=False):
    """lra_bam_phred_batch: reqs = uint32 tensor [n, 4] of (read, pos, len, 0) over the quality strings qual (uint8 tensor) / qual_off (uint64 [n_reads + 1];
    both None: no qualities) -> len bytes per request."""
    n = int(reqs.shape[0]) if reqs is not None else 0
    res = BamBytesResult()
    ctx.check(ctx.lib.lra_bam_phred_batch(ctx.h, C.c_uint64(n), _p(reqs), int(n_reads), C.c_void_p(qual.data_ptr()) if qual is not None else None,
                                          C.c_void_p(qual_off.data_ptr()) if qual_off is not None else None, C.byref(res)))
    return res if raw else _split(ctx, res, n)
