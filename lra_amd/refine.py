"""Host-side mirror of IndelRefineAlignment (reference: IndelRefine.h:53) for a batch of alignments."""
import ctypes as C

import numpy as np
import torch

from .context import Context, ptr


class RefineResult(C.Structure):
    _fields_ = [("n_aln", C.c_int32), ("n_blocks", C.c_uint64), ("n_segments", C.c_uint64), ("n_rows", C.c_uint64),
                ("n_cells", C.c_uint64), ("n_aog", C.c_uint64), ("d_block_off", C.c_void_p), ("d_blocks", C.c_void_p),
                ("d_status", C.c_void_p)]


class RefineBatch:
    """Device-resident inputs: per alignment its blocks, the read strand it lies on and its chromosome."""

    def __init__(self, ctx: Context, blocks_list, q_seq_dev, q_off, q_len, t_seq_dev, t_off, t_len):
        self.ctx = ctx
        self.n = len(blocks_list)
        nb = np.fromiter((len(b) for b in blocks_list), dtype=np.int64, count=self.n)
        boff = np.zeros(self.n + 1, dtype=np.int64)
        boff[1:] = np.cumsum(nb)
        flat = (np.concatenate([np.asarray(b, dtype=np.int32).reshape(-1, 3) for b in blocks_list]) if boff[-1]
                else np.zeros((0, 3), np.int32))
        dev = ctx.device
        self.n_blocks_in = int(boff[-1])
        self.blocks = torch.from_numpy(np.ascontiguousarray(flat).reshape(-1)).to(dev) if boff[-1] else torch.zeros(3, dtype=torch.int32, device=dev)
        self.block_off = torch.from_numpy(boff).to(dev)
        self.q_seq, self.t_seq = q_seq_dev, t_seq_dev
        self.q_off = torch.from_numpy(np.asarray(q_off, dtype=np.int64)).to(dev)
        self.q_len = torch.from_numpy(np.asarray(q_len, dtype=np.int32)).to(dev)
        self.t_off = torch.from_numpy(np.asarray(t_off, dtype=np.int64)).to(dev)
        self.t_len = torch.from_numpy(np.asarray(t_len, dtype=np.int64)).to(dev)


def refine_batch_from_device(ctx, blocks, block_off, q_seq, q_off, q_len, t_seq, t_off, t_len):
    """RefineBatch whose inputs already are device tensors (blocks int32 [nb,3], CSR offsets int64)."""
    b = RefineBatch.__new__(RefineBatch)
    b.ctx, b.n = ctx, int(block_off.numel()) - 1
    b.n_blocks_in = int(blocks.shape[0])
    b.blocks = blocks.to(torch.int32).contiguous().reshape(-1)
    b.block_off = block_off.to(torch.int64).contiguous()
    b.q_seq, b.t_seq = q_seq, t_seq
    b.q_off, b.q_len = q_off.to(torch.int64).contiguous(), q_len.to(torch.int32).contiguous()
    b.t_off, b.t_len = t_off.to(torch.int64).contiguous(), t_len.to(torch.int64).contiguous()
    return b


def indel_refine_batch(ctx: Context, b: RefineBatch, refine_band, match, mismatch, indel, end_align=False):
    res = RefineResult()
    ctx.check(ctx.lib.lra_indel_refine_batch(ctx.h, b.n, ptr(b.blocks), ptr(b.block_off), C.c_uint64(b.n_blocks_in), ptr(b.q_seq),
                                             ptr(b.q_off), ptr(b.q_len), ptr(b.t_seq), ptr(b.t_off), ptr(b.t_len), refine_band,
                                             match, mismatch, indel, 1 if end_align else 0, C.byref(res)))
    return res


def fetch(ctx: Context, res: RefineResult):
    off = ctx.to_host(res.d_block_off, res.n_aln + 1, np.uint64)
    blocks = ctx.to_host(res.d_blocks, 3 * res.n_blocks, np.int32).reshape(-1, 3)
    status = ctx.to_host(res.d_status, res.n_aln, np.int32)
    return [blocks[int(off[a]):int(off[a + 1])] for a in range(res.n_aln)], status


class StatsResult(C.Structure):
    _fields_ = [("n_aln", C.c_int32), ("n_runs", C.c_uint64), ("d_counts", C.c_void_p), ("d_value", C.c_void_p),
                ("d_run_off", C.c_void_p), ("d_runs", C.c_void_p)]


class MdResult(C.Structure):
    """lra_md_result (include/lra_hip.h)"""
    _fields_ = [("n_aln", C.c_int32), ("n_bytes", C.c_uint64), ("d_md_off", C.c_void_p), ("d_md", C.c_void_p)]


def md_strings_batch(ctx: Context, b: RefineBatch):
    """lra_md_strings_batch: the MD:Z value (lra --printMD) of every alignment of a RefineBatch-shaped input, on the device -> one bytes object per alignment."""
    res = MdResult()
    ctx.check(ctx.lib.lra_md_strings_batch(ctx.h, b.n, ptr(b.blocks), ptr(b.block_off), ptr(b.q_seq), ptr(b.q_off), ptr(b.q_len), ptr(b.t_seq), ptr(b.t_off),
                                           C.byref(res)))
    return fetch_md(ctx, res)


def fetch_md(ctx: Context, res: MdResult):
    n = int(res.n_aln)
    off = ctx.to_host(res.d_md_off, n + 1, np.uint64) if n else np.zeros(1, np.uint64)
    raw = ctx.to_host(res.d_md, int(res.n_bytes), np.uint8).tobytes() if int(res.n_bytes) else b""
    return [raw[int(off[i]):int(off[i + 1])] for i in range(n)]


class CigarTextResult(C.Structure):
    """lra_cigar_text_result (include/lra_hip.h)"""
    _fields_ = [("n_aln", C.c_int32), ("n_bytes", C.c_uint64), ("d_off", C.c_void_p), ("d_text", C.c_void_p)]


def cigar_text_batch(ctx: Context, runs, run_off, pre_clip=None, suf_clip=None, clip_op=None, raw=False):
    """lra_cigar_text_batch: the CIGAR string of every alignment from its runs ((length << 4) | op; device tensors: runs int32 / uint32 bits, run_off int64
    [n + 1]) and optional per-alignment clips (int32) and clip ops (uint8 'S' / 'H') -> one bytes object per alignment; raw=True: the CigarTextResult."""
    n = int(run_off.numel()) - 1
    res = CigarTextResult()
    p = lambda t: ptr(t) if t is not None else None
    ctx.check(ctx.lib.lra_cigar_text_batch(ctx.h, n, p(runs) if runs is not None and runs.numel() else None, ptr(run_off), p(pre_clip), p(suf_clip), p(clip_op),
                                           C.byref(res)))
    if raw:
        return res
    off = ctx.to_host(res.d_off, n + 1, np.uint64) if n else np.zeros(1, np.uint64)
    text = ctx.to_host(res.d_text, int(res.n_bytes), np.uint8).tobytes() if int(res.n_bytes) else b""
    return [text[int(off[i]):int(off[i + 1])] for i in range(n)]


class AlnStringsResult(C.Structure):
    """lra_aln_strings_result (include/lra_hip.h)"""
    _fields_ = [("n_aln", C.c_int32), ("n_cols", C.c_uint64), ("d_col_off", C.c_void_p), ("d_ref_len", C.c_void_p), ("d_q", C.c_void_p), ("d_a", C.c_void_p),
                ("d_t", C.c_void_p)]


class PairwiseTextResult(C.Structure):
    """lra_pairwise_text_result (include/lra_hip.h)"""
    _fields_ = [("n_aln", C.c_int32), ("n_bytes", C.c_uint64), ("d_off", C.c_void_p), ("d_text", C.c_void_p)]


PAIRWISE_WIDTH = 50                 # columns per printed row (PrintPairwise)
PAIRWISE_GROUP_ROWS = 16            # pairwise.hip's PW_GROUP_ROWS: the rows one wave of the emit kernel stages in its LDS tile (the tests place alignments around it)


def alignment_strings_batch(ctx: Context, b: RefineBatch):
    """lra_alignment_strings_batch: CreateAlignmentStrings of every alignment of a RefineBatch-shaped input, on the device ->
    ([(query string, alignment string, text string) per alignment], ref_len uint32[n])."""
    res = AlnStringsResult()
    ctx.check(ctx.lib.lra_alignment_strings_batch(ctx.h, b.n, ptr(b.blocks), ptr(b.block_off), ptr(b.q_seq), ptr(b.q_off), ptr(b.q_len), ptr(b.t_seq), ptr(b.t_off),
                                                  C.byref(res)))
    n, nc = int(res.n_aln), int(res.n_cols)
    if not n:
        return [], np.zeros(0, np.uint32)
    off = ctx.to_host(res.d_col_off, n + 1, np.uint64)
    q, a, t = (ctx.to_host(p, nc, np.uint8).tobytes() if nc else b"" for p in (res.d_q, res.d_a, res.d_t))
    return [(q[int(off[i]):int(off[i + 1])], a[int(off[i]):int(off[i + 1])], t[int(off[i]):int(off[i + 1])]) for i in range(n)], ctx.to_host(res.d_ref_len, n, np.uint32)


def pairwise_text_batch(ctx: Context, b: RefineBatch, raw=False):
    """lra_pairwise_text_batch: the rows Alignment::PrintPairwise prints for every alignment of a RefineBatch-shaped input (everything behind the name and
    Interval lines), built on the device from the blocks -> one bytes object per alignment; raw=True: the PairwiseTextResult."""
    res = PairwiseTextResult()
    ctx.check(ctx.lib.lra_pairwise_text_batch(ctx.h, b.n, ptr(b.blocks), ptr(b.block_off), ptr(b.q_seq), ptr(b.q_off), ptr(b.q_len), ptr(b.t_seq), ptr(b.t_off),
                                              C.byref(res)))
    if raw:
        return res
    n = int(res.n_aln)
    off = ctx.to_host(res.d_off, n + 1, np.uint64) if n else np.zeros(1, np.uint64)
    text = ctx.to_host(res.d_text, int(res.n_bytes), np.uint8).tobytes() if int(res.n_bytes) else b""
    return [text[int(off[i]):int(off[i + 1])] for i in range(n)]


def md_of_refined(ctx: Context, b: RefineBatch, rres: RefineResult):
    """lra_md_strings_batch straight on the (context-owned) output of indel_refine_batch (the blocks CalculateStatistics saw)."""
    v = RefineBatch.__new__(RefineBatch)
    v.ctx, v.n, v.n_blocks_in = ctx, b.n, int(rres.n_blocks)
    v.blocks, v.block_off = int(rres.d_blocks), int(rres.d_block_off)
    v.q_seq, v.q_off, v.q_len, v.t_seq, v.t_off, v.t_len = b.q_seq, b.q_off, b.q_len, b.t_seq, b.t_off, b.t_len
    return md_strings_batch(ctx, v)


class SvSigRec(C.Structure):
    """lra_svsig_rec (include/lra_hip.h)"""
    _fields_ = [("seq_off", C.c_uint64), ("t_start", C.c_uint32), ("len", C.c_uint32), ("kind", C.c_uint32), ("block", C.c_uint32)]


class SvSigResult(C.Structure):
    """lra_svsig_result (include/lra_hip.h)"""
    _fields_ = [("n_aln", C.c_int32), ("n_sig", C.c_uint64), ("n_seq_bytes", C.c_uint64), ("d_sig_off", C.c_void_p), ("d_sig", C.c_void_p), ("d_seq", C.c_void_p)]


SV_INS, SV_DEL = 0, 1
SVSIG_PIECE = 1024                  # svsig.hip's SV_PIECE: the output bytes one wave of the copy kernel moves (the tests place sequence lengths around it)
SVSIG_REC = np.dtype([("seq_off", "<u8"), ("t_start", "<u4"), ("len", "<u4"), ("kind", "<u4"), ("block", "<u4")])


def sv_signatures_batch(ctx: Context, b: RefineBatch, min_len=25):
    """lra_sv_signatures_batch: the SV signatures (Alignment::Printsvsig) of every alignment of a RefineBatch-shaped input, on the device ->
    (sig_off uint64[n + 1], records as a SVSIG_REC array [n_sig], the sequence bytes): alignment a's records are [sig_off[a], sig_off[a + 1]), record
    x's bases are seq[seq_off, seq_off + len)."""
    res = SvSigResult()
    ctx.check(ctx.lib.lra_sv_signatures_batch(ctx.h, b.n, ptr(b.blocks), ptr(b.block_off), ptr(b.q_seq), ptr(b.q_off), ptr(b.q_len), ptr(b.t_seq), ptr(b.t_off),
                                              C.c_int32(int(min_len)), C.byref(res)))
    n, ns, nb = int(res.n_aln), int(res.n_sig), int(res.n_seq_bytes)
    off = ctx.to_host(res.d_sig_off, n + 1, np.uint64)
    recs = ctx.to_host(res.d_sig, ns * SVSIG_REC.itemsize, np.uint8).view(SVSIG_REC) if ns else np.zeros(0, SVSIG_REC)
    seq = ctx.to_host(res.d_seq, nb, np.uint8).tobytes() if nb else b""
    return off, recs, seq


class SvSigTextResult(C.Structure):
    """lra_svsig_text_result (include/lra_hip.h)"""
    _fields_ = [("n_aln", C.c_int32), ("n_sig", C.c_uint64), ("n_bytes", C.c_uint64), ("d_aln_off", C.c_void_p), ("d_text", C.c_void_p)]


SVSIG_TEXT_CHUNK = 4096             # svsig_text.hip's SVT_CHUNK: the output bytes one wave of its copy kernel moves


def name_table(ctx: Context, names):
    """A name table as lra_svsig_text_batch takes it: (the names back to back, uint64 offsets [n + 1]) as device tensors."""
    import torch
    off = np.zeros(len(names) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in names])
    blob = np.frombuffer(b"".join(names) + b"\0" * 8, np.uint8).copy()
    return torch.from_numpy(blob).to(ctx.device), torch.from_numpy(off).to(ctx.device)


def svsig_text_batch(ctx: Context, sv: SvSigResult, aln_read, chrom, read_names, chrom_names, skip=None):
    """lra_svsig_text_batch: the lines of the signatures `sv` holds (the result of lra_sv_signatures_batch, still alive on the context), on the device.
    aln_read / chrom / skip: per alignment its read, its chromosome and (optional) 1 to print nothing; the names as lists of bytes.
    -> (the text, aln_off uint64[n_aln + 1]): alignment a's lines are text[aln_off[a]:aln_off[a + 1]]."""
    import torch
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(ctx.device)
    d_read, d_chrom = dev(np.asarray(aln_read, np.uint32).view(np.int32), np.int32), dev(chrom, np.int32)
    d_skip = dev(skip, np.uint8) if skip is not None else None
    rn, ro = name_table(ctx, read_names)
    cn, co = name_table(ctx, chrom_names)
    res = SvSigTextResult()
    ctx.check(ctx.lib.lra_svsig_text_batch(ctx.h, C.byref(sv), ptr(d_read), ptr(d_chrom), ptr(d_skip) if d_skip is not None else None, len(read_names), ptr(rn), ptr(ro),
                                           len(chrom_names), ptr(cn), ptr(co), C.byref(res)))
    assert int(res.n_aln) == int(sv.n_aln) and int(res.n_sig) == int(sv.n_sig)
    off = ctx.to_host(res.d_aln_off, int(res.n_aln) + 1, np.uint64)
    text = ctx.to_host(res.d_text, int(res.n_bytes), np.uint8).tobytes() if res.n_bytes else b""
    return text, off


STAT_NAMES = ["nm", "nmm", "nins", "ndel", "tdel", "tins", "nSmallDel", "nMedDel", "nLargeDel", "nSmallIns", "nMedIns", "nLargeIns",
              "preClip", "sufClip", "qStart", "qEnd", "tStart", "tEnd"]


def calculate_statistics_batch(ctx: Context, b: RefineBatch, lookup_table):
    """Alignment::CalculateStatistics over the alignments of a RefineBatch-shaped input (blocks + sequences).
    lookup_table: float32[2001] = logf(1), logf(6), ... from the host libm."""
    lut = np.ascontiguousarray(lookup_table, dtype=np.float32)
    res = StatsResult()
    ctx.check(ctx.lib.lra_calculate_statistics_batch(ctx.h, b.n, ptr(b.blocks), ptr(b.block_off), ptr(b.q_seq), ptr(b.q_off), ptr(b.q_len),
                                                     ptr(b.t_seq), ptr(b.t_off), C.c_void_p(lut.ctypes.data), len(lut), C.byref(res)))
    return res


def fetch_stats(ctx: Context, res: StatsResult):
    counts = ctx.to_host(res.d_counts, 18 * res.n_aln, np.int32).reshape(-1, 18)
    value = ctx.to_host(res.d_value, res.n_aln, np.float32)
    off = ctx.to_host(res.d_run_off, res.n_aln + 1, np.uint64)
    runs = ctx.to_host(res.d_runs, res.n_runs, np.uint32)
    cigars = ["".join("%d%s" % (r >> 4, "=XID"[r & 15]) for r in runs[int(off[a]):int(off[a + 1])]) for a in range(res.n_aln)]
    return counts, value, cigars


def stats_of_refined(ctx: Context, b: RefineBatch, rres: RefineResult, lookup_table):
    """CalculateStatistics straight on the (context-owned) output of indel_refine_batch, no copies."""
    v = RefineBatch.__new__(RefineBatch)
    v.ctx, v.n, v.n_blocks_in = ctx, b.n, int(rres.n_blocks)
    v.blocks, v.block_off = int(rres.d_blocks), int(rres.d_block_off)
    v.q_seq, v.q_off, v.q_len, v.t_seq, v.t_off, v.t_len = b.q_seq, b.q_off, b.q_len, b.t_seq, b.t_off, b.t_len
    return calculate_statistics_batch(ctx, v, lookup_table)
