"""The device primitives behind BAM output (bam_encode.hip): an alignment's CIGAR as BAM ops, ranges of bases as 4-bit codes, ranges of quality strings
as phred bytes.  Inputs are device tensors; results are copied to numpy.  Behind them: BamSorter (bam_sort.hip), which sorts the records of several
batches by coordinate on the device and gives back BGZF members and the .bai bytes, BamMerger (bam_merge.hip), which streams several sorted BAM files
into one under a bounded device budget, index_host, the same index from a sorted stream on the host, BamView (bam_view.hip), which prints a BAM file
as SAM text on the device, whole or for a region reached through the .bai, and bai_query, the region planner alone on the host."""
import ctypes as C
import os

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


# ---- coordinate-sorted BAM with a .bai index (bam_sort.hip) -------------------------------------------------------------------------------------------
ERR_INVALID, ERR_NOMEM = -1, -3


class SorterFull(MemoryError):
    """lra_bam_sorter_add_device's LRA_ERR_NOMEM: the batch does not fit the sorter's budget; nothing changed.  Finish a run and add again."""


class BamSorter:
    """lra_bam_sorter: raw BAM records of any number of batches, held in device memory of the sorter's own (at most max_bytes, finish included), given back
    sorted by coordinate as BGZF members, with the bytes of the .bai file."""

    def __init__(self, ctx: Context, max_bytes):
        self.ctx = ctx
        self.h = C.c_void_p()
        ctx.check(ctx.lib.lra_bam_sorter_create(ctx.h, C.c_uint64(int(max_bytes)), C.byref(self.h)))

    def add(self, stream, rec_start):
        """stream: uint8 device tensor (or raw address); rec_start: uint64 device tensor [n + 1] of record starts.  SorterFull when the budget is short."""
        n = int(rec_start.numel()) - 1
        rc = self.ctx.lib.lra_bam_sorter_add_device(self.h, C.c_void_p(stream if isinstance(stream, int) else stream.data_ptr()), C.c_void_p(rec_start.data_ptr()),
                                                    C.c_uint64(max(n, 0)))
        if rc == ERR_NOMEM:
            raise SorterFull(self.ctx.lib.lra_ctx_last_error(self.ctx.h).decode())
        self.ctx.check(rc)

    def held(self):
        """-> (records, bytes) held"""
        n, b = C.c_uint64(0), C.c_uint64(0)
        self.ctx.check(self.ctx.lib.lra_bam_sorter_held(self.h, C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)

    def finish(self, first_member_file_offset, ref_len):
        """sorts what is held; ref_len: the references' lengths.  Then pieces() / next(), then index()."""
        a = np.ascontiguousarray(ref_len, np.uint64)
        self.ctx.check(self.ctx.lib.lra_bam_sorter_finish(self.h, C.c_uint64(int(first_member_file_offset)), len(a), C.c_void_p(a.ctypes.data) if len(a) else None))

    def next(self):
        """the next piece of whole BGZF members as bytes; b"": done"""
        p, n = C.c_void_p(), C.c_uint64(0)
        self.ctx.check(self.ctx.lib.lra_bam_sorter_next(self.h, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value) if n.value else b""

    def pieces(self):
        while True:
            b = self.next()
            if not b:
                return
            yield b

    def index(self):
        """the .bai bytes of the run whose last piece has been taken; the sorter is empty afterwards"""
        p, n = C.c_void_p(), C.c_uint64(0)
        self.ctx.check(self.ctx.lib.lra_bam_sorter_index(self.h, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value)

    def stats(self):
        """ms of the last run: keys + span, the sort, the gather, the compress stage, the index"""
        a = (C.c_double * 5)()
        self.ctx.check(self.ctx.lib.lra_bam_sorter_stats(self.h, a))
        return dict(zip(("keys_span", "sort", "gather", "compress", "index"), a))

    def close(self):
        if self.h:
            if self.ctx.h:                                                      # (a sorter that outlives its context is left alone: destroy needs the context's device)
                self.ctx.lib.lra_bam_sorter_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MergerStats(C.Structure):
    """struct lra_bam_merger_stats (include/lra_hip.h)"""
    _fields_ = [("rounds", C.c_uint64), ("records", C.c_uint64), ("bytes", C.c_uint64), ("peak_device_bytes", C.c_uint64), ("refills", C.c_uint64 * 256),
                ("ms_read_inflate", C.c_double), ("ms_frame_keys", C.c_double), ("ms_bound_rank", C.c_double), ("ms_gather_span", C.c_double),
                ("ms_compress", C.c_double), ("ms_index", C.c_double)]


class BamMerger:
    """lra_bam_merger: 1 .. 256 coordinate-sorted BAM files with one reference table, merged on the device in at most max_bytes of device memory into
    BGZF members and the .bai bytes.  The caller writes header()'s bytes (compressed as it likes), passes the length of what it wrote as
    first_member_file_offset, writes pieces() behind it, then the EOF member; index() gives the .bai.  window_bytes: compressed bytes per refill of a run
    (0: from the budget)."""

    def __init__(self, ctx: Context, paths, max_bytes, first_member_file_offset, window_bytes=0):
        self.ctx = ctx
        self.h = C.c_void_p()
        self.n_runs = len(paths)
        arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
        ctx.check(ctx.lib.lra_bam_merger_create(ctx.h, C.c_uint64(int(max_bytes)), C.c_uint64(int(window_bytes)), len(paths), arr,
                                                C.c_uint64(int(first_member_file_offset)), C.byref(self.h)))

    def header(self):
        """-> (the first run's uncompressed header bytes, the references' lengths)"""
        p, n, n_ref, rl = C.c_void_p(), C.c_uint64(0), C.c_int(0), C.c_void_p()
        self.ctx.check(self.ctx.lib.lra_bam_merger_header(self.h, C.byref(p), C.byref(n), C.byref(n_ref), C.byref(rl)))
        lens = list((C.c_uint64 * n_ref.value).from_address(rl.value)) if n_ref.value else []
        return C.string_at(p, n.value), lens

    def next(self):
        """the next piece of whole BGZF members as bytes; b"": done"""
        p, n = C.c_void_p(), C.c_uint64(0)
        self.ctx.check(self.ctx.lib.lra_bam_merger_next(self.h, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value) if n.value else b""

    def pieces(self):
        while True:
            b = self.next()
            if not b:
                return
            yield b

    def index(self):
        """the .bai bytes, after the last piece"""
        p, n = C.c_void_p(), C.c_uint64(0)
        self.ctx.check(self.ctx.lib.lra_bam_merger_index(self.h, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value)

    def stats(self):
        """rounds, records, bytes, refills per run, the peak of the merger's device bytes, ms per stage"""
        s = MergerStats()
        self.ctx.check(self.ctx.lib.lra_bam_merger_stats(self.h, C.byref(s)))
        d = {k: getattr(s, k) for k, _ in MergerStats._fields_ if k != "refills"}
        d["refills"] = list(s.refills)[:self.n_runs]
        return d

    def close(self):
        if self.h:
            if self.ctx.h:
                self.ctx.lib.lra_bam_merger_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BamPass:
    """What the wrappers of the windowed passes over a BAM file share (BamView, BamDepth, BamVcf, BamSvCalls; bam_pass.h behind them): the handle, made
    and reached through the C functions <_prefix>_create, _header, _all, _region, _next, _stats and _destroy; the file's reference names and lengths,
    decoded once; a pass's start from ref / beg / end; stats() from the class's _Stats structure."""
    _prefix = None
    _Stats = None
    _header_front = 0                                                           # pointer arguments of <_prefix>_header in front of n_ref (BamView: the text, its length)

    def _fn(self, name):
        return getattr(self.ctx.lib, "%s_%s" % (self._prefix, name))

    def _create(self, ctx, path, bai, *args):
        self.ctx = ctx
        self.h = C.c_void_p()
        self._refs = None
        ctx.check(self._fn("create")(ctx.h, os.fsencode(path), os.fsencode(bai) if bai is not None else None, *args, C.byref(self.h)))

    def _references(self):
        """-> (the reference names as bytes, their lengths): new lists"""
        if self._refs is None:
            n_ref, nm, rl = C.c_int(0), C.c_void_p(), C.c_void_p()
            self.ctx.check(self._fn("header")(self.h, *([None] * self._header_front), C.byref(n_ref), C.byref(nm), C.byref(rl)))
            k = n_ref.value
            self._refs = ([C.string_at(q) for q in (C.c_char_p * k).from_address(nm.value)] if k else [],
                          list((C.c_uint64 * k).from_address(rl.value)) if k else [])
        return list(self._refs[0]), list(self._refs[1])

    def _start(self, ref, beg=0, end=None):
        """starts a pass: ref None: the whole file; ref: a reference's index or name, [beg, end) 0-based half-open (end None: the reference's end)"""
        if ref is None:
            self.ctx.check(self._fn("all")(self.h))
            return
        names, lens = self._references()
        if not isinstance(ref, int):
            key = ref.encode() if isinstance(ref, str) else ref
            if key not in names:
                raise ValueError("no reference %r in the file" % ref)
            ref = names.index(key)
        if end is None:
            end = lens[ref] if 0 <= ref < len(lens) else 0
        self.ctx.check(self._fn("region")(self.h, C.c_int32(ref), C.c_int64(int(beg)), C.c_int64(int(end))))

    def _next(self, *out):
        self.ctx.check(self._fn("next")(self.h, *[C.byref(x) for x in out]))

    def header(self):
        """-> (the reference names as bytes, their lengths)"""
        return self._references()

    def stats(self):
        s = self._Stats()
        self.ctx.check(self._fn("stats")(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in self._Stats._fields_}

    def close(self):
        if self.h:
            if self.ctx.h:                                                      # (an object that outlives its context is left alone: destroy needs the context's device)
                self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ViewStats(C.Structure):
    """struct lra_bam_view_stats (include/lra_hip.h)"""
    _fields_ = [("windows", C.c_uint64), ("records", C.c_uint64), ("bytes_read", C.c_uint64), ("bytes_inflated", C.c_uint64), ("bytes_text", C.c_uint64),
                ("ms_read_inflate", C.c_double), ("ms_frame_select", C.c_double), ("ms_tags_lengths", C.c_double), ("ms_floats", C.c_double),
                ("ms_emit", C.c_double), ("ms_copy", C.c_double)]


def parse_region(text, names, ref_len):
    """a region as samtools view takes it -- `name` or `name:beg-end`, 1-based and inclusive, commas in the numbers allowed; `name:beg` runs to the
    reference's end -- -> (ref_id, beg, end), 0-based and half-open.  A name that holds a colon is matched whole first.  ValueError otherwise."""
    names = [n.decode() if isinstance(n, bytes) else n for n in names]
    if text in names:
        r = names.index(text)
        return r, 0, int(ref_len[r])
    name, sep, span = text.rpartition(":")
    if not sep or name not in names:
        raise ValueError("region %r names no reference of the file" % text)
    r = names.index(name)
    lo, dash, hi = span.replace(",", "").partition("-")
    try:
        beg = int(lo) - 1 if lo else 0
        end = int(hi) if hi else int(ref_len[r])
    except ValueError:
        raise ValueError("region %r: not name:beg-end" % text)
    if beg < 0 or end < beg:
        raise ValueError("region %r: not a 1-based inclusive interval" % text)
    return r, beg, end


class BamView(_BamPass):
    """lra_bam_view: the records of a BAM file as SAM text, printed on the device; bai: the path of its .bai index (None: whole-file passes only);
    window_bytes: compressed bytes per step (0: the library's default)."""
    _prefix, _Stats, _header_front = "lra_bam_view", ViewStats, 2

    def __init__(self, ctx: Context, path, bai=None, window_bytes=0):
        self._create(ctx, path, bai, C.c_uint64(int(window_bytes)))

    def header(self):
        """-> (header text as bytes, the reference names as bytes, their lengths)"""
        t, n = C.c_void_p(), C.c_uint64(0)
        self.ctx.check(self.ctx.lib.lra_bam_view_header(self.h, C.byref(t), C.byref(n), None, None, None))
        return ((C.string_at(t, n.value) if n.value else b""),) + self._references()

    def set_flags(self, require=0, exclude=0):
        self.ctx.check(self.ctx.lib.lra_bam_view_set_flags(self.h, C.c_uint32(int(require)), C.c_uint32(int(exclude))))

    def fetch(self, ref=None, beg=0, end=None):
        """yields the pieces (bytes: whole SAM lines) of a pass: ref None: every record; ref: a reference's index or name, [beg, end) 0-based half-open
        (end None: the reference's end).  self.last_records counts the pass's lines."""
        self._start(ref, beg, end)
        self.last_records = 0
        while True:
            p, n, k = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
            self._next(p, n, k)
            if not n.value:
                return
            self.last_records += k.value
            yield C.string_at(p, n.value)


class DepthOpts(C.Structure):
    """struct lra_bam_depth_opts (include/lra_hip.h)"""
    _fields_ = [(k, C.c_uint32) for k in ("require", "exclude", "min_mapq", "count_deletions", "bin", "all_positions", "want_text", "want_values")] + \
               [("window_bytes", C.c_uint64), ("span_bases", C.c_uint64)]


class DepthPiece(C.Structure):
    """struct lra_bam_depth_piece (include/lra_hip.h)"""
    _fields_ = [("ref_id", C.c_int32), ("first", C.c_int64), ("count", C.c_uint64), ("depth", C.c_void_p), ("sum", C.c_void_p), ("text", C.c_void_p),
                ("text_len", C.c_uint64)]


class DepthStats(C.Structure):
    """struct lra_bam_depth_stats (include/lra_hip.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("windows", "records_read", "records_counted", "records_filtered", "slides", "covered", "depth_sum", "depth_max",
                                          "bytes_read", "bytes_inflated", "bytes_delivered")] + \
               [(k, C.c_double) for k in ("ms_read_inflate", "ms_frame_select", "ms_ops", "ms_accumulate", "ms_finish", "ms_text", "ms_copy")]


class BamDepth(_BamPass):
    """lra_bam_depth: the coverage of a coordinate-sorted BAM file, computed on the device, per base (bin 0) or per bin; bai: the path of its .bai index
    (None: whole-file passes only).  exclude None: 0x704, what samtools depth drops.  text / values: what a pass hands back."""
    _prefix, _Stats = "lra_bam_depth", DepthStats

    def __init__(self, ctx: Context, path, bai=None, require=0, exclude=None, min_mapq=0, count_deletions=False, bin=0, all_positions=False, text=True,
                 values=False, window_bytes=0, span_bases=0):
        self.bin = int(bin)
        o = DepthOpts(int(require), 0xffffffff if exclude is None else int(exclude), int(min_mapq), int(bool(count_deletions)), self.bin,
                      int(bool(all_positions)), int(bool(text)), int(bool(values)), int(window_bytes), int(span_bases))
        self._create(ctx, path, bai, C.byref(o))

    def fetch(self, ref=None, beg=0, end=None):
        """yields the pieces of a pass as (ref_id, first, count, values, text): ref None: the whole file; ref: a reference's index or name, [beg, end)
        0-based half-open (end None: the reference's end).  values: a numpy array (uint32 depths from position `first` on, or uint64 bin sums from the
        bin that starts at `first` on; None when the object was made without values) -- a view of the object's memory, valid until the next piece;
        text: bytes (b"" without text)."""
        self._start(ref, beg, end)
        while True:
            p = DepthPiece()
            self._next(p)
            if not p.count and not p.text_len:
                return
            at, dt = (p.sum, np.uint64) if self.bin else (p.depth, np.uint32)
            vals = np.ctypeslib.as_array(C.cast(at, C.POINTER(C.c_uint64 if self.bin else C.c_uint32)), shape=(p.count,)).view(dt) if at and p.count else None
            yield p.ref_id, p.first, p.count, vals, (C.string_at(p.text, p.text_len) if p.text_len else b"")


class VcfOpts(C.Structure):
    """struct lra_bam_vcf_opts (include/lra_hip.h)"""
    _fields_ = [(k, C.c_uint32) for k in ("require", "exclude", "min_mapq", "min_length", "pos_one_based", "want_text", "want_values", "drop_contained")] + \
               [("window_bytes", C.c_uint64)]


# struct lra_bam_vcf_variant (include/lra_hip.h), 40 bytes
VCF_VARIANT_DTYPE = np.dtype([("record", "<u8"), ("text_off", "<u8"), ("svlen", "<i8"), ("ref_id", "<i4"), ("pos", "<i4"), ("qstart", "<u4"), ("kind", "u1"),
                              ("strand", "u1"), ("pad", "<u2")])


class VcfPiece(C.Structure):
    """struct lra_bam_vcf_piece (include/lra_hip.h)"""
    _fields_ = [("n_variants", C.c_uint64), ("variants", C.c_void_p), ("text", C.c_void_p), ("text_len", C.c_uint64)]


class VcfStats(C.Structure):
    """struct lra_bam_vcf_stats (include/lra_hip.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("windows", "records_read", "records_walked", "records_filtered", "records_skipped", "n_ins", "n_del", "bytes_read",
                                          "bytes_inflated", "bytes_text")] + \
               [(k, C.c_double) for k in ("ms_read_inflate", "ms_frame_select", "ms_ops", "ms_walk", "ms_lengths", "ms_emit", "ms_copy")] + \
               [("records_contained", C.c_uint64)]


VCF_INFO_LINES = (
    '##INFO=<ID=QNAME,Number=1,Type=String,Description="Name of query sequence">\n'
    '##INFO=<ID=QSTART,Number=1,Type=Integer,Description="Position of query sequence">\n'
    '##INFO=<ID=QSTRAND,Number=1,Type=String,Description="Contig strand">\n'
    '##INFO=<ID=SVLEN,Number=.,Type=Integer,Description="Difference in length between REF and ALT alleles">\n'
    '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">\n'
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n')


def vcf_header(reference, names, lens, sample="unknown"):
    """the header in front of BamVcf's lines (no GPU): the file format, date and source lines of the reference's script, ##reference=<the path given>, one
    ##contig line per entry of the BAM header's reference table (names as bytes or str), the five INFO lines, the FORMAT line and the column line with
    the sample's name -> bytes"""
    text = lambda x: x.decode() if isinstance(x, bytes) else str(x)
    out = "##fileformat=VCFv4.2\n##fileDate=20190102\n##source=SamToVCF\n##reference=%s\n" % text(reference)
    out += "".join("##contig=<ID=%s,length=%d>\n" % (text(n), int(k)) for n, k in zip(names, lens))
    out += VCF_INFO_LINES + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n" % text(sample)
    return out.encode()


class BamVcf(_BamPass):
    """lra_bam_vcf: one VCF line per insertion and deletion of a BAM file's alignments, walked and printed on the device.  ctx must hold the genome and its
    chromosome table (lra_amd.genome_io.GenomeFile(...).install(ctx), or lra_ctx_load_genome + lra_ctx_load_chromosomes), in the order of the file's
    reference table.  bai: the path of its .bai index (None: whole-file passes only).  exclude None: 0x4.  text / values: what a pass hands back.
    drop_contained: records that lie inside an earlier record of their reference are not walked (the reference's ParseAlignment.py; the file must be
    coordinate-sorted, and a region pass must begin at 0)."""
    _prefix, _Stats = "lra_bam_vcf", VcfStats

    def __init__(self, ctx: Context, path, bai=None, require=0, exclude=None, min_mapq=0, min_length=1, pos_one_based=False, text=True, values=False,
                 window_bytes=0, drop_contained=False):
        o = VcfOpts(int(require), 0xffffffff if exclude is None else int(exclude), int(min_mapq), int(min_length), int(bool(pos_one_based)), int(bool(text)),
                    int(bool(values)), int(bool(drop_contained)), int(window_bytes))
        self._create(ctx, path, bai, C.byref(o))

    def fetch(self, ref=None, beg=0, end=None):
        """yields the pieces of a pass as (n_variants, values, text): ref None: the whole file; ref: a reference's index or name, [beg, end) 0-based
        half-open (end None: the reference's end).  values: a numpy record array of VCF_VARIANT_DTYPE (None when the object was made without values) -- a
        view of the object's memory, valid until the next piece; text: bytes (b"" without text)."""
        self._start(ref, beg, end)
        while True:
            p = VcfPiece()
            self._next(p)
            if not p.n_variants and not p.text_len:
                return
            vals = None
            if p.variants and p.n_variants:
                vals = np.ctypeslib.as_array(C.cast(p.variants, C.POINTER(C.c_uint8)), shape=(p.n_variants * VCF_VARIANT_DTYPE.itemsize,)).view(VCF_VARIANT_DTYPE)
            yield p.n_variants, vals, (C.string_at(p.text, p.text_len) if p.text_len else b"")


class SvCallsOpts(C.Structure):
    """struct lra_bam_svcalls_opts (include/lra_hip.h)"""
    _fields_ = [(k, C.c_uint32) for k in ("require", "exclude", "min_mapq", "min_size", "drop_contained", "pos_one_based", "vcf_columns", "want_text", "want_values",
                                          "reserved")] + [("window_bytes", C.c_uint64), ("aligner", C.c_char_p), ("hap", C.c_char_p)]


# struct lra_bam_svcalls_row (include/lra_hip.h), 64 bytes
SVCALLS_ROW_DTYPE = np.dtype([("record", "<u8"), ("text_off", "<u8"), ("nr", "<u8"), ("start", "<i8"), ("end", "<i8"), ("svlen", "<i8"), ("ref_id", "<i4"),
                              ("qstart", "<u4"), ("kind", "u1"), ("strand", "u1"), ("pad", "<u2"), ("pad2", "<u4")])


class SvCallsPiece(C.Structure):
    """struct lra_bam_svcalls_piece (include/lra_hip.h)"""
    _fields_ = [("n_rows", C.c_uint64), ("rows", C.c_void_p), ("text", C.c_void_p), ("text_len", C.c_uint64), ("ref_id", C.c_int32), ("kind", C.c_uint32)]


class SvCallsStats(C.Structure):
    """struct lra_bam_svcalls_stats (include/lra_hip.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("windows", "records_read", "records_contained", "records_walked", "small_ins", "small_del", "masked_ins", "masked_del",
                                          "merged_ins", "merged_del", "kept_ins", "kept_del", "merge_rounds", "bytes_read", "bytes_inflated", "bytes_text")] + \
               [(k, C.c_double) for k in ("ms_read_inflate", "ms_frame_select", "ms_ops", "ms_walk", "ms_lengths", "ms_rows", "ms_merge", "ms_emit", "ms_copy")]


def parse_bed(lines, names):
    """the intervals of a BED file's lines (bytes or str; 0-based, half-open; track, browser and comment lines skipped) whose name is one of `names` -- the
    BAM header's -- -> [(ref_id, beg, end)]; other names are ignored (no GPU)"""
    idx = {(n.decode() if isinstance(n, bytes) else n): k for k, n in enumerate(names)}
    out = []
    for ln in lines:
        ln = ln.decode() if isinstance(ln, bytes) else ln
        f = ln.split()
        if len(f) < 3 or f[0].startswith("#") or f[0] in ("track", "browser"):
            continue
        if f[0] in idx:
            out.append((idx[f[0]], int(f[1]), int(f[2])))
    return out


class BamSvCalls(_BamPass):
    """lra_bam_svcalls: the merged DEL and INS tables of one haplotype's assembly alignments, from a coordinate-sorted BAM -- the contained filter, the calls,
    the size and mask filters, the numbering and the merge of the reference's call_assembly_SVs pipeline, on the device (include/lra_hip.h has the rules).
    ctx must hold the genome and its chromosome table, as for BamVcf.  vcf_columns: lines without the END column."""
    _prefix, _Stats = "lra_bam_svcalls", SvCallsStats

    def __init__(self, ctx: Context, path, bai=None, require=0, exclude=None, min_mapq=0, min_size=40, drop_contained=True, aligner="aligner", hap="maternal",
                 pos_one_based=False, vcf_columns=False, text=True, values=False, window_bytes=0):
        enc = lambda x: x if isinstance(x, bytes) else str(x).encode()
        o = SvCallsOpts(int(require), 0xffffffff if exclude is None else int(exclude), int(min_mapq), int(min_size), int(bool(drop_contained)), int(bool(pos_one_based)),
                        int(bool(vcf_columns)), int(bool(text)), int(bool(values)), 0, int(window_bytes), enc(aligner), enc(hap))
        self._create(ctx, path, bai, C.byref(o))

    def set_mask(self, intervals):
        """intervals: [(ref_id, beg, end)], 0-based and half-open, in any order; [] takes the mask away"""
        iv = list(intervals)
        r = np.ascontiguousarray([x[0] for x in iv], np.int32)
        b = np.ascontiguousarray([x[1] for x in iv], np.int64)
        e = np.ascontiguousarray([x[2] for x in iv], np.int64)
        q = lambda a: C.c_void_p(a.ctypes.data) if len(a) else None
        self.ctx.check(self._fn("set_mask")(self.h, C.c_uint64(len(iv)), q(r), q(b), q(e)))

    def fetch(self, ref=None):
        """yields the pieces of a pass as (ref_id, kind "DEL" / "INS", n_rows, values, text): ref None: the whole file; ref: a reference's index or name.  A
        reference's DEL piece comes in front of its INS piece.  values: a numpy record array of SVCALLS_ROW_DTYPE (None when the object was made without
        values) -- a view of the object's memory, valid until the next piece; text: bytes (b"" without text)."""
        self._start(ref)
        while True:
            p = SvCallsPiece()
            self._next(p)
            if not p.n_rows and not p.text_len:
                return
            vals = None
            if p.rows and p.n_rows:
                vals = np.ctypeslib.as_array(C.cast(p.rows, C.POINTER(C.c_uint8)), shape=(p.n_rows * SVCALLS_ROW_DTYPE.itemsize,)).view(SVCALLS_ROW_DTYPE)
            yield p.ref_id, "DEL" if p.kind else "INS", p.n_rows, vals, (C.string_at(p.text, p.text_len) if p.text_len else b"")


class SvCombineOpts(C.Structure):
    """struct lra_sv_combine_opts (include/lra_hip.h)"""
    _fields_ = [(k, C.c_uint32) for k in ("require", "exclude", "min_mapq", "min_size", "drop_contained", "pos_one_based", "frac_num", "frac_den", "filter_pass",
                                          "want_text", "want_values", "reserved")] + [("window_bytes", C.c_uint64), ("aligner", C.c_char_p)]


# struct lra_sv_combine_row (include/lra_hip.h), 64 bytes: SVCALLS_ROW_DTYPE with hap and cls in its pad
SVCOMBINE_ROW_DTYPE = np.dtype([("record", "<u8"), ("text_off", "<u8"), ("nr", "<u8"), ("start", "<i8"), ("end", "<i8"), ("svlen", "<i8"), ("ref_id", "<i4"),
                                ("qstart", "<u4"), ("kind", "u1"), ("strand", "u1"), ("hap", "u1"), ("cls", "u1"), ("pad", "<u4")])


class SvCombinePiece(C.Structure):
    """struct lra_sv_combine_piece (include/lra_hip.h)"""
    _fields_ = [("n_rows", C.c_uint64), ("rows", C.c_void_p), ("text", C.c_void_p), ("text_len", C.c_uint64), ("hap", C.c_uint32), ("kind", C.c_uint32),
                ("cls", C.c_uint32), ("pad", C.c_uint32)]


class SvCombineStats(C.Structure):
    """struct lra_sv_combine_stats (include/lra_hip.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("runs", "het_m_ins", "het_m_del", "het_p_ins", "het_p_del", "hom_ins", "hom_del", "partnered_p_ins", "partnered_p_del",
                                          "bytes_text")] + \
               [(k, C.c_double) for k in ("ms_pass_m", "ms_pass_p", "ms_classify", "ms_emit", "ms_copy")] + [("passes", SvCallsStats * 2)]


# the seven files of tools/svcombine_bam.py in delivery order: (hap, kind, cls) -> the file's suffix behind PREFIX
SVCOMBINE_FILES = ((("maternal", "INS", "het"), ".maternal.INS.het.vcf"), (("maternal", "DEL", "het"), ".maternal.DEL.het.vcf"),
                   (("paternal", "INS", "het"), ".paternal.INS.het.vcf"), (("paternal", "DEL", "het"), ".paternal.DEL.het.vcf"),
                   (("maternal", "INS", "hom"), ".INS.hom.vcf"), (("maternal", "DEL", "hom"), ".DEL.hom.vcf"))


def parse_frac(text):
    """"3/10" -> (3, 10); ValueError unless it is NUM/DEN with 0 < NUM <= DEN (no GPU)"""
    num, sep, den = str(text).partition("/")
    if not sep or not num.strip().isdigit() or not den.strip().isdigit() or not 0 < int(num) <= int(den) < 2 ** 32:
        raise ValueError("fraction %r: not NUM/DEN with 0 < NUM <= DEN" % (text,))
    return int(num), int(den)


class SvCombine(_BamPass):
    """lra_sv_combine: two haplotypes' assembly SV calls as the diploid call set -- the rules Homcalls, Hetcalls and combineHet of the reference's
    call_assembly_SVs pipeline on the device (include/lra_hip.h has the rules).  path_m / path_p: the maternal and the paternal haplotype's coordinate-sorted
    BAM; ctx must hold the genome and its chromosome table, as for BamSvCalls.  frac: (num, den) of the partner test, None: 3 / 10.  filter_pass: the FILTER
    column is PASS, not INFO a second time."""
    _prefix, _Stats = "lra_sv_combine", SvCombineStats

    def __init__(self, ctx: Context, path_m, path_p, bai_m=None, bai_p=None, require=0, exclude=None, min_mapq=0, min_size=40, drop_contained=True,
                 aligner="aligner", pos_one_based=False, frac=None, filter_pass=False, text=True, values=False, window_bytes=0):
        enc = lambda x: x if isinstance(x, bytes) else str(x).encode()
        num, den = (0, 0) if frac is None else frac
        o = SvCombineOpts(int(require), 0xffffffff if exclude is None else int(exclude), int(min_mapq), int(min_size), int(bool(drop_contained)),
                          int(bool(pos_one_based)), int(num), int(den), int(bool(filter_pass)), int(bool(text)), int(bool(values)), 0, int(window_bytes), enc(aligner))
        self._create(ctx, path_m, bai_m, os.fsencode(path_p), os.fsencode(bai_p) if bai_p is not None else None, C.byref(o))

    set_mask = BamSvCalls.set_mask

    def stats(self):
        """-> the object's counts and times; "passes": the two lra_bam_svcalls passes' own stats, maternal first"""
        s = SvCombineStats()
        self.ctx.check(self.ctx.lib.lra_sv_combine_stats(self.h, C.byref(s)))
        out = {k: getattr(s, k) for k, _ in SvCombineStats._fields_ if k != "passes"}
        out["passes"] = [{k: getattr(p, k) for k, _ in SvCallsStats._fields_} for p in s.passes]
        return out

    def fetch(self, ref=None):
        """yields the pieces of a run as (hap "maternal" / "paternal", kind "INS" / "DEL", cls "het" / "hom", n_rows, values, text) in combineHet's order:
        the maternal het pieces (INS, DEL), the paternal ones, then the hom pieces (hap "maternal": their IDs).  ref None: the whole files; ref: a
        reference's index or name.  values: a numpy record array of SVCOMBINE_ROW_DTYPE (None without values), valid until the next piece."""
        self._start(ref)
        while True:
            p = SvCombinePiece()
            self._next(p)
            if not p.n_rows and not p.text_len:
                return
            vals = None
            if p.rows and p.n_rows:
                vals = np.ctypeslib.as_array(C.cast(p.rows, C.POINTER(C.c_uint8)), shape=(p.n_rows * SVCOMBINE_ROW_DTYPE.itemsize,)).view(SVCOMBINE_ROW_DTYPE)
            yield ("paternal" if p.hap else "maternal", "DEL" if p.kind else "INS", "hom" if p.cls else "het", p.n_rows, vals,
                   (C.string_at(p.text, p.text_len) if p.text_len else b""))


def bai_query(bai, n_ref, ref_id, beg, end, lib=None):
    """lra_bai_query_host (no GPU): the chunks [(beg, end)] of virtual offsets a region pass reads, from the .bai bytes.  n_ref: the BAM header's
    reference count (-1: not compared).  ValueError for LRA_ERR_INVALID (an index the reader refuses, ref_id outside it, beg > end)."""
    if lib is None:
        from ._lib import load_library
        lib = load_library()
    b = np.frombuffer(bytes(bai), np.uint8)
    p, n = C.c_void_p(), C.c_uint64(0)
    if lib.lra_bai_query_host(C.c_void_p(b.ctypes.data) if len(b) else None, C.c_uint64(len(b)), int(n_ref), C.c_int32(int(ref_id)), C.c_int64(int(beg)),
                              C.c_int64(int(end)), C.byref(p), C.byref(n)) != 0:
        raise ValueError("lra_bai_query_host: the index or the region is refused")
    a = np.ctypeslib.as_array((C.c_uint64 * (2 * n.value)).from_address(p.value)).copy() if n.value else np.zeros(0, np.uint64)
    return [(int(a[2 * i]), int(a[2 * i + 1])) for i in range(n.value)]


def index_host(stream, ref_len, member_off, first_member_file_offset=0, lib=None):
    """lra_bam_index_host (no GPU): the .bai bytes of the sorted raw record stream `stream` (bytes) whose BGZF members start at member_off[n_members + 1]
    behind first_member_file_offset.  ValueError for LRA_ERR_INVALID (a record cut short, a refID outside the table, a reference above 2^29 bases)."""
    if lib is None:
        from ._lib import load_library
        lib = load_library()
    s = np.frombuffer(bytes(stream), np.uint8)
    r = np.ascontiguousarray(ref_len, np.uint64)
    m = np.ascontiguousarray(member_off, np.uint64)
    q = lambda a: C.c_void_p(a.ctypes.data) if len(a) else None
    n = C.c_uint64(0)
    args = (q(s), C.c_uint64(len(s)), len(r), q(r), C.c_void_p(m.ctypes.data), C.c_uint64(len(m) - 1), C.c_uint64(int(first_member_file_offset)))
    if lib.lra_bam_index_host(*args, None, C.c_uint64(0), C.byref(n)) != 0:
        raise ValueError("lra_bam_index_host: not a sorted BAM record stream this index can hold")
    out = np.empty(int(n.value), np.uint8)
    if lib.lra_bam_index_host(*args, C.c_void_p(out.ctypes.data), C.c_uint64(len(out)), C.byref(n)) != 0:
        raise ValueError("lra_bam_index_host failed")
    return out.tobytes()
