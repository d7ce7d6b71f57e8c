"""ctypes mirror of the input side (lra_amd/csrc/input.hip): FASTA / FASTQ / SAM / BAM batches and the host-buffer boundary.  Tests and tools only."""
import ctypes as C

import numpy as np

from ._lib import load_library


READS_COMPRESSED_TEXT = 1   # LRA_READS_COMPRESSED_TEXT
READS_DEV_QUAL = 1          # LRA_READS_DEV_QUAL
READS_DEV_NO_HOST = 2       # LRA_READS_DEV_NO_HOST
PACK_CHUNK = 4096           # pack_strings.hip's PK_CHUNK: output bytes per wave of lra_pack_strings_batch (the tests' shapes)


class ReadBatchC(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("total_bases", C.c_uint64), ("seq", C.c_void_p), ("off", C.POINTER(C.c_uint64)), ("read_len", C.POINTER(C.c_int32)),
                ("names", C.POINTER(C.c_char_p)), ("reads", C.POINTER(C.c_void_p)), ("quals", C.POINTER(C.c_char_p))]


class ReadsFile:
    """ctx=None: lra_reads_next_batch (host parsing).  With a Context: lra_reads_next_batch_device (the parsing on that context's GPU; chunk = the bytes
    of a file it reads and parses per step, lra_reads_set_device_chunk; None keeps the library's default).  flag_remove: SAM / BAM records whose flag
    meets it are skipped (-Flag); passthrough: each SAM / BAM read's aux fields in the batch's "tags" (--passthrough).  compressed_text: gzip / BGZF
    FASTA and FASTQ files are read (lra_reads_open_flags with LRA_READS_COMPRESSED_TEXT); without it they are refused, as the reference refuses them.
    device_quals (device form): every batch keeps its qualities on the device too (LRA_READS_DEV_QUAL; the batch's d_qual / d_qual_off); no_host_copy
    (needs device_quals): the bases and qualities are not copied to the host (LRA_READS_DEV_NO_HOST; the batch's seqs is None, its quals are stubs)."""

    def __init__(self, files, ctx=None, chunk=None, flag_remove=0, passthrough=False, compressed_text=False, device_quals=False, no_host_copy=False):
        self.lib = load_library()
        self.ctx = ctx
        arr = (C.c_char_p * len(files))(*[f.encode() if isinstance(f, str) else f for f in files])
        self.h = C.c_void_p()
        if compressed_text:
            rc = self.lib.lra_reads_open_flags(arr, len(files), READS_COMPRESSED_TEXT, C.byref(self.h))
        else:
            rc = self.lib.lra_reads_open(arr, len(files), C.byref(self.h))
        if rc != 0:
            raise IOError("cannot determine the format of the input reads (%d)" % rc)
        if chunk is not None:
            rc = self.lib.lra_reads_set_device_chunk(self.h, C.c_uint64(int(chunk)))
            if rc != 0:
                self.close()
                raise ValueError("lra_reads_set_device_chunk(%d) failed (%d)" % (int(chunk), rc))
        if flag_remove or passthrough:
            if self.lib.lra_reads_set_flag_remove(self.h, int(flag_remove)) != 0 or self.lib.lra_reads_set_passthrough(self.h, int(bool(passthrough))) != 0:
                self.close()
                raise ValueError("lra_reads_set_flag_remove / lra_reads_set_passthrough failed")
        self.device_quals, self.no_host_copy = bool(device_quals), bool(no_host_copy)
        if device_quals or no_host_copy:
            mode = (READS_DEV_QUAL if device_quals else 0) | (READS_DEV_NO_HOST if no_host_copy else 0)
            rc = self.lib.lra_reads_set_device_resident(self.h, mode) if ctx is not None else -1
            if rc != 0:
                self.close()
                raise ValueError("lra_reads_set_device_resident(%d) failed (%d): device_quals needs the device form, no_host_copy needs device_quals" % (mode, rc))

    def next_batch(self, max_bases):
        """-> None at the end, else dict(names, seqs, quals (None for FASTA reads), off, raw=(ReadBatchC kept alive until the next call)); the device form
        adds d_seq / d_off (device pointers, valid until the next call) and n / total_bases, with device_quals d_qual / d_qual_off (the same); with
        no_host_copy seqs is None, read_len holds the reads' lengths and quals are stubs (None, or the string's first byte)"""
        b = ReadBatchC()
        if self.ctx is None:
            rc = self.lib.lra_reads_next_batch(self.h, C.c_uint64(int(max_bases)), C.byref(b))
            dev = None
        else:
            d_seq, d_off = C.c_void_p(), C.c_void_p()
            rc = self.lib.lra_reads_next_batch_device(self.h, self.ctx.h, C.c_uint64(int(max_bases)), C.byref(b), C.byref(d_seq), C.byref(d_off))
            dev = (d_seq.value, d_off.value)
        n = b.n_reads
        out = None
        if n:
            off = np.ctypeslib.as_array(b.off, shape=(n + 1,)).copy()
            seq = C.string_at(b.seq, int(b.total_bases)) if b.seq else None
            tags = C.POINTER(C.c_char_p)()
            self.lib.lra_reads_batch_tags(self.h, C.byref(tags))
            out = dict(names=[b.names[i] for i in range(n)], seqs=[seq[int(off[i]):int(off[i + 1])] for i in range(n)] if seq is not None else None, quals=[b.quals[i] for i in range(n)], off=off, raw=b,
                       tags=[tags[i] for i in range(n)] if tags else [None] * n)
            if dev is not None:
                out.update(d_seq=dev[0], d_off=dev[1], n=n, total_bases=int(b.total_bases), read_len=[int(b.read_len[i]) for i in range(n)])
                if self.device_quals:
                    d_qual, d_qual_off = C.c_void_p(), C.c_void_p()
                    if self.lib.lra_reads_batch_device_quals(self.h, C.byref(d_qual), C.byref(d_qual_off)) != 0:
                        raise RuntimeError("lra_reads_batch_device_quals failed")
                    out.update(d_qual=d_qual.value, d_qual_off=d_qual_off.value)
        if rc != 0:
            err = self.lib.lra_reads_last_error(self.h) or b""
            if not err and self.ctx is not None:
                err = self.lib.lra_ctx_last_error(self.ctx.h) or b""
            e = IOError("%s failed (%d): %s" % ("lra_reads_next_batch" if self.ctx is None else "lra_reads_next_batch_device", rc, err.decode()))
            e.partial = out                     # the reads in front of the bad record
            e.rc = rc
            raise e
        return out

    def close(self):
        if self.h:
            self.lib.lra_reads_close(self.h)
            self.h = None


def map_reads_host(mapper, raw_batch):
    """lra_map_reads_host on a batch of ReadsFile.next_batch (mapper: LowAccMapper / HighAccMapper) -> MapResult"""
    from .mapread import MapResult
    ctx = mapper.ctx
    res = MapResult()
    ctx.check(ctx.lib.lra_map_reads_host(ctx.h, raw_batch.n_reads, C.c_void_p(raw_batch.seq), raw_batch.off, C.byref(mapper.copts), C.byref(res)))
    return res


def map_reads_device(mapper, batch):
    """The driver the options select (bypassClustering: lra_map_reads_lowacc_batch, else lra_map_reads_highacc_batch, as lra_map_reads_host does) on a
    device-form batch of ReadsFile.next_batch, straight from the reader's device arrays (mapper: LowAccMapper / HighAccMapper) -> MapResult"""
    from .mapread import MapResult, set_store_all
    ctx = mapper.ctx
    res = MapResult()
    set_store_all(ctx, mapper.store_all)
    drv = ctx.lib.lra_map_reads_lowacc_batch if mapper.copts.bypassClustering else ctx.lib.lra_map_reads_highacc_batch
    ctx.check(drv(ctx.h, batch["n"], C.c_void_p(batch["d_seq"]), C.c_void_p(batch["d_off"]), C.c_uint64(batch["total_bases"]), C.byref(mapper.copts), C.byref(res)))
    return res
