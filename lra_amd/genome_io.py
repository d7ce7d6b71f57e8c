"""ctypes mirror of the genome reader (lra_amd/csrc/genome.hip: lra_genome_*): a genome FASTA -- plain text, gzip or BGZF -- into names, header.pos
and the bases back to back.  No algorithmic code here."""
import ctypes as C

import numpy as np

from ._lib import load_library


class GenomeFile:
    """ctx=None: lra_genome_read_host (parsing on the host; .seq is a numpy uint8 array).  With a Context: lra_genome_read_device (parsing on that
    context's GPU; .seq is a torch uint8 tensor there).  chunk = the bytes of the file's data per step (lra_genome_set_device_chunk; None keeps the
    library's default).  Both forms hold .seq with 64 zero bytes behind the bases: .seq is the bases alone, .padded the whole array."""

    def __init__(self, path, ctx=None, chunk=None):
        self.lib = load_library()
        self.ctx = ctx
        self.path = path
        self.h = C.c_void_p()
        rc = self.lib.lra_genome_open(path.encode() if isinstance(path, str) else path, C.byref(self.h))
        if rc != 0:
            self.h = None
            raise IOError("lra_genome_open(%s) failed (%d)" % (path, rc))
        if chunk is not None:
            rc = self.lib.lra_genome_set_device_chunk(self.h, C.c_uint64(int(chunk)))
            if rc != 0:
                self.close()
                raise ValueError("lra_genome_set_device_chunk(%d) failed (%d)" % (int(chunk), rc))
        self.names = self.chrom_pos = self.seq = self.padded = None

    def last_error(self):
        return (self.lib.lra_genome_last_error(self.h) or b"").decode()

    def read(self):
        """-> self, with names (list of bytes), chrom_pos (list of int, n_chrom + 1) and seq; IOError (with .rc) names the place of a bad file"""
        rc = self.lib.lra_genome_read_host(self.h) if self.ctx is None else self.lib.lra_genome_read_device(self.h, self.ctx.h)
        if rc != 0:
            e = IOError("%s failed (%d): %s" % ("lra_genome_read_host" if self.ctx is None else "lra_genome_read_device", rc, self.last_error()))
            e.rc = rc
            raise e
        n, nl, total = C.c_int32(0), C.c_uint64(0), C.c_uint64(0)
        assert self.lib.lra_genome_info(self.h, C.byref(n), C.byref(nl), C.byref(total)) == 0
        names = C.create_string_buffer(max(1, nl.value))
        pos = np.zeros(n.value + 1, np.uint64)
        assert self.lib.lra_genome_names(self.h, names, C.c_void_p(pos.ctypes.data)) == 0
        self.names = names.raw[:nl.value].split(b"\0")[:n.value]
        self.chrom_pos = [int(x) for x in pos]
        if self.ctx is None:
            p = self.lib.lra_genome_host_seq(self.h)
            self.padded = np.ctypeslib.as_array((C.c_uint8 * (total.value + 64)).from_address(p)).copy()   # (the reader owns its array)
        else:
            import torch
            self.padded = self.ctx.to_tensor(self.lib.lra_genome_device_seq(self.h), total.value + 64, torch.uint8)
        self.seq = self.padded[:total.value]
        return self

    def install(self, ctx):
        """lra_genome_install: the genome and the chromosome table into ctx, from what the reader holds"""
        ctx.check(self.lib.lra_genome_install(self.h, ctx.h))

    def close(self):
        if self.h:
            self.lib.lra_genome_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
