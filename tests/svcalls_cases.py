"""What the device tests of the contained filter and of lra_bam_svcalls share: crafted BAM records that carry a TLEN (the contained filter reads the stored
field), files with and without an index, a context's genome, and the oracle's view of a file (vcf_ref's tuples and svcalls_ref's cores)."""
import ctypes
import os
import struct

import numpy as np

import bai_text as bt
import bam_merge_cases as mc
import bam_text
import svcalls_ref as sr
import vcf_ref as vr

NAMES = [b"chr%d" % (i + 1) for i in range(8)]
CODE = {c: k for k, c in enumerate("MIDNSHP=X")}
Q_OPS, R_OPS = {0, 1, 4, 7, 8}, {0, 2, 3, 7, 8}


def cig(text):
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n) << 4) | CODE[ch])
            n = ""
    return out


def bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def rec(ref=0, pos=100, tlen=0, flag=0, name=b"r", ops=(), seq=None, mapq=60, rng=None):
    """a record with a real SEQ and the TLEN given.  ops: a CIGAR string or the uint32 values"""
    ops = cig(ops) if isinstance(ops, str) else list(ops)
    if seq is None:
        seq = bases(rng or np.random.default_rng(len(name) + pos), sum(o >> 4 for o in ops if (o & 15) in Q_OPS))
    span = sum(o >> 4 for o in ops if (o & 15) in R_OPS)
    bin_ = 4680 if ref < 0 else bt.reg2bin(pos, pos + max(span, 1))
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, mapq, bin_, len(ops), flag, len(seq), -1, -1, tlen) + name + b"\0"
    body += struct.pack("<%dI" % len(ops), *ops) + vr.pack_seq(seq) + b"\xff" * len(seq)
    return struct.pack("<I", len(body)) + body


def parse(r):
    return vr.parse_record(r, bam_text._tags)


def genome_of(ref_len, seed=3):
    rng = np.random.default_rng(seed)
    return [bases(rng, n) for n in ref_len]


def load(ctx, genome):
    from lra_amd.index import load_genome
    load_genome(ctx, np.frombuffer(b"".join(genome), np.uint8))
    pos = np.concatenate([[0], np.cumsum([len(g) for g in genome])]).astype(np.uint64)
    ctx.check(ctx.lib.lra_ctx_load_chromosomes(ctx.h, (ctypes.c_uint64 * len(pos))(*[int(x) for x in pos]), len(genome)))


def write(tmp_path, name, data):
    p = os.path.join(str(tmp_path), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def plain_file(tmp_path, name, recs, ref_len, level=1):
    """the records in the order given, no index"""
    return write(tmp_path, name, mc.run_bytes(recs, level=level, ref_len=ref_len))


def indexed_file(tmp_path, name, recs, ref_len, level=1):
    """the records in the order given (the caller sorts them: a stable order of equal keys matters to the filter) with a .bai -> (bam, bai)"""
    from lra_amd import bgzf
    raw = b"".join(recs)
    head = bgzf.bgzf_compress(mc.header_bytes(ref_len), 6, eof=False)
    members = [bgzf.bgzf_compress(raw[a:a + bt.MEMBER], level, eof=False) for a in range(0, len(raw), bt.MEMBER)]
    moff = bt.member_table(len(raw), [len(m) for m in members])
    bam = write(tmp_path, name, head + b"".join(members) + mc.EOF_BLOCK)
    bai = write(tmp_path, name + ".bai", bt.build(raw, len(ref_len), moff, len(head)))
    return bam, bai


def vcf_want(recs, genome, drop_contained=True, **kw):
    """lra_bam_vcf's text, values and stats by the oracles: vcf_ref's walk over the records svcalls_ref's filter keeps, `record` counting every record"""
    P = [parse(r) for r in recs]
    drop = sr.contained([sr.core_of(r) for r in recs]) if drop_contained else [False] * len(recs)
    if kw.get("region") is not None:
        drop = [d and p[0] == kw["region"][0] for d, p in zip(drop, P)]              # (the others are filtered, whatever the filter says of them)
    kept = [i for i, d in enumerate(drop) if not d]
    text, vals, st = vr.call([P[i] for i in kept], NAMES, genome, **kw)
    st["contained"] = len(recs) - len(kept)
    return text, [v[:6] + (kept[v[6]],) for v in vals], st
