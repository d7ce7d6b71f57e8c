"""The variant oracle: include/lra_hip.h's rules for lra_bam_vcf written as a walk.  A record is (ref, pos, flag, mapq, ops, seq, name) with ops the uint32
CIGAR values that count (the CG:B:I tag's for a record in that form), seq the decoded SEQ (bytes) and name the QNAME (bytes).  The genome is one bytes
object per reference, upper case."""
import struct

import numpy as np

MATCH, INS, DEL = {0, 7, 8}, {1, 4}, {2, 3}                                       # M = X | I S | D N; H and P yield nothing
SEQ_CODE = b"=ACMGRSVTWYHKDBN"


def walked(rec, require=0, exclude=0x4, min_mapq=0):
    """-> "filtered", "skipped" or "walked" """
    ref, pos, flag, mapq, ops, seq, name = rec
    if ref < 0 or (flag & require) != require or (flag & exclude) or mapq < min_mapq:
        return "filtered"
    if not ops or not seq or not any((o & 15) in MATCH and o >> 4 for o in ops):
        return "skipped"
    return "walked"


def variants(rec, genome, min_length=1):
    """the variants of one walked record, in CIGAR order -> [(kind "INS" / "DEL", anchor position 0-based, REF, ALT, qstart)]"""
    ref, pos, flag, mapq, ops, seq, name = rec
    min_length = max(int(min_length), 1)
    g = genome[ref]
    q, r = 0, pos
    aq = None                                                                     # the SEQ index of the last M = X base
    run, r0 = None, 0                                                             # the run in hand and r where it began
    out = []

    def close():
        if run == INS:
            v = ("INS", r0 - 1, g[r0 - 1:r0], seq[aq:q], aq + 1)
        else:
            v = ("DEL", r0 - 1, g[r0 - 1:r], seq[aq:aq + 1], aq + 1)
        if abs(len(v[3]) - len(v[2])) >= min_length:
            out.append(v)

    for o in ops:
        n, code = int(o) >> 4, int(o) & 15
        kind = MATCH if code in MATCH else INS if code in INS else DEL if code in DEL else None
        if not n or kind is None:
            continue
        if run is not None and kind is not run:                                   # the run is followed by another entry: it is a variant
            close()
            run = None
        if kind is MATCH:
            q += n
            r += n
            aq = q - 1
            continue
        if aq is not None and run is None:                                        # (in front of the first M = X base nothing begins)
            run, r0 = kind, r
        if kind is INS:
            q += n
        else:
            r += n
    return out                                                                    # (a run that reaches the end is none)


def line(names, rec, v, pos_one_based=False):
    kind, anchor, ref_seq, alt, qstart = v
    return b"%s\t%d\t.\t%s\t%s\t60\tPASS\tSVTYPE=%s;SVLEN=%d;QNAME=%s;QSTART=%d;QSTRAND=%s\tGT\t1/1\n" % (
        names[rec[0]], anchor + (1 if pos_one_based else 0), ref_seq, alt, kind.encode(), len(alt) - len(ref_seq), rec[6], qstart, b"-" if rec[2] & 16 else b"+")


def call(recs, names, genome, require=0, exclude=0x4, min_mapq=0, min_length=1, pos_one_based=False, region=None):
    """the pass over recs in order -> (the text, [(ref, anchor, qstart, svlen, kind 0 / 1, strand 0 / 1, the record's index)], {"walked", "skipped", "filtered"}).
    region (ref, beg, end): the variants of that reference's records whose anchor lies in [beg, end)"""
    text, vals, st = [], [], {"walked": 0, "skipped": 0, "filtered": 0}
    for k, rec in enumerate(recs):
        w = walked(rec, require, exclude, min_mapq)
        if region is not None and w != "filtered" and rec[0] != region[0]:
            w = "filtered"
        st[w] += 1
        if w != "walked":
            continue
        for v in variants(rec, genome, min_length):
            if region is not None and not region[1] <= v[1] < region[2]:
                continue
            text.append(line(names, rec, v, pos_one_based))
            vals.append((rec[0], v[1], v[4], len(v[3]) - len(v[2]), 0 if v[0] == "INS" else 1, 1 if rec[2] & 16 else 0, k))
    return b"".join(text), vals, st


def header(reference, names, lens, sample="unknown"):
    """the header lines in front of the variants"""
    s = lambda x: x.decode() if isinstance(x, bytes) else str(x)
    out = ["##fileformat=VCFv4.2", "##fileDate=20190102", "##source=SamToVCF", "##reference=" + s(reference)]
    out += ["##contig=<ID=%s,length=%d>" % (s(n), k) for n, k in zip(names, lens)]
    out += ['##INFO=<ID=QNAME,Number=1,Type=String,Description="Name of query sequence">',
            '##INFO=<ID=QSTART,Number=1,Type=Integer,Description="Position of query sequence">',
            '##INFO=<ID=QSTRAND,Number=1,Type=String,Description="Contig strand">',
            '##INFO=<ID=SVLEN,Number=.,Type=Integer,Description="Difference in length between REF and ALT alleles">',
            '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">',
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + s(sample)]
    return ("\n".join(out) + "\n").encode()


def pack_seq(seq):
    """SEQ as BAM stores it: two bases per byte, the first in the high nibble"""
    code = [SEQ_CODE.index(bytes([c])) for c in seq] + [0]
    return bytes((code[k] << 4) | code[k + 1] for k in range(0, len(seq), 2))


def parse_record(r, tags_of=None):
    """a BAM record's bytes (block_size included) -> the oracle's tuple; tags_of(aux bytes) yields (tag, type, subtype, values) for the CG:B:I form"""
    ref, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", r, 4)
    at = 36 + l_name
    ops = list(struct.unpack_from("<%dI" % n_cig, r, at))
    sq = at + 4 * n_cig
    packed = r[sq:sq + (l_seq + 1) // 2]
    b = np.frombuffer(packed, np.uint8)
    code = np.empty(2 * len(b), np.uint8)
    code[0::2], code[1::2] = b >> 4, b & 15                                        # the first base of a byte is its high nibble
    seq = np.frombuffer(SEQ_CODE, np.uint8)[code[:l_seq]].tobytes()
    if n_cig == 2 and ops[0] == (l_seq << 4 | 4) and (ops[1] & 15) == 3 and tags_of is not None:
        for t in tags_of(r[sq + (l_seq + 1) // 2 + l_seq:]):
            if t[0] == "CG" and t[1] == "B" and t[2].startswith("I"):
                ops = [int(v) for v in t[3]]
                break
    return ref, pos, flag, mapq, ops, seq, r[36:36 + l_name - 1]
