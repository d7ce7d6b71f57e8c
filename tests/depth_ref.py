"""The depth oracle: include/lra_hip.h's rules for lra_bam_depth written as a loop.  Records are (ref, pos, flag, mapq, ops) with ops the uint32 CIGAR
values that count (the CG:B:I tag's for a record in that form)."""
import numpy as np

COVER = {0, 7, 8}                                                                 # M = X
ADVANCE = {0, 2, 3, 7, 8}                                                         # M D N = X


def depth(recs, ref_len, require=0, exclude=0x704, min_mapq=0, count_deletions=False):
    """-> one uint32 array per reference"""
    out = [np.zeros(n, dtype=np.int64) for n in ref_len]
    for ref, pos, flag, mapq, ops in recs:
        if ref < 0 or (flag & require) != require or (flag & exclude) or mapq < min_mapq:
            continue
        at = pos
        for o in ops:
            n, code = int(o) >> 4, int(o) & 15
            if code in COVER or (code == 2 and count_deletions):
                out[ref][max(at, 0):max(at + n, 0)] += 1
            if code in ADVANCE:
                at += n
    return [a.astype(np.uint32) for a in out]


def base_text(name, d, beg, end, all_positions=False):
    """the per-base lines of positions [beg, end) of one reference's depths d"""
    at = range(beg, end) if all_positions else (np.nonzero(d[beg:end])[0] + beg)
    return b"".join(b"%s\t%d\t%d\n" % (name, p + 1, d[p]) for p in at)


def bin_sums(d, beg, end, bin_):
    return [int(d[a:min(a + bin_, end)].astype(np.uint64).sum()) for a in range(beg, end, bin_)]


def bin_text(name, d, beg, end, bin_):
    out = []
    for k, s in enumerate(bin_sums(d, beg, end, bin_)):
        a = beg + k * bin_
        b = min(a + bin_, end)
        h = (100 * s + (b - a) // 2) // (b - a)
        out.append(b"%s\t%d\t%d\t%d.%02d\n" % (name, a, b, h // 100, h % 100))
    return b"".join(out)
