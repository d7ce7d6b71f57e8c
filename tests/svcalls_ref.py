"""The assembly-SV oracle: the one-haplotype half of the reference's call_assembly_SVs pipeline as plain Python over vcf_ref.py's variants -- the
snakefile's rules parseAlignment (ParseAlignment.py), CallSV (SamToVCF.py: vcf_ref), FilterBySizeAndSVTYPE, FilterByCentromereAndAltChromAndAddID and
mergeCalls (bedtools intersect -wao, the awk test, mergeSV.py).  Input is a coordinate-sorted file's records; output the merged DEL and INS tables.

A record is vcf_ref's tuple; its core (ref, pos, tlen) comes with it, since the contained filter reads the stored TLEN.  Intervals are 0-based, half-open."""
import struct

import vcf_ref as vr


def core_of(r):
    """a BAM record's bytes (block_size included) -> (refID, pos, tlen)"""
    ref, pos = struct.unpack_from("<ii", r, 4)
    (tlen,) = struct.unpack_from("<i", r, 32)
    return ref, pos, tlen


def contained(cores):
    """ParseAlignment.py over the records with refID >= 0, in file order -> [dropped?] for every record.  e = pos + 1 + tlen; the first record of a run of
    equal refID is kept; a record is dropped when e <= the largest e of the earlier records of its run (equal ends drop).  Records with refID < 0 are no
    part of it: never dropped, and they do not part a run."""
    out, last, top = [], None, 0
    for ref, pos, tlen in cores:
        if ref < 0:
            out.append(False)
            continue
        e = pos + 1 + tlen
        if last is not None and ref == last and e <= top:
            out.append(True)
            continue
        top = e if last is None or ref != last else max(top, e)
        last = ref
        out.append(False)
    return out


def contained_script(cores):
    """the script's own loop, line for line (current_end moves only when a record is kept or the chromosome changes), over records that all have refID >= 0:
    what tests compare `contained` with"""
    remove = [False] * len(cores)
    end = lambda i: cores[i][2] + cores[i][1] + 1
    current_end = end(0)
    for i in range(1, len(cores)):
        if cores[i - 1][0] == cores[i][0]:
            if end(i) <= current_end:
                remove[i] = True
            else:
                current_end = end(i)
        else:
            current_end = end(i)
    return remove


def masked(ref, start, end, mask):
    """bedtools intersect -v: the row shares at least one base with an interval (ref, beg, end) of its reference; touching is no overlap"""
    return any(m[0] == ref and start < m[2] and m[1] < end for m in mask)


def related(a, b):
    """the awk of mergeCalls for the pair (first row a, second row b) of (start, end): ov / len_a >= 0.1 && ov / len_b > 0.1, in integers.  bedtools -wao
    reports ov = min(end) - max(start) when it is positive.  10 ov >= len is the double test exactly: a quotient that is not 1/10 differs from it by at
    least 1 / (10 len), far above an ulp, and ov / len == 0.1 in doubles exactly when 10 ov == len (ov / len is the correctly rounded quotient of two
    integers below 2^53, and so is the literal 0.1 of 1 / 10)."""
    ov = min(a[1], b[1]) - max(a[0], b[0])
    return ov > 0 and 10 * ov >= a[1] - a[0] and 10 * ov > b[1] - b[0]


def merge(rows):
    """mergeSV.py over rows [(ref, start, end)] in NR order -> [kept?].  A row is dropped when an earlier KEPT row of its reference is related to it (the
    script adds a kept row's partners to `seen`; a dropped row adds nothing)."""
    keep = []
    for i, r in enumerate(rows):
        keep.append(not any(keep[k] and rows[k][0] == r[0] and related(rows[k][1:], r[1:]) for k in range(i)))
    return keep


def calls(recs, cores, names, genome, mask=(), require=0, exclude=0x4, min_mapq=0, min_size=40, drop_contained=True, aligner=b"aligner", hap=b"maternal",
          region=None):
    """the pass -> {"DEL": (text, rows), "INS": (text, rows), "stats": {...}}.  rows: [(ref, start, end, nr, svlen, qstart, kind 0 INS / 1 DEL, strand, the
    record's index)] of the kept rows in NR order; text: their lines  RNAME START END ID REF ALT 60 PASS INFO GT 1/1.  region: a reference's index (the whole
    reference): NR starts at 1."""
    min_size = max(int(min_size), 1)
    drop = contained(cores) if drop_contained else [False] * len(recs)
    st = {"contained": 0, "walked": 0, "small": [0, 0], "masked": [0, 0], "merged": [0, 0], "kept": [0, 0]}
    cand = {0: [], 1: []}
    for k, rec in enumerate(recs):
        if region is not None and rec[0] != region:
            continue
        if drop[k]:
            st["contained"] += 1
            continue
        if vr.walked(rec, require, exclude, min_mapq) != "walked":
            continue
        st["walked"] += 1
        for v in vr.variants(rec, genome, 1):
            kind = 0 if v[0] == "INS" else 1
            svlen = len(v[3]) - len(v[2])
            if abs(svlen) < min_size:
                st["small"][kind] += 1
                continue
            start, end = v[1], v[1] + abs(svlen)
            if masked(rec[0], start, end, mask):
                st["masked"][kind] += 1
                continue
            cand[kind].append((rec, v, (rec[0], start, end, len(cand[kind]) + 1, svlen, v[4], kind, 1 if rec[2] & 16 else 0, k)))
    out = {"stats": st}
    for kind, word in ((1, b"DEL"), (0, b"INS")):
        keep = merge([c[2][:3] for c in cand[kind]])
        text, rows = [], []
        for (rec, v, row), kp in zip(cand[kind], keep):
            st["kept" if kp else "merged"][kind] += 1
            if not kp:
                continue
            f = vr.line(names, rec, v).split(b"\t")                                 # REF, ALT and INFO are lra_bam_vcf's bytes
            ident = b"%s.%s.%s.%d" % (aligner, word, hap, row[3])
            text.append(b"\t".join([f[0], b"%d" % row[1], b"%d" % row[2], ident] + f[3:]))
            rows.append(row)
        out[word.decode()] = (b"".join(text), rows)
    return out
