"""The record front of the BAM passes (bam_pass.h): lra_bam_view, lra_bam_depth, lra_bam_vcf and lra_bam_svcalls select the same records of a region.  One
crafted coordinate-sorted file, every record a single M op with l_seq = the op's length, so that no consumer skips or refuses one for reasons of its own;
records at every edge the shared region test decides; the counts of the four consumers against a count made here from the crafted coordinates."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bam_vcf_device as tv                                                  # noqa: E402  (the builders: rec, op, indexed_file, genome_of, load)

pytestmark = pytest.mark.gpu

REF_LEN = [300_000, 80_000]
BEG, END = 40_000, 200_000                                                        # the region on reference 0
L = 1000                                                                          # an op's length: 1.5 KB of SEQ and QUAL a record, the file's padding
WINDOW = 65536                                                                    # the pass's smallest window


def crafted():
    """[(ref, pos, span)], unsorted: fillers over both references and the edge records"""
    out = [(0, 1000 + 1500 * i, L) for i in range(150)]                           # reference 0 from 1000 to 225 500: in front of, inside and behind the region
    out += [(0, BEG - L, L),                                                      # its span ends exactly at beg: out
            (0, BEG - L + 1, L),                                                  # ends at beg + 1: in
            (0, BEG - 1, 1), (0, BEG, 1), (0, BEG - 2, 2), (0, BEG - 2, 3),       # one-base and two-base records around beg: in, in, out, in
            (0, END - 1, L), (0, END - 1, 1),                                     # start at end - 1: in
            (0, END, L), (0, END, 1),                                             # start at end: out; the first of them in file order is the stop record
            (0, END - L, L), (0, END - L - 1, L + 2),                             # end at end, reach over it: in
            (0, 0, 5), (0, REF_LEN[0] - 7, 7)]                                    # the reference's first and last bases
    out += [(1, 100 + 1500 * i, L) for i in range(50)]                            # the next reference, behind reference 0 in the same members
    out += [(1, 0, 3), (1, REF_LEN[1] - L, L), (1, REF_LEN[1] - 1, 1)]            # the edges of a whole-reference region
    return out


@pytest.fixture(scope="module")
def front(tmp_path_factory):
    """the context with the genome, the file with its .bai, the sorted (ref, pos, span) list with the refID -1 tail"""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from lra_amd.context import Context
    rng = np.random.default_rng(11)
    coords = crafted()
    recs = [tv.rec(ref=r, pos=p, name=b"c%03d" % k, ops=[tv.op(n, "M")], rng=rng) for k, (r, p, n) in enumerate(coords)]
    recs += [tv.rec(ref=-1, pos=-1, flag=4, name=b"u%d" % k, ops=[tv.op(L, "M")], rng=rng) for k in range(5)]
    assert 200 <= len(recs) <= 230
    bam, bai, recs = tv.indexed_file(tmp_path_factory.mktemp("front"), "f.bam", recs, REF_LEN, level=0)
    ctx = Context(0)
    tv.load(ctx, tv.genome_of(REF_LEN))
    yield ctx, bam, bai, coords
    ctx.close()


def expected(coords, ref, beg, end):
    return sum(1 for r, p, n in coords if r == ref and p < end and p + n > beg)


def counts(ctx, bam, bai, ref, beg, end, svcalls):
    """the records each consumer selected for [beg, end) of ref, and the windows each pass read"""
    from lra_amd.bam import BamDepth, BamSvCalls, BamVcf, BamView
    got, windows = {}, {}
    v = BamView(ctx, bam, bai, window_bytes=WINDOW)
    try:
        for _ in v.fetch(ref, beg, end):
            pass
        got["view"], windows["view"] = v.last_records, v.stats()["windows"]
    finally:
        v.close()
    d = BamDepth(ctx, bam, bai, exclude=0, min_mapq=0, window_bytes=WINDOW)
    try:
        for _ in d.fetch(ref, beg, end):
            pass
        st = d.stats()
        got["depth"], windows["depth"] = st["records_counted"], st["windows"]
    finally:
        d.close()
    c = BamVcf(ctx, bam, bai, exclude=0, min_mapq=0, drop_contained=False, window_bytes=WINDOW)
    try:
        for _ in c.fetch(ref, beg, end):
            pass
        st = c.stats()
        got["vcf"], windows["vcf"] = st["records_walked"] + st["records_skipped"], st["windows"]
    finally:
        c.close()
    if svcalls:
        s = BamSvCalls(ctx, bam, bai, exclude=0, min_mapq=0, drop_contained=False, window_bytes=WINDOW)
        try:
            for _ in s.fetch(ref):
                pass
            st = s.stats()
            got["svcalls"], windows["svcalls"] = st["records_walked"], st["windows"]
        finally:
            s.close()
    return got, windows


def test_region_on_reference_0(front):
    ctx, bam, bai, coords = front
    want = expected(coords, 0, BEG, END)
    assert 100 < want < len(coords)                                               # (records in front of the region, inside it and behind it)
    got, windows = counts(ctx, bam, bai, 0, BEG, END, svcalls=False)
    print(want, got, windows)
    assert got == {"view": want, "depth": want, "vcf": want}
    assert min(windows.values()) >= 2                                             # the region spans windows: the stop record is not in the first


def test_whole_reference_1(front):
    ctx, bam, bai, coords = front
    want = expected(coords, 1, 0, REF_LEN[1])
    assert want == sum(1 for r, _, _ in coords if r == 1)
    got, windows = counts(ctx, bam, bai, 1, 0, None, svcalls=True)                # reference 0 in front of it in the chunk, the refID -1 tail behind it
    print(want, got, windows)
    assert got == {"view": want, "depth": want, "vcf": want, "svcalls": want}
