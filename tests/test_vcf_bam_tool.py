"""lra_bam_vcf end to end and tools/vcf_bam.py: reads with planted 30 - 60 base indels are mapped to a sorted BAM by tools/map_files.py; BamVcf's text
equals tests/vcf_ref.py's walk over the records parsed from that file and holds every planted indel once; the tool prints the header and the same lines,
and honours --chrom, --minLength, a region and --one-based."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_text                                                                   # noqa: E402
import vcf_ref as vr                                                              # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES, REF_LEN = [b"chr1", b"chr2"], [70_000, 50_000]
DEL_AT, DEL_LEN, INS_AT = 1200, (40, 33, 58, 47), 2600
INS_LEN = (50, 60, 31, 44)


def tool(name, argv, ok=True):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + [str(a) for a in argv], cwd=ROOT, capture_output=True, timeout=600)
    assert (p.returncode == 0) == ok, p.stderr.decode()[-2000:]
    return p.stdout, p.stderr


@pytest.fixture(scope="module")
def mapped(tmp_path_factory):
    """-> the paths of the genome and the sorted BAM, the genome per chromosome, the oracle's records in file order, the planted indels"""
    from lra_amd import synth
    tmp = tmp_path_factory.mktemp("vcf")
    rng = np.random.default_rng(33)
    genome = synth.make_genome(120_000, seed=5, repeat_frac=0.1, n_families=2)
    fa = tmp / "g.fa"
    with open(fa, "wb") as f:
        f.write(b">chr1 test\n" + genome[:70_000].tobytes() + b"\n>chr2\n" + genome[70_000:].tobytes() + b"\n")
    planted = []
    with open(tmp / "r.fq", "wb") as f:
        for i, a in enumerate((80_000, 40_000, 5000, 100_000)):
            src = genome[a:a + 4000]
            ins = synth.BASES[rng.integers(0, 4, INS_LEN[i])]
            mod = np.concatenate([src[:DEL_AT], src[DEL_AT + DEL_LEN[i]:INS_AT], ins, src[INS_AT:]])
            r = synth.simulate_read(rng, mod, len(mod) - 1, 0.02, (30, 35, 35), i == 1)[0].tobytes()
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, bytes(rng.integers(34, 74, len(r)).astype(np.uint8))))
            ref, off = (0, a) if a < 70_000 else (1, a - 70_000)
            planted += [(b"r%d" % i, ref, off + DEL_AT - 1, -DEL_LEN[i]), (b"r%d" % i, ref, off + INS_AT - 1, INS_LEN[i])]
    bam = tmp / "out.bam"
    tool("map_files.py", ["-ONT", fa, tmp / "r.fq", "--bam", "--sort", "-o", bam])
    raw = bam_text.inflate(open(bam, "rb").read())
    _, refs, at = bam_text.parse_header(raw)
    assert refs == list(zip(NAMES, REF_LEN))
    recs = []
    while at < len(raw):
        (bs,) = struct.unpack_from("<I", raw, at)
        recs.append(vr.parse_record(raw[at:at + 4 + bs], bam_text._tags))
        at += 4 + bs
    return str(fa), str(bam), [genome[:70_000].tobytes(), genome[70_000:].tobytes()], recs, planted


def test_planted_indels_end_to_end(mapped):
    from lra_amd.bam import BamVcf
    from lra_amd.context import Context
    from lra_amd.genome_io import GenomeFile
    fa, bam, genome, recs, planted = mapped
    want, wvals, wst = vr.call(recs, NAMES, genome)
    assert wst["walked"] >= 4 and len(wvals) > 100
    c = Context(0)
    try:
        g = GenomeFile(fa, c)
        g.read().install(c)
        g.close()
        o = BamVcf(c, bam, bam + ".bai", values=True)
        pieces = [(v.copy(), t) for _, v, t in o.fetch()]
        assert b"".join(t for _, t in pieces) == want
        got = [(int(x["ref_id"]), int(x["pos"]), int(x["qstart"]), int(x["svlen"]), int(x["kind"]), int(x["strand"]), int(x["record"])) for v, _ in pieces for x in v]
        assert got == wvals
        st = o.stats()
        assert (st["records_read"], st["records_walked"], st["records_skipped"]) == (len(recs), wst["walked"], wst["skipped"])
        for ref in range(2):
            assert b"".join(p[2] for p in o.fetch(ref)) == vr.call(recs, NAMES, genome, region=(ref, 0, REF_LEN[ref]))[0]
        o.close()
    finally:
        c.close()
    big = [(recs[k][6], ref, pos, svlen) for ref, pos, _, svlen, _, _, k in wvals if abs(svlen) >= 25]
    for name, ref, pos, svlen in planted:                                          # every planted indel appears once
        hits = [b for b in big if b[0] == name and b[1] == ref and abs(b[2] - pos) <= 60 and abs(b[3] - svlen) <= 6]
        print(name, ref, pos, svlen, hits)
        assert len(hits) == 1, (name, ref, pos, svlen, [b for b in big if b[0] == name])
    assert len(big) == len(planted)


def test_tool(mapped, tmp_path):
    from lra_amd.bam import vcf_header
    fa, bam, genome, recs, planted = mapped
    head = vcf_header(fa, NAMES, REF_LEN)
    assert tool("vcf_bam.py", [bam, "--ref", fa])[0] == head + vr.call(recs, NAMES, genome)[0]
    got = tool("vcf_bam.py", [bam, "--ref", fa, "--chrom", "chr2", "--minLength", "25", "--sample", "HG002"])[0]
    want = vr.call(recs, NAMES, genome, min_length=25, region=(1, 0, REF_LEN[1]))[0]
    assert got == vcf_header(fa, NAMES, REF_LEN, "HG002") + want and want.count(b"\n") == 4 and want.count(b"chr2\t") == 4
    tool("vcf_bam.py", [bam, "--ref", fa, "chr1:40,500-42,000", "chr2:10001-31234", "--one-based", "-o", tmp_path / "o.vcf", "--window", "65536"])
    want = b"".join(vr.call(recs, NAMES, genome, pos_one_based=True, region=r)[0] for r in ((0, 40_499, 42_000), (1, 10_000, 31_234)))
    assert open(tmp_path / "o.vcf", "rb").read() == head + want and want
    assert tool("vcf_bam.py", [bam, "--ref", fa, "-F", "0x14"])[0] == head + vr.call(recs, NAMES, genome, exclude=0x14)[0]
    with open(tmp_path / "short.fa", "wb") as f:
        f.write(b">chr1\n" + genome[0] + b"\n>chr2\n" + genome[1][:-1] + b"\n")
    assert b"reference 1 (chr2): has 50000 bases in the BAM header and 49999 in the genome" in tool("vcf_bam.py", [bam, "--ref", tmp_path / "short.fa"], ok=False)[1]
    os.rename(bam + ".bai", bam + ".bai.away")
    try:
        assert b"has no index" in tool("vcf_bam.py", [bam, "--ref", fa, "--chrom", "chr1"], ok=False)[1]
        assert tool("vcf_bam.py", [bam, "--ref", fa])[0] == head + vr.call(recs, NAMES, genome)[0]   # a whole pass needs no index
    finally:
        os.rename(bam + ".bai.away", bam + ".bai")
