"""lra_bam_svcalls end to end and tools/svcalls_bam.py: reads with planted 50 - 80 base indels, and one read nested inside another, are mapped to a sorted BAM
by tools/map_files.py; the tool's two tables equal tests/svcalls_ref.py's over the records parsed from that file, hold every planted indel once -- the nested
read's copies are not called again -- and --vcf, --chrom, --mask, --one-based and --no-drop-contained do what the oracle does."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_text                                                                   # noqa: E402
import svcalls_ref as sr                                                          # noqa: E402
import vcf_ref as vr                                                              # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES, REF_LEN = [b"chr1", b"chr2"], [70_000, 50_000]
DEL_AT, DEL_LEN, INS_AT = 1200, (60, 53, 78, 67), 2600
INS_LEN = (50, 80, 61, 74)


def tool(name, argv, ok=True):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + [str(a) for a in argv], cwd=ROOT, capture_output=True, timeout=600)
    assert (p.returncode == 0) == ok, p.stderr.decode()[-2000:]
    return p.stdout, p.stderr


@pytest.fixture(scope="module")
def mapped(tmp_path_factory):
    """-> the paths of the genome and the sorted BAM, the genome per chromosome, the oracle's records and cores in file order, the planted indels"""
    from lra_amd import synth
    tmp = tmp_path_factory.mktemp("svcalls")
    rng = np.random.default_rng(34)
    genome = synth.make_genome(120_000, seed=5, repeat_frac=0.1, n_families=2)
    fa = tmp / "g.fa"
    with open(fa, "wb") as f:
        f.write(b">chr1 test\n" + genome[:70_000].tobytes() + b"\n>chr2\n" + genome[70_000:].tobytes() + b"\n")
    planted = []
    with open(tmp / "r.fq", "wb") as f:
        def put(name, seq, rev):
            r = synth.simulate_read(rng, seq, len(seq) - 1, 0.02, (30, 35, 35), rev)[0].tobytes()
            f.write(b"@%s\n%s\n+\n%s\n" % (name, r, bytes(rng.integers(34, 74, len(r)).astype(np.uint8))))
        for i, a in enumerate((80_000, 40_000, 5000, 100_000)):
            src = genome[a:a + 4000]
            ins = synth.BASES[rng.integers(0, 4, INS_LEN[i])]
            mod = np.concatenate([src[:DEL_AT], src[DEL_AT + DEL_LEN[i]:INS_AT], ins, src[INS_AT:]])
            put(b"r%d" % i, mod, i == 1)
            if i == 2:
                put(b"nested", mod[600:3400], False)                               # the same haplotype again, inside r2: both of r2's indels
            ref, off = (0, a) if a < 70_000 else (1, a - 70_000)
            planted += [(ref, off + DEL_AT - 1, -DEL_LEN[i]), (ref, off + INS_AT - 1, INS_LEN[i])]
    bam = tmp / "out.bam"
    tool("map_files.py", ["-ONT", fa, tmp / "r.fq", "--bam", "--sort", "-o", bam])
    raw = bam_text.inflate(open(bam, "rb").read())
    _, refs, at = bam_text.parse_header(raw)
    assert refs == list(zip(NAMES, REF_LEN))
    recs, cores = [], []
    while at < len(raw):
        (bs,) = struct.unpack_from("<I", raw, at)
        recs.append(vr.parse_record(raw[at:at + 4 + bs], bam_text._tags))
        cores.append(sr.core_of(raw[at:at + 4 + bs]))
        at += 4 + bs
    return str(fa), str(bam), [genome[:70_000].tobytes(), genome[70_000:].tobytes()], recs, cores, planted


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_tool_end_to_end(mapped, tmp_path):
    fa, bam, genome, recs, cores, planted = mapped
    want = sr.calls(recs, cores, NAMES, genome)
    assert want["stats"]["contained"] >= 1 and want["stats"]["walked"] >= 4        # the nested read's alignment lies inside r2's
    pre = tmp_path / "calls"
    tool("svcalls_bam.py", [bam, "--ref", fa, "-o", pre])
    assert read("%s.DEL.merge.vcf" % pre) == want["DEL"][0] and read("%s.INS.merge.vcf" % pre) == want["INS"][0]
    rows = want["DEL"][1] + want["INS"][1]
    for ref, pos, svlen in planted:                                                # every planted indel is called once
        hits = [r for r in rows if r[0] == ref and abs(r[1] - pos) <= 60 and abs(r[4] - svlen) <= 6]
        assert len(hits) == 1, (ref, pos, svlen, rows)
    assert len(rows) == len(planted)
    # with the nested read's alignment kept its calls are made again, and merged away; the mask drops what it shares a base with, and unknown names are ignored
    d0 = want["DEL"][1][0]
    with open(tmp_path / "mask.bed", "wb") as f:
        f.write(b"track name=centromeres\n%s\t%d\t%d\tcen\nchrUn_1\t0\t1000\n%s\t%d\t%d\n" % (NAMES[d0[0]], d0[2] - 1, d0[2] + 500, NAMES[d0[0]], d0[2], d0[2] + 10))
    loose = sr.calls(recs, cores, NAMES, genome, drop_contained=False, mask=[(d0[0], d0[2] - 1, d0[2] + 500)])
    assert loose["stats"]["walked"] == want["stats"]["walked"] + want["stats"]["contained"] and loose["stats"]["masked"][1] >= 1
    assert loose["stats"]["merged"][0] + loose["stats"]["merged"][1] >= 1
    tool("svcalls_bam.py", [bam, "--ref", fa, "-o", pre, "--no-drop-contained", "--mask", tmp_path / "mask.bed"])
    assert read("%s.DEL.merge.vcf" % pre) == loose["DEL"][0] and read("%s.INS.merge.vcf" % pre) == loose["INS"][0]


def test_tool_vcf_and_chrom(mapped, tmp_path):
    """--vcf: the header, ten columns, the ID third, no END, a reference's DEL calls in front of its INS calls; --chrom numbers from 1; --one-based shifts POS"""
    from lra_amd.bam import vcf_header
    fa, bam, genome, recs, cores, planted = mapped
    pre = tmp_path / "calls"
    tool("svcalls_bam.py", [bam, "--ref", fa, "-o", pre, "--vcf", "--sample", "HG002", "--aligner", "lra", "--hap", "paternal", "--minSize", "45", "--chrom", "chr2", "--one-based",
                            "--window", "65536"])
    w = sr.calls(recs, cores, NAMES, genome, min_size=45, aligner=b"lra", hap=b"paternal", region=1)
    lines = []
    for k in ("DEL", "INS"):
        for ln in w[k][0].split(b"\n")[:-1]:
            f = ln.split(b"\t")
            lines.append(b"\t".join([f[0], b"%d" % (int(f[1]) + 1), f[3]] + f[4:]) + b"\n")
    assert read("%s.vcf" % pre) == vcf_header(fa, NAMES, REF_LEN, "HG002") + b"".join(lines) and lines and all(ln.count(b"\t") == 9 for ln in lines)
    assert b"\tlra.DEL.paternal.1\t" in lines[0] and lines[0].startswith(b"chr2\t")
    os.rename(bam + ".bai", bam + ".bai.away")
    try:
        assert b"has no index" in tool("svcalls_bam.py", [bam, "--ref", fa, "-o", pre, "--chrom", "chr1"], ok=False)[1]
    finally:
        os.rename(bam + ".bai.away", bam + ".bai")


def test_vcf_bam_drop_contained(mapped):
    """tools/vcf_bam.py --drop-contained: the lines of the records the filter keeps"""
    from lra_amd.bam import vcf_header
    fa, bam, genome, recs, cores, planted = mapped
    drop = sr.contained(cores)
    assert any(drop)
    head = vcf_header(fa, NAMES, REF_LEN)
    assert tool("vcf_bam.py", [bam, "--ref", fa, "--drop-contained"])[0] == head + vr.call([r for r, d in zip(recs, drop) if not d], NAMES, genome)[0]
    want = vr.call([r for r, d in zip(recs, drop) if not d], NAMES, genome, min_length=40, region=(0, 0, REF_LEN[0]))[0]
    assert tool("vcf_bam.py", [bam, "--ref", fa, "--drop-contained", "--chrom", "chr1", "--minLength", "40"])[0] == head + want and want
    assert b"begins at 0" in tool("vcf_bam.py", [bam, "--ref", fa, "--drop-contained", "chr1:500-900"], ok=False)[1]
