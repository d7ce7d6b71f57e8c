"""lra_sv_combine end to end and tools/svcombine_bam.py: two haplotypes' reads with planted 50 - 80 base indels -- shared, maternal only, paternal only -- are
mapped to two sorted BAMs by tools/map_files.py; the tool's seven files equal tests/svcombine_ref.py's over the records parsed from those files, and every
planted indel lies in the class it was planted for."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_text                                                                   # noqa: E402
import svcalls_ref as sr                                                          # noqa: E402
import svcombine_ref as cr                                                        # noqa: E402
import vcf_ref as vr                                                              # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES, REF_LEN = [b"chr1", b"chr2"], [70_000, 50_000]
AT = (80_000, 40_000, 5000, 100_000)                                            # four regions of 4000 bases, each with room for a deletion and an insertion
DEL_AT, DEL_LEN, INS_AT, INS_LEN = 1200, (60, 53, 78, 67), 2600, (50, 80, 61, 74)
# region -> which of (DEL, INS) each haplotype carries: region 0 shared, 1 maternal only, 2 the deletion maternal and the insertion paternal, 3 paternal only
CARRIES = {"maternal": ((1, 1), (1, 1), (1, 0), (0, 0)), "paternal": ((1, 1), (0, 0), (0, 1), (1, 1))}


def tool(name, argv, ok=True):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + [str(a) for a in argv], cwd=ROOT, capture_output=True, timeout=600)
    assert (p.returncode == 0) == ok, p.stderr.decode()[-2000:]
    return p.stdout, p.stderr


def records(bam):
    raw = bam_text.inflate(open(bam, "rb").read())
    _, refs, at = bam_text.parse_header(raw)
    assert refs == list(zip(NAMES, REF_LEN))
    recs, cores = [], []
    while at < len(raw):
        (bs,) = struct.unpack_from("<I", raw, at)
        recs.append(vr.parse_record(raw[at:at + 4 + bs], bam_text._tags))
        cores.append(sr.core_of(raw[at:at + 4 + bs]))
        at += 4 + bs
    return recs, cores


@pytest.fixture(scope="module")
def mapped(tmp_path_factory):
    """-> the genome's path, the two sorted BAMs' paths, the genome per chromosome, each haplotype's (records, cores), the planted indels by class"""
    from lra_amd import synth
    tmp = tmp_path_factory.mktemp("svcombine")
    rng = np.random.default_rng(35)
    genome = synth.make_genome(120_000, seed=5, repeat_frac=0.1, n_families=2)
    fa = tmp / "g.fa"
    with open(fa, "wb") as f:
        f.write(b">chr1 test\n" + genome[:70_000].tobytes() + b"\n>chr2\n" + genome[70_000:].tobytes() + b"\n")
    inserted = [synth.BASES[rng.integers(0, 4, n)] for n in INS_LEN]
    bams, planted = {}, {}
    for hap in ("maternal", "paternal"):
        with open(tmp / (hap + ".fq"), "wb") as f:
            for i, a in enumerate(AT):
                src = genome[a:a + 4000]
                has_del, has_ins = CARRIES[hap][i]
                mod = np.concatenate([src[:DEL_AT], src[DEL_AT + (DEL_LEN[i] if has_del else 0):INS_AT], inserted[i] if has_ins else src[:0], src[INS_AT:]])
                r = synth.simulate_read(rng, mod, len(mod) - 1, 0.02, (30, 35, 35), i == 1)[0].tobytes()
                f.write(b"@%s%d\n%s\n+\n%s\n" % (hap[0].encode(), i, r, bytes(rng.integers(34, 74, len(r)).astype(np.uint8))))
        bams[hap] = str(tmp / (hap + ".bam"))
        tool("map_files.py", ["-ONT", fa, tmp / (hap + ".fq"), "--bam", "--sort", "-o", bams[hap]])
    for i, a in enumerate(AT):
        ref, off = (0, a) if a < 70_000 else (1, a - 70_000)
        for which, (pos, svlen) in enumerate(((off + DEL_AT - 1, -DEL_LEN[i]), (off + INS_AT - 1, INS_LEN[i]))):
            m, p = CARRIES["maternal"][i][which], CARRIES["paternal"][i][which]
            if m or p:
                planted.setdefault(("maternal", "hom") if m and p else ("maternal", "het") if m else ("paternal", "het"), []).append((ref, pos, svlen))
    return str(fa), bams, [genome[:70_000].tobytes(), genome[70_000:].tobytes()], {h: records(bams[h]) for h in bams}, planted


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_tool_end_to_end(mapped, tmp_path):
    from lra_amd.bam import SVCOMBINE_FILES, vcf_header
    fa, bams, genome, recs, planted = mapped
    want, wst, wm, wp = cr.run(*recs["maternal"], *recs["paternal"], NAMES, genome)
    by = {w[:3]: w for w in want}
    assert len(by) == 6                                                            # every class has rows
    pre = tmp_path / "calls"
    tool("svcombine_bam.py", [bams["maternal"], bams["paternal"], "--ref", fa, "--sample", "HG002", "-o", pre])
    for key, suffix in SVCOMBINE_FILES:
        assert read(str(pre) + suffix) == by[key][3], key
    assert read(str(pre) + ".vcf") == vcf_header(fa, NAMES, REF_LEN, "HG002") + b"".join(by[key][3] for key, _ in SVCOMBINE_FILES)
    # every planted indel is called once, in its class; a shared one is printed once, with its maternal ID
    for (hap, cls), indels in planted.items():
        rows = [r for w in want if w[0] == hap and w[2] == cls for r in w[4]]
        assert len(rows) == len(indels), (hap, cls, rows)
        for ref, pos, svlen in indels:
            assert len([r for r in rows if r[0] == ref and abs(r[1] - pos) <= 60 and abs(r[4] - svlen) <= 6]) == 1, (hap, cls, ref, pos, svlen, rows)
    assert wst["partnered_p"] == [1, 1] and all(b".maternal." in ln.split(b"\t")[2] for k in ("INS", "DEL") for ln in by["maternal", k, "hom"][3].split(b"\n")[:-1])


def test_tool_options(mapped, tmp_path):
    """--frac 1/10 --pass-filter is combinehapSV.snakefile's output; --chrom numbers from 1 and leaves the other reference's classes empty; --one-based, --aligner,
    --minSize, --mask"""
    from lra_amd.bam import SVCOMBINE_FILES
    fa, bams, genome, recs, planted = mapped
    pre = tmp_path / "opt"
    with open(tmp_path / "mask.bed", "wb") as f:
        f.write(b"chr2\t0\t12000\n")                                                # region 0 (chr2:10000) goes; region 3 (chr2:30000) stays
    tool("svcombine_bam.py", [bams["maternal"], bams["paternal"], "--ref", fa, "-o", pre, "--frac", "1/10", "--pass-filter", "--chrom", "chr2", "--one-based", "--aligner", "lra",
                              "--minSize", "45", "--mask", tmp_path / "mask.bed", "--window", "65536"])
    want, wst, wm, wp = cr.run(*recs["maternal"], *recs["paternal"], NAMES, genome, 1, 10, True, True, min_size=45, aligner=b"lra", region=1, mask=[(1, 0, 12000)])
    by = {w[:3]: w[3] for w in want}
    assert by and all(r[0] == 1 for w in want for r in w[4])
    for key, suffix in SVCOMBINE_FILES:
        assert read(str(pre) + suffix) == by.get(key, b""), key
    text = b"".join(by.values())
    assert b"\tPASS\tSVTYPE=" in text and b"\tlra.DEL.paternal.1\t" in text and wm["stats"]["masked"][0] + wm["stats"]["masked"][1] >= 1


def test_tool_refusals(mapped, tmp_path):
    """a file that is no BAM is refused with nothing written; a fraction that is none is refused before anything is opened"""
    fa, bams, genome, recs, planted = mapped
    bad = tmp_path / "bad"
    err = tool("svcombine_bam.py", [bams["maternal"], fa, "--ref", fa, "-o", bad], ok=False)[1]
    assert b"is not a BAM file" in err and not os.path.exists(str(bad) + ".vcf")
    assert b"fraction" in tool("svcombine_bam.py", [bams["maternal"], bams["paternal"], "--ref", fa, "-o", bad, "--frac", "4/3"], ok=False)[1]
