"""tools/map_files.py --bam: the file is BGZF members with the EOF member at the end; decoded by tests/bam_text.py, header and records are the plain
--device-records run's SAM file; the project's own BAM reader takes it, on the host and on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_text
from lra_amd import bgzf, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_files_bam_holds_the_plain_runs_sam(ctx, tmp_path):
    from lra_amd import reads_io
    rng = np.random.default_rng(21)
    genome = synth.make_genome(120_000, seed=5, repeat_frac=0.1, n_families=2)
    with open(tmp_path / "g.fa", "wb") as f:
        f.write(b">chr1 test\n" + genome.tobytes() + b"\n")
    with open(tmp_path / "r.fq", "wb") as f:
        for i, a in enumerate((5000, 40_000, 80_000)):
            r = synth.simulate_read(rng, genome[a:a + 4001], 4000, 0.08, (30, 35, 35), i == 1)[0].tobytes()
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, bytes(rng.integers(34, 74, len(r)).astype(np.uint8))))

    def run(out, extra):
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_files.py"), "-ONT", str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), "--printMD", "-o", out] + extra,
                       check=True, cwd=ROOT, stderr=subprocess.DEVNULL)
        return open(out, "rb").read()

    sam = run(str(tmp_path / "plain.sam"), ["--device-records"])
    z = run(str(tmp_path / "out.bam"), ["--bam"])
    assert z[:4] == b"\x1f\x8b\x08\x04" and z.endswith(bgzf.EOF_BLOCK) and bgzf.blocks(z)[0][-1] == len(z)
    raw = bam_text.inflate(z)
    text, refs, at = bam_text.parse_header(raw)
    assert refs == [(b"chr1", len(genome))]
    lines = sam.split(b"\n")[:-1]
    head = [l for l in lines if l.startswith(b"@")]
    assert text == b"".join(l + b"\n" for l in head) and len(head) == 2        # (the @PG line's CL is the lra command line: the same for both runs)
    recs = [l for l in lines if not l.startswith(b"@")]
    got = [l for _, _, l in bam_text.records(raw, refs, at)]
    assert got == recs and [l.split(b"\t")[0] for l in got if not int(l.split(b"\t")[1]) & 0x900] == [b"r0", b"r1", b"r2"]
    assert all(b"\tMD:Z:" in l for l in got)

    def batch(path, dev):
        rf = reads_io.ReadsFile([path], ctx=ctx if dev else None)
        b = rf.next_batch(10 ** 9)
        rf.close()
        return b["names"], [bytes(s) for s in b["seqs"]], b["quals"]

    for dev in (False, True):
        names, seqs, quals = batch(str(tmp_path / "out.bam"), dev)
        assert (names, seqs, quals) == batch(str(tmp_path / "plain.sam"), dev)
        assert names == [l.split(b"\t")[0] for l in recs] and len(names) >= 3
