"""tools/depth_bam.py on a file tools/map_files.py --bam --sort wrote: whole and for two regions, per base and --bin 500, against tests/depth_ref.py fed
from tools/view_bam.py's SAM text (POS, FLAG, MAPQ, CIGAR): the CG:B:I form, the = / X runs and the real index together."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref as dr                                                            # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = "MIDNSHP=X"


def tool(name, argv, ok=True):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + [str(a) for a in argv], cwd=ROOT, capture_output=True, timeout=600)
    assert (p.returncode == 0) == ok, p.stderr.decode()[-2000:]
    return p.stdout, p.stderr


def test_depth_of_a_mapped_file(tmp_path):
    from lra_amd import synth
    rng = np.random.default_rng(21)
    genome = synth.make_genome(120_000, seed=5, repeat_frac=0.1, n_families=2)
    with open(tmp_path / "g.fa", "wb") as f:
        f.write(b">chr1 test\n" + genome[:70_000].tobytes() + b"\n>chr2\n" + genome[70_000:].tobytes() + b"\n")
    with open(tmp_path / "r.fq", "wb") as f:
        for i, a in enumerate((80_000, 40_000, 5000, 100_000, 41_000)):
            r = synth.simulate_read(rng, genome[a:a + 4001], 4000, 0.08, (30, 35, 35), i == 1)[0].tobytes()
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, bytes(rng.integers(34, 74, len(r)).astype(np.uint8))))
        f.write(b"@junk\n%s\n+\n%s\n" % (bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000)), b"I" * 3000))
    bam = tmp_path / "out.bam"
    tool("map_files.py", ["-ONT", tmp_path / "g.fa", tmp_path / "r.fq", "--bam", "--sort", "-o", bam])
    names, ref_len = [b"chr1", b"chr2"], [70_000, 50_000]
    recs = []
    for ln in tool("view_bam.py", [bam])[0].splitlines():
        f = ln.split(b"\t")
        ops = [] if f[5] == b"*" else [(int(n) << 4) | CODES.index(c) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", f[5].decode())]
        recs.append((names.index(f[2]) if f[2] != b"*" else -1, int(f[3]) - 1, int(f[1]), int(f[4]), ops))
    assert sum(r[0] >= 0 for r in recs) >= 4 and any(r[0] < 0 for r in recs) and any(len(r[4]) > 100 for r in recs)
    d = dr.depth(recs, ref_len)
    assert d[0].max() >= 1 and d[1].max() >= 1
    assert tool("depth_bam.py", [bam])[0] == b"".join(dr.base_text(names[r], d[r], 0, ref_len[r]) for r in range(2))
    assert tool("depth_bam.py", [bam, "--bin", "500"])[0] == b"".join(dr.bin_text(names[r], d[r], 0, ref_len[r], 500) for r in range(2))
    regions = ["chr1:40,500-42,000", "chr2:10001-31234"]
    want = dr.base_text(names[0], d[0], 40_499, 42_000, True) + dr.base_text(names[1], d[1], 10_000, 31_234, True)
    assert tool("depth_bam.py", [bam] + regions + ["-a", "--window", "65536", "--span", "65536"])[0] == want
    tool("depth_bam.py", [bam] + regions + ["--bin", "500", "-o", tmp_path / "bins.tsv"])
    assert open(tmp_path / "bins.tsv", "rb").read() == dr.bin_text(names[0], d[0], 40_499, 42_000, 500) + dr.bin_text(names[1], d[1], 10_000, 31_234, 500)
    dj = dr.depth(recs, ref_len, count_deletions=True, min_mapq=1)
    assert tool("depth_bam.py", [bam, "-J", "-Q", "1"])[0] == b"".join(dr.base_text(names[r], dj[r], 0, ref_len[r]) for r in range(2))
    os.rename(str(bam) + ".bai", str(bam) + ".bai.away")
    assert b"has no index" in tool("depth_bam.py", [bam, "chr1"], ok=False)[1]
