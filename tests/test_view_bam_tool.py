"""tools/view_bam.py on a file tools/map_files.py --bam --sort wrote: the header and every record as tests/bam_text.py prints them, every record found
again through a region of its own interval, the count, the header alone, the flag filters."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_text as bt                                                             # noqa: E402
import bam_text                                                                   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tool(name, argv, ok=True):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + [str(a) for a in argv], cwd=ROOT, capture_output=True, timeout=600)
    assert (p.returncode == 0) == ok, p.stderr.decode()[-2000:]
    return p.stdout, p.stderr


def test_view_of_a_mapped_file(tmp_path):
    from lra_amd import synth
    rng = np.random.default_rng(21)
    genome = synth.make_genome(120_000, seed=5, repeat_frac=0.1, n_families=2)
    with open(tmp_path / "g.fa", "wb") as f:
        f.write(b">chr1 test\n" + genome[:70_000].tobytes() + b"\n>chr2\n" + genome[70_000:].tobytes() + b"\n")
    with open(tmp_path / "r.fq", "wb") as f:
        for i, a in enumerate((80_000, 40_000, 5000, 100_000)):
            r = synth.simulate_read(rng, genome[a:a + 4001], 4000, 0.08, (30, 35, 35), i == 1)[0].tobytes()
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, bytes(rng.integers(34, 74, len(r)).astype(np.uint8))))
        f.write(b"@junk\n%s\n+\n%s\n" % (bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000)), b"I" * 3000))
    bam = tmp_path / "out.bam"
    tool("map_files.py", ["-ONT", tmp_path / "g.fa", tmp_path / "r.fq", "--bam", "--sort", "-o", bam])
    assert os.path.exists(str(bam) + ".bai")

    raw = bam_text.inflate(open(bam, "rb").read())
    text, refs, at = bam_text.parse_header(raw)
    body = raw[at:]
    lines = [ln + b"\n" for _, _, ln in bam_text.records(body, refs)]
    recs = bt.walk(body)
    assert len(lines) >= 5 and any(r["ref"] < 0 for r in recs) and any(r["ref"] >= 0 for r in recs)

    flags = [struct.unpack_from("<H", body, r["at"] + 18)[0] for r in recs]
    assert tool("view_bam.py", [bam, "-h"])[0] == text + b"".join(lines)
    assert tool("view_bam.py", [bam, "-H"])[0] == text
    assert tool("view_bam.py", [bam, "-c"])[0] == b"%d\n" % len(lines)
    tool("view_bam.py", [bam, "-o", tmp_path / "out.sam", "-f", "0x10", "-F", "2048", "--window", "65536"])
    assert open(tmp_path / "out.sam", "rb").read() == b"".join(ln for ln, f in zip(lines, flags) if f & 16 and not f & 2048)

    # every record through a region of its own interval (1-based, inclusive), then a whole reference and a single base with commas, all in one call: the
    # regions print one after the other
    placed = [(r, ln) for r, ln in zip(recs, lines) if r["ref"] >= 0]
    name = refs[0][0].decode()
    regions = ["%s:%d-%d" % (refs[r["ref"]][0].decode(), r["pos"] + 1, r["end"]) for r, _ in placed] + [name, name + ":1,000-1,000"]
    got = tool("view_bam.py", [bam] + regions)[0]
    want = b""
    for r, _ in placed:
        want += b"".join(l2 for r2, l2 in placed if r2["ref"] == r["ref"] and r2["pos"] < r["end"] and r2["end"] > r["pos"])
    want += b"".join(ln for r, ln in placed if r["ref"] == 0)
    want += b"".join(ln for r, ln in placed if r["ref"] == 0 and r["pos"] < 1000 and r["end"] > 999)
    assert got == want and all(ln in got for _, ln in placed)
    os.rename(str(bam) + ".bai", str(bam) + ".bai.away")
    assert b"has no index" in tool("view_bam.py", [bam, name], ok=False)[1]
