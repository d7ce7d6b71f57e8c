"""tools/map_files.py --bam --sort --merge-runs and tools/merge_bam.py: a budget that makes the sorter write two runs ends, with --merge-runs, in the
very bytes (file and index) a budget large enough for one run gives, with no run file left; without the flag the two runs appear as before, and
merge_bam.py merges them into the same records with an index that answers region queries."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_text as bt                                                             # noqa: E402
import bam_text                                                                   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN = [70_000, 50_000]


def tool(name, argv, ok=True):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + [str(a) for a in argv], cwd=ROOT, capture_output=True, timeout=600)
    assert (p.returncode == 0) == ok, p.stderr.decode()[-2000:]
    return p.stderr


def body_of(path):
    """-> (the file's bytes, the offset of the first record in the inflated file, the raw record stream, the records)"""
    z = open(path, "rb").read()
    raw = bam_text.inflate(z)
    at = bam_text.parse_header(raw)[2]
    body = raw[at:]
    return z, at, body, [body[r["at"]:r["next"]] for r in bt.walk(body)]


def test_merge_runs(ctx, tmp_path):
    import torch
    from lra_amd import synth
    from lra_amd.bam import BamSorter, SorterFull
    rng = np.random.default_rng(21)
    genome = synth.make_genome(120_000, seed=5, repeat_frac=0.1, n_families=2)
    with open(tmp_path / "g.fa", "wb") as f:
        f.write(b">chr1 test\n" + genome[:70_000].tobytes() + b"\n>chr2\n" + genome[70_000:].tobytes() + b"\n")
    read_names = [b"r0", b"r1", b"r2", b"r3", b"junk"]
    with open(tmp_path / "r.fq", "wb") as f:
        for i, a in enumerate((80_000, 40_000, 5000, 100_000)):
            r = synth.simulate_read(rng, genome[a:a + 4001], 4000, 0.08, (30, 35, 35), i == 1)[0].tobytes()
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, bytes(rng.integers(34, 74, len(r)).astype(np.uint8))))
        f.write(b"@junk\n%s\n+\n%s\n" % (bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000)), b"I" * 3000))
    common = ["-ONT", tmp_path / "g.fa", tmp_path / "r.fq", "--batch-bases", "3000", "--bam", "--sort"]

    assert b"--sort" in tool("map_files.py", ["-ONT", tmp_path / "g.fa", tmp_path / "r.fq", "--bam", "-o", tmp_path / "x.bam", "--merge-runs"], ok=False)
    tool("map_files.py", common + ["-o", tmp_path / "one.bam"])                   # the default budget: one run
    _, _, _, recs = body_of(tmp_path / "one.bam")
    assert {r[36:36 + r[12] - 1] for r in recs} == set(read_names)

    # the budget that holds three of the five batches (a batch is a read: --batch-bases): the bisection of the sorter's own test, on batches of the same sizes
    up = []
    for nm in read_names:
        part = [r for r in recs if r[36:36 + r[12] - 1] == nm]
        st = np.concatenate([[0], np.cumsum([len(r) for r in part])]).astype(np.int64)
        up.append((torch.from_numpy(np.frombuffer(b"".join(part), np.uint8).copy()).to(ctx.device), torch.from_numpy(st).to(ctx.device)))

    def fit(budget):
        s = BamSorter(ctx, budget)
        try:
            for k, (stream, starts) in enumerate(up):
                try:
                    s.add(stream, starts)
                except SorterFull:
                    return k
            return len(up)
        finally:
            s.close()
    lo, hi = 1, 1 << 30
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if fit(mid) >= 3 else (mid, hi)
    budget = hi + 4096                                                            # (finish needs the references' counters and windows on top)
    assert fit(hi) == fit(budget) == 3

    err = tool("map_files.py", common + ["--sort-mem", budget, "--merge-runs", "-o", tmp_path / "m.bam"])
    print(err.decode()[-600:])
    assert b"2 runs merged" in err
    assert open(tmp_path / "m.bam", "rb").read() == open(tmp_path / "one.bam", "rb").read()
    assert open(tmp_path / "m.bam.bai", "rb").read() == open(tmp_path / "one.bam.bai", "rb").read()
    assert sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "m*"))) == ["m.bam", "m.bam.bai"], "no run file is left"

    err = tool("map_files.py", common + ["--sort-mem", budget, "-o", tmp_path / "two.bam"])           # without the flag: the two runs, as before
    assert b"the runs are not merged" in err and not os.path.exists(tmp_path / "two.bam")
    runs = [str(tmp_path / ("two.run%04d.bam" % i)) for i in range(2)]
    assert sorted(glob.glob(str(tmp_path / "two*"))) == sorted(runs + [p + ".bai" for p in runs])

    tool("merge_bam.py", runs + ["-o", tmp_path / "mb.bam", "--mem", 64 << 20])
    z, _, body, got = body_of(tmp_path / "mb.bam")
    assert got == recs and bam_text.parse_header(bam_text.inflate(z))[1] == [(b"chr1", 70_000), (b"chr2", 50_000)]
    bai = open(tmp_path / "mb.bam.bai", "rb").read()
    assert bt.check_queries(np.random.default_rng(3), z, bai, body, REF_LEN, 60) > 5
    bad = tool("merge_bam.py", [runs[0], tmp_path / "g.fa", "-o", tmp_path / "no.bam"], ok=False)
    assert b"g.fa is not a BAM file" in bad and not os.path.exists(tmp_path / "no.bam")
