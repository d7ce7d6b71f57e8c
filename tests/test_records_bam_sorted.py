"""lra_map_records_device_bam_to_sorter and tools/map_files.py --bam --sort: the sorted file holds lra_map_records_device_bam's records, in samtools sort's
order, and its .bai answers region queries."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bai_text as bt
import bam_text
from lra_amd import bgzf, synth
import test_records_bam as RB

T = RB.T                                                                          # the batches of test_records_bam: its module's _ont_setup, _quals, _set

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = [(b"chrA", 300_000), (b"chrB", 300_000)]
REF_LEN = [300_000, 300_000]


def _split(raw):
    return [raw[r["at"]:r["next"]] for r in bt.walk(raw)]


def _two_calls(ctx, mapper, reads, names, quals, tags, md=True):
    """the batch in two halves, each through the unsorted call and into the sorter -> (the unsorted records in call order, pieces, bai)"""
    from lra_amd import seed
    from lra_amd.bam import BamSorter
    s = BamSorter(ctx, 1 << 32)
    recs = []
    h = len(reads) // 2
    for a, b in ((0, h), (h, len(reads))):
        res = mapper.align(seed.ReadBatch(ctx, reads[a:b]))
        args = mapper.record_args(names[a:b], reads[a:b], quals[a:b])
        raw, rec_off = mapper.records_device_bam(res, args, passthrough=tags[a:b], md=md)
        off = mapper.records_device_bam_to_sorter(res, args, s, passthrough=tags[a:b], md=md)
        assert [int(x) for x in off] == [int(x) for x in rec_off]
        recs += _split(raw)
        assert s.held() == (len(recs), sum(len(r) for r in recs))
    s.finish(1234, REF_LEN)
    pieces = list(s.pieces())
    bai = s.index()
    s.close()
    return recs, pieces, bai


def test_ont_batch_in_two_calls(ctx):
    from lra_amd import mapread
    from lra_amd.bam import index_host
    mapper, reads, rng = T._ont_setup(ctx)
    n = len(reads)
    names = [b"read/%d" % i for i in range(n)]
    quals = T._quals(rng, reads)
    tags = [None if i % 3 == 0 else b"XA:i:%d" % i for i in range(n)]
    T._set(mapper, printFormat="s", hardClip=0, PrintNumAln=1)
    recs, pieces, bai = _two_calls(ctx, mapper, reads, names, quals, tags)
    data = b"".join(pieces)
    raw = bam_text.inflate(data)
    assert raw == b"".join(sorted(recs, key=bt.sort_key))                         # the order, ties in the order added
    lines = [l for _, _, l in bam_text.records(raw, REFS)]
    assert sorted(lines) == sorted(l for _, _, l in bam_text.records(b"".join(recs), REFS))
    keys = [bt.sort_key(r) for r in _split(raw)]
    assert keys == sorted(keys) and keys[0][0] == 0 and keys[-1][0] == 0xffffffff and len({k[0] for k in keys}) == 3
    member_off = bgzf.blocks(data)[0]
    assert bai == index_host(raw, REF_LEN, member_off, 1234) == bt.build(raw, 2, member_off, 1234)
    assert bt.check_queries(np.random.default_rng(2), b"\0" * 1234 + data + bgzf.EOF_BLOCK, bai, raw, REF_LEN, 200) > 25
    # the CG:B:I form: the CIGAR is <l_seq>S<span>N, and the linear index covers the span the N op gives -- the record's own t_end - t_start
    try:
        mapread.set_bam_cigar_limit(ctx, 100)
        recs, pieces, bai = _two_calls(ctx, mapper, reads, names, quals, tags)
    finally:
        mapread.set_bam_cigar_limit(ctx, 65535)
    data = b"".join(pieces)
    raw = bam_text.inflate(data)
    member_off = bgzf.blocks(data)[0]
    assert bai == bt.build(raw, 2, member_off, 1234)
    refs, _ = bt.parse(bai)
    aligned = 0
    for r in bt.walk(raw):
        if r["ref"] < 0:
            continue
        n_cig, tlen = struct.unpack_from("<H", raw, r["at"] + 16)[0], struct.unpack_from("<i", raw, r["at"] + 32)[0]
        assert n_cig == 2 and r["end"] - r["pos"] == tlen > 1000                  # (tlen holds the SAM's column 9: t_end - t_start)
        vb = bt.voff(r["at"], member_off, 1234)
        lin = refs[r["ref"]]["lin"]
        assert all(lin[w] <= vb for w in range(r["pos"] >> 14, ((r["end"] - 1) >> 14) + 1))
        aligned += 1
    assert aligned >= 12


def test_map_files_sort(ctx, tmp_path):
    from lra_amd import reads_io
    from lra_amd.bam import BamSorter, SorterFull
    import torch
    rng = np.random.default_rng(21)
    genome = synth.make_genome(120_000, seed=5, repeat_frac=0.1, n_families=2)
    with open(tmp_path / "g.fa", "wb") as f:
        f.write(b">chr1 test\n" + genome[:70_000].tobytes() + b"\n>chr2\n" + genome[70_000:].tobytes() + b"\n")
    ref_len = [70_000, 50_000]
    with open(tmp_path / "r.fq", "wb") as f:
        for i, a in enumerate((80_000, 40_000, 5000, 100_000)):
            r = synth.simulate_read(rng, genome[a:a + 4001], 4000, 0.08, (30, 35, 35), i == 1)[0].tobytes()
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, bytes(rng.integers(34, 74, len(r)).astype(np.uint8))))
        f.write(b"@junk\n%s\n+\n%s\n" % (bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000)), b"I" * 3000))

    def run(out, extra, ok=True):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_files.py"), "-ONT", str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), "--batch-bases", "3000",
                            "-o", str(out)] + extra, cwd=ROOT, capture_output=True, timeout=600)
        assert (p.returncode == 0) == ok, p.stderr.decode()[-2000:]
        return p.stderr

    def load(path):
        """-> (header text, the records, their stream); the file is sorted and its index answers region queries"""
        z = open(path, "rb").read()
        assert z.endswith(bgzf.EOF_BLOCK) and bgzf.blocks(z)[0][-1] == len(z)
        raw = bam_text.inflate(z)
        text, refs, at = bam_text.parse_header(raw)
        assert refs == [(b"chr1", 70_000), (b"chr2", 50_000)]
        body = raw[at:]
        recs = _split(body)
        keys = [bt.sort_key(r) for r in recs]
        assert keys == sorted(keys)
        bai = open(str(path) + ".bai", "rb").read()
        # the members of the records: those behind the header's (the header is cut into members of its own)
        first = next(off for off, u in zip(*bgzf.blocks(z)) if u == at)
        member_off = [off - first for off, u in zip(*bgzf.blocks(z)) if u >= at][:-1]      # (less the EOF member's end)
        assert bai == bt.build(body, 2, member_off, first)
        if recs:
            bt.check_queries(np.random.default_rng(3), z, bai, body, ref_len, 60)
        return text, recs, body

    assert b"--bam" in run(tmp_path / "x.sam", ["--sort"], ok=False)               # --sort without --bam
    run(tmp_path / "out.bam", ["--bam", "--sort", "-SV", "25", str(tmp_path / "sv.txt")])
    text, recs, body = load(tmp_path / "out.bam")
    assert text.startswith(b"@HD\tVN:1.6\tSO:coordinate\n@PG\t") and text.count(b"@SQ") == 2
    assert not os.path.exists(tmp_path / "out.run0000.bam") and os.path.exists(tmp_path / "sv.txt")
    names = [r[36:36 + r[12] - 1] for r in recs]
    assert set(names) == {b"r0", b"r1", b"r2", b"r3", b"junk"} and names[-1] == b"junk" and len({bt.sort_key(r)[0] for r in recs}) == 3
    unsorted = tmp_path / "plain.bam"
    run(unsorted, ["--bam"])
    raw = bam_text.inflate(open(unsorted, "rb").read())
    plain = _split(raw[bam_text.parse_header(raw)[2]:])
    assert sorted(plain) == sorted(recs) and plain != recs
    rf = reads_io.ReadsFile([str(tmp_path / "out.bam")], ctx=ctx)                 # the project's own BAM reader takes the file
    b = rf.next_batch(10 ** 9)
    rf.close()
    assert b["names"] == names
    # a budget that holds the first batches only: the batches are the reads (--batch-bases), their records those of the plain file in read order
    batches = [[r for r in plain if r[36:36 + r[12] - 1] == nm] for nm in (b"r0", b"r1", b"r2", b"r3", b"junk")]
    up = []
    for part in batches:
        d = b"".join(part)
        st = np.concatenate([[0], np.cumsum([len(r) for r in part])]).astype(np.int64)
        up.append((torch.from_numpy(np.frombuffer(d, np.uint8).copy()).to(ctx.device), torch.from_numpy(st).to(ctx.device)))

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
    budget = hi + 4096                                                            # (add cannot know the references: finish needs their counters and windows on top)
    assert fit(hi) == fit(budget) == 3                                            # three batches make the first run, the rest the second
    err = run(tmp_path / "two.bam", ["--bam", "--sort", "--sort-mem", str(budget)])
    assert b"two.run0000.bam" in err and not os.path.exists(tmp_path / "two.bam") and not os.path.exists(tmp_path / "two.run0002.bam")
    t0, r0, _ = load(tmp_path / "two.run0000.bam")
    t1, r1, _ = load(tmp_path / "two.run0001.bam")
    assert t0 == t1 and t0.startswith(b"@HD\tVN:1.6\tSO:coordinate\n@PG\t") and r0 and r1 and sorted(r0 + r1) == sorted(recs)   # (the @PG line holds the command line)
