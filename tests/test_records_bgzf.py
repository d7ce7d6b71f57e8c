"""lra_map_records_device_bgzf against lra_map_records_device on the same lra_map_result: the members inflate to the plain call's text byte for byte, rec_off
is the plain call's, the SV signature text is unchanged; tools/map_files.py --bgzf writes a BGZF file of the plain run's bytes."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from lra_amd import bgzf, synth
import test_records_device as T

pytestmark = pytest.mark.gpu
ROOT = T.ROOT


def _inflate(data, member_off):
    in_off, _ = bgzf.blocks(data)
    assert in_off == [int(x) for x in member_off]
    return gzip.decompress(data + bgzf.EOF_BLOCK)


def _plain(mapper, res, args, tags, md, svsig=False):
    r = mapper.records_device(res, args, passthrough=tags, md=md, svsig=svsig)
    texts, sigs = r if svsig else (r, None)
    off = np.zeros(len(texts) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in texts], dtype=np.uint64)
    return b"".join(texts), off, sigs


def _same(mapper, res, args, tags, md=False, svsig=False):
    text, off, sigs = _plain(mapper, res, args, tags, md, svsig)
    r = mapper.records_device_bgzf(res, args, passthrough=tags, md=md, svsig=svsig)
    assert _inflate(r[0], r[2]) == text
    assert np.array_equal(r[1], off)
    assert len(r[2]) - 1 == (len(text) + 65279) // 65280
    if svsig:
        assert r[3] == sigs
    return text


def test_ont_batch_formats_and_buffer_reuse(ctx):
    from lra_amd import seed
    mapper, reads, rng = T._ont_setup(ctx)
    n = len(reads)
    names = [b"read/%d" % i for i in range(n)]
    quals = T._quals(rng, reads)
    tags = [None if i % 3 == 0 else b"XA:i:%d" % i for i in range(n)]
    args = mapper.record_args(names, reads, quals)
    res = mapper.align(seed.ReadBatch(ctx, reads))
    sizes = {}
    for fmt, hard, md in (("s", 0, False), ("s", 1, True), ("P", 0, False), ("a", 0, False), ("p", 0, False), ("b", 0, False)):
        T._set(mapper, printFormat=fmt, hardClip=hard, PrintNumAln=1)
        sizes[fmt, hard] = len(_same(mapper, res, args, tags, md=md))
    assert all(sizes.values()) and sizes["s", 0] > 65280                       # more than one member
    # the signature text is the plain call's, for a device format and a fall-through one
    for fmt in "sp":
        T._set(mapper, printFormat=fmt, hardClip=0)
        _same(mapper, res, args, tags, svsig=True)
    # a bgzf call, a plain call and another bgzf call on the same context; then a smaller batch
    T._set(mapper, printFormat="s", hardClip=0)
    a = mapper.records_device_bgzf(res, args, passthrough=tags)
    text = _plain(mapper, res, args, tags, False)[0]
    b = mapper.records_device_bgzf(res, args, passthrough=tags)
    assert a[0] == b[0] and _inflate(b[0], b[2]) == text
    st = mapper.records_device_stats()
    assert st["text_bytes"] == len(text) and st["bytes_d2h"] < len(text)        # the members crossed, not the text
    sub = [6, 1, 11]
    r2 = [reads[i] for i in sub]
    res2 = mapper.align(seed.ReadBatch(ctx, r2))
    _same(mapper, res2, mapper.record_args([names[i] for i in sub], r2, [quals[i] for i in sub]), [tags[i] for i in sub])


def test_ccs_batch_through_the_high_accuracy_driver(ctx):
    from lra_amd import seed, mapread
    import test_highacc_path as H
    g = H._genome_with_repeats(19)
    rng = np.random.default_rng(8)
    reads = [r.tobytes() for r in H._sv_reads(g, rng, 0.01, n_plain=4)]
    mapper = mapread.HighAccMapper(ctx, g, None, None, [b"chrA", b"chrB"], [0, 250_000, len(g)], "ccs", index_params=(17, 10, 150, 15, 1))
    names = [b"ccs%d" % i for i in range(len(reads))]
    args = mapper.record_args(names, reads, T._quals(rng, reads))
    res = mapper.align(seed.ReadBatch(ctx, reads))
    for hard, md, fmt in ((0, False, "s"), (1, True, "s"), (0, False, "P")):
        T._set(mapper, printFormat=fmt, hardClip=hard)
        assert _same(mapper, res, args, None, md=md)


def test_map_files_bgzf_writes_the_plain_runs_bytes(ctx, tmp_path):
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

    def names_of(path):
        rf = reads_io.ReadsFile([path])
        b = rf.next_batch(10 ** 9)
        rf.close()
        return b["names"]

    for k, extra in enumerate(([], ["--device-records"])):
        plain = run(str(tmp_path / ("p%d.sam" % k)), extra)
        z = run(str(tmp_path / ("z%d.sam.gz" % k)), extra + ["--bgzf"])
        assert z.endswith(bgzf.EOF_BLOCK) and z[:4] == b"\x1f\x8b\x08\x04"
        assert bgzf.blocks(z)[0][-1] == len(z)
        assert gzip.decompress(z) == plain
        want = [l.split(b"\t")[0] for l in plain.split(b"\n") if l and not l.startswith(b"@")]
        got = names_of(str(tmp_path / ("z%d.sam.gz" % k)))
        assert got == names_of(str(tmp_path / ("p%d.sam" % k))) and list(dict.fromkeys(got)) == list(dict.fromkeys(want)) == [b"r0", b"r1", b"r2"]
