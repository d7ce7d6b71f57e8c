"""lra_map_records_device against lra_map_records_host_tags on the same lra_map_result: byte for byte, record boundaries included."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _quals(rng, reads):
    return [bytes(rng.integers(43, 74, len(r)).astype(np.uint8)) for r in reads]        # ('*' is 42: only where a test puts it)


def _both(mapper, res, names, reads, quals, tags, md=False, fmt=None):
    """(device text, host text) per read for the mapper's current options."""
    fmt = fmt or chr(mapper.copts.printFormat)
    args = mapper.record_args(names, reads, quals)
    host = mapper.records_host(mapper.snapshot(res, with_blocks=fmt == "a", md=md), args, passthrough=list(tags) if tags is not None else [None] * len(names))
    dev = mapper.records_device(res, args, passthrough=tags, md=md)
    for i, (d, h) in enumerate(zip(dev, host)):                            # (the place of a difference, not two 40 KB records)
        if d != h:
            at = next((k for k in range(min(len(d), len(h))) if d[k] != h[k]), min(len(d), len(h)))
            raise AssertionError("read %d: %d / %d bytes, first difference at %d: %r / %r" % (i, len(d), len(h), at, d[max(at - 20, 0):at + 20], h[max(at - 20, 0):at + 20]))
    return dev, host


def _set(mapper, **kw):
    for k, v in kw.items():
        setattr(mapper.copts, k, ord(v) if k == "printFormat" else int(v))


def _ont_setup(ctx):
    from lra_amd import mapread
    rng = np.random.default_rng(3)
    genome = synth.make_genome(600_000, seed=77, repeat_frac=0.2, n_families=3).copy()
    genome[330_000:354_000] = genome[100_000:124_000]                      # a segmental duplication: reads inside it have two chains (secondary records under PrintNumAln 2)
    CH = [0, 300_000, len(genome)]
    o = mapread.LowAccOptions()
    ik, ip = synth.build_global_index(genome, o.globalK, o.globalW, 100)
    mix = (30, 35, 35)
    sim = lambda a, n, rev=False, err=0.08: synth.simulate_read(rng, genome[a:a + n + 1], n, err, mix, rev)[0]
    junk = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    reads = [junk(2500)]                                                   # the first and the last read are unaligned
    reads += [sim(20_000, 6000), sim(50_000, 7000, True), sim(400_000, 5000), sim(450_000, 6500, True), sim(250_000, 3000)]
    reads.append(np.concatenate([sim(130_000, 4500), sim(500_000, 4500, True)]))              # translocation, second half reversed: SA:Z, supplementary records
    reads.append(np.concatenate([sim(160_000, 4000), sim(164_000, 2500, True), sim(166_500, 4000)]))   # inversion
    reads.append(synth.revcomp(np.concatenate([sim(200_000, 4000), sim(560_000, 4000)])))
    reads += [sim(104_000, 12_000, False, 0.02), sim(336_000, 12_000, True, 0.02), sim(108_000, 9000), sim(340_000, 8000, True)]   # inside the duplication
    reads.append(junk(3001))
    mapper = mapread.LowAccMapper(ctx, genome, ik, ip, [b"chrA", b"chrB"], CH, o)
    return mapper, [r.tobytes() for r in reads], rng


@pytest.mark.gpu
def test_ont_batch_every_option(ctx):
    import torch
    from lra_amd import seed
    mapper, reads, rng = _ont_setup(ctx)
    n = len(reads)
    names = [b"read/%d" % i for i in range(n)]
    quals = _quals(rng, reads)
    quals[2] = b"*"                                                        # an aligned read whose quality string is "*"
    quals[4] = None
    quals[0] = b"*" + quals[0][1:]                                         # an unaligned read's string is written as it is (SimplePrintSAM), a leading '*' too
    tags = [None if i % 3 == 0 else b"XA:i:%d\tXZ:Z:t%d" % (i, i) for i in range(n)]
    res = mapper.align(seed.ReadBatch(ctx, reads))
    seen = dict(rev=0, supp=0, sa=0, sec=0, un=0, star=0, md=0, hclip=0)
    for hard in (0, 1):
        for q in (quals, None):
            _set(mapper, printFormat="s", hardClip=hard, PrintNumAln=1)
            dev, host = _both(mapper, res, names, reads, q, tags)
            assert dev == host, (hard, q is None)
            for t in host:
                for line in t.split(b"\n")[:-1]:
                    f = line.split(b"\t")
                    fl = int(f[1])
                    seen["rev"] += bool(fl & 16); seen["supp"] += bool(fl & 2048); seen["un"] += bool(fl & 4); seen["sa"] += b"\tSA:Z:" in line
                    seen["star"] += f[10] == b"*" and q is not None; seen["hclip"] += b"H" in f[5]
    assert seen["rev"] >= 3 and seen["supp"] >= 3 and seen["sa"] >= 4 and seen["un"] >= 8 and seen["star"] >= 1 and seen["hclip"] >= 1, seen
    # secondary records, MD:Z, no passthrough, PAF with CIGAR
    _set(mapper, printFormat="s", hardClip=1, PrintNumAln=2)
    dev, host = _both(mapper, res, names, reads, quals, tags, md=True)
    assert dev == host
    seen["sec"] = sum(int(l.split(b"\t")[1]) & 256 != 0 for t in host for l in t.split(b"\n")[:-1])
    seen["md"] = sum(b"\tMD:Z:" in l for t in host for l in t.split(b"\n")[:-1])
    fo = mapper.fetch(res)
    groups = [sum(int(fo["job_aln_off"][i * int(res.num_aln) + p + 1] > fo["job_aln_off"][i * int(res.num_aln) + p]) for p in range(int(res.num_aln))) for i in range(n)]
    assert seen["sec"] >= 1 and seen["md"] >= n - 2, (seen, groups)
    dev, host = _both(mapper, res, names, reads, quals, None)
    assert dev == host
    _set(mapper, printFormat="P")
    dev, host = _both(mapper, res, names, reads, quals, tags)
    assert dev == host and any(b"CG:z:" in t for t in host)
    _set(mapper, PrintNumAln=1)
    for fmt in "pba":                                                      # the fall-through formats: the host path's text
        _set(mapper, printFormat=fmt)
        dev, host = _both(mapper, res, names, reads, quals, tags, fmt=fmt)
        assert dev == host and any(host), fmt
    # the qualities as a device buffer: the host strings are read at their first byte only
    _set(mapper, printFormat="s", hardClip=1)
    qoff = np.zeros(n + 1, np.int64)
    qoff[1:] = np.cumsum([len(q) if q is not None else 0 for q in quals])
    dq = torch.from_numpy(np.frombuffer(b"".join(q for q in quals if q is not None), np.uint8).copy()).to(ctx.device)
    args = mapper.record_args(names, reads, [None if q is None else q[:1] + b"!" * (len(q) - 1) for q in quals])
    exp = mapper.records_host(mapper.snapshot(res), mapper.record_args(names, reads, quals), passthrough=tags)
    assert mapper.records_device(res, args, passthrough=tags, d_qual=dq, d_qual_off=torch.from_numpy(qoff).to(ctx.device)) == exp
    st = mapper.records_device_stats()
    assert st["text_bytes"] == sum(len(t) for t in exp) and st["bytes_d2h"] < st["text_bytes"] + 64 * 1024 and st["bytes_d2h"] >= st["text_bytes"]
    # a flagged read (LRA_ST_CAPACITY = 8, set the way the flagged-read test sets it) under both rules
    one = torch.tensor([8], dtype=torch.int32, device=ctx.device)
    ctx.check(ctx.lib.lra_copy_device(ctx.h, C.c_void_p(res.d_read_status + 3 * 4), C.c_void_p(one.data_ptr()), C.c_uint64(4)))
    torch.cuda.synchronize()
    for fu in (0, 1):
        _set(mapper, flagged_unaligned=fu)
        dev, host = _both(mapper, res, names, reads, quals, tags)
        assert dev == host and (host[3] == b"") == (fu == 0)
    _set(mapper, flagged_unaligned=0)
    # a smaller batch after a larger one on the same context (the kept buffers are reused), then a batch of one read
    for sub in ([6, 1, 11], [7]):
        r2 = [reads[i] for i in sub]
        res2 = mapper.align(seed.ReadBatch(ctx, r2))
        dev, host = _both(mapper, res2, [names[i] for i in sub], r2, [quals[i] for i in sub], [tags[i] for i in sub])
        assert dev == host and all(host), sub


@pytest.mark.gpu
def test_ccs_batch_through_the_high_accuracy_driver(ctx):
    from lra_amd import seed, mapread
    import test_highacc_path as H
    g = H._genome_with_repeats(19)
    rng = np.random.default_rng(8)
    reads = [r.tobytes() for r in H._sv_reads(g, rng, 0.01, n_plain=4)]
    mapper = mapread.HighAccMapper(ctx, g, None, None, [b"chrA", b"chrB"], [0, 250_000, len(g)], "ccs", index_params=(17, 10, 150, 15, 1))
    n = len(reads)
    names = [b"ccs%d" % i for i in range(n)]
    quals = _quals(rng, reads)
    res = mapper.align(seed.ReadBatch(ctx, reads))
    for hard, md, fmt in ((0, False, "s"), (1, True, "s"), (0, False, "P")):
        _set(mapper, printFormat=fmt, hardClip=hard)
        dev, host = _both(mapper, res, names, reads, quals, None, md=md)
        assert dev == host, (hard, md, fmt)
    assert sum(b"\tSA:Z:" in t for t in host) == 0 and any(b"CG:z:" in t for t in host)


@pytest.mark.gpu
def test_map_files_device_records_writes_the_same_sam(ctx, tmp_path):
    rng = np.random.default_rng(21)
    genome = synth.make_genome(120_000, seed=5, repeat_frac=0.1, n_families=2)
    with open(tmp_path / "g.fa", "wb") as f:
        f.write(b">chr1 test\n" + genome.tobytes() + b"\n")
    with open(tmp_path / "r.fq", "wb") as f:
        for i, a in enumerate((5000, 40_000, 80_000)):
            r = synth.simulate_read(rng, genome[a:a + 4001], 4000, 0.08, (30, 35, 35), i == 1)[0].tobytes()
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, bytes(rng.integers(34, 74, len(r)).astype(np.uint8))))
    outs = []
    for extra in ([], ["--device-records"]):
        out = str(tmp_path / ("o%d.sam" % len(outs)))
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_files.py"), "-ONT", str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), "-H", "--printMD", "-o", out] + extra,
                       check=True, cwd=ROOT, stderr=subprocess.DEVNULL)
        outs.append(open(out, "rb").read())
    strip = lambda s: b"\n".join(l for l in s.split(b"\n") if not l.startswith(b"@PG"))   # (the header's @PG line quotes the command line)
    assert strip(outs[0]) == strip(outs[1]) and outs[0].count(b"\n") >= 5
