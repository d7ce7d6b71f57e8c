"""lra_reads_set_device_resident: a device reader's batch keeps its qualities on the device (LRA_READS_DEV_QUAL) and, for a caller that reads neither
bases nor qualities on the host, skips their host copies (LRA_READS_DEV_NO_HOST).  Three readers walk every corpus in step -- plain, DEV_QUAL,
DEV_QUAL | DEV_NO_HOST -- and every batch of the two new modes is held against the plain reader's; then the record stage is fed from the reader's arrays."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lra_amd import bgzf, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1                                                               # LRA_ERR_INVALID


# ---- the CPU part: the two calls' argument rules -------------------------------------------------------------------------------------------------------
def _open(path, flags=None):
    from lra_amd._lib import load_library
    lib = load_library()
    h = C.c_void_p()
    arr = (C.c_char_p * 1)(str(path).encode())
    rc = lib.lra_reads_open(arr, 1, C.byref(h)) if flags is None else lib.lra_reads_open_flags(arr, 1, C.c_uint32(flags), C.byref(h))
    return lib, h, rc


def test_setter_and_accessor_argument_rules(tmp_path):
    from lra_amd.reads_io import ReadBatchC
    p = tmp_path / "r.fq"
    p.write_bytes(b"@a\nACGT\n+\nIIII\n@b\nGG\n+\nJJ\n")
    lib, h, rc = _open(p)
    assert rc == 0
    for mode in (4, 8, 5, 7, 0x80000001, 0xffffffff):                      # undefined bits
        assert lib.lra_reads_set_device_resident(h, C.c_uint32(mode)) == INVALID, mode
    assert lib.lra_reads_set_device_resident(h, 2) == INVALID              # NO_HOST without DEV_QUAL
    assert lib.lra_reads_set_device_resident(None, 1) == INVALID
    for mode in (1, 3, 0, 1):
        assert lib.lra_reads_set_device_resident(h, mode) == 0, mode
    dq, dqo = C.c_void_p(), C.c_void_p()
    assert lib.lra_reads_batch_device_quals(h, C.byref(dq), C.byref(dqo)) == INVALID     # before the first batch
    assert lib.lra_reads_batch_device_quals(h, None, C.byref(dqo)) == INVALID
    # a host-form reader: neither call after its first batch, with or without the bit
    b = ReadBatchC()
    assert lib.lra_reads_next_batch(h, C.c_uint64(10 ** 9), C.byref(b)) == 0 and b.n_reads == 2
    assert lib.lra_reads_batch_device_quals(h, C.byref(dq), C.byref(dqo)) == INVALID and not dq.value and not dqo.value
    for mode in (0, 1, 3):
        assert lib.lra_reads_set_device_resident(h, mode) == INVALID       # only before the first batch
    lib.lra_reads_close(h)
    lib, h, rc = _open(p)                                                  # a reader without the bit
    assert rc == 0 and lib.lra_reads_batch_device_quals(h, C.byref(dq), C.byref(dqo)) == INVALID
    assert lib.lra_reads_next_batch(h, C.c_uint64(10 ** 9), C.byref(b)) == 0
    assert lib.lra_reads_batch_device_quals(h, C.byref(dq), C.byref(dqo)) == INVALID
    lib.lra_reads_close(h)


def test_open_flags_still_refuses_the_setter_bits(tmp_path):
    p = tmp_path / "r.fq"
    p.write_bytes(b"@a\nACGT\n+\nIIII\n")
    for flags in (2, 3):
        lib, h, rc = _open(p, flags)
        assert rc == INVALID and not h.value, flags
    lib, h, rc = _open(p, 1)
    assert rc == 0
    lib.lra_reads_close(h)


def test_python_reader_refuses_the_modes_without_a_device(tmp_path):
    from lra_amd import reads_io
    p = tmp_path / "r.fq"
    p.write_bytes(b"@a\nACGT\n+\nIIII\n")
    with pytest.raises(ValueError):
        reads_io.ReadsFile([str(p)], device_quals=True)                    # the host form has no device arrays


# ---- the readers in step ---------------------------------------------------------------------------------------------------------------------------------
def _batches(rf, max_bases):
    """every batch of a reader as (batch or None, (rc, message) or None); ends behind the end of the input or the first error"""
    while True:
        err = None
        try:
            b = rf.next_batch(max_bases)
        except IOError as e:
            b, err = e.partial, (e.rc, str(e))
        yield b, err
        if err is not None or b is None:
            return


def _device_quals(ctx, b, n):
    off = ctx.to_host(b["d_qual_off"], n + 1, np.uint64)
    data = ctx.to_host(b["d_qual"], int(off[n]) + 64, np.uint8).tobytes()
    return off, data


def _check_batch(ctx, p, q, h):
    """p: the plain reader's batch; q: DEV_QUAL's; h: DEV_QUAL | DEV_NO_HOST's"""
    n, tot = p["n"], p["total_bases"]
    assert q["n"] == h["n"] == n and q["total_bases"] == h["total_bases"] == tot
    for k in ("names", "seqs", "quals", "tags", "read_len"):               # DEV_QUAL leaves the host arrays as they are
        assert q[k] == p[k], k
    assert np.array_equal(q["off"], p["off"]) and np.array_equal(h["off"], p["off"])
    lens = [0 if x is None else len(x) for x in p["quals"]]
    packed = b"".join(x for x in p["quals"] if x is not None)
    for b in (q, h):
        off, data = _device_quals(ctx, b, n)
        assert off[0] == 0 and np.diff(off.astype(np.int64)).tolist() == lens      # the ranges, the empties, which reads have none
        assert data == packed + bytes(64)
    raw = h["raw"]
    assert h["seqs"] is None and not raw.seq and all(not raw.reads[i] for i in range(n))
    assert h["quals"] == [None if x is None else x[:1] for x in p["quals"]]         # NULL or the stub
    assert h["names"] == p["names"] and h["tags"] == p["tags"] and h["read_len"] == p["read_len"] == [len(s) for s in p["seqs"]]
    seq = b"".join(p["seqs"]) + bytes(64)
    for b in (p, q, h):
        assert ctx.to_host(b["d_seq"], tot + 64, np.uint8).tobytes() == seq
        assert np.array_equal(ctx.to_host(b["d_off"], n + 1, np.uint64), p["off"])


def _compare(ctx, files, max_bases, chunk=4096, **kw):
    """-> what was seen: batches, reads, reads without qualities, the error (rc, message) or None, the last batch's size"""
    from lra_amd import reads_io
    files = [str(f) for f in files]
    rfs = [reads_io.ReadsFile(files, ctx=ctx, chunk=chunk, **kw, **m) for m in ({}, dict(device_quals=True), dict(device_quals=True, no_host_copy=True))]
    seen = dict(batches=0, reads=0, none=0, err=None, last=0, bytes=0)
    try:
        ended = False
        for (p, pe), (q, qe), (h, he) in zip(*[_batches(rf, max_bases) for rf in rfs]):
            assert pe == qe == he, (pe, qe, he)                            # error codes and texts
            assert (p is None) == (q is None) == (h is None)
            if p is not None:
                _check_batch(ctx, p, q, h)
                seen["batches"] += 1; seen["reads"] += p["n"]; seen["none"] += sum(x is None for x in p["quals"]); seen["last"] = p["n"]
                seen["bytes"] += sum(len(x) for x in p["quals"] if x is not None)
            seen["err"] = pe
            ended = pe is not None or p is None
        assert ended
    finally:
        for rf in rfs:
            rf.close()
    return seen


def _fastq(recs, eol=b"\n"):
    return b"".join(b"@" + name + eol + s + eol + b"+" + eol + q + eol for name, s, q in recs)


def _recs(rng, lengths, prefix=b"q"):
    out = []
    for i, n in enumerate(lengths):
        s = bytes(np.frombuffer(b"ACGTacgtN", np.uint8)[rng.integers(0, 9, n)])
        out.append((prefix + b"%d len=%d" % (i, n), s, bytes(rng.integers(33, 127, n).astype(np.uint8))))
    return out


EDGE_LENGTHS = list(range(1, 10)) + [4095, 4096, 4097] + [200, 5, 777, 4096, 1, 4095, 3, 64, 65, 63, 255, 256, 257]


@pytest.fixture(scope="module")
def corpora(tmp_path_factory):
    d = tmp_path_factory.mktemp("device_quals")
    rng = np.random.default_rng(41)
    c = {}
    edge = _fastq(_recs(rng, EDGE_LENGTHS))
    c["edge"] = d / "edge.fq"; c["edge"].write_bytes(edge)
    c["edge_bgzf"] = d / "edge.bgzf.fq.gz"; c["edge_bgzf"].write_bytes(bgzf.bgzf_compress(edge, cuts=[3000, 3001, 9000, 14_000]))
    c["edge_gz"] = d / "edge.fq.gz"; c["edge_gz"].write_bytes(bgzf.gzip_compress(edge, 6))
    c["long"] = d / "long.fq"; c["long"].write_bytes(_fastq(_recs(rng, [300, 23_456, 70, 9000], b"L")))
    c["crlf"] = d / "crlf.fq"; c["crlf"].write_bytes(_fastq(_recs(rng, [4, 700, 4095, 2, 1300], b"c"), b"\r\n"))
    # the empty-line rules (test_input_device.py::test_device_reader_file_edges)
    c["good"] = d / "good.fa"; c["good"].write_bytes(b">g1\nACGT\n>g2\nTTTT\n")
    c["nonl"] = d / "nonl.fq"; c["nonl"].write_bytes(b"@n1\nACGT\n+\nIIII\n@n2\nGG\n+\nII")
    c["blank"] = d / "blank.fq"; c["blank"].write_bytes(b"@b1\nAC\n+\nII\n\n@b2\nGG\n+\nJJ\n")
    c["first_empty"] = d / "first_empty.fq"; c["first_empty"].write_bytes(b"@e1\nAC\n+\n\n@e2\nGG\n+\nJJ\n@e3\nTT\n+\nKK\n")
    c["short"] = d / "short.fq"; c["short"].write_bytes(b"@s1\nACGT\n+\nIIII\n@s2\nAC\n")
    fa = []
    for i, n in enumerate([10, 5000, 0, 333, 4096]):
        s = bytes(np.frombuffer(b"ACGTacgtN", np.uint8)[rng.integers(0, 9, n)])
        fa.append(b">f%d x\n" % i + b"".join(s[x:x + 60] + b"\n" for x in range(0, n, 60)))
    c["fasta"] = d / "mix.fa"; c["fasta"].write_bytes(b"".join(fa))
    recs = _recs(rng, [50, 600, 40, 900, 12], b"m")
    recs[2] = (recs[2][0], recs[2][1], recs[2][2][:-3])                    # the third record's quality line is short
    c["mismatch"] = d / "mismatch.fq"; c["mismatch"].write_bytes(_fastq(recs))
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("max_bases", [1, 5000, 10 ** 9])
def test_fastq_every_length_steps_cut_records(ctx, corpora, max_bases):
    seen = _compare(ctx, [corpora["edge"]], max_bases)
    assert seen["reads"] == len(EDGE_LENGTHS) and seen["none"] == 0 and seen["err"] is None and seen["bytes"] == sum(EDGE_LENGTHS)
    if max_bases != 5000:
        assert seen["batches"] == (len(EDGE_LENGTHS) if max_bases == 1 else 1)
    else:
        assert 3 <= seen["batches"] < len(EDGE_LENGTHS)                    # batches cut steps, steps cut batches
    seen = _compare(ctx, [corpora["edge"]], max_bases, chunk=10 ** 6)      # one step for the file
    assert seen["reads"] == len(EDGE_LENGTHS)


@pytest.mark.gpu
def test_fastq_long_read_crlf_and_empty_line_rules(ctx, corpora):
    c = corpora
    for mb in (1, 10_000, 10 ** 9):
        assert _compare(ctx, [c["long"]], mb)["bytes"] == 300 + 23_456 + 70 + 9000
        assert _compare(ctx, [c["crlf"]], mb)["reads"] == 5
    for order in (["blank", "first_empty", "good"], ["nonl", "good"], ["short", "blank", "good"], ["crlf", "good", "first_empty"], ["blank", "blank"], ["first_empty"]):
        for mb in (1, 3, 10 ** 9):
            _compare(ctx, [c[k] for k in order], mb)


@pytest.mark.gpu
def test_fasta_then_fastq_gives_mixed_batches(ctx, corpora):
    for mb in (1, 6000, 10 ** 9):
        seen = _compare(ctx, [corpora["fasta"], corpora["edge"]], mb)
        assert seen["reads"] == 5 + len(EDGE_LENGTHS) and seen["none"] == 5 and seen["err"] is None
    assert seen["batches"] == 1                                            # one batch holds reads with and without qualities


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["edge_bgzf", "edge_gz"])
def test_compressed_fastq(ctx, corpora, kind):
    for mb in (1, 5000, 10 ** 9):
        seen = _compare(ctx, [corpora[kind]], mb, compressed_text=True)
        assert seen["reads"] == len(EDGE_LENGTHS) and seen["bytes"] == sum(EDGE_LENGTHS) and seen["err"] is None


@pytest.mark.gpu
def test_bam_and_sam(ctx, tmp_path):
    from test_input_bam import _corpus
    recs, paths = _corpus(tmp_path, seed=3, n=60)
    n_noq = sum(r["qual"] is None for r in recs)
    assert n_noq >= 8 and any(r["qual"] is not None and r["flag"] & 0x900 for r in recs)
    for mb in (1, 1000, 10 ** 9):
        seen = _compare(ctx, [paths["bam"]], mb, passthrough=True)
        assert seen["reads"] == 60 and seen["none"] == n_noq and seen["err"] is None
        seen = _compare(ctx, [paths["bam"]], mb, flag_remove=0x900)        # -Flag skips records in between
        assert seen["reads"] == sum(not r["flag"] & 0x900 for r in recs) < 60
        seen = _compare(ctx, [paths["sam"]], mb, passthrough=True)         # parsed on the host: the qualities are uploaded; '*' for a read without
        assert seen["reads"] == 60 and seen["none"] == n_noq
    seen = _compare(ctx, [paths["bam"]], 10 ** 9, chunk=10 ** 6)
    assert seen["batches"] == 1 and seen["reads"] == 60
    seen = _compare(ctx, [corpora_fastq(tmp_path), paths["bam"]], 10 ** 9)  # a FASTQ file, then the BAM: runs of two files in one walk
    assert seen["reads"] >= 3


def corpora_fastq(tmp_path):
    p = tmp_path / "front.fq"
    p.write_bytes(_fastq(_recs(np.random.default_rng(2), [30, 4097, 8], b"z")))
    return p


@pytest.mark.gpu
def test_error_batch_holds_the_reads_in_front_of_the_bad_record(ctx, corpora, tmp_path):
    for mb in (1, 10 ** 9):
        seen = _compare(ctx, [corpora["mismatch"]], mb)
        assert seen["err"] is not None and seen["err"][0] != 0 and "quality string of" in seen["err"][1]
        assert seen["reads"] == 2 and seen["bytes"] == 650
    assert seen["batches"] == 1 and seen["last"] == 2                      # the error batch itself: two reads, two ranges
    # a compression fault and a bad BAM record: the batch in front of them
    edge = corpora["edge"].read_bytes()
    bz = bytearray(bgzf.bgzf_compress(edge, block=4000))
    io_, _ = bgzf.blocks(bytes(bz))
    bz[io_[3] - 8] ^= 1                                                    # the third member's CRC
    p = tmp_path / "crc.fq.gz"; p.write_bytes(bytes(bz))
    seen = _compare(ctx, [p], 10 ** 9, compressed_text=True)
    assert seen["err"] is not None and 0 < seen["reads"] < len(EDGE_LENGTHS)
    from test_input_bam import _rand_recs
    raw = bytearray(bgzf.bam_bytes(_rand_recs(np.random.default_rng(6), 20)))
    p = tmp_path / "cut.bam"; p.write_bytes(bgzf.bgzf_compress(bytes(raw[:len(raw) - 37]), 6))   # the last record is cut by the end of the file
    seen = _compare(ctx, [p], 10 ** 9)
    assert seen["err"] is not None and seen["reads"] == 19


# ---- the record stage fed from the reader ------------------------------------------------------------------------------------------------------------------
def _reader_batch(ctx, files, **kw):
    from lra_amd import reads_io
    rf = reads_io.ReadsFile([str(f) for f in files], ctx=ctx, chunk=64 << 10, device_quals=True, no_host_copy=True, **kw)
    return rf, rf.next_batch(10 ** 9)


def _three_ways(mapper, res, b, names, reads, quals, tags, md):
    """records_device from the reader's arrays (stub quals, no host reads) == records_device with uploaded qualities == lra_map_records_host_tags"""
    full = mapper.record_args(names, reads, quals)
    host = mapper.records_host(mapper.snapshot(res, md=md), full, passthrough=list(tags) if tags is not None else [None] * len(names))
    up = mapper.records_device(res, full, passthrough=tags, md=md)
    st_up = mapper.records_device_stats()
    rd = mapper.records_device(res, mapper.record_args(names, None, b["quals"], lens=b["read_len"]), passthrough=tags, md=md, d_qual=b["d_qual"], d_qual_off=b["d_qual_off"])
    st_rd = mapper.records_device_stats()
    for i, (x, y, z) in enumerate(zip(rd, up, host)):
        assert x == y == z, "read %d: %d / %d / %d bytes" % (i, len(x), len(y), len(z))
    assert len(rd) == len(up) == len(host) == len(names)                   # text and rec_off: the same cut into reads
    assert st_rd["text_bytes"] == st_up["text_bytes"] == sum(len(t) for t in host)
    if chr(mapper.copts.printFormat) == "s" and any(q is not None for q in quals):
        assert st_rd["bytes_h2d"] < st_up["bytes_h2d"], (st_rd["bytes_h2d"], st_up["bytes_h2d"])   # no quality byte goes up
    else:
        assert st_rd["bytes_h2d"] == st_up["bytes_h2d"]                    # (PAF prints no qualities: nothing to upload either way)
    return host


@pytest.mark.gpu
def test_records_from_the_readers_arrays_ont(ctx, tmp_path):
    import torch
    from lra_amd import reads_io
    from test_records_device import _ont_setup, _quals, _set
    mapper, reads, rng = _ont_setup(ctx)
    n = len(reads)
    names = [b"read/%d" % i for i in range(n)]
    quals = _quals(rng, reads)
    quals[0] = None                                                        # read 0 comes from a FASTA file: no qualities
    quals[n - 1] = b"*" + quals[n - 1][1:]                                 # an unaligned read whose string starts with '*'
    (tmp_path / "first.fa").write_bytes(b">%s\n%s\n" % (names[0], reads[0]))
    (tmp_path / "rest.fq").write_bytes(_fastq([(names[i], reads[i], quals[i]) for i in range(1, n)]))
    tags = [None if i % 3 == 0 else b"XA:i:%d\tXZ:Z:t%d" % (i, i) for i in range(n)]
    rf, b = _reader_batch(ctx, [tmp_path / "first.fa", tmp_path / "rest.fq"])
    try:
        assert b["names"] == names and b["seqs"] is None and b["read_len"] == [len(r) for r in reads]
        assert b["quals"] == [None if q is None else q[:1] for q in quals]
        res = reads_io.map_reads_device(mapper, b)
        seen = dict(rev=0, supp=0, un=0, hclip=0, md=0, star=0)
        for hard, md in ((0, False), (1, True)):
            _set(mapper, printFormat="s", hardClip=hard, PrintNumAln=1)
            for t in _three_ways(mapper, res, b, names, reads, quals, tags, md):
                for line in t.split(b"\n")[:-1]:
                    f = line.split(b"\t")
                    fl = int(f[1])
                    seen["rev"] += bool(fl & 16); seen["supp"] += bool(fl & 2048); seen["un"] += bool(fl & 4); seen["hclip"] += b"H" in f[5]
                    seen["md"] += b"\tMD:Z:" in line; seen["star"] += f[10] == b"*"
        assert seen["rev"] >= 3 and seen["supp"] >= 3 and seen["un"] >= 4 and seen["hclip"] >= 1 and seen["md"] >= n - 2 and seen["star"] >= 2, seen
        _three_ways(mapper, res, b, names, reads, quals, None, False)      # no passthrough
        # a flagged read (LRA_ST_CAPACITY = 8, set the way test_records_device.py sets it) printed as unaligned
        one = torch.tensor([8], dtype=torch.int32, device=ctx.device)
        ctx.check(ctx.lib.lra_copy_device(ctx.h, C.c_void_p(res.d_read_status + 3 * 4), C.c_void_p(one.data_ptr()), C.c_uint64(4)))
        torch.cuda.synchronize()
        _set(mapper, flagged_unaligned=1)
        host = _three_ways(mapper, res, b, names, reads, quals, tags, False)
        assert host[3] != b"" and int(host[3].split(b"\t")[1]) & 4
        _set(mapper, flagged_unaligned=0)
    finally:
        rf.close()


@pytest.mark.gpu
def test_records_from_the_readers_arrays_ccs_bam(ctx, tmp_path):
    from lra_amd import mapread, reads_io
    from test_records_device import _quals, _set
    import test_highacc_path as H
    g = H._genome_with_repeats(19)
    rng = np.random.default_rng(8)
    reads = [r.tobytes() for r in H._sv_reads(g, rng, 0.01, n_plain=4)]
    mapper = mapread.HighAccMapper(ctx, g, None, None, [b"chrA", b"chrB"], [0, 250_000, len(g)], "ccs", index_params=(17, 10, 150, 15, 1))
    n = len(reads)
    names = [b"ccs%d" % i for i in range(n)]
    quals = _quals(rng, reads)
    quals[1] = None                                                        # a BAM record with 0xff qualities
    bgzf.write_bam(str(tmp_path / "r.bam"), [dict(name=names[i], seq=reads[i], qual=quals[i], flag=4, aux=[("RG", "Z", "g%d" % i)]) for i in range(n)])
    rf, b = _reader_batch(ctx, [tmp_path / "r.bam"], passthrough=True)
    try:
        assert b["names"] == names and b["seqs"] is None and b["tags"] == [b"RG:Z:g%d" % i for i in range(n)]
        res = reads_io.map_reads_device(mapper, b)
        for hard, md, fmt in ((0, False, "s"), (1, True, "s"), (0, False, "P")):
            _set(mapper, printFormat=fmt, hardClip=hard)
            host = _three_ways(mapper, res, b, names, reads, quals, b["tags"], md)
            assert all(host) if fmt == "s" else any(b"CG:z:" in t for t in host)      # (PAF prints nothing for an unaligned read)
    finally:
        rf.close()


# ---- the tool --------------------------------------------------------------------------------------------------------------------------------------------
def _tool(tmp_path, args, extra):
    out = str(tmp_path / ("o%d.sam" % len(extra)))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_files.py"), *args, "-o", out, *extra], capture_output=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return open(out, "rb").read()


@pytest.mark.gpu
def test_map_files_device_records_ont_fastq(tmp_path):
    rng = np.random.default_rng(21)
    genome = synth.make_genome(120_000, seed=5, repeat_frac=0.1, n_families=2)
    (tmp_path / "g.fa").write_bytes(b">chr1 test\n" + genome.tobytes() + b"\n")
    with open(tmp_path / "r.fq", "wb") as f:
        for i, a in enumerate((5000, 40_000, 80_000, 20_000)):
            r = synth.simulate_read(rng, genome[a:a + 4001], 4000, 0.08, (30, 35, 35), i == 1)[0].tobytes()
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, bytes(rng.integers(34, 74, len(r)).astype(np.uint8))))
    args = ["-ONT", str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), "-H", "--printMD", "--batch-bases", "7000"]
    a, b = _tool(tmp_path, args, []), _tool(tmp_path, args, ["--device-records"])
    assert a == b and a.count(b"\n") >= 6                                  # (the @PG line quotes lra's command line: the same for both)


@pytest.mark.gpu
def test_map_files_device_records_ccs_bam_passthrough(tmp_path):
    genome = synth.make_genome(200_000, seed=3, repeat_frac=0.2, n_families=2)
    s = genome.tobytes()
    (tmp_path / "g.fa").write_bytes(b">chr1\n" + b"\n".join(s[x:x + 70] for x in range(0, len(s), 70)) + b"\n")
    reads, _ = synth.simulate_reads(genome, 10, 4000, 1000, 0.01, seed=11)
    recs = [dict(name=b"m%d" % i, seq=r.tobytes(), qual=None if i == 4 else b"5" * len(r), flag=4 if i % 6 else 0x904, aux=[("RG", "Z", "x%d" % i)]) for i, r in enumerate(reads)]
    bgzf.write_bam(str(tmp_path / "r.bam"), recs)
    args = ["-CCS", str(tmp_path / "g.fa"), str(tmp_path / "r.bam"), "--passthrough", "--batch-bases", "15000"]
    a, b = _tool(tmp_path, args, []), _tool(tmp_path, args, ["--device-records"])
    body = [l for l in a.split(b"\n") if l and not l.startswith(b"@")]
    assert a == b and len({l.split(b"\t")[0] for l in body}) == 10 and all(l.split(b"\t")[-1].startswith(b"RG:Z:x") for l in body)
