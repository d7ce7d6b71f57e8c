"""lra_reads_next_batch_device (lra_amd/csrc/input_device.hip): FASTA / FASTQ parsed on the device into the same batches as lra_reads_next_batch -- names,
bases, qualities, batch cuts, the error of a corrupt FASTQ record and its stickiness -- at the default step size and at steps of a few KiB that cut lines,
records, header names, CRLF pairs and quality lines; the device arrays; the two forms on one reader; mapping straight from the device arrays."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lra_amd import synth
from test_input import _write_files, ref_batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = [([0, 1], 500), ([2, 3, 4], 300), ([0, 1], 10 ** 9), ([2, 1], 100), ([1, 2, 4], 1)]   # test_input.py::test_reader_matches_reference_logic's


def _read_all(files, max_bases, ctx=None, chunk=None):
    """every batch of a reader -> (batches of (name, seq, qual), error text or None); the device form's arrays are checked against its host arrays"""
    from lra_amd import reads_io
    rf = reads_io.ReadsFile(files, ctx=ctx, chunk=chunk)
    got, failed = [], None
    try:
        while True:
            try:
                b = rf.next_batch(max_bases)
            except IOError as e:
                failed = str(e).split(": ", 1)[1]
                if e.partial is not None:
                    got.append(list(zip(e.partial["names"], e.partial["seqs"], e.partial["quals"])))
                    if ctx is not None:
                        _check_device_arrays(ctx, e.partial)
                with pytest.raises(IOError):                               # and it stays one
                    rf.next_batch(max_bases)
                break
            if b is None:
                break
            if ctx is not None:
                _check_device_arrays(ctx, b)
            got.append(list(zip(b["names"], b["seqs"], b["quals"])))
    finally:
        rf.close()
    return got, failed


def _check_device_arrays(ctx, b):
    n, tot = b["n"], b["total_bases"]
    seq = ctx.to_host(b["d_seq"], tot + 64, np.uint8).tobytes()
    assert seq == b"".join(b["seqs"]) + bytes(64)
    assert seq[:tot] == C.string_at(b["raw"].seq, tot + 64)[:tot] and C.string_at(b["raw"].seq, tot + 64)[tot:] == bytes(64)
    assert np.array_equal(ctx.to_host(b["d_off"], n + 1, np.uint64), b["off"]) and b["off"][0] == 0


def _same_as_host(files, max_bases, ctx, chunk=None, ref=True):
    exp = ref_batches(files, max_bases) if ref else None
    host, host_err = _read_all(files, max_bases)
    dev, dev_err = _read_all(files, max_bases, ctx=ctx, chunk=chunk)
    if ref:
        assert host == exp
    assert dev_err == host_err, (dev_err, host_err)
    assert len(dev) == len(host), (len(dev), len(host))
    for i, (d, h) in enumerate(zip(dev, host)):
        assert d == h, (i, [x[0] for x in d][:5], [x[0] for x in h][:5])
    return dev, dev_err


def test_set_device_chunk_limits(tmp_path):
    """CPU: lra_reads_set_device_chunk takes 4096 bytes and more, and is refused on a reader that has used the host form"""
    from lra_amd import reads_io
    from lra_amd._lib import load_library
    lib = load_library()
    files = _write_files(tmp_path)
    rf = reads_io.ReadsFile(files[:2])
    assert lib.lra_reads_set_device_chunk(rf.h, C.c_uint64(4095)) != 0
    assert lib.lra_reads_set_device_chunk(rf.h, C.c_uint64(4096)) == 0
    assert lib.lra_reads_set_device_chunk(rf.h, C.c_uint64(256 << 20)) == 0
    assert rf.next_batch(500) is not None
    assert lib.lra_reads_set_device_chunk(rf.h, C.c_uint64(4096)) != 0     # the host form now owns the file position
    rf.close()
    with pytest.raises(ValueError):
        reads_io.ReadsFile(files[:2], chunk=100)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 4096, 4099, 6007])
@pytest.mark.parametrize("order,max_bases", ORDERS)
def test_device_reader_matches_host_reader(ctx, tmp_path, order, max_bases, chunk):
    files = _write_files(tmp_path)
    sel = [files[i] for i in order]
    got, err = _same_as_host(sel, max_bases, ctx, chunk)
    assert sum(len(b) for b in got) >= 3
    if 4 in order:
        assert err and "short_quality" in err and "e.fq" in err, err
    else:
        assert err is None


def _rand_bases(rng, n):
    s = np.frombuffer(b"ACGTacgtN", np.uint8)[rng.integers(0, 9, n)].copy()
    if n > 50 and rng.random() < 0.5:                                       # a run of N
        a = int(rng.integers(0, n - 20)); s[a:a + int(rng.integers(5, 20))] = ord("N")
    return bytes(s)


def _rand_fasta(rng, n_rec, wrap, eol, max_len=900):
    out = []
    for i in range(n_rec):
        lead = b" \t"[: int(rng.integers(0, 3))]
        name = (b"r%d" % i) if rng.random() < 0.9 else b""
        out.append(lead + b">" + (b" " if rng.random() < 0.2 else b"") + name + (b"\tdesc %d" % i if rng.random() < 0.5 else b"") + eol)
        n = 0 if rng.random() < 0.1 else int(rng.integers(1, max_len))     # a zero-length record now and then
        s = _rand_bases(rng, n)
        if rng.random() < 0.2 and n > 10:
            s = s[:5] + b"\t" + s[5:]
        w = wrap or max(1, len(s))
        for x in range(0, len(s), w):
            out.append(s[x:x + w] + eol)
            if rng.random() < 0.05:
                out.append(eol if rng.random() < 0.5 else b"\n")            # blank lines inside the record
    data = b"".join(out)
    if not data.startswith(b">"):
        data = b">first" + eol + data
    if rng.random() < 0.5:
        data = data.rstrip(b"\n")                                           # no final newline
    return data


def _rand_fastq(rng, n_rec, eol, max_len=700):
    out = []
    for i in range(n_rec):
        n = int(rng.integers(1, max_len))
        s = _rand_bases(rng, n)
        q = bytes(rng.integers(33, 74, n).astype(np.uint8))
        if rng.random() < 0.3:
            q = b">@"[int(rng.integers(0, 2)):][:1] + q[1:]                 # '>' or '@' opening a quality line
        if rng.random() < 0.1:
            s = s[:n // 2] + b" " + s[n // 2:]; q = q[:n // 3] + b"  " + q[n // 3:]
        out.append(b"@q%d %d%s%s%s+%s%s%s" % (i, n, eol, s, eol, eol, q, eol))
    return b"".join(out)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_device_reader_random_corpora(ctx, tmp_path, seed):
    """FASTA wrapped at 1 / 60 / 80 columns and unwrapped, CRLF line ends, tabs, lower case, runs of N, '>' and '@' at the start of quality lines, blank
    lines, zero-length records, headers behind blanks, no final newline; at steps that cut all of them"""
    rng = np.random.default_rng(100 + seed)
    files = []
    for k, wrap in enumerate([1, 60, 80, None]):
        eol = b"\r\n" if (seed + k) % 3 == 0 else b"\n"
        p = tmp_path / ("f%d.fa" % k)
        p.write_bytes(_rand_fasta(rng, int(rng.integers(3, 30)), wrap, eol, max_len=300 if wrap == 1 else 900))
        files.append(str(p))
    for k in range(2):
        p = tmp_path / ("q%d.fq" % k)
        p.write_bytes(_rand_fastq(rng, int(rng.integers(3, 25)), b"\r\n" if (seed + k) % 2 else b"\n"))
        files.append(str(p))
    order = [files[i] for i in rng.permutation(len(files))]
    for chunk in (None, 4096, int(rng.integers(4096, 9000))):
        for max_bases in (1, 1000, 10 ** 9):
            _same_as_host(order, max_bases, ctx, chunk)


@pytest.mark.gpu
def test_device_reader_reads_longer_than_a_step(ctx, tmp_path):
    """a FASTA read and a FASTQ read several 4 KiB steps long, between short ones"""
    rng = np.random.default_rng(7)
    fa = tmp_path / "long.fa"; fq = tmp_path / "long.fq"
    seqs = [_rand_bases(rng, n) for n in (300, 23_456, 70, 9_000)]
    fa.write_bytes(b"".join(b">L%d x\n" % i + b"\n".join(s[x:x + 60] for x in range(0, len(s), 60)) + b"\n" for i, s in enumerate(seqs)))
    fq.write_bytes(b"".join(b"@Q%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs)))
    for chunk in (4096, 5000):
        for mb in (1, 10_000, 10 ** 9):
            got, _ = _same_as_host([str(fa), str(fq)], mb, ctx, chunk)
            assert max(len(s) for b in got for _, s, _ in b) == 23_456


@pytest.mark.gpu
def test_device_reader_file_edges(ctx, tmp_path):
    """an empty file and a file of unknown format: refused first (as by the host form), ending the input silently behind another file; FASTQ files that
    end without a newline, with a blank line, or whose first record has an empty line after a file that ended"""
    from lra_amd import reads_io
    empty = tmp_path / "empty.fa"; empty.write_bytes(b"")
    junk = tmp_path / "junk.txt"; junk.write_bytes(b"hello\nworld\n")
    fq2 = tmp_path / "two_lines.fq"; fq2.write_bytes(b"@a\nACGT")
    for f in (empty, junk, fq2):
        with pytest.raises(IOError):
            reads_io.ReadsFile([str(f)])
        with pytest.raises(IOError):
            reads_io.ReadsFile([str(f)], ctx=ctx)
    good = tmp_path / "good.fa"; good.write_bytes(b">g1\nACGT\n>g2\nTTTT\n")
    nonl = tmp_path / "nonl.fq"; nonl.write_bytes(b"@n1\nACGT\n+\nIIII\n@n2\nGG\n+\nII")
    blank = tmp_path / "blank.fq"; blank.write_bytes(b"@b1\nAC\n+\nII\n\n@b2\nGG\n+\nJJ\n")
    first_empty = tmp_path / "first_empty.fq"; first_empty.write_bytes(b"@e1\nAC\n+\n\n@e2\nGG\n+\nJJ\n@e3\nTT\n+\nKK\n")
    short = tmp_path / "short.fq"; short.write_bytes(b"@s1\nACGT\n+\nIIII\n@s2\nAC\n")
    crlf = tmp_path / "crlf.fq"; crlf.write_bytes(b"@c1\r\nACGT\r\n+\r\nIIII\r\n@c2\r\nGG\r\n+\r\nJJ\r\n")
    for order in ([good, empty, good], [good, junk], [blank, first_empty, good], [nonl, good], [short, blank, good], [crlf, good, first_empty],
                  [blank, blank], [first_empty]):
        for mb in (1, 3, 10 ** 9):
            _same_as_host([str(x) for x in order], mb, ctx, 4096)


@pytest.mark.gpu
def test_reader_forms_do_not_mix(ctx, tmp_path):
    from lra_amd import reads_io
    files = _write_files(tmp_path)
    rf = reads_io.ReadsFile(files[:2], ctx=ctx)
    assert rf.next_batch(500) is not None
    b = reads_io.ReadBatchC()
    assert rf.lib.lra_reads_next_batch(rf.h, C.c_uint64(500), C.byref(b)) != 0 and b.n_reads == 0
    assert rf.next_batch(500) is not None                                  # the device form goes on where it was
    rf.close()
    rf = reads_io.ReadsFile(files[:2])
    assert rf.next_batch(500) is not None
    d_seq, d_off = C.c_void_p(), C.c_void_p()
    assert rf.lib.lra_reads_next_batch_device(rf.h, ctx.h, C.c_uint64(500), C.byref(b), C.byref(d_seq), C.byref(d_off)) != 0 and b.n_reads == 0
    assert rf.next_batch(500) is not None
    rf.close()


def _genome_and_reads(tmp_path, err, seed):
    genome = synth.make_genome(400_000, seed=9, repeat_frac=0.2, n_families=3)
    CH = [0, 150_000, len(genome)]
    reads, _ = synth.simulate_reads(genome, 24, 6000, 1500, err, seed=seed)
    fq = tmp_path / "reads.fq"; fa = tmp_path / "reads.fa"
    with open(fq, "wb") as f:
        for i, r in enumerate(reads):
            s = r.tobytes()
            f.write(b"@r%d len=%d\n%s\n+\n%s\n" % (i, len(s), s.lower() if i % 3 == 0 else s, b"I" * len(s)))
    with open(fa, "wb") as f:
        for i, r in enumerate(reads):
            s = r.tobytes()
            f.write(b">w%d\n" % i + b"\n".join(s[x:x + 80] for x in range(0, len(s), 80)) + b"\n")
    return genome, CH, [str(fq), str(fa)]


def _records_both_forms(ctx, mapper, files, chunk):
    from lra_amd import reads_io
    out = []
    for use_dev in (False, True):
        rf = reads_io.ReadsFile(files, ctx=ctx if use_dev else None, chunk=chunk if use_dev else None)
        texts, n_batches = [], 0
        while True:
            b = rf.next_batch(60_000)
            if b is None:
                break
            res = reads_io.map_reads_device(mapper, b) if use_dev else reads_io.map_reads_host(mapper, b["raw"])
            texts += mapper.records(res, b["names"], b["seqs"], quals=b["quals"])
            n_batches += 1
        rf.close()
        out.append((texts, n_batches))
    return out


@pytest.mark.gpu
def test_map_reads_device_ont(ctx, tmp_path):
    """FASTQ and wrapped FASTA read files -> lra_reads_next_batch_device -> the -ONT driver on the reader's device arrays: the records of
    lra_reads_next_batch + lra_map_reads_host"""
    from lra_amd import mapread
    genome, CH, files = _genome_and_reads(tmp_path, 0.10, 4)
    o = mapread.LowAccOptions()
    ik, ip = synth.build_global_index(genome, o.globalK, o.globalW, 100)
    mapper = mapread.LowAccMapper(ctx, genome, ik, ip, [b"chrA", b"chrB"], CH, o)
    (h, hn), (d, dn) = _records_both_forms(ctx, mapper, files, 64 << 10)
    assert hn == dn >= 4 and len(d) == 48 and d == h
    assert sum(b"\t*\t0\t0\t" not in t for t in d) >= 40


@pytest.mark.gpu
def test_map_reads_device_ccs(ctx, tmp_path):
    """the same through the -CCS driver (lra_map_reads_highacc_batch)"""
    from lra_amd import mapread
    genome, CH, files = _genome_and_reads(tmp_path, 0.01, 6)
    mapper = mapread.HighAccMapper(ctx, genome, None, None, [b"chrA", b"chrB"], CH, preset="ccs")
    (h, hn), (d, dn) = _records_both_forms(ctx, mapper, files, 64 << 10)
    assert hn == dn >= 4 and len(d) == 48 and d == h
    assert sum(b"\t*\t0\t0\t" not in t for t in d) >= 40


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["-ONT", "-CCS"])
def test_map_files_tool_matches_host_input(tmp_path, preset):
    """tools/map_files.py on a small genome and read files: the SAM of the device reader equals that of the host reader byte for byte"""
    genome = synth.make_genome(300_000, seed=3, repeat_frac=0.2, n_families=2)
    g = tmp_path / "genome.fa"
    s = genome.tobytes()
    g.write_bytes(b">chr1 first\n" + b"\n".join(s[x:x + 70] for x in range(0, 200_000, 70)) + b"\n>chr2\n" +
                  b"\n".join(s[x:x + 70] for x in range(200_000, len(s), 70)) + b"\n")
    reads, _ = synth.simulate_reads(genome, 30, 5000, 1500, 0.08 if preset == "-ONT" else 0.01, seed=11)
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"".join(b"@m%d\n%s\n+\n%s\n" % (i, r.tobytes(), b"5" * len(r)) for i, r in enumerate(reads)))
    outs = []
    for extra in ([], ["--host-input"]):
        o = tmp_path / ("out%d.sam" % len(extra))
        cmd = [sys.executable, os.path.join(ROOT, "tools", "map_files.py"), preset, str(g), str(fq), "-o", str(o), "--batch-bases", "40000", *extra]
        p = subprocess.run(cmd, capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        outs.append(o.read_bytes())
    assert outs[0] == outs[1]
    body = [l for l in outs[0].split(b"\n") if l and not l.startswith(b"@")]
    assert outs[0].startswith(b"@") and len({l.split(b"\t")[0] for l in body}) == 30
