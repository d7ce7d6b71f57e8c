"""gzip and BGZF FASTA / FASTQ read files through lra_reads_next_batch_device: the host form's batches (tests/test_compressed_reads.py holds the corpora), the
same first fault and the same reads in front of it, at step sizes that cut members and records.  One reader per case; nothing is read again after a fault."""
import numpy as np
import pytest

from test_compressed_reads import corpus, fault_files, flat, read_all, variants, whole_records, write
from test_input_bam import _check_device_arrays

CHUNKS = (4096, 4097, 10 ** 6)     # the minimum (many steps, members cut by steps, a 3000-base record longer than a step), one off it, one step for all


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """the compressed files of both corpora and the host form's batches of each, made once"""
    d = tmp_path_factory.mktemp("zreads")
    out = []
    for kind in ("fasta", "fastq"):
        text = corpus(kind)
        for name, data in variants(text).items():
            p = write(d / (name + "." + kind + ".gz"), data)
            out.append((p, {mb: read_all([p], mb) for mb in (5000, 10 ** 9)}))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
def test_device_form_matches_host_form(ctx, cases, chunk):
    for p, host in cases:
        for mb, exp in host.items():
            assert exp[1] is None and len(flat(exp[0])) >= 30
            got = read_all([p], mb, ctx=ctx, chunk=chunk, check=lambda b: _check_device_arrays(ctx, b))
            assert got == exp, (p, mb, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
def test_device_form_faults(ctx, tmp_path, chunk):
    for kind in ("fasta", "fastq"):
        text = corpus(kind, 31, 30, zero_len=False, final_newline=True)
        plain = flat(read_all([write(tmp_path / ("plain" + kind), text)], 10 ** 9)[0])
        for name, path, good, at in fault_files(tmp_path, kind, text):
            host = read_all([path], 5000)
            got = read_all([path], 5000, ctx=ctx, chunk=chunk, check=lambda b: _check_device_arrays(ctx, b))
            assert got[1] is not None and got[1] == host[1] and path in got[1], (name, got[1], host[1])
            assert ("compressed offset %d " % at) in got[1]
            assert flat(got[0]) == flat(host[0]), (name, chunk)
            if good is not None:
                assert flat(got[0]) == plain[:whole_records(kind, good)], name


@pytest.mark.gpu
def test_device_form_quality_mismatch_and_file_list(ctx, tmp_path):
    from lra_amd import bgzf
    text = corpus("fastq", 41, 20, zero_len=False)
    lines = text.split(b"\n")
    lines[4 * 9 + 3] = lines[4 * 9 + 3][:-3]
    bad = b"\n".join(lines)
    for name, data in (("bgzf", bgzf.bgzf_compress(bad, block=3000)), ("gz", bgzf.gzip_compress(bad))):
        z = write(tmp_path / (name + ".gz"), data)
        host = read_all([z], 5000)
        assert host[1] is not None and "quality string" in host[1] and len(flat(host[0])) == 9
        assert read_all([z], 5000, ctx=ctx, chunk=4096) == host, name
    texts = [corpus("fastq", 21, 12, final_newline=True), corpus("fastq", 22, 12, zero_len=False, final_newline=True), corpus("fastq", 23, 12, final_newline=True),
             corpus("fasta", 24, 12)]
    files = [write(tmp_path / "p0", texts[0]), write(tmp_path / "m1.gz", bgzf.gzip_compress(texts[1])), write(tmp_path / "m2.gz", bgzf.bgzf_compress(texts[2], block=777)),
             write(tmp_path / "m3.gz", bgzf.bgzf_compress(texts[3], block=3000))]
    plain = [write(tmp_path / ("q%d" % i), t) for i, t in enumerate(texts)]
    for mb in (5000, 10 ** 9):
        exp = read_all(plain, mb)
        assert read_all(files, mb) == exp
        assert read_all(files, mb, ctx=ctx, chunk=4097, check=lambda b: _check_device_arrays(ctx, b)) == exp
