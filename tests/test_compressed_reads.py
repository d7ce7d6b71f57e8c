"""gzip and BGZF FASTA / FASTQ read files (lra_reads_open_flags with LRA_READS_COMPRESSED_TEXT), host form: a compressed file yields exactly the batches its
decompressed bytes yield as a plain file; compression faults give LRA_ERR_INVALID with the whole records in front of the fault.  The corpora and helpers
here also serve tests/test_compressed_reads_device.py."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

from lra_amd import bgzf

MAX_BASES = (1, 5000, 10 ** 9)


def _bases(rng, n):
    s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes())
    for i in rng.integers(0, max(n, 1), n // 40):
        s[i] = ord("N")
    return bytes(s)


def corpus(kind, seed=11, n=40, zero_len=True, crlf=True, final_newline=False):
    """~n reads of 50-3000 bases: lower-case and N bases, CRLF lines, a read of length 0, multi-line FASTA, blanks in a sequence line, a final record
    without its newline.  (In FASTQ an empty sequence line ends the file, as the reference reads it: the read of length 0 is the third from the end.)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = 0 if (zero_len and i == n - 3) else 3000 if i in (5, 17) else int(rng.integers(50, 700))
        seq = _bases(rng, ln)
        if i % 5 == 1:
            seq = seq.lower()
        if i % 7 == 2 and ln > 10:
            seq = seq[:7] + b" " + seq[7:]
        eol = b"\r\n" if (crlf and i % 9 == 4) else b"\n"
        name = b"read_%d extra words" % i if i % 3 else b"r%d" % i
        if kind == "fasta":
            w = int(rng.integers(30, 90))
            lines = [seq[a:a + w] for a in range(0, len(seq), w)] if i % 2 else [seq]
            out.append(b">" + name + eol + b"".join(l + eol for l in lines))
        else:
            q = bytes((33 + rng.integers(0, 60, len(seq))).astype(np.uint8))
            if b" " in seq:
                q = q[:7] + b" " + q[8:]
            out.append(b"@" + name + eol + seq + eol + b"+" + eol + q + eol)
    text = b"".join(out)
    return text if final_newline else text.rstrip(b"\r\n")


def rand_cuts(rng, n, lo=50, hi=400):
    cuts, p = [], 0
    while True:
        p += int(rng.integers(lo, hi + 1))
        if p >= n:
            return cuts
        cuts.append(p)


def variants(text, seed=3):
    """name -> the file's bytes, for every way the issue lists of storing `text` compressed"""
    rng = np.random.default_rng(seed)
    k = len(text) // 2 + 17
    v = {
        "bgzf": bgzf.bgzf_compress(text),
        "bgzf_cuts": bgzf.bgzf_compress(text, cuts=rand_cuts(rng, len(text))),
        "bgzf_empty_mid": bgzf.bgzf_compress(text[:k], eof=False) + bgzf.member(b"") + bgzf.bgzf_compress(text[k:], eof=True),
        "bgzf_empty_mid_noeof": bgzf.bgzf_compress(text[:k], block=5000, eof=False) + bgzf.member(b"") + bgzf.bgzf_compress(text[k:], block=5000, eof=False),
        "gz0": bgzf.gzip_compress(text, 0), "gz1": bgzf.gzip_compress(text, 1), "gz9": bgzf.gzip_compress(text, 9),
        "gz_fixed": bgzf.gzip_compress(text, 6, zlib.Z_FIXED),
        "gz_3members": bgzf.gzip_compress(text, 6, cuts=(len(text) // 3 + 1, 2 * len(text) // 3 + 5), fname=b"reads.fq", fextra=b"XY\x03\x00abc", fhcrc=True),
    }
    return v


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def read_all(files, max_bases, ctx=None, chunk=None, compressed_text=True, check=None):
    """-> (batches, error text or None): a batch is a list of (name, bases, quality or None) plus its offsets and lengths checked against them"""
    from lra_amd import reads_io
    rf = reads_io.ReadsFile(files, ctx=ctx, chunk=chunk, compressed_text=compressed_text)
    got, failed = [], None

    def rows(b):
        n = len(b["names"])
        assert [int(b["off"][i + 1] - b["off"][i]) for i in range(n)] == [len(s) for s in b["seqs"]] == [b["raw"].read_len[i] for i in range(n)]
        if check is not None:
            check(b)
        return list(zip(b["names"], b["seqs"], b["quals"]))
    try:
        while True:
            try:
                b = rf.next_batch(max_bases)
            except IOError as e:
                failed = str(e).split(": ", 1)[1]
                assert e.rc == -1 or e.rc != 0
                if e.partial is not None:
                    got.append(rows(e.partial))
                with pytest.raises(IOError) as again:                             # sticky
                    rf.next_batch(max_bases)
                assert str(again.value).split(": ", 1)[1] == failed and again.value.partial is None
                break
            if b is None:
                break
            got.append(rows(b))
    finally:
        rf.close()
    return got, failed


def whole_records(kind, good_text):
    """how many records are whole in the bytes in front of a fault (input.hip's decision 4)"""
    if kind == "fastq":
        return good_text.count(b"\n") // 4
    return max(0, len(re.findall(rb"(?:^|\n)>", good_text)) - 1)


def fault_files(tmp_path, kind, text):
    """(name, path, the decompressed bytes in front of the fault or None if the test cannot know them, the member's compressed offset) for gzip and BGZF"""
    out = []
    bz = bgzf.bgzf_compress(text, block=4000, eof=True)
    io_, oo = bgzf.blocks(bz)
    k = len(io_) // 2
    gz = bgzf.gzip_compress(text, 6)
    gz3 = bgzf.gzip_compress(text, 6, cuts=(len(text) // 2,))
    second = len(bgzf.gzip_member(text[:len(text) // 2], 6))

    def flip(data, at):
        b = bytearray(data); b[at] ^= 0x01
        return bytes(b)
    out.append(("bgzf_truncated", bz[:io_[k] + 40], text[:oo[k]], io_[k]))
    out.append(("bgzf_crc", flip(bz, io_[k + 1] - 8), text[:oo[k]], io_[k]))
    out.append(("bgzf_isize", flip(bz, io_[k + 1] - 4), text[:oo[k]], io_[k]))
    out.append(("bgzf_trailing", bz + b"trailing bytes", text, len(bz)))
    out.append(("gz_truncated", gz[:len(gz) * 3 // 5], None, 0))
    out.append(("gz_crc", flip(gz, len(gz) - 8), text, 0))
    out.append(("gz_isize", flip(gz, len(gz) - 4), text, 0))
    out.append(("gz_trailing", gz + b"trailing bytes", text, len(gz)))
    out.append(("gz_second_member_crc", flip(gz3, len(gz3) - 8), text, second))
    return [(name, write(tmp_path / (name + "." + kind + ".gz"), data), good, at) for name, data, good, at in out]


def flat(batches):
    return [r for b in batches for r in b]


# ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fasta", "fastq"])
def test_compressed_files_give_the_plain_files_batches(tmp_path, kind):
    text = corpus(kind)
    plain = write(tmp_path / ("plain." + kind), text)
    exp = {mb: read_all([plain], mb) for mb in MAX_BASES}
    assert exp[10 ** 9][1] is None and len(flat(exp[10 ** 9][0])) >= 30
    if kind == "fasta":
        assert all(q is None for _, _, q in flat(exp[1][0])) and any(len(s) == 0 for _, s, _ in flat(exp[1][0]))
    for name, data in variants(text).items():
        p = write(tmp_path / (name + "." + kind + ".gz"), data)
        for mb in MAX_BASES:
            assert read_all([p], mb) == exp[mb], (name, mb)


def test_file_list_of_plain_and_compressed(tmp_path):
    # (a FASTQ file without its last newline ends the reference's input: only the list's last file may lack it)
    texts = [corpus("fastq", 21, 12, final_newline=True), corpus("fastq", 22, 12, zero_len=False, final_newline=True), corpus("fastq", 23, 12, final_newline=True),
             corpus("fasta", 24, 12)]
    plain = [write(tmp_path / ("p%d" % i), t) for i, t in enumerate(texts)]
    mixed = [plain[0], write(tmp_path / "m1.gz", bgzf.gzip_compress(texts[1], 6)), write(tmp_path / "m2.gz", bgzf.bgzf_compress(texts[2], cuts=rand_cuts(np.random.default_rng(1), len(texts[2])))),
             write(tmp_path / "m3.gz", bgzf.bgzf_compress(texts[3], block=3000))]
    for mb in MAX_BASES:
        exp = read_all(plain, mb)
        assert exp[1] is None and len(flat(exp[0])) >= 30                        # (an empty batch where a FASTQ file hands over to the FASTA file ends max_bases = 1)
        if mb > 1:
            assert any(q is None for _, _, q in flat(exp[0]))                   # the FASTA file behind the three FASTQ files was read
        assert read_all(mixed, mb) == exp, mb


def test_refusals_and_bam_sam_unchanged(tmp_path):
    from lra_amd._lib import load_library
    from test_input_bam import _rand_recs, _read_all
    lib = load_library()

    def open_flags(path, flags):
        arr = (C.c_char_p * 1)(path.encode())
        h = C.c_void_p()
        rc = lib.lra_reads_open_flags(arr, 1, flags, C.byref(h))
        if rc == 0:
            lib.lra_reads_close(h)
        return rc
    for kind in ("fasta", "fastq"):
        for name, data in variants(corpus(kind, n=8)).items():
            p = write(tmp_path / (name + kind), data)
            with pytest.raises(IOError):
                read_all([p], 10 ** 9, compressed_text=False)                    # lra_reads_open
            assert open_flags(p, 0) != 0
            assert open_flags(p, 1) == 0
            assert open_flags(p, 2) != 0 and open_flags(p, 3) != 0               # an undefined flag
    recs = _rand_recs(np.random.default_rng(4), 20)
    bam = str(tmp_path / "x.bam"); sam = str(tmp_path / "x.sam.gz")
    raw = bgzf.write_bam(bam, recs)
    sam_text = bgzf.write_sam(sam, recs, bgzf=True)
    rng = np.random.default_rng(6)
    for name, data in (("gz_bam", bgzf.gzip_compress(raw)), ("gz_sam", bgzf.gzip_compress(sam_text)), ("gz_rnd", bgzf.gzip_compress(bytes(rng.integers(0, 256, 5000).astype(np.uint8)))),
                       ("gz_empty", bgzf.gzip_compress(b""))):
        assert open_flags(write(tmp_path / name, data), 1) != 0, name
    for p in (bam, sam):                                                        # BGZF BAM / SAM: as without the flag
        without = _read_all([p], 5000)
        got = read_all([p], 5000)
        assert without[1] is None and got[1] is None and got[0] == without[0] and len(flat(got[0])) == 20


@pytest.mark.parametrize("kind", ["fasta", "fastq"])
def test_compression_faults(tmp_path, kind):
    text = corpus(kind, 31, 30, zero_len=False, final_newline=True)
    plain = flat(read_all([write(tmp_path / "plain", text)], 10 ** 9)[0])
    behind = write(tmp_path / "behind.fa", b">never\nACGT\n")
    for name, path, good, at in fault_files(tmp_path, kind, text):
        for mb in (5000, 10 ** 9):
            got, err = read_all([path, behind], mb)
            assert err is not None, name
            assert path in err and ("compressed offset %d " % at) in err, (name, err)
            rows = flat(got)
            if good is None:
                assert 0 < len(rows) < len(plain) and rows == plain[:len(rows)], name
            else:
                assert rows == plain[:whole_records(kind, good)], (name, len(rows), whole_records(kind, good))


def test_quality_length_mismatch_inside_a_compressed_file(tmp_path):
    text = corpus("fastq", 41, 20, zero_len=False)
    lines = text.split(b"\n")
    lines[4 * 9 + 3] = lines[4 * 9 + 3][:-3]                                    # record 9: three qualities short
    bad = b"\n".join(lines)
    p = write(tmp_path / "bad.fq", bad)
    exp, exp_err = read_all([p], 5000)
    assert exp_err is not None and "quality string" in exp_err and len(flat(exp)) == 9
    for name, data in variants(bad).items():
        z = write(tmp_path / (name + ".gz"), data)
        got, err = read_all([z], 5000)
        assert got == exp and err == exp_err.replace(p, z), (name, err)
