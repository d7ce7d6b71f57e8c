"""The one BGZF step under the three device readers (lra_amd/csrc/zsource.hip: lra_bgzf_step) -- BGZF FASTQ, BAM and the genome FASTA -- against their host
forms, on the two things the shared step decides that the readers' own suites do not pin: which of two faults inside one step is reported, and a refill
that has to keep the carry of the step before it.  Small files at the smallest step, 4096 compressed bytes.  And the one gzip stream
(lra_gzip_source) where its data ends exactly at a step's end: that step is the last one."""
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genome_cases as gc   # noqa: E402
from lra_amd import bgzf
from lra_amd.genome_io import GenomeFile
from test_compressed_reads import corpus, flat, read_all, whole_records, write
from test_genome_input_device import same_in_both_forms
from test_input_bam import _check_device_arrays, _rand_recs, _read_all, _same_dev_host

STEP = 4096


def two_faults(data):
    """data as small BGZF members, the file cut inside member t and a CRC byte of an earlier member k flipped; everything inside the first step
    -> (the file, member k's compressed offset, the decompressed bytes in front of member k)"""
    z = bgzf.bgzf_compress(data, block=400, eof=False)
    io_, oo = bgzf.blocks(z)
    t = max(i for i in range(len(io_) - 1) if io_[i] + 20 <= STEP)
    k = t // 2
    assert 2 <= k < t - 1 and io_[t] + 20 < io_[t + 1]
    b = bytearray(z[:io_[t] + 20])
    b[io_[k + 1] - 8] ^= 1
    return bytes(b), io_[k], oo[k]


@pytest.mark.gpu
def test_first_bad_member_wins_over_the_truncation_behind_it(ctx, tmp_path):
    """one step holds a member with a CRC mismatch and, behind it, the member the end of the file cuts: every form names the first, and the reads in
    front of it are delivered"""
    # BGZF FASTQ
    text = corpus("fastq", 31, 12, zero_len=False, final_newline=True)
    blob, at, good = two_faults(text)
    p = write(tmp_path / "two.fq.gz", blob)
    want = "%s: a bad BGZF block at compressed offset %d (a CRC-32 mismatch)" % (p, at)
    plain = flat(read_all([write(tmp_path / "plain.fq", text)], 10 ** 9)[0])
    n = whole_records("fastq", text[:good])
    assert n >= 2
    for c, chunk in ((None, None), (ctx, STEP), (ctx, None)):
        got = read_all([p], 10 ** 9, ctx=c, chunk=chunk, check=(lambda b: _check_device_arrays(ctx, b)) if c else None)
        assert got[1] == want, (chunk, got[1])
        assert flat(got[0]) == plain[:n], chunk
    # BAM
    recs = _rand_recs(np.random.default_rng(5), 16, max_len=300)
    raw = bgzf.bam_bytes(recs)
    blob, at, good = two_faults(raw)
    p = write(tmp_path / "two.bam", blob)
    n = max(i for i in range(len(recs) + 1) if len(bgzf.bam_bytes(recs[:i])) <= good)
    assert n >= 2
    for chunk in (STEP, None):
        dev = _same_dev_host(ctx, [p], 10 ** 9, chunk)                    # (the host form against the Python reading, the device form against it)
        assert [x[0] for b in dev for x in b] == [r["name"] for r in recs[:n]]
    assert _read_all([p], 10 ** 9, ctx=ctx, chunk=STEP)[1] == "%s: a bad BGZF block at compressed offset %d (a CRC-32 mismatch)" % (p, at)
    # the genome (a read that fails delivers nothing: the text alone)
    data = gc.corpus(7, n_rec=6, plain=True)
    blob, at, _ = two_faults(data)
    p = write(tmp_path / "two.fa.gz", blob)
    for c, chunk in ((None, None), (ctx, STEP), (ctx, None)):
        g = GenomeFile(p, ctx=c, chunk=chunk)
        with pytest.raises(IOError):
            g.read()
        assert g.last_error() == "%s: a bad BGZF block at compressed offset %d (a CRC-32 mismatch)" % (p, at), chunk
        g.close()


def stored(data, first, size):
    """data as stored (level 0) members -- a member's compressed size is its data's plus 31 -- cut at `first`, then every `size` bytes"""
    z = bgzf.bgzf_compress(data, 0, cuts=[first] + list(range(first + size, len(data), size)))
    io_, oo = bgzf.blocks(z)
    assert all(b - a == (y - x) + 31 for a, b, x, y in zip(io_[:-2], io_[1:-1], oo[:-2], oo[1:-1]))
    return z, io_, oo


@pytest.mark.gpu
def test_refill_keeps_the_carry(ctx, tmp_path):
    """a short record, then one whose compressed span is several steps: the step behind the short record starts from a carry (the long record's head)
    and holds no whole record, so it is filled again, larger, from the same carry"""
    rng = np.random.default_rng(3)
    bases = lambda n: bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])
    quals = lambda n: bytes(rng.integers(35, 75, n).astype(np.uint8))

    def check_layout(io_, oo, end_short, end_long):
        assert io_[2] <= STEP < io_[3] and end_short < oo[1] < oo[2] < end_long      # step 1: members 0 and 1 = the short record, the long one's head
        assert io_[3] <= 2 * STEP < io_[4] and oo[3] < end_long                      # step 2: the carry and member 2, still inside the long record

    # BGZF FASTQ
    a = b"@a first\n%s\n+\n%s\n" % (bases(100), quals(100))
    b = b"@b long\n%s\n+\n%s\n" % (bases(6000), quals(6000))
    text = a + b + b"@c last\n%s\n+\n%s\n" % (bases(80), quals(80))
    z, io_, oo = stored(text, len(a) + 300, 3000)
    check_layout(io_, oo, len(a), len(a) + len(b))
    p = write(tmp_path / "carry.fq.gz", z)
    exp = read_all([write(tmp_path / "carry.fq", text)], 10 ** 9)
    assert exp[1] is None and [len(x[1]) for x in flat(exp[0])] == [100, 6000, 80]
    assert read_all([p], 10 ** 9) == exp
    assert read_all([p], 10 ** 9, ctx=ctx, chunk=STEP, check=lambda bt: _check_device_arrays(ctx, bt)) == exp
    # BAM
    recs = [dict(name=b"a", seq=bases(100), qual=quals(100), flag=4, aux=[("RG", "Z", "g")]), dict(name=b"b", seq=bases(6000), qual=quals(6000), flag=4, aux=[]),
            dict(name=b"c", seq=bases(80), qual=None, flag=4, aux=[("np", "C", 3)])]
    raw = bgzf.bam_bytes(recs)
    end_a, end_b = len(bgzf.bam_bytes(recs[:1])), len(bgzf.bam_bytes(recs[:2]))
    z, io_, oo = stored(raw, end_a + 300, 3000)
    check_layout(io_, oo, end_a, end_b)
    p = write(tmp_path / "carry.bam", z)
    dev = _same_dev_host(ctx, [p], 10 ** 9, STEP, passthrough=True)
    assert [len(x[1]) for bt in dev for x in bt] == [100, 6000, 80]
    # the genome: the step cuts a header line (the carry), and the member behind it is larger than a step: no whole member, read on
    wrap = lambda s: b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60))
    head = b">chr1 one\n" + wrap(bases(2800))
    data = head + b">chr2 the header line the step cuts\n" + wrap(bases(9000)) + b">chr3\nACGT\n"
    z, io_, oo = stored(data, len(head) + 12, 6000)
    assert io_[1] <= STEP < io_[2] and io_[2] - io_[1] > STEP and io_[2] > 2 * STEP
    same_in_both_forms(ctx, write(tmp_path / "carry.fa.gz", z), data, steps=(STEP,))


def exact_steps_fastq(n_bytes):
    """FASTQ text of exactly n_bytes: 100-base records, the last one stretched to fit"""
    rng = np.random.default_rng(8)
    out = b""
    while n_bytes - len(out) > 600:
        out += b"@r%d\n%s\n+\n%s\n" % (len(out), bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 100)]), b"5" * 100)
    left = n_bytes - len(out)
    name = b"@last" + b"x" * (left % 2)
    k = (left - len(name) - 5) // 2
    return out + name + b"\n" + b"A" * k + b"\n+\n" + b"5" * k + b"\n"


def exact_steps_genome():
    data = b">chr1\n" + b"ACGT" * 15 + b"\n"
    data += b">chr2 x\n" + (b"TTGCA" * 12 + b"\n") * 200
    data = data[:2 * STEP - 1] + b"\n"
    assert len(data) == 2 * STEP
    return data


def test_gzip_that_ends_at_a_step_end_host(tmp_path):
    """the inflated data is an exact multiple of the step (the host read form's step is 1 MiB, the genome's is its chunk): nothing is lost or repeated"""
    text = exact_steps_fastq(1 << 20)
    assert len(text) == 1 << 20
    exp = read_all([write(tmp_path / "exact.fq", text)], 10 ** 9)
    assert exp[1] is None and read_all([write(tmp_path / "exact.fq.gz", gzip.compress(text, 6))], 10 ** 9) == exp
    data = exact_steps_genome()
    names, pos, seq = gc.parse_rules(data)
    p = write(tmp_path / "exact.fa.gz", gzip.compress(data, 6))
    g = GenomeFile(p, chunk=STEP).read()
    assert (g.names, g.chrom_pos, g.padded.tobytes()) == (names, pos, seq + bytes(64))
    g.close()


@pytest.mark.gpu
def test_gzip_that_ends_at_a_step_end_device(ctx, tmp_path):
    text = exact_steps_fastq(3 * STEP)
    assert len(text) == 3 * STEP
    exp = read_all([write(tmp_path / "exact.fq", text)], 10 ** 9)
    p = write(tmp_path / "exact.fq.gz", gzip.compress(text, 6))
    assert exp[1] is None and read_all([p], 10 ** 9, ctx=ctx, chunk=STEP, check=lambda b: _check_device_arrays(ctx, b)) == exp
    data = exact_steps_genome()
    same_in_both_forms(ctx, write(tmp_path / "exact.fa.gz", gzip.compress(data, 6)), data, steps=(STEP,))
