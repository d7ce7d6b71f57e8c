"""lra_map_records_device_bam against lra_map_records_device's SAM text of the same lra_map_result: the record stream, decoded by tests/bam_text.py (struct,
numpy and zlib only), gives the SAM's lines.  The only normalisation on the expected side: a QUAL that is not as long as its SEQ becomes '*' (BAM's QUAL
has l_seq bytes or none)."""
import struct

import numpy as np
import pytest

import bam_text
from lra_amd import bgzf
import test_records_device as T

pytestmark = pytest.mark.gpu


def _norm(line):
    f = line.split(b"\t")
    if f[10] != b"*" and len(f[10]) != len(f[9]):
        f[10] = b"*"
        return b"\t".join(f), True
    return line, False


def _check(mapper, res, args, tags, refs, md=False, cg_form=False):
    """The raw stream against the SAM text -> (stream, [(read, flag) of every normalised record]).  rec_off is checked against the block_size chain."""
    n = args["n"]
    sam = mapper.records_device(res, args, passthrough=tags, md=md)
    raw, rec_off = mapper.records_device_bam(res, args, passthrough=tags, md=md)
    assert mapper.records_device_stats()["text_bytes"] == len(raw)
    recs = bam_text.records(raw, refs)
    starts = {at for at, _, _ in recs} | {len(raw)}
    assert int(rec_off[0]) == 0 and int(rec_off[-1]) == len(raw) and len(rec_off) == n + 1
    normalised = []
    for i in range(n):
        lines = sam[i].split(b"\n")[:-1]
        assert int(rec_off[i]) in starts, i                                   # every read's range starts at a record ...
        mine = [r for r in recs if int(rec_off[i]) <= r[0] < int(rec_off[i + 1])]
        assert len(mine) == len(lines), (i, len(mine), len(lines))            # ... and holds exactly its records
        for (at, bs, got), line in zip(mine, lines):
            exp, changed = _norm(line)
            if changed:
                normalised.append((i, int(exp.split(b"\t")[1])))
            if got != exp:
                g, e = got.split(b"\t"), exp.split(b"\t")
                k = next((x for x in range(min(len(g), len(e))) if g[x] != e[x]), min(len(g), len(e)))
                raise AssertionError("read %d, field %d of %d / %d: %r / %r" % (i, k, len(g), len(e), b"".join(g[k:k + 1])[:80], b"".join(e[k:k + 1])[:80]))
            ref_id, pos, _, _, bin_, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHIiii", raw, at + 4)
            assert (nref, npos) == (-1, -1)
            if flag & 4:
                assert (ref_id, pos, bin_, n_cig, tlen) == (-1, -1, 4680, 0, 0)
            else:
                assert bin_ == bam_text.reg2bin(pos, pos + tlen) and 0 <= ref_id < len(refs)
                assert (n_cig == 2 and b"CG:B:I" not in got) if cg_form else n_cig >= 1     # (the decoder restored the CIGAR and dropped the tag)
    return raw, normalised


def test_ont_batch(ctx):
    from lra_amd import seed, mapread
    from lra_amd._lib import LraError
    mapper, reads, rng = T._ont_setup(ctx)
    refs = [(b"chrA", 300_000), (b"chrB", 300_000)]
    n = len(reads)
    names = [b"read/%d" % i for i in range(n)]
    names[1] = b"n" * 254                                                     # the longest name a BAM record holds
    quals = T._quals(rng, reads)
    quals[2] = b"*"                                                           # an aligned read whose quality string is "*"
    quals[4] = None
    quals[0] = b"*" + quals[0][1:]                                            # an unaligned read's string goes out as it is
    short = list(quals)
    short[5] = quals[5][:100]                                                 # on purpose: a quality string shorter than its read
    short[n - 1] = quals[n - 1][:7]                                           # ... and an unaligned read's
    tags = [None if i % 3 == 0 else b"XA:i:%d\tXZ:Z:t%d\tXB:B:s,1,-2,300,%d" % (i * 1000, i, i) for i in range(n)]
    res = mapper.align(seed.ReadBatch(ctx, reads))
    args, args_short = mapper.record_args(names, reads, quals), mapper.record_args(names, reads, short)
    seen = dict(supp=0, rev=0, un=0, sa=0)
    for hard in (0, 1):
        for md in (False, True):
            T._set(mapper, printFormat="s", hardClip=hard, PrintNumAln=1)
            raw, normalised = _check(mapper, res, args, tags, refs, md=md)
            if hard == 0:
                assert normalised == []
                assert sorted({i for i, _ in _check(mapper, res, args_short, tags, refs, md=md)[1]}) == [5, n - 1]
            else:
                assert all(fl & 2048 for _, fl in normalised), normalised      # (supplementary records only: -H's two ranges)
            for _, _, line in bam_text.records(raw, refs):
                fl = int(line.split(b"\t")[1])
                seen["supp"] += bool(fl & 2048); seen["rev"] += bool(fl & 16); seen["un"] += bool(fl & 4); seen["sa"] += b"\tSA:Z:" in line
                assert (b"\tMD:Z:" in line) == (md and not fl & 4)
    assert seen["supp"] >= 3 and seen["rev"] >= 3 and seen["un"] >= 8 and seen["sa"] >= 4, seen
    # secondary records (PrintNumAln 2), no qualities at all, no passthrough
    T._set(mapper, hardClip=1, PrintNumAln=2)
    raw, _ = _check(mapper, res, args, tags, refs, md=True)
    assert any(int(l.split(b"\t")[1]) & 256 for _, _, l in bam_text.records(raw, refs))
    _check(mapper, res, mapper.record_args(names, reads, None), None, refs)
    T._set(mapper, hardClip=0, PrintNumAln=1)
    # BGZF: the members inflate to the raw stream, member_off is theirs, fewer bytes than the stream cross
    raw, _ = _check(mapper, res, args, tags, refs, md=True)
    data, rec_off, member_off = mapper.records_device_bam(res, args, passthrough=tags, md=True, bgzf=True)
    st = mapper.records_device_stats()
    assert bam_text.inflate(data) == raw and bgzf.blocks(data)[0] == [int(x) for x in member_off] and len(member_off) - 1 == (len(raw) + 65279) // 65280
    assert int(rec_off[-1]) == len(raw) == st["text_bytes"] and st["bytes_d2h"] < len(raw)
    # more CIGAR ops than the limit: <l_seq>S<ref length>N and a CG:B:I tag, for every aligned record
    try:
        for hard in (0, 1):
            T._set(mapper, hardClip=hard)
            mapread.set_bam_cigar_limit(ctx, 0)                                # the default
            plain, _ = _check(mapper, res, args, tags, refs, md=True)
            mapread.set_bam_cigar_limit(ctx, 100)
            cg, _ = _check(mapper, res, args, tags, refs, md=True, cg_form=True)
            aligned = sum(not int(l.split(b"\t")[1]) & 4 for _, _, l in bam_text.records(plain, refs))
            assert aligned >= 12 and len(cg) == len(plain) + 16 * aligned      # two placeholder ops; "CG", "B", "I" and the count
        with pytest.raises(LraError):
            mapread.set_bam_cigar_limit(ctx, 65536)
    finally:
        mapread.set_bam_cigar_limit(ctx, 65535)
    T._set(mapper, hardClip=0)
    # buffer reuse: a BAM call, a plain call and a BAM call on one context; then a smaller batch
    a = mapper.records_device_bam(res, args, passthrough=tags, md=True)[0]
    mapper.records_device(res, args, passthrough=tags)
    b = mapper.records_device_bam(res, args, passthrough=tags, md=True)[0]
    assert a == b == raw
    # the SV signature text is the plain call's
    _, sigs = mapper.records_device(res, args, passthrough=tags, svsig=True)
    r = mapper.records_device_bam(res, args, passthrough=tags, md=True, svsig=True)
    assert r[0] == raw and r[2] == sigs
    r = mapper.records_device_bam(res, args, passthrough=tags, md=True, svsig=True, bgzf=True)
    assert bam_text.inflate(r[0]) == raw and r[3] == sigs
    # what has no BAM form
    for bad_names, bad_tags, fmt, what in ((names[:7] + [b"m" * 255] + names[8:], tags, "s", "read 7"), (names, tags[:4] + [b"XA:i:12x"] + tags[5:], "s", "read 4"),
                                           (names, tags, "P", "format")):
        T._set(mapper, printFormat=fmt)
        with pytest.raises(LraError, match=what):
            mapper.records_device_bam(res, mapper.record_args(bad_names, reads, quals), passthrough=bad_tags)
    T._set(mapper, printFormat="s")
    for sub in ([6, 1, 11], [7]):
        r2 = [reads[i] for i in sub]
        res2 = mapper.align(seed.ReadBatch(ctx, r2))
        _check(mapper, res2, mapper.record_args([names[i] for i in sub], r2, [quals[i] for i in sub]), [tags[i] for i in sub], refs, md=True)


def test_stream_from_a_device_readers_arrays(ctx, tmp_path):
    """DEV_QUAL | DEV_NO_HOST: the host sees a quality string's first byte only; the stream equals the one from uploaded qualities."""
    from lra_amd import reads_io
    from test_device_quals import _fastq, _reader_batch
    mapper, reads, rng = T._ont_setup(ctx)
    n = len(reads)
    names = [b"read/%d" % i for i in range(n)]
    quals = T._quals(rng, reads)
    quals[0] = None                                                           # read 0 comes from a FASTA file: no qualities
    quals[n - 1] = b"*" + quals[n - 1][1:]
    (tmp_path / "first.fa").write_bytes(b">%s\n%s\n" % (names[0], reads[0]))
    (tmp_path / "rest.fq").write_bytes(_fastq([(names[i], reads[i], quals[i]) for i in range(1, n)]))
    tags = [None if i % 3 == 0 else b"XA:i:%d" % i for i in range(n)]
    rf, b = _reader_batch(ctx, [tmp_path / "first.fa", tmp_path / "rest.fq"])
    try:
        assert b["seqs"] is None and b["quals"] == [None if q is None else q[:1] for q in quals]
        res = reads_io.map_reads_device(mapper, b)
        for hard in (0, 1):
            T._set(mapper, printFormat="s", hardClip=hard, PrintNumAln=1)
            up, _ = _check(mapper, res, mapper.record_args(names, reads, quals), tags, [(b"chrA", 300_000), (b"chrB", 300_000)], md=True)
            h2d_up = mapper.records_device_stats()["bytes_h2d"]
            rd, rec_off = mapper.records_device_bam(res, mapper.record_args(names, None, b["quals"], lens=b["read_len"]), passthrough=tags, md=True,
                                                    d_qual=b["d_qual"], d_qual_off=b["d_qual_off"])
            assert rd == up and mapper.records_device_stats()["bytes_h2d"] < h2d_up        # no quality byte goes up
    finally:
        rf.close()


def test_a_batch_cut_over_several_host_threads(ctx):
    """64 reads and more: the host half cuts the batch into ranges of reads, one per thread, and joins their piece tables -- the indices of the SEQ ranges,
    the QUAL requests and the records' first pieces move with their range."""
    from lra_amd import seed
    mapper, reads, rng = T._ont_setup(ctx)
    pieces = [r[a:a + 1200] for r in reads for a in range(0, len(r) - 1199, 1200)]
    n = len(pieces)
    assert n >= 64
    names = [b"piece%d" % i for i in range(n)]
    quals = T._quals(rng, pieces)
    quals[40] = None
    tags = [None if i % 5 == 0 else b"XA:i:%d" % -i for i in range(n)]
    res = mapper.align(seed.ReadBatch(ctx, pieces))
    args = mapper.record_args(names, pieces, quals)
    for hard in (0, 1):
        T._set(mapper, printFormat="s", hardClip=hard, PrintNumAln=1)
        raw, _ = _check(mapper, res, args, tags, [(b"chrA", 300_000), (b"chrB", 300_000)], md=True)
        data, rec_off, member_off = mapper.records_device_bam(res, args, passthrough=tags, md=True, bgzf=True)
        assert bam_text.inflate(data) == raw and int(rec_off[-1]) == len(raw)
    assert sum(not int(l.split(b"\t")[1]) & 4 for _, _, l in bam_text.records(raw, [(b"chrA", 300_000), (b"chrB", 300_000)])) >= n // 2


def test_ccs_batch_through_the_high_accuracy_driver(ctx):
    from lra_amd import seed, mapread
    import test_highacc_path as H
    g = H._genome_with_repeats(19)
    rng = np.random.default_rng(8)
    reads = [r.tobytes() for r in H._sv_reads(g, rng, 0.01, n_plain=4)]
    mapper = mapread.HighAccMapper(ctx, g, None, None, [b"chrA", b"chrB"], [0, 250_000, len(g)], "ccs", index_params=(17, 10, 150, 15, 1))
    refs = [(b"chrA", 250_000), (b"chrB", len(g) - 250_000)]
    names = [b"ccs%d" % i for i in range(len(reads))]
    args = mapper.record_args(names, reads, T._quals(rng, reads))
    res = mapper.align(seed.ReadBatch(ctx, reads))
    for hard, md in ((0, False), (1, True)):
        T._set(mapper, printFormat="s", hardClip=hard)
        raw, normalised = _check(mapper, res, args, None, refs, md=md)
        assert raw and all(fl & 2048 for _, fl in normalised) and (hard or not normalised)
        data, _, member_off = mapper.records_device_bam(res, args, md=md, bgzf=True)
        assert bam_text.inflate(data) == raw and bgzf.blocks(data)[0] == [int(x) for x in member_off]
    assert bam_text.parse_header(mapper.bam_header())[1] == refs
