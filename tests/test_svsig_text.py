"""lra_svsig_text_batch (svsig_text.hip): the lines of a batch's SV signatures built on the device, against a restatement of the line format on crafted
batches run through lra_sv_signatures_batch at min_len 0 (GPU)."""
import ctypes as C

import numpy as np
import pytest

INS, DEL = 0, 1
ALPHA = np.frombuffer(b"ACGTacgtN", np.uint8)
READ_NAMES = [b"r", b"n" * 15, b"read/sixteen/16x", b"seventeen-bytes-x", b"L" * 255]      # 1, 15, 16, 17 and 255 bytes
CHROM_NAMES = [b"c", b"chromosome_with_a_30_byte_name"]                                    # 1 and 30 bytes
# t_start: one value on each side of every decimal width up to what an int32 block coordinate holds
T_STARTS = [0, 9, 10, 99, 100, 999, 1000, 9999, 10_000, 99_999, 100_000, 999_999, 10 ** 6, 9_999_999, 10 ** 7, 99_999_999, 10 ** 8, 999_999_999, 10 ** 9,
            2_147_483_000]
LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 100, 999, 1000, 4095, 4096, 4097, 9999, 10_000, 50_000]   # every width from 1 to 5 digits, the wave, the chunk, one long
DEL_CROSS = [(9, 2), (95, 10), (999_990, 20)]                            # the DEL's end crosses a decimal width its start does not
TEXT_LEN = 1_000_100


def format_lines(off, recs, seq, aln_read, chrom, skip, read_names, chrom_names):
    """The line format restated -> (text, aln_off)"""
    out, aln_off = [], [0]
    for a in range(len(off) - 1):
        n_bytes = 0
        for r in recs[int(off[a]):int(off[a + 1])] if not (skip is not None and skip[a]) else []:
            t, n, k, so = int(r["t_start"]), int(r["len"]), int(r["kind"]), int(r["seq_off"])
            end = (t + n - 1) & 0xffffffff if k == DEL else t
            out.append(b"%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (chrom_names[chrom[a]], read_names[aln_read[a]], t, end, n, b"DEL" if k == DEL else b"INS", seq[so:so + n]))
            n_bytes += len(out[-1])
        aln_off.append(aln_off[-1] + n_bytes)
    return b"".join(out), np.array(aln_off, np.uint64)


class Batch:
    """Alignments over one shared text (every t_off is 0: an INS reaches only into its read, so t_start may lie far outside the text)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.reads, self.blocks, self.tags = [], [], {}

    def add(self, tag, blocks, read_len):
        self.tags.setdefault(tag, []).append(len(self.blocks))
        self.blocks.append(np.asarray(blocks, np.int32).reshape(-1, 3))
        self.reads.append(ALPHA[self.rng.integers(0, len(ALPHA), read_len)].tobytes())

    def ins(self, tag, t, n):
        """one INS {t, t, n}: a block that ends at t (of length 0 at t = 0), n read bases, a block of 3"""
        first = [0, t - 1, 1] if t else [0, 0, 0]
        q = first[0] + first[2]
        self.add(tag, [first, [q + n, t, 3]], q + n + 3)

    def dele(self, tag, t, n):
        first = [0, t - 1, 1] if t else [0, 0, 0]
        q = first[0] + first[2]
        self.add(tag, [first, [q, t + n, 3]], q + 3)

    def chain(self, tag, sigs, step=7):
        """many blocks: the signatures (kind, n) in a row, blocks of `step` between them"""
        q = t = 3
        bl = []
        for kind, n in sigs:
            bl.append([q, t, step])
            q += step + (n if kind == INS else 0); t += step + (n if kind == DEL else 0)
        bl.append([q, t, step])
        assert t + step < TEXT_LEN
        self.add(tag, bl, q + step + 2)

    def run(self, ctx, min_len=0):
        import torch
        from lra_amd import refine
        n = len(self.blocks)
        q_off = np.zeros(n + 1, np.int64); q_off[1:] = np.cumsum([len(r) for r in self.reads])
        boff = np.zeros(n + 1, np.int64); boff[1:] = np.cumsum([len(b) for b in self.blocks])
        dev = lambda a, dt: torch.from_numpy(np.array(a, dt)).to(ctx.device)
        qseq = dev(np.frombuffer(b"".join(self.reads) + b"\0" * 64, np.uint8), np.uint8)
        text = ALPHA[np.random.default_rng(5).integers(0, len(ALPHA), TEXT_LEN)]
        tseq = dev(np.concatenate([text, np.zeros(64, np.uint8)]), np.uint8)
        bl = np.concatenate(self.blocks) if n else np.zeros((0, 3), np.int32)
        rb = refine.refine_batch_from_device(ctx, dev(bl, np.int32).view(-1, 3), dev(boff, np.int64), qseq, dev(q_off[:-1], np.int64),
                                             dev([len(r) for r in self.reads], np.int32), tseq, dev(np.zeros(n, np.int64), np.int64),
                                             dev(np.full(n, TEXT_LEN, np.int64), np.int64))
        self.keep = (rb, qseq, tseq)
        sv = refine.SvSigResult()
        ctx.check(ctx.lib.lra_sv_signatures_batch(ctx.h, rb.n, refine.ptr(rb.blocks), refine.ptr(rb.block_off), refine.ptr(rb.q_seq), refine.ptr(rb.q_off), refine.ptr(rb.q_len),
                                                  refine.ptr(rb.t_seq), refine.ptr(rb.t_off), C.c_int32(min_len), C.byref(sv)))
        ns, nb = int(sv.n_sig), int(sv.n_seq_bytes)
        off = ctx.to_host(sv.d_sig_off, n + 1, np.uint64)
        recs = ctx.to_host(sv.d_sig, ns * refine.SVSIG_REC.itemsize, np.uint8).view(refine.SVSIG_REC) if ns else np.zeros(0, refine.SVSIG_REC)
        seq = ctx.to_host(sv.d_seq, nb, np.uint8).tobytes() if nb else b""
        return sv, off, recs, seq


def check(ctx, batch, skip=None, min_len=0):
    """The primitive against the restatement: text, byte count (the text's length), aln_off -> (off, recs, text, aln_off)"""
    from lra_amd import refine
    sv, off, recs, seq = batch.run(ctx, min_len)
    n = len(batch.blocks)
    aln_read = np.arange(n) % len(READ_NAMES); chrom = np.arange(n) % len(CHROM_NAMES)
    text, aln_off = refine.svsig_text_batch(ctx, sv, aln_read, chrom, READ_NAMES, CHROM_NAMES, skip=skip)
    want, want_off = format_lines(off, recs, seq, aln_read, chrom, skip, READ_NAMES, CHROM_NAMES)
    assert len(text) == len(want) and np.array_equal(aln_off, want_off)
    if text != want:
        at = next(k for k in range(len(want)) if text[k] != want[k])
        raise AssertionError("first difference at byte %d of %d: %r / %r" % (at, len(want), text[max(at - 30, 0):at + 30], want[max(at - 30, 0):at + 30]))
    return off, recs, text, aln_off


def crafted():
    b = Batch(11)
    b.add("none", np.zeros((0, 3)), 4)                                    # alignments without a signature first and adjacent: 0 blocks, 1 block, 1 block
    b.add("none", [[0, 5, 4]], 6)
    b.add("none", [[1, 7, 3]], 5)
    for i, t in enumerate(T_STARTS):
        b.ins("ins", t, LENGTHS[i % len(LENGTHS)])
    b.add("none", [[2, 2, 2]], 5)
    for t, n in DEL_CROSS:
        b.dele("cross", t, n)
    rng = np.random.default_rng(2)
    sigs = [(INS, n) for n in LENGTHS] + [(DEL, n) for n in LENGTHS] + [(int(k), int(n)) for k, n in zip(rng.integers(0, 2, 60), rng.integers(1, 40, 60))]
    b.chain("many", [sigs[i] for i in rng.permutation(len(sigs))])
    b.chain("skipped", [(INS, 3), (DEL, 70), (INS, 4097), (DEL, 2)])      # a skipped alignment that has signatures
    b.chain("many", [(DEL, 33), (INS, 1)], step=1)
    b.add("none", [[0, 0, 9]], 10)                                        # ... and last
    b.add("none", np.zeros((0, 3)), 1)
    return b


def small():
    b = Batch(12)
    b.add("none", [[0, 5, 4]], 6)
    b.ins("ins", 12_345, 7)
    b.dele("cross", 99, 2)
    return b


@pytest.mark.gpu
def test_crafted_batch_then_a_small_one_on_the_same_context(ctx):
    from lra_amd.refine import SVSIG_TEXT_CHUNK
    b = crafted()
    skip = np.zeros(len(b.blocks), np.uint8)
    skip[b.tags["skipped"]] = 1
    off, recs, text, aln_off = check(ctx, b, skip)
    n_of = lambda tag: [int(off[a + 1] - off[a]) for a in b.tags[tag]]
    assert n_of("none") == [0] * 6 and n_of("ins") == [1] * len(T_STARTS) and n_of("cross") == [1] * 3 and n_of("skipped") == [4] and n_of("many")[0] >= 90
    assert b.tags["none"][:3] == [0, 1, 2] and b.tags["none"][-1] == len(b.blocks) - 1
    a = b.tags["skipped"][0]
    assert aln_off[a] == aln_off[a + 1] and aln_off[a] > 0 and aln_off[-1] > aln_off[a]
    # the numbers: every t_start asked for, the three DELs whose end is a digit wider than their start, every width of len
    ins = recs[recs["kind"] == INS]; dele = recs[recs["kind"] == DEL]
    assert set(T_STARTS) <= set(ins["t_start"].tolist())
    assert set(DEL_CROSS) <= set(zip(dele["t_start"].tolist(), dele["len"].tolist()))
    for t, n in DEL_CROSS:
        assert len(str(t + n - 1)) == len(str(t)) + 1
        assert b"\t%d\t%d\t%d\tDEL\t" % (t, t + n - 1, n) in text
    assert {len(str(n)) for n in recs["len"].tolist()} == {1, 2, 3, 4, 5}
    for kind in (INS, DEL):
        assert set(LENGTHS) <= set(recs["len"][recs["kind"] == kind].tolist())
    assert {1, 2, 3, 4, 5, 63, 64, 65, SVSIG_TEXT_CHUNK - 1, SVSIG_TEXT_CHUNK, SVSIG_TEXT_CHUNK + 1, 50_000} <= set(LENGTHS)
    # where the copy pass reads and writes: the bases of a line end in front of its newline
    src, dst = [], []
    lines = text.split(b"\n")[:-1]
    live = [r for a in range(len(b.blocks)) if not skip[a] for r in recs[int(off[a]):int(off[a + 1])]]
    assert len(lines) == len(live)
    at = 0
    for line, r in zip(lines, live):
        at += len(line) + 1
        src.append(int(r["seq_off"])); dst.append(at - 1 - int(r["len"]))
    assert {(s % 4, d % 4) for s, d in zip(src, dst)} == {(i, j) for i in range(4) for j in range(4)}      # all 16 misalignments of the dword copy
    assert {s % 16 for s in src} == set(range(16)) == {d % 16 for d in dst}
    # buffer reuse: a small batch behind the large one
    off2, recs2, text2, _ = check(ctx, small())
    assert len(recs2) == 2 and text2.count(b"\n") == 2 and len(text2) < 200 < len(text)


@pytest.mark.gpu
def test_counts(ctx):
    from lra_amd import refine
    # 4097 alignments of one or two 1-base signatures each: more alignments than a chunk has bytes, lines of ~20 bytes
    b = Batch(13)
    for i in range(4097):
        bl = [[0, 0, 2], [3, 2, 2]] + ([[5, 5, 2]] if i % 3 else [])          # INS 1 (, DEL 1)
        b.add("tiny", bl, 8)
    skip = (np.arange(4097) % 11 == 5).astype(np.uint8)
    off, recs, text, aln_off = check(ctx, b, skip)
    assert set(np.diff(off.astype(np.int64)).tolist()) == {1, 2} and set(recs["len"].tolist()) == {1} and set(recs["kind"].tolist()) == {INS, DEL}
    check(ctx, b)                                                         # no skip bytes: none is skipped
    # n_sig = 0 with n_aln > 0; n_aln = 0
    off, recs, text, aln_off = check(ctx, b, min_len=10 ** 6)
    assert len(recs) == 0 and text == b"" and len(aln_off) == 4098 and not aln_off.any()
    sv = refine.SvSigResult()
    ctx.check(ctx.lib.lra_sv_signatures_batch(ctx.h, 0, None, None, None, None, None, None, None, C.c_int32(0), C.byref(sv)))
    text, aln_off = refine.svsig_text_batch(ctx, sv, [], [], READ_NAMES, CHROM_NAMES)
    assert text == b"" and aln_off.tolist() == [0]


@pytest.mark.gpu
def test_bad_arguments(ctx):
    from lra_amd import refine
    from lra_amd.refine import ptr
    lib = ctx.lib
    b = small()
    sv, off, recs, seq = b.run(ctx)
    assert int(sv.n_sig) == 2
    n = len(b.blocks)
    import torch
    d_read = torch.zeros(n, dtype=torch.int32, device=ctx.device); d_chrom = torch.zeros(n, dtype=torch.int32, device=ctx.device)
    rn, ro = refine.name_table(ctx, READ_NAMES); cn, co = refine.name_table(ctx, CHROM_NAMES)
    out = refine.SvSigTextResult()
    call = lambda sv_, rn_, ro_, nr, cn_, co_, nc: lib.lra_svsig_text_batch(ctx.h, sv_, ptr(d_read), ptr(d_chrom), None, nr, rn_, ro_, nc, cn_, co_, C.byref(out))
    assert call(C.byref(sv), ptr(rn), ptr(ro), 5, ptr(cn), ptr(co), 2) == 0 and int(out.n_bytes) > 0
    assert call(None, ptr(rn), ptr(ro), 5, ptr(cn), ptr(co), 2) == -1                         # LRA_ERR_INVALID
    assert call(C.byref(sv), None, None, 5, ptr(cn), ptr(co), 2) == -1
    assert call(C.byref(sv), ptr(rn), ptr(ro), 5, None, None, 2) == -1
    assert call(C.byref(sv), ptr(rn), ptr(ro), -1, ptr(cn), ptr(co), 2) == -1
    assert call(C.byref(sv), ptr(rn), ptr(ro), 5, ptr(cn), ptr(co), -2) == -1
    neg = refine.SvSigResult(); neg.n_aln = -1
    assert call(C.byref(neg), ptr(rn), ptr(ro), 5, ptr(cn), ptr(co), 2) == -1
    assert lib.lra_svsig_text_batch(ctx.h, C.byref(sv), ptr(d_read), ptr(d_chrom), None, 5, ptr(rn), ptr(ro), 2, ptr(cn), ptr(co), None) == -1
    # NULL name tables are fine where there is nothing to print
    empty = refine.SvSigResult(); empty.n_aln = 3
    assert call(C.byref(empty), None, None, 0, None, None, 0) == 0 and int(out.n_bytes) == 0
    assert ctx.to_host(out.d_aln_off, 4, np.uint64).tolist() == [0, 0, 0, 0]
