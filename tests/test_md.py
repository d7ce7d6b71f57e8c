"""MD:Z (lra --printMD) on the device: lra_md_strings_batch against the reference's AlignmentStringsToMD (the goldens' M lines) and against the host
yardstick lra_md_string(lra_alignment_strings(...)) on random batches; the record stage with LRA_PACK_MD for every driver form (GPU)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from lra_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
MD_TAG = re.compile(rb"\tMD:Z:[^\t\n]*")


def host_md(lib, read: bytes, text: bytes, blocks):
    """lra_md_string(lra_alignment_strings(...)): the host restatement pinned to the reference (tests/test_order.py)."""
    b = np.ascontiguousarray(np.asarray(blocks, np.int32).reshape(-1))
    nb = len(b) // 3
    bp = b.ctypes.data_as(C.c_void_p) if nb else None
    n = C.c_uint64(0); rl = C.c_uint32(0)
    lib.lra_alignment_strings(read, text, bp, nb, None, None, None, C.c_uint64(0), C.byref(n), C.byref(rl))   # (the sizing call)
    qb = C.create_string_buffer(n.value + 1); ab = C.create_string_buffer(n.value + 1); tb = C.create_string_buffer(n.value + 1)
    assert lib.lra_alignment_strings(read, text, bp, nb, qb, ab, tb, n, C.byref(n), C.byref(rl)) == 0
    m = C.c_uint64(0)
    lib.lra_md_string(qb.raw[:n.value], tb.raw[:n.value], n, None, C.c_uint64(0), C.byref(m))
    mb = C.create_string_buffer(m.value + 1)
    assert lib.lra_md_string(qb.raw[:n.value], tb.raw[:n.value], n, mb, m, C.byref(m)) == 0
    return mb.raw[:m.value]


def device_md(ctx, cases):
    """cases: (read bytes, text bytes, blocks [nb, 3]) -> lra_md_strings_batch over all of them in ONE batch."""
    import torch
    from lra_amd import refine
    q_off, t_off, qs, ts, boff, bl = [], [], [], [], [0], []
    qa = ta = 0
    for r, t, b in cases:
        q_off.append(qa); t_off.append(ta); qs.append(r); ts.append(t); qa += len(r); ta += len(t)
        b = np.asarray(b, np.int32).reshape(-1, 3)
        bl.append(b); boff.append(boff[-1] + len(b))
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(ctx.device)
    qseq = dev(np.frombuffer(b"".join(qs) + b"\0" * 64, np.uint8), np.uint8)
    tseq = dev(np.frombuffer(b"".join(ts) + b"\0" * 64, np.uint8), np.uint8)
    blocks = np.concatenate(bl) if sum(len(x) for x in bl) else np.zeros((0, 3), np.int32)
    rb = refine.refine_batch_from_device(ctx, dev(blocks, np.int32).view(-1, 3), dev(boff, np.int64), qseq, dev(q_off, np.int64),
                                         dev([len(r) for r, _, _ in cases], np.int32), tseq, dev(t_off, np.int64), dev([len(t) for _, t, _ in cases], np.int64))
    return refine.md_strings_batch(ctx, rb)


@pytest.mark.gpu
def test_md_kernel_matches_reference_goldens(ctx):
    gold = json.load(open(os.path.join(HERE, "golden", "aln_strings_golden.json")))["cases"]
    want = [re.search(r"^M (.*)$", k["expected"], re.M).group(1).encode() for k in gold]
    got = device_md(ctx, [(k["read"].encode(), k["text"].encode(), k["blocks"]) for k in gold])
    assert len(got) == len(gold) >= 150
    assert got == want
    assert sum(b"^" in m for m in got) >= 30


ALPHA = np.frombuffer(b"ACGTACGTACGTacgtNnRYKM", np.uint8)


def _random_case(rng, kind):
    """One alignment: blocks over a random read / text pair that shares most bases (so there are runs of matches), with the shapes the issue names."""
    if kind == "empty":
        return b"ACGT", b"ACGT", np.zeros((0, 3), np.int32)
    if kind == "zero":                                                     # only zero-length blocks, no gaps between them: no columns
        return b"ACGT", b"ACGT", np.array([[1, 1, 0], [1, 1, 0]], np.int32)
    if kind == "huge":
        nb, mean = 120_000, 18
    elif kind == "long":
        nb, mean = int(rng.integers(200, 3000)), 12
    else:
        nb, mean = int(rng.integers(1, 40)), 8
    lens = rng.integers(0, 2 * mean, nb)
    if kind in ("allmatch",):
        lens = np.array([int(rng.integers(1, 500))]); nb = 1
    qg = np.where(rng.random(nb) < 0.3, rng.integers(0, 6, nb), 0); qg[-1] = 0
    tg = np.where(rng.random(nb) < 0.3, rng.integers(0, 6, nb), 0); tg[-1] = 0
    if kind == "gapfirst":                                                 # a zero-length first block: the alignment starts with an insertion / deletion
        lens[0] = 0; qg[0] = 3 if nb > 1 else 0; tg[0] = 0
    q0, t0 = int(rng.integers(0, 5)), int(rng.integers(0, 5))
    q = np.concatenate([[q0], q0 + np.cumsum(lens + qg)[:-1]]).astype(np.int64)
    t = np.concatenate([[t0], t0 + np.cumsum(lens + tg)[:-1]]).astype(np.int64)
    qlen, tlen = int(q[-1] + lens[-1] + 5), int(t[-1] + lens[-1] + 5)
    text = ALPHA[rng.integers(0, len(ALPHA), tlen)].copy()
    read = ALPHA[rng.integers(0, 12, qlen)].copy()
    # aligned columns copy the text's base (upper-cased mostly) with ~6 % substitutions, some N / R on the read against an A
    for b in range(nb):
        L = int(lens[b])
        if L:
            src = text[t[b]:t[b] + L].copy()
            up = np.where((src >= 97) & (src <= 122), src - 32, src)
            src = np.where(rng.random(L) < 0.5, up, src).astype(np.uint8)
            sub = rng.random(L) < 0.06
            src[sub] = ALPHA[rng.integers(0, len(ALPHA), int(sub.sum()))]
            if rng.random() < 0.2:
                src[int(rng.integers(0, L))] = ord("N" if rng.random() < 0.5 else "R")
            read[q[b]:q[b] + L] = src
    if kind == "allmatch":
        read[q[0]:q[0] + lens[0]] = text[t[0]:t[0] + lens[0]]
    if kind == "mmend" and lens[-1] > 0:                                  # ends on a mismatch
        read[q[-1] + lens[-1] - 1] = ord("A") if text[t[-1] + lens[-1] - 1] not in b"Aa" else ord("C")
    if kind == "mmstart" and lens[0] > 0:
        read[q[0]] = ord("G") if text[t[0]] not in b"Gg" else ord("T")
    blocks = np.stack([q, t, lens], 1).astype(np.int32)
    return read.tobytes(), text.tobytes(), blocks


@pytest.mark.gpu
def test_md_kernel_random_batches_match_host(ctx):
    rng = np.random.default_rng(2024)
    lib = ctx.lib
    kinds = ["small"] * 1700 + ["long"] * 120 + ["gapfirst"] * 60 + ["allmatch"] * 40 + ["mmend"] * 40 + ["mmstart"] * 40 + ["empty", "zero", "huge"]
    rng.shuffle(kinds)
    cases = [_random_case(rng, k) for k in kinds]
    big = [i for i, k in enumerate(kinds) if k == "huge"][0]
    assert len(cases[big][2]) > 100_000 and int(cases[big][2][-1, 1]) > 2_000_000
    got = device_md(ctx, cases)
    want = [host_md(lib, r, t, b) for r, t, b in cases]
    bad = [i for i in range(len(cases)) if got[i] != want[i]]
    assert not bad, (len(bad), kinds[bad[0]], got[bad[0]][:200], want[bad[0]][:200])
    assert got[kinds.index("empty")] == b"" and got[kinds.index("zero")] == b""
    assert any(m[:1] == b"0" for m in got) and any(b"^" in m for m in got)
    # the reference's own AlignmentStringsToMD on a sample (oracle/_ref/aln_strings_ref, when it is built)
    exe = O.ref_bin("aln_strings_ref")
    if exe:
        sample = [i for i in range(len(cases)) if kinds[i] in ("small", "gapfirst", "mmend", "mmstart", "allmatch")][:300]
        lines = [" ".join(["r%d" % i, "chr", cases[i][0].decode(), cases[i][1].decode(), str(len(cases[i][2]))] + [str(int(v)) for v in cases[i][2].reshape(-1)])
                 for i in sample]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=120).stdout
        chunks = out.split("@@END\n")[:-1]
        assert len(chunks) == len(sample)
        for i, ch in zip(sample, chunks):
            assert re.search(r"^M (.*)$", ch, re.M).group(1).encode() == got[i], i


# ---------------------------------------------------------------------------------------------------------------- the record stage
def _expected_md(mapper, d, reads, genome, r, line):
    """The host MD of the alignment a SAM line of read r prints (matched by chromosome, POS and strand), from the result's final blocks."""
    from lra_amd import mapread
    f = line.split(b"\t")
    flag, chrom, pos = int(f[1]), f[2], int(f[3])
    na = max(int(d["num_aln"]), 1)
    jo = d["job_aln_off"]
    for a in range(int(jo[r * na]), int(jo[(r + 1) * na])):
        ci = int(d["chrom"][a])
        if mapper.chrom_names[ci] != chrom or int(d["counts"][a][16]) + 1 != pos or int(d["strand"][a]) != (1 if flag & 16 else 0):
            continue
        rd = reads[r] if not d["strand"][a] else mapread.create_rc(reads[r])
        b = d["blocks"][int(d["block_off"][a]):int(d["block_off"][a + 1])]
        text = bytes(genome[mapper.chrom_pos[ci]:mapper.chrom_pos[ci + 1]])
        return host_md(mapper.ctx.lib, rd, text, b)
    raise AssertionError("no alignment for %r" % line[:80])


def _check_sam_with_md(mapper, res, reads, genome, names, plain, withmd):
    d = mapper.fetch(res)
    d["num_aln"] = int(res.num_aln)
    n_md = 0
    for r, (p, m) in enumerate(zip(plain, withmd)):
        assert MD_TAG.sub(b"", m) == p, r                                    # no other byte changes
        for pl, ml in zip(p.split(b"\n"), m.split(b"\n")):
            tags = MD_TAG.findall(ml)
            f = pl.split(b"\t")
            if len(f) < 3 or f[2] == b"*":
                assert not tags                                              # the unaligned record (SimplePrintSAM): no MD
                continue
            assert len(tags) == 1
            li = ml.index(b"\tLI:i:")
            assert ml.index(b"\tMD:Z:") == ml.index(b"\t", li + 1)           # right after LI:i, before SA:Z
            assert tags[0][6:] == _expected_md(mapper, d, reads, genome, r, pl)
            n_md += 1
    return n_md


def _fmt(mapper, fmt):
    mapper.opts.printFormat = fmt
    mapper.copts = mapper._c_opts()


def _lowacc_setup(ctx, opts, n=40, mean=6000, seed=5):
    from lra_amd import mapread
    genome = synth.make_genome(800_000, seed=77, repeat_frac=0.2, n_families=3)
    CH = [0, 350_000, 800_000]
    ik, ip = synth.build_global_index(genome, opts.globalK, opts.globalW, 100 if opts.read_type == "ont" else opts.globalMaxFreq)
    reads, truth = synth.simulate_reads(genome, n, mean, 1500, 0.10, seed=seed)
    rng = np.random.default_rng(9)
    a = synth.simulate_read(rng, genome[100_000:105_001], 4500, 0.08, (30, 35, 35), False)[0]
    b = synth.simulate_read(rng, genome[600_000:605_001], 4500, 0.08, (30, 35, 35), False)[0]
    reads.append(np.concatenate([a, b]))
    mapper = mapread.LowAccMapper(ctx, genome, ik, ip, [b"chrA", b"chrB"], CH, opts)
    return mapper, genome, [r.tobytes() for r in reads]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["ont", "ont-bp", "clr-two-stage"])
def test_lowacc_sam_with_md(ctx, form):
    from lra_amd import mapread, seed, parallel
    opts = mapread.clr_options() if form.startswith("clr") else mapread.LowAccOptions(refineBreakpoint=form.endswith("bp"))
    mapper, genome, reads = _lowacc_setup(ctx, opts)
    names = [b"read%d" % i for i in range(len(reads))]
    batch = seed.ReadBatch(ctx, reads)
    if form == "clr-two-stage":
        mapper.front(batch)
        res, bctx = mapper.back()
        m = mapper.on(bctx)
    else:
        res = mapper.align(batch)
        m = mapper
    try:
        rargs = m.record_args(names, reads)
        plain = m.records_host(m.snapshot(res, md=False), rargs)
        withmd = m.records_host(m.snapshot(res, md=True), rargs)
        assert plain != withmd
        assert _check_sam_with_md(m, res, reads, genome, [b"chrA", b"chrB"], plain, withmd) > len(reads) // 2
        # the one-call form of the records switches to the snapshot with printMD
        if form != "clr-two-stage":
            m.opts.printMD = True
            assert m.records(res, names, reads) == withmd
            m.opts.printMD = False
            assert m.records(res, names, reads) == plain
        # pack round trip: a pack with MD through lra_map_unpack_host / records_from_packed gives the snapshot's text; without, today's
        assert parallel.records_from_packed(ctx.lib, m.copts, parallel.pack_records(m.ctx, res, print_md=True), names, reads, m.chrom_names) == withmd
        assert parallel.records_from_packed(ctx.lib, m.copts, parallel.pack_records(m.ctx, res), names, reads, m.chrom_names) == plain
        # PAF and BED: no MD, identical text with and without the flag
        for fmt in "pb":
            _fmt(m, fmt)
            assert m.records_host(m.snapshot(res, md=True), rargs) == m.records_host(m.snapshot(res, md=False), rargs)
        _fmt(m, "s")
    finally:
        if form == "clr-two-stage":
            mapper.release()


@pytest.mark.gpu
def test_staged_records_with_md_equal_the_one_call(ctx):
    from lra_amd import mapread, seed
    opts = mapread.LowAccOptions(printMD=True)
    mapper, genome, reads = _lowacc_setup(ctx, opts, n=16)
    names = [b"read%d" % i for i in range(len(reads))]
    batch = seed.ReadBatch(ctx, reads)
    staged = mapper.records_staged(mapper.align_staged(batch), names, reads)
    res = mapper.align(batch)
    assert mapper.records(res, names, reads) == staged
    assert sum(len(MD_TAG.findall(t)) for t in staged) > 8


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["ccs", "contig"])
def test_highacc_sam_with_md(ctx, preset):
    from lra_amd import mapread, seed, parallel
    g = synth.make_genome(1_200_000, seed=31, repeat_frac=0.05, n_families=3)
    CH = [0, 500_000, len(g)]
    if preset == "ccs":
        reads, _ = synth.simulate_reads(g, 40, 8000, 1500, 0.01, (34, 33, 33), seed=12)
    else:
        reads, _ = synth.simulate_reads(g, 6, 150_000, 20_000, 0.002, (34, 33, 33), seed=12)
    reads = [r.tobytes() for r in reads]
    mapper = mapread.HighAccMapper(ctx, g, None, None, [b"chrA", b"chrB"], CH, preset, printMD=True)
    names = [b"read%d" % i for i in range(len(reads))]
    res = mapper.align(seed.ReadBatch(ctx, reads))
    rargs = mapper.record_args(names, reads)
    plain = mapper.records_host(mapper.snapshot(res, md=False), rargs)
    withmd = mapper.records(res, names, reads)
    assert _check_sam_with_md(mapper, res, reads, g, [b"chrA", b"chrB"], plain, withmd) >= len(reads) // 2
    assert parallel.records_from_packed(ctx.lib, mapper.copts, parallel.pack_records(ctx, res, print_md=True), names, reads, mapper.chrom_names) == withmd
