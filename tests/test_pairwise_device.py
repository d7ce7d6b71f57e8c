"""Print format 'a' on the device: lra_alignment_strings_batch and lra_pairwise_text_batch against the reference's own CreateAlignmentStrings /
PrintPairwise output (tests/golden/aln_strings_golden.json) and against the host functions tests/test_order.py pins to it, and the record stage
(lra_map_records_device, printFormat 'a') against lra_map_records_host_tags on a LRA_PACK_BLOCKS snapshot, byte for byte."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from lra_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GUARD = 0xA5
W = 50                                                                     # PrintPairwise's columns per row


def _batch(ctx, cases):
    """cases: (read bytes, text bytes, blocks [nb, 3]) -> ONE RefineBatch; every case has its own read and text offsets."""
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
    blocks = np.concatenate(bl) if sum(len(x) for x in bl) else np.zeros((1, 3), np.int32)
    return refine.refine_batch_from_device(ctx, dev(blocks, np.int32).view(-1, 3), dev(boff, np.int64), qseq, dev(q_off, np.int64),
                                           dev([len(r) for r, _, _ in cases], np.int32), tseq, dev(t_off, np.int64), dev([len(t) for _, t, _ in cases], np.int64))


def _text_with_guard(ctx, rb):
    """lra_pairwise_text_batch with a guard pattern laid behind the text before the call -> per-alignment bytes (the guard must survive)."""
    import torch
    from lra_amd import refine
    r0 = refine.pairwise_text_batch(ctx, rb, raw=True)                      # sizes the context's buffers; then the guard goes behind the text
    nb, n = int(r0.n_bytes), int(r0.n_aln)
    guard = torch.full((48,), GUARD, dtype=torch.uint8, device=ctx.device)
    ctx.check(ctx.lib.lra_copy_device(ctx.h, C.c_void_p(r0.d_text + nb), C.c_void_p(guard.data_ptr()), C.c_uint64(48)))
    torch.cuda.synchronize()
    res = refine.pairwise_text_batch(ctx, rb, raw=True)
    assert int(res.n_bytes) == nb and int(res.n_aln) == n and res.d_text == r0.d_text
    off = ctx.to_host(res.d_off, n + 1, np.uint64)
    raw = ctx.to_host(res.d_text, nb + 48, np.uint8).tobytes()
    assert raw[nb:] == bytes([GUARD]) * 48, "bytes behind the last offset were written"
    assert int(off[0]) == 0 and int(off[-1]) == nb
    return [raw[int(off[i]):int(off[i + 1])] for i in range(n)]


def _closed_form(cols):
    return 46 * ((cols + W - 1) // W) + 3 * cols


# ---------------------------------------------------------------------------------------------------------------- the reference's goldens
@pytest.fixture(scope="module")
def gold():
    cases = json.load(open(os.path.join(HERE, "golden", "aln_strings_golden.json")))["cases"]
    out = []
    for k in cases:
        lines = k["expected"].split("\n")
        assert lines[0][:2] == "Q " and lines[1][:2] == "A " and lines[2][:2] == "T " and lines[3][:2] == "R " and lines[4][:2] == "M "
        rest = lines[5:]
        assert rest[0] == k["name"]
        rest = rest[1:]
        if k["blocks"]:
            assert rest[0].startswith("Interval:\t")
            rest = rest[1:]
        out.append(dict(case=(k["read"].encode(), k["text"].encode(), k["blocks"]), q=lines[0][2:].encode(), a=lines[1][2:].replace("_", " ").encode(),
                        t=lines[2][2:].encode(), r=int(lines[3][2:]), body="\n".join(rest).encode()))
    assert len(out) == 160 and sum(not g["case"][2] for g in out) == 32
    return out


@pytest.mark.gpu
def test_strings_match_reference_goldens(ctx, gold):
    from lra_amd import refine
    strings, ref_len = refine.alignment_strings_batch(ctx, _batch(ctx, [g["case"] for g in gold]))
    assert len(strings) == len(gold)
    for i, (g, (q, a, t)) in enumerate(zip(gold, strings)):
        assert (q, a, t) == (g["q"], g["a"], g["t"]), i
        assert int(ref_len[i]) == g["r"], i
    assert any(b" " in a for _, a, _ in strings) and any(b"*" in a for _, a, _ in strings)


@pytest.mark.gpu
def test_text_matches_reference_goldens(ctx, gold):
    from lra_amd import refine
    got = _text_with_guard(ctx, _batch(ctx, [g["case"] for g in gold]))
    assert len(got) == len(gold)
    rows = set()
    for i, (g, txt) in enumerate(zip(gold, got)):
        assert txt == g["body"], (i, txt[:300], g["body"][:300])
        assert len(txt) == _closed_form(len(g["q"])), i
        rows.add((len(g["q"]) + W - 1) // W)
    assert {0, 1, 2, 3} <= rows
    # an empty batch is a call like any other
    empty = _batch(ctx, [])
    assert refine.pairwise_text_batch(ctx, empty) == [] and refine.alignment_strings_batch(ctx, empty)[0] == []
    assert int(refine.pairwise_text_batch(ctx, empty, raw=True).n_bytes) == 0


# ---------------------------------------------------------------------------------------------------------------- edges against the host functions
def _host(lib, name, chrom, read, text, blocks):
    """(q, a, t, ref_len, the rows lra_format_pairwise prints) from the host functions tests/test_order.py pins to the reference."""
    b = np.ascontiguousarray(np.asarray(blocks, np.int32).reshape(-1))
    nb = len(b) // 3
    bp = b.ctypes.data_as(C.c_void_p) if nb else None
    n = C.c_uint64(0); rl = C.c_uint32(0)
    lib.lra_alignment_strings(read, text, bp, nb, None, None, None, C.c_uint64(0), C.byref(n), C.byref(rl))
    qb = C.create_string_buffer(n.value + 1); ab = C.create_string_buffer(n.value + 1); tb = C.create_string_buffer(n.value + 1)
    assert lib.lra_alignment_strings(read, text, bp, nb, qb, ab, tb, n, C.byref(n), C.byref(rl)) == 0
    q, a, t = qb.raw[:n.value], ab.raw[:n.value], tb.raw[:n.value]
    fq, ft = (int(b[0]), int(b[1])) if nb else (0, 0)
    args = (name, chrom, nb, fq, ft, rl, q, a, t, n)
    p = C.c_uint64(0)
    lib.lra_format_pairwise(*args, None, C.c_uint64(0), C.byref(p))
    pb = C.create_string_buffer(p.value + 1)
    assert lib.lra_format_pairwise(*args, pb, p, C.byref(p)) == 0
    full = pb.raw[:p.value]
    head = name + b"\n" + (b"Interval:\t%s:%d-%d\n" % (chrom, ft, (ft + rl.value) & 0xffffffff) if nb else b"")
    assert full.startswith(head)
    return q, a, t, rl.value, full[len(head):]


QALPHA = np.frombuffer(b"ACGTACGTACGTACGTacgtNn", np.uint8)
TALPHA = np.frombuffer(b"ACGTACGTACGTacgtacgtNnRY", np.uint8)


def _case(rng, parts, first_q=0, first_t=0):
    """parts: (length, qgap, tgap) per block (the last block's gaps are not used) -> (read, text, blocks): the read copies the text under its pair columns
    with some substitutions, lower case and N on either side."""
    lens = np.array([p[0] for p in parts], np.int64); qg = np.array([p[1] for p in parts], np.int64); tg = np.array([p[2] for p in parts], np.int64)
    q = first_q + np.concatenate([[0], np.cumsum(lens + qg)[:-1]])
    t = first_t + np.concatenate([[0], np.cumsum(lens + tg)[:-1]])
    qlen, tlen = int(q[-1] + lens[-1] + 3), int(t[-1] + lens[-1] + 3)
    text = TALPHA[rng.integers(0, len(TALPHA), tlen)].copy()
    read = QALPHA[rng.integers(0, len(QALPHA), qlen)].copy()
    # pair columns (blocks and the common stretch of two gaps alike): mostly the text's base, as stored or upper-cased
    for b in range(len(parts)):
        spans = [(int(q[b]), int(t[b]), int(lens[b]))]
        if b + 1 < len(parts):
            c = int(min(qg[b], tg[b]))
            spans.append((int(q[b + 1]) - c, int(t[b + 1]) - c, c))
        for qs, tstart, L in spans:
            if L:
                src = text[tstart:tstart + L].copy()
                up = np.where((src >= 97) & (src <= 122), src - 32, src)
                src = np.where(rng.random(L) < 0.5, up, src).astype(np.uint8)
                sub = rng.random(L) < 0.08
                src[sub] = QALPHA[rng.integers(0, len(QALPHA), int(sub.sum()))]
                read[qs:qs + L] = src
    return read.tobytes(), text.tobytes(), np.stack([q, t, lens], 1).astype(np.int32)


def _edge_cases(rng):
    from lra_amd import refine
    G = refine.PAIRWISE_GROUP_ROWS * refine.PAIRWISE_WIDTH                 # the columns of a wave's row group = its LDS tile
    none = (b"ACGT", b"ACGT", np.zeros((0, 3), np.int32))
    cs = [("zero-first", none), ("zero-first-adjacent", none)]
    add = lambda label, parts, fq=0, ft=0: cs.append((label, _case(rng, parts, fq, ft)))
    for n in (1, 49, 50, 51, 99, 100, 101, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1):
        add("one block of %d" % n, [(n, 0, 0)])
    cs.append(("zero-middle", none)); cs.append(("zero-middle-adjacent", none))
    mixed = [(1, int(rng.integers(0, 3)) if rng.random() < 0.5 else 0, int(rng.integers(0, 3)) if rng.random() < 0.5 else 0) for _ in range(4097)]
    add("4097 blocks of length 1", mixed, 7, 11)
    add("one block of 20000", [(20_000, 0, 0)], 3, 5)
    add("query gap only", [(20, 6, 0), (20, 0, 0)])
    add("text gap only", [(20, 0, 6), (20, 0, 0)])
    add("both, query longer", [(20, 5, 3), (20, 0, 0)])
    add("both, text longer", [(20, 3, 5), (20, 0, 0)])
    add("all common", [(20, 4, 4), (20, 0, 0)])
    add("gaps of 1", [(10, 1, 0), (10, 0, 1), (10, 1, 1), (10, 0, 0)])
    add("query gap of 500", [(30, 500, 0), (30, 0, 0)])
    add("text gap of 500", [(30, 0, 500), (30, 0, 0)])
    add("common stretch of 500", [(30, 500, 500), (30, 0, 0)])
    add("row boundary inside a query gap", [(45, 10, 0), (45, 10, 0), (30, 0, 0)], 2, 9)
    add("row boundary inside a text gap", [(45, 0, 10), (45, 0, 10), (30, 0, 0)], 2, 9)
    add("row boundary inside a common stretch", [(45, 10, 10), (40, 25, 10), (30, 0, 0)], 2, 9)
    add("row boundary inside a common stretch behind a net gap", [(30, 10, 25), (60, 0, 0)], 1, 1)
    add("zero-length first block", [(0, 3, 0), (30, 0, 0)], 4, 4)
    # the printed numbers cross a decimal width between two rows: the first row holds one base of the crossing side
    add("q 9 -> 10", [(1, 0, 49), (60, 0, 0)], 9, 40)
    add("t 9 -> 10", [(1, 49, 0), (60, 0, 0)], 40, 9)
    add("q 99 -> 100", [(1, 0, 49), (60, 0, 0)], 99, 0)
    add("t 99 -> 100", [(1, 49, 0), (60, 0, 0)], 0, 99)
    add("q 99999 -> 100000", [(1, 0, 49), (60, 0, 0)], 99_999, 3)
    add("t 99999 -> 100000", [(1, 49, 0), (60, 0, 0)], 3, 99_999)
    add("both through full rows", [(130, 0, 0)], 99_950, 99_950)
    cs.append(("zero-last-adjacent", none)); cs.append(("zero-last", none))
    return cs


@pytest.mark.gpu
def test_edges_match_host_functions(ctx):
    from lra_amd import refine
    rng = np.random.default_rng(20)
    labelled = _edge_cases(rng)
    cases = [c for _, c in labelled]
    want = [_host(ctx.lib, b"r%d" % i, b"chrE", *c) for i, c in enumerate(cases)]
    rb = _batch(ctx, cases)
    strings, ref_len = refine.alignment_strings_batch(ctx, rb)
    text = _text_with_guard(ctx, rb)
    for i, (label, _) in enumerate(labelled):
        q, a, t, rl, body = want[i]
        assert strings[i] == (q, a, t), label
        assert int(ref_len[i]) == rl, label
        if text[i] != body:
            at = next((k for k in range(min(len(text[i]), len(body))) if text[i][k] != body[k]), min(len(text[i]), len(body)))
            raise AssertionError("%s: %d / %d bytes, first difference at %d: %r / %r" % (label, len(text[i]), len(body), at, text[i][max(at - 60, 0):at + 60], body[max(at - 60, 0):at + 60]))
        assert len(body) == _closed_form(len(q)), label
    by = {l: want[i] for i, (l, _) in enumerate(labelled)}
    assert b"         9 q: " in by["q 9 -> 10"][4] and b"        10 q: " in by["q 9 -> 10"][4]
    assert b"        99 t: " in by["t 99 -> 100"][4] and b"       100 t: " in by["t 99 -> 100"][4]
    assert b"     99999 q: " in by["q 99999 -> 100000"][4] and b"    100000 q: " in by["q 99999 -> 100000"][4]
    assert b"    100000 t: " in by["both through full rows"][4]
    assert by["row boundary inside a query gap"][2][W - 1] == ord("-") and by["row boundary inside a query gap"][2][W] == ord("-")
    assert by["row boundary inside a text gap"][0][W - 1] == ord("-") and by["row boundary inside a text gap"][0][W] == ord("-")
    assert by["zero-first"][4] == b"" and by["zero-last"][4] == b""


# ---------------------------------------------------------------------------------------------------------------- the record stage
def _set(mapper, **kw):
    for k, v in kw.items():
        setattr(mapper.copts, k, ord(v) if k == "printFormat" else int(v))


def _noruns_pack_bytes(mapper, res):
    """The bytes of the LRA_PACK_NORUNS pack lra_map_records_device copies (the layout lra_map_pack documents, every array padded to 8 bytes)."""
    nR, nJ, nA, nCh = int(res.n_reads), int(res.n_jobs), int(res.n_alignments), len(mapper.chrom_names)
    sizes = [16 * 8, (nCh + 1) * 8, nJ, nR * 4, (nJ + 1) * 8] + [nA * 4] * 7 + [18 * nA * 4, (nA + 1) * 8, 2 * nA * 4, (nA + 1) * 8]
    return sum((s + 7) & ~7 for s in sizes)


def _device_equals_host(mapper, res, names, reads, tags):
    """records_device against records_host on a LRA_PACK_BLOCKS snapshot (per read: text and rec_off alike) -> the host's per-read texts."""
    args = mapper.record_args(names, reads)
    host = mapper.records_host(mapper.snapshot(res, with_blocks=True, md=False), args, passthrough=list(tags))
    dev = mapper.records_device(res, args, passthrough=list(tags), md=False)
    assert len(dev) == len(host) == len(names)
    for i, (d, h) in enumerate(zip(dev, host)):
        if d != h:
            at = next((k for k in range(min(len(d), len(h))) if d[k] != h[k]), min(len(d), len(h)))
            raise AssertionError("read %d: %d / %d bytes, first difference at %d: %r / %r" % (i, len(d), len(h), at, d[max(at - 60, 0):at + 60], h[max(at - 60, 0):at + 60]))
    st = mapper.records_device_stats()
    total = sum(len(t) for t in host)
    assert st["text_bytes"] == total
    if total:
        assert st["text_bytes"] > 0 and st["n_pieces"] > 0
        assert st["bytes_d2h"] < st["text_bytes"] + 64 * 1024 + _noruns_pack_bytes(mapper, res)      # no block crossed, and no fall-through (its stats are zeros)
    return host


def _ont_setup(ctx):
    from lra_amd import mapread
    rng = np.random.default_rng(4)
    genome = synth.make_genome(600_000, seed=78, repeat_frac=0.2, n_families=3).copy()
    genome[330_000:354_000] = genome[100_000:124_000]                      # a segmental duplication: two chains, secondary records under PrintNumAln 2
    CH = [0, 300_000, len(genome)]
    o = mapread.LowAccOptions()
    ik, ip = synth.build_global_index(genome, o.globalK, o.globalW, 100)
    mix = (30, 35, 35)
    sim = lambda a, n, rev=False, err=0.08: synth.simulate_read(rng, genome[a:a + n + 1], n, err, mix, rev)[0]
    junk = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    reads = [junk(2500)]                                                   # the first and the last read are unaligned
    reads += [sim(20_000, 5000), sim(50_000, 6000, True), sim(400_000, 4000), sim(450_000, 5500, True)]
    reads.append(np.concatenate([sim(130_000, 4500), sim(500_000, 4500, True)]))              # translocation, second half reversed: supplementary segments
    reads.append(synth.revcomp(np.concatenate([sim(200_000, 4000), sim(560_000, 4000)])))
    reads += [sim(104_000, 10_000, False, 0.02), sim(336_000, 10_000, True, 0.02)]            # inside the duplication
    reads.append(junk(3001))
    mapper = mapread.LowAccMapper(ctx, genome, ik, ip, [b"chrA", b"chrB"], CH, o)
    return mapper, [r.tobytes() for r in reads]


@pytest.mark.gpu
def test_record_stage_ont(ctx):
    import torch
    from lra_amd import seed
    mapper, reads = _ont_setup(ctx)
    n = len(reads)
    names = [b"read/%d" % i for i in range(n)]
    tags = [None if i % 3 == 0 else b"XA:i:%d" % i for i in range(n)]
    res = mapper.align(seed.ReadBatch(ctx, reads))
    _set(mapper, printFormat="a", PrintNumAln=1)
    one = _device_equals_host(mapper, res, names, reads, tags)
    assert one[0] == b"" and one[-1] == b"" and all(one[1:-1])                  # an unaligned read prints nothing in this format
    segs = [t.count(b"Interval:\t") for t in one]
    assert max(segs) >= 2                                                   # a split read: one view per segment
    fo = mapper.fetch(res)
    assert set(int(s) for s in fo["strand"]) == {0, 1}
    _set(mapper, PrintNumAln=2)
    two = _device_equals_host(mapper, res, names, reads, tags)
    assert sum(t.count(b"Interval:\t") for t in two) > sum(segs)             # the duplication's second alignment
    # a flagged read (LRA_ST_CAPACITY = 8) prints nothing, under both rules
    flag = torch.tensor([8], dtype=torch.int32, device=ctx.device)
    ctx.check(ctx.lib.lra_copy_device(ctx.h, C.c_void_p(res.d_read_status + 3 * 4), C.c_void_p(flag.data_ptr()), C.c_uint64(4)))
    torch.cuda.synchronize()
    for fu in (0, 1):
        _set(mapper, flagged_unaligned=fu)
        got = _device_equals_host(mapper, res, names, reads, tags)
        assert got[3] == b"" and got[1] == two[1]
    _set(mapper, flagged_unaligned=0, PrintNumAln=1)
    # the formats without a long field still fall through: the host path's text, no stage statistics
    _set(mapper, printFormat="b")
    assert any(mapper.records_device(res, mapper.record_args(names, reads))) and mapper.records_device_stats()["text_bytes"] == 0
    _set(mapper, printFormat="a")
    # a smaller batch after a larger one on the same context (the kept buffers are reused), then a batch of one unaligned read
    for sub in ([5, 1], [0]):
        r2 = [reads[i] for i in sub]
        res2 = mapper.align(seed.ReadBatch(ctx, r2))
        got = _device_equals_host(mapper, res2, [names[i] for i in sub], r2, [tags[i] for i in sub])
        assert [bool(t) for t in got] == [i != 0 for i in sub]


@pytest.mark.gpu
def test_record_stage_ccs(ctx):
    from lra_amd import seed, mapread
    import test_highacc_path as H
    g = H._genome_with_repeats(23)
    rng = np.random.default_rng(9)
    reads = [r.tobytes() for r in H._sv_reads(g, rng, 0.01, n_plain=3)]
    mapper = mapread.HighAccMapper(ctx, g, None, None, [b"chrA", b"chrB"], [0, 250_000, len(g)], "ccs", index_params=(17, 10, 150, 15, 1))
    names = [b"ccs%d" % i for i in range(len(reads))]
    res = mapper.align(seed.ReadBatch(ctx, reads))
    _set(mapper, printFormat="a")
    host = _device_equals_host(mapper, res, names, reads, [None] * len(reads))
    assert sum(bool(t) for t in host) >= len(reads) - 1 and max(t.count(b"Interval:\t") for t in host) >= 2


@pytest.mark.gpu
def test_map_files_device_records_writes_the_same_pairwise_file(ctx, tmp_path):
    rng = np.random.default_rng(22)
    genome = synth.make_genome(120_000, seed=6, repeat_frac=0.1, n_families=2)
    with open(tmp_path / "g.fa", "wb") as f:
        f.write(b">chr1 test\n" + genome.tobytes() + b"\n")
    with open(tmp_path / "r.fq", "wb") as f:
        for i, a in enumerate((5000, 40_000, 80_000)):
            r = synth.simulate_read(rng, genome[a:a + 3001], 3000, 0.08, (30, 35, 35), i == 1)[0].tobytes()
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, bytes(rng.integers(34, 74, len(r)).astype(np.uint8))))
    outs = []
    for extra in ([], ["--device-records"]):
        out = str(tmp_path / ("o%d.txt" % len(outs)))
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_files.py"), "-ONT", str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), "-p", "a", "-o", out] + extra,
                       check=True, cwd=ROOT, stderr=subprocess.DEVNULL)
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and outs[0].count(b"Interval:\t") >= 3 and b" q: " in outs[0]
