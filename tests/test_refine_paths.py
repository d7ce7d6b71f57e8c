"""a14 IndelRefineAlignment: the HIP kernel's code paths at their edges, against the oracle bit for bit.

lra_indel_refine_batch picks its code by shape: the fill kernel by a segment's widest row (ir_fill<16>, ir_fill_16x2, ir_fill<64>,
ir_fill_wide), the band ring by refine_band (ir_band_chunk<16 / 64 / 128>), chunks of CB = 32 blocks that replay earlier chunks,
trace windows of 128 rows / 4096 path bytes, persistent fill grids and a gather grid capped at 262 140 workgroups.  Every case here is
built to land on one side of one of those limits, and each test proves it got there: a plain mirror of the reference's grouping and
row-window loops (IndelRefine.h:79-333, as oracle/indel_refine.cpp restates them) predicts the segments, their widths and chunks, and the
kernel's LRA_IR_DBG line (read back from stderr) must show the same counts."""
import ctypes as C
import re

import numpy as np
import pytest

from lra_amd import synth
from test_refine import perturb

pytestmark = pytest.mark.gpu

# (match, mismatch, indel): the two presets, then sets where ties decide (a mismatch = two indels), unit scores, and large scores
SCORES = [(4, -1, -2), (4, -3, -4), (4, -2, -1), (1, -1, -1), (2, -5, -3), (10, -9, -12)]
CB = 32                       # blocks per band chunk (indel_refine.hip)
GATHER_GRID = 65535 * 4       # ir_gather's grid cap

DBG = re.compile(r"\[ir\] n_seg (\d+) n_rows (\d+) n_cells (\d+) n_task (\d+) n_item (\d+) fill classes 16/32/64/wide: (\d+) (\d+) (\d+) (\d+)")


# ------------------------------------------------------------------------------------------------ case builders
def design(genome, t0, ops, rng):
    """A read written as edits of genome[t0:]: ("m", n) n bases copied, ("x", n) n bases substituted, ("i", n) n random bases
    inserted, ("d", n) n genome bases skipped.  Returns (read, blocks) with the read's true alignment as gapless blocks."""
    read, blocks = [], []
    q, t, diag = 0, t0, False
    for op, n in ops:
        if op in "mx":
            s = genome[t:t + n].copy()
            if op == "x":
                s = synth.BASES[(synth.CODE[s] + rng.integers(1, 4, size=n)) % 4]
            if diag:
                blocks[-1][2] += n
            else:
                blocks.append([q, t, n])
            read.append(s)
            q += n; t += n; diag = True
        elif op == "i":
            read.append(synth.BASES[rng.integers(0, 4, size=n)])
            q += n; diag = False
        else:
            t += n; diag = False
    return np.concatenate(read).astype(np.uint8), np.array(blocks, np.int32)


def split_blocks(blocks, rng, lo, hi, skip=0):
    """Every block cut into pieces of lo..hi bases; `skip` bases of both sequences are left out between two pieces (a gap that
    IndelRefine.h:243-250 moves back onto the diagonal)."""
    out = []
    for q, t, n in blocks:
        o = 0
        while o < n:
            m = int(min(n - o, rng.integers(lo, hi + 1)))
            out.append([q + o, t + o, m])
            o += m + skip
    return np.array(out, np.int32).reshape(-1, 3)


def simulate(rng, genome, length, err, mix):
    return synth.simulate_read_with_blocks(rng, genome, length, err, mix)


# ------------------------------------------------------------------------------------------------ mirror of the reference's loops
def mirror_segments(blocks, k, read_len=0, chrom_len=0, end_align=False):
    """The grouping loop (IndelRefine.h:79-211, :761-767).  Returns (number of output items, the segments: blocks as the segment sees
    them, qStart, tStart, qEnd, tEnd, tLen, whether it goes to AffineOneGapAlign)."""
    b = [[int(x) for x in r] for r in np.asarray(blocks).reshape(-1, 3)]
    if len(b) <= 1:
        return len(b), []
    if end_align:                                                       # :89-130
        q0, t0 = b[0][0], b[0][1]
        ms = min(q0, t0)
        qa, ta = b[-1][0] + b[-1][2], b[-1][1] + b[-1][2]
        me = min(read_len - qa, chrom_len - ta)
        if ms < 40:
            b.insert(0, [q0 - ms, t0 - ms, ms])
        if me < 40:
            b.append([qa, ta, me])
    nB, maxGap = len(b), k - 1
    items, segs = 0, []
    start = end = 0
    while end < nB:
        qStart, tStart = b[start][0], b[start][1]
        qPos, tPos = qStart + b[start][2], tStart + b[start][2]
        qGap = tGap = 0
        if end < nB - 1:
            tGap, qGap = b[end + 1][1] - tPos, b[end + 1][0] - qPos
        while end < nB - 1 and qGap < maxGap and tGap < maxGap and (start == end or b[end][2] < 100):
            end += 1
            qPos, tPos = b[end][0] + b[end][2], b[end][1] + b[end][2]
            if end + 1 < nB - 1:
                tGap, qGap = b[end + 1][1] - tPos, b[end + 1][0] - qPos
        alt = None
        if end == start:
            items += 1
        else:
            if b[start][2] > maxGap:
                adv = b[start][2] - maxGap
                items += 1
                b[start] = [b[start][0] + adv, b[start][1] + adv, maxGap]
                qStart += adv; tStart += adv
            if b[end][2] > maxGap:
                alt = [b[end][0] + maxGap, b[end][1] + maxGap, b[end][2] - maxGap]
                b[end] = [b[end][0], b[end][1], maxGap]
                qPos, tPos = b[end][0] + maxGap, b[end][1] + maxGap
            qEnd, tEnd = b[end][0] + b[end][2], b[end][1] + b[end][2]
            segs.append(dict(blocks=[tuple(x) for x in b[start:end + 1]], qStart=qStart, tStart=tStart, qEnd=qEnd, tEnd=tEnd,
                             tLen=tPos - tStart, aog=(tEnd - tStart < k or qEnd - qStart < k)))
            items += 1
        if alt is None:
            end += 1
        else:
            b[end] = alt
        start = end
    return items, segs


def block_steps(seg):
    """Per block of a segment: (rows, bqGap, btGap, length) of one iteration of the window loop (:232-315)."""
    bl, out = seg["blocks"], []
    for i, (bq, bt, n) in enumerate(bl):
        bqGap = btGap = 0
        if i < len(bl) - 1:
            bqGap, btGap = bl[i + 1][0] - (bq + n), bl[i + 1][1] - (bt + n)
            if bqGap > 0 and btGap > 0:
                c = min(bqGap, btGap); bqGap -= c; btGap -= c; n += c
        body = max(n, 0)
        out.append((body + (btGap if btGap > bqGap and btGap > 0 else 0), bqGap, btGap, n))
    return out


def mirror_windows(seg, k):
    """The row windows [qS, qE] of a DP segment (:220-333), or None where the reference would index out of range."""
    tLen, qStart, qEnd = seg["tLen"], seg["qStart"], seg["qEnd"]
    if tLen <= 0:
        return None
    qS, qE = [-1] * tLen, [-1] * tLen
    q, tOff = seg["blocks"][0][0], 0
    for _, bqGap, btGap, n in block_steps(seg):
        for _ in range(n):
            if tOff >= tLen:
                return None
            lo = max(q - k, qStart)
            qS[tOff] = lo if qS[tOff] == -1 else min(qS[tOff], lo)
            if qE[tOff] == -1 or qE[tOff] < q + k:
                qE[tOff] = min(qEnd - 1, q + k)
            for ki in range(k):
                if tOff - ki >= 0 and qE[tOff - ki] < q:
                    qE[tOff - ki] = q
                if tOff + ki < tLen and (qS[tOff + ki] == -1 or qS[tOff + ki] > q):
                    qS[tOff + ki] = q
            tOff += 1; q += 1
        if bqGap > btGap:
            for _ in range(bqGap):
                for ki in range(k):
                    if 0 <= tOff - ki < tLen and qE[tOff - ki] < q:
                        qE[tOff - ki] = q
                    if tOff + ki < tLen and (qS[tOff + ki] == 0 or qS[tOff + ki] > q):   # (sic) == 0, as the reference
                        qS[tOff + ki] = q
                q += 1
        if btGap > bqGap:
            for _ in range(btGap):
                if tOff >= tLen:
                    return None
                qS[tOff], qE[tOff] = max(q - k, qStart), min(qEnd - 1, q + k)
                tOff += 1
    for i in range(tLen - 1, 0, -1):
        qS[i - 1] = min(qS[i - 1], qS[i])
    for i in range(tLen - 1):
        qE[i + 1] = max(qE[i + 1], qE[i])
    if any(e < s or s < 0 for s, e in zip(qS, qE)):
        return None
    return qS, qE


def width_class(w):
    return 0 if w <= 16 else 1 if w <= 32 else 2 if w <= 64 else 3


def replay_depth(seg, k):
    """How many earlier chunks the deepest chunk of a segment replays (ir_band_chunk: back to a chunk that starts at or before row
    T0 - 2k + 1)."""
    rows = [r for r, _, _, _ in block_steps(seg)]
    starts = np.concatenate([[0], np.cumsum(rows)])[::CB]
    deepest = 0
    for c in range(1, len(starts)):
        f = c
        while f > 0:
            f -= 1
            if f == 0 or starts[c] - starts[f] >= 2 * k - 1:
                break
        deepest = max(deepest, c - f)
    return deepest


def predict(alns, k, end_align):
    """What the kernel's debug line must show for a batch: DP segments, chunks, items, cells, fill-class counts."""
    p = dict(n_item=0, n_dp=0, n_aog=0, n_task=0, n_cells=0, classes=[0, 0, 0, 0], widths=[], depth=0, max_blocks=0)
    for a in alns:
        items, segs = mirror_segments(a.blocks, k, a.read_len, a.chrom_len, end_align)
        p["n_item"] += items
        for s in segs:
            if s["aog"]:
                p["n_aog"] += 1
                continue
            p["n_dp"] += 1
            p["n_task"] += (len(s["blocks"]) + CB - 1) // CB
            p["max_blocks"] = max(p["max_blocks"], len(s["blocks"]))
            p["depth"] = max(p["depth"], replay_depth(s, k))
            w = mirror_windows(s, k)
            if w is None:
                continue
            width = max(e - s_ + 1 for s_, e in zip(*w))
            p["widths"].append(width)
            p["classes"][width_class(width)] += 1
            p["n_cells"] += sum(e - s_ + 1 for s_, e in zip(*w))
    return p


# ------------------------------------------------------------------------------------------------ running a batch
class Aln:
    """One alignment: its blocks, the read strand (index into the batch's strands) and the chromosome (index) it lies on."""

    def __init__(self, blocks, strand, chrom):
        self.blocks = np.asarray(blocks, np.int32).reshape(-1, 3)
        self.strand, self.chrom = strand, chrom
        self.read_len = self.chrom_len = 0


class Batch:
    """Read strands and chromosomes packed into one query and one target buffer each, behind a few bytes of padding (non-zero
    offsets everywhere; the target buffer runs past every chromosome)."""

    def __init__(self, strands, chroms, alns):
        self.strands, self.chroms, self.alns = strands, chroms, alns
        for a in alns:
            a.read_len, a.chrom_len = len(strands[a.strand]), len(chroms[a.chrom])

    def device(self, ctx):
        import torch
        from lra_amd import refine
        pad = np.frombuffer(b"TTGCA" * 7, np.uint8)
        qparts, qoff, o = [pad], [], len(pad)
        for s in self.strands:
            qoff.append(o); qparts += [s, pad]; o += len(s) + len(pad)
        tparts, toff, o = [pad], [], len(pad)
        for c in self.chroms:
            toff.append(o); tparts += [c, pad]; o += len(c) + len(pad)
        qdev = torch.from_numpy(np.concatenate(qparts + [np.zeros(64, np.uint8)])).to(ctx.device)
        tdev = torch.from_numpy(np.concatenate(tparts + [np.zeros(64, np.uint8)])).to(ctx.device)
        A = self.alns
        return refine.RefineBatch(ctx, [a.blocks for a in A], qdev, np.array([qoff[a.strand] for a in A], np.int64),
                                  np.array([a.read_len for a in A], np.int32), tdev, np.array([toff[a.chrom] for a in A], np.int64),
                                  np.array([a.chrom_len for a in A], np.int64))

    def expected(self, oracle, band, par, end_align):
        qb = [s.tobytes() for s in self.strands]
        tb = [c.tobytes() for c in self.chroms]
        return [oracle.indel_refine(a.blocks, qb[a.strand], tb[a.chrom], band, *par, end_align=end_align, read_len=a.read_len,
                                    chrom_len=a.chrom_len) for a in self.alns]


def run(ctx, oracle, monkeypatch, capfd, batch, band, par, end_align=False, all_ok=True):
    """Refine a batch on the device with the debug line on, compare every alignment with the oracle.  Returns (res, debug counts)."""
    from lra_amd import refine
    b = batch.device(ctx)
    monkeypatch.setenv("LRA_IR_DBG", "1")
    capfd.readouterr()
    res = refine.indel_refine_batch(ctx, b, band, *par, end_align=end_align)
    lines = DBG.findall(capfd.readouterr().err)
    monkeypatch.delenv("LRA_IR_DBG")
    got, status = refine.fetch(ctx, res)
    exp = batch.expected(oracle, band, par, end_align)
    n_ok = 0
    for i, (e, st) in enumerate(exp):
        assert (status[i] != 0) == (st != 0), (i, status[i], st)
        if st == 0:
            n_ok += 1
            assert np.array_equal(got[i], e), (i, len(got[i]), len(e))
    if all_ok:
        assert n_ok == len(exp)
    if not lines:                                                       # (the line is printed whenever the batch has a segment)
        assert res.n_segments == 0
        return res, None
    assert len(lines) == 1, lines
    v = [int(x) for x in lines[0]]
    dbg = dict(n_seg=v[0], n_rows=v[1], n_cells=v[2], n_task=v[3], n_item=v[4], classes=v[5:9])
    assert (dbg["n_seg"], dbg["n_rows"], dbg["n_cells"]) == (res.n_segments, res.n_rows, res.n_cells)
    return res, dbg


def check_predicted(res, dbg, p):
    """The kernel saw the shapes the mirror predicts."""
    assert dbg is not None
    assert dbg["n_item"] == p["n_item"]
    assert dbg["n_seg"] == p["n_dp"] + p["n_aog"] and res.n_aog == p["n_aog"]
    assert dbg["n_task"] == p["n_task"]
    assert dbg["classes"] == p["classes"], (dbg["classes"], p["classes"])
    assert dbg["n_cells"] == p["n_cells"]


def one_chrom_batch(genome, reads, blocks):
    return Batch(list(reads), [genome], [Aln(b, i, 0) for i, b in enumerate(blocks)])


# ------------------------------------------------------------------------------------------------ 1. fill classes at their limits
def width_designs(genome, k, rng):
    """Two-block segments around one insertion of g bases, g = 0 .. k - 2 (a gap of k - 1 would end the segment), each with a
    mismatch or two in its blocks: the insertion widens the rows around it by about g.  Returns {width: (read, blocks)}."""
    out = {}
    for g in range(0, k - 1):
        t0 = int(rng.integers(1000, len(genome) - 1000))
        ops = [("m", 20), ("x", 1), ("m", 25 + g)] + ([("i", g)] if g else [("d", 1)]) + [("m", 30), ("x", 1), ("m", 15)]
        r, b = design(genome, t0, ops, rng)
        _, segs = mirror_segments(b, k)
        ws = [max(e - s + 1 for s, e in zip(*mirror_windows(s_, k))) for s_ in segs if not s_["aog"]]
        for w in ws:
            out.setdefault(w, (r, b))
    return out


@pytest.mark.parametrize("band,limit", [(7, 16), (15, 32), (31, 64), (64, 1024)])
@pytest.mark.parametrize("par", SCORES)
def test_fill_classes_at_their_limits(ctx, oracle, monkeypatch, capfd, band, limit, par):
    """Segments whose widest row is just at and just past a fill class's limit (16|17, 32|33, 64|65), and rows of a few hundred
    cells under band 64 (stacked insertions): each class's kernel must run, on exactly the segments the mirror assigns to it."""
    genome = synth.make_genome(200000, seed=31)
    rng = np.random.default_rng(band)
    reads, blocks = [], []
    if limit < 1024:
        d = width_designs(genome, band, rng)
        assert limit in d and limit + 1 in d, sorted(d)
        for w in (limit - 1, limit, limit + 1, limit + 2):
            if w in d:
                reads.append(d[w][0]); blocks.append(d[w][1])
        # the same two shapes again at other places of the genome (other bases, other ties)
        for w in (limit, limit + 1):
            r, b = d[w]
            t0 = int(rng.integers(1000, len(genome) - 2000))
            shift = t0 - int(b[0, 1])
            nb = b.copy(); nb[:, 1] += shift
            nr = r.copy()
            for q, t, n in nb:
                nr[q:q + n] = genome[t:t + n]
            reads.append(nr); blocks.append(nb)
    else:
        for n_ins, ins in [(3, 60), (5, 61), (8, 62)]:                  # 1-base blocks between long insertions: windows of ~n_ins * ins cells
            t0 = int(rng.integers(1000, len(genome) - 2000))
            ops = [("m", 80)] + [("m", 1), ("i", ins)] * n_ins + [("m", 80)]
            r, b = design(genome, t0, ops, rng)
            reads.append(r); blocks.append(b)
    # a few ordinary reads beside them
    for _ in range(4):
        r, b = simulate(rng, genome, 1500, 0.08, (30, 35, 35))
        reads.append(r); blocks.append(perturb(rng, b))
    batch = one_chrom_batch(genome, reads, blocks)
    p = predict(batch.alns, band, False)
    if limit < 1024:
        assert limit in p["widths"] and limit + 1 in p["widths"]
        lo, hi = width_class(limit), width_class(limit + 1)
        assert p["classes"][lo] > 0 and p["classes"][hi] > 0
    else:
        assert max(p["widths"]) > 200 and p["classes"][3] > 0
    res, dbg = run(ctx, oracle, monkeypatch, capfd, batch, band, par)
    check_predicted(res, dbg, p)


# ------------------------------------------------------------------------------------------------ 2. band boundaries, invalid arguments
@pytest.mark.parametrize("end_align", [False, True])
@pytest.mark.parametrize("band", [2, 3, 8, 9, 16, 32, 33, 63, 64])
def test_band_boundaries(ctx, oracle, monkeypatch, capfd, band, end_align):
    """refine_band on both sides of the ring templates' limits (8 | 9 -> ir_band_chunk<16> | <64>, 32 | 33 -> <64> | <128>) and of
    the ABI's range (2, 64), with reads near the genome's ends so that end_align adds head and tail blocks."""
    genome = synth.make_genome(120000, seed=40 + band)
    rng = np.random.default_rng(1000 + band)
    par = SCORES[band % len(SCORES)]
    reads, blocks = [], []
    for err, mix in [(0.10, (30, 35, 35)), (0.15, (20, 40, 40)), (0.03, (80, 10, 10))]:
        for _ in range(4):
            r, b = simulate(rng, genome, 2500, err, mix)
            b = perturb(rng, b, 0.1, 0.3)
            if band <= 3:                                               # small gaps join blocks only under wide bands: cut blocks into touching pieces
                b = split_blocks(b, rng, 5, 60)
            reads.append(r); blocks.append(b)
    for d in (0, 1, 39, 40, 41):                                        # reads from the genome's first / last bases
        r = genome[d:d + 700].copy(); r[::37] = synth.BASES[(synth.CODE[r[::37]] + 1) % 4]
        reads.append(r); blocks.append(split_blocks(np.array([[0, d, 700]], np.int32), rng, 20, 90, skip=1))
        s = len(genome) - 700 - d
        r = genome[s:s + 700].copy(); r[::41] = synth.BASES[(synth.CODE[r[::41]] + 2) % 4]
        reads.append(r); blocks.append(split_blocks(np.array([[0, s, 700]], np.int32), rng, 20, 90, skip=1))
    batch = one_chrom_batch(genome, reads, blocks)
    res, dbg = run(ctx, oracle, monkeypatch, capfd, batch, band, par, end_align)
    assert dbg is not None and dbg["n_task"] > 0 and sum(dbg["classes"]) > 0


def _raw_call(ctx, b, band, match, mismatch, indel, res):
    from lra_amd.context import ptr
    return ctx.lib.lra_indel_refine_batch(ctx.h, b.n, ptr(b.blocks), ptr(b.block_off), C.c_uint64(b.n_blocks_in), ptr(b.q_seq), ptr(b.q_off),
                                          ptr(b.q_len), ptr(b.t_seq), ptr(b.t_off), ptr(b.t_len), band, match, mismatch, indel, 0, C.byref(res))


@pytest.mark.parametrize("band,indel", [(1, -2), (65, -2), (0, -2), (7, 0), (7, 1), (64, 0)])
def test_invalid_arguments_launch_nothing(ctx, oracle, monkeypatch, capfd, band, indel):
    """refine_band outside 2..64 or an indel score >= 0: LRA_ERR_INVALID, nothing launched, the result untouched, and the next valid
    call on the same context is right."""
    from lra_amd import refine
    genome = synth.make_genome(60000, seed=50)
    rng = np.random.default_rng(50)
    reads, blocks = [], []
    for _ in range(6):
        r, b = simulate(rng, genome, 2000, 0.10, (30, 35, 35))
        reads.append(r); blocks.append(perturb(rng, b))
    batch = one_chrom_batch(genome, reads, blocks)
    b = batch.device(ctx)
    res = refine.RefineResult()
    res.n_aln, res.n_blocks, res.n_segments = 12345, 777, 999
    monkeypatch.setenv("LRA_IR_DBG", "1")
    capfd.readouterr()
    rc = _raw_call(ctx, b, band, 4, -1, indel, res)
    err = capfd.readouterr().err
    monkeypatch.delenv("LRA_IR_DBG")
    assert rc == -1                                                     # LRA_ERR_INVALID
    assert (res.n_aln, res.n_blocks, res.n_segments) == (12345, 777, 999)
    assert "[ir]" not in err
    run(ctx, oracle, monkeypatch, capfd, batch, 7, (4, -1, -2))


# ------------------------------------------------------------------------------------------------ 3. chunking and replay
@pytest.mark.parametrize("band", [7, 33])
def test_chunk_boundaries(ctx, oracle, monkeypatch, capfd, band):
    """Segments of exactly 31, 32, 33, 64 and 65 blocks (one, two and three chunks of CB = 32, last chunks of one block)."""
    genome = synth.make_genome(150000, seed=60)
    rng = np.random.default_rng(60 + band)
    reads, blocks, want = [], [], (31, 32, 33, 64, 65)
    for i, n in enumerate(want * 2):
        par_err = (0.08, (30, 35, 35)) if i < len(want) else (0.12, (10, 45, 45))
        while True:
            r, b = simulate(rng, genome, 4000, *par_err)
            b = split_blocks(b, rng, 3, 40)
            b = b[:n + 8]
            # keep a run of n blocks whose gaps all join (every gap under maxGap on both sequences), starting after a gap too
            gq = b[1:, 0] - b[:-1, 0] - b[:-1, 2]
            gt = b[1:, 1] - b[:-1, 1] - b[:-1, 2]
            if len(b) >= n and np.all(gq[:n - 1] < band - 1) and np.all(gt[:n - 1] < band - 1):
                break
        reads.append(r); blocks.append(b[:n])
    batch = one_chrom_batch(genome, reads, blocks)
    p = predict(batch.alns, band, False)
    seg_blocks = sorted(len(s["blocks"]) for a in batch.alns for s in mirror_segments(a.blocks, band)[1] if not s["aog"])
    for n in want:
        assert n in seg_blocks, (n, seg_blocks)
    assert p["n_task"] == sum((n + CB - 1) // CB for n in seg_blocks)
    res, dbg = run(ctx, oracle, monkeypatch, capfd, batch, band, SCORES[band % len(SCORES)])
    check_predicted(res, dbg, p)


@pytest.mark.parametrize("band,par", [(33, (4, -1, -2)), (64, (4, -3, -4)), (33, (4, -2, -1)), (64, (2, -5, -3))])
def test_chunk_replay_crosses_chunks(ctx, oracle, monkeypatch, capfd, band, par):
    """Reads cut into blocks of 1-3 bases under a wide band: 32 blocks span fewer than 2k - 1 rows, so a chunk's replay has to walk back
    over two or more earlier chunks."""
    genome = synth.make_genome(150000, seed=70)
    rng = np.random.default_rng(band + par[2])
    reads, blocks = [], []
    for err, mix in [(0.0, (34, 33, 33)), (0.06, (30, 35, 35)), (0.10, (20, 40, 40)), (0.05, (100, 0, 0))]:
        for _ in range(2):
            r, b = simulate(rng, genome, 1500, err, mix)
            reads.append(r); blocks.append(split_blocks(b, rng, 1, 3))
    batch = one_chrom_batch(genome, reads, blocks)
    p = predict(batch.alns, band, False)
    assert p["depth"] >= 2 and p["max_blocks"] > 8 * CB
    res, dbg = run(ctx, oracle, monkeypatch, capfd, batch, band, par)
    check_predicted(res, dbg, p)
    assert dbg["n_task"] > 8 * res.n_segments


# ------------------------------------------------------------------------------------------------ 4. trace windows
@pytest.mark.parametrize("band", [7, 64])
@pytest.mark.parametrize("kind", ["exact", "indels", "mismatches"])
def test_trace_windows(ctx, oracle, monkeypatch, capfd, kind, band):
    """Segments of thousands of rows, one per read (blocks cut into touching pieces of under 100 bases): exact reads, whose paths are
    diagonal runs far longer than the 64 cells the trace looks ahead, reads with indels only, reads with mismatches only.  Under band 64
    a window holds only ~30 rows of path bytes, under band 7 it is 128 rows: both refill many times."""
    genome = synth.make_genome(200000, seed=80)
    rng = np.random.default_rng(80 + band)
    err, mix = {"exact": (0.0, (34, 33, 33)), "indels": (0.08, (0, 50, 50)), "mismatches": (0.10, (100, 0, 0))}[kind]
    reads, blocks = [], []
    for L in (3000, 6000, 9000):
        r, b = simulate(rng, genome, L, err, mix)
        reads.append(r); blocks.append(split_blocks(b, rng, 40, 99))
    par = SCORES[(band + len(kind)) % len(SCORES)]
    res, dbg = run(ctx, oracle, monkeypatch, capfd, one_chrom_batch(genome, reads, blocks), band, par)
    assert res.n_segments == 3 and res.n_aog == 0
    assert res.n_rows / res.n_segments > 2500
    assert res.n_cells >= res.n_rows * (band + 1)                      # rows of about 2k + 1 cells
    assert (dbg["classes"][0] + dbg["classes"][1] if band == 7 else dbg["classes"][3]) == 3


# ------------------------------------------------------------------------------------------------ 5. scores
@pytest.mark.parametrize("par", [(4, -1, -2), (4, -2, -1), (10, -9, -12)])
def test_scores_past_int17(ctx, oracle, monkeypatch, capfd, par):
    """One segment of 45 kb at 1 % error: its scores pass 2^17 (45 000 x match), far outside any 16-bit arithmetic."""
    genome = synth.make_genome(300000, seed=90)
    rng = np.random.default_rng(90)
    r, b = simulate(rng, genome, 45000, 0.01, (34, 33, 33))
    b = split_blocks(b, rng, 50, 99)
    r2, b2 = simulate(rng, genome, 12000, 0.05, (30, 35, 35))
    b2 = split_blocks(b2, rng, 30, 99)
    res, dbg = run(ctx, oracle, monkeypatch, capfd, one_chrom_batch(genome, [r, r2], [b, b2]), 7, par)
    assert res.n_segments == 2 and res.n_rows > 44000 + 11000


# ------------------------------------------------------------------------------------------------ 6. layout
def layout_batch(seed):
    """Two chromosomes (N runs in both) in one target buffer; reads with several alignments on both strands; alignments that start
    or end 0, 1, 39, 40, 41 bases from the read's and the chromosome's ends; N in the read, in the genome and on both sides; empty and
    single-block alignments between them."""
    rng = np.random.default_rng(seed)
    chroms = [synth.make_genome(90000, seed=seed), synth.make_genome(50000, seed=seed + 1)]
    for c in chroms:
        for p in rng.integers(0, len(c) - 30, size=40):
            c[p:p + int(rng.integers(1, 25))] = ord("N")
    strands, alns = [], []

    def add_read(fwd):
        strands.append(fwd); strands.append(synth.revcomp(fwd))
        return len(strands) - 2, len(strands) - 1

    for i in range(10):                                                 # chimeric reads: part A forward on chrom 0, part B reverse on chrom 1
        rA, bA = simulate(rng, chroms[0], int(rng.integers(1500, 4000)), 0.10, (30, 35, 35))
        rB, bB = simulate(rng, chroms[1], int(rng.integers(1500, 4000)), 0.08, (20, 40, 40))
        for rr in (rA, rB):                                             # N in the reads too, some where the genome has N
            for p in rng.integers(0, len(rr) - 10, size=6):
                rr[p:p + int(rng.integers(1, 6))] = ord("N")
        fwd = np.concatenate([rA, synth.revcomp(rB)])
        sf, sr = add_read(fwd)
        bA, bB = perturb(rng, bA), perturb(rng, bB)                     # rc strand = rB + revcomp(rA): part B's blocks as they are
        h = len(bA) // 2
        alns += [Aln(bA[:h], sf, 0), Aln(bA[h:], sf, 0), Aln(bB, sr, 1)]
        if i % 3 == 0:
            alns += [Aln(np.zeros((0, 3), np.int32), sf, 0), Aln(bB[:1], sr, 1)]
    for d in (0, 1, 39, 40, 41):                                        # distances to the read's ends (the alignment's q)
        for ci, c in enumerate(chroms):
            t0 = int(rng.integers(1000, len(c) - 3000))
            r, b = design(c, t0, [("m", 300), ("i", 2), ("m", 200), ("x", 1), ("m", 150), ("d", 3), ("m", 300)], rng)
            b[0, [0, 1]] += d; b[0, 2] -= d; b[-1, 2] -= d
            s, _ = add_read(r)
            alns.append(Aln(split_blocks(b, rng, 30, 90), s, ci))
        for ci, c in enumerate(chroms):                                 # distances to the chromosome's ends (the read runs past them)
            head = synth.BASES[rng.integers(0, 4, size=120)]
            r, b = design(c, d, [("m", 400), ("i", 1), ("m", 300)], rng)
            r = np.concatenate([head, r]); b = b.copy(); b[:, 0] += 120
            s, _ = add_read(r)
            alns.append(Aln(split_blocks(b, rng, 30, 90), s, ci))
            L = 700 + 3
            r, b = design(c, len(c) - d - L, [("m", 350), ("d", 3), ("m", 350)], rng)
            r = np.concatenate([r, synth.BASES[rng.integers(0, 4, size=120)]])
            s, _ = add_read(r)
            alns.append(Aln(split_blocks(b, rng, 30, 90), s, ci))
    return Batch(strands, chroms, alns)


@pytest.mark.parametrize("end_align", [False, True])
@pytest.mark.parametrize("band,par", [(7, (4, -1, -2)), (50, (4, -3, -4)), (20, (4, -2, -1))])
def test_layout(ctx, oracle, monkeypatch, capfd, band, par, end_align):
    """Many alignments per read on both strands' buffers, two chromosomes at non-zero offsets of one target buffer, the ends of reads
    and chromosomes at 0 / 1 / 39 / 40 / 41 bases (end_align adds head and tail blocks there), N bases, empty and single-block alignments."""
    batch = layout_batch(100 + band)
    assert len({a.chrom for a in batch.alns}) == 2 and max(a.strand for a in batch.alns) > 20
    res, dbg = run(ctx, oracle, monkeypatch, capfd, batch, band, par, end_align)
    assert res.n_segments > 0 and dbg["n_item"] > len(batch.alns)


# ------------------------------------------------------------------------------------------------ large batch
def test_large_batch_grids_loop(ctx, oracle, monkeypatch, capfd):
    """More than 40 000 fill segments and 262 140 output items in one call: the persistent fill grids (num_cu x 32 workgroups) and
    ir_gather's capped grid loop; AffineOneGapAlign segments among them."""
    genome = synth.make_genome(400000, seed=110)
    rng = np.random.default_rng(110)
    reads, blocks = [], []
    band = 7
    for _ in range(2000):
        r, b = simulate(rng, genome, 2500, 0.12, (20, 40, 40))
        # holes of `band` or more bases on both sequences between pieces of 3-12 bases: every piece alone is an item of its own,
        # every truth indel starts a short segment
        b = split_blocks(b, rng, 3, 12, skip=band + int(rng.integers(0, 3)))
        reads.append(r); blocks.append(b)
    batch = one_chrom_batch(genome, reads, blocks)
    res, dbg = run(ctx, oracle, monkeypatch, capfd, batch, band, (4, -1, -2), all_ok=False)
    assert dbg["n_item"] > GATHER_GRID
    assert sum(dbg["classes"]) >= 40000
    assert dbg["classes"][0] > 256 * 32 * 4                           # ir_fill<16>: more segments than 256 CUs x 32 workgroups x 4 per wave
    assert res.n_aog > 0
