"""a14 IndelRefineAlignment: the fill of the 16-lane classes (rows of at most 16 and of 17 .. 32 cells, ir_fill_cols), whose lanes are laid out
by query column, against the oracle bit for bit.

In that layout a row's window [S, E] is a rotating range of a 16-lane ring, so the cases here are chosen by what moves the ring: rows whose
S advances by 0 (deletions), 1 (matches) and 2 or more (insertions) between two rows, rows of exactly 16 and 17 cells, windows that start
anywhere in the ring (and so wrap it), first and last rows, and segments that end at the end of the read (the query bases past the read are
its last base).  An advance of more than 16 does not occur in rows of at most 32 cells: an insertion of g bases only widens the rows of a
segment whose band k > g, to about 2 k + 1 + g cells.  Each test checks on the host, with the mirror of the reference's window loops, that
its segments have the shapes it is about, and the kernel's debug line that they ran in the classes the mirror assigns."""
import numpy as np
import pytest

from lra_amd import synth
from test_refine_paths import Aln, Batch, design, mirror_segments, mirror_windows, one_chrom_batch, predict, run, width_designs

pytestmark = pytest.mark.gpu

SCORES = [(4, -1, -2), (4, -3, -4), (4, -2, -1), (1, -1, -1), (10, -9, -12)]


def windows(batch, band, end_align=False):
    """The row windows of every DP segment of a batch, as the mirror predicts them."""
    out = []
    for a in batch.alns:
        _, segs = mirror_segments(a.blocks, band, a.read_len, a.chrom_len, end_align)
        for s in segs:
            if not s["aog"]:
                w = mirror_windows(s, band)
                if w is not None:
                    out.append((np.array(w[0]), np.array(w[1])))
    return out


def indel_reads(genome, band, rng, n):
    """Reads with one to three indels each (insertions and deletions of 1 .. band - 2 bases, a mismatch or two), blocks as designed."""
    reads, blocks = [], []
    for _ in range(n):
        t0 = int(rng.integers(1000, len(genome) - 2000))
        ops = [("m", int(rng.integers(12, 40)))]
        for _ in range(int(rng.integers(1, 4))):
            g = int(rng.integers(1, band - 1))
            ops += [("i" if rng.random() < 0.5 else "d", g), ("m", int(rng.integers(band + 2, 30))), ("x", 1), ("m", int(rng.integers(5, 30)))]
        r, b = design(genome, t0, ops, rng)
        reads.append(r); blocks.append(b)
    return reads, blocks


@pytest.mark.parametrize("par", SCORES)
@pytest.mark.parametrize("band", [5, 7, 10, 12])
def test_ring_moves(ctx, oracle, monkeypatch, capfd, band, par):
    """Rows whose window advances by 0, 1 and several cells, starting at every lane of the ring, in both 16-lane classes."""
    genome = synth.make_genome(200000, seed=41)
    rng = np.random.default_rng(100 + band)
    reads, blocks = indel_reads(genome, band, rng, 24)
    batch = one_chrom_batch(genome, reads, blocks)
    ws = windows(batch, band)
    adv = set()
    starts = set()
    for S, E in ws:
        adv.update(np.diff(S).tolist())
        starts.update((S % 16).tolist())
    assert {0, 1, 2} <= adv and max(adv) >= min(band - 2, 3), sorted(adv)
    assert starts == set(range(16))
    p = predict(batch.alns, band, False)
    assert p["classes"][0] + p["classes"][1] > 0
    if band >= 10:
        assert p["classes"][1] > 0
    res, dbg = run(ctx, oracle, monkeypatch, capfd, batch, band, par)
    assert dbg is not None and dbg["classes"] == p["classes"]


@pytest.mark.parametrize("par", SCORES)
def test_rows_of_16_and_17_cells(ctx, oracle, monkeypatch, capfd, par):
    """The widest row at 15, 16 (one piece, all 16 lanes) and 17, 18 cells (a second piece of one or two cells)."""
    genome = synth.make_genome(200000, seed=43)
    rng = np.random.default_rng(7)
    d = width_designs(genome, 7, rng)
    assert 16 in d and 17 in d
    reads, blocks = [], []
    for w in (15, 16, 17, 18):
        if w in d:
            reads.append(d[w][0]); blocks.append(d[w][1])
    batch = one_chrom_batch(genome, reads, blocks)
    widths = [int((E - S + 1).max()) for S, E in windows(batch, 7)]
    assert 16 in widths and 17 in widths
    p = predict(batch.alns, 7, False)
    assert p["classes"][0] > 0 and p["classes"][1] > 0
    res, dbg = run(ctx, oracle, monkeypatch, capfd, batch, 7, par)
    assert dbg["classes"] == p["classes"]


@pytest.mark.parametrize("band", [7, 12])
def test_segments_at_the_read_end(ctx, oracle, monkeypatch, capfd, band):
    """Segments whose last rows reach the read's last base (endAlign adds the tail block), so that the lanes past the read load its last
    base, and one-row-apart first and last rows of short segments."""
    genome = synth.make_genome(200000, seed=47)
    rng = np.random.default_rng(band)
    strands, alns = [], []
    for i in range(16):
        t0 = int(rng.integers(1000, len(genome) - 2000))
        g = 1 + i % (band - 2)
        tail = int(rng.integers(0, 4))
        ops = [("m", 30), ("i" if i % 2 else "d", g), ("m", band + 3 + i % 5), ("x", 1), ("m", 2 + tail)]
        r, b = design(genome, t0, ops, rng)
        if tail and len(b) > 1:
            b = b.copy(); b[-1, 2] -= tail                                    # the alignment stops short of the read: endAlign's tail block
        strands.append(r); alns.append(Aln(b, i, 0))
    batch = Batch(strands, [genome], alns)
    p = predict(batch.alns, band, True)
    assert p["classes"][0] + p["classes"][1] > 0
    res, dbg = run(ctx, oracle, monkeypatch, capfd, batch, band, (4, -2, -1), end_align=True)
    assert dbg["classes"] == p["classes"]
