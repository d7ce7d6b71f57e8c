"""ir_segment (indel_refine.hip) as a wave per alignment: rounds of SEG_TILE blocks, a lane each, the segments' ends found in the round's ballots, a segment that runs
across rounds, the wave-wide copy into the augmented block list and the items written 64 at a time -- through lra_indel_refine_batch against the oracle's refined blocks,
with endAlign on and off (the added start block shifts every block by one against the rounds).  Alignments of 0, 1, 2, T - 1, T, T + 1 and 3 T blocks; gaps of k - 2,
k - 1 and k; a segment whose long last block leaves its "alt" remainder, and a block of 100 and more that ends a segment, at T - 2 .. T + 1 and 2 T - 1, 2 T.
test_crafted_alignments_group_as_intended asserts on the CPU, with the reference's grouping loop, where the segments of every crafted alignment end."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from lra_amd import synth

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lra_amd", "csrc", "indel_refine.hip")
T = int(re.search(r"constexpr int SEG_TILE = (\d+);", open(_SRC).read()).group(1))           # blocks per round, where the kernel defines it
K = 7                                                                       # refineBand: segments grow across gaps below K - 1
PAR = (4, -1, -2)
T0, LEAD = 1000, 10                                                         # the alignments start 10 bases into a read that copies the genome from 1000
EDGES = (T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T)


def _aln(lens, gaps):
    """blocks on the main diagonal of a read that copies the genome exactly: block i has lens[i] bases, gaps[i] unaligned bases on both sequences follow it"""
    lens = np.asarray(lens, np.int64); gaps = np.asarray(gaps, np.int64)
    assert len(gaps) == max(len(lens) - 1, 0)
    p = LEAD + np.concatenate([[0], np.cumsum(lens[:-1] + gaps)]) if len(lens) else np.zeros(0, np.int64)
    return np.stack([p, T0 + p, lens], axis=1).astype(np.int32) if len(lens) else np.zeros((0, 3), np.int32)


def _uniform(n):
    return _aln(np.full(n, 8), np.full(max(n - 1, 0), 2))


def _gap_mix(n):
    g = np.full(n - 1, 2); i = np.arange(n - 1)
    g[i % 7 == 2] = K - 2; g[i % 7 == 4] = K - 1; g[i % 7 == 6] = K
    return _aln(np.full(n, 8), g)


def _alt_at(pos, n):
    """the only gap of K follows block `pos`, which is 30 long: the segment ends there and leaves a remainder of 30 - (K - 1), a block by itself before the gap"""
    lens = np.full(n, 8); lens[pos] = 30
    g = np.full(n - 1, 2); g[pos] = K
    return _aln(lens, g)


def _long_at(pos, n):
    """block `pos` has 120 bases: a segment that reaches it ends with it, whatever the gap behind it"""
    lens = np.full(n, 8); lens[pos] = 120
    return _aln(lens, np.full(n - 1, 2))


_CASES = {}


def _cases():
    if not _CASES:
        named = [("n%d" % n, _uniform(n)) for n in (0, 1, 2, T - 1, T, T + 1, 3 * T)] + [("gaps", _gap_mix(3 * T))]
        named += [("alt%d" % p, _alt_at(p, 2 * T + 5)) for p in EDGES] + [("long%d" % p, _long_at(p, 2 * T + 5)) for p in EDGES]
        genome = synth.make_genome(T0 + 40 * T + 4000, seed=31)
        reads = []
        for _, b in named:
            end = int(b[-1, 0] + b[-1, 2]) if len(b) else 40
            reads.append(genome[T0:T0 + end + 10].copy())                    # 10 bases behind the last block: endAlign adds an end block too
        _CASES.update(names=[k for k, _ in named], blocks=[b for _, b in named], reads=reads, genome=genome)
    return _CASES


def _segments(b, read_len, chrom_len, end_align):
    """the grouping loop of IndelRefineAlignment on the augmented block list -> (the augmented list's length, [(startBlock, endBlock, a remainder survives)])"""
    b = [tuple(int(x) for x in r) for r in b]
    if len(b) <= 1:
        return len(b), []
    if end_align:
        m = min(b[0][0], b[0][1])
        if m < 40:
            b = [(b[0][0] - m, b[0][1] - m, m)] + b
        qe, te = b[-1][0] + b[-1][2], b[-1][1] + b[-1][2]
        m = min(read_len - qe, chrom_len - te)
        if m < 40:
            b = b + [(qe, te, m)]
    nB, max_gap, segs = len(b), K - 1, []
    s = e = 0
    while e < nB:
        q0, t0, l0 = b[s]
        qp, tp, tg, qg = q0 + l0, t0 + l0, 0, 0
        if e < nB - 1:
            tg, qg = b[e + 1][1] - tp, b[e + 1][0] - qp
        el = l0
        while e < nB - 1 and qg < max_gap and tg < max_gap and (s == e or el < 100):
            e += 1
            eq, et, el = b[e]
            qp, tp = eq + el, et + el
            if e + 1 < nB - 1:
                tg, qg = b[e + 1][1] - tp, b[e + 1][0] - qp
        alt = e != s and el > max_gap
        if e != s:
            segs.append((s, e, alt))
        if alt:
            b[e] = (b[e][0] + max_gap, b[e][1] + max_gap, el - max_gap)
        else:
            e += 1
        s = e
    return nB, segs


_EXPECTED = {}


def _expected(end_align):
    """the oracle's refined blocks, computed once and shared"""
    if end_align not in _EXPECTED:
        c = _cases(); g = c["genome"].tobytes()
        _EXPECTED[end_align] = [O.indel_refine(b, r.tobytes(), g, K, *PAR, end_align=end_align) for r, b in zip(c["reads"], c["blocks"])]
    return _EXPECTED[end_align]


def test_crafted_alignments_group_as_intended():
    c = _cases()
    assert all(st == 0 for ea in (False, True) for (_, st) in _expected(ea))
    by = dict(zip(c["names"], zip(c["blocks"], c["reads"])))
    assert T >= 64 and [len(by["n%d" % n][0]) for n in (0, 1, 2, T - 1, T, T + 1, 3 * T)] == [0, 1, 2, T - 1, T, T + 1, 3 * T]
    for end_align in (False, True):
        add = 1 if end_align else 0
        seg = lambda k: _segments(by[k][0], len(by[k][1]), len(c["genome"]), end_align)
        for n in (2, T - 1, T, T + 1, 3 * T):                                # one segment from the first block to the last, across every round
            nB, s = seg("n%d" % n)
            assert nB == n + 2 * add and s[0][:2] == (0, nB - 1)
        nB, s = seg("gaps")                                                  # gaps of K - 2 are crossed; K - 1 and K end a segment
        ends = {e - add for (_, e, _) in s}
        i = np.arange(3 * T - 1)
        assert set(i[(i % 7 == 4) | (i % 7 == 6)].tolist()) <= ends and not (set(i[i % 7 == 2].tolist()) & ends) and len(s) > T // 2
        for p in EDGES:
            nB, s = seg("alt%d" % p)                                         # ... ends at block p with a remainder, which passes through; the next one starts behind the gap
            assert (0, p + add, True) in s and s[1][0] == p + add + 1
            nB, s = seg("long%d" % p)                                        # ... ends with the long block p, the next one starts on its remainder
            assert s[0][:2] == (0, p + add) and s[1][0] == p + add and s[1][1] == nB - 1


@pytest.mark.gpu
@pytest.mark.parametrize("end_align", [False, True])
def test_hip_segments_across_tiles(ctx, end_align):
    from test_refine import _run_gpu
    c = _cases()
    (got, status), res = _run_gpu(ctx, c["genome"], c["reads"], c["blocks"], K, PAR, end_align)
    assert res.n_segments > T // 2
    for i, (exp, st) in enumerate(_expected(end_align)):
        assert st == 0 and status[i] == 0, (c["names"][i], st, status[i])
        assert np.array_equal(got[i], exp), (c["names"][i], len(got[i]), len(exp))
