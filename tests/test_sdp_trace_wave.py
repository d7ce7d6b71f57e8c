"""sdp_trace (sdp_trace.hip) as a wave per read: the walk on LDS for reads of up to TRACE_CAP anchors and from memory beyond, the wave-wide maximum (single mode),
the per-chain boxes, links and closing gather -- against the oracle, bit for bit, through the C entry points.  Reads of 0, 1, 2, 63, 64, 65, TRACE_CAP - 1,
TRACE_CAP, TRACE_CAP + 1 and 3 TRACE_CAP anchors in one batch (modes 0 and 1, and boxes); equal maxima (the first wins) and a read whose values are all 0;
NumAln 1 and 3; a candidate chain that runs into a used anchor and is rolled back; a chain that fails the 0.05 overlap test against chain 0.
test_crafted_reads_take_their_paths asserts on the CPU, from the oracle's values and chains, that every crafted read does what it was built for."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import sdp_inputs as S
from sdp_inputs import _compare, _run_hip

_SDP_H = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lra_amd", "csrc", "sdp.h")
CAP = int(re.search(r"constexpr int TRACE_CAP = (\d+);", open(_SDP_H).read()).group(1))      # the walk's LDS capacity, where the kernel defines it
SIZES = (0, 1, 2, 63, 64, 65, CAP - 1, CAP, CAP + 1, 3 * CAP)

_EMPTY = (np.array([0], np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.int32))
RATE = 5.0
# cluster mode: a gap cost under which ladders on one diagonal chain for nothing and clusters far from each other never chain (found by the oracle, asserted below)
KW0 = dict(alnthres=0.2, gapCeiling1=2 * 10 ** 9, gapCeiling2=2 ** 31 - 1, gapextend=100.0)
KW1 = dict(mode=1, NumAln=1)


def _line(n, **kw):
    return S.sdp_ladder(n, jitter=0, **kw) if n else _EMPTY


def _three_lines(total):
    """three clusters that do not chain with each other, `total` anchors in all: one candidate chain each"""
    return S.sdp_merge(_line(total - 1100, base=20000), _line(700, base=900000, q0=200000, strand=1), _line(400, base=1800000, q0=400000, strand=1))


def _y_read():
    """A: 25 anchors on one diagonal; B: 8 anchors that branch off A's 13th, 3 diagonals away: B's best chain runs down into A; C: 6 anchors far away"""
    i = np.arange(1, 9)
    return S.sdp_merge(_line(25, base=20000), S._one_cluster(12 * 37 + i * 37, 20000 + 12 * 37 + i * 37 + 3, 20, 0), _line(6, base=60000, q0=3000, strand=1))


def _overlap_read():
    """A: 25 anchors; D: 20 anchors at another q and A's t (a repeat): a chain of its own that lies within chain 0 on t; E: 6 anchors far away"""
    return S.sdp_merge(_line(25, base=20000), _line(20, base=20000, q0=4000), _line(6, base=60000, q0=8000, strand=1))


def _ties_read():
    """130 anchors none of which can follow another (t runs down as q runs up): 130 equal values; before them in the cluster's order, a shorter anchor of lower value"""
    i = np.arange(130)
    return S._one_cluster(np.concatenate([[0], 100 + i * 50]), np.concatenate([[30000], (130 - i) * 50]), np.concatenate([[5], np.full(130, 20)]), 0)


_READS = {}


def _reads(mode):
    """-> (reads, read lengths, rates, names)"""
    if mode not in _READS:
        if mode == 1:
            named = [("n%d" % n, S.sdp_ladder(n) if n else _EMPTY) for n in SIZES] + [("ties", _ties_read()), ("zero", S.sdp_ladder(70)), ("zero_big", S.sdp_ladder(CAP + 70))]
        else:
            named = [("n%d" % n, _line(n, base=20000)) for n in SIZES] + [("three%d" % n, _three_lines(n)) for n in (CAP - 1, CAP, CAP + 1)]
            named += [("y", _y_read()), ("overlap", _overlap_read()), ("zero", _line(70, base=20000))]
        names = [k for k, _ in named]; reads = [j for _, j in named]
        lens = [max(300, int(j[2].max()) + 1000) if len(j[2]) else 300 for j in reads]
        rates = np.array([0.0 if k.startswith("zero") else (RATE if mode == 0 else 20.0) for k in names], np.float32)
        _READS[mode] = (reads, lens, rates, names)
    return _READS[mode]


_ORACLE = {}


def _oracle(mode, num_aln):
    """the oracle's results, computed once and shared"""
    if (mode, num_aln) not in _ORACLE:
        reads, lens, rates, _ = _reads(mode)
        kw = KW1 if mode == 1 else dict(KW0, NumAln=num_aln)
        _ORACLE[(mode, num_aln)] = (kw, [O.sdp_chain(*job, O.sdp_opts(lens[r], **dict(kw, rate=float(rates[r])))) for r, job in enumerate(reads)])
    return _ORACLE[(mode, num_aln)]


def test_crafted_reads_take_their_paths():
    assert CAP % 64 == 0 and CAP > 130
    # single mode
    reads, lens, rates, names = _reads(1)
    _, exp = _oracle(1, 1)
    by = dict(zip(names, zip(reads, exp)))
    assert [len(j[2]) for j in reads[:len(SIZES)]] == list(SIZES)
    assert all(e["status"] >= 0 for e in exp)
    for n in SIZES[1:]:
        assert len(by["n%d" % n][1]["chains"]) == 1
    for n in SIZES[6:]:                                                      # walks of more than one round of 64 lanes, on either side of the capacity
        assert len(by["n%d" % n][1]["chains"][0]["frags"]) > 1000
    job, e = by["ties"]
    top = np.flatnonzero(e["val"] == e["val"].max())
    assert len(top) == 130 and top[0] > 0 and e["chains"][0]["frags"].tolist() == [int(top[0])]     # equal maxima in every lane's stride; the first one wins
    for k in ("zero", "zero_big"):
        job, e = by[k]
        assert e["val"].max() == 0.0 and e["chains"][0]["frags"].tolist() == [0] and e["chains"][0]["value"] == 0.0
    # cluster mode
    reads, lens, rates, names = _reads(0)
    for num_aln in (1, 3):
        kw, exp = _oracle(0, num_aln)
        by = dict(zip(names, zip(reads, exp)))
        assert [len(j[2]) for j in reads[:len(SIZES)]] == list(SIZES)
        assert all(e["status"] >= 0 for e in exp)
        for n in SIZES[3:]:
            assert [len(c["frags"]) for c in by["n%d" % n][1]["chains"]] == [n]
        for n in (CAP - 1, CAP, CAP + 1):                                    # three chains back to back in the read's range
            job, e = by["three%d" % n]
            assert len(job[2]) == n and [len(c["frags"]) for c in e["chains"]] == [n - 1100, 700, 400][:num_aln]
        assert len(by["zero"][1]["chains"]) == 0 and by["zero"][1]["val"].max() == 0.0
        if num_aln == 1:
            continue
        thres = lambda e: kw["alnthres"] * e["val"].max()
        # y: chain 0 is all of A; B's top comes next in value order, is worth more than every anchor outside chain 0 together -- so its trace runs into chain 0's
        # anchors and is rolled back, as are the rest of B; C is kept after them
        job, e = by["y"]
        A, B, Cc = range(0, 25), range(25, 33), range(33, 39)
        assert [sorted(c["frags"].tolist()) for c in e["chains"]] == [list(A), list(Cc)]
        vB, vC = e["val"][list(B)].max(), e["val"][list(Cc)].max()
        assert vB >= thres(e) and vB > vC >= thres(e) and vB > RATE * job[4][25:].sum()
        # overlap: D's top is next after chain 0 = A, and is worth exactly its own 20 anchors: its trace ends within D, the chain passes the length tests
        # (else the loop would end before E) and lies within chain 0 on t: not kept, its anchors stay used; E is kept
        job, e = by["overlap"]
        A, D, E = range(0, 25), range(25, 45), range(45, 51)
        assert [sorted(c["frags"].tolist()) for c in e["chains"]] == [list(A), list(E)]
        vD, vE = e["val"][list(D)].max(), e["val"][list(E)].max()
        assert vD == RATE * job[4][25:45].sum() and vD > vE >= thres(e)
        c0 = e["chains"][0]["box"]
        assert c0[2] <= job[3][25:45].min() < c0[3]


def _run_mode(ctx, mode, num_aln):
    reads, lens, rates, _ = _reads(mode)
    kw, exp = _oracle(mode, num_aln)
    res, out = _run_hip(ctx, reads, lens, kw, rates=rates)
    assert _compare(out, int(res.num_aln), reads, lens, kw, must_have_result=True, rates=rates, oracle_results=exp) == len(reads)
    return out


@pytest.mark.gpu
def test_hip_trace_single_mode(ctx):
    """mode 1: the read sizes around 64 and around TRACE_CAP in one batch, equal maxima, all-zero values (below and above TRACE_CAP)"""
    _run_mode(ctx, 1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("num_aln", [1, 3])
def test_hip_trace_cluster_mode(ctx, num_aln):
    """mode 0: the read sizes, three chains per read around TRACE_CAP, the rolled-back candidate, the chain that overlaps chain 0, all-zero values"""
    out = _run_mode(ctx, 0, num_aln)
    names = _reads(0)[3]
    assert int(out["n_chains"][names.index("y")]) == (2 if num_aln == 3 else 1)


# ---------------------------------------------------------------- boxes --------------------------------------------------
BOX_K = 17
BOX_KW = dict(rate=1.0, NumAln=3, alnthres=0.3, globalK=BOX_K)
BOX_SIZES = (0, 1, 2, 63, 64, 65, CAP - 1, CAP, CAP + 1, 2 * CAP + 7)


def _box_line(n, q0=0, t0=1000, val=50):
    i = np.arange(n, dtype=np.int64)
    return dict(qs=q0 + 100 * i, qe=q0 + 100 * i + 100, ts=t0 + 100 * i, te=t0 + 100 * i + 100, strand=np.zeros(n, np.int64), val=np.full(n, val, np.int64), num=1 + i % 7)


def _box_cat(*parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _box_y():
    """30 collinear boxes and 3 that branch off the 26th, 40 diagonals away"""
    b = _box_line(3, q0=2600, t0=1000 + 2600 + 40)
    return _box_cat(_box_line(30), b)


_BOXES = {}


def _box_reads():
    if not _BOXES:
        reads = [_box_line(n) for n in BOX_SIZES] + [_box_y()]
        lens = [max(300, int(b["qe"].max()) + 500) if len(b["qs"]) else 300 for b in reads]
        exp = [O.sdp_chain_boxes(b["qs"], b["qe"], b["ts"], b["te"], b["strand"], b["val"], b["num"], O.sdp_opts(lens[r], **BOX_KW)) if len(b["qs"]) else None
               for r, b in enumerate(reads)]
        _BOXES.update(reads=reads, lens=lens, exp=exp)
    return _BOXES["reads"], _BOXES["lens"], _BOXES["exp"]


def test_crafted_boxes_take_their_paths():
    reads, lens, exp = _box_reads()
    assert [len(b["qs"]) for b in reads[:-1]] == list(BOX_SIZES)
    assert all(e is None or e["status"] >= 0 for e in exp)
    for n, e in zip(BOX_SIZES[1:], exp[1:-1]):
        assert [len(c["frags"]) for c in e["chains"]] == [n] and e["chains"][0]["num_anchors"] == int(reads[BOX_SIZES.index(n)]["num"].sum())
    # the branch's top is a candidate (within 130 K of the best), worth more than the branch alone, and in no chain: its trace ran into chain 0 and was rolled back
    e = exp[-1]
    assert [sorted(c["frags"].tolist()) for c in e["chains"]] == [list(range(30))]
    best = e["val"].max(); vB = e["val"][30:].max()
    assert vB >= max(BOX_KW["alnthres"] * best, best - 130 * BOX_K) and vB > BOX_KW["rate"] * reads[-1]["val"][30:].sum()


@pytest.mark.gpu
def test_hip_trace_boxes(ctx):
    """the box driver (DecidePrimaryChains :1587): the read sizes in one batch and a rolled-back candidate; boxes, values and anchor counts are wave reductions"""
    import torch
    from lra_amd import chain
    reads, lens, exp = _box_reads()
    dev = ctx.device
    off = np.concatenate([[0], np.cumsum([len(b["qs"]) for b in reads])]).astype(np.int64)
    cat = lambda k: torch.tensor(np.concatenate([b[k] for b in reads]).astype(np.int32), device=dev)
    roff = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), device=dev)
    res = chain.sparse_dp_boxes_batch(ctx, len(reads), torch.tensor(off, device=dev), cat("qs"), cat("qe"), cat("ts"), cat("te"), cat("strand"), cat("val"), cat("num"), roff,
                                      chain.sdp_opts(**BOX_KW))
    co = chain.fetch(ctx, res)
    na = int(res.num_aln)
    for r, e in enumerate(exp):
        if e is None:
            assert co["n_chains"][r] == 0
            continue
        assert co["status"][r] == 0, (r, co["status"][r])
        f0, f1 = int(co["frag_off"][r]), int(co["frag_off"][r + 1])
        assert f1 - f0 == len(reads[r]["qs"])
        assert np.array_equal(co["frag_val"][f0:f1].view(np.uint32), e["val"].view(np.uint32)), r
        assert int(co["n_chains"][r]) == len(e["chains"]), (r, co["n_chains"][r], len(e["chains"]))
        for c, ch in enumerate(e["chains"]):
            s = r * na + c
            a = int(co["chain_start"][s]); ln = int(co["chain_len"][s])
            assert ln == len(ch["frags"]), (r, c)
            assert np.array_equal(co["chain_cluster"][a:a + ln], ch["frags"]), (r, c)
            assert np.array_equal(co["chain_link"][a:a + ln - 1], ch["link"]), (r, c)
            assert np.array_equal(co["chain_box"][s], ch["box"]), (r, c)
            assert np.float32(co["chain_value"][s]).view(np.uint32) == np.float32(ch["value"]).view(np.uint32)
            assert int(co["chain_num_anchors"][s]) == ch["num_anchors"]
            assert np.array_equal(co["chain_q"][a:a + ln], reads[r]["qs"][ch["frags"]].astype(np.uint32)), (r, c)
            assert np.array_equal(co["chain_t"][a:a + ln], reads[r]["ts"][ch["frags"]].astype(np.uint32)), (r, c)
            assert np.array_equal(co["chain_alen"][a:a + ln], reads[r]["val"][ch["frags"]].astype(np.int32)), (r, c)
