"""The sparse DP's visit records as planes (sdp.h, ReadArena: one plane of P records per (family pair, level) a read can have, the row family's planes first): reads whose
two families differ in depth, reads on every side of a power of two of distinct rows / columns (a family of n lines has ceil(log2 n) + 1 levels), those small reads
between two long ones in one batch (per-read plane offsets; one read's clear must leave its neighbours alone), and a lattice whose points overstate its lines.  Through the
wave-per-read kernels (planes bounded from the points, or from the count pass's rows / columns: LRA_SDP_ONEPASS=0), the workgroup kernels (rows / columns from k_big_lines)
and the box driver, against the oracle bit for bit.  A plane too few makes sdp_build flag the read (LRA_ST_RANGE): _compare fails on any status.  Every GPU test first
asserts on the CPU (sdp_inputs.sdp_case_shape) that its reads have the shape they were built for; test_plane_cases_have_their_shapes does that part without a GPU."""
import numpy as np
import pytest

import oracle_lib as O
import sdp_inputs as S
from sdp_inputs import _compare, _one_cluster, _run_hip, sdp_case_shape, sdp_ladder, sdp_lattice

WAVE, WG = "100000", "40"                                                   # LRA_SDP_BIG_POINTS: every read a wave job / every read of 40 points and more a workgroup job
LINES = (1, 2, 3, 4, 5, 8, 9)                                               # distinct rows = distinct columns of the boundary reads
DEPTH = (1, 2, 3, 3, 4, 4, 5)                                               # ceil(log2 n) + 1


def depth(n):
    """levels of a decomposition over n distinct lines (vis_planes, sdp.h)"""
    return 1 if n <= 1 else int(n - 1).bit_length() + 1


def _mode_kw(mode):
    return dict(mode=1, NumAln=1) if mode == 1 else dict()


def _lens(reads):
    return [max(300, int(q.max()) + 1000) if len(q) else 300 for (_, _, q, _, _) in reads]


# ---------------------------------------------------------------- the crafted reads --------------------------------------
def _chain_of(n, strand, length=20, q0=100, t0=7000):
    """A read with exactly n distinct rows and n distinct columns: n - 1 anchors of one length head to tail (a corner of one is the next one's), on the reverse strand t
    running down; n = 1 is one anchor of length 0, whose two points are one."""
    if n == 1:
        return _one_cluster([q0], [t0], 0, strand)
    i = np.arange(n - 1, dtype=np.int64)
    return _one_cluster(q0 + i * length, t0 + (i if strand == 0 else n - 2 - i) * length, length, strand)


def _three_by_two_hundred(transpose, strand, length=30):
    """100 anchors of one length that start on two rows a length apart -- 3 distinct rows -- with 200 distinct columns (or the transpose)"""
    i = np.arange(100, dtype=np.int64)
    a = 500 + (i & 1) * length                                               # rows 500, 530, 560
    b = 5000 + i * (2 * length + 1)                                          # b and b + length never meet
    return _one_cluster(b, a, length, strand) if transpose else _one_cluster(a, b, length, strand)


_EMPTY = (np.array([0], np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.int32))


def _unequal(mode):
    reads = [_three_by_two_hundred(tr, st) for tr in (False, True) for st in (0, 1)]
    want = [dict(rows=200 if tr else 3, cols=3 if tr else 200) for tr in (False, True) for st in (0, 1)]
    return reads, want


def _boundaries(mode):
    reads = [_chain_of(n, strand=k & 1) for k, n in enumerate(LINES)] + [_EMPTY]
    want = [dict(rows=n, cols=n) for n in LINES] + [dict(points=0, rows=0, cols=0)]
    return reads, want


def _mixed(mode):
    small, want = _boundaries(mode)
    extra = 0 if mode == 1 else 4
    reads = [sdp_ladder(300)] + small + [sdp_ladder(2000, strand=1)]
    want = [dict(points=600 + extra, rows=600, cols=600)] + want + [dict(points=4000 + extra, rows=4000, cols=4000)]
    return reads, want


def _lattice(mode):
    return [sdp_lattice(256, seed=11)], [dict(points=512 + (0 if mode == 1 else 4))]


_BUILDERS = dict(unequal=_unequal, boundaries=_boundaries, mixed=_mixed, lattice=_lattice)
_CASES, _ORACLE = {}, {}


def _case(name, mode):
    if (name, mode) not in _CASES:
        reads, want = _BUILDERS[name](mode)
        _CASES[(name, mode)] = (reads, _lens(reads), want)
    return _CASES[(name, mode)]


def _oracle(name, mode):
    """the oracle's results of a case: computed once, shared by the tests that compare with them, never changed"""
    if (name, mode) not in _ORACLE:
        reads, lens, _ = _case(name, mode)
        _ORACLE[(name, mode)] = [O.sdp_chain(*job, O.sdp_opts(lens[r], **_mode_kw(mode))) for r, job in enumerate(reads)]
    return _ORACLE[(name, mode)]


def _assert_shapes(name, mode):
    reads, lens, want = _case(name, mode)
    assert len(reads) == len(want)
    shapes = [sdp_case_shape(job, mode) for job in reads]
    for i, (got, w) in enumerate(zip(shapes, want)):
        for k, v in w.items():
            assert got[k] == v, (name, mode, i, k, got[k], v)
    if name == "unequal":                                                    # the row family 3 planes and the column family 9, or the other way round
        assert [(depth(s["rows"]), depth(s["cols"])) for s in shapes] == [(3, 9), (3, 9), (9, 3), (9, 3)]
    if name in ("boundaries", "mixed"):
        small = shapes[:len(LINES)] if name == "boundaries" else shapes[1:1 + len(LINES)]
        assert tuple(depth(s["rows"]) for s in small) == DEPTH and tuple(depth(s["cols"]) for s in small) == DEPTH
        assert [s["points"] for s in small][:2] == [2 if mode == 1 else 4, 2 if mode == 1 else 4]   # the length-0 anchor and the one-anchor read
    if name == "lattice":                                                    # planes bounded from the points exceed the planes the read's lines use
        s = shapes[0]
        assert depth(s["points"]) > max(depth(s["rows"]), depth(s["cols"])) and min(s["rows"], s["cols"]) > 1
    return reads, lens


def _run_and_compare(ctx, name, mode):
    reads, lens = _assert_shapes(name, mode)
    kw = _mode_kw(mode)
    res, out = _run_hip(ctx, reads, lens, kw)
    assert _compare(out, int(res.num_aln), reads, lens, kw, must_have_result=True, oracle_results=_oracle(name, mode)) == len(reads)


def _set_run(monkeypatch, run):
    monkeypatch.setenv("LRA_SDP_BIG_POINTS", WG if run == "workgroup" else WAVE)
    if run == "counted":
        monkeypatch.setenv("LRA_SDP_ONEPASS", "0")


def test_plane_cases_have_their_shapes():
    assert tuple(depth(n) for n in LINES) == DEPTH and depth(0) == 1 and depth(131072) == 18 and depth(131073) == 19
    for mode in (0, 1):
        for name in _BUILDERS:
            _assert_shapes(name, mode)
            assert all(e["status"] >= 0 for e in _oracle(name, mode)), (name, mode)


RUNS = ["wave", "counted", "workgroup"]                                      # planes from the points; from the count pass's lines; from k_big_lines (NW = 16 build, sdp_process_wg)


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("mode", [0, 1], ids=["clusters", "single"])
def test_hip_sdp_families_of_unequal_depth(ctx, mode, run, monkeypatch):
    """3 distinct rows x 200 distinct columns and the transpose, on either strand: where the lines are counted the row family has 3 planes and the column family 9"""
    _set_run(monkeypatch, run)
    _run_and_compare(ctx, "unequal", mode)


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("mode", [0, 1], ids=["clusters", "single"])
def test_hip_sdp_plane_count_boundaries(ctx, mode, run, monkeypatch):
    """1, 2, 3, 4, 5, 8, 9 distinct rows and columns (depth 1, 2, 3, 3, 4, 4, 5), a one-anchor read and an empty read among them.  (None of them reaches 40 points:
    they are wave jobs in every run -- planes from the points, or from the count pass's rows and columns; the workgroup kernels meet them in the mixed batch's launch)"""
    _set_run(monkeypatch, run)
    _run_and_compare(ctx, "boundaries", mode)


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("mode", [0, 1], ids=["clusters", "single"])
def test_hip_sdp_mixed_batch(ctx, mode, run, monkeypatch):
    """the small reads between ladders of 300 and 2000 anchors: every read's planes at its own offset, sized for itself"""
    _set_run(monkeypatch, run)
    _run_and_compare(ctx, "mixed", mode)


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("mode", [0, 1], ids=["clusters", "single"])
def test_hip_sdp_lattice_with_heavy_ties(ctx, mode, run, monkeypatch):
    """a lattice of 256 anchors: far fewer distinct rows and columns than points"""
    _set_run(monkeypatch, run)
    _run_and_compare(ctx, "lattice", mode)


# ---------------------------------------------------------------- the box driver -----------------------------------------
BOX_KW = dict(rate=1.0, NumAln=3, alnthres=0.3, globalK=17)
BOX_SIZES = (0, 1, 2, 4, 5, 300)                                             # boxes in a line, apart from each other: 2 n distinct rows and columns


def _box_line(n):
    i = np.arange(n, dtype=np.int64)
    return dict(qs=150 * i, qe=150 * i + 100, ts=1000 + 150 * i, te=1000 + 150 * i + 100, strand=np.zeros(n, np.int64), val=np.full(n, 50, np.int64), num=1 + i % 7)


_BOXES = {}


def _box_reads():
    if not _BOXES:
        reads = [_box_line(n) for n in BOX_SIZES]
        lens = [max(300, int(b["qe"].max()) + 500) if len(b["qs"]) else 300 for b in reads]
        exp = [O.sdp_chain_boxes(b["qs"], b["qe"], b["ts"], b["te"], b["strand"], b["val"], b["num"], O.sdp_opts(lens[r], **BOX_KW)) if len(b["qs"]) else None
               for r, b in enumerate(reads)]
        _BOXES.update(reads=reads, lens=lens, exp=exp)
    return _BOXES["reads"], _BOXES["lens"], _BOXES["exp"]


def _assert_box_shapes():
    """the points of a box are (qs + 1, ts + 1), (qe - 1, te - 1), (qs + 1, te - 1), (qe - 1, ts + 1) (k_points): rows and columns 2, 4, 8, 10, 600 -- depth 2, 3, 4, 5, 11"""
    reads, lens, exp = _box_reads()
    rows = [len(np.unique(np.concatenate([b["qs"] + 1, b["qe"] - 1]))) for b in reads]
    cols = [len(np.unique(np.concatenate([b["ts"] + 1, b["te"] - 1]))) for b in reads]
    assert rows == cols == [2 * n for n in BOX_SIZES]
    assert [depth(n) for n in rows[1:]] == [2, 3, 4, 5, 11]
    assert all(e is None or e["status"] >= 0 for e in exp)
    return reads, lens, exp


def test_plane_boxes_have_their_shapes():
    _assert_box_shapes()


@pytest.mark.gpu
@pytest.mark.parametrize("run", ["wave", "workgroup"])
def test_hip_sdp_boxes_plane_counts(ctx, run, monkeypatch):
    """the box driver over reads of 0 .. 300 boxes in one batch (4 points a box)"""
    import torch
    from lra_amd import chain
    _set_run(monkeypatch, run)
    reads, lens, exp = _assert_box_shapes()
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
