"""The first sparse DP (SDP#A: sdp_points / sdp_build / sdp_process / sdp_process_wg / sdp_trace.hip) at the hard boundaries of its code, on crafted reads against the
oracle, bit for bit: the build variants of small_builds by point count, the SPW = 2 / 3 cut and the LV = 18 level limit, the gap-cost table's ends (PEN_TAB_WAVE,
PEN_TAB_WG) and the option sets that drop the table, coordinates and diagonals beyond 2^31, the span at which sdp_process_wg leaves its LDS window, per-read rates and
the NumAln limits.  Every GPU test first asserts on the CPU that its reads have the shape they were built for (sdp_inputs.sdp_case_shape), so a case that drifts off
its boundary fails instead of passing beside it; test_crafted_cases_have_their_shapes_and_an_oracle_result does that part without a GPU."""
import numpy as np
import pytest

import oracle_lib as O
import sdp_inputs as S
from sdp_inputs import _MIX_OPTS, _compare, _random_read_mix, _run_hip

ST_RANGE = 4                                                                # LRA_ST_RANGE (include/lra_hip.h)
WAVE, WG = "100000", "40"                                                   # LRA_SDP_BIG_POINTS: every test read a wave job / every read of 40 points and more a workgroup job


def _mode_kw(mode, **kw):
    return dict(kw, mode=1, NumAln=1) if mode == 1 else dict(kw)


# ---------------------------------------------------------------- the crafted reads (deterministic; built once) ---------
_CASES = {}


def _case(name, mode):
    """-> (reads, read_lens, want): want[i] = the shape read i was built for (a subset of sdp_case_shape's keys)"""
    key = (name, mode)
    if key not in _CASES:
        reads, want = _BUILDERS[name](mode)
        lens = [max(300, int(q.max()) + 1000) if len(q) else 300 for (_, _, q, _, _) in reads]
        _CASES[key] = (reads, lens, want)
    return _CASES[key]


def _assert_shapes(name, mode):
    reads, lens, want = _case(name, mode)
    assert len(reads) == len(want)
    for i, (job, w) in enumerate(zip(reads, want)):
        got = S.sdp_case_shape(job, mode)
        for k, v in w.items():
            assert got[k] == v, (name, mode, i, k, got[k], v)
    return reads, lens


def _build_classes(mode):
    """A read on every cut of small_builds and two points above it: LDS arrays for <= 128 / 256 / 512 points, 16-bit indices in the arena below 16384 points, the wide
    build from 16384 (single mode only); and lattices with heavy ties at 128, 256 and 512 points.  Forward and reverse ladders alternate."""
    ns = (64, 65, 128, 129, 256, 257, 8191, 8192, 8193) if mode == 1 else (62, 63, 126, 127, 254, 255)
    extra = 0 if mode == 1 else 4
    reads = [S.sdp_ladder(n, strand=i & 1) for i, n in enumerate(ns)]
    want = [dict(points=2 * n + extra, rows=2 * n, cols=2 * n) for n in ns]
    for k, n in enumerate((64, 128, 256) if mode == 1 else (62, 126, 254)):
        reads.append(S.sdp_lattice(n, seed=3 + k, strand=k & 1)); want.append(dict(points=2 * n + extra))
    assert sorted(w["points"] for w in want)[:8] == [128, 128, 130, 256, 256, 258, 512, 512]
    return reads, want


def _lines(n):
    return lambda mode: ([S.sdp_ladder(n)], [dict(points=2 * n + (0 if mode == 1 else 4), rows=2 * n, cols=2 * n)])


def _range_batch(mode):
    """two ordinary reads, then one with 131074 distinct rows and columns: one level more than LV = 18 holds"""
    n = 65537
    reads = [S.sdp_ladder(300, strand=1), S.sdp_lattice(200, seed=9), S.sdp_ladder(n)]
    return reads, [dict(rows=600), dict(), dict(rows=2 * n, cols=2 * n)]


_TAB_D = (2046, 2047, 2048, 2049, 4094, 4095, 4096, 4097)                   # around PEN_TAB_WAVE = 2048 and PEN_TAB_WG = 4096 (the table serves distances below them)


def _table_edges(mode):
    """Neighbouring anchors on diagonals exactly d apart for every d of _TAB_D, with both signs, on either strand (reverse: the diagonal is t + q).  400-base anchors
    4700 bases apart: a link across the widest gap costs less than the anchor it reaches is worth, so the chain takes every one of them."""
    steps = []
    for d in _TAB_D:
        steps += [d, -d]
    steps += [-s for s in steps]
    return [S.sdp_diag_steps(steps, strand=s, length=400, advance=4700) for s in (0, 1)], [dict(points=66 + (0 if mode == 1 else 4))] * 2


def _far(strand_a, strand_b):
    a = S.sdp_ladder(40, base=1000, strand=strand_a, length=30)
    b = S.sdp_ladder(60, base=4100000000, strand=strand_b, q0=40 * 37 + 100, length=30)
    return S.sdp_merge(a, b)


def _big_coords(mode):
    """ladders whose t straddles 2^31 and lies at 4.2e9, forward and reverse; reads of two clusters, one at t ~ 1000 and one at t ~ 4.1e9: diagonals more than 2^31 apart"""
    reads = [S.sdp_ladder(300, base=2147483000), S.sdp_ladder(300, base=2147483000, strand=1), S.sdp_ladder(300, base=4200000000),
             S.sdp_ladder(300, base=4200000000, strand=1), _far(0, 0), _far(1, 1), _far(0, 1)]
    for job in reads[:2]:
        assert job[3].min() < 2 ** 31 < job[3].max()
    for job in reads[4:]:
        assert job[3].min() < 2000 and job[3].max() > 2 ** 32 - 2 * 10 ** 8
    return reads, [dict(rows=600, cols=600)] * 4 + [dict(rows=200, cols=200)] * 3


def _no_table(mode):
    reads, want = _big_coords(mode)
    return [S.sdp_ladder(300), S.sdp_ladder(300, strand=1)] + reads[4:], [dict(rows=600, cols=600)] * 2 + want[4:]


def _overlap(n, length, jitter, mod):
    """anchors one base apart on (nearly) one diagonal, each `length` long: ~2 length points between an anchor's start point and its end point"""
    i = np.arange(n, dtype=np.int64)
    return S._one_cluster(i, i + 7000 + (i % mod) * jitter, length, 0)


def _window_span(mode):
    """3100 anchors (the window's 2048 entries come round a second time) with the longest span the LDS window of sdp_process_wg serves, 991 points
    (span + RING_LEAD + RING_CHECK + 1 <= RING_W), and the shortest one that goes to the words at L2, 992.  The first and last anchor's second pair (cluster mode) and the
    parity of the jitter decide the last point: the variants below were found by computing the span."""
    if mode == 1:
        reads = [_overlap(3100, 496, 0, 3), _overlap(3100, 496, 50, 3)]
    else:
        reads = [_overlap(3100, 495, 50, 2), _overlap(3100, 496, 50, 2)]
    return reads, [dict(span=991), dict(span=992)]


def _disjoint(K, n, rev_every):
    parts = []
    for k in range(K):
        strand = 1 if k % rev_every == 0 else 0
        parts.append(S.sdp_ladder(n + k, q0=k * 2000, base=(K - k) * 5000 if strand == 0 else (k + 1) * 5000, strand=strand))
    return S.sdp_merge(*parts)


def _many_clusters(mode):
    return [_disjoint(30, 6, 2), _disjoint(17, 9, 2), _disjoint(10, 12, 3)], [dict(), dict(), dict()]


_BUILDERS = dict(build_classes=_build_classes, lines_32768=_lines(16384), lines_32770=_lines(16385), lines_131072=_lines(65536), range_batch=_range_batch,
                 table_edges=_table_edges, big_coords=_big_coords, no_table=_no_table, window_span=_window_span, many_clusters=_many_clusters)

# the gap cost's option sets: the table kept with penalties that differ across its ends; the table dropped (a penalty above 16 bits); penalties above 2e9 (the
# long long path of pwl_w); no gap cost at all; and links across 2^31 that are cheap enough to be taken, with ceilings that do not clamp them (the last segment's slope)
_TABLE_OPTS = dict(default={}, high_ceilings=dict(gapCeiling1=20000, gapCeiling2=30000))
_NO_TABLE_OPTS = dict(no_table=dict(gapextend=2000.0, gapCeiling1=10 ** 6, gapCeiling2=2 * 10 ** 6), above_2e9=dict(gapextend=1e7, gapCeiling1=2 * 10 ** 9, gapCeiling2=2 ** 31 - 1),
                      free=dict(gapopen=0.0, gapextend=0.0), cheap_far_links=dict(gapopen=0.0, gapextend=0.0001, gapCeiling1=2 * 10 ** 9, gapCeiling2=2 ** 31 - 1))
_COORD_OPTS = dict(default={}, three_chains=dict(NumAln=3, alnthres=0.3))
_MANY_OPTS = dict(all_chains=dict(NumAln=16, alnthres=0.0), tenth=dict(NumAln=16, alnthres=0.1))

_ORACLE = {}


def _oracle(name, mode, kw, rates=None):
    """the oracle's results for a case's reads under kw: computed once, shared by the tests (and parameters) that compare with them, never changed"""
    key = (name, mode, tuple(sorted(kw.items())), None if rates is None else tuple(float(x) for x in rates))
    if key not in _ORACLE:
        reads, lens, _ = _case(name, mode)
        _ORACLE[key] = [O.sdp_chain(*job, O.sdp_opts(lens[r], **(kw if rates is None else dict(kw, rate=float(rates[r]))))) for r, job in enumerate(reads)]
    return _ORACLE[key]


def _chain_links(job, exp):
    """|difference of the diagonals| of every two anchors a chain of the oracle links"""
    offs, st, q, t, ln = job
    q = q.astype(np.int64); t = t.astype(np.int64)
    out = set()
    for ch in exp["chains"]:
        f = ch["frags"]; cl = np.searchsorted(offs, f, side="right") - 1
        out |= set(np.abs(np.diff(np.where(st[cl] == 0, t[f] - q[f], t[f] + q[f]))).tolist())
    return out


def _check_table_edges(mode, kw):
    reads, lens = _assert_shapes("table_edges", mode)
    exp = _oracle("table_edges", mode, kw)
    for job, e in zip(reads, exp):
        offs, st, q, t, ln = job
        o = np.argsort(q)
        dg = t[o].astype(np.int64) - q[o] if st[0] == 0 else t[o].astype(np.int64) + q[o]
        assert set(_TAB_D) <= set(np.abs(np.diff(dg)).tolist()) and (np.diff(dg) > 0).any() and (np.diff(dg) < 0).any()
        assert e["status"] >= 1 and set(_TAB_D) <= _chain_links(job, e)      # the comparison means something only where a chain crosses each distance
    return reads, lens, exp


def _penalties(kw, xs):
    """-w of the oracle's gap cost at the distances xs - 1 (the table's entry d is the penalty at x = d + 1)"""
    d = dict(O.SDP_ONT); d.update(kw)
    w = O.sdp_pwl((d["gapopen"], d["gapextend"], d["gaproot"], d["gapCeiling1"], d["gapCeiling2"]), xs)[1].view(np.float32)
    return -w.astype(np.float64)


def _rates(n):
    """distinct per read, from 1.0 to 20.0 (both ends included), in no order"""
    return (1.0 + 19.0 * ((np.arange(n) * 7) % n) / (n - 1)).astype(np.float32)


def test_crafted_cases_have_their_shapes_and_an_oracle_result():
    """Everything the GPU tests below assume of their inputs, without a GPU: the shapes, an oracle result (status >= 0) for every read under every option set, chains
    that cross every table-edge distance, far links that are taken, more than two chains under NumAln = 16."""
    n_reads = 0
    for mode in (0, 1):
        for name, optsets in (("build_classes", {"": {}}), ("lines_32768", {"": {}}), ("lines_32770", {"": {}}), ("lines_131072", {"": {}}), ("window_span", {"": {}}),
                              ("big_coords", _COORD_OPTS if mode == 0 else {"": {}}), ("no_table", _NO_TABLE_OPTS), ("many_clusters", _MANY_OPTS if mode == 0 else {})):
            for kw in optsets.values():
                _assert_shapes(name, mode)
                exp = _oracle(name, mode, _mode_kw(mode, **kw))
                assert all(e["status"] >= 0 for e in exp), (name, mode, kw)
                n_reads += len(exp)
        for kw in _TABLE_OPTS.values():
            _check_table_edges(mode, _mode_kw(mode, **kw))
        reads, lens = _assert_shapes("range_batch", mode)                    # (the oracle has no level limit; the device flags the third read)
        assert all(e["status"] >= 0 for e in _oracle("range_batch", mode, _mode_kw(mode))[:2])
    assert n_reads > 80
    # a chain of the oracle links the cluster at t ~ 1000 with the one at t ~ 4.1e9 -- under the default options, and under the ones made for it
    for name, kw, r in (("big_coords", {}, 4), ("big_coords", {}, 6), ("no_table", _NO_TABLE_OPTS["cheap_far_links"], 2), ("no_table", _NO_TABLE_OPTS["free"], 2)):
        job = _case(name, 0)[0][r]
        ch = _oracle(name, 0, kw)[r]["chains"][0]
        assert len(set((np.searchsorted(job[0], ch["frags"], side="right") - 1).tolist())) == 2, (name, kw, r)
    # which option sets keep the 16-bit table (pwl_table, k_pen_table), where the penalties pass 2e9, and that the cheap far link is not clamped
    tab_x = np.arange(1, 4097)
    for kw, kept in ((_TABLE_OPTS["default"], True), (_TABLE_OPTS["high_ceilings"], True), (_NO_TABLE_OPTS["no_table"], False), (_NO_TABLE_OPTS["above_2e9"], False),
                     (_NO_TABLE_OPTS["free"], True), (_NO_TABLE_OPTS["cheap_far_links"], True)):
        assert (_penalties(kw, tab_x).max() <= 32767) == kept, kw
    hi = _penalties(_TABLE_OPTS["high_ceilings"], np.array(_TAB_D) + 1)
    assert len(set(hi.tolist())) > 4 and hi.max() < 20000                    # distinct, unclamped penalties across the table's ends
    far_x = np.array([4100000000])
    assert _penalties(_NO_TABLE_OPTS["above_2e9"], np.array([5000, 100000])).min() >= 2e9 and 0 < _penalties(_NO_TABLE_OPTS["cheap_far_links"], far_x)[0] < 2e9
    assert [len(e["chains"]) for e in _oracle("many_clusters", 0, _MANY_OPTS["all_chains"])] == [16, 16, 5]
    assert [len(e["chains"]) for e in _oracle("many_clusters", 0, _MANY_OPTS["tenth"])] == [3, 16, 5]
    mix, mix_lens = _random_read_mix()
    rates = _rates(len(mix))
    assert len(set(rates.tolist())) == len(mix) and rates.min() == 1.0 and rates.max() == 20.0
    for kw in _MIX_OPTS:
        assert all(O.sdp_chain(*job, O.sdp_opts(mix_lens[r], **dict(kw, rate=float(rates[r]))))["status"] >= 0 for r, job in enumerate(mix))


def _run_and_compare(ctx, name, mode, kw, rates=None):
    reads, lens = _assert_shapes(name, mode)
    res, out = _run_hip(ctx, reads, lens, kw, rates=rates)
    assert _compare(out, int(res.num_aln), reads, lens, kw, must_have_result=True, oracle_results=_oracle(name, mode, kw, rates)) == len(reads)
    return out


# ---------------------------------------------------------------- GPU ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("run", ["estimated", "counted", "outgrown", "workgroup"])
@pytest.mark.parametrize("mode", [0, 1], ids=["clusters", "single"])
def test_hip_sdp_build_classes(ctx, mode, run, monkeypatch):
    """1. Every variant of small_builds in one launch, each with a read on its cut and one two points above it: sized from the estimate, from the count pass
    (LRA_SDP_ONEPASS=0: the count-pass variants take the same cuts) and from estimates that the reads outgrow (attempt 1 crosses the cuts again); the reads of 16384 and
    16386 points stay wave jobs (the threshold is raised above them), so sdp_build<EMIT, 1, 0> runs.  `workgroup`: the same reads through the 1024-thread build."""
    monkeypatch.setenv("LRA_SDP_BIG_POINTS", WG if run == "workgroup" else WAVE)
    if run == "counted":
        monkeypatch.setenv("LRA_SDP_ONEPASS", "0")
    if run == "outgrown":
        monkeypatch.setenv("LRA_SDP_ESTIMATE", "2.0,0.5")
    _run_and_compare(ctx, "build_classes", mode, _mode_kw(mode))


@pytest.mark.gpu
@pytest.mark.parametrize("window", ["window", "l2"])
@pytest.mark.parametrize("mode", [0, 1], ids=["clusters", "single"])
def test_hip_sdp_workgroup_slots_per_wave(ctx, mode, window, monkeypatch):
    """2. launch_process_wg takes SPW = 2 up to 32768 distinct rows and columns and SPW = 3 beyond: a read with exactly 32768 of both and one with 32770, each in a call
    of its own (the launch's largest read decides)."""
    monkeypatch.delenv("LRA_SDP_BIG_POINTS", raising=False)                  # (the default thresholds make reads of 32768 points workgroup jobs)
    if window == "l2":
        monkeypatch.setenv("LRA_SDP_WG_RING", "0")
    for name in ("lines_32768", "lines_32770"):
        _run_and_compare(ctx, name, mode, _mode_kw(mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["clusters", "single"])
def test_hip_sdp_all_eighteen_levels(ctx, mode, monkeypatch):
    """2. 131072 distinct rows and columns = 2^(LV-1): the decompositions use all 18 levels, the result is the oracle's."""
    monkeypatch.delenv("LRA_SDP_BIG_POINTS", raising=False)
    _run_and_compare(ctx, "lines_131072", mode, _mode_kw(mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["clusters", "single"])
def test_hip_sdp_range_flag_beside_ordinary_reads(ctx, mode, monkeypatch):
    """2. 131074 rows: sdp_build gives the read up with LRA_ST_RANGE (its levels 0 .. 17 are complete and nothing refers to a level beyond: ProcessPoint walks built
    sub-problems only, the trace skips the read); it has that bit alone and no chain, and the two ordinary reads of the batch have the oracle's result."""
    monkeypatch.delenv("LRA_SDP_BIG_POINTS", raising=False)
    kw = _mode_kw(mode)
    reads, lens = _assert_shapes("range_batch", mode)
    res, out = _run_hip(ctx, reads, lens, kw)
    assert int(out["status"][2]) == ST_RANGE and int(out["n_chains"][2]) == 0
    assert _compare(out, int(res.num_aln), reads[:2], lens[:2], kw, must_have_result=True, oracle_results=_oracle("range_batch", mode, kw)[:2]) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("opts", sorted(_TABLE_OPTS))
@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
@pytest.mark.parametrize("mode", [0, 1], ids=["clusters", "single"])
def test_hip_sdp_gap_table_edges(ctx, mode, kernel, opts, monkeypatch):
    """3. Diagonal differences of 2046 .. 2049 and 4094 .. 4097 between neighbouring anchors of a chain: the last entries of the wave kernel's and the workgroup kernel's
    table and the first distances that go to pwl_w, with penalties clamped (default) and distinct (high ceilings) across the ends."""
    monkeypatch.setenv("LRA_SDP_BIG_POINTS", WG if kernel == "workgroup" else WAVE)
    kw = _mode_kw(mode, **_TABLE_OPTS[opts])
    reads, lens, exp = _check_table_edges(mode, kw)
    res, out = _run_hip(ctx, reads, lens, kw)
    assert _compare(out, int(res.num_aln), reads, lens, kw, must_have_result=True, oracle_results=exp) == len(reads)


@pytest.mark.gpu
@pytest.mark.parametrize("opts", sorted(_NO_TABLE_OPTS))
@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
@pytest.mark.parametrize("mode", [0, 1], ids=["clusters", "single"])
def test_hip_sdp_without_table_and_large_penalties(ctx, mode, kernel, opts, monkeypatch):
    """4. pwl_w by itself (pwl_table drops the table when a penalty does not fit 16 bits), its long long path (penalties above 2e9), the clamps with large ceilings, no
    gap cost at all, and its branch for distances above 2^31 - 1 with a slope that decides the chain: ladders and the reads with clusters 4.1e9 apart."""
    monkeypatch.setenv("LRA_SDP_BIG_POINTS", WG if kernel == "workgroup" else WAVE)
    _run_and_compare(ctx, "no_table", mode, _mode_kw(mode, **_NO_TABLE_OPTS[opts]))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
@pytest.mark.parametrize("mode,opts", [(0, "default"), (0, "three_chains"), (1, "default")], ids=["clusters", "clusters-three_chains", "single"])
def test_hip_sdp_coordinates_beyond_2_31(ctx, mode, opts, kernel, monkeypatch):
    """5. t across 2^31 and at 4.2e9 (the keys q << 33 | t << 1, t << 31 | q << 1 and the + 2^32 diagonal key of k_points / k_gather, the build's 32-bit diagonals,
    ProcessPoint's 64-bit ones, the chain boxes), and clusters whose diagonals are more than 2^31 apart."""
    monkeypatch.setenv("LRA_SDP_BIG_POINTS", WG if kernel == "workgroup" else WAVE)
    out = _run_and_compare(ctx, "big_coords", mode, _mode_kw(mode, **_COORD_OPTS[opts]))
    if mode == 0:                                                            # (the single-cluster driver leaves the boxes at zero, as the oracle does)
        assert int(out["chain_box"][:, 3].max()) > 2 ** 32 - 10 ** 8          # a box's tEnd arrives as the unsigned number it is


@pytest.mark.gpu
@pytest.mark.parametrize("window", ["window", "l2"])
@pytest.mark.parametrize("mode", [0, 1], ids=["clusters", "single"])
def test_hip_sdp_window_span_limit(ctx, mode, window, monkeypatch):
    """6. Spans of exactly 991 (the last read the LDS window serves) and 992 (the first that takes the words at L2) on 3100 anchors, each read in a call of its own and
    with the window switched off as well."""
    monkeypatch.setenv("LRA_SDP_BIG_POINTS", "3000")
    if window == "l2":
        monkeypatch.setenv("LRA_SDP_WG_RING", "0")
    kw = _mode_kw(mode)
    reads, lens = _assert_shapes("window_span", mode)
    exp = _oracle("window_span", mode, kw)
    for r in range(len(reads)):
        res, out = _run_hip(ctx, reads[r:r + 1], lens[r:r + 1], kw)
        assert _compare(out, int(res.num_aln), reads[r:r + 1], lens[r:r + 1], kw, must_have_result=True, oracle_results=exp[r:r + 1]) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("run", ["default", "workgroup-outgrown"])
def test_hip_sdp_per_read_rates(ctx, run, monkeypatch):
    """7. rate= of chain.sparse_dp_batch: a rate of its own for every read of the random mix (k_points, both ProcessPoint kernels); with the threshold lowered and
    estimates that the reads outgrow, k_reset_frags and the second attempt use it too."""
    if run == "workgroup-outgrown":
        monkeypatch.setenv("LRA_SDP_BIG_POINTS", WG)
        monkeypatch.setenv("LRA_SDP_ESTIMATE", "2.0,0.5")
    reads, lens = _random_read_mix()
    rates = _rates(len(reads))
    for kw in _MIX_OPTS:
        res, out = _run_hip(ctx, reads, lens, kw, rates=rates)
        assert _compare(out, int(res.num_aln), reads, lens, kw, must_have_result=True, rates=rates) == len(reads)


@pytest.mark.gpu
@pytest.mark.parametrize("opts", sorted(_MANY_OPTS))
def test_hip_sdp_sixteen_alignments(ctx, opts):
    """8. NumAln = MAXALN = 16 on reads of many clusters that do not chain with each other: 16 (the limit), 16 and 5 chains; 3, 16 and 5 with alnthres 0.1."""
    _run_and_compare(ctx, "many_clusters", 0, _MANY_OPTS[opts])


@pytest.mark.gpu
@pytest.mark.parametrize("num_aln", [0, 17])
def test_hip_sdp_num_aln_out_of_range(ctx, num_aln):
    """8. NumAln outside 1 .. 16 is LRA_ERR_INVALID, and the context serves the next call."""
    from lra_amd._lib import LraError
    reads, lens, _ = _case("many_clusters", 0)
    with pytest.raises(LraError, match=r"error -1\b.*NumAln"):
        _run_hip(ctx, reads, lens, dict(NumAln=num_aln))
    _run_and_compare(ctx, "many_clusters", 0, _MANY_OPTS["all_chains"])
