"""Tier-2 at every class boundary: lra_local_index_batch / _masked_batch (local_sketch staged and unstaged, local_sort_unique, the three local_sort_radix classes,
local_sort_exact_wave in both size classes, local_sort_filter staged and in HBM, RemoveFrequent in all three places) and lra_local_compare_batch (local_compare<2> with
local_compact_pairs or the local_compare<1> re-walk, local_compare_cached<2> with local_compact_rows and the local_compare_cached<1> re-walk) against the oracle
(oracle.local_index_seq, oracle.compare_lists_local; pinned to the reference's golden file in test_local.py), on the cases of local_cases.py.  Every comparison is
exact, and every sequence, window and task of every batch is compared.

The kernels are not instrumented: which kernel a case goes through follows from its raw list length, whether a key repeats, the window's stride, and a task's list
lengths and pair count.  The CPU tests below assert those numbers from the oracle alone, so a GPU test cannot quietly miss the class it is named for.

Deliberately out of reach:
  * the local_compare<1, true> re-walk: it needs more than 2^20 tasks that each outgrow a 512-pair row, over 4 GB of pairs;
  * the n_win >= 2^32 branch of the index entry;
  * local_sort_exact_wave's depth-limit branch (heap sort on one lane): the index entry only sorts the k-mers of a real sequence, an introsort adversary cannot be
    spelled as overlapping k-mers, and the heap sort it calls is std_sort.h's, which test_sort.py's adversaries cover."""
import ctypes as C

import numpy as np
import pytest

import local_cases as LC

MF = 15
INDEX = LC.index_batches()
_IDX = {}


# ---------------------------------------------------------------------------------------------------------------- the oracle's numbers
def _windows(oracle, name):
    """Per window of the batch, in the entry's order: (sequence label, window in sequence, raw length, a key repeats, kept length); and per sequence the oracle's
    (tuples, boundaries)."""
    if name not in _IDX:
        c = INDEX[name]
        wins, exp = [], []
        for lab, s in c["seqs"]:
            rt, rb = oracle.local_index_seq(s.tobytes(), c["k"], c["w"], c["window"], LC.ALL_KEPT)
            et, eb = oracle.local_index_seq(s.tobytes(), c["k"], c["w"], c["window"], c["max_freq"])
            assert len(rb) == len(eb)
            for wi in range(len(rb) - 1):
                keys = rt[int(rb[wi]):int(rb[wi + 1])] & 0xFFFFF
                wins.append((lab, wi, len(keys), len(np.unique(keys)) < len(keys), int(eb[wi + 1] - eb[wi])))
            exp.append((et, eb))
        _IDX[name] = (wins, exp)
    return _IDX[name]


def _by_label(wins):
    d = {}
    for lab, _wi, n, tie, kept in wins:
        d.setdefault(lab, []).append((n, tie, kept))
    return d


def test_w1_lists_have_every_length_tied_and_untied(oracle):
    """A.1: at w = 1 a window of L bases is a list of L - k + 1 tuples; every length round a class limit occurs without a repeated key (local_sort_unique up to
    RANK_CAP, then the radix class of its length) and with one (the exact sort: local_sort_exact_wave, stride 4087)."""
    wins, _ = _windows(oracle, "w1_k10")
    have = {(n, tie) for _l, _w, n, tie, _k in wins}
    assert {(n, False) for n in LC.LENS} <= have
    assert {(n, True) for n in LC.LENS if n > 1} <= have                  # (one tuple cannot tie)
    d = _by_label(wins)
    for n in LC.LENS:
        assert d["plain%d" % n] == [(n, False, n)]
        if n > 1:
            assert d["tied%d" % n][0][:2] == (n, True)
    wins7, _ = _windows(oracle, "w1_k7")
    d7 = _by_label(wins7)
    assert {n for _l, _w, n, _t, _k in wins7} >= set(LC.LENS) | {4090}
    assert d7["plain4090"][0][:2] == (4090, True) and d7["plain1025"][0][1] and d7["plain2049"][0][1]
    # k = 1: 4096 tuples of four keys -- n == NT * IPT of the last radix class, n == capAll of the exact wave
    wa, ea = _windows(oracle, "w1_k1_all")
    assert _by_label(wa)["four_keys"] == [(4096, True, 4096)] and len(np.unique(ea[0][0] & 0xFFFFF)) == 4
    wn, en = _windows(oracle, "w1_k1_none")
    assert _by_label(wn)["four_keys"] == [(4096, True, 0)] and len(en[0][0]) == 0 and list(en[0][1]) == [0, 0]


def test_stride_pair_sits_on_the_limit(oracle):
    """A.2: window 265 / 266 at k = 10, w = 1 are strides RANK_CAP / RANK_CAP + 1 -- the same tied lists go to local_sort_filter / to the exact wave."""
    w265, w266 = _windows(oracle, "stride_w265")[0], _windows(oracle, "stride_w266")[0]
    assert INDEX["stride_w265"]["window"] - 10 + 1 == LC.RANK_CAP and INDEX["stride_w266"]["window"] - 10 + 1 == LC.RANK_CAP + 1
    a, b = _by_label(w265), _by_label(w266)
    assert [x[0] for x in a["multi531"]] == [256, 256, 0] and [x[0] for x in b["multi531"]] == [257, 256]
    assert a["full265"] == [(256, False, 256)] and b["full266"] == [(257, False, 257)]                      # 257 untied: local_sort_radix<256, 4>'s shortest list
    assert a["tied265"][0][:2] == (256, True) and b["tied266"][0][:2] == (257, True)
    for d in (a, b):
        assert {d["tiedhbm%d" % n][0][:2] for n in (161, 162, 200, 255, 256)} == {(n, True) for n in (161, 162, 200, 255, 256)}   # above LCAP: sorted in HBM
        assert {d["tiedlds%d" % n][0][:2] for n in (2, 16, 17, 100, 159, 160)} == {(n, True) for n in (2, 16, 17, 100, 159, 160)}  # staged
    # local_sort_filter's blocks at stride 256 are 64 consecutive tied lists; one block's staged lists outgrow LS_WORDS, so its later lists are sorted in HBM
    tied = [n for _l, _w, n, tie, _k in w265 if tie]
    spill = 0
    for i in range(0, len(tied), 64):
        need = np.cumsum([n if n <= LC.LCAP else 0 for n in tied[i:i + 64]])
        spill += int(((need > LC.LS_WORDS) & (np.array(tied[i:i + 64]) <= LC.LCAP)).sum())
    assert spill >= 10
    # window 257 at w = 5: full windows are one base beyond WMAX (read from HBM), tails are staged; the N run covers the last two positions of window 0 and the first of 1
    c = INDEX["window257"]
    assert c["window"] == LC.WMAX + 1
    lens = {lab: len(s) for lab, s in c["seqs"]}
    assert lens["one"] == 257 and lens["one_plus"] == 258 and lens["staged"] == 256 and lens["two"] == 514
    s = dict(c["seqs"])["n255_257"]
    assert bytes(s[254:259]) == bytes([s[254]]) + b"NNN" + bytes([s[258]])
    w257 = _by_label(_windows(oracle, "window257")[0])
    assert [x[0] for x in w257["one_plus"]] == [w257["one_plus"][0][0], 0] and w257["one_plus"][0][0] > 80
    assert all(x[0] > 0 for x in w257["n255_257"])


def test_short_tied_lists(oracle):
    """A.3: a 13-base unit tiled to 25 / 26 / 35 / 36 bases: 16 / 17 / 26 / 27 tuples of 13 keys -- the exact wave with no partition (n <= 16) and its first."""
    for name in ("stride_w266", "stride_w265", "cut_w4096"):
        wins, exp = _windows(oracle, name)
        d = _by_label(wins)
        assert [d["unit13x%d" % L][0][:2] for L in (25, 26, 35, 36)] == [(16, True), (17, True), (26, True), (27, True)]
    seqs = dict(INDEX["stride_w266"]["seqs"])
    for L in (25, 26, 35, 36):
        assert len(np.unique(LC.kmer_keys(seqs["unit13x%d" % L], 10))) == 13


def test_remove_frequent_cut(oracle):
    """A.4: runs of max_freq - 1 stay, runs of max_freq go.  37-base unit, k = 10, w = 1, one window, max_freq 15: 14 copies are runs of 13 and 14 (all 509 kept), 15
    copies runs of 14 and 15 (the 9 keys of 14 kept: 126), 16 copies runs of 15 and 16 (nothing).  In windows of 265 / 266 the runs are 6 and 7: the cut is met at
    max_freq 6, 7, 8."""
    d = _by_label(_windows(oracle, "cut_w4096")[0])
    assert d["unit37x14"] == [(509, True, 509)] and d["unit37x15"] == [(546, True, 126)] and d["unit37x16"] == [(583, True, 0)]
    for window, n0 in ((265, 256), (266, 257)):
        kept = {}
        for mf in (6, 7, 8, 15):
            name = "stride_w%d" % window + ("_mf%d" % mf if mf != 15 else "")
            kept[mf] = _by_label(_windows(oracle, name)[0])["unit37x16"][0]
            assert kept[mf][0] == n0
        assert kept[6][2] == 0 and 0 < kept[7][2] < n0 and kept[8][2] == n0 and kept[15][2] == n0
        assert kept[7][2] % 6 == 0                                              # only the runs of 6 survive max_freq 7
    # max_freq 1 removes everything (the dispatcher's max_freq < 2 branch: local_sort_filter alone); 2 is the smallest value at which an untied list stays whole
    for name in ("mf1_w5", "mf1_w1"):
        assert all(k == 0 for *_x, k in _windows(oracle, name)[0])
    for name in ("mf2_w5", "mf2_w1"):
        wins = _windows(oracle, name)[0]
        assert all(k == n for _l, _w, n, tie, k in wins if not tie) and any(0 < k < n for _l, _w, n, tie, k in wins if tie)


def test_sketch_edge_counts(oracle):
    """A.5 (w = 5, k = 10, span 14): 13 / 14 / 15 / 23 / 24 bases give 0 / 0 / 1 / 3 / 4 tuples, as a sequence and as the tail behind a full window; a one-base tail
    is an empty window; an N every 14th base leaves no valid span; an all-N window between two good ones; lower case indexes like upper case."""
    wins, exp = _windows(oracle, "sketch_256")
    d = _by_label(wins)
    want = {13: 0, 14: 0, 15: 1, 23: 3, 24: 4}
    for L, n in want.items():
        assert d["len%d" % L] == [(n, False, n)], L
        assert len(d["tail%d" % L]) == 2 and d["tail%d" % L][1][0] == n, L
    assert len(d["exact"]) == 1 and [x[0] for x in d["plus1"]][1:] == [0] and d["plus1"][0][0] > 50
    assert all(x[0] == 0 for x in d["n_every_span"]) and len(d["n_every_span"]) == 3
    assert [x[0] > 50 for x in d["n_window"]] == [True, False, True] and d["n_window"][1][0] == 0
    for lab in ("n_first", "n_span_last", "n_last", "n_window_last", "n_window_first"):
        assert d[lab][0][0] > 50 and len(d[lab]) == 3
    seqs = dict(INDEX["sketch_256"]["seqs"])
    up = oracle.local_index_seq(seqs["lower"].tobytes().upper(), 10, 5, 256, MF)
    lo = exp[[l for l, _ in INDEX["sketch_256"]["seqs"]].index("lower")]
    assert np.array_equal(up[0], lo[0]) and len(lo[0]) > 80 and seqs["lower"].tobytes().islower()
    c = INDEX["sketch_maxw"]
    assert c["w"] == 16 and c["window"] == c["w"] + c["k"] and sum(n for _l, _w, n, _t, _k in _windows(oracle, "sketch_maxw")[0]) > 10
    for k in range(1, 11):
        assert INDEX["k%d" % k]["k"] == k and sum(n for _l, _w, n, _t, _k in _windows(oracle, "k%d" % k)[0]) > 50


def _pairs(oracle, t, mf=MF):
    return len(oracle.compare_lists_local(t.q, t.t, mf, t.max_diag, t.min_diag)[0])


def test_compare_builder_counts(oracle):
    """B: the builder's pair counts, list lengths and word counts sit on CMP_CAP, 255 / 256, CMP_TASK_MAX and CW_ROW; the batches are on the side of the switch they
    are named for."""
    for (a, b, m, last), n in LC.TABLE.items():
        q, t = LC.run_task(a, b, m, last)
        assert len(oracle.compare_lists_local(q, t, MF)[0]) == n, (a, b, m, last)
    assert sorted(LC.TABLE.values()) == [127, 128, 129, 511, 512, 513]
    q, t = LC.run_task(8, 16, 0, True)
    assert len(oracle.compare_lists_local(q, t, 8)[0]) == 128 and len(oracle.compare_lists_local(q, t, 7)[0]) == 0
    assert len(oracle.compare_lists_local(*LC.run_task(9, 16, 0, True), 8)[0]) == 0
    within = {t.name: t for t in LC.within_small_tasks()}
    over = {t.name: t for t in LC.over_small_tasks()}
    assert {_pairs(oracle, within[n]) for n in ("pairs127", "pairs128")} | {_pairs(oracle, over["pairs129"])} == {127, 128, 129}
    assert {len(within["q255"].q), len(within["t255"].t), len(over["q256"].q), len(over["t256"].t)} == {255, 256}
    assert len(within["both255"].q) == len(within["both255"].t) == 255 and len(over["both512"].q) == len(over["both512"].t) == 512
    assert {over["words512"].words, over["words513"].words} == {512, 513}
    assert (_pairs(oracle, within["run8"], 8), _pairs(oracle, within["run8"], 7), _pairs(oracle, within["run9"], 8)) == (128, 0, 0)
    for t in within.values():                                                  # nothing in `within` is above a limit of the one-pass form at any max_freq used
        assert len(t.q) <= 255 and len(t.t) <= 255 and t.words <= LC.CMP_TASK_MAX and max(_pairs(oracle, t, mf) for mf in (MF, 8, 7)) <= LC.CMP_CAP, t.name
    for name, t in over.items():
        above = [_pairs(oracle, t) > LC.CMP_CAP, len(t.q) > 255 or len(t.t) > 255]
        assert any(above), name
    crowd = [t.words for t in LC.within_small_tasks() if t.name.startswith("crowd")]
    assert len(crowd) == 128 and all(w == 200 for w in crowd) and 64 * 200 > LC.CMP_WORDS
    assert {_pairs(oracle, t) for t in LC.row_tasks()} == {511, 512, 513}
    assert {t.words > LC.CMP_TASK_MAX for t in LC.row_tasks()} == {False, True}
    assert all(_pairs(oracle, t) > 2000 for t in LC.thousands_tasks())
    for name, ts in LC.small_form_batches().items():
        assert 2 * LC.n_big(ts) <= len(ts), name
        n_over = sum(_pairs(oracle, t) > LC.CMP_CAP or len(t.q) > 255 or len(t.t) > 255 for t in ts)
        assert n_over == (0 if name == "within" else 1 if name != "over_all" else n_over) and (name != "over_all" or n_over > 10), name
    for name, ts in LC.large_form_batches().items():
        assert 2 * LC.n_big(ts) > len(ts), name
        n_row = sum(_pairs(oracle, t) > LC.CW_ROW for t in ts)
        assert (n_row == 0) == (name == "rows_fit"), name                      # rows_fit: the re-walk launch is skipped
        assert {511, 512} <= {_pairs(oracle, t) for t in ts}
    lo, hi = LC.switch_batches(20)
    assert len(lo) == len(hi) == 40 and LC.n_big(lo) == 20 and LC.n_big(hi) == 21


def test_line_tasks_cover_the_search_window(oracle):
    """B.4: from the walk restated in Python (held against the oracle pair for pair): lower bounds 0, 1, 11, 12, 13 and 300 above ts, upper bounds 1, 11, 12, 13 and 300 below te;
    list offsets and list ends of every residue mod 8 on both sides."""
    ts = LC.line_tasks()
    lows, ups = set(), set()
    for t in ts:
        oq, ot, lo, up = LC.walk_trace(t.q, t.t, MF)
        eq, et = oracle.compare_lists_local(t.q, t.t, MF)
        assert np.array_equal(np.array(oq, np.uint32), eq) and np.array_equal(np.array(ot, np.uint32), et), t.name
        lows |= set(lo); ups |= set(up)
    for near in (0, 1, LC.NEAR - 1, LC.NEAR, LC.NEAR + 1):
        assert near in lows and (near in ups or near == 0), near              # (the back branch is only taken with a key above the query's at te - 1: never 0)
    assert max(lows) >= 300 and max(ups) >= 300
    assert all(t.words > LC.CMP_TASK_MAX for t in ts[-16:]) and 2 * LC.n_big(ts) <= len(ts)   # (the batch is made large by the big tasks the test adds)
    ts = ts + LC.big_tasks(200, seed=95)
    _qa, _ta, ql, qh, tl, th = LC.layout(ts, *LC.line_gaps(ts))
    for arr in (ql, qh, tl, th):
        assert {x % LC.LINE for x in arr} == set(range(LC.LINE))
    assert len({(a % LC.LINE, b % LC.LINE) for a, b in zip(ql, tl)}) == LC.LINE * LC.LINE


# ---------------------------------------------------------------------------------------------------------------- A on the device
def _device_seqs(ctx, seqs):
    import torch
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    off = np.zeros(len(seqs) + 1, dtype=np.int64); off[1:] = np.cumsum(lens)
    buf = np.concatenate(list(seqs) + [np.zeros(64, np.uint8)])
    return torch.from_numpy(buf).to(ctx.device), torch.from_numpy(off).to(ctx.device)


def _check_index(got, labels, exp, active=None):
    win_off, bnd, tup = got
    assert len(win_off) == len(labels) + 1
    for i, lab in enumerate(labels):
        et, eb = exp[i]
        w0, w1 = int(win_off[i]), int(win_off[i + 1])
        assert w1 - w0 == len(eb) - 1, ("windows", lab)
        got_b = bnd[w0:w1 + 1] - bnd[w0]
        if active is not None and not active[i]:
            assert not got_b.any(), ("masked sequence has tuples", lab)
            continue
        assert np.array_equal(got_b, eb), ("boundaries", lab, got_b.tolist()[:8], eb.tolist()[:8])
        g = tup[int(bnd[w0]):int(bnd[w1])]
        if not np.array_equal(g, et):
            bad = int(np.nonzero(g != et)[0][0])
            raise AssertionError(("tuples", lab, "window", int(np.searchsorted(eb, bad, side="right") - 1), "at", bad))
    assert int(bnd[-1]) == len(tup)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INDEX))
def test_hip_local_index_edges(ctx, oracle, name):
    """One call of lra_local_index_batch per batch of local_cases.index_batches(); every sequence's windows, boundaries and tuples equal the oracle's."""
    from lra_amd import local
    c = INDEX[name]
    _wins, exp = _windows(oracle, name)
    sd, od = _device_seqs(ctx, [s for _l, s in c["seqs"]])
    li = local.LocalIndex(ctx, sd, od, c["k"], c["w"], c["window"], c["max_freq"])
    _check_index(li.fetch(), [l for l, _s in c["seqs"]], exp)


MASKED = LC.masked_seqs()


@pytest.mark.gpu
@pytest.mark.parametrize("mask", sorted(LC.masks(len(MASKED))))
@pytest.mark.parametrize("window", [256, 266])
def test_hip_local_index_masked(ctx, oracle, mask, window):
    """lra_local_index_masked_batch, the entry both map drivers call: a switched-off sequence keeps its windows in win_off, with empty tuple ranges; every other
    sequence's tuples are the oracle's."""
    import torch
    from lra_amd import local
    act = LC.masks(len(MASKED))[mask]
    k, w = (10, 5) if window == 256 else (10, 1)
    exp = [oracle.local_index_seq(s.tobytes(), k, w, window, MF) for _l, s in MASKED]
    sd, od = _device_seqs(ctx, [s for _l, s in MASKED])
    li = local.LocalIndex(ctx, sd, od, k, w, window, MF, active=torch.from_numpy(act).to(ctx.device))
    assert li.n_windows == sum(len(eb) - 1 for _et, eb in exp)
    assert li.n_tuples == sum(len(et) for (et, _eb), a in zip(exp, act) if a)
    _check_index(li.fetch(), [l for l, _s in MASKED], exp, act)


@pytest.mark.gpu
def test_hip_local_index_entry_validation(ctx):
    """k outside 1..10, w outside 1..16, a window below w + k or above 4096 are LRA_ERR_INVALID; no sequences is an empty result."""
    from lra_amd import local
    from lra_amd.context import ptr
    g = LC.genome(53)[:600].copy()
    sd, od = _device_seqs(ctx, [g])
    call = lambda n, k, w, window, res: ctx.lib.lra_local_index_batch(ctx.h, n, ptr(sd), ptr(od), k, w, window, MF, C.byref(res))
    for k, w, window in ((0, 5, 256), (11, 5, 256), (10, 0, 256), (10, 17, 256), (10, 5, 14), (10, 16, 25), (1, 1, 1), (10, 5, 4097)):
        assert call(1, k, w, window, local.LocalIndexResult()) == -1, (k, w, window)          # LRA_ERR_INVALID
    assert call(-1, 10, 5, 256, local.LocalIndexResult()) == -1
    for k, w, window in ((10, 5, 15), (1, 1, 2), (10, 16, 26), (10, 5, 4096)):               # the limits themselves are accepted
        assert call(1, k, w, window, local.LocalIndexResult()) == 0, (k, w, window)
    res = local.LocalIndexResult()
    res.n_windows = res.n_tuples = 99
    assert call(0, 10, 5, 256, res) == 0
    assert (res.n_seqs, res.n_windows, res.n_tuples, res.bytes) == (0, 0, 0, 0)
    mres = local.LocalIndexResult()
    assert ctx.lib.lra_local_index_masked_batch(ctx.h, 0, ptr(sd), ptr(od), None, 10, 5, 256, MF, C.byref(mres)) == 0 and mres.n_windows == 0


# ---------------------------------------------------------------------------------------------------------------- B on the device
def _expected(oracle, t, mf):
    """The oracle's pairs of a task, kept on the task (the batches share their tasks)."""
    memo = t.__dict__.setdefault("expected", {})
    if mf not in memo:
        memo[mf] = oracle.compare_lists_local(t.q, t.t, mf, t.max_diag, t.min_diag)
    return memo[mf]


def _check_compare(ctx, oracle, tasks, mf=MF, gaps=None):
    from lra_amd import local
    qa, ta, ql, qh, tl, th = LC.layout(tasks, *(gaps or (None, None)))
    A, B = LC.Raw(ctx, qa), LC.Raw(ctx, ta)
    banded = any(t.max_diag or t.min_diag for t in tasks)
    kw = dict(max_diag=[t.max_diag for t in tasks], min_diag=[t.min_diag for t in tasks]) if banded else {}
    off, pqi, pti = local.local_compare_batch(ctx, A, ql, qh, B, tl, th, mf, **kw)
    total = 0
    for x, t in enumerate(tasks):
        eq, et = _expected(oracle, t, mf)
        a, b = int(off[x]), int(off[x + 1])
        assert b - a == len(eq), ("pair count", x, t.name, b - a, len(eq))
        assert np.array_equal(pqi[a:b], eq + np.uint32(ql[x])) and np.array_equal(pti[a:b], et + np.uint32(tl[x])), ("pairs", x, t.name)
        total += b - a
    assert int(off[-1]) == total == len(pqi) == len(pti)
    return total


SMALL = LC.small_form_batches()
LARGE = LC.large_form_batches()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SMALL))
def test_hip_local_compare_small_form(ctx, oracle, name):
    """local_compare<2>: `within` has no task above the one-pass limits (local_compact_pairs lays the pairs out); each over_* batch has one task above one limit (129
    pairs, a list of 256 on either side, 512 / 513 words) and takes the local_compare<1> re-walk; over_all has them all, and big tasks short of half the batch."""
    assert _check_compare(ctx, oracle, SMALL[name]) > 3000


@pytest.mark.gpu
@pytest.mark.parametrize("mf", [8, 7])
def test_hip_local_compare_small_form_query_run_cut(ctx, oracle, mf):
    """A query run of max_freq keys is not paired, one of max_freq - 1 is: 8 copies at max_freq 8 give 128 pairs, at 7 none; 9 copies at 8 none."""
    _check_compare(ctx, oracle, SMALL["within"], mf)
    _check_compare(ctx, oracle, SMALL["over_all"], mf)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["within", "over_all"])
def test_hip_local_compare_small_form_banded(ctx, oracle, name):
    """Per-task diagonal bounds: a bound of exactly 0 on one side only switches the filter off (CompareLists.h:87); a pair on maxDiag and a pair on minDiag stay."""
    assert _check_compare(ctx, oracle, LC.with_bounds(SMALL[name], oracle, MF)) > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LARGE))
def test_hip_local_compare_large_form(ctx, oracle, name):
    """local_compare_cached<2> + local_compact_rows: rows_fit has tasks of 511 and 512 pairs and none above (the re-walk launch is skipped); rows_over adds 513 pairs
    and thousands (local_compare_cached<1> through overList).  The small form's boundary tasks ride along in the cached walk."""
    assert _check_compare(ctx, oracle, LARGE[name]) > 20000


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LARGE))
def test_hip_local_compare_large_form_banded(ctx, oracle, name):
    assert _check_compare(ctx, oracle, LC.with_bounds(LARGE[name], oracle, MF)) > 5000


@pytest.mark.gpu
def test_hip_local_compare_large_form_query_run_cut(ctx, oracle):
    _check_compare(ctx, oracle, LARGE["rows_over"], 8)


@pytest.mark.gpu
def test_hip_local_compare_form_switch(ctx, oracle):
    """2 * big > tasks: of two batches of 40 tasks from one set, the one with 20 big tasks takes the small form and the one with 21 the large form."""
    lo, hi = LC.switch_batches(20)
    _check_compare(ctx, oracle, lo)
    _check_compare(ctx, oracle, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("banded", [False, True])
def test_hip_local_compare_cached_lines(ctx, oracle, banded):
    """The cached walk's 8-word lines and its 12-element search window: list offsets and ends of every residue mod 8 on both sides, bounds 0 / 1 / 11 / 12 / 13 / 300
    elements from the cursor in both directions, runs of 9 (longer than a line) on all four cursors."""
    tasks = LC.line_tasks() + LC.big_tasks(200, seed=95)
    assert 2 * LC.n_big(tasks) > len(tasks)
    if banded:
        tasks = LC.with_bounds(tasks, oracle, MF)
    assert _check_compare(ctx, oracle, tasks, gaps=LC.line_gaps(tasks)) > 5000
