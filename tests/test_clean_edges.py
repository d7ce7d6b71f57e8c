"""a5 / a7 on crafted matches: CleanMatches (clean_wave_kernel), MatchesToFineClusters (fc_kernel) and the pair version of LinearExtend
(linear_extend_kernel) at the boundaries their arguments rest on, injected through lra_seed_set_matches.

A segment (one read, one strand) is a list of diagonal runs in the order the stage's sort leaves them: inside a run the sort diagonal (q - t forward, the 32-bit q + t
reverse) never decreases and q rises, a sub-run break is a jump in [SecondCleanMaxDiag, cleanMaxDiag), a run break a jump >= cleanMaxDiag, a run of one match an
isolated match (it shifts the following runs along the 64-match chunks of the kernel's ballots).  The matches are shuffled before they are injected.
"""
import numpy as np
import pytest

import oracle_lib as O

C3 = [0, 1_000_000, 2_000_000, 4_000_000]                  # three chromosomes
LENS = [1, 2, 3, 9, 10, 11, 29, 30, 31, 62, 63, 64, 65, 66, 99, 100, 101, 126, 127, 128, 129, 130, 191, 192, 193, 256, 257, 1000]
THRESHOLDS = [1.0, 1.5, 2.0, 3.0, 4.0]
CLEAN_SETS = {
    "ONT": dict(O.CLEAN_PRESETS["ONT"]),
    "CCS": dict(O.CLEAN_PRESETS["CCS"]),
    # cleanClustersize 20: (len - cc) / cc is 0, 1, 2 at 20..39, 40..59, 60..79
    "ONT_CC20": dict(O.CLEAN_PRESETS["ONT"], cleanClustersize=20),
    # small thresholds: punish_anchorfreq / 2 == 0, so MinDiagCluster <= 0 and MinDiagCluster >= len both occur at small sizes, and runs of avgfreq >= 10 survive
    "SMALL": dict(globalK=17, cleanMaxDiag=150, minDiagCluster=2, bypassClustering=0, cleanClustersize=20, SecondCleanMinDiagCluster=3, SecondCleanMaxDiag=100,
                  punish_anchorfreq=1, anchorPerlength=2),
}
FINE_SETS = {
    "CCS": dict(globalK=17, RoughClustermaxGap=500, maxDiag=500, maxGap=400, minClusterSize=10, minUniqueStretchNum=1, minUniqueStretchDist=50),
    "CONTIG": dict(globalK=19, RoughClustermaxGap=500, maxDiag=100, maxGap=500, minClusterSize=10, minUniqueStretchNum=1, minUniqueStretchDist=50),
    "LOOSE": dict(globalK=17, RoughClustermaxGap=200, maxDiag=60, maxGap=150, minClusterSize=2, minUniqueStretchNum=1, minUniqueStretchDist=20),
    "TIGHT": dict(globalK=17, RoughClustermaxGap=500, maxDiag=500, maxGap=400, minClusterSize=2, minUniqueStretchNum=1, minUniqueStretchDist=10),
}
f32 = np.float32


def second_round_threshold(o, length, distinct):
    """MinDiagCluster of Clustering.h:635-693 for a run (None: the run is kept or dropped whole), in the reference's float arithmetic."""
    f = f32(length) / f32(distinct)
    cc = o["cleanClustersize"]; S = o["SecondCleanMinDiagCluster"]; p = o["punish_anchorfreq"]; a = o["anchorPerlength"]
    fl = lambda x: float(np.floor(f32(x)))
    if f >= 3 and length < 10:
        return None
    if o["bypassClustering"]:
        if f >= 2 and length >= cc:
            return int(S + fl((f - f32(1.5)) / f32(1.0)) * p + ((length - cc) // cc) * a)
        if f >= 1.5 and length >= cc:
            return int(S + fl((f - f32(1.5)) / f32(1.5)) * p + ((length - cc) // cc) * a)
        return None
    if f >= 4 and length >= cc:
        return int(S + fl((f - f32(1.5)) / f32(1.0)) * p + ((length - cc) // cc) * a)
    if f >= 1.5 and length >= cc:
        return int(S + fl((f - f32(1.5)) / f32(1.5)) * p + ((length - cc) // cc) * a)
    if f > 1 and length >= cc:
        return int(S - (5 - fl((f - f32(1.0)) / f32(0.1))) * (p // 2) + ((length - cc) // cc) * (a // 2))
    if f > 1:
        return int(S - (5 - fl((f - f32(1.0)) / f32(0.1))) * (p // 2) - ((cc - length) // 15) * (a // 2))
    return None


def sub_run_patterns(L, M):
    """Splits of a run of L matches into sub-runs whose lengths sit at M - 1, M and M + 1 (M = its MinDiagCluster)."""
    if M is None or M < 2 or M >= L:
        return [[L], [L // 2, L - L // 2]] if L >= 4 else [[L]]
    pats = [[L]]
    for a in (M - 1, M, M + 1):
        if 0 < a < L:
            pats += [[a, L - a], [L - a, a]]
    if 3 * M <= L:
        pats.append([M - 1, M, L - 3 * M + 2, M - 1] if L - 3 * M + 2 > 0 else [M - 1, M, M - 1])   # short, long, ..., short: the survivors are an inner span
        pats.append([M - 1, M, M - 1, M + 1, L - 4 * M + 1] if L - 4 * M + 1 > 0 else [M - 1, M, L - 2 * M + 1])
    n = L // max(1, M - 1)
    if M - 1 >= 2:
        pats.append([M - 1] * n + ([L - n * (M - 1)] if L - n * (M - 1) else []))                  # nothing long enough
    return [p for p in pats if sum(p) == L and all(x > 0 for x in p)]


class Segment:
    """One strand of one read under construction (matches in sorted order)."""

    def __init__(self, o, strand, rng):
        self.o, self.strand, self.rng = o, strand, rng
        self.q, self.cum, self.key = [], [], []
        self.c = 0; self.qn = int(rng.integers(0, 50)); self.kn = 1; self.first_run = None

    def run(self, sub, distinct=None, qstep=3, jitter=2, big=None):
        """A run: sub = the sub-run lengths; distinct = its number of different read k-mers (default all different)."""
        o = self.o; L = sum(sub); distinct = L if distinct is None else max(1, min(L, distinct))
        if self.q:
            self.c += int(big if big is not None else o["cleanMaxDiag"] + self.rng.integers(0, 3) * 50)
        if L > 1 and self.first_run is None:
            self.first_run = (len(self.q), len(self.q) + L)
        i = 0
        for s_i, s in enumerate(sub):
            if s_i:
                self.c += int(self.rng.integers(o["SecondCleanMaxDiag"], o["cleanMaxDiag"]))
            for j in range(s):
                if j:
                    self.c += int(self.rng.integers(0, jitter + 1))
                self.q.append(self.qn); self.cum.append(self.c); self.key.append(self.kn + i % distinct)
                self.qn += qstep; i += 1
        self.kn += L + 1
        return self

    def isolated(self, n):
        for _ in range(n):
            self.run([1])
        return self

    def finish(self, target=None, wrap=False):
        """-> (q, t, key) uint arrays, shuffled.  target: the smallest t of the first run; wrap: the reverse diagonal q + t crosses 2^32."""
        q = np.asarray(self.q, np.int64); cum = np.asarray(self.cum, np.int64)
        if len(q) == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint64)
        t = (q - cum) if self.strand == 0 else (cum - q)                 # sort diagonal q - t = cum (forward), q + t = cum (reverse), up to the shift below
        a, b = self.first_run if self.first_run else (0, len(q))
        if wrap:
            assert self.strand == 1
            t = t + (2 ** 32 - int(np.sort(q + t)[len(q) // 2]))           # the sums pass 2^32 in the middle of the segment (t near 0xFFFFF000)
            assert t.min() > 0xFFFF0000
            assert (q + t).max() >= 2 ** 32 > (q + t).min()
            t = t % 2 ** 32
        else:
            t = t + ((C3[1] + 300_000 if target is None else target) - int(t[a:b].min()))
            assert t.min() >= 0 and t.max() + 64 < C3[3]
        assert len(set(zip(q.tolist(), t.tolist()))) == len(q)           # distinct (q, t) pairs: one sorted order
        p = self.rng.permutation(len(q))
        return q[p].astype(np.uint32), t[p].astype(np.uint32), np.asarray(self.key, np.uint64)[p]


def _clean_segments(o, rng, wrap):
    """The clean stage's boundaries for option set o -> list of (strand, q, t, key)"""
    CM = o["cleanMaxDiag"]
    segs = []
    targets = [C3[1], C3[1] - 1, C3[1] + 1, C3[2], C3[2] - 1, C3[2] + 1, C3[1] - 5, None, None, None]
    add = lambda s, **kw: segs.append((s.strand,) + s.finish(**kw))
    strand_of = lambda: len(segs) % 2
    # the smallest segments
    add(Segment(o, 0, rng)); add(Segment(o, 1, rng))
    add(Segment(o, 0, rng).run([1])); add(Segment(o, 1, rng).run([1]))
    add(Segment(o, 0, rng).run([2])); add(Segment(o, 1, rng).run([2]))          # n == 2 on the diagonal
    add(Segment(o, 0, rng).isolated(2)); add(Segment(o, 1, rng).isolated(2))    # ... and off it
    add(Segment(o, 0, rng).run([1]).run([1], big=CM)); add(Segment(o, 0, rng).run([1]).run([1], big=CM - 1))   # the jump exactly at cleanMaxDiag / one below
    add(Segment(o, 0, rng).isolated(130))                                        # no neighbour on a diagonal, over several chunks
    # every run length at every avgfreq threshold, alone in its segment (one single run; it ends at n - 1) and behind 0 / 1 / 62 / 63 isolated matches
    combo = 0
    for L in LENS[1:]:
        for thr in THRESHOLDS:
            for step in (-1, 0, 1):
                d = int(L / thr) + step
                if d < 1 or d > L or (step and int(L / thr) == L / thr and False):
                    continue
                M = second_round_threshold(o, L, d)
                pats = sub_run_patterns(L, M)
                sub = pats[combo % len(pats)]
                pad = (0, 1, 62, 63, 0, 64)[combo % 6]
                s = Segment(o, strand_of(), rng).isolated(pad).run(sub, d)
                if combo % 3 == 1:
                    L2 = LENS[1:-1][(combo // 3) % (len(LENS) - 2)]
                    s.run([L2], max(1, L2 - combo % 4))
                if combo % 4 == 3:
                    s.isolated(1 + combo % 3)                                    # the last run does not end the segment
                add(s, target=targets[combo % len(targets)])
                combo += 1
    # all the sub-run patterns of a few runs whose second round has room for them
    for L, d in ((100, 50), (101, 40), (130, 60), (193, 48), (257, 120), (30, 12), (31, 7), (66, 30), (64, 31), (129, 64), (192, 96), (1000, 400), (1000, 900)):
        M = second_round_threshold(o, L, d)
        for k, sub in enumerate(sub_run_patterns(L, M)):
            add(Segment(o, strand_of(), rng).isolated((0, 63, 1, 62)[k % 4]).run(sub, d).isolated(k % 2), target=targets[(k + 7) % len(targets)])
    # many runs in one segment: open runs carried over chunk ends, the key table of a run next to the following run's
    for k in range(6):
        s = Segment(o, k % 2, rng)
        for j in range(40):
            L = LENS[1:-1][(7 * j + k) % (len(LENS) - 2)]
            s.run([L], max(1, L - (j % 5) * (L // 6)))
        add(s)
    if wrap:
        for k in range(4):
            s = Segment(o, 1, rng).isolated(k)
            for L in (64, 3, 130, 31, 100):
                s.run([L], max(1, L - k * (L // 5)))
            add(s, wrap=True)
    return segs


def _fine_segments(o, rng):
    """Segments aimed at the branches of SplitRoughClustersWithGaps / StoreFineClusters -> list of (strand, q, t, key, first_in_read)"""
    out = []

    def seg(strand, groups, distinct_drop=2, target=None, first=False):
        """groups: list of (n, qstep, tstep, gap_q, gap_t, dup): n matches; gap before the group; dup: the group's first q carries a second match 40 further in t"""
        q, t = [], []
        cq, ct = 100, 0
        for (n, qs, ts, gq, gt, dup) in groups:
            cq += gq; ct += gt
            for j in range(n):
                q.append(cq); t.append(ct)
                if dup and j == 0:
                    q.append(cq); t.append(ct + 40)
                cq += qs; ct += ts
        q = np.asarray(q, np.int64); t = np.asarray(t, np.int64)
        if strand == 1:
            t = t.max() - t
        t = t + ((C3[1] + 500_000 if target is None else target) - t.min())
        n = len(q)
        key = np.arange(n, dtype=np.uint64) % np.uint64(max(1, n - distinct_drop)) + np.uint64(7)
        p = rng.permutation(n)
        out.append((strand, q[p].astype(np.uint32), t[p].astype(np.uint32), key[p], first))

    for st in (0, 1):
        A = (20, 20, 20, 0, 0, False)
        seg(st, [A, (16, 20, 20, 450, 450, False)])                                                     # a leftover stretch of 16 behind the largest
        seg(st, [A, (16, 1, 12, 450, 450, False)])                                                        # ... too steep: dropped by the ratio test
        seg(st, [A, (16, 20, 20, 450, 450, False)], target=C3[2] - (20 * 20 + 450 + 100 if st == 0 else 100))   # ... across a chromosome start: dropped
        seg(st, [(20, 1, 12, 0, 0, False), (16, 20, 20, 450, 450, False)], target=C3[2] - (20 * 12 + 450 + 100 if st == 0 else 100), first=True)   # nothing before it
        seg(st, [(20, 1, 12, 0, 0, False)])                                                              # the main cluster too steep
        seg(st, [(12, 20, 20, 0, 0, False), (8, 20, 20, 30, 30, True), (6, 20, 20, 30, 30, True)])        # forward picks past doubled read positions
        seg(st, [(6, 20, 20, 0, 0, False), (8, 20, 20, 30, 30, True), (12, 20, 20, 30, 30, True)])        # backward picks
        seg(st, [(5, 20, 20, 0, 0, False), (7, 20, 20, 30, 30, True), (15, 20, 20, 30, 30, True), (6, 20, 20, 30, 30, True)])
        seg(st, [(12, 20, 20, 0, 0, False), (12, 20, 20, 510 - 20, 510 - 20, False)])                    # CloseToPreviousCluster: merged
        seg(st, [(12, 20, 20, 0, 0, False), (12, 20, 20, 600, 600, False)])                              # ... too far: pushed
        seg(st, [(12, 20, 20, 0, 0, False), (3, 20, 20, 600, 600, False), (12, 20, 20, 600, 600, False)])
        seg(st, [(30, 20, 20, 0, 0, False)], distinct_drop=0, target=C3[1] - 5)                          # anchorfreq 1 across a chromosome start
        seg(st, [(30, 20, 20, 0, 0, False)], target=C3[1] - 5)                                           # the same with anchorfreq > 1
        seg(st, [(30, 20, 20, 0, 0, False)], target=C3[1] - 1)
        seg(st, [(10, 20, 20, 0, 0, False)])                                                             # exactly minClusterSize matches
        seg(st, [(11, 20, 20, 0, 0, False)])
        seg(st, [(3, 20, 20, 0, 0, False)])
        seg(st, [(12, 0, 5, 0, 0, False)], distinct_drop=11)                                             # one read position twelve times: avgfreq 12, one group
        seg(st, [(14, 20, 20, 0, 0, False)], distinct_drop=13)                                           # avgfreq 14 over distinct read positions
        seg(st, [(2, 0, 5, 0, 0, False)], distinct_drop=1)
    return out


_SETS = {}


def crafted(name, for_fine=False):
    """The crafted batch for clean option set `name` (built once): list of reads, each (q, t, key, n_forward) with the forward-strand matches first.
    for_fine: without the segments whose q + t crosses 2^32 (their boxes wrap; the clean stage alone is defined there)."""
    k = (name, for_fine)
    if k in _SETS:
        return _SETS[k]
    o = CLEAN_SETS[name]
    rng = np.random.default_rng(20 + sorted(CLEAN_SETS).index(name))
    segs = _clean_segments(o, rng, wrap=not for_fine)
    fwd = [s for s in segs if s[0] == 0]; rev = [s for s in segs if s[0] == 1]
    e = (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint64))
    reads = []
    for i in range(max(len(fwd), len(rev))):
        f = fwd[i][1:] if i < len(fwd) and i % 11 != 5 else e             # (every eleventh read has reverse matches only)
        r = rev[i][1:] if i < len(rev) else e
        reads.append((np.concatenate([f[0], r[0]]), np.concatenate([f[1], r[1]]), np.concatenate([f[2], r[2]]), len(f[0])))
    for (st, q, t, key, first) in _fine_segments(o, rng):
        reads.append((q, t, key, len(q) if st == 0 else 0))
    _SETS[k] = reads
    return reads


def _run_clean_oracle(name, reads):
    opts = O.CleanOpts(**CLEAN_SETS[name])
    res = []
    for (q, t, key, nf) in reads:
        res.append([O.clean_matches(q[:nf], t[:nf], key[:nf], 0, opts, C3), O.clean_matches(q[nf:], t[nf:], key[nf:], 1, opts, C3)])
    return res


def _fine_clean_opts(name):
    return dict(CLEAN_SETS[name], bypassClustering=0)


# ------------------------------------------------------------------------------------------------------------------------------- CPU
# branches no input can reach (DESIGN.md "a5: forms that cannot occur"): they must stay at zero
CLEAN_UNREACHABLE = {"sr_exit_one_match"}
FINE_UNREACHABLE = {"pop_qspan_zero", "ub_qspan_zero"}


def test_crafted_set_reaches_every_branch(oracle):
    """The oracle over the whole crafted set reaches every counted branch of CleanOffDiagonal / SecondRoundCleanOffDiagonal and of SplitRoughClustersWithGaps /
    StoreFineClusters; the branches that cannot occur stay at zero.  Hits over the four option sets (2326 segments, 481537 matches; 4636 fine-cluster reads):
      clean  no_neighbour 24, min_diag_zero 108, run_too_short 63, bypass_drop 28, bypass_ge2 527, bypass_ge1_5 161, bypass_keep 964, drop 27, ge4 96, ge1_5 581,
             gt1_long 318, gt1_short 408, keep 232, sr_exit_ge_len 125, sr_exit_le_zero 106, sr_exit_one_match 0 (cannot occur), sr_none_long 135, sr_one_long 1030,
             sr_several_long 695, sr_inner_span 114
      fine   freq_ge10 24, merge 24, push 11140, freq_one 1662, freq_one_pop_chrom 192, one_group 8, whole_split 7573, backward_pick 1373, forward_pick 799,
             leftover 56, pop_chrom 842, pop_size 24, pop_qspan_zero 0 (cannot occur), pop_ratio 42, leftover_pop_chrom 24, leftover_pop_ratio 16, ub_empty 8,
             ub_qspan_zero 0 (cannot occur)
    (the decision of Clustering.h:638 / :661, `avgfreq >= 3 and len < 10`, is written once per bypassClustering mode: ten slots for the nine branches.)"""
    O.clean_counters(reset=True); O.fine_counters(reset=True)
    n_seg = n_match = 0
    for name in CLEAN_SETS:
        reads = crafted(name)
        _run_clean_oracle(name, reads)
        n_seg += 2 * len(reads); n_match += sum(len(r[0]) for r in reads)
    clean = O.clean_counters(reset=True)
    n_ub = n_reads = 0
    for name in CLEAN_SETS:
        co = O.CleanOpts(**_fine_clean_opts(name))
        for fname, fo in FINE_SETS.items():
            for (q, t, key, nf) in crafted(name, for_fine=True):
                _, st = O.matches_to_fine_clusters(q, t, key, nf, co, O.FineOpts(**fo), C3)
                n_ub += st != 0; n_reads += 1
    fine = O.fine_counters(reset=True)
    print("clean", clean); print("fine", fine); print("segments", n_seg, "matches", n_match, "fine reads", n_reads, "undefined", n_ub)
    for k, v in clean.items():
        assert (v == 0) if k in CLEAN_UNREACHABLE else (v > 0), ("clean", k, v)
    for k, v in fine.items():
        assert (v == 0) if k in FINE_UNREACHABLE else (v > 0), ("fine", k, v)
    assert n_ub > 0 and n_ub * 20 <= n_reads, (n_ub, n_reads)           # reads the reference leaves undefined: some, and at most 5 %


@pytest.mark.parametrize("name", sorted(CLEAN_SETS))
def test_oracle_clean_properties(oracle, name):
    """Survivors are a subset of the input in sort order, the clusters tile them, the boxes are the min / max of their matches plus K."""
    K = CLEAN_SETS[name]["globalK"]; CM = CLEAN_SETS[name]["cleanMaxDiag"]
    reads = crafted(name)
    n_cl = 0
    for (q, t, key, nf), both in zip(reads, _run_clean_oracle(name, reads)):
        for strand, (oq, ot, cl) in enumerate(both):
            a, b = (0, nf) if strand == 0 else (nf, len(q))
            iq, it = q[a:b].astype(np.int64), t[a:b].astype(np.int64)
            d = (iq - it) if strand == 0 else ((iq + it) % 2 ** 32)
            order = np.lexsort((iq, d))
            pairs = list(zip(iq[order].tolist(), it[order].tolist()))
            pos = {p: i for i, p in enumerate(pairs)}
            idx = [pos[p] for p in zip(oq.tolist(), ot.tolist())]         # KeyError: a survivor that was never put in
            assert all(x < y for x, y in zip(idx, idx[1:]))
            nc = len(cl["start"])
            assert (nc == 0) == (len(oq) == 0)
            if nc:
                assert cl["start"][0] == 0 and cl["end"][-1] == len(oq) and np.array_equal(cl["start"][1:], cl["end"][:-1]) and np.all(cl["end"] > cl["start"])
            for c in range(nc):
                s, e = int(cl["start"][c]), int(cl["end"][c])
                cq, ct = oq[s:e], ot[s:e]
                assert (cl["qStart"][c], cl["qEnd"][c], cl["tStart"][c]) == (cq.min(), cq.max() + K, ct.min())
                assert cl["tEnd"][c] == np.uint32(ct.max() + np.uint32(K))
                assert idx[e - 1] - idx[s] == e - s - 1                    # one contiguous piece of the sorted input
                dd = d[order][idx[s]:idx[e - 1] + 1]
                assert np.all(np.abs(np.diff(dd)) < CM)
                assert cl["chrom"][c] == np.searchsorted(np.asarray(C3), int(ct.min()), side="right") - 1
                n_cl += 1
    assert n_cl > 100


# ------------------------------------------------------------------------------------------------------------------------------- GPU
def _inject(ctx, reads):
    from lra_amd import seed
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r[0]) for r in reads])
    cat = lambda i, dt: np.concatenate([r[i] for r in reads]).astype(dt) if reads else np.zeros(0, dt)
    return seed.set_matches(ctx, off, [r[3] for r in reads], cat(0, np.uint32), cat(1, np.uint32), cat(2, np.uint64)), off


def _clusters_of(out, r):
    got = []
    for x in range(int(out["cluster_off"][r]), int(out["cluster_off"][r + 1])):
        a, b = int(out["start"][x]), int(out["end"][x])
        got.append((int(out["strand"][x]), int(out["qStart"][x]), int(out["qEnd"][x]), int(out["tStart"][x]), int(out["tEnd"][x]), int(out["chrom"][x]),
                    int(out["freq"][x:x + 1].view(np.uint32)[0]), out["cl_qpos"][a:b].tolist(), out["cl_tpos"][a:b].tolist()))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CLEAN_SETS))
def test_hip_clean_crafted(ctx, oracle, name):
    from lra_amd import cluster
    reads = crafted(name)
    _inject(ctx, reads)
    out = cluster.fetch(ctx, cluster.clean_matches_batch(ctx, cluster.CleanOpts(**CLEAN_SETS[name]), C3))
    total = 0
    for r, both in enumerate(_run_clean_oracle(name, reads)):
        exp = []
        for strand, (oq, ot, cl) in enumerate(both):
            for i in range(len(cl["start"])):
                a, b = int(cl["start"][i]), int(cl["end"][i])
                exp.append((strand, int(cl["qStart"][i]), int(cl["qEnd"][i]), int(cl["tStart"][i]), int(cl["tEnd"][i]), int(cl["chrom"][i]),
                            int(cl["freq"][i:i + 1].view(np.uint32)[0]), oq[a:b].tolist(), ot[a:b].tolist()))
        got = _clusters_of(out, r)
        assert len(got) == len(exp), (r, len(got), len(exp))
        for x, (g, e) in enumerate(zip(got, exp)):
            assert g == e, (r, x, g[:7], e[:7])
        total += len(exp)
    assert total > 100


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CLEAN_SETS))
def test_hip_fine_crafted(ctx, oracle, name):
    from lra_amd import cluster
    reads = crafted(name, for_fine=True)
    cl = _fine_clean_opts(name)
    _inject(ctx, reads)
    rough = cluster.clean_matches_batch(ctx, cluster.CleanOpts(**cl), C3)
    co = O.CleanOpts(**cl)
    for fname, fd in FINE_SETS.items():
        out = cluster.fetch_fine(ctx, cluster.fine_clusters_batch(ctx, rough, cluster.FineOpts(**fd), C3))
        fo = O.FineOpts(**fd)
        n_cl = n_skip = 0
        for r, (q, t, key, nf) in enumerate(reads):
            exp, st = O.matches_to_fine_clusters(q, t, key, nf, co, fo, C3)
            assert (out["status"][r] != 0) == (st != 0), (fname, r)
            if st:
                n_skip += 1
                continue
            c0, c1 = int(out["cluster_off"][r]), int(out["cluster_off"][r + 1])
            assert c1 - c0 == len(exp["strand"]), (fname, r, c1 - c0, len(exp["strand"]))
            for c in range(c1 - c0):
                a, b = int(out["match_off"][c0 + c]), int(out["match_off"][c0 + c + 1])
                ea, eb = int(exp["off"][c]), int(exp["off"][c + 1])
                assert np.array_equal(out["q"][a:b], exp["q"][ea:eb]) and np.array_equal(out["t"][a:b], exp["t"][ea:eb]), (fname, r, c)
                assert out["box"][c0 + c].tolist() == exp["box"][c].tolist() and out["strand"][c0 + c] == exp["strand"][c] and out["chrom"][c0 + c] == exp["chrom"][c], (fname, r, c)
                assert np.float32(out["freq"][c0 + c]).view(np.uint32) == np.float32(exp["freq"][c]).view(np.uint32), (fname, r, c)
                n_cl += 1
        assert n_cl > 50 and n_skip * 20 <= len(reads), (fname, n_cl, n_skip)


# ---- LinearExtend
XK = 17
XCH = [0, 10_000, 20_000]
XSIZES = [2, 63, 64, 65, 128, 129, 200]          # (a cluster of one match cannot leave the clean stage: a run has two)


def _extend_case(rng, genome, n, strand, chrom, mode):
    """One read holding one cluster of n matches -> (read bytes, q, t global).  mode: 'mixed' (every kind of pair; diagonal changes at the pairs tested by lanes 63 and 0),
    'none' (one diagonal, every walk completes), 'all' (a diagonal change at every pair).  The first match sits at q == 0, the last at q + K == readLen; the forward
    cluster ends at t + K == chromLen, the reverse one at t == 0."""
    G = genome[XCH[chrom]:XCH[chrom + 1]]
    kinds = []
    for i in range(1, n):
        if mode == "none":
            kinds.append(("walk", "walk0")[i % 2])
        elif mode == "all":
            kinds.append("diag")
        elif i % 64 in (0, 63):
            kinds.append("diag")
        else:
            kinds.append(("walk", "mm_before", "overlap", "walk0", "mm_first", "walk", "mm_mid", "diag", "walk", "mm_on")[(i + n) % 10])
    q = [0]; cum = [0]
    for kd in kinds:
        gap = {"overlap": int(rng.integers(1, XK)), "walk0": XK, "diag": int(rng.integers(1, 30))}.get(kd, XK + int(rng.integers(2, 12)))
        q.append(q[-1] + gap)
        cum.append(cum[-1] + (int(rng.integers(1, 4)) if kd == "diag" else 0))
    q = np.asarray(q, np.int64); cum = np.asarray(cum, np.int64)
    RL = int(q[-1]) + XK
    L = len(G)
    if strand == 0:
        t = q + (L - XK - q[-1] + cum[-1]) - cum                           # q - t rises with cum; the last match ends the chromosome
    else:
        t = (q[-1] - cum[-1] + cum) - q                                    # q + t rises with cum; the last match has t == 0
    assert t.min() >= 0 and t.max() + XK <= L and len(set(zip(q.tolist(), t.tolist()))) == n
    read = rng.integers(0, 4, RL)
    other = lambda b: (b + 1 + int(rng.integers(0, 3))) % 4
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    g = np.vectorize(code.get)(G)
    for i, kd in enumerate(kinds, start=1):
        q1, t1, q2 = int(q[i - 1]), int(t[i - 1]), int(q[i])
        if kd == "diag" or kd == "overlap":
            continue
        for j in range(q2 - (q1 + XK) + 1):                               # the walk's own comparison: G[t1 + K + j] forward, G[t1 - 1 - j] reverse, against R[q1 + K + j]
            tt = t1 + XK + j if strand == 0 else t1 - 1 - j
            if 0 <= tt < L and q1 + XK + j < RL:
                read[q1 + XK + j] = g[tt]
        plant = {"mm_before": q2 - 1, "mm_first": q1 + XK, "mm_mid": (q1 + XK + q2) // 2, "mm_on": q2}.get(kd)
        if plant is not None and plant < RL:
            tt = t1 + XK + (plant - q1 - XK) if strand == 0 else t1 - 1 - (plant - q1 - XK)
            if 0 <= tt < L:
                read[plant] = other(int(g[tt]))
    rb = np.frombuffer(b"ACGT", np.uint8)[read]
    p = rng.permutation(n)
    return rb, q[p].astype(np.uint32), (t[p] + XCH[chrom]).astype(np.uint32)


@pytest.mark.gpu
def test_hip_linear_extend_crafted(ctx, oracle):
    """linear_extend_kernel against the oracle on clusters whose pairs overlap, walk to the next match, stop at a planted mismatch (first base, middle, one before the
    next match, on it) or change diagonal -- at lanes 0 and 63 of a chunk, nowhere, everywhere -- on both strands and chromosomes, with matches at q == 0, q + K == readLen,
    t == 0 and t + K == chromLen.  (Under those bounds no walk is clipped by the read or chromosome end before it meets the next match, and a reverse match at
    t == 0 has no same-diagonal successor: the clips of Checkbp are met at equality only.)"""
    from lra_amd import seed, cluster
    rng = np.random.default_rng(77)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, XCH[-1])]
    ctx.check(ctx.lib.lra_ctx_load_genome(ctx.h, genome.ctypes.data, len(genome)))
    cases = [(n, st, (i + st) % 2, "mixed") for i, n in enumerate(XSIZES) for st in (0, 1)]
    cases += [(n, st, st, mode) for n in (65, 129) for st in (0, 1) for mode in ("none", "all")]
    built = [_extend_case(rng, genome, *c) for c in cases]
    reads = [(q, t, np.arange(len(q), dtype=np.uint64) + np.uint64(1), len(q) if c[1] == 0 else 0) for c, (rb, q, t) in zip(cases, built)]
    batch = seed.ReadBatch(ctx, [rb.tobytes() for rb, _, _ in built])
    _inject(ctx, reads)
    copts = dict(O.CLEAN_PRESETS["ONT"], globalK=XK, minDiagCluster=2)
    out = cluster.fetch(ctx, cluster.clean_matches_batch(ctx, cluster.CleanOpts(**copts), XCH))
    eo = cluster.fetch_extend(ctx, cluster.linear_extend_batch(ctx, XK, batch))
    n_anchor = n_merged = 0
    for r, (c, (rb, q, t)) in enumerate(zip(cases, built)):
        c0, c1 = int(out["cluster_off"][r]), int(out["cluster_off"][r + 1])
        assert c1 - c0 == 1 and int(out["end"][c0]) - int(out["start"][c0]) == c[0], (r, c)     # the crafted cluster came through the clean stage whole
        x = c0
        a, b = int(out["start"][x]), int(out["end"][x])
        ch = int(out["chrom"][x]); off = XCH[ch]
        assert ch == c[2] and int(out["strand"][x]) == c[1]
        eq, et, el, box = O.linear_extend(out["cl_qpos"][a:b], out["cl_tpos"][a:b] - np.uint32(off), c[1], XK, rb.tobytes(), genome[off:XCH[ch + 1]].tobytes())
        es, ec = int(eo["e_start"][x]), int(eo["e_count"][x])
        assert ec == len(eq), (r, c, ec, len(eq))
        assert np.array_equal(eo["e_qpos"][es:es + ec], eq) and np.array_equal(eo["e_tpos"][es:es + ec], et + np.uint32(off)) and np.array_equal(eo["e_len"][es:es + ec], el), (r, c)
        assert eo["box"][x].tolist() == [int(box[0]), int(box[1]), int(box[2]) + off, int(box[3]) + off], (r, c)
        if c[3] == "none":
            assert ec == 1 and el[0] == int(q.max()) + XK                   # every walk completed: one anchor over the whole read
        if c[3] == "all":
            assert ec == c[0]
        n_anchor += ec; n_merged += int((el > XK).sum())
    assert n_anchor > 300 and n_merged > 100


# ---- the injection itself
@pytest.mark.gpu
def test_hip_set_matches_roundtrip(ctx, oracle):
    """What lra_seed_set_matches was given comes back from the seed result; a following lra_seed_batch on real reads matches the oracle (the arrays regrow, nothing
    stale stays behind), and so does a larger injection after it."""
    from lra_amd import seed, synth
    from lra_amd._lib import LraError

    def check(reads):
        res, off = _inject(ctx, reads)
        so = seed.fetch(ctx, res)
        assert res.n_reads == len(reads) and res.n_matches == int(off[-1]) and res.n_minimizers == 0
        assert np.array_equal(so["match_off"], off) and so["n_forward"].tolist() == [r[3] for r in reads]
        assert np.array_equal(so["sep_qpos"], np.concatenate([r[0] for r in reads])) and np.array_equal(so["sep_tpos"], np.concatenate([r[1] for r in reads]))

    ctx.release_buffers()
    small = crafted("SMALL")[:12]
    check(small)
    genome = synth.make_genome(120_000, seed=9, repeat_frac=0.3)
    ik, ip = synth.build_global_index(genome, 17, 10, 60)
    rds, _ = synth.simulate_reads(genome, 8, 6000, 1500, 0.05, seed=3)
    seed.load_reference(ctx, genome, ik, ip)
    batch = seed.ReadBatch(ctx, [r.tobytes() for r in rds])
    so = seed.fetch(ctx, seed.seed_batch(ctx, batch, 17, 10, 150))
    g = genome.tobytes() + b"\0" * 64
    assert int(so["match_off"][-1]) > 2 * int(sum(len(r[0]) for r in small))                # more matches than the injection left room for
    for r, read in enumerate(rds):
        keys, pos = O.store_minimizers(read.tobytes(), 17, 10)
        sk, sp = O.sort_minimizers(keys, pos)
        qi, ti = O.compare_lists(sk, sp, ik, ip, 150)
        st = O.separate_strand(read.tobytes(), g, 17, sp[qi], ip[ti])
        m0, m1, nf = int(so["match_off"][r]), int(so["match_off"][r + 1]), int(so["n_forward"][r])
        assert nf == int((st == 0).sum()) and m1 - m0 == len(st), r
        for a, b, sel in ((m0, m0 + nf, st == 0), (m0 + nf, m1, st == 1)):
            assert sorted(zip(so["sep_qpos"][a:b].tolist(), so["sep_tpos"][a:b].tolist())) == sorted(zip(sp[qi][sel].tolist(), ip[ti][sel].tolist())), r
    check(crafted("CCS"))                                                                      # larger than anything before: the arrays regrow
    res, _ = _inject(ctx, [])                                                                  # an empty batch: no arrays behind the result
    assert res.n_reads == 0 and res.n_matches == 0
    with pytest.raises(LraError):
        seed.set_matches(ctx, [0, 5, 3], [0, 0], np.zeros(5, np.uint32), np.zeros(5, np.uint32), np.zeros(5, np.uint64))      # offsets decrease
    with pytest.raises(LraError):
        seed.set_matches(ctx, [0, 2], [3], np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(2, np.uint64))            # more forward matches than matches
    with pytest.raises(LraError):
        seed.set_matches(ctx, [1, 2], [0], np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(2, np.uint64))            # does not start at 0
