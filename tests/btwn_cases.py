"""Crafted chains of refined clusters for Refine_Btwnsplitchain (refine_btwn.hip, stage a11) and for the merge / extend / trim pass behind it (merge_extend.hip,
stage a9 / the second a7): a small world (three chromosomes of random bases), a builder that cuts reads out of it and replaces chosen stretches, a description of
a chain as a list of refined clusters in the walk's order, a packer that lays any list of chains out as the arrays the two entry points read, and a registry of
*threshold pairs* -- two cases that differ in one quantity sitting on either side of one comparison, under a name that says which.  Shared by
tests/test_btwn_cases.py, tests/test_refine_btwn_edges.py, tests/test_merge_extend_edges.py and tools/oracle_mutants_btwn.py.  Plain helpers, CPU only, no fixtures.

The box of a cluster is chosen freely; the matches are then put on its corners.  The walk reads the box alone, but every append recomputes the box from all matches
(SetClusterBoundariesFromMatches, Clustering.h:308-322), and the stage's input always has box == bounds(matches) (ChainRefine.h:568), which refine_btwn.hip relies on
(it extends the box instead of recomputing it).  A cluster given explicit `matches` keeps them as they are: padding fragments and clusters nothing is appended to."""
import ctypes as C

import numpy as np

import oracle_lib as O

K, W = 10, 5
CHROM = [0, 30001, 50001, 53001]            # chromosome 1 starts off a 256-base window edge; chromosome 2 is 3000 bases: its end can be reached exactly
GLEN = [CHROM[i + 1] - CHROM[i] for i in range(3)]
ACGT = np.frombuffer(b"ACGT", np.uint8)
GENOME = ACGT[np.random.default_rng(20240611).integers(0, 4, CHROM[-1])]
GBYTES = GENOME.tobytes()
_COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"): _COMP[_a] = _b
OPTS = dict(rsd=10000, sparse=0.01)


def revcomp(a):
    return _COMP[a[::-1]]


def unrelated(n, seed):
    return ACGT[np.random.default_rng(1000 + seed).integers(0, 4, n)]


def chrom_seq(chrom, t0, n):
    """genome[chrom][t0 : t0 + n), unrelated bases where that leaves the chromosome"""
    out = unrelated(n, 7 * t0 + chrom)
    lo, hi = max(t0, 0), min(t0 + n, GLEN[chrom])
    if hi > lo: out[lo - t0:hi - t0] = GENOME[CHROM[chrom] + lo:CHROM[chrom] + hi]
    return out


def compose(L, pieces, seed=1):
    """a read of L bases: unrelated bases, then for every piece (q0, n, chrom, t0, strand) read[q0 : q0 + n) = genome[chrom][t0 : t0 + n), reverse-complemented on
    strand 1 (the piece then aligns to the reverse strand: the reverse-complemented read holds those genome bases at [L - q0 - n, L - q0))"""
    r = unrelated(L, seed)
    for q0, n, chrom, t0, st in pieces:
        assert 0 <= q0 and q0 + n <= L, (q0, n, L)
        s = chrom_seq(chrom, t0, n)
        r[q0:q0 + n] = revcomp(s) if st else s
    return r.tobytes()


# ---- the chain description ----------------------------------------------------------------------------------------------------------------------------------
def cl(box, strand=0, chrom=0, matches=None, nm=2):
    """one refined cluster: box (qStart, qEnd, tStart, tEnd) in forward-read coordinates, t relative to its chromosome.  matches None: nm matches spanning the box
    exactly (two on its corners, the rest on the line between them); a list: those, whatever the box says"""
    qs, qe, ts, te = (int(v) for v in box)
    if matches is None:
        assert qe - qs >= K and te - ts >= K and nm >= 2, box
        f = np.linspace(0.0, 1.0, nm)
        mq = (qs + np.floor(f * (qe - K - qs))).astype(np.int64)
        mt = (ts + np.floor(f * (te - K - ts))).astype(np.int64)
        if strand: mt = mt[::-1]
        matches = list(zip(mq.tolist(), mt.tolist()))
    return dict(box=(qs, qe, ts, te), strand=int(strand), chrom=int(chrom), matches=[(int(a), int(b)) for a, b in matches])


def bcase(read, clusters, link=None, **opts):
    """a chain for Refine_Btwnsplitchain: clusters in the walk's order (index 0 is the read's end, q descends), link[nsp - 1], the read, the options"""
    n = len(clusters)
    link = [0] * max(n - 1, 0) if link is None else [int(v) for v in link]
    assert len(link) == max(n - 1, 0)
    o = dict(OPTS); o.update(opts)
    for c in clusters: assert c["box"][0] <= c["box"][1] <= len(read), c["box"]
    return dict(kind="btwn", read=read, clusters=list(clusters), link=link, opts=o)


def mcase(read, clusters):
    """a chain for the merge / extend / trim pass (lra_merge_extend_batch): the clusters are those Refine_Btwnsplitchain would leave"""
    return dict(kind="merge", read=read, clusters=list(clusters), link=[0] * max(len(clusters) - 1, 0), opts=dict(OPTS))


def tcase(q, t, ln, strand):
    """one extended cluster for TrimOverlappedAnchors (lra_trim_overlapped_anchors_batch): anchors given directly"""
    return dict(kind="trim", q=[int(v) for v in q], t=[int(v) for v in t], len=[int(v) for v in ln], strand=int(strand))


def pcase(q, t, ln):
    """one anchor list for the pair version of TrimOverlappedAnchors (lra_trim_anchor_pairs_batch)"""
    return dict(kind="trimpairs", q=[int(v) for v in q], t=[int(v) for v in t], len=[int(v) for v in ln])


def csr(clusters):
    off = [0]; mq = []; mt = []
    for c in clusters:
        mq += [m[0] for m in c["matches"]]; mt += [m[1] for m in c["matches"]]; off.append(len(mq))
    return off, mq, mt


def opts_key(case):
    return (case["opts"]["rsd"], float(np.float32(case["opts"]["sparse"])))


def oracle_btwn(case):
    cls = case["clusters"]
    off, mq, mt = csr(cls)
    rd = np.frombuffer(case["read"], np.uint8)
    return O.refine_btwn_splitchain(off, mq, mt, np.array([c["box"] for c in cls], np.uint32).reshape(-1, 4), [c["strand"] for c in cls], [c["chrom"] for c in cls],
                                    case["link"], case["read"], revcomp(rd).tobytes(), GBYTES, CHROM, K=K, W=W, refineSpaceDist=case["opts"]["rsd"],
                                    anchorstoosparse=float(np.float32(case["opts"]["sparse"])), match=4, mismatch=-1, indel=-2, max_freq=15)


def oracle_merge(case):
    cls = case["clusters"]
    off, mq, mt = csr(cls)
    return O.merge_extend(off, mq, mt, np.array([c["box"] for c in cls], np.uint32).reshape(-1, 4), [c["strand"] for c in cls], [c["chrom"] for c in cls],
                          case["read"], GBYTES, CHROM, K=K)


def oracle_trim(case):
    if case["kind"] == "trim":
        return O.trim_overlapped_anchors(case["q"], case["t"], case["len"], case["strand"])
    L = O.lib()
    Q = np.array(case["q"], np.uint32); T = np.array(case["t"], np.uint32); ln = np.array(case["len"], np.int32)
    L.oracle_trim_anchor_pairs(C.c_int(len(Q)), Q.ctypes.data_as(C.POINTER(C.c_uint32)), T.ctypes.data_as(C.POINTER(C.c_uint32)), ln.ctypes.data_as(C.POINTER(C.c_int)))
    return Q, ln


PAIRS = {}          # name -> (case, case): the oracle's decisions must differ
SINGLES = {}        # name -> case: layouts and paths
SAME = []           # (name, name): singles whose oracle output must be equal


def pair(name, a, b):
    assert name not in PAIRS, name
    PAIRS[name] = (a, b)


def single(name, c):
    assert name not in SINGLES, name
    SINGLES[name] = c
    return c


def build(section):
    """run one section's builder now (the test modules parametrise over the registry, so it exists at collection); a failed search or construction check says where"""
    try: section()
    except Exception as e:
        raise RuntimeError("tests/btwn_cases.py: building %s failed after %d pairs, %d singles (last: %s): %r" % (
            section.__name__, len(PAIRS), len(SINGLES), (list(PAIRS) + list(SINGLES))[-1] if PAIRS or SINGLES else None, e)) from e


def run(case):
    """The oracle's whole output for one case, as a hashable value (None where the reference would read outside its arrays)."""
    k = case["kind"]
    if k == "btwn":
        r = oracle_btwn(case)
        if r is None: return None
        return (r["off"].tobytes(), r["q"].tobytes(), r["t"].tobytes(), r["box"].tobytes(), r["refinespace"].tobytes())
    if k == "merge":
        r = oracle_merge(case)
        return tuple(r[f].tobytes() for f in ("member", "anchor_off", "q", "t", "len", "box", "strand", "chrom"))
    q, ln = oracle_trim(case)
    return (np.asarray(q, np.uint32).tobytes(), np.asarray(ln, np.int32).tobytes())


def decision(case):
    """run() without the echoed coordinates: matches per cluster and flags; groups, anchors per group, lengths, strand, chromosome; trimmed lengths"""
    r = run(case)
    if r is None: return None
    if case["kind"] == "btwn": return (r[0], r[4])
    if case["kind"] == "merge": return (r[0], r[1], r[4], r[6], r[7])
    return (r[1],)


def all_cases():
    """[(name, case)]: both sides of every pair, then the singles"""
    out = []
    for n, (a, b) in PAIRS.items(): out += [(n + "/a", a), (n + "/b", b)]
    out += list(SINGLES.items())
    return out


def added(case):
    """per cluster: the matches the oracle appended, as [(q, t)] in order"""
    r = oracle_btwn(case)
    out = []
    for k, c in enumerate(case["clusters"]):
        a, b = int(r["off"][k]) + len(c["matches"]), int(r["off"][k + 1])
        out.append(list(zip(r["q"][a:b].tolist(), r["t"][a:b].tolist())))
    return out


# ---- Refine_Btwnsplitchain: two clusters and the gap between them -------------------------------------------------------------------------------------------
# Only the gap's read bases and the target range a problem is given decide what RefineSpace finds; the clusters' own bases are never read.  So a case is two (or
# more) boxes and a `fill`: read[qs : qe) copied from the target range a problem will look at, on that problem's strand.  Everything else in the read is unrelated.
L0 = 1300                                   # cur covers q [0, 400), prev q [800, 1300): no space beyond either end of the read
CQ, PQ = (0, 400), (800, 1300)


def gap2(cur_t, prev_t, cst=0, pst=0, link=0, fill=(), chrom=0, pchrom=None, cur_q=CQ, prev_q=PQ, L=L0, cur_m=None, prev_m=None, seed=1, **opts):
    """chain [prev, cur]: prev is cluster 0 (the read's end), cur cluster 1; fill: compose() pieces"""
    prev = cl(prev_q + tuple(prev_t), pst, chrom if pchrom is None else pchrom, matches=prev_m)
    cur = cl(cur_q + tuple(cur_t), cst, chrom, matches=cur_m)
    return bcase(compose(L, fill, seed), [prev, cur], [link], **opts)


def dense(qs, n, chrom, ts, st):
    """the piece that makes the problem (q [qs, qs + n) of the forward read, target [ts, ts + n), strand st) find every minimizer"""
    return (qs, n, chrom, ts, st)


def first(ok, cands):
    """the first candidate that satisfies ok (the search is deterministic: the world is seeded)"""
    for c in cands:
        if ok(c): return c
    raise AssertionError("no candidate")


def _gap_loop():
    for st in (0, 1):
        z = "s%d" % st
        # same strand, link 0.  Strand 0 chains descend on the target too (cur below prev), strand 1 chains ascend (cur above prev); the other order is the other arm
        lo, hi = (5000, 5400), (5800, 6300)
        f = [dense(400, 400, 0, 5400, st)]
        below = lambda dc=(0, 0), dp=(0, 0), **kw: gap2((lo[0] + dc[0], lo[1] + dc[1]), (hi[0] + dp[0], hi[1] + dp[1]), st, st, 0, f, **kw)     # cur below prev
        above = lambda dc=(0, 0), dp=(0, 0), **kw: gap2((hi[0] + dc[0], hi[1] + dc[1]), (lo[0] + dp[0], lo[1] + dp[1]), st, st, 0, f, **kw)     # cur above prev
        pair("gap.cur_empty/" + z, below(), below(cur_m=[]))
        pair("gap.prev_empty/" + z, below(), below(prev_m=[]))
        pair("gap.qe<=qs/" + z, below(cur_q=(0, 780)), below(cur_q=(0, 800)))                       # a read gap of 20 against none
        pair("gap.same0.cur.tEnd<=prev.tStart/" + z, below(dc=(0, 300)), below(dc=(0, 401)))        # a target gap of 100 against an overlap of 1 (at 0 `te1 <= ts1` skips)
        pair("gap.same0.cur.tStart>prev.tEnd/" + z, above(dc=(-300, 0)), above(dc=(-400, 0)))       # a target gap of 100 against none: the third arm skips
        pair("gap.te1<=ts1/" + z, below(dc=(0, 300)), below(dc=(0, 400)))                           # a target of 100 against 0
        f1 = [dense(400, 400, 0, 5400 if st == 0 else 4600, st)]                                      # what problem 1 of the inversion arm looks at
        pair("gap.diff0.plans_nothing/" + z, gap2(lo, hi, st, 1 - st, 1, f1), gap2(lo, hi, st, 1 - st, 0, f1))
        pair("gap.chrom/" + z, below(), below(pchrom=1))
        # te1 >= glen on chromosome 2 (3000 bases): prev starts at 2999 | 3000
        g2 = [dense(400, 400, 2, 2600, st)]
        end2 = lambda te: (gap2((2200, 2600), (te, te + 300), st, st, 0, g2, chrom=2) if st == 0 else gap2((te, te + 300), (2200, 2600), st, st, 0, g2, chrom=2))
        pair("gap.te1>=glen/" + z, end2(2999), end2(3000))
        # SpaceLength: the read gap is the longer side
        def tiny(n, t0):                                                                             # a gap of n on both sides, its bases from [t0, t0 + n)
            return gap2((t0 - 400, t0), (t0 + n, t0 + n + 500), st, st, 0, [dense(800 - n, n, 0, t0, st)], cur_q=(0, 800 - n))
        t20 = first(lambda t0: sum(len(a) for a in added(tiny(20, t0))) > 0, range(5400, 5500))    # twenty bases that hold a shared minimizer
        pair("gap.space>=20/" + z, tiny(20, t20), tiny(19, t20))
        pair("gap.space<=RSD/" + z, below(rsd=400), below(cur_q=(0, 399), rsd=400))                                  # 400 | 401
        pair("gap.space<=RSD.target/" + z, below(rsd=400), below(dc=(0, -1), rsd=400))                               # the target side 400 | 401
    # strands differ, link 1 (an inversion): problem 1 continues cur, problem 2 continues prev.  p1 / p2: which problem the gap's bases answer
    G = 400
    for st1 in (0, 1):
        z = "st1=%d" % st1
        st2 = 1 - st1
        for geo in ("below", "above"):          # cur.tEnd <= prev.tStart | cur.tStart > prev.tEnd
            ct, pt = ((5000, 5400), (7000, 7500)) if geo == "below" else ((7000, 7400), (5000, 5500))
            t1 = ct[1] if st1 == 0 else ct[0] - G                                       # problem 1: [cur.tEnd, + gap) | [cur.tStart - gap, cur.tStart)
            t2 = (pt[1] if geo == "below" else ct[0] - G) if st1 == 0 else pt[0] - G   # problem 2: st1 0: [prev.tEnd, + gap) | [cur.tStart - gap, ..); st1 1: below prev.tStart
            def inv(which=1, ct=ct, pt=pt, t1=t1, t2=t2, **kw):
                fill = [dense(400, G, 0, t1, st1)] if which == 1 else [dense(400, G, kw.get("pchrom", 0), t2, st2)]     # problem 2 looks at prev's chromosome
                return gap2(ct, pt, st1, st2, 1, fill, **kw)
            y = "%s/%s" % (geo, z)
            for w in (1, 2):
                pair("gap.diff1.p%d_appends/%s" % (w, y), inv(which=w), gap2(ct, pt, st1, st2, 1, []))
                pair("gap.diff1.link/%s/p%d" % (y, w), inv(which=w), dict(inv(which=w), link=[0]))
                pair("gap.diff1.space<=RSD/%s/p%d" % (y, w), inv(which=w, rsd=400), inv(which=w, rsd=399))
                pair("gap.diff1.chrom/%s/p%d" % (y, w), inv(which=w), inv(which=w, pchrom=1))
        # the arm boundaries: cur [5000, 5400), prev starting at 5400 | 5399 (below at equality, then neither); prev ending at 4999 | 5000 (above, then neither)
        for w in (1, 2):
            at = lambda ps, w=w: gap2((5000, 5400), (ps, ps + 500), st1, st2, 1, [dense(400, G, 0, 5400 if st1 == 0 else 4600, st1)] if w == 1 else
                                      [dense(400, G, 0, ps + 500 if st1 == 0 else ps - G, st2)])
            pair("gap.diff1.cur.tEnd<=prev.tStart/%s/p%d" % (z, w), at(5400), at(5399))
            ab = lambda pe, w=w: gap2((5000, 5400), (pe - 500, pe), st1, st2, 1, [dense(400, G, 0, 5400 if st1 == 0 else 4600, st1)] if w == 1 else
                                      [dense(400, G, 0, 4600 if st1 == 0 else pe - 500 - G, st2)])
            pair("gap.diff1.cur.tStart>prev.tEnd/%s/p%d" % (z, w), ab(4999), ab(5000))
    # the clamps te > gap ? te - gap : 0 at the start of chromosome 0: te = gap + 1 | gap | gap - 1 give ts = 1 | 0 | 0
    for d in (1, 0, -1):
        te = G + d
        single("gap.diff1.clamp.te1=gap%+d" % d, gap2((te, te + 400), (7000, 7500), 1, 0, 1, [dense(400, G, 0, max(te - G, 0), 1)]))
        single("gap.diff1.clamp.te2=gap%+d" % d, gap2((5000, 5400), (te, te + 500), 1, 0, 1, [dense(400, G, 0, max(te - G, 0), 0)]))
        single("gap.diff1.clamp.above.te2=gap%+d" % d, gap2((te, te + 400), (te + 600, te + 1100), 0, 1, 1, [dense(400, G, 0, max(te - G, 0), 1)]))
        single("gap.same1.clamp.te2=gap%+d/s0" % d, gap2((te + 300, te + 700), (te, te + 500), 0, 0, 1, [dense(400, G, 0, max(te - G, 0), 0)]))
        single("gap.same1.clamp.te1=gap%+d/s1" % d, gap2((te, te + 400), (te + 100, te + 600), 1, 1, 1, [dense(400, G, 0, max(te - G, 0), 1)]))
    # SpaceLength >= 20 for the second problem: a gap of 20 | 19 whose bases continue prev (strand 1) beyond its target end
    def tiny2(n, pe):
        return gap2((5000, 5400), (pe - 500, pe), 0, 1, 1, [dense(800 - n, n, 0, pe, 1)], cur_q=(0, 800 - n))
    pe20 = first(lambda pe: len(added(tiny2(20, pe))[0]) > 0, range(7500, 7600))
    pair("gap.diff1.space>=20/p2", tiny2(20, pe20), tiny2(19, pe20))
    # the 5 RSD exit of the first problem skips the second as well: RSD 100, a gap of 499 | 500 whose bases continue prev
    for g in (499, 500):
        single("gap.diff1.space>=5RSD.%d" % g, gap2((5000, 5400), (7000, 7500), 0, 1, 1, [dense(400, g, 0, 7500, 1)], prev_q=(400 + g, 900 + g), L=900 + g, rsd=100))
    # te2 <= ts2: problem 2 ends at prev.tStart = 0 (st1 = 1) | 30
    pair("gap.diff1.te2<=ts2", gap2((5000, 5400), (30, 530), 1, 0, 1, [dense(400 + G - 30, 30, 0, 0, 0)]), gap2((5000, 5400), (0, 500), 1, 0, 1, [dense(400 + G - 30, 30, 0, 0, 0)]))
    # te2 >= glen: problem 2 = [prev.tEnd, prev.tEnd + gap) on chromosome 2, prev ending at 2599 | 2600
    e2 = lambda pe: gap2((1000, 1400), (pe - 500, pe), 0, 1, 1, [dense(400, G, 2, pe, 1)], chrom=2)
    pair("gap.diff1.te2>=glen", e2(2599), e2(2600))
    # te1 >= glen skips problem 2 as well: cur ending at 2599 | 2600 below a prev that problem 2 would extend
    e1 = lambda ce: gap2((ce - 400, ce), (ce + 1, ce + 301), 1, 0, 1, [dense(400, G, 2, ce + 1 - G, 0)], chrom=2)
    single("gap.diff1.te1<glen.p2_runs", e1(2600))
    # same strand, link 1 (a tandem duplication): strand 0 needs cur.tEnd > prev.tStart, strand 1 cur.tStart < prev.tEnd
    for w in (1, 2):
        d0 = lambda ce, w=w: gap2((ce - 400, ce), (5400, 5900), 0, 0, 1, [dense(400, G, 0, ce, 0)] if w == 1 else [dense(400, G, 0, 5400 - G, 0)])
        pair("gap.same1.cur.tEnd>prev.tStart/s0/p%d" % w, d0(5401), d0(5400))
        d1 = lambda cs, w=w: gap2((cs, cs + 400), (4900, 5400), 1, 1, 1, [dense(400, G, 0, cs - G, 1)] if w == 1 else [dense(400, G, 0, 5400, 1)])
        pair("gap.same1.cur.tStart<prev.tEnd/s1/p%d" % w, d1(5399), d1(5400))
        pair("gap.same1.link/s0/p%d" % w, d0(5600), dict(d0(5600), link=[0]))
        pair("gap.same1.link/s1/p%d" % w, d1(5200), dict(d1(5200), link=[0]))
        pair("gap.same1.space<=RSD/s0/p%d" % w, dict(d0(5600), opts=dict(OPTS, rsd=400)), dict(d0(5600), opts=dict(OPTS, rsd=399)))
        pair("gap.same1.space<=RSD/s1/p%d" % w, dict(d1(5200), opts=dict(OPTS, rsd=400)), dict(d1(5200), opts=dict(OPTS, rsd=399)))


build(_gap_loop)


# ---- the two end rounds -------------------------------------------------------------------------------------------------------------------------------------
def end1(st, end, gap, T, fill=None, chrom=0, L=900, shift=0, **opts):
    """a chain of one cluster with `gap` read bases beyond one end only.  end "first": beyond cluster 0 (q [L - gap, L)); "last": before the last one (q [0, gap)).
    T: the cluster's target side the round starts from -- tEnd where the target continues upward (strand 0 first, strand 1 last: [T, T + gap) and 500 more),
    tStart where it continues downward (strand 1 first, strand 0 last: [T - gap, T) and up to 500 before).  fill None: the gap's bases from that range moved down by
    `shift`"""
    up = (st == 0) == (end == "first")
    q = (0, L - gap) if end == "first" else (gap, L)
    t = (T - 300, T) if up else (T, T + 300)
    q0 = L - gap if end == "first" else 0
    if fill is None: fill = [dense(q0, gap, chrom, (T if up else max(T - gap, 0)) - shift, st)] if gap else []
    return bcase(compose(L, fill), [cl(q + t, st, chrom)], [], **opts)


def _ends():
    for st in (0, 1):
        for end in ("first", "last"):
            z = "%s/s%d" % (end, st)
            up = (st == 0) == (end == "first")
            e = lambda gap, T=5000, **kw: end1(st, end, gap, T, **kw)
            pair("end.qe>qs/" + z, e(30), e(0))
            t20 = first(lambda T: sum(len(a) for a in added(e(20, T))) > 0, range(5000, 5100))
            pair("end.space>=20/" + z, e(20, t20), e(19, t20))
            pair("end.space<RSD/" + z, e(299, rsd=300), e(300, rsd=300))                                     # strict, unlike the gap loop's
            single("end.space<RSD.at_RSD/" + z, e(300, rsd=300))
            pair("end.empty/" + z, e(200), e(200, fill=[]))
            # te + 500 < glen on chromosome 2: te = 2499 | 2500
            if up: pair("end.te+500<glen/" + z, e(200, 2299, chrom=2), e(200, 2300, chrom=2))
            else:
                pair("end.te+500<glen/" + z, e(200, 2499, chrom=2), e(200, 2500, chrom=2))
                # ts > 500 gives the target 500 more bases in front (lrts = lrlength = 500): ts = 501 | 500, the gap's bases from 60 below the plain range
                pair("end.ts>500/" + z, e(200, 701, shift=60), e(200, 700, shift=60))
                # te against the gap at the start of the chromosome: te = gap + 1 gives ts = 1; te = gap plans nothing at the first end (strand 1) and
                # gives ts = 0 at the last (strand 0); te = gap - 1 is clamped there
                if end == "first": pair("end.te<=gap/" + z, e(200, 201), e(200, 200))
                else:
                    for d in (1, 0, -1): single("end.clamp.te=gap%+d/%s" % (d, z), e(200, 200 + d))
            # any non-empty result is appended and sets refinespace, however sparse: one island of 50 bases under anchorstoosparse 0.2
            pair("end.sparse_appends/" + z, e(200, sparse=0.2, fill=[dense((700 if end == "first" else 0) + 60, 50, 0, 5060 if up else 4860, st)]),
                 e(200, sparse=0.2, fill=[]))
            # RefineSpace's class from here: the target is gap + 500 long, the query stays short
            for g in (499, 500, 501): single("end.class.target=%d/%s" % (g + 500, z), e(g, L=1400))


build(_ends)


# ---- what is done with a result -----------------------------------------------------------------------------------------------------------------------------
def sgap(st, g, isl=(), whole=False, tg=None, **kw):
    """same strand, link 0, a read gap of g and a target gap of tg (default g).  isl: islands (o, n, d) in the problem's own coordinates (strand 1: those of the
    reverse-complemented read): n target bases from offset o copied to query offset o + d, so the island lies on diagonal t - q = -d.  whole: the whole gap copied"""
    tg = g if tg is None else tg
    if whole: isl = [(0, min(g, tg), 0)]
    if st == 0:
        cur_t, prev_t = (5000, 5400), (5400 + tg, 5900 + tg)
        fill = [(400 + o + d, n, 0, 5400 + o, 0) for o, n, d in isl]
    else:
        cur_t, prev_t = (5400 + tg, 5800 + tg), (4900, 5400)
        fill = [(400 + g - (o + d) - n, n, 0, 5400 + o, 1) for o, n, d in isl]
    return gap2(cur_t, prev_t, st, st, 0, fill, prev_q=(400 + g, 900 + g), L=900 + g, **kw)


def found(case):
    """every pair RefineSpace finds in the gap of a two-cluster chain, sorted by (q, t) as CartesianSort leaves them: the case under a tiny anchorstoosparse"""
    a = added(dict(case, opts=dict(case["opts"], sparse=1e-9)))
    return sorted(a[0] + a[1])


def widest_step(case):
    """(|dq|, |dt|) of the widest step between neighbours of the sorted result"""
    P = found(case)
    return max(((abs(b[0] - a[0]), abs(b[1] - a[1])) for a, b in zip(P, P[1:])), key=min)


def run_dists(case, st):
    """(dist_cur, dist_prev) of append_to_closetcluster (ChainRefine.h:22-56) for the whole result of a two-cluster chain taken as one run"""
    P = found(case)
    if not P: return (-1, -2)
    qS, qE = min(p[0] for p in P), max(p[0] for p in P) + K
    tS, tE = min(p[1] for p in P), max(p[1] for p in P) + K
    pq, _, pts, pte = case["clusters"][0]["box"]; _, cqe, cts, cte = case["clusters"][1]["box"]
    pos = lambda v: max(v, 0)
    if st == 0: return max(pos(qS - cqe), pos(tS - cte)), max(pos(pq - qE), pos(pts - tE))
    return max(pos(qS - cqe), pos(cts - tE)), max(pos(pq - qE), pos(tS - pte))


def f32_above(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def _results():
    for st in (0, 1):
        z = "s%d" % st
        pair("res.empty/" + z, sgap(st, 400, whole=True), sgap(st, 400))
        # eff >= 2 anchorstoosparse at equality: n pairs over a span of 512 are exact in float32, and so is n / 1024
        n = len(found(sgap(st, 512, whole=True)))
        assert n > 20
        pair("res.eff>=2sparse/" + z, sgap(st, 512, whole=True, sparse=n / 1024.0), sgap(st, 512, whole=True, sparse=f32_above(n / 1024.0)))
        one = sgap(st, 512, [(0, 505, 0)])
        if len(found(one)) == n - 1:                                                     # one pair fewer under the same threshold
            pair("res.eff>=2sparse.one_fewer/" + z, sgap(st, 512, whole=True, sparse=n / 1024.0), dict(one, opts=dict(OPTS, sparse=n / 1024.0)))
        # the run cut min(|dq|, |dt|) <= 200: two islands of six pairs each, the step between them 200 | 201 on the read (d = -40: 40 more on the target) and on the
        # target (d = +40: 40 more on the read)
        for co, sg in (("dq", -1), ("dt", 1)):
            ix = 0 if co == "dq" else 1
            two = lambda od: sgap(st, 460, [(20, 60, 0), (od[0], 60, od[1])], sparse=0.2)
            def at(v):                                                                    # (the pairs sit on the aligner's blocks: they do not move base by base)
                return first(lambda od: widest_step(two(od))[ix] == v and widest_step(two(od))[1 - ix] > v + 20, [(o, sg * d) for d in range(40, 50) for o in range(250, 330)])
            pair("res.cut<=200.%s/%s" % (co, z), two(at(200)), two(at(201)))
        # a run needs four pairs
        cnt = lambda n: len(found(sgap(st, 400, [(100, n, 0)])))
        n4 = first(lambda n: cnt(n) == 4, range(30, 70))
        assert cnt(n4 - 1) == 3
        pair("res.run>=4/" + z, sgap(st, 400, [(100, n4, 0)], sparse=0.2), sgap(st, 400, [(100, n4 - 1, 0)], sparse=0.2))
        # dist_cur <= dist_prev: one run, prev.qStart (and its target side) moved until both distances are equal, then one further either way
        def tie(dg):
            return sgap(st, 300 + dg, [(100, 60, 0)], sparse=0.2)
        rel = lambda fn, d: first(lambda dg: run_dists(fn(dg), st)[1] - run_dists(fn(dg), st)[0] == d and run_dists(fn(dg), st)[0] > 0, range(-60, 150))
        pair("res.dist_cur<=dist_prev/" + z, tie(rel(tie, 0)), tie(rel(tie, -1)))          # equal: cur; prev nearer by one: prev
        single("res.dist_cur<dist_prev/" + z, tie(rel(tie, 1)))
        # the same with the two distances decided on the target: the island lies off the diagonal
        for d in (20, -20):
            tie_t = lambda v, d=d: sgap(st, 300 + v[0], [(v[1], 60, d)], sparse=0.2)
            diff = lambda v, by: run_dists(tie_t(v), st)[1] - run_dists(tie_t(v), st)[0] == by and run_dists(tie_t(v), st)[0] > 0
            cands = [(dg, o) for o in (100, 90, 110, 80, 120) for dg in range(-60, 150)]
            pair("res.dist_cur<=dist_prev.target%+d/%s" % (d, z), tie_t(first(lambda v: diff(v, 0), cands)), tie_t(first(lambda v: diff(v, -1), cands)))
        # refinespace: set by the dense append, not by the sparse one (the same result under anchorstoosparse 0.01 | 0.2)
        pair("res.refinespace.dense|sparse/" + z, sgap(st, 400, whole=True), sgap(st, 400, whole=True, sparse=0.2))
        # max(gap, te - ts) >= 5 RSD leaves the iteration; below it `SpaceLength <= RSD` refuses the problem all the same: RSD 100, a space of 499 | 500
        for g in (499, 500): single("gap.space>=5RSD.%d/%s" % (g, z), sgap(st, g, whole=True, rsd=100))
        # several runs of one result: to different clusters, and the second seeing the box the first moved.  A (near cur) and a middle run M that is nearer to prev
        # than to cur's old box but nearer to cur once A has moved cur's box; with A one pair short (three: no run), M goes to prev
        single("res.runs.two_clusters/" + z, sgap(st, 900, [(20, 60, 0), (800, 60, 0)], sparse=0.2))
        mid = lambda nA: sgap(st, 900, [(20, nA, 0), (470, 60, 0)], sparse=0.2)
        pair("res.runs.second_sees_moved_box/" + z, mid(300), mid(n4 - 1))
        # RefineSpace's class from here: query and target 999 | 1000, and the target alone
        for g in (999, 1000, 1001): single("res.class.q=t=%d/%s" % (g, z), sgap(st, g, whole=True))
        single("res.class.q=999.t=1000/" + z, sgap(st, 999, whole=True, tg=1000))
        single("res.class.q=1000.t=999/" + z, sgap(st, 1000, whole=True, tg=999))
        # space_diag: floor(max(100, 0.15f (qe - qs))) capped at 1000 is the band of the long class (a target of 1000 or more): 673 | 674 bases give 100 | 101,
        # 6666 | 6667 give 999 | 1000.  One island on diagonal t - q = -101 | -1000, the lower edge of the band
        for lo, D in ((673, 101), (6666, 1000)):
            assert int(np.floor(max(np.float32(100), np.float32(0.15) * np.float32(lo)))) == D - 1 and int(np.floor(np.float32(0.15) * np.float32(lo + 1))) == D
            band = lambda g: sgap(st, g, [(200, 60, D)], tg=g + 1100, sparse=1e-6)
            pair("diag.%d|%d/%s" % (D - 1, D, z), band(lo + 1), band(lo))
    # two blocks: a sparse first problem is dropped, at the same equality; a sparse second problem is appended
    for st1 in (0, 1):
        z = "st1=%d" % st1
        G = 512
        t1 = 5400 if st1 == 0 else 5000 - G
        inv = lambda fill, **kw: gap2((5000, 5400), (7000, 7500), st1, 1 - st1, 1, fill, prev_q=(400 + G, 900 + G), L=900 + G, **kw)
        n = len(found(inv([dense(400, G, 0, t1, st1)])))
        pair("res.two.eff>=2sparse/" + z, inv([dense(400, G, 0, t1, st1)], sparse=n / 1024.0), inv([dense(400, G, 0, t1, st1)], sparse=f32_above(n / 1024.0)))
        t2 = 7500 if st1 == 0 else 7000 - G
        isl2 = [dense(400 + 200, 60, 0, t2 + (200 if st1 == 1 else G - 260), 1 - st1)]
        pair("res.two.second_appends_sparse/" + z, inv(isl2, sparse=0.2), inv([], sparse=0.2))


build(_results)


# ---- order: what a gap reads after the gap before it ----------------------------------------------------------------------------------------------------------
# Gap c reads prev = cluster c - 1, to which gap c - 1 may have appended as ITS cur.  Whatever gap c - 1 finds lies between clusters c - 2 and c - 1 on the read, so with
# box == bounds(matches) it can raise prev.qEnd, never move prev.qStart: `qe` of gap c and its `qe <= qs` test cannot change.  On the target it moves prev.tEnd (a
# chain that descends there) or prev.tStart (problem 1 of an inversion, which looks below cur.tStart), and those gap c does read.  A run given to prev, or an append
# to the last cluster, moves the target side the end rounds start from when the chain runs the other way on the target (strand 0 ascending, strand 1 descending).
Q3 = ((1400, 1700), (700, 1000), (0, 300))            # c0, c1, c2 on the read; gap 1 = q [1000, 1400), gap 2 = q [300, 700)


def chain3(t, st=(0, 0, 0), link=(0, 0), fill=(), L=1700, nm=(2, 2, 2), **opts):
    return bcase(compose(L, fill), [cl(Q3[i] + tuple(t[i]), st[i], 0, nm=nm[i]) for i in range(3)], link, **opts)


def gap2_added(case):
    """what clusters 1 and 2 of a three-cluster chain received after gap 1 (gap 2's doing, given that gap 1 appends to cluster 1 only, and dense)"""
    a = added(case)
    return a[2], [p for p in a[1] if p[0] < Q3[1][0]]


def fresh(case):
    """the case, after checking that gap 2 planned on the boxes as they were before gap 1 would give something else: clusters 1 and 2 alone, same read"""
    stale = added(dict(case, clusters=case["clusters"][1:], link=case["link"][1:]))
    now = gap2_added(case)
    assert (stale[1], [p for p in stale[0] if p[0] < Q3[1][0]]) != now, "gap 2 does not depend on gap 1 here"      # (cluster 1 is the sub-chain's read end)
    return case


def _order():
    g1 = dense(1000, 400, 0, 5300, 0)                 # gap 1 = target [5300, 5700): appended to c1, whose tEnd goes from 5300 to about 5700
    # (a) gap 2's target starts at prev.tEnd: c2 lies above c1 on the target, so gap 2 is [c1.tEnd, 6100)
    t = ((5700, 6000), (5000, 5300), (6100, 6400))
    g2 = [dense(300, 200, 0, 5300, 0), dense(500, 200, 0, 5900, 0)]      # the first piece answers only the range gap 2 would have had without gap 1
    pair("order.gap2.ts1_moves", fresh(chain3(t, fill=[g1] + g2)), chain3(t, fill=g2))
    # (a) the same move takes gap 2 from the second arm (c2.tStart 5500 > c1.tEnd 5300) to the third (an overlap: skipped)
    t = ((5700, 6000), (5000, 5300), (5500, 5800))
    g2 = dense(300, 200, 0, 5300, 0)
    pair("order.gap2.arm_flips_to_skip", fresh(chain3(t, fill=[g1, g2])), chain3(t, fill=[g2]))
    # (a) an inversion's problem 1 lowers c1.tStart (c1 on strand 1: [c1.tStart - 400, c1.tStart)); gap 2 (strand 1, link 0, c2 below c1) ends at c1.tStart
    t = ((9000, 9300), (6000, 6300), (5000, 5300))
    i1 = dense(1000, 400, 0, 5600, 1)
    g2 = dense(300, 400, 0, 5300, 1)
    pair("order.gap2.te1_moves", fresh(chain3(t, (0, 1, 1), (1, 0), [i1, g2])), chain3(t, (0, 1, 1), (1, 0), [g2]))
    # (a) the append grows only sides gap 2 does not read (everything descends: gap 2 reads c1.qStart and c1.tStart): gap 2 finds the same with and without it
    t = ((5700, 6000), (5000, 5300), (4300, 4600))
    g2 = dense(300, 400, 0, 4600, 0)
    single("order.unread_sides.with", chain3(t, fill=[g1, g2])); single("order.unread_sides.without", chain3(t, fill=[g2]))
    # (a) the same lowering takes gap 2 from the first arm (c2.tEnd 5700 <= c1.tStart 6000) to neither (c1.tStart is 5600 afterwards, c2 does not lie above c1)
    t = ((9000, 9300), (6000, 6300), (5400, 5700))
    pair("order.gap2.first_arm_flips_to_skip", fresh(chain3(t, (0, 1, 1), (1, 0), [i1, dense(300, 300, 0, 5700, 1)])), chain3(t, (0, 1, 1), (1, 0), [dense(300, 300, 0, 5700, 1)]))
    # (b) a sparse run given to prev = cluster 0 at gap 1 moves the side of cluster 0 that the first end round starts from, when the chain runs the other way on the
    # target: strand 0 with cur above prev (the second arm; the run raises prev.tEnd), strand 1 with cur below prev (the first arm; the run lowers prev.tStart).
    # moved / stale: the read's end copies the target the round looks at after / before the run; with the run only `moved` is found, without it only `stale`
    for st in (0, 1):
        cur_t, prev_t = ((5900, 6300), (5000, 5500)) if st == 0 else ((5000, 5400), (5800, 6300))
        isl = dense(700, 60, 0, 5800 if st == 0 else 5440, st)                       # next to prev on the read, on the gap's diagonal
        def b(run, end_t, st=st, cur_t=cur_t, prev_t=prev_t, isl=isl):
            return gap2(cur_t, prev_t, st, st, 0, ([isl] if run else []) + [dense(1300, 200, 0, end_t, st)], L=1500, sparse=0.2)
        box = oracle_btwn(b(True, 9000))["box"][0]
        assert len(added(b(True, 9000))[0]) >= 4 and (box[3] > 5800 if st == 0 else box[2] < 5500), "the run did not go to prev"
        moved = int(box[3]) if st == 0 else int(box[2]) - 200
        stale = 5500 if st == 0 else 5800 - 200
        pair("order.run_to_prev.moves_first_end/s%d" % st, b(True, moved), b(False, moved))
        pair("order.run_to_prev.moves_first_end.stale/s%d" % st, b(True, stale), b(False, stale))
        assert len(added(b(True, moved))[0]) > len(added(b(True, stale))[0]) >= 4 and len(added(b(False, stale))[0]) > 4 > len(added(b(False, moved))[0])
    # (b) the last cluster as cur of the last gap, strand 0, cur above prev: what the gap appends lowers cur.tStart, where the last end round ends its target
    def last(run, end_t):
        return gap2((5900, 6300), (5000, 5500), 0, 0, 0, ([dense(400, 400, 0, 5500, 0)] if run else []) + [dense(0, 200, 0, end_t, 0)], cur_q=(200, 400))
    assert int(oracle_btwn(last(True, 9000))["box"][1][2]) == 5500
    pair("order.append_to_last.moves_last_end", last(True, 5300), last(False, 5300))
    pair("order.append_to_last.moves_last_end.stale", last(True, 5700), last(False, 5700))
    assert len(added(last(True, 5300))[1]) > len(added(last(True, 5700))[1]) and len(added(last(False, 5700))[1]) > len(added(last(False, 5300))[1])
    # (b) a chain that descends on the target: the run given to prev cannot move what the first end round reads; both happen on cluster 0
    t = ((5700, 6000), (5000, 5300), (4300, 4600))
    isl = dense(1000 + 300, 60, 0, 5300 + 300, 0)
    single("order.run_to_prev.then_first_end", chain3(t, fill=[isl, dense(1700, 200, 0, 6000, 0)], L=1900, sparse=0.2))
    pair("order.run_to_prev.then_first_end.run", chain3(t, fill=[isl, dense(1700, 200, 0, 6000, 0)], L=1900, sparse=0.2), chain3(t, fill=[dense(1700, 200, 0, 6000, 0)], L=1900, sparse=0.2))
    # (c) one cluster: both end rounds act on it, the second on the box and count the first left
    for st in (0, 1):
        lo, hi = dense(0 if st == 0 else 700, 200, 0, 4800, st), dense(700 if st == 0 else 0, 200, 0, 5500, st)
        one = lambda fill: bcase(compose(900, fill), [cl((200, 700, 5000, 5500), st, 0)], [])
        pair("order.nsp1.both_ends/s%d" % st, one([lo, hi]), one([lo]))
        pair("order.nsp1.both_ends'/s%d" % st, one([lo, hi]), one([hi]))
    # (d) chains of 0, 1, 2, 3 and 6 clusters for one batch; six clusters on one diagonal, every gap dense
    single("layout.nsp=0", bcase(compose(300, []), [], []))
    six = [cl((2500 - 500 * i, 2800 - 500 * i, 7500 - 500 * i, 7800 - 500 * i), 0, 1) for i in range(6)]
    single("layout.nsp=6", bcase(compose(2800, [dense(0, 2800, 1, 5000, 0)]), six, [0] * 5))
    single("layout.nsp=6.s1", bcase(compose(2800, [dense(0, 2800, 1, 5000, 1)]), [cl((2500 - 500 * i, 2800 - 500 * i, 5000 + 500 * i, 5300 + 500 * i), 1, 1) for i in range(6)], [0] * 5))
    # (e) a first round of a few pairs and a later round of several thousand: an island in gap 1, 9000 identical bases in gap 2
    q3 = ((9700, 10000), (9000, 9300), (0, 300))
    t3 = ((14700, 15000), (14000, 14300), (5000, 5300))
    big = bcase(compose(10000, [dense(9300 + 100, 60, 0, 14400, 0), dense(300, 8700, 0, 5300, 0)]), [cl(q3[i] + t3[i], 0, 0) for i in range(3)], [0, 0])
    single("pool.few_then_thousands", big)
    # (f) base match counts and appended segments of 63 | 64 | 65 (the layout copies by waves), and a cluster with several segments
    for n in (63, 64, 65):
        g = first(lambda g: len(found(sgap(0, g, whole=True))) == n, range(10 * n - 20, 10 * n + 40))
        c = sgap(0, g, whole=True)
        c["clusters"][1] = cl(c["clusters"][1]["box"], 0, 0, nm=n)
        single("layout.base=%d.segment=%d" % (n, n), c)
    t = ((5700, 6000), (5000, 5300), (4300, 4600))
    single("layout.three_segments", chain3(t, fill=[dense(1000, 150, 0, 5300, 0), dense(1000 + 300, 60, 0, 5300 + 300, 0), dense(300 + 300, 60, 0, 4600 + 300, 0), dense(300, 60, 0, 4600, 0)],
                                           nm=(2, 64, 2), sparse=0.2))


build(_order)


# ---- MergeChain, DiagonalSort, concatenation (lra_merge_extend_batch) -----------------------------------------------------------------------------------------
# MergeChain reads the boxes alone and nothing here recomputes them, so they are free; the matches are what LinearExtend gets.  ML bases of chromosome c at
# [MT, MT + ML) make the forward read (strand 1 clusters: its reverse complement is taken as the read), so matches on the main (anti)diagonal are true ones.
ML, MT = 3000, 4000


def mread(chrom=0, st=0):
    return compose(ML, [dense(0, ML, chrom, MT, st)])


def on_diag(q0, n, st=0, step=K):
    """n true matches from read position q0 on, `step` apart"""
    return [(q0 + step * i, MT + q0 + step * i) if st == 0 else (q0 + step * i, MT + ML - K - (q0 + step * i)) for i in range(n)]


def off_diag(q0, n, st=0, t0=MT):
    """n matches on n different diagonals: LinearExtend makes one anchor of K bases of each"""
    return [(q0 + 3 * i, t0 + 20 * i) if st == 0 else (q0 + 3 * i, t0 + 17 * i) for i in range(n)]


def mcl(box, st=0, chrom=0, matches=()):
    return cl(box, st, chrom, matches=list(matches))


def two_boxes(qd, td, st=0):
    """(prev box, cur box) at read distance qd (negative: an overlap) and target distance td in the direction the strand's chains run (negative: the wrong side)"""
    cur = (1000, 1300, 5000, 5300)
    pq = 1300 + qd
    prev = (pq, pq + 300, 5300 + td, 5600 + td) if st == 0 else (pq, pq + 300, 4700 - td, 5000 - td)
    return prev, cur


def _merge():
    for st in (0, 1):
        z = "s%d" % st
        rd = mread(0, st)
        def two(qd, td, pst=st, pchrom=0):
            p, c = two_boxes(qd, td, pst)                                              # (the target distance is taken the way prev's strand says)
            return mcase(rd, [mcl(p, pst, pchrom, on_diag(1400, 8, pst)), mcl(c, st, 0, on_diag(1000, 8, st))])
        pair("merge.qdist<=500/" + z, two(500, 100), two(501, 100))
        pair("merge.qdist.overlap_is_0/" + z, two(-100, 100), two(501, 100))
        single("merge.qdist=0|1/%s/0" % z, two(0, 100)); single("merge.qdist=0|1/%s/1" % z, two(1, 100))
        pair("merge.tdist<=500/" + z, two(100, 500), two(100, 501))
        pair("merge.tdist.touching_is_0/" + z, two(100, 0), two(100, -1))            # strand 0 prev.tStart >= cur.tEnd, strand 1 prev.tEnd <= cur.tStart: else 9999
        pair("merge.chrom/" + z, two(100, 100), two(100, 100, pchrom=1))
        pair("merge.strand/" + z, two(100, 100), two(100, 100, pst=1 - st))
        # groupings: chains of 1, 2 and 6 clusters; 6: all merged, none merged, runs in the middle (0 | 1 2 3 | 4 | 5)
        def six(cuts):
            cls = []; q = 2600; t = 16000 if st == 0 else 4000
            for i in range(6):
                if i:
                    far = 2000 if i in cuts else 50
                    t = t - 300 - far if st == 0 else t + 300 + far
                    q -= 350
                cls.append(mcl((q, q + 300, t, t + 300), st, 0, on_diag(q, 5 + i, st)))
            return mcase(rd, cls)
        single("merge.n=1/" + z, mcase(rd, [mcl((1000, 1300, 5000, 5300), st, 0, on_diag(1000, 8, st))]))
        pair("merge.n=6.all|none/" + z, six(()), six((1, 2, 3, 4, 5)))
        pair("merge.n=6.middle_run/" + z, six((1, 4, 5)), six((1, 3, 4, 5)))
        # members without matches: inside a group, as its last member, and a group with no anchors at all (box zeros, strand 0, chromosome 0)
        def three(e):
            cls = [mcl((1700 - 350 * i, 2000 - 350 * i, 5700 - 350 * i, 6000 - 350 * i) if st == 0 else (1700 - 350 * i, 2000 - 350 * i, 5000 + 350 * i, 5300 + 350 * i),
                       st, 2 if e == "all" else 0, [] if (e == "all" or i in e) else on_diag(1700 - 350 * i, 6, st)) for i in range(3)]
            return mcase(mread(2 if e == "all" else 0, st), cls)
        pair("merge.member_empty.middle/" + z, three(()), three((1,)))
        pair("merge.member_empty.last/" + z, three(()), three((2,)))
        pair("merge.group_without_anchors/" + z, three(()), three("all"))
        # concatenation: 63 | 64 | 65 anchors in a group of one member and of three (the box is reduced across lanes that hold nothing)
        for n in (63, 64, 65):
            single("merge.concat.one=%d/%s" % (n, z), mcase(rd, [mcl((100, 400, 5000, 5300), st, 0, off_diag(100, n, st))]))
            parts = (n - 40, 17, 23)
            cls = [mcl((1700 - 350 * i, 2000 - 350 * i, 5700 - 350 * i, 6000 - 350 * i) if st == 0 else (1700 - 350 * i, 2000 - 350 * i, 5000 + 350 * i, 5300 + 350 * i),
                       st, 0, off_diag(100 + 400 * i, parts[i], st, MT + 100 * i)) for i in range(3)]
            single("merge.concat.three=%d/%s" % (n, z), mcase(rd, cls))
    # DiagonalSort keys: q - t negative, zero and positive in one cluster (the positive side needs the very start of chromosome 0), chromosomes 1 and 2 (the
    # chromosome's offset is added and taken off again), cluster sizes around the workgroup sort's limits
    r0 = compose(ML, [dense(0, ML, 0, 0, 0)])
    single("merge.sort.diag_signs", mcase(r0, [mcl((0, 900, 0, 900), 0, 0, [(500, 20), (30, 30), (10, 400), (700, 100), (100, 700), (60, 60), (300, 250), (250, 300), (510, 30), (40, 40)])]))
    for c in (1, 2):
        rc = compose(ML, [dense(0, ML, c, 0, 0)])
        single("merge.sort.chrom%d" % c, mcase(rc, [mcl((0, 900, 0, 900), 0, c, [(500, 20), (30, 30), (10, 400), (700, 100), (100, 700)] + [(1000 + 10 * i, 1000 + 10 * i) for i in range(12)])]))
    rng = np.random.default_rng(5)
    for n in (256, 257, 1024, 1025):
        for st in (0, 1):
            qq = rng.permutation(ML - K)[:n]; tt = rng.integers(5, 2900, n)
            single("merge.sort.n=%d/s%d" % (n, st), mcase(mread(0, st), [mcl((0, ML, 0, 2900), st, 0, zip(qq.tolist(), tt.tolist()))]))
    single("merge.no_matches", mcase(mread(), [mcl((1700, 2000, 5700, 6000)), mcl((1350, 1650, 5350, 5650))]))
    single("merge.nsp=0", mcase(mread(), []))


# ---- TrimOverlappedAnchors, anchors given directly ----------------------------------------------------------------------------------------------------------------
def _trim():
    for kind, minlen in (("trim", 40), ("trimpairs", 50)):
        for st in ((0, 1) if kind == "trim" else (0,)):
            z = "%s/s%d" % (kind, st)
            def mk(anchors, st=st):
                """anchors (q, t, len) in read order on strand 0; strand 1 mirrors the read (q -> 10000 - q - len): LongAnchors then walks them in the same order"""
                if st: anchors = [(10000 - q - l, t, l) for q, t, l in anchors]
                q, t, l = zip(*anchors)
                return tcase(q, t, l, st) if kind == "trim" else pcase(q, t, l)
            pair("trim.len>=%d/%s" % (minlen, z), mk([(100, 5000, minlen), (100 + minlen - 10, 6000, 60)]), mk([(100, 5000, minlen - 1), (100 + minlen - 11, 6000, 60)]))
            pair("trim.cur.len>=%d/%s" % (minlen, z), mk([(100, 5000, 60), (150, 6000, minlen)]), mk([(100, 5000, 60), (150, 6000, minlen - 1)]))
            pair("trim.read_overlap>0/" + z, mk([(100, 5000, 60), (159, 6000, 60)]), mk([(100, 5000, 60), (160, 6000, 60)]))
            pair("trim.read_overlap<=30/" + z, mk([(100, 5000, 60), (130, 6000, 60)]), mk([(100, 5000, 60), (129, 6000, 60)]))
            pair("trim.genome_overlap>0/" + z, mk([(100, 5000, 60), (400, 5059, 60)]), mk([(100, 5000, 60), (400, 5060, 60)]))
            pair("trim.genome_overlap<=30/" + z, mk([(100, 5000, 60), (400, 5030, 60)]), mk([(100, 5000, 60), (400, 5029, 60)]))
            pair("trim.max_of_both/" + z, mk([(100, 5000, 60), (150, 5040, 60)]), mk([(100, 5000, 60), (150, 5050, 60)]))          # read 10, genome 20 | 10
            pair("trim.max_of_both'/" + z, mk([(100, 5000, 60), (140, 5050, 60)]), mk([(100, 5000, 60), (150, 5050, 60)]))         # read 20 | 10, genome 10
            # three in a row: the middle one is trimmed as prev after serving as cur; with the first trim its end no longer reaches the third | it still does
            pair("trim.middle_as_prev/" + z, mk([(100, 5000, 60), (150, 6000, 60), (205, 7000, 60)]), mk([(100, 5000, 60), (150, 6000, 60), (210, 7000, 60)]))
    # forty long anchors with equal sort keys and different lengths: their order is libstdc++'s (past the insertion-sort size of 16), and the walk depends on it
    rng = np.random.default_rng(9)
    ln = (40 + rng.permutation(40)).tolist()
    single("trim.equal_keys/trim/s0", tcase([500] * 40 + [520, 90], [7000] * 40 + [7030, 3000], ln + [70, 45], 0))
    single("trim.equal_keys/trim/s1", tcase([1000 - l for l in ln] + [960, 2000], [7000] * 40 + [7030, 3000], ln + [70, 45], 1))
    ln5 = (50 + rng.permutation(40)).tolist()
    single("trim.equal_keys/trimpairs/s0", pcase([500] * 40 + [520, 90], [7000] * 40 + [7030, 3000], ln5 + [70, 55]))
    single("trim.none_long", tcase([10, 50, 90], [100, 140, 180], [39, 39, 20], 0))
    single("trim.empty", tcase([], [], [], 0))


build(_merge)
build(_trim)


# ---- the packer -----------------------------------------------------------------------------------------------------------------------------------------------
NUM_ALN = 3
JUNK = 0xDEADBEEF


def pack(named, pad=True, marked=True, empty_slots=0, num_aln=NUM_ALN, all_marked=False):
    """Lay chains out as the arrays lra_refine_btwn_splitchain_batch / lra_merge_extend_batch read (numpy, host side).  named: [(name, case)], kind btwn or merge, in
    slot order.  Consecutive cases with the same read share one read (up to NUM_ALN chains on it, n_chains often below NUM_ALN).  pad: one or two unused fragments
    between chains, with matches of their own and junk boxes / strands / chromosomes.  marked: every fourth read starts with a slot whose split status is non-zero and
    whose chain_start is junk.  Unused slots (at or past n_chains) hold junk too.  n_split of unused and marked slots is 1: the host takes the number of gap rounds
    from the maximum over ALL slots.  empty_slots: that many reads without a chain in front.  all_marked: every chain's slot gets a non-zero status.  -> dict of arrays, and `where`: name -> (slot, first fragment)"""
    reads = []                                        # [read bytes, [(name, case) or None (a marked slot)]]
    for name, case in named:
        if reads and reads[-1][0] == case["read"] and len(reads[-1][1]) < num_aln: reads[-1][1].append((name, case))
        else:
            reads.append([case["read"], []])
            if marked and num_aln > 1 and len(reads) % 4 == 2: reads[-1][1].append(None)
            reads[-1][1].append((name, case))
    reads = [[b"ACGTACGTAC", []] for _ in range(empty_slots)] + reads
    n_reads = len(reads)
    n_slots = n_reads * num_aln
    n_chains = np.zeros(n_reads, np.uint32)
    chain_start = np.full(n_slots, 0xFFFFFFFFFFF0, np.uint64)
    n_split = np.ones(n_slots, np.uint32)
    status = np.zeros(n_slots, np.uint32)
    strand = []; chrom = []; link = []; box = []; moff = [0]; mq = []; mt = []
    where = {}

    def junk_frag(k):
        strand.append(7); chrom.append(99); link.append(1); box.extend([JUNK, 3, JUNK, 5])
        for i in range(1 + k % 3): mq.append(17 + i); mt.append(JUNK)
        moff.append(len(mq))

    k = 0
    for r, (_, chains) in enumerate(reads):
        n_chains[r] = len(chains)
        for c, item in enumerate(chains):
            s = r * num_aln + c
            if item is None:
                status[s] = 3
                continue
            name, case = item
            if pad:
                for _ in range(1 + k % 2): junk_frag(k)
            k += 1
            cls = case["clusters"]
            chain_start[s] = len(strand); n_split[s] = len(cls); status[s] = 5 if all_marked else 0
            where[name] = (s, len(strand))
            for i, cc in enumerate(cls):
                strand.append(cc["strand"]); chrom.append(cc["chrom"]); link.append(case["link"][i] if i < len(cls) - 1 else 1); box.extend(cc["box"])
                mq.extend(m[0] for m in cc["matches"]); mt.extend(m[1] for m in cc["matches"]); moff.append(len(mq))
    if pad: junk_frag(k)
    if not strand: junk_frag(0)
    fwd = [np.frombuffer(rd, np.uint8) for rd, _ in reads]
    read_off = np.cumsum([0] + [len(f) for f in fwd]).astype(np.uint64)
    tot = int(read_off[-1])
    strands = np.concatenate(fwd + [revcomp(f) for f in fwd] + [np.zeros(64, np.uint8)])
    return dict(n_reads=n_reads, num_aln=num_aln, n_slots=n_slots, n_frags=len(strand), n_matches=len(mq), n_chains=n_chains, chain_start=chain_start, n_split=n_split,
                status=status, sp_strand=np.array(strand, np.uint8), sp_chrom=np.array(chrom, np.int32), split_link=np.array(link, np.uint8),
                box=np.array(box, np.uint32), match_off=np.array(moff, np.uint64), match_q=np.array(mq + [0], np.uint32), match_t=np.array(mt + [0], np.uint32),
                read_off=read_off, strands=strands, rc_base=tot, genome=np.concatenate([GENOME, np.zeros(64, np.uint8)]), where=where)


def to_device(ctx, P):
    """the packed arrays on the GPU and the three structures pointing at them (only the fields the two entry points read are set) -> (keep-alive, chains, split, refined)"""
    import torch
    from lra_amd import chain
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    dev = {k: torch.from_numpy(v.view(view.get(v.dtype, v.dtype))).to(ctx.device) for k, v in P.items() if isinstance(v, np.ndarray)}
    ch = chain.ChainResult(); ch.n_reads = P["n_reads"]; ch.num_aln = P["num_aln"]; ch.d_n_chains = dev["n_chains"].data_ptr(); ch.d_chain_start = dev["chain_start"].data_ptr()
    sp = chain.SplitResult(); sp.n_slots = P["n_slots"]; sp.n_frags = P["n_frags"]
    sp.d_n_split = dev["n_split"].data_ptr(); sp.d_status = dev["status"].data_ptr(); sp.d_sp_strand = dev["sp_strand"].data_ptr(); sp.d_sp_chrom = dev["sp_chrom"].data_ptr()
    sp.d_split_link = dev["split_link"].data_ptr()
    rf = chain.RefinedResult(); rf.n_frags = P["n_frags"]; rf.n_matches = P["n_matches"]
    rf.d_match_off = dev["match_off"].data_ptr(); rf.d_match_q = dev["match_q"].data_ptr(); rf.d_match_t = dev["match_t"].data_ptr(); rf.d_box = dev["box"].data_ptr()
    return dev, ch, sp, rf
