"""Crafted chains for the per-chain walks of chain_split.hip (the six filters of Chain.h, the low-accuracy SPLITChain walk and the high-accuracy one): a builder
that places every anchor so that the diagonal gap to its predecessor is exactly what the description asks for, and a registry of *threshold pairs* -- two cases that
differ in one quantity sitting on either side of one comparison, under a name that says which.  Shared by tests/test_chain_filter_edges.py,
tests/test_chain_split_edges.py and tools/oracle_mutants.py.  Plain helpers, CPU only, no fixtures."""
import numpy as np

import oracle_lib as O

M32 = 1 << 32
CHROM = [0, 3_000_000, 6_000_000, 4_200_000_000]


# ---- the builder --------------------------------------------------------------------------------------------------------------------------------------------
def make_chain(lens, strand=0, asc=False, gaps=None, flips=(), q0=None, t0=1_000_000, sp=None, qend=None, link=None, cluster=None):
    """One chain in the order the walks see it.  lens: per-anchor lengths.  strand: of anchor 0; it toggles at every index in `flips`.  asc: q ascending
    along the chain (FinalChain order) instead of descending (trace-back order).  gaps: {c: diagonal gap between anchors c-1 and c}, 0 elsewhere -- on strand 0
    t - q changes by it, on strand 1 qEnd + t does (across a flip the walks take no gap; the anchor is placed as if its predecessor had the new strand).
    sp: read distance between neighbours, a number, {c: distance} over the default, or None for the default 10 / 30 alternation (a constant distance has
    deviation 0, and refineEnds then calls every distance invalid).  qend: {c: surplus of qEnd over q + len}; the gap is exact for that qEnd.
    Positions are kept as Python integers and reduced modulo 2^32 at the end."""
    n = len(lens)
    gaps = gaps or {}
    qend = qend or {}
    spd = sp if isinstance(sp, dict) else {}
    sp0 = None if sp is None or isinstance(sp, dict) else int(sp)
    dist = lambda c: spd[c] if c in spd else (sp0 if sp0 is not None else (10 if c % 2 else 30))
    st = []
    s = strand
    for c in range(n):
        if c in flips: s ^= 1
        st.append(s)
    if q0 is None:
        q0 = 50 if asc else 50 + sum(lens) + sum(max(dist(c), 0) for c in range(1, n))
    q = [q0][:n]; t = [t0][:n]
    qe = lambda c: q[c] + lens[c] + qend.get(c, 0)
    for c in range(1, n):
        q.append(q[c - 1] + lens[c - 1] + dist(c) if asc else q[c - 1] - lens[c] - dist(c))
        g = gaps.get(c, 0)
        if st[c] == 0: t.append(t[c - 1] - q[c - 1] + q[c] + g)
        else: t.append(qe(c - 1) + t[c - 1] + g - qe(c))
    u32 = lambda v: np.array([x % M32 for x in v], np.uint32)
    lk = [(c * 5 % 3 == 0) for c in range(n - 1)] if link is None else list(link)
    cl = [0] * n if cluster is None else list(cluster)
    return dict(q=u32(q), t=u32(t), len=np.array(lens, np.int32), strand=np.array(st, np.uint8), link=np.array(lk, np.uint8),
                qend=u32([qe(c) for c in range(n)]), cluster=np.array(cl, np.int32))


def shifted(ch, dt):
    """the same chain moved by dt on the target (every diagonal gap and every distance unchanged)"""
    out = dict(ch)
    out["t"] = ((ch["t"].astype(np.int64) + dt) % M32).astype(np.uint32)
    return out


def cross_t(ch, c, boundary):
    """the chain moved on the target so that `boundary` lies between the starts of anchors c - 1 and c"""
    a, b = int(ch["t"][c - 1]), int(ch["t"][c])
    assert a != b
    return shifted(ch, boundary - (a + b) // 2 - 1 + (1 if abs(a - b) == 1 else 0))


def cross_sum(ch, c):
    """a reverse chain moved so that qEnd + t passes 2^32 between anchors c - 1 and c: the 32-bit sum wraps there"""
    a, b = int(ch["qend"][c - 1]) + int(ch["t"][c - 1]), int(ch["qend"][c]) + int(ch["t"][c])
    out = shifted(ch, M32 - 1 - min(a, b))
    sa, sb = int(out["qend"][c - 1]) + int(out["t"][c - 1]), int(out["qend"][c]) + int(out["t"][c])
    assert (sa >= M32) != (sb >= M32) and int(out["t"].max()) < M32
    return out


# ---- cases and the registry ---------------------------------------------------------------------------------------------------------------------------------
def fcase(chain, ops, link=True, qend=False):
    return dict(kind="filter", chain=chain, ops=tuple(ops), link=bool(link), qend=bool(qend))


def scase(chain, splitdist=50000, bypass=1, chrom=CHROM):
    return dict(kind="split", chain=chain, splitdist=int(splitdist), bypass=int(bypass), chrom=tuple(chrom))


def hcase(strand, chrom, box, link, splitdist=100000):
    return dict(kind="hsplit", strand=list(strand), chrom=list(chrom), box=[list(b) for b in box], link=list(link), splitdist=int(splitdist))


PAIRS = {}          # name -> (case, case): the oracle's outputs must differ
SINGLES = {}        # name -> case: layout, coordinates, op orders


def pair(name, a, b):
    assert name not in PAIRS, name
    PAIRS[name] = (a, b)


def single(name, c):
    assert name not in SINGLES, name
    SINGLES[name] = c


def run(case):
    """The oracle's whole output for one case, as a hashable value (None where the reference would read outside its arrays)."""
    k = case["kind"]
    if k == "filter":
        ch = case["chain"]
        keep, lk = O.filter_chain(ch["q"], ch["t"], ch["len"], ch["strand"], ch["link"] if case["link"] else None, list(case["ops"]),
                                  qend=ch["qend"] if case["qend"] else None)
        return (keep.tobytes(), lk.tobytes())
    if k == "split":
        ch = case["chain"]
        r = O.split_chain(ch["q"], ch["t"], ch["len"], ch["strand"], ch["cluster"], ch["link"], list(case["chrom"]), case["splitdist"], case["bypass"])
        if r is None: return None
        return (r["keep"].tobytes(), r["link"].tobytes(), r["split_link"].tobytes(),
                tuple((s["idx"].tobytes(), s["link"].tobytes(), s["type"], s["strand"], s["chrom"], s["box"].tobytes(), s["clusters"].tobytes()) for s in r["splits"]))
    r = O.split_chain_highacc(case["strand"], case["chrom"], np.array(case["box"], np.uint32).reshape(-1, 4), case["link"], case["splitdist"])
    return (r["off"].tobytes(), r["idx"].tobytes(), r["type"].tobytes(), r["strand"].tobytes(), r["box"].tobytes(), r["lsc"])


def decision(case):
    """run() without the boxes: what the walk decided, not the coordinates it echoes.  The two sides of a pair must differ in THIS."""
    r = run(case)
    if r is None or case["kind"] == "filter": return r
    if case["kind"] == "split": return r[:3] + (tuple(p[:5] + p[6:] for p in r[3]),)
    return r[:4] + r[5:]


def all_cases():
    """[(name, case)]: both sides of every pair, then the singles"""
    out = []
    for n, (a, b) in PAIRS.items(): out += [(n + "/a", a), (n + "/b", b)]
    out += list(SINGLES.items())
    return out


# ---- filters: one SV pair in a short chain ------------------------------------------------------------------------------------------------------------------
VARIANTS = [(0, False), (1, False), (0, True), (1, True)]      # (strand, q ascending)
vname = lambda s, a: "s%d%s" % (s, "a" if a else "d")


def sv_chain(g1, g2, d=1, L=20, n=9, at=3, lens=None, **kw):
    """n anchors of length L, diagonal gaps g1 at anchor `at` and g2 at anchor at + d"""
    ln = [L] * n
    for i, v in (lens or {}).items(): ln[i] = v
    return make_chain(ln, gaps={at: g1, at + d: g2}, **kw)


def _sv_pairs(tag, ops_list, a_kw, b_kw, variants=VARIANTS, links=(True, False), signs=(1, -1)):
    """register a pair for every op set, strand, q order, link presence and sign of the first jump"""
    for ops in ops_list:
        for s, asc in variants:
            for lk in links:
                for sg in signs:
                    A = dict(a_kw); B = dict(b_kw)
                    for K in (A, B): K["g1"] *= sg; K["g2"] *= sg
                    pair("%s/op%s/%s%s%s" % (tag, "".join(map(str, ops)), vname(s, asc), "L" if lk else "", "+" if sg > 0 else "-"),
                         fcase(sv_chain(strand=s, asc=asc, **A), ops, lk), fcase(sv_chain(strand=s, asc=asc, **B), ops, lk))


def _filters():
    # op 1  RemoveSmallPairedIndels: 5 < |gap| <= 50, |sum| <= 20, distance < 3, len <= 50
    _sv_pairs("op1.gap>5", [(1,)], dict(g1=6, g2=-6), dict(g1=5, g2=-6))
    _sv_pairs("op1.gap<=50", [(1,)], dict(g1=50, g2=-45), dict(g1=51, g2=-45))
    _sv_pairs("op1.sum<=20", [(1,)], dict(g1=40, g2=-20), dict(g1=41, g2=-20))
    _sv_pairs("op1.dist<3", [(1,)], dict(g1=30, g2=-30, d=2), dict(g1=30, g2=-30, d=3))
    _sv_pairs("op1.len<=50", [(1,)], dict(g1=30, g2=-30, lens={3: 50}), dict(g1=30, g2=-30, lens={3: 51}))
    # op 8  RemoveSpuriousJump: |gap| > 100, distance == 1, len < 50
    _sv_pairs("op8.gap>100", [(8,)], dict(g1=101, g2=-150), dict(g1=100, g2=-150))
    _sv_pairs("op8.dist==1", [(8,)], dict(g1=200, g2=-200, d=1), dict(g1=200, g2=-200, d=2))
    _sv_pairs("op8.len<50", [(8,)], dict(g1=200, g2=-200, lens={3: 49}), dict(g1=200, g2=-200, lens={3: 50}))
    for s, asc in VARIANTS:                                               # three alternating jumps: the second pair tests rm[] of the first pair's position
        three = lambda g3, s=s, asc=asc: fcase(make_chain([20] * 9, s, asc, gaps={3: 200, 4: -200, 5: g3}), (8,))
        pair("op8.three/" + vname(s, asc), three(200), three(100))
    # ops 2 and 3  RemovePairedIndels: |gap| > 30, both >= 300 or |sum| < 100, distance < 3, len < 100
    o23 = [(2,), (3,)]
    _sv_pairs("op23.gap>30", o23, dict(g1=31, g2=-40, sp={3: 60, 4: 80}), dict(g1=30, g2=-40, sp={3: 60, 4: 80}))
    _sv_pairs("op23.both>=300", o23, dict(g1=300, g2=-400), dict(g1=299, g2=-400))
    _sv_pairs("op23.both>=300'", o23, dict(g1=400, g2=-300), dict(g1=400, g2=-299))
    _sv_pairs("op23.sum<100", o23, dict(g1=200, g2=-101), dict(g1=200, g2=-100))
    _sv_pairs("op23.dist<3", o23, dict(g1=200, g2=-200, d=2), dict(g1=200, g2=-200, d=3))
    _sv_pairs("op23.len<100", o23, dict(g1=200, g2=-200, lens={3: 99}), dict(g1=200, g2=-200, lens={3: 100}))
    _sv_pairs("op23.len<100.300rule", o23, dict(g1=300, g2=-400, lens={3: 99}), dict(g1=300, g2=-400, lens={3: 100}))      # |sum| = 100: the 300 rule alone
    for ops in o23:
        for s, asc in VARIANTS:                                           # a strand flip between the two jumps is an SV of 0: neither pair fires
            f = lambda flips, s=s, asc=asc, ops=ops: fcase(make_chain([20] * 9, s, asc, gaps={3: 200, 5: -200}, flips=flips), ops)
            pair("op23.flip/op%d/%s" % (ops[0], vname(s, asc)), f(()), f((4,)))
    # op 4  RemoveSpuriousAnchors: |gap| >= 500, distance <= 10, no anchor of len >= 50 in the run; link untouched
    _sv_pairs("op4.gap>=500", [(4,)], dict(g1=500, g2=600, d=3), dict(g1=499, g2=600, d=3))
    _sv_pairs("op4.gap>=500'", [(4,)], dict(g1=600, g2=-500, d=3), dict(g1=600, g2=-499, d=3))
    _sv_pairs("op4.dist<=10", [(4,)], dict(g1=600, g2=600, d=10, n=16), dict(g1=600, g2=600, d=11, n=16))
    _sv_pairs("op4.len>=50", [(4,)], dict(g1=600, g2=600, d=3, L=49, lens={4: 49}), dict(g1=600, g2=600, d=3, L=49, lens={4: 50}))
    for s, asc in VARIANTS:                                               # a strand flip inside the run is an SV of 0: neither neighbour pair fires
        f = lambda flips, s=s, asc=asc: fcase(make_chain([20] * 10, s, asc, gaps={3: 600, 6: 600}, flips=flips), (4,))
        pair("op4.flip/" + vname(s, asc), f(()), f((5,)))
    # op 5  RemovePairedIndels(GenomePairs&): |gap| > 30 on t - q whatever the strand; the distance between the two SVs' t starts against max(2 blink, 1000) / 500
    def o5(g1, g2, dd, L=20, lk=False):
        """two adjacent SVs; dd = |t(c) - t(c-1)| for an insertion second (g2 > 0), |t(c) - g2 - t(c-1)| for a deletion second"""
        sp4 = (dd - L) if g2 < 0 else (g2 + dd - L)                      # descending: t(c) - t(c-1) = g2 - L - sp
        return fcase(make_chain([L] * 9, 0, False, gaps={3: g1, 4: g2}, sp={4: sp4}), (5,), lk)
    for sg, lk in ((1, False), (-1, False), (1, True), (-1, True)):      # op 5 leaves link alone: with it, the vector comes out whole
        z = ("+" if sg > 0 else "-") + ("L" if lk else "")
        pair("op5.gap>30/" + z, o5(sg * 31, -sg * 40, 100, lk=lk), o5(sg * 30, -sg * 40, 100, lk=lk))
        pair("op5.sum<600/" + z, o5(sg * 1000, -sg * 401, 700, lk=lk), o5(sg * 1000, -sg * 400, 700, lk=lk))
        pair("op5.lim1000/" + z, o5(sg * 200, -sg * 200, 999, lk=lk), o5(sg * 200, -sg * 200, 1000, lk=lk))
        pair("op5.lim2blink/" + z, o5(sg * 600, -sg * 600, 1199, lk=lk), o5(sg * 600, -sg * 600, 1200, lk=lk))
        pair("op5.lim500/" + z, o5(sg * 1000, -sg * 400, 499, lk=lk), o5(sg * 1000, -sg * 400, 500, lk=lk))
        pair("op5.same.lim1000/" + z, o5(sg * 200, sg * 200, 999, lk=lk), o5(sg * 200, sg * 200, 1000, lk=lk))
        pair("op5.same.lim2blink/" + z, o5(sg * 700, sg * 600, 1399, lk=lk), o5(sg * 700, sg * 600, 1400, lk=lk))
        pair("op5.len<100/" + z, o5(sg * 200, -sg * 200, 100, L=99, lk=lk), o5(sg * 200, -sg * 200, 100, L=100, lk=lk))
        pair("op5.len<100.lim500/" + z, o5(sg * 1000, -sg * 400, 100, L=99, lk=lk), o5(sg * 1000, -sg * 400, 100, L=100, lk=lk))
        pair("op5.len<100.same/" + z, o5(sg * 200, sg * 200, 100, L=99, lk=lk), o5(sg * 200, sg * 200, 100, L=100, lk=lk))
    mixed = lambda c: dict(c, chain=dict(c["chain"], strand=np.array([0, 1, 1, 0, 1, 0, 0, 1, 1], np.uint8)))
    pair("op5.strands_ignored", mixed(o5(200, -200, 999)), mixed(o5(200, -200, 1000)))
    single("op5.strands_ignored.plain", o5(200, -200, 999))


AT_LIMIT = [136] + [0] * 16
BELOW_LIMIT = [136] + [0] * 7 + [17] + [0] * 8


def _refine_ends():
    """op 2's refineEnds: a distance is valid below mean + 4 sd; ends of one or two anchors before the first / behind the last valid distance go"""
    N = 120
    far = 50000
    for s, asc in ((0, False), (1, False)):
        for k in range(3):
            pair("op2.firstValid=%d|%d/%s" % (k, k + 1, vname(s, asc)), fcase(make_chain([20] * N, s, asc, sp={c: far for c in range(1, k + 1)}), (2,)),
                 fcase(make_chain([20] * N, s, asc, sp={c: far for c in range(1, k + 2)}), (2,)))
        for k in range(2):
            pair("op2.N-lastValid=%d|%d/%s" % (k + 1, k + 2, vname(s, asc)), fcase(make_chain([20] * N, s, asc, sp={N - 1 - c: far for c in range(k)}), (2,)),
                 fcase(make_chain([20] * N, s, asc, sp={N - 1 - c: far for c in range(k + 1)}), (2,)))
        for end, c, spc in (("front", 0, 1), ("back", N - 1, N - 1)):        # the end anchor itself of length 99 | 100
            e = lambda L, s=s, asc=asc, c=c, spc=spc: fcase(make_chain([20] * c + [L] + [20] * (N - 1 - c), s, asc, sp={spc: far}), (2,))
            pair("op2.%s_end.len<100/%s" % (end, vname(s, asc)), e(99), e(100))
    # exactly at the limit and one below it, in integers so that the float arithmetic is exact (exact_limit): 17 distances, 136 and sixteen zeros have
    # mean 8, variance 1024, sd 32, limit 136 -- the first distance is AT the limit, invalid; 136, 17 and fifteen zeros have mean 9, variance 1024, limit 137
    for s in (0, 1):
        pair("op2.at_limit/s%d" % s, fcase(make_chain([20] * 18, s, False, sp={c: v for c, v in enumerate(AT_LIMIT, 1)}), (2,)),
             fcase(make_chain([20] * 18, s, False, sp={c: v for c, v in enumerate(BELOW_LIMIT, 1)}), (2,)))
        pair("op2.none_valid/s%d" % s, fcase(make_chain([20] * 12, s, False, sp=10), (2,)), fcase(make_chain([20] * 12, s, False, sp={c: 10 if c != 6 else 9 for c in range(1, 12)}), (2,)))
    # q ascending: the read distance is qS(c) - tE(c-1) as written.  t = q - D puts it at sp + D; one target jump of 60000 then leaves min(tDist, qDist) = sp + D
    # at anchor 1, an invalid first distance; with D = 0 it is sp like everywhere else
    qa = lambda D: fcase(make_chain([20] * 60, 0, True, gaps={1: 60000}, q0=100000, t0=100000 - D), (2,))
    pair("op2.qasc_minus_tE", qa(50000), qa(0))
    # dist * dist summed in 64 bits: one distance of 3.0e9 (square below 2^63: the 3.0e9 alone is invalid), one of 3.1e9 (above 2^63: a negative sum, a NaN
    # deviation, nothing valid, everything short goes), two of 3.1e9 (the sum passes 2^64 and comes back positive: a small deviation, both invalid, nothing goes).
    # The second is a step UP the read and the target (a negative sp): its read distance is then qS(c) - tE(c-1) = 3.1e9 + 100 with t = q - 100.
    big = lambda sp: fcase(make_chain([20] * 60, 0, False, sp=sp, q0=3_200_000_000, t0=3_200_000_000 - 100), (2,))
    pair("op2.sq.below_2^63|above", big({30: 3_000_000_000}), big({30: 3_100_000_000}))
    pair("op2.sq.above_2^63|wrapped_2^64", big({30: 3_100_000_000}), big({30: 3_100_000_000, 40: -(3_100_000_000 + 40)}))
    single("op2.sq.small_overlap", big({30: -5}))


def exact_limit(sps):
    """(mean, variance, sd, limit) of a distance list when all are integers below 2^24 (so the float arithmetic of the walk is exact), else None"""
    m = len(sps); tot = sum(sps); sq = sum(v * v for v in sps)
    if tot % m or sq % m or sq >= 1 << 24: return None
    mean = tot // m; var = sq // m - mean * mean
    sd = int(round(var ** 0.5))
    if sd * sd != var: return None
    return mean, var, sd, mean + 4 * sd


def _qend_links_orders():
    # qend: a reverse chain built with qEnd = q + len + 40 at anchor 3 and no gap anywhere.  With its qend the filters see no SV; on q + len they see -40 / +40
    for ops in ((1, 3, 4), (1,)):
        ch = make_chain([20] * 9, 1, False, qend={3: 40})
        pair("qend.changes_class/op%s" % "".join(map(str, ops)), fcase(ch, ops, True, True), fcase(ch, ops, True, False))
    ch = make_chain([20] * 9, 1, False, qend={3: 40}, gaps={3: 25, 4: -25})   # exact for that qEnd: 25 / -25; on q + len -15 / +15
    pair("qend.sum", fcase(ch, (1,), True, True), fcase(make_chain([20] * 9, 1, False, qend={3: 40}, gaps={3: 25, 4: -46}), (1,), True, True))
    # links: op 4 and 5 leave the vector alone, 2 and 3 keep the old size when nothing survives, and the next op compacts on that state
    run4 = make_chain([20] * 16, 0, False, gaps={3: 600, 6: 600, 9: 30, 10: -30, 12: 200, 13: -200})
    for ops in ((4,), (4, 1), (4, 8), (4, 8, 1), (4, 3), (5, 4), (5, 1)):
        single("link.after_op%s" % "".join(map(str, ops)), fcase(run4, ops, True))
    wipe = lambda lens: make_chain(lens, 0, False, sp=10)
    pair("link.op2.nothing_survives", fcase(wipe([20] * 8), (2,), True), fcase(wipe([20] * 7 + [100]), (2,), True))
    pair("link.op2.nothing_survives.then8", fcase(wipe([20] * 8), (2, 8), True), fcase(wipe([100] + [20] * 6 + [100]), (2, 8), True))
    some = make_chain([100, 20, 100, 20, 20, 100, 20, 100, 100], 0, False, sp=10, gaps={3: 30, 5: -30})
    for ops in ((2,), (2, 1), (2, 4, 1)):
        single("link.op2.some_survive/op%s" % "".join(map(str, ops)), fcase(some, ops, True))
    # the op orders of the two mappers, {8} alone, and one order of six
    for s, asc in VARIANTS:
        lens = [20, 20, 30, 45, 60, 20, 99, 100, 20, 20, 150, 20, 20, 20, 49, 50, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20, 20]
        ch = make_chain(lens, s, asc, gaps={2: 10, 3: -12, 6: 400, 7: -380, 10: 600, 14: -700, 17: 150, 18: -150, 21: 35, 23: -45, 26: 320, 27: -900}, flips=(24,))
        for ops in ((2, 4), (1, 2, 4), (1, 3, 4), (5, 4), (8,), (8, 1, 3, 5, 4, 2)):
            for lk in (True, False):
                single("orders/op%s/%s%s" % ("".join(map(str, ops)), vname(s, asc), "L" if lk else ""), fcase(ch, ops, lk))


def _coordinates():
    """whole chains at 3.0e9, chains crossing 2^31 between the two SV anchors, reverse chains whose qEnd + t wraps 2^32 there; every gap and distance is that of the
    low-coordinate chain, so the expectation is the same"""
    basics = [((1,), dict(g1=28, g2=-27)), ((8,), dict(g1=200, g2=-200)), ((2,), dict(g1=400, g2=-400)), ((3,), dict(g1=200, g2=-150)),
              ((4,), dict(g1=600, g2=-600, d=3)), ((2, 4), dict(g1=400, g2=-400)), ((1, 3, 4), dict(g1=28, g2=-27))]
    for ops, kw in basics:
        for s, asc in VARIANTS:
            base = sv_chain(strand=s, asc=asc, q0=5000, **kw)
            tag = "op%s/%s" % ("".join(map(str, ops)), vname(s, asc))
            COORD_SAME.append(("coord.3e9/" + tag, "coord.low/" + tag))
            single("coord.low/" + tag, fcase(base, ops))
            single("coord.3e9/" + tag, fcase(shifted(base, 3_000_000_000 - 1_000_000), ops))
            for c in (3, 4):
                single("coord.x2^31@%d/%s" % (c, tag), fcase(cross_t(base, c, 1 << 31), ops))
                COORD_SAME.append(("coord.x2^31@%d/%s" % (c, tag), "coord.low/" + tag))
                if s == 1 and int(base["qend"][c - 1]) + int(base["t"][c - 1]) != int(base["qend"][c]) + int(base["t"][c]):
                    single("coord.sum_x2^32@%d/%s" % (c, tag), fcase(cross_sum(base, c), ops))
                    COORD_SAME.append(("coord.sum_x2^32@%d/%s" % (c, tag), "coord.low/" + tag))
    # op 5 reads (int)t: the crossing stays at anchors 0 / 1, away from the SV pair at 5 / 6
    for sg in (1, -1):
        base = make_chain([20] * 9, 0, False, gaps={5: sg * 200, 6: -sg * 200})
        single("coord.low/op5/%d" % sg, fcase(base, (5,), False))
        for nm, ch in (("coord.3e9", shifted(base, 3_000_000_000 - 1_000_000)), ("coord.x2^31@1", cross_t(base, 1, 1 << 31))):
            single("%s/op5/%d" % (nm, sg), fcase(ch, (5,), False))
            COORD_SAME.append(("%s/op5/%d" % (nm, sg), "coord.low/op5/%d" % sg))


COORD_SAME = []     # (name, name): singles whose oracle output must be equal (a translation on the target)


LAYOUT_N = (63, 64, 65, 127, 128, 129, 1000, 5000)
LAYOUT_OPS = ((2, 4), (8,), (4,), (1, 3, 4))


def layout_case(n, s, ops):
    """the chain of n anchors with the SV pair on anchors 63 / 64 and the op 4 run over 60..69"""
    nm = "layout.n=%d/s%d/op%s" % (n, s, "".join(map(str, ops)))
    return PAIRS[nm][0] if nm in PAIRS else SINGLES[nm]


def _layout():
    """chain lengths around the wave and far beyond it, an SV pair on anchors 63 / 64, an op 4 run over 60..69; ends that go"""
    for n in (0, 1, 2, 3):
        for ops in ((2, 4), (8,), (1, 3, 4)):
            single("layout.n=%d/op%s" % (n, "".join(map(str, ops))), fcase(make_chain([20] * n, n % 2, False, gaps={1: 200, 2: -200}), ops))
    for n in LAYOUT_N:
        for s in (0, 1):
            # every seventh anchor is long, but none in 56..72: the +400 / -400 pair on anchors 63 / 64 takes anchor 63 (ops 2, 3, 8), the 600 / 600 run takes 60..68 (op 4)
            lens = [120 if c % 7 == 3 and not 56 <= c <= 72 else 20 for c in range(n)]
            ends = {n - 2: 200, n - 1: -200, 1: -150, 2: 150}
            build = lambda gg: make_chain(lens, s, False, gaps={c: v for c, v in gg.items() if 0 < c < n}, sp={1: 50000, n - 1: 50000} if n >= 127 else None)
            ch = build({**ends, 63: 400, 64: -400, 60: 600, 69: 600})
            for ops in LAYOUT_OPS:
                nm = "layout.n=%d/s%d/op%s" % (n, s, "".join(map(str, ops)))
                if 127 <= n <= 129: pair(nm, fcase(ch, ops), fcase(build(ends), ops))     # against the same chain without the gaps at the wave's edge
                else: single(nm, fcase(ch, ops))
    # neighbours in the batch: the first loses its last anchor, the second its first (refineEnds)
    N = 60
    single("layout.ends.last_goes", fcase(make_chain([20] * N, 0, False, sp={N - 1: 50000}), (2,)))
    single("layout.ends.first_goes", fcase(make_chain([20] * N, 0, False, sp={1: 50000}), (2,)))


# ---- the low-accuracy split walk ----------------------------------------------------------------------------------------------------------------------------
def split_dists(ch, cur):
    """(qdist, tdist, |diag difference|) of SPLITChain's step prev = cur - 1 -> cur"""
    p = cur - 1
    q = ch["q"].astype(np.int64); t = ch["t"].astype(np.int64); ln = ch["len"].astype(np.int64); s = ch["strand"]
    qd = int(q[p] - q[cur] - ln[cur])
    td = int(t[p] - t[cur] - ln[cur]) if t[p] > t[cur] + ln[cur] else int(t[cur] + ln[cur] - t[p])
    dg = lambda i: int(q[i] + ln[i] + t[i]) if s[i] else int(t[i] - q[i])
    return qd, td, abs(dg(cur) - dg(p))


def _split():
    cl = lambda n, cuts: [sum(c >= x for x in cuts) for c in range(n)]
    # the jump filter in front (keep[])
    for s in (0, 1):
        z = "s%d" % s
        j = lambda **kw: scase(sv_chain(strand=s, **kw))
        pair("split.jump.gap>100/" + z, j(g1=101, g2=-150), j(g1=100, g2=-150))
        pair("split.jump.dist==1/" + z, j(g1=200, g2=-200), j(g1=200, g2=-200, d=2))
        pair("split.jump.len<50/" + z, j(g1=200, g2=-200, lens={3: 49}), j(g1=200, g2=-200, lens={3: 50}))
        # the N cut: dist = min(qdist, tdist) >= 1000 and |diag difference| <= ceil(0.15 dist)
        def ncut(sp, g, want=None, s=s):
            ch = make_chain([20] * 8, s, False, gaps={4: g}, sp={4: sp}, cluster=cl(8, [4]))
            qd, td, dd = split_dists(ch, 4)
            if want is not None: assert (min(qd, td), qd < td, dd) == want, (qd, td, dd, want)
            return scase(ch)
        gq, gt = (-10, 10) if s == 0 else (10, -60)                      # a gap that leaves qdist / tdist the smaller
        pair("split.N.dist>=1000.q/" + z, ncut(1000, gq, (1000, True, abs(gq))), ncut(999, gq, (999, True, abs(gq))))
        o = 10 if s == 0 else 20
        pair("split.N.dist>=1000.t/" + z, ncut(1000 + o, gt, (1000, False, abs(gt))), ncut(999 + o, gt, (999, False, abs(gt))))
        gn = -151 if s == 0 else 151
        pair("split.N.ceil/" + z, ncut(1001, gn, (1001, True, 151)), ncut(1001, gn + (-1 if s == 0 else 1), (1001, True, 152)))
        if s == 1:                                                        # unequal lengths: diag is qEnd + t, not q + t
            def nlen(g):
                ch = make_chain([20, 20, 20, 20, 40, 20, 20, 20], 1, False, gaps={4: g}, sp={4: 1001}, cluster=cl(8, [4]))
                assert split_dists(ch, 4)[::2] == (1001, abs(g))
                return scase(ch)
            pair("split.N.ceil.len/" + z, nlen(151), nlen(152))
        pair("split.N.ceil.t/" + z, ncut(1001, gn, (1001, True, 151)), ncut(1001, -gn, None))
        # the T cut: tS(cur) > tE(prev) + splitdist, tE(cur) + splitdist < tS(prev)
        def tcut(delta, up, s=s):
            """target distance between the two anchors = splitdist + delta, cur above (up) or below prev"""
            sd = 50000
            if up: g = (sd + delta - 10) if s == 1 else (sd + delta + 20 + 10 + 20)
            else: g = -(sd + delta - 10) if s == 0 else -(sd + delta + 20 + 10 + 20)
            ch = make_chain([20] * 8, s, False, gaps={4: g}, sp={4: 10}, cluster=cl(8, [4]))
            t = ch["t"].astype(np.int64)
            d = int(t[4] - (t[3] + 20)) if up else int(t[3] - (t[4] + 20))
            assert d == sd + delta, (d, sd + delta)
            return scase(ch, splitdist=sd)
        pair("split.T.up/" + z, tcut(0, True), tcut(1, True))
        pair("split.T.down/" + z, tcut(0, False), tcut(1, False))
        single("split.T.up-1/" + z, tcut(-1, True)); single("split.T.down-1/" + z, tcut(-1, False))
        # the I cut: split_link 1
        pair("split.I/" + z, scase(make_chain([20] * 10, s, False, flips=(5,), cluster=cl(10, [5]))), scase(make_chain([20] * 10, s, False, cluster=cl(10, [5]))))
    # failed pushes and CHROMIndex: TStart + 1 and TEnd are looked up in pos[]
    def at(tstart, n=6, chrom=CHROM):
        """a forward run whose TStart (the last anchor's t) is tstart"""
        ch = make_chain([20] * n, 0, False)
        return scase(shifted(ch, tstart - int(ch["t"][-1])), chrom=chrom)
    pair("split.chrom.spans_boundary", at(3_000_000 - 50), at(3_000_000 + 50))
    pair("split.chrom.TStart+1==pos", at(3_000_000 - 1), at(3_000_000 - 2))
    def tend(te, chrom):
        ch = make_chain([20] * 6, 0, False)
        return scase(shifted(ch, te - 20 - int(ch["t"][0])), chrom=chrom)
    small = [0, 3_000_000, 6_000_000]
    pair("split.chrom.TEnd==pos[last]", tend(6_000_000, small), tend(6_000_000 - 1, small))
    pair("split.chrom.TEnd==pos[last]+1", tend(6_000_000 + 1, small), tend(6_000_000, small))
    OOB.append("split.chrom.TEnd==pos[last]+1/a")
    # MergeSplitchainINS: A | X | A' ...: the gap at X throws the chain far away, the gap at A' brings it back to `tdist` from A
    def aXa(tdist, s=0, lens=(4, 3, 4), far=(200_000,), back_flip=False, t_of_A=None, bypass=1, tail=0, links=None):
        """pieces of the given sizes; piece 1, 3, .. far away (T cuts), piece 2, 4, .. back at |c.TStart - nn.TEnd| = tdist from piece 0 (a list: one per return);
        tail: one more far piece at the end"""
        sizes = list(lens) + ([3] if tail else [])
        n = sum(sizes); starts = np.cumsum([0] + sizes)[:-1].tolist()
        tds = tdist if isinstance(tdist, (list, tuple)) else [tdist] * len(sizes)
        gaps = {}
        fars = list(far) * len(sizes)
        flips = (starts[2], ) if back_flip else ()
        def build():
            return make_chain([20] * n, s, False, gaps=gaps, flips=flips, cluster=cl(n, starts[1:]), link=links)
        sign = 1 if s == 0 else -1
        for k in range(1, len(sizes)):
            if k % 2 == 1 or (tail and k == len(sizes) - 1):
                gaps[starts[k]] = sign * fars[k] * (k + 1)
                continue
            gaps[starts[k]] = -sum(gaps.values())
            for _ in range(3):
                ch = build()
                t = ch["t"].astype(np.int64)
                a0, a1 = starts[0], starts[1]; b0 = starts[k]; b1 = b0 + sizes[k]
                cTS = t[a1 - 1] if s == 0 else t[a0]
                nTE = t[b0] + 20 if ch["strand"][b0] == 0 else t[b1 - 1] + 20
                cur = abs(int(cTS - nTE))
                if cur == tds[k]: break
                gaps[starts[k]] += (tds[k] - cur) * (-1 if cTS > nTE else 1)
            assert cur == tds[k], (cur, tds[k])
        ch = build()
        if t_of_A is not None: ch = shifted(ch, t_of_A - int(ch["t"][starts[1] - 1]))
        return scase(ch, bypass=bypass)
    for by in (0, 1):
        z = "by%d" % by
        for s in (0, 1):
            pair("split.merge.tdist<=1500/s%d/%s" % (s, z), aXa(1500, s, bypass=by, tail=1), aXa(1501, s, bypass=by, tail=1))
        pair("split.merge.other_strand/" + z, aXa(1000, bypass=by, tail=1), aXa(1000, back_flip=True, bypass=by, tail=1))
        pair("split.merge.other_chrom/" + z, aXa(1000, bypass=by, tail=1, t_of_A=3_000_500), aXa(1000, bypass=by, tail=1, t_of_A=3_002_000))
        # A X A' Y A'': A' lies 1000 below A and reaches 1140 below it; A'' at 2600 below A is within 1500 of the MERGED piece only, at 2700 of neither
        pair("split.merge.chained/" + z, aXa([0, 0, 1000, 0, 2600], lens=(4, 3, 4, 3, 4), bypass=by, tail=1), aXa([0, 0, 1000, 0, 2700], lens=(4, 3, 4, 3, 4), bypass=by, tail=1))
        pair("split.merge.skipped/" + z, aXa([0, 0, 40000, 0, 1000], lens=(4, 3, 4, 3, 4), bypass=by, tail=1), aXa([0, 0, 40000, 0, 1501], lens=(4, 3, 4, 3, 4), bypass=by, tail=1))
        single("split.merge.two_pieces/" + z, aXa(1000, lens=(4, 3), bypass=by))
        single("split.merge.last_piece/" + z, aXa(1000, lens=(4, 3, 4), bypass=by))
    pair("split.merge.bypass", aXa(1000, bypass=0, tail=1), aXa(1000, bypass=1, tail=1))
    pair("split.merge.bypass.links", aXa(1000, bypass=0, tail=1, links=[1] * 13), aXa(1000, bypass=1, tail=1, links=[1] * 13))
    # RemoveSpuriousSplitChain: a piece goes below min(filter, 2) = 2, behind an I link below min(filterDI, 4) with filterDI = max(floor(0.03 total), 2)
    def rss(total, m, first=40, s=0, inv=True):
        """`total` anchors: `first`, then a piece of m behind an I link (inv) or a T link, then the rest behind another such link"""
        if inv: ch = make_chain([20] * total, s, False, flips=(first, first + m), cluster=cl(total, [first, first + m]))
        else: ch = make_chain([20] * total, s, False, gaps={first: 300_000, first + m: 300_000}, cluster=cl(total, [first, first + m]))
        return scase(ch)
    for s in (0, 1):
        z = "s%d" % s
        pair("split.rss.total99|100/" + z, rss(99, 2, s=s), rss(100, 2, s=s))
        pair("split.rss.total133|134/" + z, rss(133, 3, s=s), rss(134, 3, s=s))
        pair("split.rss.size1|2/" + z, rss(60, 1, s=s, inv=False), rss(60, 2, s=s, inv=False))
        pair("split.rss.size3.I|T/" + z, rss(140, 3, s=s), rss(140, 3, s=s, inv=False))
        pair("split.rss.size2.I|T/" + z, rss(110, 2, s=s), rss(110, 2, s=s, inv=False))
        pair("split.rss.piece0_goes/" + z, rss(60, 5, first=1, s=s, inv=False), rss(60, 5, first=2, s=s, inv=False))
        pair("split.rss.piece0_goes.I/" + z, rss(60, 5, first=1, s=s), rss(60, 5, first=2, s=s))
        # a later piece: four pieces, the third of size 1
        lp = lambda m3, s=s: scase(make_chain([20] * 40, s, False, gaps={10: 300_000, 20: 300_000, 20 + m3: 300_000}, cluster=cl(40, [10, 20, 20 + m3])))
        pair("split.rss.piece2_goes/" + z, lp(1), lp(2))
        lpi = lambda m3, s=s: scase(make_chain([20] * 140, s, False, flips=(10,), gaps={20: 300_000, 20 + m3: 300_000}, cluster=cl(140, [10, 20, 20 + m3])))
        pair("split.rss.I_then_T_pieces/" + z, lpi(1), lpi(2))
        # piece 1 of size 1 behind a T link, piece 2 behind an I link: slot 0 of split_link keeps its own entry (`c > 1` in the reference)
        p1 = lambda m, s=s: scase(make_chain([20] * 40, s, False, gaps={10: 300_000}, flips=(10 + m,), cluster=cl(40, [10, 10 + m])))
        pair("split.rss.piece1_goes.T_then_I/" + z, p1(1), p1(2))
    # A | X | A' | B with X on the other strand and ending next to A': links 0 (T), 1 (I), 0 (T).  After the merge bypassClustering rewrites split_link from
    # the pieces' types (1, 0); without it the first two old entries stay (0, 1)
    bsl = lambda by: scase(make_chain([20] * 18, 0, False, flips=(4, 11), gaps={4: -60000, 5: 9000, 6: 9000, 7: 9000, 8: 9000, 9: 9000, 10: 9000, 11: 4780, 15: -300_000},
                                      cluster=cl(18, [4, 11, 15])), bypass=by)
    pair("split.merge.bypass.split_link", bsl(0), bsl(1))
    # coordinates: a whole chain at 3.0e9 and one across 2^31, cut and merged like its low twin
    for nm, c in (("split.merge", aXa(1000, tail=1)), ("split.I", scase(make_chain([20] * 10, 0, False, flips=(5,)))), ("split.N", scase(make_chain([20] * 8, 1, False, gaps={4: 10}, sp={4: 1000})))):
        single(nm + ".3e9", dict(c, chain=shifted(c["chain"], 3_000_000_000)))
        single(nm + ".x2^31", dict(c, chain=cross_t(c["chain"], 2, 1 << 31)))


OOB = []            # names of cases ("pair/a") for which the oracle returns None and the kernel must flag the slot


# ---- the high-accuracy split walk ---------------------------------------------------------------------------------------------------------------------------
def _hsplit():
    SD = 100000
    bx = lambda q, ql, t, tl: [q, q + ql, t, t + tl]
    def two(ts_cur, st=(0, 0), link=0, chrom=(0, 0), tl=(1000, 1000), ts_prev=500_000):
        return hcase(st, chrom, [bx(100, 1000, ts_prev, tl[0]), bx(1200, 1000, ts_cur, tl[1])], [link], SD)
    # T: tS(cur) > tE(prev) + splitdist; tE(cur) + splitdist < tS(prev)
    for st in ((0, 0), (1, 1)):
        z = "s%d" % st[0]
        pair("hsplit.T.up/" + z, two(501_000 + SD, st), two(501_000 + SD + 1, st)); single("hsplit.T.up-1/" + z, two(501_000 + SD - 1, st))
        pair("hsplit.T.down/" + z, two(500_000 - SD - 1000, st), two(500_000 - SD - 1001, st)); single("hsplit.T.down+1/" + z, two(500_000 - SD - 999, st))
    pair("hsplit.T.chrom", two(501_100), two(501_100, chrom=(0, 1)))
    # D: (link 1, strands 0 0) or (link 0, strands 1 1), both overlap rates >= 0.6 (600 / 1000 in float is 0.6f > 0.6)
    for st, lk in (((0, 0), 1), ((1, 1), 0)):
        z = "s%d" % st[0]
        pair("hsplit.D.ovl600|599/" + z, two(500_400, st, lk), two(500_401, st, lk))
        pair("hsplit.D.prev_only/" + z, two(500_400, st, lk, tl=(1000, 800)), two(500_401, st, lk, tl=(1000, 800)))          # 600/1000 | 599/1000, cur 0.75
        pair("hsplit.D.cur_only/" + z, two(500_000, st, lk, tl=(800, 1000), ts_prev=499_800), two(500_000, st, lk, tl=(800, 1000), ts_prev=499_799))   # cur 600/1000 | 599/1000, prev 0.75
        pair("hsplit.D.one_direction/" + z, two(500_000, st, lk, tl=(500, 1000)), two(500_000, st, lk, tl=(500, 800)))        # prev 1.0 both; cur 0.5 | 0.625
        pair("hsplit.D.link/" + z, two(500_100, st, lk), two(500_100, st, 1 - lk))
        pair("hsplit.D_before_T/" + z, two(500_100, st, lk), two(500_100, st, lk, chrom=(0, 1)))
    pair("hsplit.I", two(501_100, (0, 1)), two(501_100, (0, 0)))
    pair("hsplit.I'", two(501_100, (1, 0), 1), two(501_100, (1, 1), 1))
    # merge: A | X | A' | B, A' back at tdist from A; A' as the last piece is never merged onto
    def axab(tdist, tail=True, st=0, chromA2=0):
        A = bx(100, 1000, 500_000, 1000); X = bx(1200, 500, 900_000, 500)
        A2 = bx(1800, 1000, 500_000 - tdist - 1000, 1000); B = bx(3000, 700, 100_000, 700)
        b = [A, X, A2] + ([B] if tail else [])
        return hcase([st] * len(b), [0, 0, chromA2, 0][:len(b)], b, [0] * (len(b) - 1), SD)
    for st in (0, 1):
        pair("hsplit.merge.tdist<=1500/s%d" % st, axab(1500, st=st), axab(1501, st=st))
    pair("hsplit.merge.never_last", axab(1000), axab(1000, tail=False))
    single("hsplit.merge.other_chrom", axab(1000, chromA2=1))
    # LargestSplitChain_dist: the first of two equal widest pieces; qe <= qs counts as width 0
    def lsc(widths):
        b = []; t = 100_000
        for w in widths: b.append([5000, 5000 + w, t, t + 800]); t += 300_000
        return hcase([0] * len(b), [0] * len(b), b, [0] * (len(b) - 1), SD)
    pair("hsplit.lsc.equal_widest", lsc([500, 900, 900, 100]), lsc([500, 900, 901, 100]))
    pair("hsplit.lsc.qe<=qs", lsc([0, -40, 0]), lsc([0, 40, 0]))
    pair("hsplit.lsc.first_is_widest", lsc([900, 900]), lsc([899, 900]))
    single("hsplit.n=1", hcase([1], [2], [bx(5, 50, 700, 90)], [], SD))
    single("hsplit.n=0", hcase([], [], [], [], SD))
    single("hsplit.3e9", hcase([0, 0, 0], [0, 0, 0], [bx(100, 1000, 3_000_000_000, 1000), bx(1200, 1000, 3_000_000_400, 1000), bx(2300, 1000, 3_000_001_400 + SD + 1, 1000)], [1, 0], SD))
    single("hsplit.x2^31", hcase([1, 1], [0, 0], [bx(100, 1000, (1 << 31) - 500, 1000), bx(1200, 1000, (1 << 31) - 100, 1000)], [0], SD))


_filters()
_refine_ends()
_qend_links_orders()
_coordinates()
_layout()
_split()
_hsplit()
