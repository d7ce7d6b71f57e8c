"""Crafted jobs for LocalRefineAlignment / RefinedAlignmentbtwnAnchors (local_refine.hip, stage a13): one read, one to three chains of exact-match anchors on a
small two-chromosome genome, each built to sit on one side of one comparison of the walk.  A chain is written in the alignment's own coordinates as pieces: runs
of abutting exact anchors (nothing lies between two of them, so "blocks so far" = "anchors so far"), spaces whose read side is a function of the genome side
(copied, mutated, inverted, junk, edited with indels), and raw jumps (overlaps).  Every case exists on both strands.  `expected()` runs the oracle with its trace;
`mirror_pairs()` is a second, plain statement of the arithmetic that depends on the anchors alone (type, K / W / maxFreq, diagonal band).

Not built, on purpose: the K = 6 branch (max(rd, gd) < 100) cannot be reached, because a space is large only when min(rd, gd) >= 300; the non-ONT band's cap of
500 needs a space of 50 000 bases, too large for a unit test.  Could not be steered to: a single anchor under 100 bases between two gaps of OPPOSITE sign (the
inner sparse DP never chains it, so the length limit sits on same-sign gaps and the opposite-sign clauses on runs of short anchors); lr_decide's nf >= nr with
nr > 0 (a tried space has at most a handful of forward seeds, and a reverse set that small breaks the alignment unless its identity is 0.8, which brings seeds);
the two break clauses of lr_decide apart from each other when nr == 0 (they agree there).  Overlap by one base on the way to a LARGE space (gd >= 300) is guarded
in the kernel like the overlaps of two or more, but has no case: only the two named overlap families may be undefined.

Where each limit lives: classification_cases (min 300, max 500, abutting, cge against ngs, RefineBySDP off, chromosome ends), band_cases (ONT 100 / 2000, others
80, 2 sv, the pair where the band decides), reverse_cases (999 | 1000 for inverted / junk / mutated spaces, identity 0.8, 4 | 5 blocks, a second event 3 | 6 blocks
on, the drift clause, events on a chain's first and last pair, inverted anchors without boundary anchors), inner_cases (gaps of 30 | 31, anchors of 99 | 100, the
three distance limits, the final piece), walk_cases (chains of 0 / 1 / 2+ anchors, ties, secondary jobs, an explicit LSC, an event in a second chain),
overlap_cases.  Shared by tests/test_local_refine_edges.py.  Plain helpers, CPU only, no fixtures."""
import zlib

import numpy as np

from lra_amd import synth

import oracle_lib as O

M32 = 1 << 32
CH = [0, 50_000, 120_000]
ALEN = 40
_G = None


def genome():
    global _G
    if _G is None:
        _G = synth.make_genome(CH[-1], seed=4242, repeat_frac=0.0)
    return _G


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _other(b, k=1):
    return synth.BASES[(synth.CODE[b] + k) % 4]


# ---- what the read holds opposite a genome stretch g ---------------------------------------------------------------------------------------------------------
def sp_copy(g, rng): return g.copy()
def sp_inv(g, rng): return synth.revcomp(g)
def sp_junk(n): return lambda g, rng: synth.BASES[rng.integers(0, 4, n)]


def sp_mut(rate):
    def f(g, rng):
        s = g.copy(); m = rng.random(len(s)) < rate
        s[m] = _other(s[m], rng.integers(1, 4, int(m.sum())))
        return s
    return f


def sp_every(step, inv=False, cut=None):
    """a substitution every `step` bases (no exact K-mer of 12 survives at step 10, the identity stays 1 - 1 / step); inv: of the reverse complement;
    cut = (at, n): n genome bases left out at `at`"""
    def f(g, rng):
        s = g.copy()
        if cut: s = np.concatenate([s[:cut[0]], s[cut[0] + cut[1]:]])
        s[step // 2::step] = _other(s[step // 2::step])
        return synth.revcomp(s) if inv else s
    return f


def sp_edit(ops):
    """("m", n) copied, ("x", n) copied with a substitution every 25 bases, ("s", n) n substituted bases (an exact match ends there), ("d", n) genome bases left
    out, ("i", n) junk inserted (its first and last base differ from the genome bases an exact match could run into)"""
    def f(g, rng):
        out = []; t = 0
        for op, n in ops:
            if op == "m": out.append(g[t:t + n].copy()); t += n
            elif op == "x":
                s = g[t:t + n].copy(); s[12::25] = _other(s[12::25]); out.append(s); t += n
            elif op == "s": out.append(_other(g[t:t + n], 2)); t += n
            elif op == "d": t += n
            else:
                s = synth.BASES[rng.integers(0, 4, n)]
                if t < len(g): s[0] = _other(g[t]); s[-1] = _other(g[t - 1], 2) if s[-1] == g[t - 1] else s[-1]
                out.append(s)
        assert t == len(g), (t, len(g))
        return np.concatenate(out)
    return f


# ---- chains and jobs -----------------------------------------------------------------------------------------------------------------------------------------
def make_chain(name, pieces, strand, chrom=0, place=None, alen=ALEN):
    """pieces: ("A", n) n abutting exact anchors; ("S", gd, f) a space of gd genome bases, f(g, rng) its read side; ("X", dq, dt) the next anchor starts dq / dt
    bases after the end of the last one (negative: it overlaps; positive: junk / skipped genome).  place: None anywhere, "start" / "end" flush with the
    chromosome's first / last base.  Returns dict(seg, anchors [(qr, tr, len)] ascending, marks [index of the anchor before each S / X piece], strand, chrom)."""
    rng = _rng(name)
    G = genome()
    span = sum(p[1] * alen if p[0] == "A" else p[1] if p[0] == "S" else p[2] for p in pieces)
    clen = CH[chrom + 1] - CH[chrom]
    t0 = 0 if place == "start" else clen - span if place == "end" else int(rng.integers(2000, clen - span - 2000))
    seg = np.zeros(0, np.uint8); t = t0; anchors = []; marks = []
    for p in pieces:
        if p[0] == "A":
            for _ in range(p[1]):
                anchors.append((len(seg), t, alen)); seg = np.concatenate([seg, G[CH[chrom] + t:CH[chrom] + t + alen]]); t += alen
        elif p[0] == "S":
            marks.append(len(anchors) - 1)
            g = G[CH[chrom] + t:CH[chrom] + t + p[1]]
            seg = np.concatenate([seg, p[2](g, rng)]); t += p[1]
        else:
            marks.append(len(anchors) - 1)
            seg = seg[:len(seg) + p[1]] if p[1] < 0 else np.concatenate([seg, synth.BASES[rng.integers(0, 4, p[1])]])
            t += p[2]
    return dict(seg=seg, anchors=anchors, marks=marks, strand=int(strand), chrom=int(chrom))


EMPTY = dict(seg=np.zeros(0, np.uint8), anchors=[], marks=[], strand=0, chrom=0)


def make_job(name, family, chains, h=0, lsc=None, opts=None, expect=None, tag=None, none_ok=False):
    """The arrays of one job.  The read is the chains' segments one after the other (reverse-complemented for strand 1) with junk around them; anchors are given
    as the kernels take them: forward-read q, chromosome-relative t, chain order = descending q.  expect: {field: value} the trace must show at the first mark of
    the first chain with one; tag: (limit, side) for the registry of limits."""
    rng = _rng(name + "/job")
    parts = [synth.BASES[rng.integers(0, 4, 23)]]; offs = []
    for c in chains:
        offs.append(sum(len(x) for x in parts))
        parts += [synth.revcomp(c["seg"]) if c["strand"] else c["seg"], synth.BASES[rng.integers(0, 4, 31)]]
    read = np.concatenate(parts).astype(np.uint8)
    off = [0]; aq = []; at = []; al = []
    for c, o in zip(chains, offs):
        rows = [((o + len(c["seg"]) - qr - ln) if c["strand"] else (o + qr), tr, ln) for (qr, tr, ln) in c["anchors"]]
        rows.sort(key=lambda x: -x[0])
        aq += [r[0] for r in rows]; at += [r[1] for r in rows]; al += [r[2] for r in rows]; off.append(len(aq))
    nch = len(chains)
    return dict(name=name, family=family, chains=chains, read=read, off=np.array(off, np.int64), aq=np.array(aq, np.uint32), at=np.array(at, np.uint32),
                al=np.array(al, np.int32), strand=[c["strand"] for c in chains], chrom=[c["chrom"] for c in chains], value=[float(100 + 1.5 * i) for i in range(nch)],
                n0=[7 + i for i in range(nch)], n1=[len(c["anchors"]) for c in chains], h=int(h), lsc=lsc, opts=dict(opts or {}), expect=dict(expect or {}), tag=tag,
                none_ok=none_ok)


def trace_cur(chain, i_asc):
    """the trace's `cur` of the pair that starts at the chain's i_asc-th anchor (ascending alignment coordinate)"""
    return i_asc if chain["strand"] else len(chain["anchors"]) - 1 - i_asc


def probe(job, rows, which=0):
    """the trace record of the which-th marked pair of the job (chains in order)"""
    k = 0
    for ci, c in enumerate(job["chains"]):
        for m in c["marks"]:
            if k == which:
                hit = [r for r in rows if int(r["chain"]) == ci and int(r["cur"]) == trace_cur(c, m)]
                assert len(hit) == 1, (job["name"], which, len(hit))
                return hit[0]
            k += 1
    raise AssertionError((job["name"], which))


def job_lsc(job, high):
    """LargestSplitChain as the caller of the high-accuracy overload hands it over (the case's own, or the first largest chain)"""
    if high and job["lsc"] is not None: return int(job["lsc"])
    sizes = np.diff(job["off"])
    return int(np.argmax(sizes)) if len(sizes) else 0


def job_opts(job, is_ont):
    d = dict(isOnt=int(is_ont)); d.update(job["opts"])
    return d


def expected(job, high, is_ont, trace=True):
    """the oracle's alignments (None: undefined) and its trace for one job under one overload and one option set"""
    fwd = job["read"].tobytes(); rc = synth.revcomp(job["read"]).tobytes()
    return O.local_refine_alignment(job["off"], job["aq"], job["at"], job["al"], job["strand"], job["chrom"], job["value"], job["n0"], job["n1"], job["h"], fwd, rc,
                                    genome().tobytes(), CH, lsc=job_lsc(job, high), min_anchors=1 if high else 2, trace=trace, **job_opts(job, is_ont))


# ---- the second statement of the anchor-only arithmetic ----------------------------------------------------------------------------------------------------
def mirror_pairs(job, high, is_ont, local_max_freq=15):
    """RefinedAlignmentbtwnAnchors :209-283 for every pair in walk order, from the anchors alone: type, rd, gd and, for a large space, K, W, maxFreq, diag, sv"""
    o = job_opts(job, is_ont)
    L = len(job["read"]); out = []
    f32 = np.float32
    for ci in range(len(job["strand"])):
        a0, a1 = int(job["off"][ci]), int(job["off"][ci + 1]); m = a1 - a0
        if m < (1 if high else 2): continue
        q = [int(x) for x in job["aq"][a0:a1]]; t = [int(x) for x in job["at"][a0:a1]]; ln = [int(x) for x in job["al"][a0:a1]]
        st = job["strand"][ci]
        for step in range(m - 1):
            cur = step if st else m - 1 - step; nx = cur + 1 if st else cur - 1
            if st == 0: cre, nrs = q[cur] + ln[cur], q[nx]
            else: cre, nrs = L - q[cur], L - q[nx] - ln[nx]
            cge, ngs = t[cur] + ln[cur], t[nx]
            r = dict(chain=ci, cur=cur, type=0)
            if cge <= ngs:
                rd, gd = (nrs - cre) % M32, (ngs - cge) % M32
                r.update(rd=rd, gd=gd, type=1)
                if o.get("refineBySDP", 1) and min(rd, gd) >= 300:
                    sv = max(rd, gd) - min(rd, gd)
                    if o["isOnt"]: d = min(int(np.floor(max(f32(100), f32(0.15) * f32(rd)))), 2000)
                    else: d = min(int(np.floor(max(f32(80), f32(0.01) * f32(rd)))), 500)
                    d = max(2 * sv, d)
                    K, W, mf = (6, 5, local_max_freq) if max(rd, gd) < 100 else (9, 7, 50) if max(rd, gd) < 500 else (12, 7, local_max_freq)
                    r.update(type=2, K=K, W=W, maxFreq=mf)
                    if rd < 1 << 31: r.update(diag=d, sv=sv)               # (a read span that wrapped: the reference's int arithmetic on it is undefined)
            out.append(r)
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------------
def _both(name, family, pieces, **kw):
    """the same chain on both strands (and on both chromosomes); seed: the name that places the chain and draws its junk, if not the case's own"""
    place = kw.pop("place", None); seed = kw.pop("seed", None) or name
    return [make_job("%s%s" % (name, "+-"[s]), family, [make_chain("%s/%d" % (seed, s), pieces, s, chrom=s, place=place)], **kw) for s in (0, 1)]


def _sized(rd, gd, rate=0.08):
    """a space of rd read bases against gd genome bases: the genome's first min(rd, gd) bases mutated, junk for the rest of the read side"""
    def f(g, rng):
        s = sp_mut(rate)(g[:min(rd, gd)], rng)
        return s if rd <= gd else np.concatenate([s, synth.BASES[rng.integers(0, 4, rd - gd)]])
    return f


def classification_cases():
    out = []
    big = dict(type=2); direct = dict(type=1)
    for rd, gd, lim, side, exp in [
            (299, 299, "min300/equal", "below", direct), (300, 300, "min300/equal", "at", big),
            (299, 3000, "min300/read", "below", direct), (300, 3000, "min300/read", "at", big),
            (3000, 299, "min300/genome", "below", direct), (3000, 300, "min300/genome", "at", big),
            (499, 400, "max500/read", "below", dict(type=2, K=9, W=7, maxFreq=50)), (500, 400, "max500/read", "at", dict(type=2, K=12, W=7, maxFreq=15)),
            (400, 499, "max500/genome", "below", dict(type=2, K=9, W=7, maxFreq=50)), (400, 500, "max500/genome", "at", dict(type=2, K=12, W=7, maxFreq=15)),
            (0, 60, "abut", "read", dict(type=1, rd=0, gd=60)), (60, 0, "abut", "genome", dict(type=1, rd=60, gd=0))]:
        out += _both("cls_%d_%d" % (rd, gd), "classify", [("A", 6), ("S", gd, _sized(rd, gd)), ("A", 3)], tag=(lim, side), expect=dict(exp, rd=rd, gd=gd))
    # abutting on both sides: every pair of an "A" run is one; cge == ngs + 1: the genome sides overlap by one base, nothing at all between
    out += _both("cls_abut_both", "classify", [("A", 6), ("X", 0, 0), ("A", 3)], tag=("abut", "both"), expect=dict(type=1, rd=0, gd=0))
    out += _both("cls_gen_touch", "classify", [("A", 6), ("X", 25, 0), ("A", 3)], tag=("cge_ngs", "equal"), expect=dict(type=1, rd=25, gd=0))
    out += _both("cls_gen_over1", "classify", [("A", 6), ("X", 25, -1), ("A", 3)], tag=("cge_ngs", "over"), expect=dict(type=0))
    # RefineBySDP off: a space of 2000 on both sides goes direct
    out += _both("cls_nosdp", "classify", [("A", 6), ("S", 2000, sp_mut(0.05)), ("A", 3)], opts=dict(refineBySDP=0), tag=("refineBySDP", "off"), expect=dict(type=1, rd=2000, gd=2000))
    out += _both("cls_sdp", "classify", [("A", 6), ("S", 2000, sp_mut(0.05)), ("A", 3)], tag=("refineBySDP", "on"), expect=dict(type=2, rd=2000, gd=2000))
    # the chromosome's first and last bases
    for place in ("start", "end"):
        out += _both("cls_300_%s" % place, "classify", [("A", 2), ("S", 300, _sized(300, 300)), ("A", 2)], place=place, expect=dict(type=2, K=9))
        out += _both("cls_299_%s" % place, "classify", [("A", 2), ("S", 299, _sized(299, 299)), ("A", 2)], place=place, expect=dict(type=1))
    return out


def band_cases():
    """the diagonal band: floor(max(100, 0.15 rd)) capped at 2000 (ONT), floor(max(80, 0.01 rd)) (others), then max(2 sv, .).  0.15 rd passes 100 between 666 and 667
    but its floor stays 100 up to 673, and 0.01 rd passes 80 at 8000 but its floor stays 80 up to 8099: each limit has the pair where the product crosses and the
    pair where the band itself changes."""
    out = []
    for rd, lim, side, ont, d in [(666, "ont100/product", "below", 1, 100), (667, "ont100/product", "above", 1, 100), (673, "ont100", "below", 1, 100), (674, "ont100", "above", 1, 101),
                                  (13333, "ont2000", "below", 1, 1999), (13334, "ont2000", "at", 1, 2000), (13341, "ont2000", "capped", 1, 2000),
                                  (7999, "non80/product", "below", 0, 80), (8001, "non80/product", "above", 0, 80), (8090, "non80", "below", 0, 80), (8110, "non80", "above", 0, 81)]:
        both = _both("band_%d" % rd, "band", [("A", 5), ("S", rd, sp_mut(0.10)), ("A", 2)], tag=(lim, side), expect=dict(type=2, rd=rd, gd=rd, sv=0, diag=d), opts=dict(isOnt=ont))
        out += both if rd < 10000 else both[:1] if rd != 13334 else both[1:]                        # the 13 kb spaces: one strand each, both strands among them
    # 2 sv just below and just above the band (ONT 100, others 80)
    for rd, gd, ont, lim, side, d in [(600, 649, 1, "2sv/ont", "below", 100), (600, 651, 1, "2sv/ont", "above", 102), (700, 739, 0, "2sv/non", "below", 80),
                                      (700, 741, 0, "2sv/non", "above", 82)]:
        out += _both("band_sv_%d" % gd, "band", [("A", 5), ("S", gd, _sized(rd, gd)), ("A", 2)], tag=(lim, side), expect=dict(type=2, rd=rd, gd=gd, diag=d), opts=dict(isOnt=ont))
    # the band matters: 90 bases left out, 700 copied, 90 inserted: the 700 lie on a diagonal 90 off, inside the ONT band of 100 and outside the other of 80
    ops = [("m", 600), ("d", 90), ("m", 700), ("i", 90), ("m", 610)]
    out += _both("band_matters", "band_matters", [("A", 5), ("S", 2000, sp_edit(ops)), ("A", 2)], expect=dict(type=2, rd=2000, gd=2000, sv=0))
    return out


def reverse_cases():
    out = []
    for side in (999, 1000):
        for kind, f in [("inv", sp_inv), ("junk", sp_junk(side)), ("mut", sp_mut(0.10))]:
            out += _both("rev_%s_%d" % (kind, side), "reverse", [("A", 6), ("S", side, f), ("A", 3)], tag=("side1000/" + kind, "below" if side < 1000 else "at"),
                         expect=dict(type=2, rd=side, gd=side))
    # below 1000 the identity is real: 0.9 with no exact 12-mer -> few pairs, yet no reverse try
    out += _both("rev_ident", "reverse", [("A", 6), ("S", 800, sp_every(10)), ("A", 3)], tag=("identity", "high"), expect=dict(type=2, nf=0, super=0, tried=0, outcome=3))
    out += _both("rev_ident_low", "reverse", [("A", 6), ("S", 800, sp_junk(800)), ("A", 3)], tag=("identity", "low"), expect=dict(type=2, super=1, tried=1))
    # the block-count clause: an inverted space after 4 and after 5 blocks
    for n in (4, 5):
        out += _both("rev_blocks_%d" % n, "blocks", [("A", n), ("S", 1500, sp_inv), ("A", 3)], tag=("blocks5", str(n)), expect=dict(type=2, super=1, blocks=n, tried=int(n >= 5)))
    # a second event 3 and 6 blocks after a first: the fresh alignment starts at 0 blocks
    for n in (3, 6):
        out += _both("rev_second_%d" % n, "blocks", [("A", 6), ("S", 1500, sp_inv), ("A", n), ("S", 1500, sp_inv), ("A", 3)], tag=("second", str(n)),
                     expect=dict(type=2, tried=1, outcome=2))
    # an inverted stretch with substitutions: several inverted anchors, no boundary anchors among them (btc_start 0, btc_end k - 1)
    out += _both("rev_inv_mut", "reverse", [("A", 6), ("S", 1500, lambda g, rng: synth.revcomp(sp_mut(0.05)(g, rng))), ("A", 3)], tag=("btc", "inverted"),
                 expect=dict(type=2, tried=1, outcome=2, btc_start=0))
    # lr_decide.  Both seed sets empty between 500 and 1000, the other strand's identity 0.9: only the drift clause can break, and it holds for ONT
    # (sv 65 <= 0.10 x 800) and not for the others (65 > max(50, 0.01 x 800))
    out += _both("rev_drift", "decide", [("A", 6), ("S", 865, sp_every(10, inv=True, cut=(400, 65))), ("A", 3)], tag=("drift", "both"),
                 expect=dict(type=2, rd=800, gd=865, nf=0, tried=1, nr=0))
    # events on the first and on the last pair of a chain
    out += _both("rev_first_pair", "events", [("A", 1), ("S", 1500, sp_junk(1500)), ("A", 7)], tag=("event_at", "first"), expect=dict(type=2, tried=0, blocks=1))
    out += _both("rev_last_pair", "events", [("A", 7), ("S", 1500, sp_junk(1500)), ("A", 1)], tag=("event_at", "last"), expect=dict(type=2, tried=1, outcome=0))
    return out


def inner_cases():
    """true sequence with edits inside a space of 3 kb: what the inner chain carries into RemovePairedIndels (pair version)"""
    out = []

    def add(name, ops, lim, side, seed=None, **exp):
        gd = sum(n for op, n in ops if op in "mxsd")
        out.extend(_both("inner_" + name, "inner", [("A", 6), ("S", gd, sp_edit(ops)), ("A", 3)], tag=(lim, side), expect=dict(type=2, **exp), seed=seed))
    # LinearExtend spans an anchor from its first to its last seed, so the length of the anchor between two gaps follows the minimizers, not the edit script: the
    # copied stretches of 102 and 106 bases below were found by search to give anchors of exactly 99 and 100 on both strands, and rm_max / kept_min pin that.
    # Between two OPPOSITE gaps of more than 30 a single anchor under 100 bases never enters the inner chain (the sparse DP skips it), so the length limit is
    # taken on same-sign gaps and the opposite-sign clauses on stretches of several short anchors.
    two = lambda gap, mid: [("m", 900), ("d", gap), ("s", 1), ("m", mid), ("s", 1), ("d", gap), ("m", 900)]
    add("len_99", two(45, 102), "len100", "99", seed="inner_same_102", rm_max=99)
    add("len_100", two(45, 106), "len100", "100", seed="inner_same_106", rm_max=-1, kept_min=100)
    add("gap_30", two(30, 82), "gap30", "30", seed="inner_same_82", rm_max=-1, kept_min=80)      # a gap of 30 is no gap
    add("gap_31", two(31, 82), "gap30", "31", seed="inner_same_82", inner_before=5, inner_after=4)
    opp = lambda far, ins: [("m", 600), ("x", 100), ("d", 100), ("x", far), ("i", ins), ("m", 700)]      # -100 then +ins, `far` bases of short anchors between
    for far in (470, 530):                                                 # |sum| = 700 >= 600: only the distance-under-500 clause is left
        add("sum700_%d" % far, opp(far, 800), "dist500", str(far))
    for far in (1150, 1250):                                               # |sum| = 500 < 600: distance under max(2 x 600, 1000)
        add("sum500_%d" % far, opp(far, 600), "dist2blink", str(far))
    for far in (950, 1050):                                                # |sum| = 200: distance under max(2 x 300, 1000)
        add("sum200_%d" % far, opp(far, 300), "dist1000", str(far))
    # where the inner chain ends: the space ends in a copy (the last inner anchor runs into the boundary anchor: no final piece) or in junk
    add("tail_copy", [("m", 600), ("x", 600), ("m", 300)], "final", "copy")
    add("tail_junk", [("m", 600), ("x", 600), ("i", 80), ("d", 80)], "final", "junk")
    add("head_junk", [("i", 80), ("d", 80), ("m", 600), ("x", 600)], "final", "head_junk")
    return out


def walk_cases():
    """chains of 0, 1, 2 and more anchors in several orders, ties for the largest, secondary jobs, an explicit LSC"""
    out = []
    for s in (0, 1):
        c = lambda n, tagc, st=None, ch=None: make_chain("walk/%s/%d/%d" % (tagc, n, s), [("A", n)], s if st is None else st, chrom=s if ch is None else ch)
        ev = make_chain("walk/ev/%d" % s, [("A", 6), ("S", 1500, sp_inv), ("A", 2)], s, chrom=1 - s)
        sfx = "+-"[s]
        out += [make_job("walk_0_2_1" + sfx, "walk", [EMPTY, c(2, "a"), c(1, "b")], tag=("sizes", "0_2_1")),
                make_job("walk_1_0_2" + sfx, "walk", [c(1, "a"), EMPTY, c(2, "b", st=1 - s)], h=1, tag=("sizes", "1_0_2")),
                make_job("walk_tie_2_2" + sfx, "walk", [c(2, "a"), c(2, "b", ch=1 - s)], tag=("tie", "2_2")),
                make_job("walk_tie_1_3_3" + sfx, "walk", [c(1, "a"), c(3, "b"), c(3, "c", st=1 - s)], h=2, tag=("tie", "1_3_3")),
                make_job("walk_only_1" + sfx, "walk", [c(1, "a")], tag=("sizes", "1")),
                make_job("walk_empty" + sfx, "walk", [EMPTY, EMPTY], tag=("sizes", "0_0")),
                make_job("walk_none" + sfx, "walk", [], tag=("sizes", "none")),
                make_job("walk_lsc_small" + sfx, "walk", [c(5, "a"), c(2, "b"), c(1, "d")], lsc=1, tag=("lsc", "not_largest")),
                make_job("walk_lsc_one" + sfx, "walk", [c(3, "a"), c(1, "b")], lsc=1, h=1, tag=("lsc", "one_anchor")),
                make_job("walk_event_second_chain" + sfx, "walk", [c(3, "a"), ev, c(1, "b")], tag=("sizes", "event"))]
    return out


def overlap_cases():
    """the next anchor starts before the current one ends on the read.  By one base the reference aligns nothing; by two or more it builds a string of negative length:
    undefined, the oracle answers None and the device must flag the job."""
    out = []
    out += _both("ovl_1", "overlap1", [("A", 6), ("X", -1, 50), ("A", 3)], tag=("overlap", "one"), expect=dict(type=1, rd=M32 - 1, gd=50))
    out += _both("ovl_5_small", "overlap_small", [("A", 6), ("X", -5, 50), ("A", 3)], tag=("overlap", "small"), expect=dict(type=1, rd=M32 - 5, gd=50), none_ok=True)
    out += _both("ovl_5_big", "overlap_big", [("A", 6), ("X", -5, 400), ("A", 3)], tag=("overlap", "big"), expect=dict(type=2, rd=M32 - 5, gd=400), none_ok=True)
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = classification_cases() + band_cases() + reverse_cases() + inner_cases() + walk_cases() + overlap_cases()
        assert len({j["name"] for j in _CASES}) == len(_CASES)
    return _CASES


def family(*names):
    return [j for j in all_cases() if j["family"] in names]
