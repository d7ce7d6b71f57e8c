"""a12 AffineOneGapAlign (aog.hip): every dispatch class, every path through solve(), both sides of every size limit.

aog.hip is several kernels behind one entry point; lra_aog_class_of_batch (the classification arithmetic the device code itself calls, run
on the host) says which one a (qLen, tLen, k0) problem takes: the class, and a path code (suffix band used; scores in LDS, in registers, in
rotating LDS windows or in the HBM work slot; sequence codes in LDS or not).  The CPU tests here pin down which (class, path) pairs exist
at all and that the GPU tests' inputs reach every one of them; the GPU tests compare HIP with oracle.affine_one_gap_align exactly (score, block
triples, status: integers, no tolerance).  The class of a problem depends on its lengths and band only, so sequences of a given shape can be
anything: mutated copies, unrelated pairs, N and lower-case bases."""
import functools
import random

import numpy as np
import pytest

PAR = (4, -3, -4)
PAR2 = (4, -1, -2)
ST_RANGE, ST_CAPACITY = 4, 8

# (class, path) -> the smallest (qLen, tLen, k0) that takes it: smallest qLen + tLen, then k0, then qLen.  What test_coverage_table's sweep finds; for
# the pairs no problem up to 400 x 400 reaches (marked *), an example from the sampled part of the sweep.
TABLE = {
    (1, 8): (35, 44, 35),          # LDS sweep, 64 KB, prefix band only
    (1, 9): (27, 82, 27),
    (2, 2): (2057, 2038, 11),      # * HBM slot: register sweep, codes in HBM
    (2, 6): (64, 64, 64),          # plain HBM sweep, no suffix band
    (2, 7): (39, 118, 39),         # plain HBM sweep with the suffix band
    (2, 10): (66, 127, 31),        # register sweep, codes in LDS
    (2, 12): (54, 58, 54),         # rolling LDS windows
    (3, 9): (0, 4, 1),
    (5, 8): (32, 32, 32),          # LDS sweep, 32 KB, prefix band only
    (6, 2): (6480, 6485, 31),      # *
    (6, 6): (4979, 5043, 40),      # *
    (6, 7): (3000, 3200, 70),      # *
    (7, 9): (8, 21, 6),
    (8, 9): (16, 45, 14),
    (9, 9): (21, 64, 21),
    (10, 10): (11, 25, 7),
    (11, 10): (9, 25, 8),
    (12, 10): (16, 25, 16),
    (14, 8): (0, 0, 1),
    (15, 8): (2, 4, 1),
    (16, 8): (3, 7, 2),
    (17, 8): (4, 11, 4),
    (18, 8): (6, 17, 6),
}
SAMPLED_ONLY = {(2, 2), (6, 2), (6, 6), (6, 7)}
PAST_SLOT = (9850, 10084, 40)      # needs more than the class 6 slot: LRA_ST_RANGE


def classes(q, t, k, par=PAR):
    from lra_amd.align import aog_class_of_batch
    return aog_class_of_batch(q, t, k, *par)


def test_table_path_codes():
    """TABLE's path numbers, spelt with the library's names (lra_amd.align.PATH_*, include/lra_hip.h LRA_AOG_PATH_*)."""
    from lra_amd.align import PATH_SUFFIX, PATH_SCORES_LDS, PATH_SCORES_REGS, PATH_SCORES_ROLLING, PATH_SCORES_HBM, PATH_CODES_LDS
    lds = PATH_SCORES_LDS | PATH_CODES_LDS
    names = {lds: 8, lds | PATH_SUFFIX: 9, PATH_SCORES_REGS | PATH_CODES_LDS: 10, PATH_SCORES_REGS: 2, PATH_SCORES_ROLLING | PATH_CODES_LDS: 12,
             PATH_SCORES_HBM: 6, PATH_SCORES_HBM | PATH_SUFFIX: 7}
    assert all(k == v for k, v in names.items()) and {f[1] for f in TABLE} == set(names.values())
    assert {f[1] for f in TABLE if f[0] in (10, 11, 12)} == {PATH_SCORES_REGS | PATH_CODES_LDS}
    assert {f[1] for f in TABLE if f[0] >= 14} == {lds}
    assert {f[1] for f in TABLE if f[0] in (2, 6)} == {2, 6, 7, 10, 12}


def form_of(shape, par=PAR):
    c, p = classes([shape[0]], [shape[1]], [shape[2]], par)
    return int(c[0]), int(p[0])


# ---------------------------------------------------------------- sequences of a given shape
def _rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def make_pair(rng, qLen, tLen, kind):
    """q, t of exactly these lengths.  'mut': the longer one is the shorter one with substitutions, small indels and one run inserted (or removed) to make
    up the length difference; 'unrel': unrelated; 'nlow': 'mut' with N in one and the other in lower case; 'same': no substitutions, one run."""
    lo, hi = min(qLen, tLen), max(qLen, tLen)
    a = _rnd(rng, lo)
    if kind == "unrel":
        b = _rnd(rng, hi)
    else:
        out = []
        for c in a:
            r = rng.random() if kind != "same" else 1.0
            if r < 0.05:
                out.append(rng.choice("ACGT"))
            elif r < 0.08:
                out.append(c + rng.choice("ACGT"))
            elif r < 0.11:
                continue
            else:
                out.append(c)
        b = "".join(out)
        if len(b) > hi:
            p = rng.randint(0, hi)
            b = b[:p] + b[p + len(b) - hi:]
        elif len(b) < hi:
            p = rng.randint(0, len(b))
            b = b[:p] + _rnd(rng, hi - len(b)) + b[p:]
    if kind == "nlow":
        a = a.replace("A", "N", 2)
        b = b.lower()
    q, t = (a, b) if qLen <= tLen else (b, a)
    if qLen == tLen and rng.random() < 0.5:
        q, t = t, q
    assert len(q) == qLen and len(t) == tLen
    return q.encode(), t.encode()


KINDS = ["mut", "unrel", "nlow", "mut", "same", "unrel", "mut", "mut"]


def neighbours(shape, form, want):
    """Up to `want` other shapes near `shape` that take the same (class, path), by the library's own answer."""
    q0, t0, k0 = shape
    cand = [(q0 + dq, t0 + dt, k0 + dk) for dk in (0, 1, -1) for dq in (0, 1, -1, 2, 5, -3) for dt in (0, 1, -1, 3, -2, 7) if (dq, dt, dk) != (0, 0, 0)]
    cand = [s for s in cand if s[0] >= 0 and s[1] >= 0 and s[2] >= 1]
    c, p = classes([s[0] for s in cand], [s[1] for s in cand], [s[2] for s in cand])
    return [s for s, cc, pp in zip(cand, c, p) if (int(cc), int(pp)) == form][:want]


@functools.lru_cache(maxsize=None)
def form_inputs():
    """The problems of test_every_form: {(class, path): [(q, t, k0), ...]}.  Per pair at least 20 (class 6: 3, each ~5 MB of work memory and a wave to itself):
    the smallest shape that takes the form, with mutated, unrelated, N / lower-case and identical sequences, and shapes next to it."""
    out = {}
    for form, small in sorted(TABLE.items()):
        rng = random.Random(1000 * form[0] + form[1])
        probs = []
        if form[0] == 6:
            for i, kind in enumerate(["mut", "unrel", "nlow"]):
                probs.append(make_pair(rng, small[0], small[1], kind) + (small[2],))
        else:
            for i in range(8):
                probs.append(make_pair(rng, small[0], small[1], KINDS[i]) + (small[2],))
            near = neighbours(small, form, 4)
            i = 0
            while len(probs) < 24:
                s = near[i % len(near)] if near else small
                probs.append(make_pair(rng, s[0], s[1], KINDS[i % len(KINDS)]) + (s[2],))
                i += 1
        out[form] = probs
    return out


def forms_of_problems(probs, par=PAR):
    c, p = classes([len(x[0]) for x in probs], [len(x[1]) for x in probs], [x[2] for x in probs], par)
    return list(zip(c.tolist(), p.tolist()))


# ---------------------------------------------------------------- a. coverage table (CPU)
def _sweep():
    """Every qLen, tLen <= 400 with k0 <= 130 (exhaustive), then a seeded sample up to 12000 with k0 up to 500: uniform lengths, log-uniform lengths with a
    small or a moderate length difference (where the prefix-only forms of the large classes live), short against anything."""
    L = np.arange(401, dtype=np.int32)
    q, t = [a.ravel() for a in np.meshgrid(L, L, indexing="ij")]
    for k0 in range(1, 131):
        yield True, q, t, np.full(q.size, k0, np.int32)
    rng = np.random.default_rng(20240612)
    n = 400000
    for mode in range(5):
        hi = [12000, 12000, 3000, 12000, 600][mode]
        q = rng.integers(0, hi + 1, n) if mode == 0 else np.exp(rng.uniform(0, np.log(hi), n)).astype(np.int64)
        if mode in (0, 4):
            t = rng.integers(0, hi + 1, n)
        else:
            d = 600 if mode == 3 else 40
            t = np.clip(q + rng.integers(-d, d + 1, n), 0, 12000)
        k = rng.integers(1, 80, n) if mode == 2 else rng.integers(1, 501, n)
        if mode % 2:
            q, t = t, q
        yield False, q.astype(np.int32), t.astype(np.int32), k.astype(np.int32)


def test_coverage_table():
    """The (class, path) pairs that occur are exactly TABLE's (plus LRA_ST_RANGE), TABLE's example of each is the smallest the exhaustive part of the sweep
    finds, and test_every_form's inputs reach every pair: >= 20 problems each (class 6: 3), the smallest shape among them.  (Classes 0 and 4, and the
    prefix-only forms of 3, 7, 8, 9, cannot occur: DESIGN.md, a12.)"""
    seen, smallest = set(), {}
    for exhaustive, q, t, k in _sweep():
        c, p = classes(q, t, k)
        key = c.astype(np.int64) * 16 + p
        for u in np.unique(key):
            form = (int(u) // 16, int(u) % 16) if u >= 0 else (-1, 0)
            seen.add(form)
            if exhaustive and form[0] >= 0:
                idx = np.flatnonzero(key == u)
                s = q[idx].astype(np.int64) + t[idx]
                o = idx[np.lexsort((q[idx], s))[0]]                       # (k0 is constant within one part of the exhaustive sweep, parts come in k0 order)
                cand = (int(q[o]) + int(t[o]), int(k[o]), int(q[o]), int(t[o]))
                if form not in smallest or cand < smallest[form]:
                    smallest[form] = cand
    assert seen == set(TABLE) | {(-1, 0)}, sorted(seen ^ (set(TABLE) | {(-1, 0)}))
    assert set(TABLE) - set(smallest) == SAMPLED_ONLY
    for form, cand in smallest.items():
        assert TABLE[form] == (cand[2], cand[3], cand[1]), (form, cand)
    for form in SAMPLED_ONLY:
        assert form_of(TABLE[form]) == form, form
    assert form_of(PAST_SLOT) == (-1, 0)
    # the scoring set moves no problem of these sizes to another class (it only enters the 2^28 score range check)
    for form, shape in TABLE.items():
        assert form_of(shape, PAR2) == form
    # the inputs of test_every_form
    inputs = form_inputs()
    assert set(inputs) == set(TABLE)
    for form, probs in inputs.items():
        assert all(f == form for f in forms_of_problems(probs)), form
        assert len(probs) >= (3 if form[0] == 6 else 20), (form, len(probs))
        assert any((len(x[0]), len(x[1]), x[2]) == TABLE[form] for x in probs), form
        assert len({(x[0], x[1]) for x in probs}) >= (3 if form[0] == 6 else 12), form                 # (sequences of at most 3 bases repeat)
        assert any(b"N" in x[0] + x[1] or x[0] + x[1] != (x[0] + x[1]).upper() for x in probs) or max(TABLE[form][:2]) < 3, form


# ---------------------------------------------------------------- running and comparing
_ORACLE = {}


def expected(oracle, q, t, k, par):
    """oracle.affine_one_gap_align, cached by (q, t, k, params); k0 < 1 is the library's own LRA_ST_RANGE (the reference has no such input)."""
    key = (q, t, k, par)
    if key not in _ORACLE:
        s, b, st = oracle.affine_one_gap_align(q, t, par[0], par[1], par[2], k, cap=min(len(q), len(t)) + 2)
        _ORACLE[key] = (int(s), b.astype(np.int32), int(st))
    return _ORACLE[key]


def run_raw(ctx, probs, par, caps=None, sentinel=None):
    """One lra_affine_one_gap_align_batch call.  caps: block slots per problem (default: what always suffices); the block buffer is pre-filled with
    `sentinel`.  Returns score, nblocks, status, blocks [slots, 3], block_off."""
    import torch
    from lra_amd.align import AogBatch
    b = AogBatch(ctx, [x[0] for x in probs], [x[1] for x in probs], [x[2] for x in probs], *par)
    if caps is not None:
        boff = np.zeros(len(probs) + 1, dtype=np.int64)
        boff[1:] = np.cumsum(np.asarray(caps, dtype=np.int64))
        b.block_off_h = boff
        b.block_off = torch.from_numpy(boff).to(ctx.device)
        b.blocks = torch.empty(max(1, int(boff[-1])) * 3, dtype=torch.int32, device=ctx.device)
    if sentinel is not None:
        b.blocks.fill_(sentinel)
    b.run()
    torch.cuda.synchronize(ctx.device)
    return b.score.cpu().numpy(), b.nblocks.cpu().numpy(), b.status.cpu().numpy(), b.blocks.cpu().numpy().reshape(-1, 3), b.block_off_h


def check(ctx, oracle, probs, par=PAR):
    """HIP == oracle on every problem of the batch (LRA_ST_RANGE, score 0, no blocks where the library takes no problem); repeated problems are compared together."""
    score, nb, st, blocks, boff = run_raw(ctx, probs, par)
    where = {}
    for i, x in enumerate(probs):
        where.setdefault(x, []).append(i)
    cls = dict(zip(probs, forms_of_problems(probs, par)))
    for x, idx in where.items():
        idx = np.asarray(idx)
        tag = (len(x[0]), len(x[1]), x[2], par, int(idx[0]))
        if cls[x][0] < 0:                                                   # k0 < 1, or larger than the class 6 slot: the library's own LRA_ST_RANGE
            assert (st[idx] == ST_RANGE).all() and (score[idx] == 0).all() and (nb[idx] == 0).all(), tag
            continue
        es, eb, est = expected(oracle, x[0], x[1], x[2], par)
        assert not est & 2, tag                                             # (the reference never returns: nothing to compare -- no input here is built that way)
        assert (st[idx] == est).all(), tag + (st[idx[0]], est)
        assert (score[idx] == es).all(), tag + (score[idx[0]], es)
        assert (nb[idx] == len(eb)).all(), tag + (nb[idx[0]], len(eb))
        if len(eb):
            got = blocks[boff[idx][:, None] + np.arange(len(eb))[None, :]]
            assert (got == eb[None]).all(), tag
    return st


# ---------------------------------------------------------------- b. every reachable form (GPU)
@pytest.mark.gpu
def test_every_form(ctx, oracle):
    """>= 20 problems of every (class, path) pair -- 3 of each class 6 path -- in one mixed batch, then class by class; one problem past the class 6 slot and
    k0 = 0 / -1 are LRA_ST_RANGE with score 0 and no blocks, their neighbours in the batch right."""
    inputs = form_inputs()
    rng = random.Random(5)
    past = make_pair(rng, PAST_SLOT[0], PAST_SLOT[1], "mut") + (PAST_SLOT[2],)
    k0q, k0t = make_pair(rng, 40, 44, "mut")
    mixed = [x for form in sorted(inputs) for x in inputs[form]]
    rng.shuffle(mixed)
    at = [len(mixed) // 3, len(mixed) // 2, 2 * len(mixed) // 3]
    for pos, extra in zip(at, [(k0q, k0t, -1), past, (k0q, k0t, 0)]):
        mixed[pos:pos] = [extra]
    assert [f[0] for f in forms_of_problems([mixed[p] for p in at])] == [-1] * 3 and mixed[at[1]] is past
    assert all(f[0] >= 0 for i, f in enumerate(forms_of_problems(mixed)) if mixed[i] is not past and mixed[i][2] >= 1)
    check(ctx, oracle, mixed)
    by_class = {}
    for form in sorted(inputs):
        by_class.setdefault(form[0], []).extend(inputs[form])
    for cls, probs in sorted(by_class.items()):
        check(ctx, oracle, probs)
        check(ctx, oracle, probs[:24], PAR2)


# ---------------------------------------------------------------- c. both sides of every threshold
def _grid(qs, ts, ks):
    q, t, k = [a.ravel().astype(np.int32) for a in np.meshgrid(np.asarray(qs), np.asarray(ts), np.asarray(ks), indexing="ij")]
    return q, t, k


def flips(below, above, q, t, k, axis, want=64):
    """Pairs of problems one step apart along `axis` (0: qLen, 1: tLen, 2: k0), the first of form `below`, the second of form `above`: the closest inputs on
    either side of the comparison that separates the two forms, as the library itself classifies them.  `t` may be given relative to q (see callers)."""
    d = [np.zeros_like(q), np.zeros_like(q), np.zeros_like(q)]
    d[axis] = np.ones_like(q)
    c0, p0 = classes(q, t, k)
    c1, p1 = classes(q + d[0], t + d[1], k + d[2])
    hit = np.flatnonzero((c0 == below[0]) & (p0 == below[1]) & (c1 == above[0]) & (p1 == above[1]))
    if len(hit) > want:
        hit = hit[np.linspace(0, len(hit) - 1, want).astype(np.int64)]
    lo = [(int(q[i]), int(t[i]), int(k[i])) for i in hit]
    hi = [(int(q[i] + d[0][i]), int(t[i] + d[1][i]), int(k[i] + d[2][i])) for i in hit]
    return lo, hi


def _top(qs, gaps, ks):
    """long-gap shapes: tLen = qLen + 2 k0 + 1 + gap (the suffix band is used as soon as the length difference exceeds 2 k)"""
    q, g, k = _grid(qs, gaps, ks)
    return q, q + 2 * k + 1 + g, k


def _near(qs, ds, ks):
    q, d, k = _grid(qs, ds, ks)
    return q, np.maximum(q + d, 0), k


# name -> (form below, form above, candidate shapes, axis the step is taken along).  The step is along the axis the compared quantity is finest in: the long
# sequence's length for `need` of a long-gap problem (4 bytes every 4 bases), a length for the others, k0 for the band comparisons.
def thresholds():
    R = np.arange
    return {
        "need<=2560 (3|7)": ((3, 9), (7, 9), _top(R(1, 40), R(0, 200), [1, 2, 3, 5, 8, 12, 15]), 1),
        "need<=10K (7|8)": ((7, 9), (8, 9), _top(R(1, 80), R(0, 300), [2, 5, 9, 14, 20, 25, 31]), 1),
        "need<=20K (8|9)": ((8, 9), (9, 9), _top(R(1, 120), R(0, 300), [3, 8, 14, 20, 26, 31]), 1),
        "need<=32K (9|1)": ((9, 9), (1, 9), _top(R(1, 200), R(0, 400), [3, 8, 14, 21, 27, 31]), 1),
        "need<=32K (5|1) prefix-only": ((5, 8), (1, 8), _near(R(30, 80), R(-6, 7), R(32, 60)), 1),
        "need<=64K (1|2) long gap": ((1, 9), (2, 7), _top(R(1, 300), R(0, 400), [3, 8, 14, 21, 27, 33, 40]), 1),
        "need<=64K (1|2 rolling)": ((1, 8), (2, 12), _near(R(40, 140), R(-6, 7), R(32, 63)), 1),
        "k+2<=16 (10|11)": ((10, 10), (11, 10), _near(R(25, 60), R(-4, 5), [7]), 2),
        "k+2<=32 (11|12)": ((11, 10), (12, 10), _near(R(25, 160), R(-4, 5), [15]), 2),
        "k+2<=64 (12|5)": ((12, 10), (5, 8), _near(R(32, 60), R(-4, 5), [31]), 2),
        "k+2<=64 (12|1)": ((12, 10), (1, 8), _near(R(40, 130), R(-4, 5), [31]), 2),
        "k+2<=64 (2 regs|2 rolling)": ((2, 10), (2, 12), _near(R(130, 330, 7), R(-4, 5), [31]), 2),
        "k+2<=64 (2 regs, codes in HBM|2 plain HBM)": ((2, 2), (2, 6), _near(R(2050, 2300, 50), R(-3, 4), [31]), 2),
        "nr<=2048 (10|11)": ((10, 10), (11, 10), _near(R(25, 400), R(-14, 15), R(1, 8)), 1),
        "nr<=8192 (11|12)": ((11, 10), (12, 10), _near(R(25, 1300), R(-30, 31, 3), R(2, 16)), 1),
        "nr<=16384 (12|2)": ((12, 10), (2, 10), _near(R(60, 2600, 3), R(-40, 41, 5), R(3, 32, 2)), 1),
        "2k+3<=256 (2 rolling|2 plain HBM)": ((2, 12), (2, 6), _near(R(64, 700, 13), R(-5, 6), [63]), 2),
        "qLen+tLen+2<=4096 (2 regs)": ((2, 10), (2, 2), _near(R(2030, 2065), R(-8, 9), [1, 5, 11, 20, 31]), 1),
        "qLen+tLen+2<=4096 (2 rolling|2 plain HBM)": ((2, 12), (2, 6), _near(R(2030, 2065), R(-8, 9), [32, 40, 50, 63]), 1),
        "max len<=3 (14|15)": ((14, 8), (15, 8), _near(R(0, 5), R(-4, 5), R(1, 8)), 1),
        "max len<=6 (15|16)": ((15, 8), (16, 8), _near(R(0, 8), R(-7, 8), R(1, 8)), 1),
        "max len<=10 (16|17)": ((16, 8), (17, 8), _near(R(0, 12), R(-11, 12), R(1, 12)), 1),
        "max len<=16 (17|18)": ((17, 8), (18, 8), _near(R(0, 18), R(-17, 18), R(1, 18)), 1),
        "max len<=24 (18|10)": ((18, 8), (10, 10), _near(R(0, 26), R(-25, 26), R(1, 8)), 1),
        "max len<=24 (18|11)": ((18, 8), (11, 10), _near(R(0, 26), R(-25, 26), R(8, 16)), 1),
        "max len<=24 (18|12)": ((18, 8), (12, 10), _near(R(0, 26), R(-25, 26), R(16, 30)), 1),
    }


# k + 1 against 16 and against 32: long-gap problems whose band is exactly k0, one step apart, the same form on both sides
SAME_FORM_STEPS = [((16, 60, 15), (16, 60, 16)), ((20, 80, 15), (20, 80, 16)), ((32, 110, 31), (32, 110, 32)), ((40, 140, 31), (40, 140, 32)), ((200, 300, 31), (200, 300, 32))]

# one problem on either side is enough for the two HBM slot sizes (4 MiB of work memory and a wave each)
SLOT_THRESHOLDS = {
    "need<=4 MiB (2|6) plain HBM": ((2, 6), (6, 6), _near([4979], np.arange(40, 80), [40]), 1),
    "need<=4 MiB (2|6) regs": ((2, 2), (6, 2), _near([6400], np.arange(0, 200), [31]), 1),
    "need<=8 MiB (6|range)": ((6, 6), (-1, 0), _near(np.arange(9900, 10300), [0], [40]), 1),
}


@functools.lru_cache(maxsize=None)
def threshold_inputs():
    """{name: (at-limit problems, problems just past the limit)}: 64 of each with different sequences (16-lane groups: 16 problems per workgroup, lane
    kernels: 64 per wave -- a workgroup full of at-limit problems, so that one writing a byte past its slice lands in a neighbour that is checked too)."""
    out = {}
    for name, (below, above, (q, t, k), axis) in thresholds().items():
        lo, hi = flips(below, above, q, t, k, axis)
        assert lo, name
        rng = random.Random(name)
        big = max(s[0] + s[1] for s in lo) > 1500
        n = 8 if big else 64                                                # (the 4 kb problems sit in HBM slots, a wave each: nothing shares a slice with them)
        lo = [lo[i % len(lo)] for i in range(n)]
        hi = [hi[i % len(hi)] for i in range(n)]
        mk = lambda ss: [make_pair(rng, s[0], s[1], KINDS[i % len(KINDS)]) + (s[2],) for i, s in enumerate(ss)]
        out[name] = (below, above, mk(lo), mk(hi))
    for name, (below, above, (q, t, k), axis) in SLOT_THRESHOLDS.items():
        lo, hi = flips(below, above, q, t, k, axis, want=1)
        assert lo, name
        rng = random.Random(name)
        out[name] = (below, above, [make_pair(rng, lo[0][0], lo[0][1], "mut") + (lo[0][2],)], [make_pair(rng, hi[0][0], hi[0][1], "mut") + (hi[0][2],)])
    return out


def test_threshold_inputs_sit_on_both_sides():
    """Every comparison of the shared classifier has inputs one step apart that fall on either side of it (found with the library's own answer).
    Three comparisons separate no two forms -- k + 1 <= 16 and k + 1 <= 32 (a long-gap band of 15 needs more than class 3's 2560 bytes, one of 32 more than
    the 32 KB of classes 7 - 9; a prefix-only band is even and goes to the register classes) and need <= 64 KB for a prefix-only band of 2 k + 3 > 256 (65 rows
    of it are more than 64 KB): their two sides are SAME_FORM_STEPS, run on the GPU with the others."""
    inp = threshold_inputs()
    assert len(inp) == len(thresholds()) + len(SLOT_THRESHOLDS)
    for name, (below, above, lo, hi) in inp.items():
        assert all(f == below for f in forms_of_problems(lo)), name
        assert all(f == above for f in forms_of_problems(hi)), name
        assert len(lo) == len(hi) and len({x[:2] for x in lo}) >= (len(lo) if min(len(x[1]) for x in lo) > 12 else len(lo) // 2), name     # (short sequences repeat)
        for a, b in zip(lo, hi):
            assert abs(len(a[0]) - len(b[0])) + abs(len(a[1]) - len(b[1])) + abs(a[2] - b[2]) == 1, name
    for k0, never in ((15, {3}), (31, {0, 4, 5, 7, 8, 9})):                 # on either side of k + 1 = 16 / 32 no problem is small enough for the classes the comparison guards
        q, t, k = _top(np.arange(k0, 300), np.arange(0, 50), [k0, k0 + 1])
        assert not (set(classes(q, t, k)[0].tolist()) & never), k0
    q, t, k = _near(np.arange(74, 400), np.arange(-10, 11), np.arange(64, 131))         # (both sequences at least 64 long: the band is 2 k0)
    assert 1 not in set(classes(q, t, k)[0].tolist())
    for a, b in SAME_FORM_STEPS:
        assert form_of(a) == form_of(b), (a, b)


@pytest.mark.gpu
def test_both_sides_of_every_threshold(ctx, oracle):
    inp = threshold_inputs()
    for name, (below, above, lo, hi) in inp.items():
        check(ctx, oracle, lo)                                              # a batch of at-limit problems alone: they share workgroups with each other
        check(ctx, oracle, [x for pair in zip(lo, hi) for x in pair])
    rng = random.Random(16)
    check(ctx, oracle, [make_pair(rng, s[0], s[1], kind) + (s[2],) for pair in SAME_FORM_STEPS for s in pair for kind in ("mut", "unrel", "nlow", "mut")])


# ---------------------------------------------------------------- d. lane classes exhaustively
@pytest.mark.gpu
@pytest.mark.parametrize("seed,par", [(1, PAR), (2, PAR2)])
def test_lane_classes_exhaustive(ctx, oracle, seed, par):
    """Every (qLen, tLen) in [0, 25]^2 with k0 in {1, 2, 3, 7, 12, 13, 30}: both lengths zero, the two-word arrow rows of the 24-base class (more than 16
    cells in a band row), and 25, just outside the lane classes.  Two seeds of sequences, two scoring sets."""
    rng = random.Random(seed)
    probs = []
    for k0 in (1, 2, 3, 7, 12, 13, 30):
        for ql in range(26):
            for tl in range(26):
                probs.append(make_pair(rng, ql, tl, KINDS[(ql + tl + k0) % len(KINDS)]) + (k0,))
    forms = set(forms_of_problems(probs, par))
    assert {(c, 8) for c in (14, 15, 16, 17, 18)} <= forms
    check(ctx, oracle, probs, par)


# ---------------------------------------------------------------- e. second problem in the same slice or slot
def resident_groups(num_cu):
    """Groups (problems in flight) of each class's launch when the batch is large: aog.hip's grids (lra_aog_launch_device; a comment there points here)."""
    return {1: num_cu * 2, 2: num_cu * 8, 3: num_cu * 8 * 16, 5: num_cu * 5, 7: num_cu * 2 * 8, 8: num_cu * 4 * 2, 9: num_cu * 2 * 2,
            10: num_cu * 10 * 16, 11: num_cu * 10 * 4, 12: num_cu * 10,
            14: num_cu * 32 * 64, 15: num_cu * 32 * 64, 16: num_cu * 22 * 64, 17: num_cu * 14 * 64, 18: num_cu * 7 * 64}


# class -> (a large and a small shape of the class); 0 and 4 take no problem (test_coverage_table)
REUSE_SHAPES = {
    1: [(120, 400, 20), (35, 44, 35)], 2: [(700, 700, 40), (64, 64, 64)], 3: [(5, 40, 5), (0, 4, 1)], 5: [(40, 40, 36), (32, 32, 32)],
    7: [(30, 90, 9), (8, 21, 6)], 8: [(60, 140, 10), (16, 45, 14)], 9: [(120, 260, 9), (21, 64, 21)],
    10: [(90, 88, 4), (11, 25, 7)], 11: [(180, 178, 9), (9, 25, 8)], 12: [(200, 195, 16), (16, 25, 16)],
    14: [(3, 3, 2), (0, 1, 1)], 15: [(6, 5, 3), (2, 4, 1)], 16: [(10, 9, 4), (3, 7, 2)], 17: [(16, 14, 7), (4, 11, 4)], 18: [(24, 23, 12), (6, 17, 6)],
}


def test_reuse_shapes_are_of_their_class():
    assert set(REUSE_SHAPES) == {f[0] for f in TABLE} - {6}
    for cls, shapes in REUSE_SHAPES.items():
        assert [form_of(s)[0] for s in shapes] == [cls, cls], cls
    assert set(resident_groups(1)) == set(REUSE_SHAPES)


def reuse_batch(groups):
    """Which of six problems (size: 0 large / 1 small; sequences: 0 .. 2; index = size + 2 * sequences) sits at each position of a batch of one class whose
    launch has `groups` groups: every kernel hands group g the list positions g, g + groups, ..., so position p is round p // groups of slice p % groups.
    Neighbouring slices alternate large / small, and a slice's next round has the other size and other sequences."""
    i = np.arange(groups + groups // 2 + 7)
    g, r = i % groups, i // groups
    return (g + r) % 2 + 2 * ((g // 2 + r) % 3)


def test_reuse_batch_changes_shape_in_every_slice():
    """From the group counts and the batch order: the problem a slice takes second differs from its first in size and in sequences, both orders (small after
    large, large after small) occur, and more than `groups` problems are submitted.  (The class list aog_scatter builds keeps the batch order up to whole
    waves of 64 problems changing places; within one round every wave has the same pattern, so that changes nothing there.)"""
    for num_cu in (256, 304, 64, 8, 1):
        for cls, groups in resident_groups(num_cu).items():
            b = reuse_batch(groups)
            first, second = b[:len(b) - groups], b[groups:]
            assert len(b) > groups and len(second) >= groups // 2
            assert (first % 2 != second % 2).all() and (first // 2 != second // 2).all(), (num_cu, cls)
            assert {(int(a) % 2, int(c) % 2) for a, c in zip(first[:4], second[:4])} == {(0, 1), (1, 0)} or groups < 2, (num_cu, cls)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", sorted(REUSE_SHAPES))
def test_second_problem_in_the_same_slice(ctx, oracle, cls):
    """More problems of one class than its launch has resident groups: every LDS slice / HBM slot (and lane) of the first half of the grid takes a second
    problem, a small one after a large one and the other way round, with other sequences (reuse_batch).  Six distinct problems repeated.  Class 6 is left
    out: its launch has one 8 MiB slot per CU, and num_cu + 1 problems of more than 4 MiB each are too much for one test."""
    import torch
    num_cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    groups = resident_groups(num_cu)[cls]
    rng = random.Random(cls)
    big, small = REUSE_SHAPES[cls]
    distinct = [make_pair(rng, s[0], s[1], kind) + (s[2],) for kind in ("mut", "unrel", "nlow") for s in (big, small)]
    assert len({x[:2] for x in distinct}) == 6 or cls == 14                # (at most 3 bases: sequences may repeat)
    probs = [distinct[j] for j in reuse_batch(groups).tolist()]
    c, _ = classes([len(x[0]) for x in probs], [len(x[1]) for x in probs], [x[2] for x in probs])
    assert (c == cls).all() and int((c == cls).sum()) > groups
    check(ctx, oracle, probs)


# ---------------------------------------------------------------- f. staged traceback window
def _indel_cases(rng, T, k0, ch):
    """Problems of t length T whose prefix walk crosses the staged windows [T - (e + 1) ch + 1, T - e ch]: identical sequences; one base of t missing from q
    (a deletion) / one extra base in q (an insertion) at, one before and one after every window edge; runs of exactly 64 and 65 diagonal arrows that end on an edge."""
    t = _rnd(rng, T)
    edges = [T - e * ch for e in range(1, T // ch + 1) if T - e * ch >= 2]
    tl = list(t)
    for c in edges:                                                         # no two equal neighbours where a base goes missing: the gap has one place to be
        for p in (c, c + 65, c + 66):
            for x in range(max(1, p - 3), min(T - 1, p + 3)):
                while tl[x] == tl[x - 1]:
                    tl[x] = rng.choice("ACGT")
    t = "".join(tl)
    out = [(t, t)]
    for c in edges:
        for p in (c - 1, c, c + 1):                                         # 1-based row of t
            if 2 <= p <= T - 1:
                out.append((t[:p - 1] + t[p:], t))
                other = [b for b in "ACGT" if b != t[p - 1] and b != t[p - 2]][0]
                out.append((t[:p - 1] + other + t[p - 1:], t))
        for run in (64, 65):                                                # rows c + 1 .. c + run match, a missing base below and above them
            if c >= 2 and c + run + 1 <= T - 1:
                out.append((t[:c - 1] + t[c:c + run] + t[c + run + 1:], t))
    return [(q.encode(), t_.encode(), k0) for q, t_ in out]


WINDOW_CASES = [((2, 10), 300, 31), ((2, 10), 600, 8), ((2, 12), 300, 32), ((2, 12), 330, 50), ((2, 12), 200, 63)]


@functools.lru_cache(maxsize=None)
def window_inputs():
    out = []
    for form, T, k0 in WINDOW_CASES:
        ch = 8192 // (2 * (2 * k0) + 3)                                     # rows of the 8 KB window: these problems use the prefix band only, k = 2 k0
        out.append((form, T, ch, _indel_cases(random.Random(T + k0), T, k0, ch)))
    return out


def test_window_inputs_cross_the_staged_window(oracle):
    """The problems of test_staged_traceback_window take the forms with a staged walk, have more rows than a window holds, and the oracle's blocks show a run of
    64 and of 65 whose lowest row is the first row of a window (the walk's next arrow is in the window below)."""
    for form, T, ch, probs in window_inputs():
        assert all(f == form for f in forms_of_problems(probs)), (form, T)
        assert T > 2 * ch
        edges = {T - e * ch for e in range(1, T // ch + 1)}
        for run in (64, 65):
            assert any(any(int(b[2]) == run and int(b[1]) in edges for b in expected(oracle, *x, PAR)[1]) for x in probs), (form, T, run)


@pytest.mark.gpu
def test_staged_traceback_window(ctx, oracle):
    probs = [x for _, _, _, ps in window_inputs() for x in ps]
    st = check(ctx, oracle, probs)
    assert (st == 0).all()


# ---------------------------------------------------------------- g. status and score edges
# form name -> shapes whose walk leaves several blocks: the LDS sweep (classes 3, 7, 1), solve_reg (10, 11, 12), the lane kernel (15 .. 18), the staged walk (class 2, registers and rolling windows)
CAPACITY_SHAPES = {
    "lds sweep": [(8, 30, 3), (5, 40, 5), (30, 90, 9), (35, 44, 35)],
    "solve_reg": [(60, 58, 4), (150, 146, 9), (200, 195, 16)],
    "lane": [(6, 5, 3), (10, 9, 4), (16, 14, 7), (24, 23, 12)],
    "staged walk": [(300, 296, 31), (300, 303, 32)],
}
CAPACITY_CLASSES = {"lds sweep": {3, 7, 1}, "solve_reg": {10, 11, 12}, "lane": {15, 16, 17, 18}, "staged walk": {2}}


@functools.lru_cache(maxsize=None)
def capacity_inputs():
    out = {}
    for name, shapes in CAPACITY_SHAPES.items():
        rng = random.Random(name)
        out[name] = [make_pair(rng, s[0], s[1], "mut") + (s[2],) for s in shapes for _ in range(3)]
    return out


def test_capacity_inputs(oracle):
    for name, probs in capacity_inputs().items():
        assert {f[0] for f in forms_of_problems(probs)} == CAPACITY_CLASSES[name], name
        assert sum(len(expected(oracle, *x, PAR)[1]) >= 2 for x in probs) >= len(probs) // 2, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CAPACITY_SHAPES))
def test_capacity_status(ctx, oracle, name):
    """block_off gives some problems fewer block slots than their walk produces: LRA_ST_CAPACITY is set, nblocks is the full count, the other status bits,
    the score and the problems with room are as the oracle says, and the slots after the short problem's (they belong to a k0 = 0 problem, which writes none)
    keep their sentinel."""
    SENT = -777
    probs, caps, kinds = [], [], []
    for i, x in enumerate(capacity_inputs()[name]):
        full = len(expected(oracle, *x, PAR)[1])
        cap = [full - 1, 0, 1][i % 3] if full >= 2 else full
        probs += [x, (x[0], x[1], 0), x]
        caps += [cap, 4, full]
        kinds += ["short" if cap < full else "room", "guard", "room"]
    score, nb, st, blocks, boff = run_raw(ctx, probs, PAR, caps=caps, sentinel=SENT)
    assert kinds.count("short") >= 3
    for i, (x, kind) in enumerate(zip(probs, kinds)):
        if kind == "guard":
            assert st[i] == ST_RANGE and (blocks[boff[i]:boff[i + 1]] == SENT).all(), (name, i)
            continue
        es, eb, est = expected(oracle, *x, PAR)
        assert score[i] == es and nb[i] == len(eb), (name, i, score[i], es, nb[i], len(eb))
        if kind == "short":
            assert st[i] == (est | ST_CAPACITY), (name, i, st[i])
        else:
            assert st[i] == est and np.array_equal(blocks[boff[i]:boff[i + 1]], eb), (name, i)


# Scores below -2^29 are the device's MISS domain mapped back to the reference's INT_MIN arithmetic on output.  No problem the kernels take returns one: the
# corner of a prefix-only problem lies inside its (doubled) band and a path of indels reaches it, the corner of a long-gap problem takes the long gap from the
# prefix band's row / column maxima, of which [0] is 0.  So no form has such a case to run; this search (the oracle alone) is what says so.
def test_no_form_returns_a_miss_domain_score(oracle):
    rng = random.Random(77)
    lens = [0, 1, 2, 3, 5, 8, 13, 24, 25, 40, 70, 130]
    low = 0
    forms = set()
    for ql in lens:
        for tl in lens + [300]:
            for k0 in (1, 2, 7, 15, 31, 32, 64):
                for par in (PAR, (1, -1, -1)):
                    x = make_pair(rng, ql, tl, "unrel" if (ql + tl + k0) % 2 else "mut")
                    s, _, st = oracle.affine_one_gap_align(x[0], x[1], par[0], par[1], par[2], k0)
                    low = min(low, s)
                    forms.add(form_of((ql, tl, k0))[0])
    assert low > -(1 << 29), low
    assert forms >= {1, 2, 3, 5, 7, 8, 9, 10, 11, 12, 14, 15, 16, 17, 18}
