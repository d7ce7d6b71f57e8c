"""lra_refine_btwn_splitchain_batch (refine_btwn.hip) on the crafted chains of tests/btwn_cases.py: every threshold pair of the walk, the order in which a chain's gaps
read each other's boxes, and the layouts (chains of 0 to 6 clusters in one batch, any slot order, padding fragments, several chains on a read, marked slots, 257
slots, a pair pool that grows between rounds, segments of 63 / 64 / 65 matches).  All cases that share (refineSpaceDist, anchorstoosparse) go into one call; every
cluster's matches in order, its box and its refinespace flag, the match offsets of the padding fragments and the number of rounds are compared with the oracle
exactly.  tests/test_btwn_cases.py checks on the CPU that the cases are what their names say."""
import numpy as np
import pytest

import btwn_cases as bc

BTWN = [(n, c) for n, c in bc.all_cases() if c["kind"] == "btwn"]
GROUPS = {}
for _n, _c in BTWN: GROUPS.setdefault(bc.opts_key(_c), []).append((_n, _c))
KEYS = sorted(GROUPS)
_EXPECTED = {}


def expected(name, case):
    """the oracle's output for a case, computed once"""
    if name not in _EXPECTED:
        _EXPECTED[name] = bc.oracle_btwn(case)
        assert _EXPECTED[name] is not None, name
    return _EXPECTED[name]


def run_batch(ctx, named, key, **layout):
    """one call on the packed chains -> {name: (off, q, t, box, refinespace)} per chain, after checking the batch-wide arrays"""
    from lra_amd import chain
    P = bc.pack(named, **layout)
    dev, ch, sp, rf = bc.to_device(ctx, P)
    bres = chain.refine_btwn_splitchain_batch(ctx, ch, sp, rf, dev["read_off"], dev["strands"], P["rc_base"], dev["genome"], bc.CHROM, K=bc.K, W=bc.W,
                                              refineSpaceDist=key[0], anchorstoosparse=key[1], match=4, mismatch=-1, indel=-2, max_freq=15)
    bo = chain.fetch_btwn(ctx, bres)
    # match_off over ALL fragments: a chain's clusters hold what the oracle says, a padding fragment keeps the matches it came with
    cnt = np.diff(P["match_off"].astype(np.int64))
    for n, c in named:
        e = expected(n, c)
        b = P["where"][n][1]
        cnt[b:b + len(c["clusters"])] = np.diff(e["off"])
    assert bres.n_frags == P["n_frags"] and bres.n_matches == int(cnt.sum())
    assert np.array_equal(bo["match_off"].astype(np.int64), np.concatenate([[0], np.cumsum(cnt)])), "match_off (padding fragments included)"
    longest = max(len(c["clusters"]) for _, c in named)
    assert bres.n_rounds == (longest - 1 + 2 if longest else 2), (bres.n_rounds, longest)      # one round per gap index, two end rounds
    out = {}
    for n, c in named:
        b = P["where"][n][1]; k = len(c["clusters"])
        m0, m1 = int(bo["match_off"][b]), int(bo["match_off"][b + k])
        out[n] = (bo["match_off"][b:b + k + 1].astype(np.int64) - m0, bo["match_q"][m0:m1], bo["match_t"][m0:m1], bo["box"][b:b + k], bo["refinespace"][b:b + k])
    return out


def check(named, out):
    for n, c in named:
        e = expected(n, c)
        off, q, t, box, rs = out[n]
        assert np.array_equal(off, e["off"]), (n, "matches per cluster", np.diff(off).tolist(), np.diff(e["off"]).tolist())
        assert np.array_equal(q, e["q"]) and np.array_equal(t, e["t"]), (n, "matches")
        assert np.array_equal(box, e["box"]), (n, "box", box.tolist(), e["box"].tolist())
        assert np.array_equal(rs, e["refinespace"]), (n, "refinespace", rs.tolist(), e["refinespace"].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS, ids=["rsd=%d,sparse=%.9g" % k for k in KEYS])
def test_hip_refine_btwn_edges(ctx, oracle, key):
    """every case registered under one option set, in one batch with padding fragments, marked slots and several chains per read"""
    named = GROUPS[key]
    check(named, run_batch(ctx, named, key))


MIX = ["layout.nsp=0", "order.nsp1.both_ends/s0/a", "gap.same0.cur.tEnd<=prev.tStart/s0/a", "order.gap2.ts1_moves/a", "layout.nsp=6", "order.nsp1.both_ends/s1/a",
       "gap.diff1.p2_appends/below/st1=0/a", "order.gap2.te1_moves/a", "layout.nsp=6.s1", "order.unread_sides.with", "gap.same1.link/s1/p1/a"]


@pytest.mark.gpu
def test_hip_refine_btwn_mixed_lengths_any_order(ctx, oracle):
    """chains of 0, 1, 2, 3 and 6 clusters in one batch: seven rounds, the short chains untouched by the rounds beyond their length; the same chains in reversed slot
    order and without padding fragments give the same per-chain result"""
    cases = dict(BTWN)
    named = [(n, cases[n]) for n in MIX]
    assert sorted({len(c["clusters"]) for _, c in named}) == [0, 1, 2, 3, 6] and len({bc.opts_key(c) for _, c in named}) == 1
    key = bc.opts_key(named[0][1])
    a = run_batch(ctx, named, key)
    check(named, a)
    for layout in (dict(pad=False, marked=False), dict(pad=True, marked=False, empty_slots=3)):
        b = run_batch(ctx, named[::-1], key, **layout)
        check(named, b)
        for n, _ in named:
            assert all(np.array_equal(x, y) for x, y in zip(a[n], b[n])), n


@pytest.mark.gpu
def test_hip_refine_btwn_pool_grows_between_rounds(ctx, oracle):
    """a first round of a few pairs, a later round of several thousand: the pair pool and the segment table grow while they hold the earlier rounds' data.  The
    same batch again on the same context, its buffers now large enough, gives the same output"""
    cases = dict(BTWN)
    names = ["res.run>=4/s0/b", "pool.few_then_thousands", "gap.same0.cur.tEnd<=prev.tStart/s0/a", "order.gap2.ts1_moves/a"]
    named = [(n, dict(cases[n], opts=dict(bc.OPTS))) for n in names]
    named[0] = ("res.run>=4/s0/b@0.01", named[0][1])                                        # (registered under another anchorstoosparse)
    key = bc.opts_key(named[1][1])
    e = expected(*named[1])
    assert int(e["off"][3] - e["off"][2]) > 2000 and 4 <= int(e["off"][2] - e["off"][1]) - 2 < 20     # round 1: six pairs; round 2: thousands
    ctx.release_buffers()                                                                   # start from empty work buffers: the pool has to grow
    first = run_batch(ctx, named, key)
    check(named, first)
    again = run_batch(ctx, named, key)
    check(named, again)
    for n, _ in named:
        assert all(np.array_equal(x, y) for x, y in zip(first[n], again[n])), n


@pytest.mark.gpu
def test_hip_refine_btwn_257_slots(ctx, oracle):
    """one slot more than a block of the plan / apply kernels, all but the last five without a chain"""
    cases = dict(BTWN)
    names = ["gap.same0.cur.tEnd<=prev.tStart/s0/a", "order.nsp1.both_ends/s1/a", "order.gap2.arm_flips_to_skip/a", "gap.diff1.p1_appends/above/st1=1/a", "res.empty/s1/a"]
    named = [(n, cases[n]) for n in names]
    key = bc.opts_key(named[0][1])
    assert all(bc.opts_key(c) == key for _, c in named)
    P = bc.pack(named, num_aln=1, empty_slots=252)
    assert P["n_slots"] == 257 and P["where"][names[-1]][0] == 256
    check(named, run_batch(ctx, named, key, num_aln=1, empty_slots=252))
