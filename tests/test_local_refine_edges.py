"""a13 LocalRefineAlignment / RefinedAlignmentbtwnAnchors at every threshold its walk branches on (local_refine.hip), both overloads, ONT and non-ONT options.

The cases come from local_refine_cases.py.  The CPU test proves from the oracle's trace that every case took the branch it was built for and that both sides of
every limit are present; the GPU tests compare each batch with the oracle bit for bit and read the kernel's LRA_DEBUG counts back: the pairs it sent to the direct
aligner, the large spaces, the spaces it searched on the other strand, the seed sets it extended and the alignment problems of its second batch must be the ones
the trace predicts, so a kernel that reaches the right answer by another road fails too.

Each of these one-line changes to local_refine.hip fails here (the case that catches it): min(rd, gd) > 300 and max(rd, gd) <= 500 (cls_300_*, cls_500_400 /
cls_400_500), curBlocks > 5 (rev_blocks_5), the two driftRate constants swapped (rev_drift), the ONT and non-ONT band formulas swapped (band_*, band_matters),
XL < 100 to <= 100 (inner_len_100), the LSC loop's > to >= (walk_tie_2_2), kept[0] == ne - 1 (every space with read-strand seeds)."""
import re

import numpy as np
import pytest

import local_refine_cases as LC

_EXP = {}


def expected(job, high, ont):
    """the oracle's (alignments or None, trace) of a job, computed once"""
    ont = LC.job_opts(job, ont)["isOnt"]
    k = (job["name"], int(high), int(ont))
    if k not in _EXP:
        _EXP[k] = LC.expected(job, high, ont)
    return _EXP[k]


def own_ont(job, ont):
    """a case that fixes isOnt runs only in the batch of that option set"""
    return LC.job_opts(job, ont)["isOnt"] == ont


# ------------------------------------------------------------------------------------------------------------------------------------------------ the cases
# limit -> what must differ between its sides (a trace field or a function of the record); the sides themselves are asserted by every case's own `expect`
DIFFER = {
    "min300/equal": "type", "min300/read": "type", "min300/genome": "type", "max500/read": "K", "max500/genome": "maxFreq", "cge_ngs": "type", "refineBySDP": "type",
    "ont100": "diag", "ont2000": "diag", "non80": "diag", "2sv/ont": "diag", "2sv/non": "diag",
    "side1000/inv": lambda r: r["idF"] == -1, "side1000/junk": lambda r: r["idR"] == -1, "side1000/mut": lambda r: r["idF"] == -1,
    "identity": "super", "blocks5": "tried", "event_at": "tried", "len100": "rm_max", "gap30": lambda r: r["inner_after"] < r["inner_before"],
    "dist500": lambda r: r["inner_after"] < r["inner_before"], "dist2blink": lambda r: r["inner_after"] < r["inner_before"],
    "dist1000": lambda r: r["inner_after"] < r["inner_before"], "overlap": "type",
}
SAME = {"ont100/product": ("diag", 100), "non80/product": ("diag", 80)}     # the product crosses the floor's argument, the band does not move (see band_cases)


def same_alignments(a, b):
    return len(a) == len(b) and all(all(x[f] == y[f] for f in ("strand", "supp", "secondary", "n0", "n1", "chrom")) and np.array_equal(x["blocks"], y["blocks"]) for x, y in zip(a, b))


def test_local_refine_cases_hold_what_they_are_for(oracle):
    cases = LC.all_cases()
    assert len(cases) > 140
    by_limit = {}; none_families = set(); n_none = 0; rows_all = []
    for j in cases:
        for ont in (0, 1):
            if not own_ont(j, ont): continue
            for high in (0, 1):
                res, rows = expected(j, high, ont)
                mir = LC.mirror_pairs(j, high, ont)
                # the second statement of the anchor-only arithmetic agrees with the trace, pair by pair (an undefined job stops early)
                assert len(rows) == len(mir) if res is not None else 0 < len(rows) <= len(mir), (j["name"], len(rows), len(mir))
                for r, m in zip(rows, mir):
                    for k, v in m.items():
                        assert int(r[k]) == v, (j["name"], ont, high, k, r[k], v)
                assert (res is None) == j["none_ok"], (j["name"], ont, high)
                plain = LC.expected(j, high, ont, trace=False)              # the untraced entry answers the same
                assert (plain is None) == (res is None) and (res is None or (same_alignments(plain, res) and [a["value"] for a in plain] == [a["value"] for a in res])), j["name"]
                if res is None:
                    n_none += 1; none_families.add(j["family"])
                if j["expect"]:
                    r = LC.probe(j, rows)
                    for k, v in j["expect"].items():
                        assert r[k] == v, (j["name"], ont, high, k, r[k], v)
                if high == 0:
                    rows_all += [r for r in rows if r["type"] == 2]
                    if j["tag"] and j["expect"]:
                        by_limit.setdefault(j["tag"][0], {}).setdefault(j["tag"][1], []).append(LC.probe(j, rows))
    # only the two overlap-by-two-or-more families are undefined: 2 families x 2 strands x 2 option sets x 2 overloads
    assert none_families == {"overlap_small", "overlap_big"} and n_none == 16
    # every limit has both sides, and they differ in the field they are meant to differ in
    for lim, what in DIFFER.items():
        sides = by_limit.get(lim, {})
        assert len(sides) >= 2, (lim, sorted(sides))
        f = what if callable(what) else (lambda r, k=what: r[k])
        vals = {s: {f(r) for r in rs} for s, rs in sides.items()}
        assert all(len(v) == 1 for v in vals.values()), (lim, vals)
        assert len({next(iter(v)) for v in vals.values()}) >= 2, (lim, vals)
    for lim, (k, v) in SAME.items():
        sides = by_limit[lim]
        assert len(sides) == 2 and all(r[k] == v for rs in sides.values() for r in rs), lim
    assert set(by_limit["abut"]) == {"read", "genome", "both"}
    name = {j["name"]: j for j in cases}
    for s in "+-":
        # the band matters: the same input under the two option sets keeps / loses the seeds 90 off the diagonal, and the alignments differ
        j = name["band_matters" + s]
        (a1, t1), (a0, t0) = expected(j, 0, 1), expected(j, 0, 0)
        r1, r0 = LC.probe(j, t1), LC.probe(j, t0)
        assert r1["diag"] >= 100 > 90 > r0["diag"] == 80 and r1["nf"] > r0["nf"] + 100 and not same_alignments(a1, a0)
        # 4 | 5 blocks: the same space, not tried | tried, and the alignments differ
        a4, a5 = expected(name["rev_blocks_4" + s], 0, 1)[0], expected(name["rev_blocks_5" + s], 0, 1)[0]
        assert len(a4) == 1 and len(a5) == 3 and a5[1]["strand"] != a5[0]["strand"]
        # a second event 3 | 6 blocks after a first: the fresh alignment starts at 0 blocks
        for n, tried in ((3, 0), (6, 1)):
            j = name["rev_second_%d%s" % (n, s)]
            al, tr = expected(j, 0, 1)
            r = LC.probe(j, tr, 1)
            assert (r["super"], r["blocks"], r["tried"]) == (1, n, tried) and len(al) == (5 if tried else 3), (j["name"], r)
        # the drift clause: ONT breaks, the others align the whole space (nf >= nr with both 0)
        j = name["rev_drift" + s]
        (ab, tb), (aw, tw) = expected(j, 0, 1), expected(j, 0, 0)
        assert LC.probe(j, tb)["outcome"] == 0 and LC.probe(j, tw)["outcome"] == 3 and LC.probe(j, tw)["idR"] >= 0.8 and len(ab) == 2 and len(aw) == 1
        # LSC: the first largest chain wins a tie, an empty chain never wins; the high-accuracy caller may name a smaller one; one anchor is an alignment there
        assert [a["supp"] for a in expected(name["walk_tie_2_2" + s], 0, 1)[0]] == [0, 1]
        assert [a["supp"] for a in expected(name["walk_tie_1_3_3" + s], 0, 1)[0]] == [0, 1] and expected(name["walk_tie_1_3_3" + s], 0, 1)[0][0]["secondary"] == 1
        assert [a["supp"] for a in expected(name["walk_0_2_1" + s], 0, 1)[0]] == [0]
        assert [a["supp"] for a in expected(name["walk_lsc_small" + s], 1, 1)[0]] == [1, 0, 1] and [a["supp"] for a in expected(name["walk_lsc_small" + s], 0, 1)[0]] == [0, 1]
        hi = expected(name["walk_lsc_one" + s], 1, 1)[0]
        assert len(hi) == 2 and len(hi[1]["blocks"]) == 1 and hi[1]["supp"] == 0 and hi[1]["n1"] == 0 and len(expected(name["walk_lsc_one" + s], 0, 1)[0]) == 1
        assert expected(name["walk_only_1" + s], 0, 1)[0] == [] and len(expected(name["walk_only_1" + s], 1, 1)[0]) == 1
    # lr_decide's outcomes, the inner chain's ends and the final piece: every value is reached somewhere
    tried = [r for r in rows_all if r["tried"] == 1]
    assert {r["outcome"] for r in tried} == {0, 2, 3} and any(r["nr"] > r["nf"] for r in tried) and any(r["nr"] == 0 == r["nf"] and r["outcome"] == 3 for r in tried)
    inner = [r for r in rows_all if r["inner_after"] > 0]
    assert {r["btc_start"] for r in inner} == {0, 1} and {r["final"] for r in inner} == {0, 1}
    assert {int(r["inner_after"] - 1 - r["btc_end"]) for r in inner} == {0, 1}
    assert any(r["super"] == 1 and r["tried"] == 0 and r["spec"] == 2 for r in rows_all)      # the device plans an inverted seed set the walk never uses


# ------------------------------------------------------------------------------------------------------------------------------------------------ on the device
DBG = {k: re.compile(p) for k, p in dict(nDir=r"classified: NA \d+ nDir (\d+)", nBig=r"classified: NA \d+ nDir \d+ nBig (\d+)", nRev=r"spaces done: nF \d+ nRev (\d+)",
                                         nJ=r"spaces done: nF \d+ nRev \d+ nR \d+ nJ (\d+)", nP2=r"second AOG done: nP2 (\d+)").items()}


def run_batch(ctx, jobs, high, ont, monkeypatch=None, capfd=None):
    """one call of the overload on the jobs in the order given -> (result struct, fetched arrays, the kernel's debug counts or None)"""
    import torch
    from lra_amd import chain, seed
    opts = {}
    for j in jobs:
        o = LC.job_opts(j, ont)
        assert not opts or o == opts, "one option set per call"
        opts = o
    batch = seed.ReadBatch(ctx, [j["read"].tobytes() for j in jobs])
    dev = ctx.device
    tot = int(batch.off[-1])
    both = torch.zeros(2 * tot + 64, dtype=torch.uint8, device=dev)
    both[:tot] = batch.seq[:tot]; both[tot:2 * tot] = seed.create_rc(ctx, batch)[:tot]
    gdev = torch.from_numpy(np.concatenate([LC.genome(), np.zeros(64, np.uint8)])).to(dev)
    jco = [0]; cao = [0]; cs = []; cc = []; cv = []; c0 = []; c1 = []; Q = []; T = []; Ln = []
    for j in jobs:
        base = len(Q)
        Q += j["aq"].tolist(); T += j["at"].tolist(); Ln += j["al"].tolist()
        cao += [base + int(x) for x in j["off"][1:]]
        cs += j["strand"]; cc += j["chrom"]; cv += j["value"]; c0 += j["n0"]; c1 += j["n1"]
        jco.append(len(cs))
    tt = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    args = (tt(cao, np.int64), tt(cs, np.int32), tt(cc, np.int32), tt(cv, np.float32), tt(c0, np.int32), tt(c1, np.int32), tt(Q, np.int64).to(torch.int32),
            tt(T, np.int64).to(torch.int32), tt(Ln, np.int32), batch.off, both, tot, gdev, LC.CH)
    head = (tt(jco, np.int64), tt(np.arange(len(jobs)), np.int32), tt([j["h"] for j in jobs], np.int32))
    if monkeypatch is not None:
        monkeypatch.setenv("LRA_DEBUG", "1")
        capfd.readouterr()
    if high:
        res = chain.local_refine_highacc_batch(ctx, *head, tt([LC.job_lsc(j, True) for j in jobs], np.int32), *args, **opts)
    else:
        res = chain.local_refine_batch(ctx, *head, *args, **opts)
    dbg = None
    if monkeypatch is not None:
        err = capfd.readouterr().err
        monkeypatch.delenv("LRA_DEBUG")
        dbg = {}
        for k, rx in DBG.items():
            m = rx.findall(err)
            assert len(m) == 1, (k, err[-2000:])
            dbg[k] = int(m[0])
    return res, chain.fetch_alignments(ctx, res), dbg


def job_result(out, ji):
    """a job's alignments as the oracle lists them (value as float bits)"""
    a0, a1 = int(out["job_aln_off"][ji]), int(out["job_aln_off"][ji + 1])
    r = []
    for x in range(a0, a1):
        b0, b1 = int(out["block_off"][x]), int(out["block_off"][x + 1])
        r.append(dict({f: int(out[f][x]) for f in ("strand", "supp", "secondary", "n0", "n1", "chrom")}, value=int(np.float32(out["value"][x]).view(np.uint32)),
                      blocks=out["blocks"][b0:b1].copy()))
    return r


def check_jobs(jobs, out, high, ont):
    for ji, j in enumerate(jobs):
        exp, _ = expected(j, high, ont)
        if exp is None:
            assert out["status"][ji] != 0, j["name"]
            continue
        assert out["status"][ji] == 0, (j["name"], out["status"][ji])
        got = job_result(out, ji)
        assert len(got) == len(exp), (j["name"], len(got), len(exp))
        for k, (g, e) in enumerate(zip(got, exp)):
            for f in ("strand", "supp", "secondary", "n0", "n1", "chrom"):
                assert g[f] == e[f], (j["name"], k, f, g[f], e[f])
            assert g["value"] == int(np.float32(e["value"]).view(np.uint32)), (j["name"], k)
            assert len(g["blocks"]) == len(e["blocks"]) and np.array_equal(g["blocks"], e["blocks"]), (j["name"], k, len(g["blocks"]), len(e["blocks"]))


def check_counts(jobs, res, dbg, high, ont):
    """the kernel went the way the trace says: direct pairs, large spaces, spaces searched on the other strand (the ratio and identity clauses, whatever the block
    count), seed sets extended, problems of the second alignment batch"""
    rows = [r for j in jobs for r in expected(j, high, ont)[1]]
    big = [r for r in rows if r["type"] == 2]
    want = dict(nDir=sum(r["type"] == 1 for r in rows), nBig=len(big), nRev=sum(int(r["super"]) for r in big), nJ=sum(int(r["jobs"]) for r in big),
                nP2=sum(int(r["np2"]) for r in big))
    assert dbg == want, (dbg, want)
    assert (int(res.n_big), int(res.n_inner_jobs)) == (want["nBig"], want["nJ"])


GROUPS = {"classify": ("classify", "overlap1"), "band": ("band", "band_matters"), "reverse": ("reverse", "blocks", "decide", "events"), "inner": ("inner",), "walk": ("walk",)}


@pytest.mark.gpu
@pytest.mark.parametrize("ont", [1, 0])
@pytest.mark.parametrize("high", [0, 1])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_family_against_oracle(ctx, oracle, monkeypatch, capfd, group, high, ont):
    """one batch per family group, overload and option set: every job bit for bit, and the kernel's own counts of the roads it took"""
    jobs = [j for j in LC.family(*GROUPS[group]) if own_ont(j, ont)]
    assert 8 <= len(jobs) <= 80
    parts = {}
    for j in jobs:                                                          # (the RefineBySDP-off cases are a call of their own)
        parts.setdefault(tuple(sorted(LC.job_opts(j, ont).items())), []).append(j)
    for part in parts.values():
        res, out, dbg = run_batch(ctx, part, high, ont, monkeypatch, capfd)
        check_jobs(part, out, high, ont)
        check_counts(part, res, dbg, high, ont)


@pytest.mark.gpu
@pytest.mark.parametrize("high", [0, 1])
@pytest.mark.parametrize("fam", ["overlap_small", "overlap_big"])
def test_overlapping_anchors_are_flagged(ctx, oracle, fam, high):
    """anchors that overlap on the read by two or more bases: undefined in the reference, so the job must carry a status; jobs beside them are untouched"""
    for ont in (1, 0):
        jobs = LC.family(fam) + LC.family("overlap1") + LC.family("walk")[:4]
        res, out, _ = run_batch(ctx, jobs, high, ont)
        assert sum(expected(j, high, ont)[0] is None for j in jobs) == 2
        check_jobs(jobs, out, high, ont)
        assert all(out["status"][i] == 4 for i, j in enumerate(jobs) if j["none_ok"])          # LRA_ST_RANGE


@pytest.mark.gpu
@pytest.mark.parametrize("high", [0, 1])
def test_mixed_batch_in_two_orders(ctx, oracle, monkeypatch, capfd, high):
    """all families in one batch (every second case, so that the batch stays small), shuffled; a second order gives the same per-job results"""
    ont = 1
    pool = [j for j in LC.all_cases() if own_ont(j, ont) and not j["none_ok"] and not j["opts"].get("refineBySDP", 1) == 0 and len(j["read"]) < 10000]
    fams = {j["family"] for j in pool}
    rng = np.random.default_rng(7)
    jobs = [pool[i] for i in rng.permutation(len(pool)) if i % 2 == high]
    assert {j["family"] for j in jobs} == fams and 40 <= len(jobs) <= 80
    res, out, dbg = run_batch(ctx, jobs, high, ont, monkeypatch, capfd)
    check_jobs(jobs, out, high, ont)
    check_counts(jobs, res, dbg, high, ont)
    order = rng.permutation(len(jobs))
    res2, out2, _ = run_batch(ctx, [jobs[i] for i in order], high, ont)
    for k, i in enumerate(order):
        a, b = job_result(out, int(i)), job_result(out2, k)
        assert out2["status"][k] == 0 and len(a) == len(b), jobs[i]["name"]
        for x, y in zip(a, b):
            assert all(x[f] == y[f] for f in ("strand", "supp", "secondary", "n0", "n1", "chrom", "value")) and np.array_equal(x["blocks"], y["blocks"]), jobs[i]["name"]
