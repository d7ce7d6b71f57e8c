"""split_kernel (lra_split_chains_batch) and hsplit_kernel (lra_split_chains_highacc_batch) at every threshold they branch on, on the crafted chains of
tests/chain_cases.py.  CPU: the oracle tells the two sides of every threshold pair apart, and for named anchor cases its pieces equal literals worked out by hand
from the reference's text -- low accuracy: RemoveSpuriousJump Chain.h:897-957, SPLITChain Mapping_ultility.h:385-441 (the N cut :400, the T cut :406), push_new
:349-383, SplitChain::CHROMIndex Chain.h:386-394 (:388 TStart + 1, :390 TEnd) over GenomeHeader::Find Genome.h:20-32, diag Chain.h:243-246, MergeSplitchainINS
Mapping_ultility.h:172-262 (:193 tdist > 1500), RemoveSpuriousSplitChain Map_lowacc.h:38-66 (:47, :50); high accuracy: SPLITChain Mapping_ultility.h:266-346 (:278 the
repeat test, :282-283 the T cut), OverlaprateOnGenome Clustering.h:397-406, LargestSplitChain_dist Chain.h:974-985.  GPU: every output array against the oracle."""
import numpy as np
import pytest

import chain_cases as cc
import oracle_lib as O

SPLIT_PAIRS = {n: p for n, p in cc.PAIRS.items() if p[0]["kind"] == "split"}
HSPLIT_PAIRS = {n: p for n, p in cc.PAIRS.items() if p[0]["kind"] == "hsplit"}
SPLIT_CASES = [(n, c) for n, c in cc.all_cases() if c["kind"] == "split"]
HSPLIT_CASES = [(n, c) for n, c in cc.all_cases() if c["kind"] == "hsplit"]
R = lambda a, b: list(range(a, b))
D = lambda a, b: list(range(b - 1, a - 1, -1))       # a forward piece lists its anchors last to first (:436-441)

# name of a pair -> per side ([(type, indices into the filtered chain)], split_link), None where the reference reads outside the chromosome table
PIECES = {
    # the N cut (:400): eight anchors, the step 3 -> 4 with dist = min(qdist, tdist) and the diagonal difference as named
    "split.N.dist>=1000.q/s0": (([("N", D(0, 4)), ("N", D(4, 8))], [0]), ([("N", D(0, 8))], [])),
    "split.N.dist>=1000.t/s1": (([("N", R(0, 4)), ("N", R(4, 8))], [0]), ([("N", R(0, 8))], [])),
    "split.N.ceil/s0": (([("N", D(0, 4)), ("N", D(4, 8))], [0]), ([("N", D(0, 8))], [])),          # dist 1001: ceil(150.15) = 151 against 152
    "split.N.ceil.len/s1": (([("N", R(0, 4)), ("N", R(4, 8))], [0]), ([("N", R(0, 8))], [])),      # anchor 4 twice as long: diag is qEnd + t
    # the T cut (:406), splitdist 50000: a target distance of exactly splitdist is no cut
    "split.T.up/s1": (([("N", R(0, 8))], []), ([("T", R(0, 4)), ("N", R(4, 8))], [0])),
    "split.T.down/s0": (([("N", D(0, 8))], []), ([("T", D(0, 4)), ("N", D(4, 8))], [0])),
    "split.T.up/s0": (([("N", D(0, 8))], []), ([("T", D(0, 4)), ("N", D(4, 8))], [0])),
    # the I cut (:411-): ten anchors, the strand changes at 5
    "split.I/s0": (([("I", D(0, 5)), ("N", R(5, 10))], [1]), ([("N", D(0, 10))], [])),
    # CHROMIndex: a run across pos[1] is pushed nowhere; TStart + 1 == pos[1] is chromosome 1; TEnd == pos[last] is found (and differs from TStart's), one more is not
    "split.chrom.spans_boundary": (([], []), ([("N", D(0, 6))], [])),
    "split.chrom.TStart+1==pos": (([("N", D(0, 6))], []), ([], [])),
    "split.chrom.TEnd==pos[last]": (([], []), ([("N", D(0, 6))], [])),
    "split.chrom.TEnd==pos[last]+1": (None, ([], [])),
    # MergeSplitchainINS: A (0..3) | X (4..6) | A' (7..10) | B (11..13); A' joins A at 1500, takes A's slot and hands it its own type
    "split.merge.tdist<=1500/s0/by1": (([("T", D(7, 11) + D(0, 4)), ("T", D(4, 7)), ("N", D(11, 14))], [0, 0]),
                                       ([("T", D(0, 4)), ("T", D(4, 7)), ("T", D(7, 11)), ("N", D(11, 14))], [0, 0, 0])),
    "split.merge.tdist<=1500/s1/by0": (([("T", R(0, 4) + R(7, 11)), ("T", R(4, 7)), ("N", R(11, 14))], [0, 0]),
                                       ([("T", R(0, 4)), ("T", R(4, 7)), ("T", R(7, 11)), ("N", R(11, 14))], [0, 0, 0])),
    # A' 1000 below A: with A's TStart at 3000500 it lies on chromosome 0 and A on 1 -- no merge; with both on chromosome 1 they merge
    "split.merge.other_chrom/by1": (([("T", D(0, 4)), ("T", D(4, 7)), ("T", D(7, 11)), ("N", D(11, 14))], [0, 0, 0]),
                                    ([("T", D(7, 11) + D(0, 4)), ("T", D(4, 7)), ("N", D(11, 14))], [0, 0])),
    # A X A' Y A'' B: A'' is within 1500 of the merged A + A' only (2600 below A, A' reaches 1140 below); at 2700 it stays alone
    "split.merge.chained/by1": (([("T", D(14, 18) + D(7, 11) + D(0, 4)), ("T", D(4, 7)), ("T", D(11, 14)), ("N", D(18, 21))], [0, 0, 0]),
                                ([("T", D(7, 11) + D(0, 4)), ("T", D(4, 7)), ("T", D(11, 14)), ("T", D(14, 18)), ("N", D(18, 21))], [0, 0, 0, 0])),
    # RemoveSpuriousSplitChain: 40 anchors, an inverted piece of m, the rest; behind an I link a piece needs min(max(floor(0.03 total), 2), 4) anchors
    "split.rss.total99|100/s0": (([("I", D(0, 40)), ("I", R(40, 42)), ("N", D(42, 99))], [1, 1]), ([("I", D(0, 40)), ("N", D(42, 100))], [1])),
    "split.rss.total133|134/s0": (([("I", D(0, 40)), ("I", R(40, 43)), ("N", D(43, 133))], [1, 1]), ([("I", D(0, 40)), ("N", D(43, 134))], [1])),
    "split.rss.size1|2/s0": (([("T", D(0, 40)), ("N", D(41, 60))], [0]), ([("T", D(0, 40)), ("T", D(40, 42)), ("N", D(42, 60))], [0, 0])),
    "split.rss.piece0_goes/s0": (([("T", D(1, 6)), ("N", D(6, 60))], [0]), ([("T", D(0, 2)), ("T", D(2, 7)), ("N", D(7, 60))], [0, 0])),
    # piece 1 (one anchor behind a T link) goes, piece 2 sits behind an I link: slot 0 of split_link keeps its own 0 (`c > 1`, :59-63)
    "split.rss.piece1_goes.T_then_I/s0": (([("T", D(0, 10)), ("N", R(11, 40))], [0]), ([("T", D(0, 10)), ("I", D(10, 12)), ("N", R(12, 40))], [0, 1])),
}
# name of a pair -> per side ([(type, elements)], lsc)
HPIECES = {
    "hsplit.T.up/s0": (([("N", [0, 1])], 0), ([("T", [0]), ("N", [1])], 0)),
    "hsplit.T.down/s1": (([("N", [0, 1])], 0), ([("T", [0]), ("N", [1])], 0)),
    "hsplit.T.chrom": (([("N", [0, 1])], 0), ([("T", [0]), ("N", [1])], 0)),
    "hsplit.D.ovl600|599/s0": (([("D", [0]), ("N", [1])], 0), ([("N", [0, 1])], 0)),        # 600 / 1000 in float is above 0.6; 599 / 1000 is not
    "hsplit.D.prev_only/s1": (([("D", [0]), ("N", [1])], 0), ([("N", [0, 1])], 0)),
    "hsplit.D.cur_only/s0": (([("D", [0]), ("N", [1])], 0), ([("N", [0, 1])], 0)),
    "hsplit.D.link/s0": (([("D", [0]), ("N", [1])], 0), ([("N", [0, 1])], 0)),
    "hsplit.D.link/s1": (([("D", [0]), ("N", [1])], 0), ([("N", [0, 1])], 0)),
    "hsplit.D_before_T/s0": (([("D", [0]), ("N", [1])], 0), ([("T", [0]), ("N", [1])], 0)),
    "hsplit.I": (([("I", [0]), ("N", [1])], 0), ([("N", [0, 1])], 0)),
    "hsplit.merge.tdist<=1500/s0": (([("T", [0, 2]), ("T", [1]), ("N", [3])], 0), ([("T", [0]), ("T", [1]), ("T", [2]), ("N", [3])], 0)),
    "hsplit.merge.never_last": (([("T", [0, 2]), ("T", [1]), ("N", [3])], 0), ([("T", [0]), ("T", [1]), ("N", [2])], 0)),
    "hsplit.lsc.equal_widest": (([("T", [0]), ("T", [1]), ("T", [2]), ("N", [3])], 1), ([("T", [0]), ("T", [1]), ("T", [2]), ("N", [3])], 2)),
    "hsplit.lsc.qe<=qs": (([("T", [0]), ("T", [1]), ("N", [2])], 0), ([("T", [0]), ("T", [1]), ("N", [2])], 1)),
}


def _split_oracle(c):
    ch = c["chain"]
    return O.split_chain(ch["q"], ch["t"], ch["len"], ch["strand"], ch["cluster"], ch["link"], list(c["chrom"]), c["splitdist"], c["bypass"])


def _hsplit_oracle(c):
    return O.split_chain_highacc(c["strand"], c["chrom"], np.array(c["box"], np.uint32).reshape(-1, 4), c["link"], c["splitdist"])


def test_split_pairs_differ(oracle):
    assert len(SPLIT_PAIRS) >= 60 and len(HSPLIT_PAIRS) >= 25
    same = [n for n, (a, b) in list(SPLIT_PAIRS.items()) + list(HSPLIT_PAIRS.items()) if cc.decision(a) == cc.decision(b)]
    assert not same, same


def test_split_out_of_table_is_none(oracle):
    """TEnd one past pos[last]: GenomeHeader::Find runs off the table, the oracle returns None (and the kernel must flag the slot)"""
    assert cc.OOB
    for name in cc.OOB:
        assert cc.run(dict(cc.all_cases())[name]) is None, name


def test_split_literals(oracle):
    for name, sides in PIECES.items():
        for case, want in zip(SPLIT_PAIRS[name], sides):
            r = _split_oracle(case)
            if want is None:
                assert r is None, name
                continue
            got = ([(s["type"], s["idx"].tolist()) for s in r["splits"]], r["split_link"].tolist())
            assert got == want, (name, got, want)
            assert r["n_kept"] == len(case["chain"]["q"])
    # the merged piece: 0 links across the junction, ClusterIndex of A alone without bypassClustering, of both with it (:226-236), the box over both
    a1 = _split_oracle(SPLIT_PAIRS["split.merge.tdist<=1500/s0/by1"][0])["splits"][0]
    a0 = _split_oracle(SPLIT_PAIRS["split.merge.tdist<=1500/s0/by0"][0])["splits"][0]
    assert a1["clusters"].tolist() == [0, 2] and a0["clusters"].tolist() == [0] and a1["idx"].tolist() == a0["idx"].tolist()
    ch = SPLIT_PAIRS["split.merge.tdist<=1500/s0/by1"][0]["chain"]
    assert a1["box"].tolist() == [int(ch["q"][10]), int(ch["q"][0]) + 20, int(ch["t"][10]), int(ch["t"][0]) + 20] and int(ch["t"][3]) - int(ch["t"][7]) - 20 == 1500
    lk = np.concatenate([ch["link"][0:3], [0], ch["link"][7:10]])[::-1]      # A's links, 0 at the junction (:205), A''s; reversed with the piece
    assert a1["link"].tolist() == lk.tolist()
    # split_link after a merge: kept entries without bypassClustering, rewritten from the pieces' types with it (:255-259)
    b0, b1 = (_split_oracle(c) for c in SPLIT_PAIRS["split.merge.bypass.split_link"])
    assert b0["split_link"].tolist() == [0, 1] and b1["split_link"].tolist() == [1, 0]
    assert [s["type"] for s in b0["splits"]] == ["T", "I", "N"] == [s["type"] for s in b1["splits"]]
    # the jump filter in front (keep[])
    for z in ("s0", "s1"):
        for nm in ("split.jump.gap>100/", "split.jump.dist==1/", "split.jump.len<50/"):
            a, b = (_split_oracle(c) for c in SPLIT_PAIRS[nm + z])
            assert a["keep"].tolist() == [1, 1, 1, 0, 1, 1, 1, 1, 1] and b["keep"].tolist() == [1] * 9, nm + z


def test_hsplit_literals(oracle):
    for name, sides in HPIECES.items():
        for case, want in zip(HSPLIT_PAIRS[name], sides):
            r = _hsplit_oracle(case)
            got = ([(chr(int(r["type"][k])), r["idx"][r["off"][k]:r["off"][k + 1]].tolist()) for k in range(len(r["type"]))], r["lsc"])
            assert got == want, (name, got, want)
    r = _hsplit_oracle(cc.SINGLES["hsplit.n=0"])
    assert len(r["type"]) == 0 and r["lsc"] == 0


def _check_split(out, s, b, case):
    exp = _split_oracle(case)
    if exp is None:
        assert out["status"][s] != 0, s
        return 1
    assert out["status"][s] == 0, s
    n = len(case["chain"]["q"])
    assert out["keep"][b:b + n].tolist() == exp["keep"].tolist(), s
    assert out["n_kept"][s] == exp["n_kept"], s
    assert out["link"][b:b + max(exp["n_kept"] - 1, 0)].tolist() == exp["link"].tolist(), s
    assert out["n_split"][s] == len(exp["splits"]), (s, out["n_split"][s], len(exp["splits"]))
    for k, e in enumerate(exp["splits"]):
        x = b + k
        a0, m = b + int(out["sp_beg"][x]), int(out["sp_len"][x])
        assert out["sp_idx"][a0:a0 + m].tolist() == e["idx"].tolist(), (s, k)
        assert out["sp_link"][a0:a0 + m - 1].tolist() == e["link"].tolist(), (s, k)
        assert chr(out["sp_type"][x]) == e["type"] and out["sp_strand"][x] == e["strand"] and out["sp_chrom"][x] == e["chrom"], (s, k)
        assert out["sp_box"][x].tolist() == e["box"].tolist(), (s, k)
        c0, cm = b + int(out["ci_beg"][x]), int(out["ci_len"][x])
        assert out["ci_idx"][c0:c0 + cm].tolist() == e["clusters"].tolist(), (s, k)
    assert out["n_split_link"][s] == len(exp["split_link"]), s
    assert out["split_link"][b:b + len(exp["split_link"])].tolist() == exp["split_link"].tolist(), s
    return 0


def _run_split(ctx, slots, num_aln, n_chains, chrom, splitdist, bypass):
    """slots: one case or None (a slot of length 0) per chain slot, num_aln slots per read; n_chains[r] slots of read r are live.  Returns the flagged slots."""
    import torch
    from lra_amd import chain
    assert len(slots) % num_aln == 0 and len(n_chains) == len(slots) // num_aln
    empty = cc.make_chain([])
    chains = [empty if c is None else c["chain"] for c in slots]
    start = np.cumsum([0] + [len(c["q"]) for c in chains]).astype(np.int64)
    cat = lambda k, dt: np.concatenate([c[k] for c in chains] + [np.zeros(1, dt)]).astype(dt)
    link = np.concatenate([np.concatenate([c["link"], [0]])[:len(c["q"])] for c in chains] + [np.zeros(1, np.uint8)]).astype(np.uint8)
    dev = ctx.device
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    u32 = lambda a: tt(np.ascontiguousarray(a, np.uint32).view(np.int32))
    bufs = dict(n_chains=tt(np.array(n_chains, np.int32)), start=tt(start[:-1].copy()), length=tt(np.array([len(c["q"]) for c in chains], np.int32)),
                q=u32(cat("q", np.uint32)), t=u32(cat("t", np.uint32)), ln=tt(cat("len", np.int32)), st=tt(cat("strand", np.uint8)), cl=tt(cat("cluster", np.int32)), lk=tt(link))
    res = chain.ChainResult()
    res.n_reads = len(n_chains); res.num_aln = num_aln; res.n_frags = int(start[-1])
    res.d_n_chains = bufs["n_chains"].data_ptr(); res.d_chain_start = bufs["start"].data_ptr(); res.d_chain_len = bufs["length"].data_ptr()
    res.d_chain_q = bufs["q"].data_ptr(); res.d_chain_t = bufs["t"].data_ptr(); res.d_chain_alen = bufs["ln"].data_ptr(); res.d_chain_strand = bufs["st"].data_ptr()
    res.d_chain_cluster = bufs["cl"].data_ptr(); res.d_chain_link = bufs["lk"].data_ptr()
    out = chain.fetch_split(ctx, chain.split_chains_batch(ctx, res, list(chrom), splitdist, bypass))
    flagged = 0
    for s, c in enumerate(slots):
        live = s % num_aln < n_chains[s // num_aln]
        if c is None or not live:
            assert (out["n_kept"][s], out["n_split"][s], out["n_split_link"][s], out["status"][s]) == (0, 0, 0, 0), s
            continue
        flagged += _check_split(out, s, int(start[s]), c)
    return flagged


@pytest.mark.gpu
def test_hip_split_edges(ctx):
    """every crafted chain, one launch per (chromosome table, splitdist, bypass), two slots per read: reads with both slots live, with the second slot dead
    (n_chains 1: its chain must be ignored), with no live slot, and live slots of length 0"""
    groups = {}
    for name, c in SPLIT_CASES:
        groups.setdefault((c["chrom"], c["splitdist"], c["bypass"]), []).append(c)
    flagged = 0
    for (chrom, sd, by), cases in groups.items():
        slots = []; n_chains = []
        for i in range(0, len(cases), 2):
            pr = cases[i:i + 2]
            kind = (i // 2) % 4
            if len(pr) == 2 and kind != 1:
                slots += pr; n_chains.append(2)
            else:                                                           # the case alone in its read, a dead chain beside it
                for c in pr:
                    slots += [c, cases[0]]; n_chains.append(1)
            if kind == 2: slots += [None, cases[0]]; n_chains.append(2)    # a live slot of length 0 beside a full one
            if kind == 3: slots += [cases[0], cases[1 % len(cases)]]; n_chains.append(0)
        flagged += _run_split(ctx, slots, 2, n_chains, chrom, sd, by)
    assert flagged == len(cc.OOB) >= 1


@pytest.mark.gpu
def test_hip_split_slot_counts(ctx):
    """63, 64 and 65 slots: the last block full, one lane short, one lane over"""
    pool = [c for _, c in SPLIT_CASES if c["chrom"] == tuple(cc.CHROM) and c["splitdist"] == 50000 and c["bypass"] == 1]
    assert len(pool) >= 65
    for n in (63, 64, 65):
        assert _run_split(ctx, pool[:n], 1, [1] * n, cc.CHROM, 50000, 1) == 0
    assert _run_split(ctx, pool[:63] + [None] * 2, 5, [5] * 12 + [3], cc.CHROM, 50000, 1) == 0


def _run_hsplit(ctx, cases):
    import torch
    from lra_amd import chain
    sd = cases[0]["splitdist"]
    assert all(c["splitdist"] == sd for c in cases)
    dev = ctx.device
    job_off = np.concatenate([[0], np.cumsum([len(c["strand"]) for c in cases])]).astype(np.int64)
    link_off = np.concatenate([[0], np.cumsum([len(c["link"]) for c in cases])]).astype(np.int64)
    cat = lambda k, dt: np.concatenate([np.asarray(c[k], np.int64).reshape(-1) for c in cases] + [np.zeros(4, np.int64)]).astype(dt)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    strand = tt(cat("strand", np.int32))[:int(job_off[-1])]
    res = chain.split_chains_highacc_batch(ctx, tt(job_off), strand, tt(cat("chrom", np.int32)), tt(cat("box", np.uint32).view(np.int32)), tt(link_off), tt(cat("link", np.uint8)), sd)
    out = chain.fetch_hsplit(ctx, res)
    assert int(out["job_piece_off"][0]) == 0
    kinds = set()
    for j, c in enumerate(cases):
        exp = _hsplit_oracle(c)
        p0, p1 = int(out["job_piece_off"][j]), int(out["job_piece_off"][j + 1])
        assert p1 - p0 == len(exp["type"]), j
        assert int(out["lsc"][j]) == exp["lsc"], j
        for k in range(p1 - p0):
            a, b = int(out["piece_off"][p0 + k]), int(out["piece_off"][p0 + k + 1])
            assert out["sptc"][a:b].tolist() == exp["idx"][exp["off"][k]:exp["off"][k + 1]].tolist(), (j, k)
            assert out["type"][p0 + k] == exp["type"][k] and out["strand"][p0 + k] == exp["strand"][k] and out["box"][p0 + k].tolist() == exp["box"][k].tolist(), (j, k)
            assert int(out["job"][p0 + k]) == j
            kinds.add(chr(int(exp["type"][k])))
    return kinds


@pytest.mark.gpu
def test_hip_hsplit_edges(ctx):
    """every crafted job in one launch, the job of 0 elements among them; then 255, 256 and 257 jobs (the block of hsplit_lay)"""
    cases = [c for _, c in HSPLIT_CASES]
    assert any(len(c["strand"]) == 0 for c in cases) and any(len(c["strand"]) == 1 for c in cases)
    assert _run_hsplit(ctx, cases) == {"T", "D", "I", "N"}
    pool = (cases * 5)[:257]
    for n in (255, 256, 257):
        _run_hsplit(ctx, pool[:n])
        _run_hsplit(ctx, pool[257 - n:])
