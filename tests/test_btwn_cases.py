"""The crafted cases of tests/btwn_cases.py, on the CPU: the oracle tells the two sides of every threshold pair apart by what it DECIDES (matches per cluster and
flags; groups, anchors per group, lengths, strand, chromosome; trimmed lengths), no registered case makes it leave its arrays, and every comparison of the walks named
below has a pair under its name -- a pair deleted from the registry fails here.  The comparisons are those of oracle/refine_btwn.cpp:163-250 (Refine_Btwnsplitchain,
ChainRefine.h:579-754, with RefineBtwnSpace_AppendCloseCluster :59-121 and append_to_closetcluster :22-56) and of oracle/merge_extend.cpp (MergeChain ChainRefine.h:767-802,
TrimOverlappedAnchors LinearExtend.h:574-649 and :722-780)."""
import numpy as np

import btwn_cases as bc

S01 = ("s0", "s1")
ST1 = ("st1=0", "st1=1")
ENDS = tuple("%s/s%d" % (e, s) for e in ("first", "last") for s in (0, 1))
DOWN = ("first/s1", "last/s0")                       # the ends whose target runs downward: te = tStart, ts = te - gap
P12 = ("p1", "p2")
TRIMS = ("trim/s0", "trim/s1", "trimpairs/s0")

# comparison -> the pairs that must exist for it.  (Singles are listed where no output can differ in a decision: see profiles/btwn_merge_edges.md.)
REQUIRED = {
    # the gap loop: skip tests
    "a cluster of the pair is empty": ["gap.cur_empty/" + z for z in S01] + ["gap.prev_empty/" + z for z in S01],
    "qe <= qs": ["gap.qe<=qs/" + z for z in S01],
    # the three strand / link arms
    "same strand, link 0: cur.tEnd <= prev.tStart": ["gap.same0.cur.tEnd<=prev.tStart/" + z for z in S01],
    "same strand, link 0: cur.tStart > prev.tEnd, else skip": ["gap.same0.cur.tStart>prev.tEnd/" + z for z in S01],
    "strands differ, link 1: cur.tEnd <= prev.tStart": ["gap.diff1.cur.tEnd<=prev.tStart/%s/%s" % (z, p) for z in ST1 for p in P12],
    "strands differ, link 1: cur.tStart > prev.tEnd, else skip": ["gap.diff1.cur.tStart>prev.tEnd/%s/%s" % (z, p) for z in ST1 for p in P12],
    "strands differ, link 1: both geometries on both st1": ["gap.diff1.p%d_appends/%s/%s" % (w, g, z) for w in (1, 2) for g in ("below", "above") for z in ST1],
    "strands differ, link 1 against link 0": ["gap.diff1.link/%s/%s/%s" % (g, z, p) for g in ("below", "above") for z in ST1 for p in P12],
    "same strand, link 1: st1 == 0 && cur.tEnd > prev.tStart": ["gap.same1.cur.tEnd>prev.tStart/s0/" + p for p in P12] + ["gap.same1.link/s0/" + p for p in P12],
    "same strand, link 1: st1 == 1 && cur.tStart < prev.tEnd": ["gap.same1.cur.tStart<prev.tEnd/s1/" + p for p in P12] + ["gap.same1.link/s1/" + p for p in P12],
    "strands differ, link 0: plans nothing": ["gap.diff0.plans_nothing/" + z for z in S01],
    # space tests
    "te1 <= ts1": ["gap.te1<=ts1/" + z for z in S01],
    "te1 >= glen": ["gap.te1>=glen/" + z for z in S01],
    "SpaceLength >= 20": ["gap.space>=20/" + z for z in S01],
    "SpaceLength <= RSD": ["gap.space<=RSD/" + z for z in S01] + ["gap.space<=RSD.target/" + z for z in S01],
    "cur.chrom == prev.chrom": ["gap.chrom/" + z for z in S01],
    "second problem: te2 <= ts2": ["gap.diff1.te2<=ts2"],
    "second problem: te2 >= glen": ["gap.diff1.te2>=glen"],
    "second problem: SpaceLength >= 20": ["gap.diff1.space>=20/p2"],
    "second problem: SpaceLength <= RSD": ["gap.diff1.space<=RSD/%s/%s/p2" % (g, z) for g in ("below", "above") for z in ST1] + ["gap.same1.space<=RSD/%s/p2" % z for z in S01],
    "second problem: cur.chrom == prev.chrom": ["gap.diff1.chrom/%s/%s/p2" % (g, z) for g in ("below", "above") for z in ST1],
    # the two end rounds, on both strands
    "end: st == 1 with te <= qe - qs": ["end.te<=gap/first/s1"],
    "end: qe > qs": ["end.qe>qs/" + z for z in ENDS],
    "end: SpaceLength >= 20": ["end.space>=20/" + z for z in ENDS],
    "end: SpaceLength < RSD (strict)": ["end.space<RSD/" + z for z in ENDS],
    "end: te + 500 < glen": ["end.te+500<glen/" + z for z in ENDS],
    "end: ts > 500": ["end.ts>500/" + z for z in DOWN],
    "end: any non-empty result is appended": ["end.sparse_appends/" + z for z in ENDS] + ["end.empty/" + z for z in ENDS],
    # space_diag
    "0.15f (qe - qs) crossing 100": ["diag.100|101/" + z for z in S01],
    "0.15f (qe - qs) crossing 1000": ["diag.999|1000/" + z for z in S01],
    # the decisions on a result
    "an empty result": ["res.empty/" + z for z in S01],
    "eff >= 2 anchorstoosparse at equality": ["res.eff>=2sparse/" + z for z in S01],
    "the same for a two-block first problem": ["res.two.eff>=2sparse/" + z for z in ST1],
    "the second problem appends any non-empty result": ["res.two.second_appends_sparse/" + z for z in ST1],
    "min(|dq|, |dt|) <= 200": ["res.cut<=200.%s/%s" % (c, z) for c in ("dq", "dt") for z in S01],
    "run length >= 4": ["res.run>=4/" + z for z in S01],
    "dist_cur <= dist_prev": ["res.dist_cur<=dist_prev/" + z for z in S01] + ["res.dist_cur<=dist_prev.target%+d/%s" % (d, z) for d in (20, -20) for z in S01],
    "several runs, the second sees the box the first moved": ["res.runs.second_sees_moved_box/" + z for z in S01],
    # order
    "gap c after gap c - 1": ["order.gap2.ts1_moves", "order.gap2.arm_flips_to_skip", "order.gap2.te1_moves", "order.gap2.first_arm_flips_to_skip",
                              "order.run_to_prev.then_first_end.run"],
    "the end rounds after the gap rounds": ["order.run_to_prev.moves_first_end/" + z for z in S01] + ["order.run_to_prev.moves_first_end.stale/" + z for z in S01] +
                                           ["order.append_to_last.moves_last_end", "order.append_to_last.moves_last_end.stale"],
    "refinespace set by the dense append, not by the sparse one": ["res.refinespace.dense|sparse/" + z for z in S01],
    "nsp == 1: both end rounds on one cluster": ["order.nsp1.both_ends/" + z for z in S01] + ["order.nsp1.both_ends'/" + z for z in S01],
    # MergeChain
    "qdist <= 500": ["merge.qdist<=500/" + z for z in S01] + ["merge.qdist.overlap_is_0/" + z for z in S01],
    "tdist <= 500": ["merge.tdist<=500/" + z for z in S01],
    "prev.tStart >= cur.tEnd / prev.tEnd <= cur.tStart at equality": ["merge.tdist.touching_is_0/" + z for z in S01],
    "different chromosome, different strand": ["merge.chrom/" + z for z in S01] + ["merge.strand/" + z for z in S01],
    "groupings": ["merge.n=6.all|none/" + z for z in S01] + ["merge.n=6.middle_run/" + z for z in S01],
    "members without matches": ["merge.member_empty.middle/" + z for z in S01] + ["merge.member_empty.last/" + z for z in S01] + ["merge.group_without_anchors/" + z for z in S01],
    # trim
    "long anchor length 39 | 40 and 49 | 50": ["trim.len>=%d/%s" % (50 if z.startswith("trimpairs") else 40, z) for z in TRIMS] +
                                              ["trim.cur.len>=%d/%s" % (50 if z.startswith("trimpairs") else 40, z) for z in TRIMS],
    "read overlap 0 | 1 and 30 | 31": ["trim.read_overlap>0/" + z for z in TRIMS] + ["trim.read_overlap<=30/" + z for z in TRIMS],
    "genome overlap 0 | 1 and 30 | 31": ["trim.genome_overlap>0/" + z for z in TRIMS] + ["trim.genome_overlap<=30/" + z for z in TRIMS],
    "the maximum of both overlaps": ["trim.max_of_both/" + z for z in TRIMS] + ["trim.max_of_both'/" + z for z in TRIMS],
    "the middle anchor trimmed as prev after serving as cur": ["trim.middle_as_prev/" + z for z in TRIMS],
}
# layouts and paths that must stay registered as singles
REQUIRED_SINGLES = (["gap.space>=5RSD.%d/%s" % (g, z) for g in (499, 500) for z in S01] + ["gap.diff1.space>=5RSD.%d" % g for g in (499, 500)] +
                    ["gap.diff1.clamp.te1=gap%+d" % d for d in (1, 0, -1)] + ["gap.diff1.clamp.te2=gap%+d" % d for d in (1, 0, -1)] +
                    ["end.clamp.te=gap%+d/last/s0" % d for d in (1, 0, -1)] + ["end.space<RSD.at_RSD/" + z for z in ENDS] +
                    ["end.class.target=%d/%s" % (g, z) for g in (999, 1000, 1001) for z in ENDS] + ["res.class.q=t=%d/%s" % (g, z) for g in (999, 1000, 1001) for z in S01] +
                    ["layout.nsp=0", "layout.nsp=6", "layout.nsp=6.s1", "pool.few_then_thousands", "layout.three_segments", "order.unread_sides.with", "order.unread_sides.without"] +
                    ["layout.base=%d.segment=%d" % (n, n) for n in (63, 64, 65)] + ["merge.concat.%s=%d/%s" % (k, n, z) for k in ("one", "three") for n in (63, 64, 65) for z in S01] +
                    ["merge.sort.diag_signs", "merge.sort.chrom1", "merge.sort.chrom2", "merge.no_matches", "merge.nsp=0"] +
                    ["merge.sort.n=%d/s%d" % (n, s) for n in (256, 257, 1024, 1025) for s in (0, 1)] + ["trim.equal_keys/" + z for z in TRIMS])


def test_pairs_differ_in_the_decision():
    same = [n for n, (a, b) in bc.PAIRS.items() if bc.decision(a) == bc.decision(b)]
    assert not same, same


def test_no_case_leaves_the_arrays():
    none = [n for n, c in bc.all_cases() if bc.run(c) is None]
    assert not none, none


def test_every_named_comparison_has_its_pairs():
    missing = [(k, n) for k, names in REQUIRED.items() for n in names if n not in bc.PAIRS]
    missing += [("single", n) for n in REQUIRED_SINGLES if n not in bc.SINGLES]
    assert not missing, missing
    listed = {n for names in REQUIRED.values() for n in names}
    assert len(listed) == sum(len(v) for v in REQUIRED.values())                          # no pair counted for two comparisons


def test_unread_sides_leave_the_next_gap_alone():
    """gap 1's append grows only c1.qEnd / c1.tEnd; gap 2 reads c1.qStart / c1.tStart: it finds the same with and without that append"""
    a, b = bc.SINGLES["order.unread_sides.with"], bc.SINGLES["order.unread_sides.without"]
    assert bc.gap2_added(a) == bc.gap2_added(b) and len(bc.gap2_added(a)[0]) > 10
    assert len(bc.added(a)[1]) > len(bc.added(b)[1])


def test_named_paths_are_what_they_say():
    """a few singles whose name promises a path: the counts the layout copies by waves, the late round of thousands, runs to both clusters, the clamps"""
    for n in (63, 64, 65):
        c = bc.SINGLES["layout.base=%d.segment=%d" % (n, n)]
        assert [len(x["matches"]) for x in c["clusters"]] == [2, n] and [len(a) for a in bc.added(c)] == [0, n]
    big = bc.added(bc.SINGLES["pool.few_then_thousands"])
    assert 4 <= len(big[1]) < 20 and len(big[2]) > 2000
    for z in S01:
        to = [len(a) for a in bc.added(bc.SINGLES["res.runs.two_clusters/" + z])]
        assert min(to) >= 4
        a, b = bc.PAIRS["res.eff>=2sparse/" + z]
        ra, rb = bc.oracle_btwn(a), bc.oracle_btwn(b)
        assert ra["refinespace"].tolist() == [0, 1] and rb["refinespace"].tolist() == [0, 0]     # the dense append sets the flag, the sparse one does not
        assert len(ra["q"]) == len(rb["q"])
    for n in [k for k in bc.SINGLES if "space>=5RSD" in k]:
        assert [len(a) for a in bc.added(bc.SINGLES[n])] == [0, 0], n                       # refused on either side of 5 RSD
    seg = bc.oracle_btwn(bc.SINGLES["layout.three_segments"])
    assert seg["refinespace"].tolist() == [0, 0, 0] and int(seg["off"][2] - seg["off"][1]) > 64 + 8
    assert [len(a) for a in bc.added(bc.SINGLES["layout.nsp=6"])] == [0] + [19] * 5


def test_packer_layout():
    named = [(n, c) for n, c in bc.all_cases() if c["kind"] == "btwn"]
    P = bc.pack(named)
    assert len(P["where"]) == len(named) and P["n_slots"] == P["n_reads"] * P["num_aln"] and int(P["match_off"][-1]) == P["n_matches"]
    assert int(P["n_chains"].max()) == 3 and int((P["n_chains"] < P["num_aln"]).sum()) > 10 and int((P["status"] != 0).sum()) > 10
    used = np.zeros(P["n_frags"], bool)
    for n, c in named:
        s, b = P["where"][n]
        nsp = len(c["clusters"])
        assert int(P["chain_start"][s]) == b and int(P["n_split"][s]) == nsp and P["status"][s] == 0 and s % P["num_aln"] < P["n_chains"][s // P["num_aln"]]
        assert not used[b:b + nsp].any()
        used[b:b + nsp] = True
        assert P["box"].reshape(-1, 4)[b:b + nsp].tolist() == [list(x["box"]) for x in c["clusters"]]
        assert P["split_link"][b:b + max(nsp - 1, 0)].tolist() == c["link"]
        r = s // P["num_aln"]
        assert P["strands"][int(P["read_off"][r]):int(P["read_off"][r + 1])].tobytes() == c["read"]
        assert P["strands"][P["rc_base"] + int(P["read_off"][r]):P["rc_base"] + int(P["read_off"][r + 1])].tobytes() == bc.revcomp(np.frombuffer(c["read"], np.uint8)).tobytes()
    assert int((~used).sum()) > len(named)                                                  # padding fragments between the chains
    assert np.all(np.diff(P["match_off"].astype(np.int64))[~used] > 0)                     # ... with matches of their own
    rev = bc.pack(named[::-1], pad=False, marked=False)
    assert rev["n_frags"] == int(used.sum()) and rev["where"][named[0][0]][0] > rev["where"][named[-1][0]][0]
    one = bc.pack(named[:5], num_aln=1, empty_slots=252)
    assert one["n_slots"] == 257 and one["where"][named[4][0]][0] == 256


def test_world():
    assert bc.CHROM[1] % 256 != 0 and bc.GLEN[2] == 3000 and len(bc.GBYTES) == bc.CHROM[-1]
