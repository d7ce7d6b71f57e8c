#!/usr/bin/env python3
"""What the inputs of Refine_Btwnsplitchain and of the merge / extend / trim pass can tell apart, measured on the CPU with the machinery of tools/oracle_mutants.py:
one comparison or constant of the WALK in oracle/refine_btwn.cpp or oracle/merge_extend.cpp (not RefineSpace, not LinearExtend) is changed at a time in a temporary
copy, the copy is compiled alone to a shared object (RefineSpace and LinearExtend resolve against the unchanged oracle library), and two sets of inputs are run
through it: the arguments tests/oracle_pipeline.py passes to refine_btwn_splitchain / merge_extend for simulated reads of the kinds the older GPU tests use (plain
reads, two-locus chimeras, an inversion, a 6 kb deletion; splitdist 5000, both anchorstoosparse values of test_hip_refine_btwn_splitchain_oracle), and the crafted
cases of tests/btwn_cases.py.  Printed per mutant: the number of inputs whose expected output changes.  A mutant that changes no input is one the kernels could
carry while every test passes.  CPU only; not part of the suite.

    python tools/oracle_mutants_btwn.py [--jobs N] [--only SUBSTRING] [--reads N]"""
import argparse
import concurrent.futures as cf
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle_mutants import compile_one, mutate  # noqa: E402

BTWN = os.path.join(ROOT, "oracle", "refine_btwn.cpp")
MERGE = os.path.join(ROOT, "oracle", "merge_extend.cpp")

CLAMP1 = "ts1 = (te1 > (qe - qs) ? te1 - (qe - qs) : 0)"
CLAMP2 = "ts2 = (te2 > (qe - qs) ? te2 - (qe - qs) : 0)"
GAP_SPACE = "if (SpaceLength >= 20 && SpaceLength <= RSD && cur.chrom == prev.chrom) append_close"
GAP_SPACE2 = "if (SpaceLength >= 20 && SpaceLength <= RSD && cur.chrom == prev.chrom) btwn_space"
END_SPACE = "if (SpaceLength >= 20 && SpaceLength < RSD && te + 500 < glen(h.chrom)) {"
R_OVL = "if (Q[cur] < Q[prev] + L[prev] && Q[cur] >= Q[prev] + L[prev] - 30)"
R_OVL1 = "if (Q[cur] + L[cur] > Q[prev] && Q[cur] + L[cur] <= Q[prev] + 30)"
G_OVL = "if (T[cur] < T[prev] + L[prev] && T[cur] >= T[prev] + L[prev] - 30)"

# (part, name, old text, new text, which occurrence (None: all), expect: "" or the reason no input can separate it)
MUTANTS = [
    # ---- Refine_Btwnsplitchain: the gap loop
    ("btwn", "skip test ignores an empty cur", "cur.m.empty() || prev.m.empty()", "prev.m.empty()", None, ""),
    ("btwn", "skip test ignores an empty prev", "cur.m.empty() || prev.m.empty()", "cur.m.empty()", None, ""),
    ("btwn", "qe <= qs -> <", "if (qe <= qs) { c++; continue; }", "if (qe < qs) { c++; continue; }", None, "at qe == qs the query has length 0: RefineSpace finds nothing"),
    ("btwn", "same strand link 0: cur.tEnd <= prev.tStart -> <", "if (cur.tEnd <= prev.tStart) { ts1 = cur.tEnd; te1 = prev.tStart; }", "if (cur.tEnd < prev.tStart) { ts1 = cur.tEnd; te1 = prev.tStart; }", None,
     "at equality te1 == ts1, skipped by the next test; under < the second arm fails too"),
    ("btwn", "same strand link 0: first arm never taken", "if (cur.tEnd <= prev.tStart) { ts1 = cur.tEnd; te1 = prev.tStart; }", "if (false) { ts1 = cur.tEnd; te1 = prev.tStart; }", None, ""),
    ("btwn", "same strand link 0: cur.tStart > prev.tEnd -> >=", "else if (cur.tStart > prev.tEnd) { ts1 = prev.tEnd; te1 = cur.tStart; }", "else if (cur.tStart >= prev.tEnd) { ts1 = prev.tEnd; te1 = cur.tStart; }", None,
     "at equality te1 == ts1, skipped by the next test"),
    ("btwn", "same strand link 0: second arm never taken", "else if (cur.tStart > prev.tEnd) { ts1 = prev.tEnd; te1 = cur.tStart; }", "else if (false) { ts1 = prev.tEnd; te1 = cur.tStart; }", None, ""),
    ("btwn", "strands differ: link ignored", "} else if (cur.strand != prev.strand && link[c - 1] == 1) {", "} else if (cur.strand != prev.strand) {", None, ""),
    ("btwn", "strands differ link 1: cur.tEnd <= prev.tStart -> <", "      if (cur.tEnd <= prev.tStart) {\n        if (st1 == 0) { ts1 = cur.tEnd; te1 = ts1 + qe - qs; ts2 = prev.tEnd;",
     "      if (cur.tEnd < prev.tStart) {\n        if (st1 == 0) { ts1 = cur.tEnd; te1 = ts1 + qe - qs; ts2 = prev.tEnd;", None, ""),
    ("btwn", "strands differ link 1: cur.tStart > prev.tEnd -> >=", "      } else if (cur.tStart > prev.tEnd) {\n        if (st1 == 0)", "      } else if (cur.tStart >= prev.tEnd) {\n        if (st1 == 0)", None, ""),
    ("btwn", "strands differ link 1, below, st1 0: ts2 = prev.tEnd -> prev.tStart", "ts2 = prev.tEnd; te2 = ts2 + qe - qs; }", "ts2 = prev.tStart; te2 = ts2 + qe - qs; }", None, ""),
    ("btwn", "strands differ link 1, above, st1 0: te2 = cur.tStart -> prev.tStart", "te1 = ts1 + qe - qs; te2 = cur.tStart;", "te1 = ts1 + qe - qs; te2 = prev.tStart;", None, ""),
    ("btwn", "same strand link 1: link ignored", "} else if (cur.strand == prev.strand && link[c - 1] == 1) {", "} else if (cur.strand == prev.strand) {", None, "unreachable: link 0 took the first branch"),
    ("btwn", "same strand link 1: cur.tEnd > prev.tStart -> >=", "if (st1 == 0 && cur.tEnd > prev.tStart)", "if (st1 == 0 && cur.tEnd >= prev.tStart)", None, ""),
    ("btwn", "same strand link 1: cur.tStart < prev.tEnd -> <=", "else if (st1 == 1 && cur.tStart < prev.tEnd)", "else if (st1 == 1 && cur.tStart <= prev.tEnd)", None, ""),
    ("btwn", "clamp te1 > gap -> >= (all three)", CLAMP1, CLAMP1.replace("te1 > (qe", "te1 >= (qe"), None, "te - gap is 0 at te == gap: both forms give ts = 0"),
    ("btwn", "clamp te2 > gap -> >= (all four)", CLAMP2, CLAMP2.replace("te2 > (qe", "te2 >= (qe"), None, "te - gap is 0 at te == gap: both forms give ts = 0"),
    ("btwn", "clamp te1: no clamp (wraps below 0)", CLAMP1, "ts1 = te1 - (qe - qs)", None, ""),
    ("btwn", "clamp te2: no clamp (wraps below 0)", CLAMP2, "ts2 = te2 - (qe - qs)", None, ""),
    ("btwn", "te1 <= ts1 -> <", "if (te1 <= ts1) { c++; continue; }", "if (te1 < ts1) { c++; continue; }", None, "a target of length 0: RefineSpace finds nothing (and the strands-differ, link 0 case has a query to offer but te1 = ts1 = 0)"),
    ("btwn", "te1 >= glen -> >", "if (te1 >= glen(cur.chrom)) { c++; continue; }", "if (te1 > glen(cur.chrom)) { c++; continue; }", None, ""),
    ("btwn", "first problem: 5 RSD test removed", "if (std::max(qe - qs, te1 - ts1) >= 5 * RSD) { c++; continue; }", "", None,
     "a space of 5 RSD or more fails `<= RSD` as well, and the second problem's space has the same read gap: it fails there too"),
    ("btwn", "first problem: SpaceLength >= 20 -> >", GAP_SPACE, GAP_SPACE.replace(">= 20", "> 20"), None, ""),
    ("btwn", "first problem: SpaceLength <= RSD -> <", GAP_SPACE, GAP_SPACE.replace("<= RSD", "< RSD"), None, ""),
    ("btwn", "first problem: chromosome test removed", GAP_SPACE, GAP_SPACE.replace(" && cur.chrom == prev.chrom", ""), None, ""),
    ("btwn", "te2 <= ts2 -> <", "if (te2 <= ts2) { c++; continue; }", "if (te2 < ts2) { c++; continue; }", None, "a target of length 0: RefineSpace finds nothing"),
    ("btwn", "te2 <= ts2 test removed", "if (te2 <= ts2) { c++; continue; }", "", None, "te2 < ts2 needs te2 = ts2 + gap to wrap past 2^32: no chromosome is that long here"),
    ("btwn", "te2 >= glen -> >", "if (te2 >= glen(cur.chrom)) { c++; continue; }", "if (te2 > glen(cur.chrom)) { c++; continue; }", None, ""),
    ("btwn", "second problem: 5 RSD test removed", "if (std::max(qe - qs, te2 - ts2) >= 5 * RSD) { c++; continue; }", "", None, "a space of 5 RSD or more fails `<= RSD` as well"),
    ("btwn", "second problem: SpaceLength >= 20 -> >", GAP_SPACE2, GAP_SPACE2.replace(">= 20", "> 20"), None, ""),
    ("btwn", "second problem: SpaceLength <= RSD -> <", GAP_SPACE2, GAP_SPACE2.replace("<= RSD", "< RSD"), None, ""),
    ("btwn", "second problem: chromosome test removed", GAP_SPACE2, GAP_SPACE2.replace(" && cur.chrom == prev.chrom", ""), None, ""),
    # ---- the two end rounds
    ("btwn", "first end, strand 1: te > gap -> >=", "if (te > qe - qs) ts = te - (qe - qs); else { te = 0; tsSet = false; }", "if (te >= qe - qs) ts = te - (qe - qs); else { te = 0; tsSet = false; }", None, ""),
    ("btwn", "first end: qe > qs -> >=", "if (qe > qs && te > ts) {", "if (qe >= qs && te > ts) {", 0, "at qe == qs, te == ts on strand 0 and te = 0 on strand 1: `te > ts` fails"),
    ("btwn", "first end: SpaceLength >= 20 -> >", END_SPACE, END_SPACE.replace(">= 20", "> 20"), 0, ""),
    ("btwn", "first end: SpaceLength < RSD -> <=", END_SPACE, END_SPACE.replace("< RSD", "<= RSD"), 0, ""),
    ("btwn", "first end: te + 500 < glen -> <=", END_SPACE, END_SPACE.replace("te + 500 < glen", "te + 500 <= glen"), 0, ""),
    ("btwn", "first end: ts > 500 -> >=", "else { if (ts > 500) lrts = 500; lrlength = lrts; }", "else { if (ts >= 500) lrts = 500; lrlength = lrts; }", None, ""),
    ("btwn", "last end: clamp te > gap -> >=", "if (te > qe - qs) ts = te - (qe - qs); else ts = 0; }", "if (te >= qe - qs) ts = te - (qe - qs); else ts = 0; }", None, "te - gap is 0 at te == gap"),
    ("btwn", "last end: qe > qs -> >=", "if (qe > qs && te > ts) {", "if (qe >= qs && te > ts) {", 1, "at qe == 0 the gap is 0 and te == ts"),
    ("btwn", "last end: SpaceLength >= 20 -> >", END_SPACE, END_SPACE.replace(">= 20", "> 20"), 1, ""),
    ("btwn", "last end: SpaceLength < RSD -> <=", END_SPACE, END_SPACE.replace("< RSD", "<= RSD"), 1, ""),
    ("btwn", "last end: te + 500 < glen -> <=", END_SPACE, END_SPACE.replace("te + 500 < glen", "te + 500 <= glen"), 1, ""),
    ("btwn", "last end: ts > 500 -> >=", "if (st == 0) { if (ts > 500) lrts = 500; lrlength = lrts; }", "if (st == 0) { if (ts >= 500) lrts = 500; lrlength = lrts; }", None, ""),
    # ---- space_diag
    ("btwn", "space_diag floor 100 -> 101", "std::max(100.f, 0.15f * (qe - qs))", "std::max(101.f, 0.15f * (qe - qs))", None, ""),
    ("btwn", "space_diag cap 1000 -> 999", "0.15f * (qe - qs))), 1000); }", "0.15f * (qe - qs))), 999); }", None, ""),
    ("btwn", "space_diag 0.15f -> 0.1501f", "0.15f * (qe - qs)", "0.1501f * (qe - qs)", None, ""),
    # ---- the decisions on a result
    ("btwn", "eff >= 2 sparse -> > (first problem)", "if (eff >= E.o->anchorstoosparse * 2) { c->m.insert", "if (eff > E.o->anchorstoosparse * 2) { c->m.insert", None, ""),
    ("btwn", "a sparse two-block first problem is not dropped", "  if (twoblocks) return;\n  std::sort(P.begin(), P.end());", "  std::sort(P.begin(), P.end());", None, ""),
    ("btwn", "dense append leaves refinespace 0", "c->bounds(E.o->K); c->refinespace = 1; return; }\n  if (twoblocks) return;\n  std::sort", "c->bounds(E.o->K); return; }\n  if (twoblocks) return;\n  std::sort", None, ""),
    ("btwn", "sparse append sets refinespace", "  d->bounds(K);\n}", "  d->bounds(K); d->refinespace = 1;\n}", None, ""),
    ("btwn", "run cut <= 200 -> <", "<= 200) end++;", "< 200) end++;", None, ""),
    ("btwn", "run cut on the read step alone", "std::min(std::labs((long)P[end].first - (long)P[end - 1].first), std::labs((long)P[end].second - (long)P[end - 1].second)) <= 200", "std::labs((long)P[end].first - (long)P[end - 1].first) <= 200", None, ""),
    ("btwn", "run cut on the target step alone", "std::min(std::labs((long)P[end].first - (long)P[end - 1].first), std::labs((long)P[end].second - (long)P[end - 1].second)) <= 200", "std::labs((long)P[end].second - (long)P[end - 1].second) <= 200", None, ""),
    ("btwn", "run length >= 4 -> >= 5", "if (end - start >= 4) append_to_closest", "if (end - start >= 5) append_to_closest", None, ""),
    ("btwn", "run length >= 4 -> >= 3", "if (end - start >= 4) append_to_closest", "if (end - start >= 3) append_to_closest", None, ""),
    ("btwn", "dist_cur <= dist_prev -> <", "Clu* d = dist_cur <= dist_prev ? c : p;", "Clu* d = dist_cur < dist_prev ? c : p;", None, ""),
    ("btwn", "dist_cur: strand 0 target distance on both strands", "if (st == 0) tdist = (tStart >= c->tEnd) ? tStart - c->tEnd : 0;", "if (true) tdist = (tStart >= c->tEnd) ? tStart - c->tEnd : 0;", None, ""),
    ("btwn", "dist_prev: strand 0 target distance on both strands", "if (st == 0) tdist = (p->tStart >= tEnd) ? p->tStart - tEnd : 0;", "if (true) tdist = (p->tStart >= tEnd) ? p->tStart - tEnd : 0;", None, ""),
    ("btwn", "dist: read distance alone", "const int dist_cur = std::max(qdist, tdist);", "const int dist_cur = qdist;", None, ""),
    ("btwn", "second problem / ends: a sparse result is not appended", "if ((!P.empty() && twoblocks) || (!P.empty() && eff >= E.o->anchorstoosparse * 2)) {", "if (!P.empty() && eff >= E.o->anchorstoosparse * 2) {", None, ""),
    # ---- MergeChain
    ("merge", "qdist: prev.qStart > cur.qEnd -> >=", "qdist = (pqs > cqe) ? (int)(pqs - cqe) : 0;", "qdist = (pqs >= cqe) ? (int)(pqs - cqe) : 0;", None, "pqs - cqe is 0 at equality"),
    ("merge", "qdist <= 500 -> <", "if (qdist <= 500 && tdist <= 500) continue;", "if (qdist < 500 && tdist <= 500) continue;", None, ""),
    ("merge", "tdist <= 500 -> <", "if (qdist <= 500 && tdist <= 500) continue;", "if (qdist <= 500 && tdist < 500) continue;", None, ""),
    ("merge", "strand 0: prev.tStart >= cur.tEnd -> >", "tdist = (pts >= cte) ? (int)(pts - cte) : 9999;", "tdist = (pts > cte) ? (int)(pts - cte) : 9999;", None, ""),
    ("merge", "strand 1: prev.tEnd <= cur.tStart -> <", "else tdist = (pte <= cts) ? (int)(cts - pte) : 9999;", "else tdist = (pte < cts) ? (int)(cts - pte) : 9999;", None, ""),
    ("merge", "strand 0 target distance on both strands", "if (strand[prev] == 0) tdist = (pts >= cte)", "if (true) tdist = (pts >= cte)", None, ""),
    ("merge", "an overlap on the target counts as 0", "tdist = (pts >= cte) ? (int)(pts - cte) : 9999;", "tdist = (pts >= cte) ? (int)(pts - cte) : 0;", None, ""),
    ("merge", "chromosome ignored", "if (chrom[prev] == chrom[cur] && strand[prev] == strand[cur]) {", "if (strand[prev] == strand[cur]) {", None, ""),
    ("merge", "strand ignored", "if (chrom[prev] == chrom[cur] && strand[prev] == strand[cur]) {", "if (chrom[prev] == chrom[cur]) {", None, ""),
    ("merge", "DiagonalSort: diagonals descending", "if (aDiag != bDiag) return aDiag < bDiag;", "if (aDiag != bDiag) return aDiag > bDiag;", None, ""),
    ("merge", "DiagonalSort: q descending within a diagonal", "        return a.first < b.first;\n      });", "        return a.first > b.first;\n      });", None, ""),
    ("merge", "DiagonalSort: diagonal in 32 bits unsigned", "const long aDiag = (long)a.first - (long)a.second, bDiag = (long)b.first - (long)b.second;",
     "const long aDiag = (long)(uint32_t)(a.first - a.second), bDiag = (long)(uint32_t)(b.first - b.second);", None, ""),
    ("merge", "a group without anchors keeps its last member's strand and chromosome", "} else { gstrand[r] = 0; gchrom[r] = 0; }", "} else { gstrand[r] = (uint8_t)st; gchrom[r] = ci; }", None, ""),
    ("merge", "strand and chromosome from the last member WITH matches", "      st = strand[cI]; ci = chrom[cI];\n      const int n = matchOff[cI + 1] - matchOff[cI];",
     "      const int n = matchOff[cI + 1] - matchOff[cI];\n      if (n) { st = strand[cI]; ci = chrom[cI]; }", None, "members of one group have the same strand and chromosome"),
    # ---- TrimOverlappedAnchors (all copies of the walk at once: the one inside merge_extend sees the older inputs, the two entry points the crafted anchors)
    ("trim", "long anchor >= 40 -> >", "if (L[i] >= 40) idx.push_back", "if (L[i] > 40) idx.push_back", None, ""),
    ("trim", "long anchor >= 50 -> > (pair version)", "if (L[i] >= 50) idx.push_back", "if (L[i] > 50) idx.push_back", None, ""),
    ("trim", "read overlap: Q[cur] < end -> <=", R_OVL, R_OVL.replace("Q[cur] < Q[prev]", "Q[cur] <= Q[prev]"), None, "an overlap of 0 changes nothing unless the genome overlaps too; then the maximum is the genome's"),
    ("trim", "read overlap: >= end - 30 -> >", R_OVL, R_OVL.replace("Q[cur] >= Q[prev] + L[prev] - 30", "Q[cur] > Q[prev] + L[prev] - 30"), None, ""),
    ("trim", "read overlap: 30 -> 31", R_OVL, R_OVL.replace("- 30", "- 31"), None, ""),
    ("trim", "strand 1 read overlap: > Q[prev] -> >=", R_OVL1, R_OVL1.replace("Q[cur] + L[cur] > Q[prev]", "Q[cur] + L[cur] >= Q[prev]"), None, "an overlap of 0 changes nothing"),
    ("trim", "strand 1 read overlap: <= Q[prev] + 30 -> <", R_OVL1, R_OVL1.replace("<= Q[prev] + 30", "< Q[prev] + 30"), None, ""),
    ("trim", "strand 1 read overlap: 30 -> 31", R_OVL1, R_OVL1.replace("+ 30", "+ 31"), None, ""),
    ("trim", "genome overlap: T[cur] < end -> <=", G_OVL, G_OVL.replace("T[cur] < T[prev]", "T[cur] <= T[prev]"), None, "an overlap of 0 changes nothing"),
    ("trim", "genome overlap: >= end - 30 -> >", G_OVL, G_OVL.replace("T[cur] >= T[prev] + L[prev] - 30", "T[cur] > T[prev] + L[prev] - 30"), None, ""),
    ("trim", "genome overlap: 30 -> 31", G_OVL, G_OVL.replace("- 30", "- 31"), None, ""),
    ("trim", "the smaller of the two overlaps", "const int overlap = std::max(overlap_r, overlap_g);", "const int overlap = std::min(overlap_r, overlap_g) > 0 ? std::min(overlap_r, overlap_g) : std::max(overlap_r, overlap_g);", None, ""),
    ("trim", "strand 1: Q[prev] not moved", "if (S == 1) Q[prev] += overlap + 1;", "", None, ""),
    ("trim", "trim by overlap, not overlap + 1", "L[prev] -= overlap + 1;", "L[prev] -= overlap;", None, ""),
    ("trim", "strand 1 order: read end ascending", "if (Q[i] + L[i] != Q[j] + L[j]) return Q[i] + L[i] > Q[j] + L[j];", "if (Q[i] + L[i] != Q[j] + L[j]) return Q[i] + L[i] < Q[j] + L[j];", None, ""),
    ("trim", "equal keys ordered by length (a stable order)", "return T[i] < T[j];", "if (T[i] != T[j]) return T[i] < T[j]; return L[i] < L[j];", None, ""),
]


def older_inputs(n_reads):
    """the arguments of refine_btwn_splitchain / merge_extend on simulated reads, as cases of tests/btwn_cases.py would be run: [(kind, args, kwargs)]"""
    import oracle_lib as O
    import oracle_pipeline as OP
    from lra_amd import synth
    genome = synth.make_genome(300_000, seed=41, repeat_frac=0.3, n_families=3)
    CH = [0, 149_900, len(genome)]
    ik, ip = synth.build_global_index(genome, 17, 10, 100)
    tups, bnd = [], [0]
    for c in range(2):
        t, b = O.local_index_seq(genome[CH[c]:CH[c + 1]].tobytes(), 10, 5, 256, 15)
        tups.append(t); bnd.extend((b[1:] + bnd[-1]).tolist())
    g_index = (OP.seq_offsets_multi(CH, 256), np.array(bnd, np.uint64), np.concatenate(tups))
    gbytes = genome.tobytes() + b"\0" * 64
    reads, _ = synth.simulate_reads(genome, n_reads, 9000, 3000, 0.10, seed=19)
    rng = np.random.default_rng(8)
    sim = lambda a, n, e, rev=False: synth.simulate_read(rng, genome[a:a + n + 1], n, e, (30, 35, 35), rev)[0]
    for j in range(max(2, n_reads // 4)):
        a = int(rng.integers(10_000, 120_000)); b = int(rng.integers(160_000, 280_000))
        reads.append(np.concatenate([sim(a, 4000, 0.08), sim(b, 4000, 0.08, bool(j & 1))]))
    for j in range(max(2, n_reads // 8)):
        a = int(rng.integers(20_000, 120_000))
        reads.append(np.concatenate([sim(a, 4000, 0.06), sim(a + 4000, 2500, 0.06, True), sim(a + 6500, 4000, 0.06)]))
        b = int(rng.integers(160_000, 270_000))
        de = np.concatenate([sim(b, 4000, 0.06), sim(b + 10_000, 4000, 0.06)])
        reads.append(de if j & 1 else synth.revcomp(de))
    got = []
    real_b, real_m = O.refine_btwn_splitchain, O.merge_extend

    def spy_b(*a, **k):
        got.append(("btwn", a, k))
        return real_b(*a, **k)

    def spy_m(*a, **k):
        got.append(("merge", a, k))
        return real_m(*a, **k)
    O.refine_btwn_splitchain, O.merge_extend = spy_b, spy_m
    try:
        for sparse in (0.01, 0.2):
            for rd in reads:
                OP.map_read_lowacc_py(rd.tobytes(), gbytes, ik, ip, g_index, dict(splitdist=5000, refineSpaceDist=10000, anchorstoosparse=sparse), stats=False, chrom_pos=CH)
    finally:
        O.refine_btwn_splitchain, O.merge_extend = real_b, real_m
    return got, len(reads)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", default=None, help="run only the mutants whose name contains this")
    ap.add_argument("--reads", type=int, default=24, help="plain simulated reads among the older inputs (chimeras, inversions and deletions are added in proportion)")
    a = ap.parse_args()
    import btwn_cases as bc
    import oracle_lib as O
    base_lib = O.lib()
    C.CDLL(os.path.join(ROOT, "oracle", "liblra_oracle.so"), mode=C.RTLD_GLOBAL)          # RefineSpace / LinearExtend for the mutated copies
    old, n_old_reads = older_inputs(a.reads)
    kinds = {"btwn": ("btwn",), "merge": ("merge",), "trim": ("merge", "trim", "trimpairs")}
    new = {p: [c for _, c in bc.all_cases() if c["kind"] in kinds[p]] for p in kinds}
    n_lists = sum(c["kind"] in ("trim", "trimpairs") for c in new["trim"])
    oldp = {p: [x for x in old if x[0] in kinds[p]] for p in kinds}
    muts = [m for m in MUTANTS if a.only is None or a.only in m[1]]
    text = {"btwn": open(BTWN).read(), "merge": open(MERGE).read(), "trim": open(MERGE).read()}
    hashable = lambda r: None if r is None else tuple((k, v.tobytes() if hasattr(v, "tobytes") else v) for k, v in sorted(r.items()))
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(tmp, 0, text["btwn"]), (tmp, 1, text["merge"])] + [(tmp, k + 2, mutate(text[m[0]], m[2], m[3], m[4])) for k, m in enumerate(muts)]
        with cf.ThreadPoolExecutor(a.jobs) as ex:
            sos = list(ex.map(compile_one, jobs))

        def outputs(so, part):
            O._LIB = C.CDLL(so)
            try:
                o = [hashable((O.refine_btwn_splitchain if k == "btwn" else O.merge_extend)(*args, **kw)) for k, args, kw in oldp[part]]
                return o, [bc.run(c) for c in new[part]]
            finally:
                O._LIB = base_lib
        base = {"btwn": outputs(sos[0], "btwn"), "merge": outputs(sos[1], "merge"), "trim": outputs(sos[1], "trim")}
        print("older inputs: %d reads -> %s calls; crafted cases: %s" % (n_old_reads, ", ".join("%s %d" % (p, len(oldp[p])) for p in kinds),
                                                                         "btwn %d chains, merge %d chains, trim %d anchor lists (the trim mutants run the merge chains as well)" % (len(new["btwn"]), len(new["merge"]), n_lists)))
        print("| part | mutant | older inputs changed | crafted cases changed | why nothing can change |")
        print("|---|---|---|---|---|")
        zero_old = zero_new = unexplained = 0
        for so, (part, name, _, _, _, why) in zip(sos[2:], muts):
            o, n = outputs(so, part)
            do = sum(x != y for x, y in zip(o, base[part][0])); dn = sum(x != y for x, y in zip(n, base[part][1]))
            zero_old += do == 0; zero_new += dn == 0; unexplained += dn == 0 and not why
            print("| %s | %s | %d | %d | %s |" % (part, name, do, dn, why if dn == 0 else ""))
        print("%d mutants; %d change no older input; %d change no crafted case, %d of them unexplained" % (len(muts), zero_old, zero_new, unexplained))


if __name__ == "__main__":
    main()
