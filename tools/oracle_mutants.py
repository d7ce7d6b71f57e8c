#!/usr/bin/env python3
"""What the chain-walk test inputs can tell apart, measured on the CPU: one comparison or constant of oracle/chain_split.cpp is changed at a time in a temporary
copy, the copy is compiled alone to a shared object, and both the random inputs of the older GPU tests (tests/test_chain_split.py, test_hip_split_chains_highacc_oracle:
same seeds, op sets and splitdist) and the crafted cases of tests/chain_cases.py are run through it.  Printed per mutant: the number of cases whose expected output
changes.  A mutant that changes no case is one chain_split.hip could carry while every test passes.  CPU only; not part of the suite (it compiles some 70 times).

    python tools/oracle_mutants.py [--jobs N] [--only SUBSTRING]"""
import argparse
import concurrent.futures as cf
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SRC = os.path.join(ROOT, "oracle", "chain_split.cpp")

LT100 = "if (ch[i].len < 100) remove[i] = true;"
LT50 = "if (ch[i].len < 50) remove[i] = true;"
T_UP = "tS(cur) > tE(prev) + (uint32_t)splitdist"
T_DOWN = "tE(cur) + (uint32_t)splitdist < tS(prev)"
H_T = "    if (tS(cur) > tE(prev) + (uint32_t)splitdist || tE(cur) + (uint32_t)splitdist < tS(prev) || chrom[cur] != chrom[prev]) cut('T');\n    else if (rep_map) cut('D');"
H_D_FIRST = "    if (rep_map) cut('D');\n    else if (tS(cur) > tE(prev) + (uint32_t)splitdist || tE(cur) + (uint32_t)splitdist < tS(prev) || chrom[cur] != chrom[prev]) cut('T');"

# (part, name, old text, new text, which occurrence (None: all), listed: one of the mutants no older input notices)
MUTANTS = [
    ("filters", "op 1 len <= 50 -> <", "if (ch[i].len <= 50) remove", "if (ch[i].len < 50) remove", None, True),
    ("filters", "op 8 len < 50 -> <=", LT50, LT50.replace("< 50", "<= 50"), 1, True),
    ("filters", "op 2/3 both >= 300 -> >", "std::abs(SV[c]) >= 300 && std::abs(SV[c - 1]) >= 300", "std::abs(SV[c]) > 300 && std::abs(SV[c - 1]) > 300", None, True),
    ("filters", "op 2 firstValid < 3 -> < 2", "firstValid < 3", "firstValid < 2", None, True),
    ("filters", "op 2 qDist = qS(c) - tE(c-1) -> - qE(c-1)", "qDist = qS(c) - tE(c - 1)", "qDist = qS(c) - qE(c - 1)", None, True),
    ("filters", "op 4 >= 500 -> >", "std::abs(Gap) >= 500", "std::abs(Gap) > 500", None, True),
    ("filters", "op 4 <= 10 -> <", "SVpos[c] - SVpos[c - 1] <= 10", "SVpos[c] - SVpos[c - 1] < 10", None, True),
    ("filters", "op 4 len >= 50 -> >", "if (ch[b].len >= 50)", "if (ch[b].len > 50)", None, True),
    ("filters", "op 5 < 600 -> <=", "std::abs(SV[c] + SV[c - 1]) < 600", "std::abs(SV[c] + SV[c - 1]) <= 600", None, True),
    ("filters", "op 5 max(2*blink, 1000) -> 1001", "std::max(2 * blink, 1000)", "std::max(2 * blink, 1001)", None, True),
    ("filters", "op 5 2*blink -> 2*blink+1", "std::max(2 * blink, 1000)", "std::max(2 * blink + 1, 1000)", None, True),
    ("filters", "op 5 < 500 -> <=", "< 500)", "<= 500)", None, True),
    ("split_kernel", "jump len < 50 -> <=", LT50, LT50.replace("< 50", "<= 50"), 0, True),
    ("split_kernel", "dist >= 1000 -> >", "dist >= 1000", "dist > 1000", None, True),
    ("split_kernel", "ceil(0.15*dist) -> floor", "std::ceil(0.15 * dist)", "std::floor(0.15 * dist)", None, True),
    ("split_kernel", "tS(cur) > tE(prev)+splitdist -> >=", T_UP, T_UP.replace(">", ">="), 0, True),
    ("split_kernel", "tE(cur)+splitdist < tS(prev) -> <=", T_DOWN, T_DOWN.replace("<", "<="), 0, True),
    ("split_kernel", "merge tdist > 1500 -> >=", "if (tdist > 1500) { nn++; continue; }", "if (tdist >= 1500) { nn++; continue; }", None, True),
    ("split_kernel", "merge ignoring chromIndex", "if (sp[c].chromIndex != sp[nn].chromIndex) { nn++; continue; }", "", None, True),
    ("split_kernel", "CHROMIndex TStart + 1 -> TStart", "(uint64_t)s.TStart + 1", "(uint64_t)s.TStart", None, True),
    ("hsplit_kernel", "overlap >= 0.6 -> > (prev on cur)", "ovl(prev, cur) >= 0.6", "ovl(prev, cur) > 0.6", None, True),
    ("hsplit_kernel", "overlap >= 0.6 -> > (cur on prev)", "ovl(cur, prev) >= 0.6", "ovl(cur, prev) > 0.6", None, True),
    ("hsplit_kernel", "T cut tS(cur) > tE(prev)+splitdist -> >=", T_UP, T_UP.replace(">", ">="), 1, True),
    ("hsplit_kernel", "T cut tE(cur)+splitdist < tS(prev) -> <=", T_DOWN, T_DOWN.replace("<", "<="), 1, True),
    ("hsplit_kernel", "merge tdist > 1500 -> >=", "if (tdist > 1500 || sp[c].Strand", "if (tdist >= 1500 || sp[c].Strand", None, True),
    ("hsplit_kernel", "LSC d > maxi_d -> >=", "if (d > maxi_d)", "if (d >= maxi_d)", None, True),
    ("hsplit_kernel", "D tested before T", H_T, H_D_FIRST, None, True),
    # caught by a handful of the older inputs
    ("filters", "op 8 > 100 -> >=", ": (std::abs(Gap) > 100);", ": (std::abs(Gap) >= 100);", None, False),
    ("filters", "op 2/3 link resized when nothing survives", "{ if (m > 0) lk.resize(m - 1); }", "{ lk.resize(m > 0 ? m - 1 : 0); }", None, False),
    ("split_kernel", "merge ignoring strand", "if (sp[c].Strand != sp[nn].Strand) { nn++; continue; }", "", None, False),
    ("split_kernel", "reverse-strand diag qE + t -> qS + t", "ch[i].strand == 1 ? (long)qE(i) + (long)tS(i)", "ch[i].strand == 1 ? (long)qS(i) + (long)tS(i)", None, False),
    ("split_kernel", "min(filterDI, 4) -> 2", "std::min(filterDI, 4)", "std::min(filterDI, 2)", None, False),
    # the rest of the comparisons
    ("filters", "op 1 |gap| > 5 -> >=", "std::abs(Gap) > 5 ", "std::abs(Gap) >= 5 ", None, False),
    ("filters", "op 1 |gap| <= 50 -> <", "std::abs(Gap) <= 50)", "std::abs(Gap) < 50)", None, False),
    ("filters", "op 1 |sum| <= 20 -> <", "std::abs(SV[c] + SV[c - 1]) <= 20", "std::abs(SV[c] + SV[c - 1]) < 20", None, False),
    ("filters", "op 1 distance < 3 -> <=", "SVpos[c] - SVpos[c - 1] < 3", "SVpos[c] - SVpos[c - 1] <= 3", 0, False),
    ("filters", "op 8 distance == 1 -> <= 2", "SVpos[c] - SVpos[c - 1] == 1", "SVpos[c] - SVpos[c - 1] <= 2", 1, False),
    ("filters", "op 8 without the rm[pPos] == 0 clause", "} else if (remove[SVpos[c - 1]] == 0 && sgn", "} else if (sgn", None, False),
    ("filters", "op 2/3 |gap| > 30 -> >=", "std::abs(Gap) > 30", "std::abs(Gap) >= 30", 0, False),
    ("filters", "op 2/3 |sum| < 100 -> <=", "std::abs(SV[c] + SV[c - 1]) < 100", "std::abs(SV[c] + SV[c - 1]) <= 100", None, False),
    ("filters", "op 2/3 distance < 3 -> <= (300 rule)", "SVpos[c] - SVpos[c - 1] < 3", "SVpos[c] - SVpos[c - 1] <= 3", 1, False),
    ("filters", "op 2/3 distance < 3 -> <= (sum rule)", "SVpos[c] - SVpos[c - 1] < 3", "SVpos[c] - SVpos[c - 1] <= 3", 2, False),
    ("filters", "op 2/3 len < 100 -> <= (300 rule)", LT100, LT100.replace("< 100", "<= 100"), 0, False),
    ("filters", "op 2/3 len < 100 -> <= (sum rule)", LT100, LT100.replace("< 100", "<= 100"), 1, False),
    ("filters", "op 2 len < 100 -> <= (nothing valid)", LT100, LT100.replace("< 100", "<= 100"), 2, False),
    ("filters", "op 2 len < 100 -> <= (front end)", LT100, LT100.replace("< 100", "<= 100"), 3, False),
    ("filters", "op 2 len < 100 -> <= (back end)", LT100, LT100.replace("< 100", "<= 100"), 4, False),
    ("filters", "op 2 dist < mean + 4 sd -> <=", "if (dist < meanDist + 4 * sdDist)", "if (dist <= meanDist + 4 * sdDist)", None, False),
    ("filters", "op 2 4 sd -> 3 sd", "meanDist + 4 * sdDist", "meanDist + 3 * sdDist", None, False),
    ("filters", "op 2 N - lastValid < 3 -> < 2", "N - lastValid < 3", "N - lastValid < 2", None, False),
    ("filters", "op 2 squared sum without the 64-bit wrap", "const long totDistSq = (long)totDistSqU;", "const double totDistSq = (double)totDistSqU;", None, False),
    ("filters", "op 4 without the SV != 0 test", "if (SV[c] != 0 && SV[c - 1] != 0 && SVpos[c] - SVpos[c - 1] <= 10)", "if (SVpos[c] - SVpos[c - 1] <= 10)", None, False),
    ("filters", "op 4 removal len < 50 -> <=", LT50, LT50.replace("< 50", "<= 50"), 2, False),
    ("filters", "op 4 compacts link", "touchLink = false;", "touchLink = true;", 1, False),
    ("filters", "op 5 compacts link", "touchLink = false;", "touchLink = true;", 0, False),
    ("filters", "op 5 |gap| > 30 -> >=", "std::abs(Gap) > 30", "std::abs(Gap) >= 30", 1, False),
    ("filters", "op 5 gap by strand", "      for (int c = 1; c < N; c++) {\n        int Gap = (int)(((long)tS(c) - (long)qS(c)) - ((long)tS(c - 1) - (long)qS(c - 1)));",
     "      for (int c = 1; c < N; c++) {\n        int Gap = ch[c].strand == ch[c - 1].strand ? gap_of(c) : 0;", None, False),
    ("filters", "op 5 len < 100 -> <= (first branch)", LT100, LT100.replace("< 100", "<= 100"), 5, False),
    ("filters", "op 5 len < 100 -> <= (500 branch)", LT100, LT100.replace("< 100", "<= 100"), 6, False),
    ("filters", "op 5 len < 100 -> <= (same-sign branch)", LT100, LT100.replace("< 100", "<= 100"), 7, False),
    ("filters", "qEnd always q + len", "return qend ? qend[ch[i].orig] : ch[i].q", "return false ? qend[ch[i].orig] : ch[i].q", None, False),
    ("split_kernel", "jump |gap| > 100 -> >=", "if (std::abs(Gap) > 100) {", "if (std::abs(Gap) >= 100) {", None, False),
    ("split_kernel", "jump distance == 1 -> <= 2", "SVpos[c] - SVpos[c - 1] == 1", "SVpos[c] - SVpos[c - 1] <= 2", 0, False),
    ("split_kernel", "jump without the remove[] == 0 clause", "      if (remove[SVpos[c - 1]] == 0 && sgn", "      if (sgn", 0, False),
    ("split_kernel", "|diag difference| <= -> <", "<= std::ceil(0.15 * dist)", "< std::ceil(0.15 * dist)", None, False),
    ("split_kernel", "I cut with split_link 0", "sp.back().type = 'I'; spl.push_back(1);", "sp.back().type = 'I'; spl.push_back(0);", None, False),
    ("split_kernel", "link across a merge 0 -> 1", "if (s == t1) sp[c].link[s - 1] = 0;", "if (s == t1) sp[c].link[s - 1] = 1;", None, False),
    ("split_kernel", "split_link rewritten without bypass", "if (bypass) for (size_t k = 1;", "if (true) for (size_t k = 1;", None, False),
    ("split_kernel", "ClusterIndex merged without bypass", "        if (bypass) {\n          int pv", "        if (true) {\n          int pv", None, False),
    ("split_kernel", "piece size < min(filter, 2) -> <=", "(int)sp[i].sptc.size() < std::min(filter, 2)", "(int)sp[i].sptc.size() <= std::min(filter, 2)", None, False),
    ("split_kernel", "size filter behind every link", "if (spl[i - 1] == 1 && (int)sp[i]", "if ((int)sp[i]", None, False),
    ("split_kernel", "split_link moved for slot 1 too (c > 1 -> c > 0)", "if (c > 1) spl[c - 1] = spl[i - 1];", "if (c > 0 && i > 0) spl[c - 1] = spl[i - 1];", None, False),
    ("split_kernel", "filterDI 0.03 -> 0.02", "std::floor(0.03f * (float)total)", "std::floor(0.02f * (float)total)", None, False),
    ("split_kernel", "filter 0.02 -> 0.5 (dead: min(filter, 2) is 2)", "std::floor(0.02f * (float)total)", "std::floor(0.5f * (float)total)", None, False),
    ("hsplit_kernel", "D on link 0 for forward pairs", "(link[im] == 1 && strand[cur] == 0", "(link[im] == 0 && strand[cur] == 0", None, False),
    ("hsplit_kernel", "D on link 1 for reverse pairs", "(link[im] == 0 && strand[cur] == 1", "(link[im] == 1 && strand[cur] == 1", None, False),
    ("hsplit_kernel", "T without the chromosome test", " || chrom[cur] != chrom[prev]) cut('T');", ") cut('T');", None, False),
    ("hsplit_kernel", "merge ignoring chromIndex", "if (tdist > 1500 || sp[c].Strand != sp[nn].Strand || sp[c].chromIndex != sp[nn].chromIndex)", "if (tdist > 1500 || sp[c].Strand != sp[nn].Strand)", None, False),
]


def mutate(text, old, new, which):
    n = text.count(old)
    if n == 0 or (which is not None and which >= n):
        raise SystemExit("mutant text not found (%d of %d): %r" % (which or 0, n, old))
    if which is None:
        return text.replace(old, new)
    pos = -1
    for _ in range(which + 1):
        pos = text.index(old, pos + 1)
    return text[:pos] + new + text[pos + len(old):]


def compile_one(args):
    tmp, k, text = args
    cpp = os.path.join(tmp, "m%03d.cpp" % k); so = os.path.join(tmp, "m%03d.so" % k)
    with open(cpp, "w") as f:
        f.write(text)
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-w", "-shared", "-I", os.path.join(ROOT, "oracle"), "-o", so, cpp], check=True)
    return so


def old_inputs():
    """the inputs of test_hip_split_chains_oracle, test_hip_filter_chains_oracle and test_hip_split_chains_highacc_oracle as chain_cases cases"""
    import chain_cases as cc
    import test_chain_split as tcs
    import test_highacc_path as thp
    out = {"split_kernel": [], "filters": [], "hsplit_kernel": []}
    rng = np.random.default_rng(3)
    chains = [tcs._random_chain(rng, int(rng.integers(1, 120)), kind=k % 4) for k in range(400)]
    for splitdist, bypass in ((50000, 1), (50000, 0)):
        for c in chains:
            out["split_kernel"].append(cc.scase(dict(q=c[0], t=c[1], len=c[2], strand=c[3], cluster=c[4], link=c[5]), splitdist, bypass, tcs.CHROM))
    rng = np.random.default_rng(12)
    chains = [tcs._indel_chain(rng, int(rng.integers(1, 90))) for _ in range(300)]
    off = np.cumsum([0] + [len(c[0]) for c in chains])
    cat = lambda j: np.concatenate([c[j] for c in chains]).astype(np.int64)
    qend = cat(0) + cat(2) + np.where(rng.random(int(off[-1])) < 0.3, rng.integers(0, 300, int(off[-1])), 0)
    for ops, with_link, ex in (([2, 4], True, False), ([1, 2, 4], False, False), ([1, 3, 4], True, False), ([8], True, False), ([4, 8, 1], True, False), ([2], True, False),
                               ([5], False, False), ([5, 4], True, False), ([1, 3, 4], False, True), ([1, 2, 4], True, True)):
        for i, c in enumerate(chains):
            out["filters"].append(cc.fcase(dict(q=c[0], t=c[1], len=c[2], strand=c[3], link=c[4], qend=qend[int(off[i]):int(off[i + 1])].astype(np.uint32)), ops, with_link, ex))
    rng = np.random.default_rng(23)
    for strand, chrom, box, link in thp._random_cluster_chains(rng, 400):
        out["hsplit_kernel"].append(cc.hcase(strand, chrom, box, link, 100000))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", default=None, help="run only the mutants whose name contains this")
    a = ap.parse_args()
    import chain_cases as cc
    import oracle_lib as O
    kind = {"filters": "filter", "split_kernel": "split", "hsplit_kernel": "hsplit"}
    old = old_inputs()
    new = {p: [c for _, c in cc.all_cases() if c["kind"] == kind[p]] for p in kind}
    muts = [m for m in MUTANTS if a.only is None or a.only in m[1]]
    text = open(SRC).read()
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(tmp, 0, text)] + [(tmp, k + 1, mutate(text, m[2], m[3], m[4])) for k, m in enumerate(muts)]
        with cf.ThreadPoolExecutor(a.jobs) as ex:
            sos = list(ex.map(compile_one, jobs))

        def outputs(so, part):
            O._LIB = C.CDLL(so)
            return [cc.run(c) for c in old[part]], [cc.run(c) for c in new[part]]
        base = {p: outputs(sos[0], p) for p in kind}
        print("old inputs: %s; crafted cases: %s" % (", ".join("%s %d" % (p, len(old[p])) for p in kind), ", ".join("%s %d" % (p, len(new[p])) for p in kind)))
        print("| part | mutant | listed as unnoticed | old inputs changed | crafted cases changed |")
        print("|---|---|---|---|---|")
        zero_old = zero_new = 0
        for so, (part, name, _, _, _, listed) in zip(sos[1:], muts):
            o, n = outputs(so, part)
            do = sum(x != y for x, y in zip(o, base[part][0])); dn = sum(x != y for x, y in zip(n, base[part][1]))
            zero_old += do == 0; zero_new += dn == 0
            print("| %s | %s | %s | %d | %d |" % (part, name, "yes" if listed else "", do, dn))
        print("%d mutants; %d change no old input; %d change no crafted case" % (len(muts), zero_old, zero_new))
        O._LIB = None


if __name__ == "__main__":
    main()
