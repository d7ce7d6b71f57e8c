#!/usr/bin/env python
"""Golden vectors for tests/svcalls_ref.py from the REFERENCE's own scripts: call_assembly_SVs/ParseAlignment.py (needs pandas) and mergeSV.py, run on
crafted inputs.  Writes tests/golden/svcalls_scripts_golden.json -- the inputs and what the scripts print; none of their text.

    python tools/make_golden_svcalls.py [REFERENCE_CHECKOUT]          (default: $REF, else /root/reference, as oracle/Makefile)

parse cases: SAM lines of eleven columns each (pandas refuses ragged rows), POS 1-based, TLEN in column 9; the expected value is the 0-based indices of
the lines the script keeps.  merge cases: rows (chrom, start, end) in NR order; the twelfth column mergeSV.py reads -- the IDs bedtools groupby collects
for a row, that is every row the snakefile's awk test relates it to, itself included -- is computed here by svcalls_ref.related, stored with the case
and pinned by the test; the expected value is the IDs the script prints."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svcalls_ref as sr                                                          # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF", "/root/reference")
SCRIPTS = os.path.join(REF, "call_assembly_SVs")
rng = np.random.default_rng(20261021)

# ---- ParseAlignment.py: (chrom, POS 1-based, TLEN) per line ------------------------------------------------------------------------------------------------
parse_cases = {
    "issue_example": [("c1", 101, 500), ("c1", 151, 300), ("c1", 201, 400), ("c1", 251, 351), ("c1", 701, 10),
                      ("c2", 6, 10), ("c2", 6, 10), ("c2", 7, 8), ("c2", 7, 20)],
    "equal_ends": [("c1", 1, 100), ("c1", 51, 50), ("c1", 100, 1), ("c1", 101, 0), ("c1", 101, 0)],           # every end is 101
    "one_record": [("c1", 5, 7)],
    "first_of_a_run": [("c1", 1, 1000), ("c2", 1, 10), ("c3", 1, 5), ("c3", 1, 5), ("c1", 2, 3)],
    "reference_change": [("c1", 1, 1000), ("c1", 10, 10), ("c2", 10, 10), ("c2", 11, 9), ("c2", 11, 10), ("c1", 10, 10)],
    "dropped_does_not_lower": [("c1", 1, 100), ("c1", 2, 10), ("c1", 3, 50), ("c1", 20, 81), ("c1", 20, 82), ("c1", 30, 72)],
    "negative_tlen": [("c1", 100, -50), ("c1", 100, -60), ("c1", 100, -40), ("c1", 101, 0), ("c1", 200, -200)],
    "large": [("c1", 2_000_000_000, 2_000_000_000), ("c1", 2_000_000_001, 1_999_999_999), ("c1", 2_000_000_001, 2_000_000_000)],
}
for k in range(12):
    n = int(rng.integers(2, 40))
    chrom = np.sort(rng.integers(1, 4, n))
    parse_cases["random%d" % k] = [("c%d" % c, int(p), int(t)) for c, p, t in zip(chrom, np.sort(rng.integers(1, 300, n)), rng.integers(-20, 200, n))]


def run_parse(lines):
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, "in.sam"), os.path.join(tmp, "out.sam")
        with open(a, "w") as f:
            for i, (c, p, t) in enumerate(lines):
                f.write("\t".join(["q%d" % i, "0", c, str(p), "60", "10M", "*", "0", str(t), "ACGTACGTAC", "*"]) + "\n")
        subprocess.run([sys.executable, os.path.join(SCRIPTS, "ParseAlignment.py"), "--inputsam", a, "--parsedsam", b], check=True, capture_output=True)
        return [int(ln.split("\t")[0][1:]) for ln in open(b)]


# ---- mergeSV.py: (chrom, start, end) per row, in NR order --------------------------------------------------------------------------------------------------
merge_cases = {
    "chain_A_B_C": [("c1", 0, 100), ("c1", 80, 180), ("c1", 160, 260)],           # A~B, B~C, not A~C: B goes, C stays
    "disjoint": [("c1", 0, 100), ("c1", 50, 150), ("c1", 1000, 1100)],
    "one_way_kept": [("c1", 90, 140), ("c1", 0, 100)],                            # ov 10: 10 ov == len of the second row: not related this way round
    "one_way_dropped": [("c1", 0, 100), ("c1", 90, 140)],                         # 10 ov == len of the first row: related
    "touching": [("c1", 0, 50), ("c1", 50, 100)],
    "nr_not_start_order": [("c1", 500, 600), ("c1", 100, 200), ("c1", 520, 620), ("c1", 110, 210), ("c1", 0, 50)],
    "two_references": [("c1", 0, 100), ("c2", 0, 100), ("c1", 10, 110), ("c2", 500, 600)],
    "all_related": [("c1", 10 * k, 1000 + 10 * k) for k in range(9)],
    "long_chain": [("c1", 80 * k, 80 * k + 100) for k in range(21)],
}
for k in range(12):
    n = int(rng.integers(2, 30))
    st = rng.integers(0, 400, n)
    merge_cases["random%d" % k] = [("c%d" % c, int(s), int(s + w)) for c, s, w in zip(rng.integers(1, 3, n), st, rng.integers(1, 120, n))]


def intersect_column(rows):
    ids = ["aligner.DEL.maternal.%d" % (i + 1) for i in range(len(rows))]
    return ids, [",".join(ids[j] for j, b in enumerate(rows) if b[0] == a[0] and sr.related(a[1:], b[1:])) for a in rows]


def run_merge(rows):
    ids, col = intersect_column(rows)
    text = "".join("\t".join([c, str(s), str(e), ident, "A", "AC", "60", "PASS", "SVTYPE=X", "GT", "1/1", x]) + "\n" for (c, s, e), ident, x in zip(rows, ids, col))
    out = subprocess.run([sys.executable, os.path.join(SCRIPTS, "mergeSV.py")], input=text, capture_output=True, text=True, check=True).stdout
    return col, [int(ln.split("\t")[3].rsplit(".", 1)[1]) - 1 for ln in out.splitlines()]


gold = {"source": "call_assembly_SVs/ParseAlignment.py and mergeSV.py of the reference, run by tools/make_golden_svcalls.py", "parse": [], "merge": []}
for name, lines in parse_cases.items():
    gold["parse"].append({"name": name, "lines": [list(x) for x in lines], "kept": run_parse(lines)})
for name, rows in merge_cases.items():
    col, kept = run_merge(rows)
    gold["merge"].append({"name": name, "rows": [list(x) for x in rows], "intersect": col, "kept": kept})
with open(os.path.join(ROOT, "tests", "golden", "svcalls_scripts_golden.json"), "w") as f:
    json.dump(gold, f, indent=0)
print(len(gold["parse"]), "parse cases,", len(gold["merge"]), "merge cases")
