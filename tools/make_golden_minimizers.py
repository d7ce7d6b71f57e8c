"""Golden vectors for StoreMinimizers' window logic (MinCount.h:8-179): runs oracle/_ref/minimizers_ref (the reference's own StoreMinimizers<GenomeTuple, Tuple>
compiled in place) on the crafted reads of tests/seed_cases.py -- every other read of every (k, w) pair's batch, which keeps all families -- and writes the emitted
positions -> tests/golden/minimizers_golden.json.  The key at a position is the canonical key tuple_ops_golden.json already pins; the tool checks that every
emitted key is that key before it drops it."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seed_cases  # noqa: E402


def golden_cases():
    """(k, w, family, read) of every golden case, in file order."""
    cases = []
    for k, w in seed_cases.KW:
        reads = seed_cases.a1_reads(k, w)
        by_family = {}
        for fam, r in reads:
            by_family.setdefault(fam, []).append(r)
        for fam in sorted(by_family):
            for r in by_family[fam][::2]:
                cases.append((k, w, fam, r))
    return cases


def main():
    cases = golden_cases()
    exe = os.path.join(ROOT, "oracle", "_ref", "minimizers_ref")
    text = "".join("%d %d %s\n" % (k, w, seed_cases.to_text(r)) for k, w, _f, r in cases)
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
    gold = []
    n_tuples = 0
    for (k, w, fam, r), line in zip(cases, out):
        f = line.split()
        n = int(f[0])
        assert len(f) == 1 + 2 * n
        t = np.array(f[1::2], dtype=np.uint64); pos = [int(x) for x in f[2::2]]
        ck, cr = seed_cases.keys_of(r, k)
        for ti, p in zip(t, pos):
            assert int(ti) == int(ck[p]) | (int(cr[p]) << 63), (k, w, p)
        gold.append(dict(k=k, w=w, family=fam, seq=seed_cases.to_text(r), pos=pos))
        n_tuples += n
    path = os.path.join(ROOT, "tests", "golden", "minimizers_golden.json")
    with open(path, "w") as fh:
        json.dump(dict(source="MinCount.h:8-179 StoreMinimizers<GenomeTuple, Tuple>(Global = true) through oracle/ref_harness/minimizers_ref.cpp; "
                              "seq: '0'..'7' stand for the bytes 0..7", cases=gold), fh, separators=(",", ":"))
    print(len(gold), "cases,", n_tuples, "tuples,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
