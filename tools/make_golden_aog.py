"""Generate tests/golden/aog_golden.json by running the REFERENCE's AffineOneGapAlign
(oracle/_ref/aog_ref, compiled from /root/reference) in this container.

Inputs: (i) the 22 query/target pairs the reference's own TestAffineOneGapAlign.cpp:19-68
holds (string literals = test data), with its parameters (4,-4,-3,15) and with the
preset parameter sets the live path uses; (ii) seeded random pairs covering equal
lengths, long one-sided gaps (the "alignTop" branch), length 0/1 and N bases.
Only inputs + the reference's outputs are stored (no reference source).

A second file, tests/golden/aog_golden_wide.json, holds bands the first one stops short of:
k in {31, 32, 33, 50, 60, 63, 64, 100, 127, 128} (the -CONTIG preset refines with k = 50), lengths up to ~400,
the same four scoring sets; prefix-only and long-gap ("alignTop") pairs in both orientations, unrelated pairs, N and
lower-case bases, empty strings.  The reference reads outside its matrices or never returns on some inputs: a case goes
to the reference binary only if the oracle (oracle/aog.cpp) reports status 0 for it, and the number dropped is stored
in the file ("n_dropped_oracle_status").
"""
import json, os, re, random, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_TEST = "/root/reference/TestAffineOneGapAlign.cpp"
BIN = os.path.join(ROOT, "oracle", "_ref", "aog_ref")


def reference_test_pairs():
    src = open(REF_TEST).read()
    src = src.split("/*\n\tstring target")[0]
    pairs = []
    for mobj in re.finditer(r'Test\(\s*"([A-Za-z]*)"\s*,\s*"([A-Za-z]*)"\s*\)', src):
        pairs.append((mobj.group(1), mobj.group(2)))
    return pairs


def mutate(rng, s, sub, ins, dele):
    out = []
    for c in s:
        r = rng.random()
        if r < sub:
            out.append(rng.choice("ACGT"))
        elif r < sub + ins:
            out.append(c); out.append(rng.choice("ACGT"))
        elif r < sub + ins + dele:
            continue
        else:
            out.append(c)
    return "".join(out)


def random_pairs(seed=7, n=260):
    rng = random.Random(seed)
    cases = []
    for x in range(n):
        L = rng.choice([0, 1, 2, 3, 5, 8, 9, 12, 20, 31, 47, 62, 90, 150, 300, 640])
        s = "".join(rng.choice("ACGT") for _ in range(L))
        mode = x % 5
        if mode == 0:
            q, t = s, mutate(rng, s, 0.05, 0.03, 0.03)
        elif mode == 1:   # long insertion in q
            g = "".join(rng.choice("ACGT") for _ in range(rng.choice([40, 90, 200, 500])))
            p = rng.randint(0, L)
            q, t = s[:p] + g + s[p:], mutate(rng, s, 0.03, 0.02, 0.02)
        elif mode == 2:   # long insertion in t
            g = "".join(rng.choice("ACGT") for _ in range(rng.choice([40, 90, 200, 500])))
            p = rng.randint(0, L)
            q, t = mutate(rng, s, 0.03, 0.02, 0.02), s[:p] + g + s[p:]
        elif mode == 3:   # unrelated
            q = s
            t = "".join(rng.choice("ACGT") for _ in range(rng.choice([0, 1, 4, 17, 33, 80])))
        else:             # with N / lowercase
            q = mutate(rng, s, 0.1, 0.05, 0.05).replace("A", "N", 1)
            t = s.lower() if x % 2 else s
        k = rng.choice([1, 2, 3, 5, 7, 15, 30])
        par = rng.choice([(4, -3, -4), (4, -1, -2), (4, -4, -3), (1, -1, -1)])
        cases.append((q, t, par[0], par[1], par[2], k))
    return cases


WIDE_K = [31, 32, 33, 50, 60, 63, 64, 100, 127, 128]
PARS = [(4, -3, -4), (4, -1, -2), (4, -4, -3), (1, -1, -1)]


def wide_pairs(seed=11, n=400):
    rng = random.Random(seed)
    rnd = lambda L: "".join(rng.choice("ACGT") for _ in range(L))
    cases = []
    for x in range(n):
        k = WIDE_K[x % len(WIDE_K)]
        par = PARS[(x // len(WIDE_K)) % len(PARS)]
        mode = (x // (len(WIDE_K) * len(PARS))) % 10
        L = rng.choice([k - 1, k, k + 1, 2 * k, 2 * k + 1, 40, 97, 150, 230, 320, 400])
        L = max(1, min(L, 400))
        s = rnd(L)
        if mode in (0, 1):        # prefix band only: the lengths differ by less than the band
            q, t = s, mutate(rng, s, 0.05, 0.03, 0.03)
        elif mode in (2, 3):      # long gap ("alignTop"): one side carries an insertion longer than diag + 2k allows
            g = rnd(2 * k + rng.choice([1, 2, 17, 60]) + max(0, L - 400 // 3))
            g = g[:max(2 * k + 1, 400 - L)] if L + len(g) > 400 + 2 * k else g
            p_ = rng.randint(0, L)
            q, t = s[:p_] + g + s[p_:], mutate(rng, s, 0.03, 0.02, 0.02)
        elif mode in (4, 5):      # unrelated
            q, t = s, rnd(rng.choice([1, 4, 17, 33, 80, k, 2 * k, 3 * k + 5, L]))
        elif mode in (6, 7):      # N / lower case
            q = mutate(rng, s, 0.1, 0.05, 0.05).replace("A", "N", 2)
            t = s.lower() if x % 2 else s.replace("C", "n", 1)
        elif mode == 8:           # a short stretch against a long one, and the band's own length
            q, t = s[:rng.choice([1, 2, 3, k // 2])], s
        else:                     # empty strings
            q, t = "", (s if x % 3 else "")
        if (mode % 2) if mode < 8 else ((x % 10 + x // 10) % 2):   # both orientations: of modes 0 - 7 by the mode, within modes 8 and 9 case by case
            q, t = t, q
        cases.append((q, t, par[0], par[1], par[2], k))
    return cases


def run_reference(cases):
    inp = "".join("%s %s %d %d %d %d\n" % (q or "-", t or "-", m, mm, indel, k) for q, t, m, mm, indel, k in cases)
    out = subprocess.run([BIN], input=inp.encode(), stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode().splitlines()
    assert len(out) == len(cases)
    recs = []
    for c, line in zip(cases, out):
        v = [int(x) for x in line.split()]
        assert len(v) == 2 + 3 * v[1]
        recs.append({"q": c[0], "t": c[1], "m": c[2], "mm": c[3], "indel": c[4], "k": c[5], "score": v[0], "blocks": v[2:]})
    return recs


def main_wide():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    cases = wide_pairs()
    kept = [c for c in cases if oracle_lib.affine_one_gap_align(c[0].encode(), c[1].encode(), c[2], c[3], c[4], c[5])[2] == 0]
    recs = run_reference(kept)
    path = os.path.join(ROOT, "tests", "golden", "aog_golden_wide.json")
    json.dump({"source": "oracle/_ref/aog_ref (reference AffineOneGapAlign.h compiled in place)", "k": WIDE_K,
               "n_generated": len(cases), "n_dropped_oracle_status": len(cases) - len(kept), "cases": recs}, open(path, "w"))
    print("wrote", path, len(recs), "cases (", len(cases) - len(kept), "of", len(cases), "dropped: oracle status != 0 )")


def main():
    cases = []
    for q, t in reference_test_pairs():
        for (m, mm, indel, k) in [(4, -4, -3, 15), (4, -3, -4, 15), (4, -1, -2, 30), (4, -3, -4, 7)]:
            cases.append((q, t, m, mm, indel, k))
    n_ref = len(cases)
    cases += random_pairs()
    inp = "".join("%s %s %d %d %d %d\n" % (q or "-", t or "-", m, mm, indel, k) for q, t, m, mm, indel, k in cases)
    out = subprocess.run([BIN], input=inp.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(cases)
    recs = []
    for c, line in zip(cases, out):
        v = [int(x) for x in line.split()]
        assert len(v) == 2 + 3 * v[1]
        recs.append({"q": c[0], "t": c[1], "m": c[2], "mm": c[3], "indel": c[4], "k": c[5], "score": v[0], "blocks": v[2:]})
    path = os.path.join(ROOT, "tests", "golden", "aog_golden.json")
    json.dump({"source": "oracle/_ref/aog_ref (reference AffineOneGapAlign.h compiled in place)",
               "n_from_reference_test_inputs": n_ref, "cases": recs}, open(path, "w"))
    print("wrote", path, len(recs), "cases (", n_ref, "from TestAffineOneGapAlign.cpp inputs )")


if __name__ == "__main__":
    main()
    main_wide()
