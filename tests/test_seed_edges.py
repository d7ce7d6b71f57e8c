"""Seeding at crafted edges: the windowed sketch (a1), the index walk (a3) and the strand split (a4) of lra_seed_batch against the stage oracles, on the reads
and indexes of seed_cases.py.  The oracles are pinned to the reference's own code (tests/test_seed.py: minimizers_golden.json, comparelists_golden.json).

What each family contributes is counted from the oracle alone and asserted (test_*_cover_their_families, CPU), so a later change to a generator cannot quietly
empty a family."""
import numpy as np
import pytest

import seed_cases as S
from lra_amd import synth

M63 = S.M63


# ---------------------------------------------------------------------------------------------------------------- shared plumbing
def _run(ctx, genome, ik, ip, reads, k, w, max_freq):
    from lra_amd import seed
    seed.load_reference(ctx, genome, ik, ip)
    batch = seed.ReadBatch(ctx, reads)
    return seed.fetch(ctx, seed.seed_batch(ctx, batch, k, w, max_freq))


def _expect(oracle, read, sk, sp, gbytes, ik, ip, k, max_freq):
    """The oracle's a3 + a4 of one read whose sorted minimizers are (sk, sp): match lists in discovery order, the forward count, the separated positions."""
    qi, ti = oracle.compare_lists(sk, sp, ik, ip, max_freq)
    strand = oracle.separate_strand(read, gbytes, k, sp[qi], ip[ti])
    eq, et = sp[qi], ip[ti]
    return dict(qi=qi, ti=ti, nf=int((strand == 0).sum()), sq=np.concatenate([eq[strand == 0], eq[strand == 1]]),
                st=np.concatenate([et[strand == 0], et[strand == 1]]), strand=strand)


def _cat(parts, dtype):
    parts = [np.asarray(p, dtype=dtype) for p in parts]
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


def _first_bad(off, got, exp):
    """The first read whose slice differs (for the assertion message)."""
    n = min(len(got), len(exp))
    d = np.nonzero(got[:n] != exp[:n])[0]
    at = int(d[0]) if len(d) else n
    return int(np.searchsorted(off, at, side="right") - 1)


def _check_minimizers(out, mins):
    """mins: per read of the batch its expected sorted (keys, positions)."""
    off = np.zeros(len(mins) + 1, np.uint64); off[1:] = np.cumsum([len(m[0]) for m in mins])
    assert np.array_equal(out["mm_off"], off), _first_bad(np.arange(len(off)), out["mm_off"], off) - 1
    ek, ep = _cat([m[0] for m in mins], np.uint64), _cat([m[1] for m in mins], np.uint32)
    assert np.array_equal(out["mm_key"], ek), ("mm_key, read", _first_bad(off, out["mm_key"], ek))
    assert np.array_equal(out["mm_pos"], ep), ("mm_pos, read", _first_bad(off, out["mm_pos"], ep))


def _check_matches(out, exps):
    """exps: per read of the batch its _expect()."""
    off = np.zeros(len(exps) + 1, np.uint64); off[1:] = np.cumsum([len(e["qi"]) for e in exps])
    assert np.array_equal(out["match_off"], off), ("match count, read", _first_bad(np.arange(len(off)), out["match_off"], off) - 1)
    for name, key, dt in (("match_qi", "qi", np.uint32), ("match_ti", "ti", np.uint32), ("sep_qpos", "sq", np.uint32), ("sep_tpos", "st", np.uint32)):
        e = _cat([x[key] for x in exps], dt)
        assert np.array_equal(out[name], e), (name, "read", _first_bad(off, out[name], e))
    nf = np.array([e["nf"] for e in exps], dtype=np.uint32)
    assert np.array_equal(out["n_forward"], nf), ("n_forward, read", int(np.nonzero(out["n_forward"] != nf)[0][0]))
    return int(off[-1])


# ---------------------------------------------------------------------------------------------------------------- B: a1 on crafted reads
_A1 = {}


def _a1_case(oracle, k, w):
    if (k, w) not in _A1:
        reads = S.a1_reads(k, w)
        mins = [S.sorted_minimizers(oracle, r, k, w) for _f, r in reads]
        _A1[(k, w)] = (reads, mins, S.a1_stats(oracle, k, w, reads))
    return _A1[(k, w)]


@pytest.mark.parametrize("k,w", S.KW)
def test_sketch_reads_cover_their_families(oracle, k, w):
    """Every family of section B occurs in the (k, w) batch, counted from the oracle and the pinned key function alone."""
    reads, _mins, st = _a1_case(oracle, k, w)
    span = w + k - 1
    lens = {len(r) for f, r in reads if f.startswith("len")}
    assert {0, span - 1, span, span + 1, 2 * w + k - 2, 2 * w + k - 1, 2 * w + k} <= lens
    assert {nk + k - 1 for nk in (63, 64, 65, 127, 128, 129, 193)} <= lens
    for alpha in (1, 2, 4):
        assert st["fam"]["len%d" % alpha][0] == 14
    assert st["tie_cross_tile"] >= 5          # runs of tied minima that cross a 64-position tile edge, beyond the literal replay
    assert st["n_emits"] >= 20                # reads with a non-ACGT byte that still emit (sketch_kernel<true> writes into sketch_compact's gaps)
    assert st["empty_out"] >= 8               # reads that emit nothing, clean and not
    assert st["last_window"] >= 1             # a clean window that starts exactly at L - span after an N: found by no search
    assert st["first_window"] >= 3            # the unmasked first-window comparison picked a forward key over a smaller reverse key
    assert st["fam"]["first_window"][0] >= 3
    if k % 2 == 0:
        assert st["palindrome"] >= 1          # an emitted k-mer that is its own reverse complement (the key carries the reverse flag)
    for fam in ("tie_period", "tie_homopolymer", "tie_recur", "n_one", "n_two", "n_all", "lower", "bytes0_7", "other_byte"):
        assert st["fam"][fam][0] >= 2, fam
    assert all(len(r) >= 300 for f, r in reads if f.startswith("tie"))
    assert st["fam"].get("tie_phase", [w - 1])[0] == w - 1 or w == 2
    # two equal minima in the window of a tile's last position, the older one active (what crosses the tile edge is the active position, not the ring choice)
    assert w == 2 or st["tile_end_tie"] >= 1
    # reads with an N, clean reads and reads without output alternate: the batch order changes kind at least 20 times
    kind = np.array([0 if S.is_clean(r) else 1 for _f, r in reads])
    assert (np.diff(kind) != 0).sum() >= 20
    assert (np.diff(np.array([len(m[0]) == 0 for m in _mins]).astype(int)) != 0).sum() >= 10


@pytest.mark.gpu
@pytest.mark.parametrize("k,w", S.KW)
def test_sketch_crafted_reads(ctx, oracle, k, w):
    """sketch_wave_kernel / flagN / sketch_kernel / sketch_compact (+ the sort) == StoreMinimizers + std::sort of the oracle, tuple for tuple, on the crafted
    batch of this (k, w)."""
    reads, mins, st = _a1_case(oracle, k, w)
    rng = np.random.default_rng(3)
    genome = synth.BASES[rng.integers(0, 4, size=256)]
    ik = np.array([1, 2, 2 | (1 << 63), 5], dtype=np.uint64); ip = np.array([0, 7, 100, 200], dtype=np.uint32)
    out = _run(ctx, genome, ik, ip, [r for _f, r in reads], k, w, 10)
    print("a1 (k=%d, w=%d): %d reads, %d tuples; %s" % (k, w, st["reads"], st["tuples"], {f: tuple(v) for f, v in sorted(st["fam"].items())}))
    _check_minimizers(out, mins)


# ---------------------------------------------------------------------------------------------------------------- C: a3 on a crafted index
WALK_K, WALK_W = 15, 8
WALK_MF = (1, 2, 3, 4, 5, 6, 7, 9)           # m - 1, m, m + 1 for query runs of m = 2, 3, 5 and m = 4, 6, 8 (beyond the three-key prefetch)
_WALK = {}


def _walk_set(oracle, k=WALK_K, w=WALK_W):
    """The distinct reads of the walk tests at (k, w), their sorted minimizers, a genome that holds every read, and the crafted indexes."""
    if (k, w) in _WALK:
        return _WALK[(k, w)]
    fam_reads = S.walk_reads(k, w)
    reads = [r for _f, r in fam_reads]
    mins = [S.sorted_minimizers(oracle, r, k, w) for r in reads]
    rng = np.random.default_rng(11)
    starts = np.zeros(len(reads) + 1, np.int64); starts[1:] = np.cumsum([len(r) for r in reads])
    genome = np.frombuffer(b"".join(reads) + S._rand(rng, 300), dtype=np.uint8)
    places = {}
    for d, (sk, sp) in enumerate(mins):
        for key, p in zip((sk & M63).tolist(), sp.tolist()):
            places.setdefault(key, int(starts[d]) + p)
    keys = np.array(sorted(places), dtype=np.uint64)
    idx = {"main": S.crafted_index(keys, len(genome), k, rng, places)}
    idx["empty"] = (np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    mid = keys[len(keys) // 2]
    idx["one"] = (np.array([mid], np.uint64), np.array([places[int(mid)]], np.uint32))
    idx["two"] = (np.array([mid | S.REV, mid], np.uint64), np.array([3, places[int(mid)]], np.uint32))
    idx["low"] = S.crafted_index(keys[:len(keys) // 3], len(genome), k, rng, places, foreign=False)     # every index key below most read keys: the last bucket's clamp
    idx["plain"] = S.crafted_index(keys, len(genome), k, rng, places, foreign=False)
    ws = dict(k=k, w=w, fam=[f for f, _r in fam_reads], reads=reads, mins=mins, genome=genome, gbytes=genome.tobytes() + b"\0" * 64, idx=idx, exp={})
    _WALK[(k, w)] = ws
    return ws


def _walk_expect(oracle, ws, name, mf):
    if (name, mf) not in ws["exp"]:
        ik, ip = ws["idx"][name]
        ws["exp"][(name, mf)] = [_expect(oracle, r, sk, sp, ws["gbytes"], ik, ip, ws["k"], mf) for r, (sk, sp) in zip(ws["reads"], ws["mins"])]
    return ws["exp"][(name, mf)]


def _query_runs(sk):
    """Lengths of the runs of equal masked keys in a sorted minimizer list, with the run's key."""
    mk = sk & M63
    if not len(mk):
        return np.zeros(0, np.int64), mk
    cut = np.nonzero(np.concatenate([[True], mk[1:] != mk[:-1]]))[0]
    return np.diff(np.concatenate([cut, [len(mk)]])), mk[cut]


def test_walk_cases_cover_their_families(oracle):
    ws = _walk_set(oracle)
    ik, ip = ws["idx"]["main"]
    imk = ik & M63
    assert np.all(imk[1:] >= imk[:-1])
    # index runs of every length on both sides of the 4-step switch, with mixed strand bits inside a run and at its end
    u, cnt = np.unique(imk, return_counts=True)
    assert {1, 2, 3, 4, 5, 6, 40} <= set(cnt.tolist())
    mixed = sum(1 for key in u[cnt >= 4][:200] if len(set((ik[imk == key] >> np.uint64(63)).tolist())) == 2)
    assert mixed >= 20
    nmin = [len(m[0]) for m in ws["mins"]]
    assert {0, 1, 2, 3} <= set(nmin)
    # foreign keys below / above every read key; the low index ends below most read keys
    allq = np.concatenate([m[0] & M63 for m in ws["mins"]])
    assert imk[0] < allq.min() and imk[-1] > allq.max()
    lk = ws["idx"]["low"][0] & M63
    assert (allq > lk.max()).mean() > 0.5
    # query runs of m equal keys that the index holds, for every m the max_freq values bracket; at the front and at the back of a read's list
    have = set(u.tolist())
    runs = set(); first_rep = last_rep = 0
    for sk, _sp in ws["mins"]:
        ln, key = _query_runs(sk)
        runs |= {int(n) for n, kk in zip(ln, key) if int(kk) in have}
        if len(ln) > 1:
            first_rep += ln[0] > 1 and int(key[0]) in have
            last_rep += ln[-1] > 1 and int(key[-1]) in have
    assert {2, 3, 4, 5, 6, 8} <= runs, runs
    assert first_rep >= 1 and last_rep >= 1
    # and the threshold shows: each max_freq lets more matches through than the one before where a run of that length exists
    tot = [sum(len(e["qi"]) for e in _walk_expect(oracle, ws, "main", mf)) for mf in WALK_MF]
    assert all(b > a for a, b in zip(tot[:6], tot[1:7])) and tot[7] > tot[6], tot
    assert len(ws["reads"]) >= 250 and max(len(r) for r in ws["reads"]) <= 200


def _walk_batch(ws, n):
    """n reads from the distinct set, tiled and permuted (n = 1: the read with the most minimizers)."""
    D = len(ws["reads"])
    if n == 1:
        return np.array([int(np.argmax([len(m[0]) for m in ws["mins"]]))])
    return np.random.default_rng(n).permutation(np.arange(n) % D)


@pytest.mark.gpu
@pytest.mark.parametrize("n_reads", [1, 1023, 2048, 32768 + 5])
def test_walk_reads_per_wave(ctx, oracle, n_reads):
    """compare_kernel with 1, 1, 2 and 32 reads per wave (FLAT_LANES = clamp(n_reads / 1024, 1, 32)) and a partly filled last block: every copy of every
    distinct read gets the oracle's match list, strand split included."""
    ws = _walk_set(oracle)
    exp = _walk_expect(oracle, ws, "main", 4)
    sel = _walk_batch(ws, n_reads)
    ik, ip = ws["idx"]["main"]
    out = _run(ctx, ws["genome"], ik, ip, [ws["reads"][d] for d in sel], ws["k"], ws["w"], 4)
    _check_minimizers(out, [ws["mins"][d] for d in sel])
    n = _check_matches(out, [exp[d] for d in sel])
    print("a3 reads per wave: %d reads, %d minimizers, %d matches" % (n_reads, len(out["mm_key"]), n))
    assert n > 0


@pytest.mark.gpu
@pytest.mark.parametrize("max_freq", WALK_MF)
def test_walk_max_freq(ctx, oracle, max_freq):
    """The query-run threshold `qs - qsStart < maxFreq` at m - 1, m, m + 1 for runs of m = 2..8 equal keys, at both ends of the walk."""
    ws = _walk_set(oracle)
    exp = _walk_expect(oracle, ws, "main", max_freq)
    ik, ip = ws["idx"]["main"]
    out = _run(ctx, ws["genome"], ik, ip, ws["reads"], ws["k"], ws["w"], max_freq)
    _check_minimizers(out, ws["mins"])
    n = _check_matches(out, exp)
    print("a3 max_freq %d: %d reads, %d matches" % (max_freq, len(ws["reads"]), n))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["empty", "one", "two", "low", "plain"])
def test_walk_index_shapes(ctx, oracle, name):
    """Indexes of 0, 1 and 2 entries, one whose largest key lies below most read keys (bounds_kernel's bucket clamp), one without foreign keys."""
    ws = _walk_set(oracle)
    exp = _walk_expect(oracle, ws, name, 5)
    ik, ip = ws["idx"][name]
    out = _run(ctx, ws["genome"], ik, ip, ws["reads"], ws["k"], ws["w"], 5)
    _check_minimizers(out, ws["mins"])
    n = _check_matches(out, exp)
    print("a3 index %s: %d entries, %d matches" % (name, len(ik), n))
    assert (n > 0) == (name != "empty")


@pytest.mark.gpu
def test_walk_k32_index(ctx, oracle):
    """k = 32: the largest masked index key has bit 62 set, so the bucket directory is built over all 63 key bits."""
    ws = _walk_set(oracle, 32, 8)
    ik, ip = ws["idx"]["main"]
    assert int((ik & M63).max()) >> 62 == 1
    exp = _walk_expect(oracle, ws, "main", 3)
    out = _run(ctx, ws["genome"], ik, ip, ws["reads"], 32, 8, 3)
    _check_minimizers(out, ws["mins"])
    n = _check_matches(out, exp)
    print("a3 k=32: %d entries, %d matches" % (len(ik), n))
    assert n > 1000


# ---------------------------------------------------------------------------------------------------------------- D: a4 at its edges
STRAND_K = (7, 8, 9, 15, 16, 17, 24, 31, 32)       # 0..4 full 8-byte words, with and without a byte tail
STRAND_W = 5
STRAND_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
STRAND_PATTERNS = ("forward", "reverse", "alternating", "last_round")
_STRAND = {}


def _strand_read(oracle, k):
    """A read R whose reverse complement R2 has a minimizer at its last k-mer, with a key that occurs once in R2; the genome ends with R2, so R2's last k-mer
    is the genome's last k-mer."""
    for s in range(400):
        rng = np.random.default_rng(7000 + 31 * k + s)
        R = S._rand(rng, 900)
        R2 = S._revcomp(R)
        sk, sp = S.sorted_minimizers(oracle, R2, k, STRAND_W)
        mk = sk & M63
        j = int(np.argmax(sp))
        if int(sp[j]) == len(R2) - k and (mk == mk[j]).sum() == 1:
            return R, R2, rng
    raise AssertionError("no read with a minimizer at its last k-mer")


def _strand_case(oracle, k):
    if k in _STRAND:
        return _STRAND[k]
    R, R2, rng = _strand_read(oracle, k)
    L = len(R)
    sk, sp = S.sorted_minimizers(oracle, R, k, STRAND_W)
    mk = sk & M63
    u, first, cnt = np.unique(mk, return_index=True, return_counts=True)
    once = u[cnt == 1]
    # between the two copies, a near miss of every such k-mer: all its bytes but byte i % k, so that a compare that skips a word or the tail calls it forward
    near, near_at, near_byte = [], {}, {}
    for i, x in enumerate(first[cnt == 1].tolist()):
        qp = int(sp[x]); j = i % k
        b = bytearray(R[qp:qp + k]); b[j] = b"CGTA"[b"ACGT".index(b[j])]
        near_at[qp] = L + i * k; near_byte[qp] = j
        near.append(bytes(b))
    NM = len(near) * k
    genome = np.frombuffer(R + b"".join(near) + R2, dtype=np.uint8)
    G = len(genome)
    gbytes = genome.tobytes() + b"\0" * 64
    order = rng.permutation(len(once))
    missed = set()
    cases = []
    for c in STRAND_COUNTS:
        # the walk drops or repeats a pair now and then (its `qs >= qe` exit, the raw-key skip): grow the key set until it finds exactly c
        n = c
        for _ in range(40):
            ik = np.sort(once[order[:n]])
            qi, ti = oracle.compare_lists(sk, sp, ik, np.zeros(len(ik), np.uint32), 1000)
            if len(qi) == c:
                break
            n += c - len(qi)
        assert len(qi) == c and n <= len(once), (k, c, len(qi), n)
        for pat in STRAND_PATTERNS:
            fwd = {"forward": np.ones(c, bool), "reverse": np.zeros(c, bool), "alternating": np.arange(c) % 2 == 0,
                   "last_round": np.arange(c) >= 64 * ((c - 1) // 64)}[pat]
            ip = np.zeros(len(ik), np.uint32)
            for m, (q, t) in enumerate(zip(qi.tolist(), ti.tolist())):
                qp = int(sp[q])
                if fwd[m]:
                    ip[t] = qp                                                  # the forward copy: the same bytes
                else:
                    # the reverse-complement copy; every third one elsewhere: the near miss, or anywhere
                    cand = [near_at[qp]] if m % 3 == 0 else [L + NM + (L - k - qp)] if m % 6 != 1 else []
                    cand += [int(x) for x in rng.integers(0, G - k + 1, size=8)]
                    ip[t] = next(x for x in cand if gbytes[x:x + k] != R[qp:qp + k])
                    if ip[t] == near_at[qp]:
                        missed.add(near_byte[qp])
            cases.append((c, pat, ik, ip, int(fwd.sum())))
    # the genome's last k-mer, as a forward match of R2
    sk2, sp2 = S.sorted_minimizers(oracle, R2, k, STRAND_W)
    mk2 = sk2 & M63
    last_key = mk2[int(np.argmax(sp2))]
    u2, c2 = np.unique(mk2, return_counts=True)
    ik_end = np.unique(np.concatenate([u2[c2 == 1][::7], [last_key]]))
    ip_end = np.array([G - k if key == last_key else int(rng.integers(0, G - k + 1)) for key in ik_end], np.uint32)
    _STRAND[k] = dict(missed=missed, R=R, R2=R2, genome=genome, gbytes=gbytes, sk=sk, sp=sp, sk2=sk2, sp2=sp2, cases=cases, end=(ik_end, ip_end))
    return _STRAND[k]


@pytest.mark.parametrize("k", STRAND_K)
def test_strand_cases_cover_their_families(oracle, k):
    sc = _strand_case(oracle, k)
    seen = set()
    for c, pat, ik, ip, nfwd in sc["cases"]:
        e = _expect(oracle, sc["R"], sc["sk"], sc["sp"], sc["gbytes"], ik, ip, k, 1000)
        assert len(e["qi"]) == c and e["nf"] == nfwd, (k, c, pat, len(e["qi"]), e["nf"])
        if pat == "last_round" and c:
            assert not e["strand"][64 * ((c - 1) // 64):].any() and e["strand"][:64 * ((c - 1) // 64)].all()
        if pat == "alternating":
            assert np.array_equal(e["strand"], (np.arange(c) % 2).astype(np.uint8))
        lo = _expect(oracle, sc["R"].lower(), sc["sk"], sc["sp"], sc["gbytes"], ik, ip, k, 1000)
        assert len(lo["qi"]) == c and lo["nf"] == 0                               # lower case never equals the upper-case genome (strncmp)
        seen.add((c, pat))
    assert seen == {(c, p) for c in STRAND_COUNTS for p in STRAND_PATTERNS}
    assert sc["missed"] == set(range(k))                                          # reverse matches that differ from the read in byte j alone, for every j < k
    ik, ip = sc["end"]
    e = _expect(oracle, sc["R2"], sc["sk2"], sc["sp2"], sc["gbytes"], ik, ip, k, 1000)
    at_end = ip[e["ti"]] == len(sc["genome"]) - k
    assert at_end.sum() == 1 and e["strand"][at_end][0] == 0                      # a forward match at the genome's last k-mer


@pytest.mark.gpu
@pytest.mark.parametrize("k", STRAND_K)
def test_strand_split_edges(ctx, oracle, k):
    """strand_kernel's k-byte compare (k / 8 words + k % 8 tail bytes) and its stable partition in rounds of 64: 0..200 matches per read in four strand
    patterns, a lower-case copy of the read (no forward match), the empty read, and a forward match at the genome's last k-mer.  The genome is the read, a
    near miss of each of its minimizer k-mers (one byte changed, every byte position in turn) and the read's reverse complement; reverse matches point at the
    reverse-complement copy, at a near miss or anywhere."""
    sc = _strand_case(oracle, k)
    reads = [sc["R"], sc["R"].lower(), b"", sc["R2"]]
    mins = [(sc["sk"], sc["sp"]), (sc["sk"], sc["sp"]), (np.zeros(0, np.uint64), np.zeros(0, np.uint32)), (sc["sk2"], sc["sp2"])]
    tot = 0
    for c, pat, ik, ip, _nf in sc["cases"] + [(None, "genome_end") + sc["end"] + (None,)]:
        exp = [_expect(oracle, r, m[0], m[1], sc["gbytes"], ik, ip, k, 1000) for r, m in zip(reads, mins)]
        out = _run(ctx, sc["genome"], ik, ip, reads, k, STRAND_W, 1000)
        _check_minimizers(out, mins)
        try:
            tot += _check_matches(out, exp)
        except AssertionError as e:
            raise AssertionError("k=%d count=%s pattern=%s: %s" % (k, c, pat, e))
    print("a4 k=%d: %d batches, %d matches" % (k, len(sc["cases"]) + 1, tot))
