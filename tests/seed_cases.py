"""Crafted reads and indexes for the seeding stages (a1 StoreMinimizers, a3 CompareLists, a4 SeparateMatchesByStrand): one seeded generator shared by
tools/make_golden_minimizers.py (the reference's own StoreMinimizers -> tests/golden/minimizers_golden.json), the CPU pin in tests/test_seed.py and the device
tests in tests/test_seed_edges.py.  Plain helpers, no fixtures."""
import numpy as np

from lra_amd import synth

M63 = np.uint64((1 << 63) - 1)
REV = np.uint64(1 << 63)

# (k, w) pairs of the a1 cases: w = 2 and w = MAX_W = 32 (2w = a whole 64-position tile), k = 31 / 32 (the key fills the word), tiny k, odd and even k
KW = [(1, 2), (3, 2), (5, 5), (8, 16), (15, 10), (16, 32), (31, 32), (32, 2), (32, 32), (21, 31)]
LONG = 320          # bases of the tie-run reads: k-mer positions in five 64-position tiles
ALPHABETS = (b"ACGT", b"AC", b"A")


def to_text(seq: bytes) -> str:
    """The golden file's / the reference driver's spelling of a read: the bytes 0..7 as the characters '0'..'7'."""
    return bytes(c + 48 if c < 8 else c for c in seq).decode("ascii")


def from_text(s: str) -> bytes:
    return bytes(c - 48 if 48 <= c < 56 else c for c in s.encode("ascii"))


def _rand(rng, n, alpha=b"ACGT"):
    return bytes(np.frombuffer(alpha, dtype=np.uint8)[rng.integers(0, len(alpha), size=n)]) if n > 0 else b""


def _revcomp(b: bytes) -> bytes:
    return synth.revcomp(np.frombuffer(b, dtype=np.uint8)).tobytes()


def keys_of(seq: bytes, k):
    """(masked canonical key, reverse flag) of every k-mer (synth.canonical_keys; bytes that are no base count as A, as seqMap has it)."""
    if len(seq) < k:
        return np.zeros(0, np.uint64), np.zeros(0, bool)
    return synth.canonical_keys(np.frombuffer(seq, dtype=np.uint8), k)


def is_clean(seq: bytes):
    return all(c < 8 or c in b"ACGTacgt" for c in seq)


def first_window_quirk(seq: bytes, k, w):
    """True when, among the first w k-mers, a reverse-strand key has a smaller masked value than every forward key (and there is a forward key): MinCount.h:91
    compares the first window unmasked, so the forward key wins there."""
    if len(seq) < w + k:
        return False
    key, rev = keys_of(seq[:w + k - 1], k)
    return bool(rev.any() and (~rev).any() and key[rev].min() < key[~rev].min())


def a1_reads(k, w, seed=0):
    """[(family, read bytes)] for one (k, w): the batch of tests/test_seed_edges.py::test_sketch_crafted_reads and the golden cases, in a seeded shuffle so that
    reads with an N, clean reads and reads that emit nothing alternate."""
    rng = np.random.default_rng(1000 * k + w + 7919 * seed)
    span = w + k - 1
    out = []
    # ---- read lengths: around the span, around the end of the literal replay (2w k-mers), k-mer counts around the 64-position tiles, the empty read
    lens = [span - 1, span, span + 1, 2 * w + k - 2, 2 * w + k - 1, 2 * w + k] + [nk + k - 1 for nk in (63, 64, 65, 127, 128, 129, 193)] + [0]
    for alpha in ALPHABETS:
        for L in lens:
            out.append(("len%d" % len(alpha), _rand(rng, L, alpha)))
    # ---- runs of tied window minima, LONG bases each
    tile = lambda unit: (unit * (LONG // len(unit) + 1))[:LONG]
    for per in (w - 1, w, w + 1):
        if per >= 1:
            out.append(("tie_period", tile(_rand(rng, per))))
    # a period of w - 1 puts two equal minima into one window once per period, and the active one is then not the ring-order choice: every rotation of the
    # unit, so that this window falls on the last position of a tile (the state carried into the next tile) for some of them
    if w > 2:
        unit = _rand(rng, w - 1)
        for s in range(w - 1):
            out.append(("tie_phase", tile(unit[s:] + unit[:s])))
    out.append(("tie_period", tile(b"AC")))
    out.append(("tie_period", tile(b"ACGT")))
    for base in (b"A", b"C"):
        h = LONG // 3
        out.append(("tie_homopolymer", base * h + _revcomp(base) * h + _rand(rng, LONG - 2 * h)))
    # the minimum k-mer of a period-w read recurs every w positions exactly: the active minimizer leaves the window as its equal enters.  A unit whose w
    # rotations have one smallest key is looked for; where the key space is too small for that (k = 1) the last try stands.
    for _ in range(64):
        unit = _rand(rng, w)
        key, _r = keys_of((unit * (k // w + 3))[:w + k - 1], k)
        if (key[:w] == key[:w].min()).sum() == 1:
            break
    out.append(("tie_recur", tile(unit)))
    out.append(("tie_recur", _rand(rng, 37) + tile(unit)[:LONG - 37]))
    # ---- first window: a reverse-strand key below every forward key
    found = 0
    for _ in range(4000):
        r = _rand(rng, 2 * w + k + 70)
        if first_window_quirk(r, k, w):
            out.append(("first_window", r)); found += 1
            if found == 4:
                break
    # ---- palindromic k-mers (fwd == rc: the key takes the reverse flag), even k only
    if k % 2 == 0:
        half = _rand(rng, k // 2)
        pal = half + _revcomp(half)
        out.append(("palindrome", _rand(rng, 40) + pal + _rand(rng, 50) + pal + _rand(rng, 30)))
        out.append(("palindrome", tile(pal)[:200]))
        out.append(("palindrome", tile(b"AT" if k > 1 else b"A")[:150]))
    # ---- the N route
    L = 137 + span
    for alpha in (b"ACGT", b"AC"):
        for off in (0, 1, span - 1, span, 63, 64, 65, 127, 128, L - span - 1, L - span, L - k, L - 1):
            r = bytearray(_rand(rng, L, alpha)); r[off] = ord("N")
            out.append(("n_one", bytes(r)))
    for gap in (span + 1, span):
        for at in (0, 40, L - gap - 1):
            r = bytearray(_rand(rng, L)); r[at] = ord("N"); r[at + gap] = ord("N")
            out.append(("n_two", bytes(r)))
    out.append(("n_all", b"N" * L))
    out.append(("n_all", b"N" * (span + 1)))
    r = _rand(rng, L)
    out.append(("lower", r[:50] + r[50:50 + span + 5].lower() + r[50 + span + 5:]))
    out.append(("lower", r.lower()))
    out.append(("lower", r[:70].lower() + b"n" + r[71:]))
    out.append(("bytes0_7", bytes(synth.CODE[np.frombuffer(r, dtype=np.uint8)].astype(np.uint8))))                     # 0..3
    out.append(("bytes0_7", bytes((synth.CODE[np.frombuffer(r, dtype=np.uint8)] + 4 * (np.arange(L) % 2)).astype(np.uint8))))   # 0..7 mixed
    out.append(("bytes0_7", r[:60] + bytes([4, 5, 6, 7, 0, 1, 2, 3]) * 3 + r[84:]))
    for ch in (b"X", b"-"):
        b2 = bytearray(r); b2[L // 2] = ch[0]; b2[L // 2 + span + 3] = ch[0]
        out.append(("other_byte", bytes(b2)))
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def a1_stats(oracle, k, w, reads):
    """Per-family counts, from the oracle and the pinned key function alone, of what the reads of one (k, w) exercise."""
    span = w + k - 1
    st = dict(reads=len(reads), tuples=0, empty_out=0, tie_cross_tile=0, n_emits=0, last_window=0, first_window=0, palindrome=0, tile_end_tie=0, fam={})
    for fam, r in reads:
        key, pos = oracle.store_minimizers(r, k, w)
        f = st["fam"].setdefault(fam, [0, 0]); f[0] += 1; f[1] += len(key)
        st["tuples"] += len(key)
        st["empty_out"] += len(key) == 0
        clean = is_clean(r)
        if not clean and len(key):
            st["n_emits"] += 1
        # the last-window quirk: a clean run of exactly one window at the read's end (the byte before it is no base) is found by no search, :27 / :115
        L = len(r)
        if not clean and L > span and is_clean(r[L - span:]) and not is_clean(r[L - span - 1:L - span]) and not (len(pos) and pos.max() >= L - span):
            st["last_window"] += 1
        if clean and L > span and first_window_quirk(r, k, w):
            ck, cr = keys_of(r[:span], k)
            masked_arg = int(np.argmin(ck))
            if len(pos) and int(pos[0]) != masked_arg and not cr[int(pos[0])]:
                st["first_window"] += 1
        if clean and L >= k and k % 2 == 0:
            a = np.frombuffer(r.upper() if r.isalpha() else r, dtype=np.uint8)
            c = synth.CODE[a]
            n = L - k + 1
            pal = np.ones(n, bool)
            for i in range(k // 2):
                pal &= c[i:i + n] + c[k - 1 - i:k - 1 - i + n] == 3
            if pal.any() and len(key) and np.isin(np.nonzero(pal)[0], pos).any():
                st["palindrome"] += 1
        # the window that ends at a tile's last position (p = 63 mod 64, beyond the literal replay) holds its minimum twice
        if clean and L >= k:
            ck, _cr = keys_of(r, k)
            for p in range(63, len(ck), 64):
                if p >= 2 * w:
                    win = ck[p - w + 1:p + 1]
                    if (win == win.min()).sum() >= 2:
                        st["tile_end_tie"] += 1
                        break
        # two equal minimal keys within w of each other at emitted positions p1 < 64 j <= p2, beyond the literal replay
        if clean and len(pos) > 1:
            mk = key & M63
            p = pos.astype(np.int64)
            eq = (mk[1:] == mk[:-1]) & (p[1:] - p[:-1] <= w) & (p[:-1] // 64 != p[1:] // 64) & (p[1:] >= 2 * w)
            st["tie_cross_tile"] += int(eq.any())
    return st


# ------------------------------------------------------------------------------------------------------------------ a3: crafted index
RUN_LENGTHS = (0, 1, 2, 3, 4, 5, 6, 40)             # index entries per read key, cycling: both sides of bounds_kernel's 4-step switch
STRAND_PATTERNS = ("F", "R", "FR", "FFRR")           # strand bits within a run of equal masked keys, cycling


def sorted_minimizers(oracle, read: bytes, k, w):
    key, pos = oracle.store_minimizers(read, k, w)
    return oracle.sort_minimizers(key, pos)


def walk_reads(k, w, seed=0):
    """[(family, read)]: a few hundred distinct reads of at most 200 bases for the index walk -- random reads, reads with 0..3 minimizers (lengths around the
    span), and tandem repeats in which minimizer keys occur m = 2..8 times, with and without unique flanks."""
    rng = np.random.default_rng(4242 + 100 * k + w + seed)
    span = w + k - 1
    out = [("empty", b""), ("short", _rand(rng, span - 1)), ("short", _rand(rng, span))]
    for L in (span + 1, span + 1, span + 2, span + 3, span + 4, span + 6, span + 8):
        out.append(("few", _rand(rng, L)))
    for _ in range(150):
        out.append(("random", _rand(rng, int(rng.integers(span + 1, 201)))))
    for copies in (2, 3, 4, 5, 6, 8):
        for _ in range(12):
            u = int(rng.integers(max(w, 3), max(w, 3) + 12))
            unit = _rand(rng, u)
            room = 200 - copies * u
            if room < 0:
                u = 200 // copies; unit = unit[:u]; room = 200 - copies * u
            a = int(rng.integers(0, room + 1)); b = int(rng.integers(0, room - a + 1))
            out.append(("tandem%d" % copies, _rand(rng, a) + unit * copies + _rand(rng, b)))
    for _ in range(20):
        out.append(("lowcomplex", _rand(rng, int(rng.integers(span + 1, 160)), b"AC")))
    out.append(("lowcomplex", b"C" * 120))              # (not A: poly-A's key is 0, and the index wants a foreign key below every read key)
    out.append(("lowcomplex", b"AC" * 70))
    return out


def crafted_index(all_keys, genome_len, k, rng, places=None, foreign=True):
    """Index arrays over the given sorted unique masked keys: key i gets RUN_LENGTHS[i % 8] entries whose strand bits follow STRAND_PATTERNS[(i // 8) % 4];
    with `foreign`, keys that no read has go below the smallest, between, and above the largest.  ip: places[key] for every other entry where given (a spot of
    the genome that holds the k-mer), else anywhere in the genome."""
    ik, ip = [], []
    hi = genome_len - k
    def add(mk, n, pat, place=None):
        for j in range(n):
            ik.append(int(mk) | (int(REV) if pat[j % len(pat)] == "R" else 0))
            ip.append(int(place) if place is not None and j % 2 == 0 else int(rng.integers(0, hi + 1)))
    keys = [int(x) for x in all_keys]
    present = set(keys)
    if foreign and keys:
        lo = keys[0]
        for f in sorted({lo // 3, lo // 2, lo - 1} - present - {-1}):
            add(f, 2, "FR")
    for i, mk in enumerate(keys):
        add(mk, RUN_LENGTHS[i % 8], STRAND_PATTERNS[(i // 8) % 4], None if places is None else places.get(mk))
        if foreign and i % 5 == 2 and mk + 1 not in present:
            add(mk + 1, 1 + i % 3, "RF")
    if foreign and keys:
        top = keys[-1]
        for f in (top + 1, top + 7, min(top * 2, int(M63))):
            if f not in present and f <= int(M63):
                add(f, 3, "FRF")
    ik = np.array(ik, dtype=np.uint64); ip = np.array(ip, dtype=np.uint32)
    order = np.argsort(ik & M63, kind="stable")
    return ik[order], ip[order]
