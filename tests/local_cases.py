"""Case builders for test_local_edges.py: sequences for the tier-2 index (local_sketch, the five sort kernels, RemoveFrequent) and task lists for
CompareLists<LocalTuple,SmallTuple> (the four forms of the walk), each built so that the class it goes through follows from numbers the oracle gives on the CPU.

Plain functions, deterministic, no device.  The constants below restate the limits local.hip dispatches on; the tests assert the cases sit on them."""
import numpy as np

from lra_amd import synth

# ---- the limits of local.hip
WMAX = 256                      # local_sketch: staged window length
LCAP, LS_WORDS = 160, 6144      # local_sort_filter: staged list length, a block's LDS words
RANK_CAP = 256                  # local_sort_unique's longest list; stride > RANK_CAP sends ties to radix + exact wave
CMP_CAP = 128                   # pairs a task keeps in the one-pass small form
CMP_TASK_MAX, CMP_WORDS = 512, 10240
CW_ROW = 512                    # pairs a task keeps in the cached walk's row
NEAR = 12                       # the cached walk's search reads through its lines this close to the cursor, directly beyond
LINE = 8                        # words a cursor's line holds

ALL_KEPT = 1 << 20              # a max_freq at which RemoveFrequent removes nothing: the raw list
LENS = (1, 2, 16, 17, 160, 161, 256, 257, 1024, 1025, 2048, 2049, 4087)

_G = {}


def genome(seed=31, n=120_000):
    if (seed, n) not in _G:
        _G[(seed, n)] = synth.make_genome(n, seed=seed, repeat_frac=0.0)
    return _G[(seed, n)]


def B(s):
    return np.frombuffer(s, np.uint8).copy()


def tile(unit, length):
    return np.tile(unit, length // len(unit) + 1)[:length].copy()


def force_tie(seq, k):
    """A copy of seq with one stretch (30 bases where it fits, never fewer than k) copied to a second place: at least one key twice.  A sequence too short for two
    disjoint stretches becomes one base repeated (all its k-mers equal)."""
    s = seq.copy()
    L = len(s)
    if L < 2 * k:
        s[:] = s[0]
        return s
    n = min(30, L // 2)
    s[L - n:] = s[:n]
    return s


def untie(seq, k):
    """A copy of seq in which no k-mer occurs twice: wherever the k-mer that ends at a base has been seen, that base is changed to the first one that gives a new k-mer."""
    s = seq.copy()
    c = synth.CODE[s].astype(np.int64)
    seen = set()
    mask = (1 << (2 * k)) - 1
    v = 0
    for i in range(len(s)):
        if i < k - 1:
            v = (v << 2) | int(c[i])
            continue
        for d in range(4):
            b = (int(c[i]) + d) & 3
            x = ((v << 2) | b) & mask
            if x not in seen:
                break
        else:
            raise AssertionError("no free k-mer")
        seen.add(x); v = x; c[i] = b
    return synth.BASES[c]


def kmer_keys(seq, k):
    """The k-mer of every position, as the 2-bit packing a LocalTuple holds (ACGT only)."""
    c = synth.CODE[seq].astype(np.int64)
    nk = len(seq) - k + 1
    v = np.zeros(max(nk, 0), np.int64)
    for i in range(k):
        v = (v << 2) | c[i:i + len(v)]
    return v


# ---------------------------------------------------------------------------------------------------------------- A: index batches
def _w1_lengths(k, lens, seed, untied=False):
    """Per raw length n: a genome slice of n + k - 1 bases (w = 1: one tuple per k-mer; untied: with the few substitutions that make its k-mers pairwise different)
    and the same slice with a tie forced.  A list of one tuple needs an N: a sequence of k bases has no span the reference takes (MinCount.h:200), so it is k + 1
    bases, the last one N; a list of one tuple has no tied form."""
    g = genome(seed)
    out = []
    at = 100
    for n in lens:
        L = n + k - 1
        s = g[at:at + L].copy(); at += L + 13
        if n == 1:
            out.append(("plain1", np.concatenate([s, B(b"N")])))
            continue
        out.append(("plain%d" % n, untie(s, k) if untied else s))
        out.append(("tied%d" % n, force_tie(s, k)))
    return out


def stride_seqs():
    """The sequences of the stride pair (window 265 / 266 at k = 10, w = 1: strides 256 / 257)."""
    g = genome(33)
    seqs = [("full265", g[0:265].copy()), ("full266", g[300:566].copy()), ("multi531", g[600:1131].copy()),
            ("tied265", force_tie(g[1200:1465], 10)), ("tied266", force_tie(g[1500:1766], 10))]
    at = 2000
    for n in (161, 162, 200, 255, 256):                                   # tied lists above LCAP: local_sort_filter in HBM at window 265
        seqs.append(("tiedhbm%d" % n, force_tie(g[at:at + n + 9], 10))); at += 300
    for n in (2, 16, 17, 100, 159, 160):                                  # tied lists that stage
        seqs.append(("tiedlds%d" % n, force_tie(g[at:at + n + 9], 10))); at += 300
    for i in range(80):                                                   # 80 tied lists of 150: a block's 64 need 9600 words of the 6144
        seqs.append(("crowd%d" % i, force_tie(g[at:at + 159], 10))); at += 170
    seqs += short_tie_seqs() + cut_seqs()
    return seqs


UNIT13 = B(b"ACGGTCATTGCAG")
UNIT37 = B(b"ACGTTGCAAGGCTTACCGATAGTCCATGGATCAGTCA")


def short_tie_seqs():
    """A 13-base unit tiled to 25, 26, 35, 36 bases: 16, 17, 26, 27 tuples of 13 keys (k = 10, w = 1)."""
    return [("unit13x%d" % L, tile(UNIT13, L)) for L in (25, 26, 35, 36)]


def cut_seqs():
    """A 37-base unit 14, 15 and 16 times: at k = 10, w = 1 in one window every key 13..14, 14..15, 15..16 times."""
    return [("unit37x%d" % c, np.tile(UNIT37, c)) for c in (14, 15, 16)]


def sketch_seqs(window, k=10, w=5):
    """Sketch edges at span = w + k - 1: lengths and tails round the span, exact and one-over window lengths, N placements, lower case."""
    g = genome(35)
    span = w + k - 1
    seqs = []
    for L in (span - 1, span, span + 1, span + 9, span + 10):
        seqs.append(("len%d" % L, g[SKETCH_AT:SKETCH_AT + L].copy()))
        seqs.append(("tail%d" % L, np.concatenate([g[5000:5000 + window], g[SKETCH_AT:SKETCH_AT + L]])))
    seqs.append(("exact", g[6000:6000 + window].copy()))
    seqs.append(("plus1", g[7000:7000 + window + 1].copy()))
    base = g[8000:8000 + 2 * window + 40].copy()
    for name, pos in (("n_first", [0]), ("n_span_last", [span - 1]), ("n_last", [len(base) - 1]), ("n_window_last", [window - 1]), ("n_window_first", [window])):
        s = base.copy(); s[pos] = ord("N"); seqs.append((name, s))
    s = base.copy(); s[span - 1::span] = ord("N"); seqs.append(("n_every_span", s))                       # no valid span anywhere
    s = g[9000:9000 + 3 * window].copy(); s[window:2 * window] = ord("N"); seqs.append(("n_window", s))  # an all-N window between two good ones
    seqs.append(("lower", np.frombuffer(g[10000:10000 + window + 77].tobytes().lower(), np.uint8).copy()))
    seqs.append(("mixed_case", np.frombuffer(g[11000:11300].tobytes().lower()[:150] + g[11150:11300].tobytes(), np.uint8).copy()))
    seqs.append(("empty", np.zeros(0, np.uint8)))
    return seqs


SKETCH_AT = 4004                 # where the span-length slices are cut: chosen so that 13, 14, 15, 23, 24 bases give 0, 0, 1, 3, 4 tuples (asserted)


def window257_seqs():
    """window = 257 at w = 5: full windows one base beyond the sketch's staged length, tails staged; an N run over window positions 255 .. 257."""
    g = genome(37)
    seqs = [("one", g[0:257].copy()), ("one_plus", g[300:558].copy()), ("two", g[600:1114].copy()), ("long", g[1200:2200].copy()), ("staged", g[2300:2556].copy())]
    s = g[2600:3400].copy(); s[255:258] = ord("N"); seqs.append(("n255_257", s))
    s = g[3500:4300].copy(); s[256] = ord("N"); seqs.append(("n256", s))
    return seqs


def index_batches():
    """name -> dict(k, w, window, max_freq, seqs=[(label, sequence)]).  Every batch is one call of the index entry."""
    b = {}
    w1_10 = _w1_lengths(10, LENS, 41, untied=True)
    w1_7 = _w1_lengths(7, LENS + (4090,), 43)
    b["w1_k10"] = dict(k=10, w=1, window=4096, max_freq=15, seqs=w1_10)
    b["w1_k7"] = dict(k=7, w=1, window=4096, max_freq=15, seqs=w1_7)
    poly = [("four_keys", genome(45)[500:4596].copy()), ("four_keys_b", genome(45)[5000:9096].copy()), ("short", genome(45)[9100:9117].copy())]
    b["w1_k1_all"] = dict(k=1, w=1, window=4096, max_freq=ALL_KEPT, seqs=poly)                            # 4096 tuples of four keys: n == NT * IPT == capAll
    b["w1_k1_none"] = dict(k=1, w=1, window=4096, max_freq=15, seqs=poly)                                 # everything removed
    st = stride_seqs()
    for window in (265, 266):
        b["stride_w%d" % window] = dict(k=10, w=1, window=window, max_freq=15, seqs=st)
        for mf in (6, 7, 8):                                                                              # the unit37 windows hold runs of 6 and 7
            b["stride_w%d_mf%d" % (window, mf)] = dict(k=10, w=1, window=window, max_freq=mf, seqs=st)
    b["cut_w4096"] = dict(k=10, w=1, window=4096, max_freq=15, seqs=cut_seqs() + short_tie_seqs())
    b["window257"] = dict(k=10, w=5, window=257, max_freq=15, seqs=window257_seqs())
    ordinary = [("g3000", genome(47)[0:3000].copy()), ("g4096", genome(47)[4000:8096].copy()), ("tied", force_tie(genome(47)[9000:9700], 10)),
                ("tied250", force_tie(genome(47)[9800:10050], 10)), ("acg", tile(B(b"ACG"), 900))]
    for mf in (1, 2):
        b["mf%d_w5" % mf] = dict(k=10, w=5, window=256, max_freq=mf, seqs=ordinary)
        b["mf%d_w1" % mf] = dict(k=10, w=1, window=4096, max_freq=mf, seqs=ordinary + w1_10)
    b["sketch_256"] = dict(k=10, w=5, window=256, max_freq=15, seqs=sketch_seqs(256))
    b["sketch_w16"] = dict(k=10, w=16, window=256, max_freq=15, seqs=sketch_seqs(256, 10, 16))
    b["sketch_maxw"] = dict(k=10, w=16, window=26, max_freq=15, seqs=sketch_seqs(26, 10, 16))             # window = w + k, the smallest the entry accepts
    g = genome(49)
    for k in range(1, 11):
        b["k%d" % k] = dict(k=k, w=5, window=64, max_freq=15, seqs=[("g", g[k * 500:k * 500 + 333].copy()), ("short", g[100:100 + k + 4].copy()),
                                                                     ("tied", force_tie(g[k * 500 + 400:k * 500 + 464], k))])
    return b


def masks(n):
    """Activity masks over n sequences: first off, last off, two neighbours off, all off, all on, every other."""
    m = {}
    a = np.ones(n, np.uint8); a[0] = 0; m["first_off"] = a
    a = np.ones(n, np.uint8); a[-1] = 0; m["last_off"] = a
    a = np.ones(n, np.uint8); a[n // 2] = a[n // 2 + 1] = 0; m["neighbours_off"] = a
    m["all_off"] = np.zeros(n, np.uint8)
    m["all_on"] = np.ones(n, np.uint8)
    a = np.ones(n, np.uint8); a[::2] = 0; m["every_other"] = a
    a = np.zeros(n, np.uint8); a[n // 3] = 7; m["one_on"] = a                                             # any non-zero byte is on
    return m


def masked_seqs():
    g = genome(51)
    return [("a", g[0:700].copy()), ("b", g[800:1056].copy()), ("empty", np.zeros(0, np.uint8)), ("c", g[1100:1357].copy()), ("tied", force_tie(g[1400:1900], 10)),
            ("d", g[2000:2014].copy()), ("e", g[2100:3500].copy()), ("empty2", np.zeros(0, np.uint8)), ("f", g[3600:3900].copy())]


# ---------------------------------------------------------------------------------------------------------------- B: CompareLists tasks
def pack(t, pos):
    return (np.asarray(t, dtype=np.uint32) & np.uint32(0xFFFFF)) | (np.asarray(pos, dtype=np.uint32) << np.uint32(20))


def run_task(a, b, m, last, q_only=0, t_only=0, seed=0, span=256):
    """Two sorted lists: one key a times in the query and b times in the target, then m keys once on both sides with q_only / t_only unshared keys among them, then
    (last) one more shared key at the end of both.  Positions are random below `span`.  Returns (q words, t words)."""
    rng = np.random.default_rng(1000 + seed)
    n_mid = m + q_only + t_only
    keys = 1000 + 3 * np.arange(n_mid + 2, dtype=np.int64)               # the run's key, the middle keys, the last key
    kind = np.zeros(n_mid, np.int8); kind[m:m + q_only] = 1; kind[m + q_only:] = 2
    rng.shuffle(kind)
    mid = keys[1:1 + n_mid]
    qk = [np.full(a, keys[0])] + [mid[kind != 2]] + ([keys[-1:]] if last else [])
    tk = [np.full(b, keys[0])] + [mid[kind != 1]] + ([keys[-1:]] if last else [])
    qk, tk = np.concatenate(qk), np.concatenate(tk)
    return pack(qk, rng.integers(0, span, len(qk))), pack(tk, rng.integers(0, span, len(tk)))


def random_task(rng, nq, nt, nkeys, span=256):
    keys = np.sort(rng.choice(1 << 20, nkeys, replace=False)).astype(np.uint32)
    qk = np.sort(rng.choice(keys, nq)) if nq else np.zeros(0, np.uint32)
    tk = np.sort(rng.choice(keys, nt)) if nt else np.zeros(0, np.uint32)
    return pack(qk, rng.integers(0, span, nq)), pack(tk, rng.integers(0, span, nt))


class Task:
    def __init__(self, name, q, t, max_diag=0, min_diag=0):
        self.name, self.q, self.t, self.max_diag, self.min_diag = name, np.asarray(q, np.uint32), np.asarray(t, np.uint32), int(max_diag), int(min_diag)

    @property
    def words(self):
        return len(self.q) + len(self.t)


E = np.zeros(0, np.uint32)


class Raw:
    """Stands in for a LocalIndex in local_compare_batch: a raw tuple array on the device."""

    def __init__(self, ctx, words):
        import torch
        from lra_amd import local
        self.t_ = torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).to(ctx.device)
        self.res = local.LocalIndexResult()
        self.res.d_tuples = self.t_.data_ptr()

# (a, b, m, last) -> pairs at max_freq = 15 (the reference's walk never pairs the query's last element from the front)
TABLE = {(8, 16, 0, True): 128, (8, 16, 1, True): 129, (8, 64, 0, True): 512, (8, 64, 1, True): 513, (15, 34, 2, False): 511, (7, 18, 1, True): 127}


def within_small_tasks():
    """Tasks at, not above, the small form's limits: 127 / 128 pairs, lists of 255, empty and one-tuple lists, and 128 tasks of ~200 words side by side (a block's
    64 outgrow CMP_WORDS)."""
    rng = np.random.default_rng(61)
    ts = [Task("pairs127", *run_task(7, 18, 1, True, seed=1)), Task("pairs128", *run_task(8, 16, 0, True, seed=2)),
          Task("q255", run_task(1, 1, 253, True, seed=3)[0], run_task(1, 1, 100, True, seed=3)[1]),
          Task("t255", run_task(1, 1, 100, True, seed=4)[0], run_task(1, 1, 253, True, seed=4)[1]),
          Task("both255", *run_task(1, 1, 90, True, q_only=163, t_only=163, seed=5)),
          Task("empty_q", E, random_task(rng, 0, 30, 60)[1]), Task("empty_t", random_task(rng, 30, 0, 60)[0], E), Task("empty_both", E, E),
          Task("one_one_same", pack([77], [5]), pack([77], [9])), Task("one_one_diff", pack([77], [5]), pack([78], [9])),
          Task("one_q", pack([500000], [1]), random_task(rng, 0, 40, 50)[1]), Task("one_t", random_task(rng, 40, 0, 50)[0], pack([500000], [1])),
          Task("run8", *run_task(8, 16, 0, True, seed=6)), Task("run9", *run_task(9, 14, 0, True, seed=7))]
    for i in range(128):
        nq = int(rng.integers(90, 111)); ts.append(Task("crowd%d" % i, *random_task(rng, nq, 200 - nq, 150)))
    for i in range(40):
        ts.append(Task("rand%d" % i, *random_task(rng, int(rng.integers(1, 60)), int(rng.integers(1, 60)), 50)))
    return ts


def over_small_tasks():
    """Each is above exactly one of the small form's limits (CMP_CAP pairs, 255 tuples a list, CMP_TASK_MAX words)."""
    return [Task("pairs129", *run_task(8, 16, 1, True, seed=11)),
            Task("q256", run_task(1, 1, 254, True, seed=12)[0], run_task(1, 1, 100, True, seed=12)[1]),
            Task("t256", run_task(1, 1, 100, True, seed=13)[0], run_task(1, 1, 254, True, seed=13)[1]),
            Task("words512", *run_task(1, 1, 100, True, q_only=100, t_only=208, seed=14)),            # 202 + 310
            Task("words513", *run_task(1, 1, 100, True, q_only=100, t_only=209, seed=15)),            # 202 + 311: the first task the staging leaves in HBM
            Task("pairs254", *run_task(1, 1, 253, True, seed=17)),                                   # lists of 255 that pair all the way
            Task("both512", *run_task(1, 1, 510, True, seed=16))]


def big_tasks(n, seed=71, span=2048, sparse=False):
    """Tasks of more than CMP_TASK_MAX words (lists of 260 .. 1000 tuples): the kind that turns a batch to the large form.  sparse: keys enough that no task comes
    near CW_ROW pairs."""
    rng = np.random.default_rng(seed)
    ts = []
    for i in range(n):
        if sparse and i % 9 != 7:
            nq, nt, nkeys = int(rng.integers(260, 1000)), int(rng.integers(260, 1000)), int(rng.integers(2600, 3000))
        elif i % 9 == 4:
            nq, nt, nkeys = 400, 350, 30                                                               # long runs on both sides, beyond max_freq too
        elif i % 9 == 7:
            nq, nt, nkeys = int(rng.integers(1, 4)), int(rng.integers(520, 900)), 700
        else:
            nq, nt, nkeys = int(rng.integers(260, 1000)), int(rng.integers(260, 1000)), int(rng.integers(600, 3000))
        ts.append(Task("big%d" % i, *random_task(rng, nq, nt, nkeys, span)))
    return ts


def row_tasks():
    """Pair counts round CW_ROW, as small tasks and (with unshared keys added) as tasks above CMP_TASK_MAX words."""
    ts = []
    for (a, b, m, last), n in sorted(TABLE.items()):
        if n >= 511:
            ts.append(Task("pairs%d" % n, *run_task(a, b, m, last, seed=20 + n, span=2048)))
            ts.append(Task("pairs%d_wide" % n, *run_task(a, b, m, last, q_only=300, t_only=350, seed=30 + n, span=2048)))
    return ts


def thousands_tasks():
    return [Task("pairs4200", *run_task(14, 300, 5, True, q_only=40, t_only=10, seed=41, span=2048)),
            Task("pairs2800_wide", *run_task(10, 280, 5, True, q_only=400, t_only=300, seed=42, span=2048))]


def with_bounds(tasks, oracle, max_freq, seed=81):
    """The same tasks with per-task diagonal bounds, cycling through: both zero; one side zero (the filter is off, CompareLists.h:87); a band round a pair's diagonal;
    maxDiag on a pair's diagonal; minDiag on a pair's diagonal; a band that holds nothing."""
    rng = np.random.default_rng(seed)
    out = []
    for i, t in enumerate(tasks):
        eq, et = oracle.compare_lists_local(t.q, t.t, max_freq)
        d = ((t.t[et] >> 20).astype(np.int64) - (t.q[eq] >> 20).astype(np.int64)) if len(eq) else np.zeros(0, np.int64)
        d = d[(d != 0) & (d != 40) & (d != -40)]
        d0 = int(d[int(rng.integers(0, len(d)))]) if len(d) else 17
        mode = i % 7
        mx, mn = [(0, 0), (d0, 0), (0, d0), (d0 + 30, d0 - 30), (d0, d0 - 40), (d0 + 40, d0), (5000, 4999)][mode]
        out.append(Task(t.name + "_b%d" % mode, t.q, t.t, mx, mn))
    return out


def layout(tasks, q_gaps=None, t_gaps=None):
    """The two tuple arrays (each padded with LINE zero words: the cached walk fetches whole lines) and the index ranges of the tasks.  q_gaps / t_gaps: filler words
    in front of each task's list (to choose its offset)."""
    qs, ts_, ql, qh, tl, th = [], [], [], [], [], []
    qo = to = 0
    for i, t in enumerate(tasks):
        gq = int(q_gaps[i]) if q_gaps is not None else 0
        gt = int(t_gaps[i]) if t_gaps is not None else 0
        qs.append(np.full(gq, 0xFFFFFFFF, np.uint32)); qo += gq
        ts_.append(np.full(gt, 0xFFFFFFFF, np.uint32)); to += gt
        qs.append(t.q); ql.append(qo); qo += len(t.q); qh.append(qo)
        ts_.append(t.t); tl.append(to); to += len(t.t); th.append(to)
    qa = np.concatenate(qs + [np.zeros(LINE, np.uint32)]); ta = np.concatenate(ts_ + [np.zeros(LINE, np.uint32)])
    return qa, ta, ql, qh, tl, th


def n_big(tasks):
    return sum(t.words > CMP_TASK_MAX for t in tasks)


def small_form_batches():
    """name -> tasks; fewer than half of each batch's tasks are above CMP_TASK_MAX words."""
    base = within_small_tasks()
    b = {"within": base}
    for o in over_small_tasks():
        b["over_" + o.name] = base[:100] + [o] + base[100:]
    b["over_all"] = over_small_tasks() + base + row_tasks() + big_tasks(20)
    return b


def large_form_batches():
    """name -> tasks; more than half of each batch's tasks are above CMP_TASK_MAX words."""
    small = within_small_tasks()
    small = small[:14] + small[14:142:8] + small[142:]                       # (every eighth of the crowd: the batch stays mostly big)
    over = over_small_tasks()
    rows = row_tasks()
    big = big_tasks(150)
    b = {"rows_fit": small + over + [t for t in rows if "513" not in t.name] + big_tasks(150, seed=73, sparse=True),
         "rows_over": small + over + rows + thousands_tasks() + big}
    return b


def _interleave(x, y):
    return [t for p in zip(x, y) for t in p]


def switch_batches(m=20):
    """Two batches of 2 m tasks from one set: m tasks above CMP_TASK_MAX words (2 * m > 2 m is false: the small form) and m + 1 (the large form)."""
    big = big_tasks(m + 1, seed=91)
    small = (within_small_tasks()[:14] + over_small_tasks()[:3] + row_tasks()[::2])[:m]
    assert len(small) == m
    lo = _interleave(big[:m], small)
    hi = _interleave(big[:m - 1], small[:m - 1]) + [big[m - 1], big[m]]
    return lo, hi


# ---- the cached walk's lines and search window
DISTANCES = (0, 1, 11, 12, 13, 300)


def front_task(dists, a=1, b=1, seed=0, span=2048):
    """A task whose every step searches the target upwards: the lists share their last key (the end gap is 0, so the walk takes its front branch), and in front of
    the i-th shared key the target holds dists[i] keys of its own.  a / b: copies of each shared key in the query / target."""
    rng = np.random.default_rng(2000 + seed)
    qk, tk = [], []
    key = 5000
    for d in dists:
        tk += list(range(key, key + d)); key += d + 5
        qk += [key] * a; tk += [key] * b; key += 7
    qk.append(key); tk.append(key)
    return pack(qk, rng.integers(0, span, len(qk))), pack(tk, rng.integers(0, span, len(tk)))


def back_task(dists, a=1, b=1, seed=0, span=2048):
    """The mirror: the target's first key lies one below the query's first (a start gap of 1, never more than the end gap), so the walk takes its back branch, and
    behind the i-th shared key from the end the target holds dists[i] keys of its own."""
    rng = np.random.default_rng(3000 + seed)
    qk, tk = [], []
    key = 900000
    for d in dists:
        tk += list(range(key - d + 1, key + 1))[::-1]; key -= d + 5
        qk += [key] * a; tk += [key] * b; key -= 7
    qk += [key, key - 3]; tk += [key - 4]
    qk, tk = qk[::-1], tk[::-1]
    return pack(qk, rng.integers(0, span, len(qk))), pack(tk, rng.integers(0, span, len(tk)))


def line_tasks():
    """Tasks for the cached walk: every rotation of DISTANCES from both ends, single keys and runs of 9 (a run of 9 crosses a line of 8 wherever it starts), list
    lengths of every residue mod LINE (the trailing filler of front / back tasks varies with the rotation; asserted)."""
    ts = []
    n = len(DISTANCES)
    for r in range(n):
        d = DISTANCES[r:] + DISTANCES[:r]
        for a, b in ((1, 1), (9, 1), (1, 9), (9, 9), (2, 3)):
            ts.append(Task("front_r%d_a%d_b%d" % (r, a, b), *front_task(d + d[:r % 3], a, b, seed=r)))
            ts.append(Task("back_r%d_a%d_b%d" % (r, a, b), *back_task(d + d[:r % 3], a, b, seed=r)))
    rng = np.random.default_rng(93)
    for i in range(16):                                                      # list lengths of every residue, both sides
        ts.append(Task("res%d" % i, *random_task(rng, 300 + i % 8, 330 + (i * 3) % 8, 500, 2048)))
    return ts


def line_gaps(tasks):
    """Filler in front of each task's lists so that (q_lo, t_lo) mod LINE runs through every pair of residues, task after task."""
    gq, gt = [], []
    qo = to = 0
    for i, t in enumerate(tasks):
        a = (i % LINE - qo) % LINE; b = ((i // LINE) % LINE - to) % LINE
        gq.append(a); gt.append(b)
        qo += a + len(t.q); to += b + len(t.t)
    return gq, gt


def walk_trace(q, t, max_freq, max_diag=0, min_diag=0):
    """CompareLists<LocalTuple,SmallTuple> (CompareLists.h:9-146) restated in Python, recording how far each lower bound lay above ts and each upper bound below te.
    Returns (qi, ti, lower distances, upper distances); the tests hold its pairs against the oracle's."""
    Q = [int(x) & 0xFFFFF for x in q]; T = [int(x) & 0xFFFFF for x in t]
    QP = [int(x) >> 20 for x in q]; TP = [int(x) >> 20 for x in t]
    oq, ot, lows, ups = [], [], [], []
    nq, nt = len(Q), len(T)

    def emit(qi, ti):
        if max_diag != 0 and min_diag != 0:
            d = TP[ti] - QP[qi]
            if not (min_diag <= d <= max_diag):
                return
        oq.append(qi); ot.append(ti)
    if nq == 0 or nt == 0:
        return oq, ot, lows, ups
    qs, qe, ts, te = 0, nq - 1, 0, nt
    while True:
        while qs <= qe and Q[qs] < T[ts]:
            qs += 1
        if qs >= qe:
            break
        start_gap = (Q[qs] - T[ts]) & 0xFFFFF
        while qe > qs and te > ts and Q[qe] > T[te - 1]:
            qe -= 1
        end_gap = (T[te - 1] - Q[qe]) & 0xFFFFF
        if start_gap == 0 or start_gap > end_gap:
            ts_orig, qs_orig = ts, qs
            lo = ts
            while lo < te and T[lo] < Q[qs]:
                lo += 1
            lows.append(lo - ts)
            ts = lo
            if ts < te and T[ts] == Q[qs]:
                tsi = ts
                while tsi != te and Q[qs] == T[tsi]:
                    tsi += 1
                qs_start = qs
                while qs < qe and Q[qs + 1] == Q[qs]:
                    qs += 1
                if qs - qs_start < max_freq:
                    for ti in range(ts, tsi):
                        for qi in range(qs_start, qs + 1):
                            emit(qi, ti)
            raw = T[ts_orig]
            while ts < te and T[ts] == raw:
                ts += 1
            raw = Q[qs_orig]
            while qs < qe and Q[qs] == raw:
                qs += 1
        else:
            if not (te != nt and T[te - 1] == Q[qe]):
                hi = te
                while hi > ts and Q[qe] < T[hi - 1]:
                    hi -= 1
                ups.append(te - hi)
                te = hi
            te_start = te
            tei = te
            while tei > ts and T[tei - 1] == Q[qe]:
                tei -= 1
            if tei < te_start and te_start > 0:
                qe_start = qe
                while qe > qs and Q[qe] == Q[qe - 1]:
                    qe -= 1
                if qe_start - qe < max_freq:
                    for ti in range(tei, te_start):
                        for qi in range(qe, qe_start + 1):
                            emit(qi, ti)
            te = tei
        if not (qs < qe and ts < te):
            break
    return oq, ot, lows, ups
