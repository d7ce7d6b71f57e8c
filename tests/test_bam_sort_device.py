"""lra_bam_sorter on crafted record streams (no mapper): the sorted members inflate to Python's stable sort of the records, the .bai bytes equal
lra_bam_index_host's and tests/bai_text.py's builder, region queries through the index find the brute-force overlap set, the budget holds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_text as bt                                                             # noqa: E402
import bam_text                                                                   # noqa: E402

pytestmark = pytest.mark.gpu

REF_LEN = [400_000, 300_000, 250_000]
FIRST = 4711                                                                      # the file offset of the first member: a header of so many bytes in front
GUARD = 69                                                                        # bytes in front of the first record in the caller's stream (odd: the records start unaligned)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def records():
    """5000 records on refID -1, 0, 1, 2 with many ties, names of 1 .. 254 bytes, 0 .. 300 ops; behind them the special ones"""
    rng = np.random.default_rng(42)
    recs = bt.random_records(rng, 4994, REF_LEN)
    recs.append(bt.make_record(0, 77, 0, b"x", [(3 << 4) | (7 if k % 3 else 2) for k in range(65535)], 100))      # the most ops n_cigar_op holds: 1024 steps of its wave
    recs.append(bt.cg_record(1, 500, 16, b"cgform", [(2 << 4) | (7 if k % 2 else 1) for k in range(70000)], 70000))  # 70000 ops: the CG:B:I form, > 65280 bytes
    recs.append(bt.make_record(2, 10, 0, b"n" * 254, [(100 << 4) | 0], 4000))                                     # > 4096 bytes
    recs.append(bt.make_record(2, 10, 16, b"m", [(100 << 4) | 0], 50_000))                                        # > 65280 bytes
    recs.append(bt.make_record(-1, -1, 4, b"u", [], 3000))
    recs.append(bt.make_record(0, 0, 0, b"z", [], 0))                                                              # no ops: one base of span
    assert len(recs) == 5000
    names = {r[12] - 1 for r in recs}
    assert 1 in names and 254 in names and {bt.sort_key(r)[0] for r in recs} == {0, 1, 2, 0xffffffff}
    return recs


def upload(ctx, recs):
    """-> (guarded stream tensor, guarded starts tensor): the records start GUARD bytes into the stream; 0xA5 bytes / words around both arrays"""
    import torch
    data = b"".join(recs)
    buf = np.frombuffer(b"\xa5" * GUARD + data + b"\xa5" * 64, np.uint8)
    g = np.array([0xa5a5a5a5a5a5a5a5], np.uint64)
    starts = np.concatenate([g, (GUARD + np.concatenate([[0], np.cumsum([len(r) for r in recs], dtype=np.int64)])).astype(np.uint64), g])
    return torch.from_numpy(buf.copy()).to(ctx.device), torch.from_numpy(starts.view(np.int64).copy()).to(ctx.device), len(data)


def guards_intact(stream, starts, n_bytes, recs):
    s, t = stream.cpu().numpy(), starts.cpu().numpy().view(np.uint64)
    assert bytes(s[:GUARD]) == b"\xa5" * GUARD and bytes(s[GUARD + n_bytes:]) == b"\xa5" * 64 and bytes(s[GUARD:GUARD + n_bytes]) == b"".join(recs)
    assert t[0] == t[-1] == 0xa5a5a5a5a5a5a5a5 and int(t[1]) == GUARD and int(t[-2]) == GUARD + n_bytes


def add_all(ctx, sorter, recs, cuts):
    """the records in len(cuts) + 1 add calls; the caller's arrays are checked afterwards"""
    held = []
    for a, b in zip([0] + cuts, cuts + [len(recs)]):
        part = recs[a:b]
        stream, starts, nb = upload(ctx, part)
        sorter.add(stream, starts[1:-1])
        held.append((stream, starts, nb, part))
    return held


def run(ctx, recs, cuts=(), round_members=0):
    from lra_amd.bam import BamSorter
    ctx.check(ctx.lib.lra_bgzf_compress_set_round(ctx.h, int(round_members)))
    s = BamSorter(ctx, 1 << 32)
    try:
        held = add_all(ctx, s, recs, list(cuts))
        assert s.held() == (len(recs), sum(len(r) for r in recs))
        s.finish(FIRST, REF_LEN)
        pieces = list(s.pieces())
        bai = s.index()
        assert s.held() == (0, 0)
        for h in held:
            guards_intact(*h)
        return pieces, bai
    finally:
        s.close()
        ctx.check(ctx.lib.lra_bgzf_compress_set_round(ctx.h, 0))


def check(ctx, recs, pieces, bai, rng=None, queries=0):
    from lra_amd import bgzf
    from lra_amd.bam import index_host
    data = b"".join(pieces)
    want = b"".join(sorted(recs, key=bt.sort_key))
    got = bam_text.inflate(data)
    if got != want:
        k = next(i for i in range(min(len(got), len(want))) if got[i] != want[i]) if len(got) == len(want) else -1
        raise AssertionError("the sorted stream differs: %d / %d bytes, first at %d" % (len(got), len(want), k))
    member_off = bgzf.blocks(data)[0] if data else [0]
    assert len(member_off) - 1 == (len(want) + bt.MEMBER - 1) // bt.MEMBER
    assert bai == index_host(want, REF_LEN, member_off, FIRST)
    assert bai == bt.build(want, len(REF_LEN), member_off, FIRST)
    if queries:
        hit = bt.check_queries(rng, b"\0" * FIRST + data + EOF_BLOCK, bai, want, REF_LEN, queries)
        assert hit > queries // 8
    return data


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65])
def test_small_counts(ctx, records, n):
    recs = records[:n]
    pieces, bai = run(ctx, recs)
    check(ctx, recs, pieces, bai)
    assert len(pieces) == (1 if n else 0)


def test_5000_records_adds_rounds_index_and_queries(ctx, records):
    from lra_amd import deflate
    starts = np.concatenate([[0], np.cumsum([len(r) for r in records])]) + GUARD
    assert {int(x) % 16 for x in starts[:-1]} == set(range(16)), "every start alignment"
    one, bai = run(ctx, records)
    data = check(ctx, records, one, bai, np.random.default_rng(1), 200)
    assert len(one) == 1
    # two and three add calls: the same bytes (the ties keep the order in which the records were added)
    for cuts in ((2100,), (64, 3000)):
        p, b = run(ctx, records, cuts)
        assert b"".join(p) == data and b == bai
    # a small round: several pieces, the members of one call; and the members one call of the stream stage cuts
    p, b = run(ctx, records, (), round_members=7)
    assert len(p) == -(-len(bam_text.inflate(data)) // (7 * bt.MEMBER)) > 3 and b"".join(p) == data and b == bai
    assert deflate.compress_device(ctx, b"".join(sorted(records, key=bt.sort_key)))[0] == data
    # records of one (refID, bin) that are not neighbours make several chunks of that bin
    refs, n_no_coor = bt.parse(bai)
    assert n_no_coor == sum(bt.sort_key(r)[0] == 0xffffffff for r in records)
    assert any(len(ch) > 1 for R in refs for ch in R["bins"].values())


def test_budget(ctx, records):
    from lra_amd.bam import BamSorter, SorterFull
    from lra_amd._lib import LraError
    batches = [records[0:200], records[200:400], records[400:600]]
    up = [upload(ctx, b) for b in batches]
    ctx.check(ctx.lib.lra_bgzf_compress_set_round(ctx.h, 2))
    try:
        def fit(budget):
            s = BamSorter(ctx, budget)
            try:
                for k, (stream, starts, _) in enumerate(up):
                    try:
                        s.add(stream, starts[1:-1])
                    except SorterFull:
                        return k
                return 3
            finally:
                s.close()
        lo, hi = 1, 1 << 30                                                       # the smallest budget that takes all three
        assert fit(hi) == 3 and fit(lo) == 0
        while lo + 1 < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if fit(mid) == 3 else (mid, hi)
        budget = hi - 1
        assert fit(budget) == 2, "a byte less holds two of the three batches"
        s = BamSorter(ctx, budget)
        s.add(up[0][0], up[0][1][1:-1])
        s.add(up[1][0], up[1][1][1:-1])
        held = s.held()
        assert held == (400, sum(len(r) for r in batches[0] + batches[1]))
        with pytest.raises(SorterFull):
            s.add(up[2][0], up[2][1][1:-1])
        assert s.held() == held
        with pytest.raises(LraError):
            s.index()                                                             # nothing finished
        s.finish(FIRST, REF_LEN)
        with pytest.raises(LraError):
            s.index()                                                             # before the last piece
        with pytest.raises(LraError):
            s.add(up[2][0], up[2][1][1:-1])                                       # a finished run is taken first
        first = next(s.pieces())
        pieces = [first] + list(s.pieces())
        check(ctx, batches[0] + batches[1], pieces, s.index())
        assert s.held() == (0, 0)
        s.add(up[2][0], up[2][1][1:-1])                                           # the second run
        s.finish(FIRST, REF_LEN)
        pieces = list(s.pieces())
        check(ctx, batches[2], pieces, s.index())
        s.close()
        for (stream, starts, nb), b in zip(up, batches):
            guards_intact(stream, starts, nb, b)
    finally:
        ctx.check(ctx.lib.lra_bgzf_compress_set_round(ctx.h, 0))


def test_what_the_sorter_refuses(ctx, records):
    from lra_amd.bam import BamSorter
    from lra_amd._lib import LraError
    s = BamSorter(ctx, 1 << 30)
    assert any(bt.sort_key(r)[0] in (1, 2) for r in records[:10])
    stream, starts, _ = upload(ctx, records[:10])
    s.add(stream, starts[1:-1])
    with pytest.raises(LraError):
        s.finish(0, REF_LEN[:1])                                                  # a record names reference 1 or 2: outside the table
    assert s.held()[0] == 10                                                      # nothing changed
    with pytest.raises(LraError):
        s.next()
    s.finish(0, [1 << 30, 1 << 20, 1 << 20])                                      # a reference BAI cannot address: the members come, the index does not
    data = b"".join(s.pieces())
    assert bam_text.inflate(data) == b"".join(sorted(records[:10], key=bt.sort_key))
    with pytest.raises(LraError, match="2\\^29"):
        s.index()
    assert s.held() == (0, 0)
    s.close()
