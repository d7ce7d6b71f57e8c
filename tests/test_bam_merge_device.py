"""lra_bam_merger on crafted run files (tests/bam_merge_cases.py; test_bam_merge_cases.py checks them on the CPU): the merged members inflate to Python's
stable sort of the runs' concatenation and are the members one call of the compress stage cuts from that stream, the .bai bytes equal
lra_bam_index_host's and tests/bai_text.py's builder, region queries through the index find the brute-force overlap set; small windows stream in
many rounds inside the budget and give the same bytes; ties keep run order, then file order; what the merger refuses it refuses cleanly."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_text as bt                                                             # noqa: E402
import bam_merge_cases as mc                                                      # noqa: E402
import bam_text                                                                   # noqa: E402

pytestmark = pytest.mark.gpu

REF_LEN = mc.REF_LEN
FIRST = 4711                                                                      # the file offset of the first member: a header of so many bytes in front
BUDGET = 1 << 32


@pytest.fixture(scope="module")
def cases():
    return mc.cases()


@pytest.fixture(scope="module")
def small(cases):
    """two small runs for the merger that must work after a refusal"""
    return cases["small"]["runs"]


def write_runs(d, runs, level=1, **kw):
    paths = []
    for i, run in enumerate(runs):
        p = os.path.join(str(d), "run%04d.bam" % i)
        with open(p, "wb") as f:
            f.write(mc.run_bytes(run, level, **kw))
        paths.append(p)
    return paths


def merge(ctx, paths, max_bytes=BUDGET, window=0, round_members=0, first=FIRST):
    """-> (pieces, bai, stats, (header bytes, reference lengths))"""
    from lra_amd.bam import BamMerger
    ctx.check(ctx.lib.lra_bgzf_compress_set_round(ctx.h, int(round_members)))
    m = BamMerger(ctx, paths, max_bytes, first, window)
    try:
        head = m.header()
        pieces = list(m.pieces())
        bai = m.index()
        return pieces, bai, m.stats(), head
    finally:
        m.close()
        ctx.check(ctx.lib.lra_bgzf_compress_set_round(ctx.h, 0))


def check(ctx, runs, pieces, bai, rng=None, queries=0, ref_len=REF_LEN):
    from lra_amd import bgzf, deflate
    from lra_amd.bam import index_host
    data = b"".join(pieces)
    want = b"".join(mc.merged(runs))
    got = bam_text.inflate(data)
    if got != want:
        k = next(i for i in range(min(len(got), len(want))) if got[i] != want[i]) if len(got) == len(want) else -1
        raise AssertionError("the merged stream differs: %d / %d bytes, first at %d" % (len(got), len(want), k))
    assert data == deflate.compress_device(ctx, want)[0], "the members of one call of the compress stage on the merged stream"
    member_off = bgzf.blocks(data)[0] if data else [0]
    assert len(member_off) - 1 == (len(want) + bt.MEMBER - 1) // bt.MEMBER
    assert bai == index_host(want, ref_len, member_off, FIRST)
    assert bai == bt.build(want, len(ref_len), member_off, FIRST)
    if queries:
        hit = bt.check_queries(rng, b"\0" * FIRST + data + mc.EOF_BLOCK, bai, want, ref_len, queries)
        assert hit > queries // 8
    return data


def works_afterwards(ctx, tmp_path, small):
    d = tmp_path / "after"
    d.mkdir(exist_ok=True)
    pieces, bai, _, _ = merge(ctx, write_runs(d, small))
    check(ctx, small, pieces, bai)


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_consecutive_slices(ctx, cases, tmp_path, k):
    runs = cases["consecutive_%d" % k]["runs"]
    pieces, bai, st, (head, ref_len) = merge(ctx, write_runs(tmp_path, runs))
    assert head == mc.header_bytes() and ref_len == REF_LEN
    check(ctx, runs, pieces, bai, np.random.default_rng(k), 200)
    assert st["records"] == 5000 and st["bytes"] == sum(len(r) for run in runs for r in run) and len(st["refills"]) == k


def test_streaming(ctx, cases, tmp_path):
    c = cases["streaming"]
    paths = write_runs(tmp_path, c["runs"], c["level"])
    whole, bai0, st0, _ = merge(ctx, paths)
    data = check(ctx, c["runs"], whole, bai0)
    budget = 64 << 20
    pieces, bai, st, _ = merge(ctx, paths, budget, c["window"])
    print("rounds", st["rounds"], "refills", st["refills"], "peak", st["peak_device_bytes"], "against one window each:", st0["rounds"], st0["peak_device_bytes"])
    assert st["rounds"] >= 10 and all(n >= 1 for n in st["refills"]) and st["peak_device_bytes"] <= budget
    assert b"".join(pieces) == data and bai == bai0
    # a round of 7 members in the compress stage: the same bytes in more pieces
    p7, b7, _, _ = merge(ctx, paths, budget, c["window"], round_members=7)
    assert len(p7) > len(whole) and all(len(bam_text.inflate(p)) <= 7 * bt.MEMBER for p in p7)
    assert b"".join(p7) == data and b7 == bai0


@pytest.mark.parametrize("name", ["one_key", "straddle"])
def test_ties_keep_run_order_then_file_order(ctx, cases, tmp_path, name):
    c = cases[name]
    paths = write_runs(tmp_path, c["runs"], c["level"])
    pieces, bai, st, _ = merge(ctx, paths, 64 << 20, c["window"])
    check(ctx, c["runs"], pieces, bai)
    assert st["rounds"] >= 10 and all(n >= 1 for n in st["refills"])
    if name == "one_key":                                                         # one key: the output is run 0, run 1, run 2, each in file order
        assert bam_text.inflate(b"".join(pieces)) == b"".join(r for run in c["runs"] for r in run)


def test_a_record_larger_than_the_window(ctx, cases, tmp_path, small):
    from lra_amd._lib import LraError
    from lra_amd.bam import BamMerger
    recs = mc.fixture_records()
    big = [r for r in recs if len(r) > 4 * mc.WINDOW]
    assert len(big) >= 2, "the 65535-op record and the CG:B:I record"
    runs = cases["larger"]["runs"]                                                # both runs small but for the large records in the second
    assert all(b in runs[1] for b in big)
    paths = write_runs(tmp_path, runs, 0)
    pieces, bai, st, _ = merge(ctx, paths, BUDGET, mc.WINDOW)
    check(ctx, runs, pieces, bai)
    peak = st["peak_device_bytes"]
    m = BamMerger(ctx, paths, peak - 1, FIRST, mc.WINDOW)                         # a byte less than the grown window needs
    with pytest.raises(LraError, match=r"error -3: .*needs (\d+) bytes.*budget is %d" % (peak - 1)) as e:
        list(m.pieces())
    assert int(re.search(r"needs (\d+) bytes", str(e.value)).group(1)) > peak - 1
    with pytest.raises(LraError, match="error -3"):                               # the merger only refuses now
        m.next()
    m.close()
    works_afterwards(ctx, tmp_path, small)


def test_shapes_of_files(ctx, cases, tmp_path):
    a, _, b, c, d = cases["shapes"]["runs"]
    rng = np.random.default_rng(5)
    n_c = sum(len(r) for r in c)
    paths = []
    shapes = [
        mc.run_bytes(a, 1),
        mc.run_bytes([], 1),                                                      # header and EOF only, between two others
        mc.run_bytes(b, 1, header_member=False),                                  # the records begin in the header's member
        mc.run_bytes(c, 1, cuts=sorted({int(x) for x in rng.integers(1, n_c, 40)} | set(range(60000, n_c, 60000)))),   # uneven members, cut inside records
        mc.run_bytes(d, 1, eof=False),                                            # no EOF member
    ]
    for i, s in enumerate(shapes):
        paths.append(str(tmp_path / ("s%d.bam" % i)))
        open(paths[-1], "wb").write(s)
    runs = [a, [], b, c, d]
    pieces, bai, st, _ = merge(ctx, paths)
    check(ctx, runs, pieces, bai, np.random.default_rng(6), 50)
    pieces, bai, st, _ = merge(ctx, paths, 64 << 20, mc.WINDOW)
    check(ctx, runs, pieces, bai)
    assert st["refills"][1] == 0


def refused(ctx, paths, match, at_create=False, **kw):
    from lra_amd._lib import LraError
    from lra_amd.bam import BamMerger
    if at_create:
        with pytest.raises(LraError, match=match):
            BamMerger(ctx, paths, BUDGET, FIRST, **kw)
        return
    m = BamMerger(ctx, paths, BUDGET, FIRST, **kw)
    try:
        with pytest.raises(LraError, match=match):
            list(m.pieces())
        with pytest.raises(LraError, match=match):                                # and again: a merger that failed only refuses
            m.index()
    finally:
        m.close()


def test_what_the_merger_refuses(ctx, tmp_path, small):
    from lra_amd._lib import LraError
    from lra_amd.bam import BamMerger
    good = write_runs(tmp_path, small)
    # two records swapped: the ordinal of the one that sorts in front of its neighbour
    run = list(small[1])
    i = next(j for j in range(40, len(run) - 1) if bt.sort_key(run[j]) != bt.sort_key(run[j + 1]))
    run[i], run[i + 1] = run[i + 1], run[i]
    p = str(tmp_path / "swapped.bam")
    open(p, "wb").write(mc.run_bytes(run))
    refused(ctx, [good[0], p], r"swapped\.bam: record %d " % (i + 1))
    works_afterwards(ctx, tmp_path, small)
    # a reference table that differs in one length
    p = str(tmp_path / "otherlen.bam")
    open(p, "wb").write(mc.run_bytes(small[1], ref_len=[400_000, 300_001, 250_000]))
    refused(ctx, [good[0], p], r"otherlen\.bam: reference 1 \(chr2\) has length 300001", at_create=True)
    # a refID outside the table (both headers name two references)
    assert any(bt.sort_key(r)[0] == 2 for r in small[1])
    two = [str(tmp_path / "two0.bam"), str(tmp_path / "two1.bam")]
    for q, run in zip(two, small):
        open(q, "wb").write(mc.run_bytes([r for r in run if bt.sort_key(r)[0] != 2] if q == two[0] else run, ref_len=REF_LEN[:2]))
    refused(ctx, two, r"two1\.bam: .*names a reference outside \[-1, 2\)")
    works_afterwards(ctx, tmp_path, small)
    # a member with a broken CRC
    from lra_amd import bgzf
    raw = bytearray(mc.run_bytes(small[1]))
    in_off, _ = bgzf.blocks(bytes(raw))
    raw[in_off[2] - 8] ^= 0x40                                                    # the CRC-32 of the first member of records
    p = str(tmp_path / "crc.bam")
    open(p, "wb").write(bytes(raw))
    refused(ctx, [good[0], p], r"crc\.bam: a bad BGZF block at compressed offset %d \(a CRC-32 mismatch\)" % in_off[1])
    works_afterwards(ctx, tmp_path, small)
    # the number of runs
    refused(ctx, [], "1 .. 256", at_create=True)
    refused(ctx, [good[0]] * 257, "1 .. 256", at_create=True)
    # index before the last piece
    m = BamMerger(ctx, good, BUDGET, FIRST)
    with pytest.raises(LraError, match="last piece"):
        m.index()
    pieces = list(m.pieces())
    check(ctx, small, pieces, m.index())
    m.close()
    # a reference BAI cannot address: the members come, the index does not
    long_ref = [(1 << 29) + 1, 300_000, 250_000]
    lp = [str(tmp_path / "long0.bam"), str(tmp_path / "long1.bam")]
    for q, run in zip(lp, small):
        open(q, "wb").write(mc.run_bytes(run, ref_len=long_ref))
    m = BamMerger(ctx, lp, BUDGET, FIRST)
    assert bam_text.inflate(b"".join(m.pieces())) == b"".join(mc.merged(small))
    with pytest.raises(LraError, match="2\\^29"):
        m.index()
    m.close()
    works_afterwards(ctx, tmp_path, small)
