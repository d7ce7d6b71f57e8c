"""lra_bgzf_deflate_host (deflate.hip, the rules of bgzf_deflate.h): one batch of edge members and three seeded texts.  Every member round-trips through
zlib and through lra_bgzf_inflate_host, the concatenation walks as BGZF, no byte outside a member is written, and the output's size is held against
lra_amd.bgzf's zlib members on the same 65280-byte cuts."""
import zlib

import numpy as np
import pytest

from lra_amd import bgzf
import bgzf_deflate_cases as K


@pytest.fixture(scope="module")
def edge():
    items = K.edge_members()
    out, out_len, status = K.run_host([d for _, d in items])
    return items, out, out_len, status, K.members_of(out, out_len, status)


def test_edge_members_round_trip(edge):
    items, out, out_len, status, members = edge
    K.check_sentinels(out, out_len, status)
    good = []
    for (name, data), m, st in zip(items, members, status):
        if len(data) > K.IN_MAX:
            assert st != 0 and m is None, name                 # refused alone: its neighbours are members (below)
            continue
        assert st == 0, name
        K.check_member(m, data)
        good.append((m, data))
    assert len(good) == len(items) - 1
    K.inflate_host([m for m, _ in good], [d for _, d in good])
    cat = b"".join(m for m, _ in good)
    in_off, out_off = bgzf.blocks(cat)
    assert in_off[-1] == len(cat) and [b - a for a, b in zip(out_off, out_off[1:])] == [len(d) for _, d in good]


def test_empty_batch_and_bad_arguments():
    lib = K.load_library()
    assert lib.lra_bgzf_deflate_host(0, None, None, None, None, None) == 0
    assert lib.lra_bgzf_deflate_host(-1, None, None, None, None, None) != 0


def _member(edge, name):
    items, _, _, _, members = edge
    i = [n for n, _ in items].index(name)
    return members[i], items[i][1]


def _matches(blocks):
    return [t for b in blocks for t in b["tokens"] if isinstance(t, tuple)]


def test_empty_member(edge):
    m, _ = _member(edge, "len0")
    assert len(m) <= 40 and zlib.decompress(m, 31) == b""


def test_runs_and_periods(edge):
    for name, dists in [("one_byte_value", None), ("period3", None), ("period258", {258, 516})]:
        m, data = _member(edge, name)
        mt = _matches(K.deflate_blocks(m))
        assert len(m) < len(data) // 20, (name, len(m))
        assert max(l for l, _ in mt) == 258 and all(3 <= l <= 258 and 1 <= d <= 32768 for l, d in mt)
        if dists:
            assert {d for _, d in mt} <= dists
    m, _ = _member(edge, "one_byte_value")
    assert sum(l == 258 for l, _ in _matches(K.deflate_blocks(m))) >= 15        # chains of the longest match


def test_distance_limit(edge):
    m, _ = _member(edge, "dist32768")
    assert any(d == 32768 for _, d in _matches(K.deflate_blocks(m)))
    m, _ = _member(edge, "dist32769")
    mt = _matches(K.deflate_blocks(m))
    assert mt and all(d < 32768 for _, d in mt)                                  # the zeros between match; the far copy of x does not


def test_one_distance(edge):
    m, _ = _member(edge, "one_distance")
    blocks = K.deflate_blocks(m)
    mt = _matches(blocks)
    assert len(mt) > 40 and {d for _, d in mt} == {2048}
    assert all(b["type"] == 2 and sum(1 for n in b["dist_lengths"] if n) == 2 for b in blocks)   # the one distance and the symbol that completes the code


def test_fibonacci_counts_hit_the_length_limit(edge):
    """counts in Fibonacci proportion whose unrestricted Huffman tree is 16 deep inside one block: the code comes out 15 deep and complete"""
    import collections
    m, data = _member(edge, "fibonacci")
    blocks = K.deflate_blocks(m)
    assert len(blocks) == 1 and blocks[0]["type"] == 2 and not _matches(blocks)
    counts = collections.Counter(blocks[0]["tokens"])
    assert sorted(counts.values()) == K.FIB_COUNTS and K.huffman_depth(list(counts.values()) + [1]) == 16                   # (+ the end-of-block symbol)
    lens = [n for n in blocks[0]["lit_lengths"] if n]
    assert len(lens) == 17 and max(lens) == 15 and sum(2.0 ** -n for n in lens) == 1.0


def test_one_symbol_block(edge):
    """one byte value and no match: a dynamic block whose literal code is that value and the end of the block, one bit each, and whose distance code,
    with nothing to send, is completed to two codes of one bit (a decoder may insist on a complete code)"""
    m, data = _member(edge, "one_symbol")
    blocks = K.deflate_blocks(m)
    assert len(blocks) == 1 and blocks[0]["type"] == 2
    assert blocks[0]["tokens"] == [65] * 60
    lit = blocks[0]["lit_lengths"]
    assert {s: n for s, n in enumerate(lit) if n} == {65: 1, 256: 1}
    assert blocks[0]["dist_lengths"] == [1, 1]
    assert len(m) < 18 + 5 + len(data) + 8                                        # smaller than its stored form


def test_all_byte_values_and_code_length_runs(edge):
    m, _ = _member(edge, "all_bytes")
    blocks = K.deflate_blocks(m)
    assert blocks[0]["type"] == 2 and len([n for n in blocks[0]["lit_lengths"][:256] if n]) == 256
    used = {s for name in ("all_bytes", "one_byte_value", "fibonacci") for b in K.deflate_blocks(_member(edge, name)[0]) for s in b["cl_symbols"]}
    assert {16, 17, 18} <= used


def test_random_bytes_are_stored(edge):
    m, data = _member(edge, "random")
    assert len(data) == K.IN_MAX and len(m) <= K.SLOT
    assert all(b["type"] == 0 for b in K.deflate_blocks(m))


@pytest.fixture(scope="module")
def texts():
    out = {}
    for name, text in [("sam", K.sam_like()), ("paf", K.paf_like()), ("rep", K.repetitive())]:
        datas = K.cut(text)
        o, ln, st = K.run_host(datas)
        assert (st == 0).all()
        K.check_sentinels(o, ln, st)
        out[name] = (text, datas, K.members_of(o, ln, st))
    return out


def test_texts_round_trip(texts):
    import gzip
    for name, (text, datas, members) in texts.items():
        for m, d in zip(members, datas):
            K.check_member(m, d)
        K.inflate_host(members, datas)
        cat = b"".join(members)
        assert bgzf.blocks(cat)[1][-1] == len(text)
        assert gzip.decompress(cat + bgzf.EOF_BLOCK) == text


def test_compression_conditions(texts):
    size = {}
    for name, (text, _, members) in texts.items():
        ours = sum(len(m) for m in members)
        huff, l1, l6 = K.bgzf_size(text, 1, zlib.Z_HUFFMAN_ONLY), K.bgzf_size(text, 1), K.bgzf_size(text, 6)
        size[name] = (ours, huff, l1)
        print("%s: text %d  ours %d  huffman-only %d  level 1 %d  level 6 %d  ours/huffman %.4f  ours/level1 %.4f" %
              (name, len(text), ours, huff, l1, l6, ours / huff, ours / l1))
    for name in ("paf", "rep"):
        ours, huff, l1 = size[name]
        assert abs(ours - l1) < abs(ours - huff), (name, ours, huff, l1)
    ours, huff, _ = size["sam"]
    assert ours <= 1.03 * huff, (ours, huff)
