"""lra_bam_header: the head of a BAM file (magic, header text, reference table) decoded by tests/bam_text.py and held against its inputs.  Host code only."""
import ctypes as C

import pytest

import bam_text


def _lib():
    import __graft_entry__ as g
    g.build()
    from lra_amd._lib import load_library
    return load_library()


CASES = [
    (b"", [], [0]),                                                          # no chromosome, an empty text
    (b"@PG\tID:lra\n", [b"c"], [0, 1]),                                      # a 1-byte name, a 1-base chromosome
    (b"@PG\tID:lra\tPN:lra\n@SQ\tSN:chrA\tLN:300000\n@SQ\tSN:b\tLN:7\n@SQ\tSN:chr_with_a_longer_name.1\tLN:2147000000\n",
     [b"chrA", b"b", b"chr_with_a_longer_name.1"], [0, 300_000, 300_007, 300_007 + 2_147_000_000]),
    (b"", [b"x", b"y", b"z"], [5, 5, 6, 106]),                               # an empty chromosome, an empty text
]


@pytest.mark.parametrize("text,names,pos", CASES)
def test_header_decodes_to_its_inputs(text, names, pos):
    _lib()
    from lra_amd import mapread
    raw = mapread.bam_header(text, names, pos)
    got_text, refs, end = bam_text.parse_header(raw)
    assert end == len(raw) == 4 + 4 + len(text) + 4 + sum(4 + len(n) + 1 + 4 for n in names)
    assert got_text == text
    assert [r[0] for r in refs] == names and [r[1] for r in refs] == [pos[i + 1] - pos[i] for i in range(len(names))]
    assert bam_text.records(raw, refs, end) == []


def test_header_sizing_call_and_bad_arguments():
    lib = _lib()
    names = (C.c_char_p * 2)(b"a", b"bb")
    pos = (C.c_uint64 * 3)(0, 10, 30)
    ln = C.c_uint64(0)
    assert lib.lra_bam_header(b"xy", 2, 2, names, pos, None, 0, C.byref(ln)) == 0 and ln.value == 4 + 4 + 2 + 4 + (4 + 2 + 4) + (4 + 3 + 4)
    buf = (C.c_uint8 * 64)(*([0xA5] * 64))
    assert lib.lra_bam_header(b"xy", 2, 2, names, pos, buf, ln.value - 1, C.byref(ln)) != 0          # too small: nothing is written
    assert bytes(buf) == b"\xa5" * 64
    assert lib.lra_bam_header(b"xy", 2, 2, names, pos, buf, ln.value, C.byref(ln)) == 0
    assert bytes(buf[ln.value:]) == b"\xa5" * (64 - ln.value) and bam_text.parse_header(bytes(buf[:ln.value]))[1] == [(b"a", 10), (b"bb", 20)]
    assert lib.lra_bam_header(b"xy", 2, 2, names, pos, buf, 64, None) != 0
    assert lib.lra_bam_header(None, 2, 0, None, None, None, 0, C.byref(ln)) != 0
    assert lib.lra_bam_header(b"", 0, 2, None, pos, None, 0, C.byref(ln)) != 0
    back = (C.c_uint64 * 3)(0, 10, 5)                                       # a chromosome that ends in front of its start
    assert lib.lra_bam_header(b"", 0, 2, names, back, None, 0, C.byref(ln)) != 0
    big = (C.c_uint64 * 3)(0, 10, 10 + (1 << 31))                           # l_ref is an int32
    assert lib.lra_bam_header(b"", 0, 2, names, big, None, 0, C.byref(ln)) != 0
