"""The exports of lra_sv_combine exist after build(), with the ABI number unchanged; its ctypes structures have the sizes of include/lra_hip.h's structs;
the pass's sink is no export (no compute calls here)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lra_sv_combine_" + k for k in ("create", "header", "set_mask", "all", "region", "next", "stats", "destroy")]


def test_exports_and_structures():
    import __graft_entry__ as g
    g.build()
    from lra_amd._lib import library_path, SYMBOLS, load_library
    from lra_amd import bam
    lib = ctypes.CDLL(library_path())
    for n in NAMES:
        assert hasattr(lib, n), "missing export: " + n
        assert n in SYMBOLS
    assert load_library().lra_abi_version() == 9
    assert not hasattr(lib, "lra_bam_svcalls_set_sink")
    exported = subprocess.run(["nm", "-D", "--defined-only", library_path()], capture_output=True, text=True, check=True).stdout
    assert "set_sink" not in exported and "lra_sv_combine_next" in exported
    # 12 words, window_bytes, aligner; svcalls_row's 64 bytes with hap and cls in its pad; 4 words behind 4 x 8 bytes; 10 counts, 5 times, two passes' stats
    assert ctypes.sizeof(bam.SvCombineOpts) == 64 and bam.SVCOMBINE_ROW_DTYPE.itemsize == 64 == bam.SVCALLS_ROW_DTYPE.itemsize
    assert bam.SVCOMBINE_ROW_DTYPE.fields["hap"][1] == bam.SVCALLS_ROW_DTYPE.fields["pad"][1] and bam.SVCOMBINE_ROW_DTYPE.fields["cls"][1] == 59
    assert ctypes.sizeof(bam.SvCombinePiece) == 48
    assert ctypes.sizeof(bam.SvCombineStats) == 8 * 15 + 2 * ctypes.sizeof(bam.SvCallsStats)
    assert [k for k, _ in bam.SVCOMBINE_FILES] == [("maternal", "INS", "het"), ("maternal", "DEL", "het"), ("paternal", "INS", "het"), ("paternal", "DEL", "het"),
                                                   ("maternal", "INS", "hom"), ("maternal", "DEL", "hom")]
    assert bam.parse_frac("3/10") == (3, 10) and bam.parse_frac("1/1") == (1, 1)
    for bad in ("0/7", "4/3", "3", "a/b", "1/0"):
        try:
            bam.parse_frac(bad)
        except ValueError:
            continue
        raise AssertionError(bad)
