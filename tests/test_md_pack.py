"""The MD section of the record buffer (lra_map_pack with LRA_PACK_MD, include/lra_hip.h) on the host: a hand-built pack with header word 10 = the MD bytes
and word 11 = 1 prints MD:Z in SAM records (format 's', after LI:i) and nowhere else; a pack whose words 10 and 11 are 0 unpacks as before."""
import ctypes as C
import re

import numpy as np

import test_parallel as TP

MD_TAG = re.compile(rb"\tMD:Z:[^\t\n]*")


def _with_md(packed, mds):
    """The pack with an MD section appended: header words 10 / 11, then md_off u64[nA + 1] | md bytes, each padded to 8 bytes."""
    hdr = np.frombuffer(packed[:128].tobytes(), np.int64).copy()
    nA = int(hdr[4])
    assert len(mds) == nA and hdr[5] == 0                                  # (no blocks section: the MD section follows the runs)
    text = b"".join(mds)
    off = np.zeros(nA + 1, np.uint64); off[1:] = np.cumsum([len(m) for m in mds])
    hdr[10] = len(text); hdr[11] = 1
    body = packed[128:].tobytes()
    out = hdr.tobytes() + body + off.tobytes() + text + b"\0" * ((-len(text)) % 8)
    return np.frombuffer(out, np.uint8).copy()


def _texts(fmt, packed, ordinals, reads):
    lib, m = TP._opts()
    m.printFormat = ord(fmt)
    return TP._texts(lib, m, ordinals, packed, reads)


def test_pack_with_md_prints_md_in_sam_only():
    ordinals = list(range(TP.N_READS))
    packed, reads = TP.pack(ordinals)
    nA = int(np.frombuffer(packed[:128].tobytes(), np.int64)[4])
    mds = [b"%d%s^AC%d" % (7 + a, b"ACGT"[a % 4:a % 4 + 1], a) for a in range(nA)]
    mds[0] = b""                                                           # an alignment without columns: "MD:Z:" with nothing behind it
    withmd = _with_md(packed, mds)
    plain = _texts("s", packed, ordinals, reads)
    got = _texts("s", withmd, ordinals, reads)
    assert got != plain
    n_tags = 0
    for p, g in zip(plain, got):
        assert MD_TAG.sub(b"", g) == p                                     # nothing else changes
        for line in g.split(b"\n"):
            tags = MD_TAG.findall(line)
            if not line:
                continue
            f = line.split(b"\t")
            if f[2] == b"*":
                assert not tags                                            # unaligned records (SimplePrintSAM) print no MD
                continue
            assert len(tags) == 1 and tags[0][6:] in mds
            assert line.index(b"\tMD:Z:") == line.index(b"\t", line.index(b"\tLI:i:") + 1)
            n_tags += 1
    assert n_tags >= TP.N_READS // 2
    for fmt in "pPb":                                                      # PrintPAF / PrintBed print no MD
        assert _texts(fmt, withmd, ordinals, reads) == _texts(fmt, packed, ordinals, reads)


def test_pack_without_md_unpacks_as_before():
    from lra_amd._lib import load_library
    ordinals = list(range(TP.N_READS))
    packed, reads = TP.pack(ordinals)
    hdr = np.frombuffer(packed[:128].tobytes(), np.int64)
    assert hdr[10] == 0 and hdr[11] == 0
    text = _texts("s", packed, ordinals, reads)
    assert not any(MD_TAG.search(t) for t in text)
    # a pack that announces an MD section it does not hold is refused, not read past its end
    bad = packed.copy()
    h = np.frombuffer(bad[:128].tobytes(), np.int64).copy(); h[10] = 1 << 20; h[11] = 1
    bad[:128] = np.frombuffer(h.tobytes(), np.uint8)
    snap = C.c_void_p()
    assert load_library().lra_map_unpack_host(C.c_void_p(bad.ctypes.data), C.c_uint64(bad.nbytes), C.byref(snap)) != 0
