"""The SV section of the record buffer (lra_map_pack with LRA_PACK_SVSIG, include/lra_hip.h) on the host: a hand-built pack with header word 12 = the
section's bytes and word 13 = 1 goes through lra_map_unpack_host and lra_map_svsig_host, which prints Alignment::Printsvsig's lines (Alignment.h:374-399)
read by read; the record text does not change; a pack without the section, or with a broken one, is refused."""
import ctypes as C

import numpy as np

import test_md_pack as MP
import test_parallel as TP

REC = np.dtype([("seq_off", "<u8"), ("t_start", "<u4"), ("len", "<u4"), ("kind", "<u4"), ("block", "<u4")])
INS, DEL = 0, 1
N = 128                                                                     # reads: enough for four host threads (one per 32 reads)


def _alignments(ordinals):
    """(read index, job, chrom) of every alignment of TP.pack(ordinals), in pack order."""
    out = []
    for r, i in enumerate(ordinals):
        for p, job in enumerate(TP._read(i)["jobs"]):
            out += [(r, p, a["chrom"]) for a in job]
    return out


def _sigs():
    """alignment -> [(t_start, kind, block, bases)], chosen by hand around reads 3 .. 7 (kinds of TP._read: 3 = two segments, 4 = two chains, the second on
    the reverse strand, 5 = flagged, 0 / 1 = one alignment on the forward / reverse strand), plus one per later single-alignment read."""
    alns = _alignments(range(N))
    at = {}
    for a, (r, p, _) in enumerate(alns):
        at.setdefault(r, []).append(a)
    sig = {a: [] for a in range(len(alns))}
    sig[at[4][0]] = [(1200, INS, 0, b"ACGTTGCAACGTTGCAACGTTGCAACGTTG"), (1300, DEL, 1, b"g" * 26)]
    sig[at[4][1]] = [(77, DEL, 0, b"NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN")]
    sig[at[5][0]] = [(5, INS, 0, b"T" * 30)]                               # the flagged read: its signature is not printed
    sig[at[7][0]] = [(4000000000, DEL, 1, b"ACgt")]                        # positions are unsigned 32-bit
    for r in range(12, N):
        if r % 6 in (0, 1):
            sig[at[r][0]] = [(1000 + r, INS if r % 2 else DEL, r % 2, b"ACGT"[r % 4:r % 4 + 1] * (26 + r))]
    return alns, sig


def _with_sv(packed, sig, n_aln, mutate=None):
    """The pack with an SV section appended: header words 12 / 13, then sig_off u64[nA + 1] | records | the sequences padded to 8 bytes."""
    hdr = np.frombuffer(packed[:128].tobytes(), np.int64).copy()
    assert int(hdr[4]) == n_aln and hdr[5] == 0
    off = np.zeros(n_aln + 1, np.uint64)
    off[1:] = np.cumsum([len(sig[a]) for a in range(n_aln)])
    recs = np.zeros(int(off[-1]), REC)
    seq = b""
    x = 0
    for a in range(n_aln):
        for t, kind, block, bases in sig[a]:
            recs[x] = (len(seq), t, len(bases), kind, block)
            seq += bases
            x += 1
    if mutate:
        mutate(off, recs)
    section = off.tobytes() + recs.tobytes() + seq + b"\0" * ((-len(seq)) % 8)
    hdr[12] = len(section); hdr[13] = 1
    return np.frombuffer(hdr.tobytes() + packed[128:].tobytes() + section, np.uint8).copy()


def _unpack(lib, packed):
    snap = C.c_void_p()
    rc = lib.lra_map_unpack_host(C.c_void_p(packed.ctypes.data), C.c_uint64(packed.nbytes), C.byref(snap))
    return rc, snap


def _svsig(lib, packed, n_threads):
    rc, snap = _unpack(lib, packed)
    assert rc == 0
    names = [b"read%d" % i for i in range(N)]
    text = C.c_char_p(); ln = C.c_uint64(0); roff = C.POINTER(C.c_uint64)()
    rc = lib.lra_map_svsig_host(snap, (C.c_char_p * N)(*names), (C.c_char_p * 2)(*TP.CHROM_NAMES), n_threads, C.byref(text), C.byref(ln), C.byref(roff))
    if rc:
        lib.lra_map_host_free(snap)
        return rc, None
    raw = C.string_at(text, ln.value)
    out = [raw[roff[i]:roff[i + 1]] for i in range(N)]
    assert roff[0] == 0 and roff[N] == ln.value
    lib.lra_map_host_free(snap)
    return 0, out


def test_pack_with_sv_section_prints_the_signature_lines():
    lib, m = TP._opts()
    packed, reads = TP.pack(list(range(N)))
    alns, sig = _sigs()
    withsv = _with_sv(packed, sig, len(alns))
    rc, got = _svsig(lib, withsv, 1)
    assert rc == 0
    # reads 3 .. 7 written out: none, three (two of the first chain's alignment, then the second chain's, which lies on chrB), the flagged read, none, one
    c4 = [TP.CHROM_NAMES[c] for r, p, c in alns if r == 4]
    c7 = [TP.CHROM_NAMES[c] for r, p, c in alns if r == 7]
    assert c4 == [b"chrA", b"chrB"] and c7 == [b"chrB"]
    assert got[3] == b""
    assert got[4] == (b"chrA\tread4\t1200\t1200\t30\tINS\tACGTTGCAACGTTGCAACGTTGCAACGTTG\n"
                      b"chrA\tread4\t1300\t1325\t26\tDEL\tgggggggggggggggggggggggggg\n"
                      b"chrB\tread4\t77\t117\t41\tDEL\tNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\n")
    assert got[5] == b"" and got[6] == b""
    assert got[7] == b"chrB\tread7\t4000000000\t4000000003\t4\tDEL\tACgt\n"
    # every read: the lines of its alignments in pack order
    want = [b""] * N
    for a, (r, p, c) in enumerate(alns):
        if r % 6 == 5:
            continue
        for t, kind, block, bases in sig[a]:
            want[r] += b"%s\tread%d\t%d\t%d\t%d\t%s\t%s\n" % (TP.CHROM_NAMES[c], r, t, t + len(bases) - 1 if kind == DEL else t, len(bases),
                                                            b"DEL" if kind == DEL else b"INS", bases)
    assert got == want and sum(1 for w in want if w) > 30
    rc, got4 = _svsig(lib, withsv, 4)
    assert rc == 0 and got4 == got
    # the record text is the one of the pack without the section, byte for byte, with an MD section in front of it as well
    plain = TP._texts(lib, m, list(range(N)), packed, reads)
    assert TP._texts(lib, m, list(range(N)), withsv, reads) == plain
    mds = [b"%dA" % a for a in range(len(alns))]
    withmd = MP._with_md(packed, mds)
    both = _with_sv(withmd, sig, len(alns))
    assert TP._texts(lib, m, list(range(N)), both, reads) == TP._texts(lib, m, list(range(N)), withmd, reads) != plain
    rc, gotb = _svsig(lib, both, 2)
    assert rc == 0 and gotb == got


def test_pack_without_sv_section_is_refused_by_the_printer():
    lib, m = TP._opts()
    packed, reads = TP.pack(list(range(N)))
    hdr = np.frombuffer(packed[:128].tobytes(), np.int64)
    assert hdr[12] == 0 and hdr[13] == 0
    rc, got = _svsig(lib, packed, 1)
    assert rc == -1 and got is None                                        # LRA_ERR_INVALID
    assert len(TP._texts(lib, m, list(range(N)), packed, reads)) == N      # and its records print as before


def test_broken_sv_sections_are_refused_at_unpack():
    lib, _ = TP._opts()
    packed, _ = TP.pack(list(range(N)))
    alns, sig = _sigs()
    nA = len(alns)
    good = _with_sv(packed, sig, nA)
    rc, snap = _unpack(lib, good)
    assert rc == 0
    lib.lra_map_host_free(snap)

    def refused(buf):
        rc, snap = _unpack(lib, buf)
        assert snap.value is None
        return rc == -1

    assert refused(good[:-8].copy())                                       # the section cut short
    assert refused(good[:len(packed) + 8 * (nA + 1) + 24].copy())          # ... inside its records
    def not_monotone(off, recs):
        off[1] = off[nA] + 1                                               # a step back from sig_off[1] to sig_off[2]
    bad = _with_sv(packed, sig, nA, not_monotone)
    o = np.frombuffer(bad[len(packed):len(packed) + 8 * (nA + 1)].tobytes(), np.uint64)
    assert (np.diff(o.astype(np.int64)) < 0).any()
    assert refused(bad)

    def seq_past_end(off, recs):
        recs[-1]["seq_off"] += 8
    assert refused(_with_sv(packed, sig, nA, seq_past_end))

    def first_not_zero(off, recs):
        off[0] = 1
    assert refused(_with_sv(packed, sig, nA, first_not_zero))

    def block_outside(off, recs):
        recs[0]["block"] = 2                                               # the alignments of TP.pack have three blocks: gaps behind blocks 0 and 1
    assert refused(_with_sv(packed, sig, nA, block_outside))

    def bad_kind(off, recs):
        recs[0]["kind"] = 2
    assert refused(_with_sv(packed, sig, nA, bad_kind))
