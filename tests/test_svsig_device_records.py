"""lra_map_records_device with LRA_PACK_SVSIG: the SV signature text built on the device (svsig.hip + svsig_text.hip) and returned by
lra_map_records_device_svsig, byte for byte against lra_map_svsig_host on a LRA_PACK_SVSIG snapshot of the same result, for the -ONT and -CCS drivers and
tools/map_files.py --device-records -SV (GPU)."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from lra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INS, DEL = 0, 1
SVSIG, MD, BLOCKS = 4, 2, 1                                               # LRA_PACK_SVSIG, LRA_PACK_MD, LRA_PACK_BLOCKS
INVALID = -1                                                              # LRA_ERR_INVALID


def _batch(err):
    """test_svsig's planted reads (an indel of 40-300 bases in the middle of 14 reads of 6 kb, of both kinds on both strands) behind four plain ones, a read
    whose halves come from two chromosomes (two alignments) and one that cannot align."""
    from test_svsig import planted_reads, CH
    genome, reads = planted_reads(err, n_plain=4)
    rng = np.random.default_rng(9)
    sim = lambda a, n, rev=False: synth.simulate_read(rng, genome[a:a + n + 1], n, err * 0.8, (30, 35, 35), rev)[0]
    reads.append(np.concatenate([sim(CH[0] + 120_000, 4500), sim(CH[1] + 200_000, 4500, True)]).tobytes())
    reads.append(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 2500)].tobytes())
    return genome, reads


def _mapper(ctx, form, genome):
    from lra_amd import mapread
    from test_svsig import CH, CHROMS
    if form == "ccs":
        return mapread.HighAccMapper(ctx, genome, None, None, CHROMS, CH, "ccs")
    opts = mapread.LowAccOptions()
    ik, ip = synth.build_global_index(genome, opts.globalK, opts.globalW, 100)
    return mapread.LowAccMapper(ctx, genome, ik, ip, CHROMS, CH, opts)


def _set_len(m, n):
    if hasattr(m, "opts"):
        m.opts = dataclasses.replace(m.opts, svsigLen=n)
    else:
        m.svsigLen = n


def _device(m, res, args, flags, fmt):
    """lra_map_records_device with `flags` -> (rc, the records per read)"""
    from lra_amd import mapread
    m.copts.printFormat = ord(fmt)
    mapread.set_svsig_len(m.ctx, m.svsig_len)
    text = C.c_void_p(); ln = C.c_uint64(0); roff = C.POINTER(C.c_uint64)()
    rc = m.ctx.lib.lra_map_records_device(m.ctx.h, C.byref(res), C.byref(m.copts), args["names"], args["reads"], args["quals"], args["lens"], args["chroms"], None, None, None,
                                          flags, 0, C.byref(text), C.byref(ln), C.byref(roff))
    if rc:
        return rc, None
    raw = C.string_at(text, ln.value) if ln.value else b""
    assert roff[0] == 0 and roff[args["n"]] == ln.value
    return rc, [raw[roff[i]:roff[i + 1]] for i in range(args["n"])]


def _accessor(m, n):
    """lra_map_records_device_svsig -> (rc, text, len, rec_off)"""
    text = C.c_void_p(); ln = C.c_uint64(0); roff = C.POINTER(C.c_uint64)()
    rc = m.ctx.lib.lra_map_records_device_svsig(m.ctx.h, C.byref(text), C.byref(ln), C.byref(roff))
    if rc:
        return rc, None, None, None
    return rc, (C.string_at(text, ln.value) if ln.value else b""), int(ln.value), [int(roff[i]) for i in range(n + 1)]


def _host(m, res, names):
    """lra_map_svsig_host on a LRA_PACK_SVSIG snapshot of the result -> (text, len, rec_off)"""
    lib = m.ctx.lib
    n = len(names)
    snap = m.snapshot(res, md=False, svsig=True)
    text = C.c_char_p(); ln = C.c_uint64(0); roff = C.POINTER(C.c_uint64)()
    rc = lib.lra_map_svsig_host(snap, (C.c_char_p * n)(*names), (C.c_char_p * len(m.chrom_names))(*m.chrom_names), 2, C.byref(text), C.byref(ln), C.byref(roff))
    try:
        assert rc == 0
        return (C.string_at(text, ln.value) if ln.value else b""), int(ln.value), [int(roff[i]) for i in range(n + 1)]
    finally:
        lib.lra_map_host_free(snap)


def _same(got, want, what):
    """per-read texts equal; else the place of the first difference, not two 40 KB records"""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            at = next((k for k in range(min(len(g), len(w))) if g[k] != w[k]), min(len(g), len(w)))
            raise AssertionError("%r read %d: %d / %d bytes, first difference at %d: %r / %r" % (what, i, len(g), len(w), at, g[max(at - 40, 0):at + 40], w[max(at - 40, 0):at + 40]))
    assert len(got) == len(want)


def _kinds_by_strand(m, d, res, reads, genome, min_len):
    """{(kind, strand)} of the signatures in the result's final blocks (test_svsig's restatement of the rule), and the alignments per read"""
    from lra_amd import mapread
    from test_svsig import expected_signatures
    na = max(int(res.num_aln), 1)
    jo = d["job_aln_off"]
    gb = genome.tobytes()
    seen, per_read = set(), []
    for r in range(len(reads)):
        per_read.append(int(jo[(r + 1) * na]) - int(jo[r * na]))
        for a in range(int(jo[r * na]), int(jo[(r + 1) * na])):
            ci = int(d["chrom"][a])
            rd = reads[r] if not d["strand"][a] else mapread.create_rc(reads[r])
            b = d["blocks"][int(d["block_off"][a]):int(d["block_off"][a + 1])]
            seen |= {(s[1], int(d["strand"][a])) for s in expected_signatures(rd, gb[m.chrom_pos[ci]:m.chrom_pos[ci + 1]], b, min_len)}
    return seen, per_read


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["ont", "ccs"])
def test_device_signatures_equal_the_host_printer(ctx, form):
    import torch
    from lra_amd import seed
    from lra_amd.context import Context
    genome, reads = _batch(0.01 if form == "ccs" else 0.10)
    n = len(reads)
    names = [b"read/%d" % i if i % 2 else b"r%d" % i for i in range(n)]
    quals = [bytes([40 + i % 30]) * len(r) for i, r in enumerate(reads)]
    m = _mapper(ctx, form, genome)
    lib = ctx.lib
    try:
        # the accessor before any call on a context
        c2 = Context(0)
        try:
            assert c2.lib.lra_map_records_device_svsig(c2.h, None, C.byref(C.c_uint64(0)), None) == INVALID
        finally:
            c2.close()
        res = m.align(seed.ReadBatch(ctx, reads))
        d = m.fetch(res)
        seen, per_read = _kinds_by_strand(m, d, res, reads, genome, 25)
        assert seen == {(INS, 0), (INS, 1), (DEL, 0), (DEL, 1)}, seen     # equality below is not vacuous
        assert max(per_read) >= 2 and per_read[-1] == 0, per_read          # a read with two alignments, an unaligned read
        args = m.record_args(names, reads, quals)
        _set_len(m, 25)
        want = _host(m, res, names)
        assert want[1] > 0 and want[0].count(b"\tINS\t") >= 2 and want[0].count(b"\tDEL\t") >= 2
        for fmt in "sPapb":
            rc, plain = _device(m, res, args, 0, fmt)
            assert rc == 0 and _accessor(m, n)[0] == INVALID, fmt          # the last call had no flag
            rc, plain_md = _device(m, res, args, MD, fmt)
            assert rc == 0 and _accessor(m, n)[0] == INVALID
            for flags, base in ((SVSIG, plain), (SVSIG | MD, plain_md)):
                rc, recs = _device(m, res, args, flags, fmt)
                assert rc == 0, (fmt, flags)
                _same(recs, base, (fmt, flags))                            # the record text is unchanged by the flag
                rc, text, ln, roff = _accessor(m, n)
                assert rc == 0 and (ln, roff) == want[1:] and text == want[0], (fmt, flags)
        rc, plain_s = _device(m, res, args, 0, "s")
        # other flag bits
        assert _device(m, res, args, SVSIG | BLOCKS, "s")[0] == INVALID and _device(m, res, args, 8, "s")[0] == INVALID
        # svsigLen 0: every net gap of every alignment; 10^6: nothing
        _set_len(m, 0)
        want0 = _host(m, res, names)
        recs, sigs = m.records_device(res, args, md=False, svsig=True)
        rc, text, ln, roff = _accessor(m, n)
        assert rc == 0 and (ln, roff) == want0[1:] and text == want0[0]
        assert recs == plain_s
        assert sigs == [text[roff[i]:roff[i + 1]] for i in range(n)]       # the Python form: per read
        assert want0[0].count(b"\n") > 20 * want[0].count(b"\n")
        st = m.records_device_stats()
        assert st["svsig_text_bytes"] == ln and ln <= st["svsig_bytes_d2h"] < ln + 8 * (n + 1) + 64 and 0 < st["svsig_bytes_h2d"] < 64 * (n + 3)
        _set_len(m, 10 ** 6)
        assert _device(m, res, args, SVSIG, "s")[0] == 0
        assert _accessor(m, n) == (0, b"", 0, [0] * (n + 1)) and _host(m, res, names) == (b"", 0, [0] * (n + 1))
        # a read with signatures flagged (LRA_ST_CAPACITY = 8, set as tests/test_records_device.py sets it): no lines
        _set_len(m, 25)
        r = next(i for i in range(n) if want[2][i + 1] > want[2][i])
        one = torch.tensor([8], dtype=torch.int32, device=ctx.device)
        ctx.check(lib.lra_copy_device(ctx.h, C.c_void_p(res.d_read_status + r * 4), C.c_void_p(one.data_ptr()), C.c_uint64(4)))
        torch.cuda.synchronize()
        wantf = _host(m, res, names)
        assert wantf[2][r + 1] == wantf[2][r] and 0 < wantf[1] < want[1]
        assert _device(m, res, args, SVSIG, "s")[0] == 0 and _accessor(m, n)[1:] == wantf
        # a small batch behind the large one on the same context
        sub = [r, n - 1]
        r2 = [reads[i] for i in sub]; n2 = [names[i] for i in sub]
        res2 = m.align(seed.ReadBatch(ctx, r2))
        want2 = _host(m, res2, n2)
        assert _device(m, res2, m.record_args(n2, r2, [quals[i] for i in sub]), SVSIG, "s")[0] == 0
        assert _accessor(m, 2)[1:] == want2 and want2[2][1] == want2[1] > 0
    finally:
        lib.lra_ctx_set_svsig_len(ctx.h, 25)


@pytest.mark.gpu
def test_map_files_device_records_writes_the_same_signatures(tmp_path):
    from test_svsig import planted_reads, CH, CHROMS
    genome, reads = planted_reads(0.10, n_plain=2)
    reads = reads[:8]
    fa = tmp_path / "g.fa"; fq = tmp_path / "r.fq"
    with open(fa, "wb") as f:
        for c in range(2):
            f.write(b">" + CHROMS[c] + b"\n" + genome[CH[c]:CH[c + 1]].tobytes() + b"\n")
    with open(fq, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d\n" % i + r + b"\n+\n" + bytes([35 + i]) * len(r) + b"\n")
    outs = []
    for extra in ([], ["--device-records"], ["--device-records", "--host-input"]):       # device input (the reader's arrays alone), then host input
        sam = tmp_path / ("o%d.sam" % len(outs)); sig = tmp_path / ("o%d.svsig" % len(outs))
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_files.py"), "-ONT", str(fa), str(fq), "-o", str(sam), "-SV", "25", str(sig)] + extra,
                       check=True, cwd=ROOT, timeout=300, stderr=subprocess.DEVNULL)
        strip = lambda s: b"\n".join(l for l in s.split(b"\n") if not l.startswith(b"@PG"))   # (the header's @PG line quotes the command line)
        outs.append((strip(open(sam, "rb").read()), open(sig, "rb").read()))
    assert outs[1] == outs[0] and outs[2] == outs[0]
    assert outs[0][1].count(b"\n") >= 1 and outs[0][0].count(b"\n") >= 8
