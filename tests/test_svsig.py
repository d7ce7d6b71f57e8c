"""SV signatures (Alignment::Printsvsig, MapRead's svsigstrm) on the device: lra_sv_signatures_batch against a restatement of the rule on one crafted batch,
and the record stage with LRA_PACK_SVSIG (lra_map_svsig, the snapshot and the pack) for the -ONT, two-stage -CLR and -CCS drivers and tools/map_files.py (GPU)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lra_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INS, DEL = 0, 1
ALPHA = np.frombuffer(b"ACGTACGTACGTacgtN", np.uint8)


def expected_signatures(read: bytes, text: bytes, blocks, min_len):
    """Alignment.h:345-408 restated: for every block but the last, q / t = its end, the gaps to the next block less their common part; a net query gap
    above min_len is INS {t, t, qg, read[q:q + qg]}, otherwise a net text gap above it DEL {t, t + tg - 1, tg, text[t:t + tg]}; a negative gap (the
    reference asserts) gives nothing.  -> [(block, kind, start, end, length, bases)]"""
    b = np.asarray(blocks, np.int64).reshape(-1, 3)
    if len(b) < 2:
        return []
    q = b[:-1, 0] + b[:-1, 2]; t = b[:-1, 1] + b[:-1, 2]
    qg = b[1:, 0] - q; tg = b[1:, 1] - t
    ok = (qg >= 0) & (tg >= 0)
    c = np.minimum(qg, tg)
    qg = qg - c; tg = tg - c
    out = []
    for i in np.flatnonzero(ok & ((qg > min_len) | (tg > min_len))):
        i = int(i)
        if qg[i] > min_len:
            out.append((i, INS, int(t[i]), int(t[i]), int(qg[i]), read[int(q[i]):int(q[i] + qg[i])]))
        else:
            out.append((i, DEL, int(t[i]), int(t[i] + tg[i] - 1), int(tg[i]), text[int(t[i]):int(t[i] + tg[i])]))
    return out


def signature_lines(chrom: bytes, name: bytes, sigs):
    """Alignment.h:374-399"""
    return b"".join(b"%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (chrom, name, s, e, n, b"DEL" if k == DEL else b"INS", bases) for _, k, s, e, n, bases in sigs)


# ---------------------------------------------------------------------------------------------------------------- the kernels
def _aln(rng, lens, qg, tg, q0=0, t0=0, q_pad=0, t_pad=0):
    """One alignment from block lengths and the gaps behind every block (the last pair is ignored): blocks by cumulative sums, as _random_case of
    tests/test_md.py lays them out, over a random read and text."""
    lens = np.asarray(lens, np.int64); qg = np.asarray(qg, np.int64).copy(); tg = np.asarray(tg, np.int64).copy()
    nb = len(lens)
    if nb == 0:
        return b"ACGT", b"ACGTA", np.zeros((0, 3), np.int32)
    qg[-1] = tg[-1] = 0
    q = np.concatenate([[q0], q0 + np.cumsum(lens + qg)[:-1]])
    t = np.concatenate([[t0], t0 + np.cumsum(lens + tg)[:-1]])
    qlen, tlen = int(q[-1] + lens[-1] + 3 + q_pad), int(t[-1] + lens[-1] + 3 + t_pad)
    read = ALPHA[rng.integers(0, len(ALPHA), qlen)].tobytes()
    text = ALPHA[rng.integers(0, len(ALPHA), tlen)].tobytes()
    return read, text, np.stack([q, t, lens], 1).astype(np.int32)


def _crafted_batch():
    """-> (cases [(read, text, blocks)], tags {name: alignment index or list of them})"""
    from lra_amd.refine import SVSIG_PIECE as P
    rng = np.random.default_rng(77)
    cases, tags = [], {}

    def add(tag, *a, **k):
        tags.setdefault(tag, []).append(len(cases))
        cases.append(_aln(rng, *a, **k))

    add("empty", [], [], [])
    add("one", [12], [0], [0])
    cases.append((b"ACGT", b"ACGTA", np.array([[1, 1, 0], [1, 1, 0], [1, 1, 0]], np.int32))); tags["zeros"] = [len(cases) - 1]
    add("gapfirst", [0, 9, 9], [30, 0, 0], [0, 31, 0])                    # a zero-length first block, the alignment opens with an insertion
    add("edges", [7] * 6, [25, 26, 0, 0, 1, 0], [0, 0, 25, 26, 0, 0])     # net gaps of exactly 25 (nothing at min_len 25), 26 and 1 on each side
    add("edges", [7] * 3, [0, 0, 0], [1, 0, 0])
    add("both", [8] * 4, [40, 30, 5, 0], [10, 30, 31, 0])                 # INS 30 at the block's end, nothing, DEL 26
    # two neighbours whose cross pair (last block of one, first of the next) would be an insertion of ~2800 and a deletion of ~3000
    add("cross", [20, 20], [0, 0], [0, 0], q0=10, t0=10)
    add("cross", [20, 20], [0, 0], [0, 0], q0=3000, t0=200)
    add("cross", [20, 20], [0, 0], [0, 0], q0=90, t0=3300)
    add("cross", [20, 20], [0, 0], [0, 0], q0=0, t0=0)                    # (and a step back: negative gaps)
    # > 100 000 blocks, > 2 000 signatures: every scan tile and workgroup boundary lies inside it
    nb = 100_500
    lens = rng.integers(1, 14, nb)
    big = rng.random(nb) < 0.025
    side = rng.random(nb) < 0.5
    small_q = np.where(rng.random(nb) < 0.3, rng.integers(0, 5, nb), 0); small_t = np.where(rng.random(nb) < 0.3, rng.integers(0, 5, nb), 0)
    gap = rng.integers(26, 70, nb)
    add("huge", lens, np.where(big & side, gap + small_t, small_q), np.where(big & ~side, gap + small_q, small_t), q0=3, t0=5)
    # exactly 63, 64 and 65 signatures
    for k in (63, 64, 65):
        nbk = 300
        at = rng.choice(nbk - 1, k, replace=False)
        qg = np.zeros(nbk, np.int64); tg = np.zeros(nbk, np.int64)
        qg[at[::2]] = 30; tg[at[1::2]] = 33
        add("n%d" % k, rng.integers(1, 9, nbk), qg, tg)
    # sequence lengths around the wave, around the copy kernel's piece, and one long deletion -- of each kind
    for n in (63, 64, 65, P - 1, P, P + 1):
        add("len%d" % n, [5, 6, 7, 8], [n, 0, 2, 0], [0, n, 0, 0])
        add("len%d" % n, [3, 4], [n + 9, 0], [9, 0])
    add("longdel", [11, 12, 13], [0, 7, 0], [100_123, 0, 0])
    add("longins", [11, 12], [20_011, 0], [0, 0])
    # the reads and texts of 32 consecutive alignments start at every residue mod 16 (their lengths are 1 and 3 mod 16)
    for i in range(32):
        lens = [6, 5, 4]
        base_q = 6 + 5 + 4 + 31 + 3; base_t = 6 + 5 + 4 + 40 + 3
        add("mod16", lens, [31, 0, 0], [0, 40, 0], q_pad=(1 - base_q) % 16, t_pad=(3 - base_t) % 16)
    # the rest: small random alignments
    for _ in range(300):
        nbk = int(rng.integers(1, 40))
        qg = np.where(rng.random(nbk) < 0.2, rng.integers(0, 60, nbk), 0); tg = np.where(rng.random(nbk) < 0.2, rng.integers(0, 60, nbk), 0)
        add("small", rng.integers(0, 20, nbk), qg, tg, q0=int(rng.integers(0, 5)), t0=int(rng.integers(0, 5)))
    return cases, tags


def _device_batch(ctx, cases):
    import torch
    from lra_amd import refine
    q_off, t_off, boff, bl = [], [], [0], []
    qa = ta = 0
    for r, t, b in cases:
        q_off.append(qa); t_off.append(ta); qa += len(r); ta += len(t)
        bl.append(np.asarray(b, np.int32).reshape(-1, 3)); boff.append(boff[-1] + len(bl[-1]))
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(ctx.device)
    qseq = dev(np.frombuffer(b"".join(c[0] for c in cases) + b"\0" * 64, np.uint8), np.uint8)
    tseq = dev(np.frombuffer(b"".join(c[1] for c in cases) + b"\0" * 64, np.uint8), np.uint8)
    rb = refine.refine_batch_from_device(ctx, dev(np.concatenate(bl), np.int32).view(-1, 3), dev(boff, np.int64), qseq, dev(q_off, np.int64),
                                         dev([len(c[0]) for c in cases], np.int32), tseq, dev(t_off, np.int64), dev([len(c[1]) for c in cases], np.int64))
    return rb, np.array(q_off), np.array(t_off)


@pytest.fixture(scope="module")
def crafted(ctx):
    cases, tags = _crafted_batch()
    rb, q_off, t_off = _device_batch(ctx, cases)
    return dict(cases=cases, tags=tags, rb=rb, q_off=q_off, t_off=t_off)


def _compare(ctx, crafted, min_len):
    """The device's records and bytes against the restatement, record for record; -> (expected per alignment, sig_off)"""
    from lra_amd import refine
    cases = crafted["cases"]
    off, recs, seq = refine.sv_signatures_batch(ctx, crafted["rb"], min_len)
    want = [expected_signatures(r, t, b, min_len) for r, t, b in cases]
    assert len(off) == len(cases) + 1 and off[0] == 0
    assert np.array_equal(np.diff(off.astype(np.int64)), [len(w) for w in want])
    assert len(recs) == int(off[-1])
    flat = [s for w in want for s in w]
    assert np.array_equal(recs["block"], [s[0] for s in flat]) and np.array_equal(recs["kind"], [s[1] for s in flat])
    assert np.array_equal(recs["t_start"], [s[2] for s in flat]) and np.array_equal(recs["len"], [s[4] for s in flat])
    ends = np.cumsum([s[4] for s in flat]) if flat else np.zeros(0, np.int64)
    assert np.array_equal(recs["seq_off"], ends - recs["len"]) and len(seq) == (int(ends[-1]) if flat else 0)     # back to back, in signature order
    assert seq == b"".join(s[5] for s in flat)
    return want, off


@pytest.mark.gpu
def test_kernel_matches_restatement_at_the_default_length(ctx, crafted):
    from lra_amd.refine import SVSIG_PIECE as P
    want, off = _compare(ctx, crafted, 25)
    tags, cases = crafted["tags"], crafted["cases"]
    n = lambda tag: [len(want[a]) for a in tags[tag]]
    kinds = lambda tag: {(s[1], s[4]) for a in tags[tag] for s in want[a]}
    assert int(off[-1]) >= 3000
    assert n("empty") == [0] and n("one") == [0] and n("zeros") == [0] and n("cross") == [0, 0, 0, 0]
    assert [s[:5] for s in want[tags["gapfirst"][0]]] == [(0, INS, 0, 0, 30), (1, DEL, 9, 39, 31)]
    assert kinds("edges") == {(INS, 26), (DEL, 26)}
    b = cases[tags["both"][0]]
    assert [s[:5] for s in want[tags["both"][0]]] == [(0, INS, 8, 8, 30), (2, DEL, int(b[2][2][1]) + 8, int(b[2][2][1]) + 8 + 25, 26)]
    assert want[tags["both"][0]][0][5] == b[0][8:38]                       # the insertion sits in front of the common columns: at the block's end
    assert len(cases[tags["huge"][0]][2]) > 100_000 and n("huge")[0] > 2000
    assert {k for k, _ in kinds("huge")} == {INS, DEL}
    assert n("n63") == [63] and n("n64") == [64] and n("n65") == [65]
    for m in (63, 64, 65, P - 1, P, P + 1):
        assert {(INS, m), (DEL, m)} <= kinds("len%d" % m), m
    assert (DEL, 100_123) in kinds("longdel") and (INS, 20_011) in kinds("longins")
    assert {int(crafted["q_off"][a]) % 16 for a in tags["mod16"]} == set(range(16)) == {int(crafted["t_off"][a]) % 16 for a in tags["mod16"]}
    assert kinds("mod16") == {(INS, 31), (DEL, 40)}


@pytest.mark.gpu
def test_kernel_matches_restatement_at_length_zero(ctx, crafted):
    want, off = _compare(ctx, crafted, 0)
    lens = {(s[1], s[4]) for w in want for s in w}
    assert {(INS, 1), (DEL, 1), (INS, 25), (DEL, 25)} <= lens
    assert int(off[-1]) > 20_000


@pytest.mark.gpu
def test_kernel_finds_nothing_above_a_million_and_handles_an_empty_batch(ctx, crafted):
    from lra_amd import refine
    want, off = _compare(ctx, crafted, 10 ** 6)
    assert int(off[-1]) == 0 and not off.any()
    res = refine.SvSigResult()
    ctx.check(ctx.lib.lra_sv_signatures_batch(ctx.h, 0, None, None, None, None, None, None, None, C.c_int32(25), C.byref(res)))
    assert (int(res.n_aln), int(res.n_sig), int(res.n_seq_bytes)) == (0, 0, 0)
    assert ctx.to_host(res.d_sig_off, 1, np.uint64)[0] == 0
    assert ctx.lib.lra_sv_signatures_batch(ctx.h, 0, None, None, None, None, None, None, None, C.c_int32(-1), C.byref(res)) == -1
    assert ctx.lib.lra_ctx_svsig_len(ctx.h) == 25 and ctx.lib.lra_ctx_set_svsig_len(ctx.h, -1) == -1 and ctx.lib.lra_ctx_svsig_len(ctx.h) == 25


# ---------------------------------------------------------------------------------------------------------------- the record stage
# The planted reads: seed and sizes chosen with tests/oracle_pipeline.py on the CPU (map_read_lowacc, -ONT options, on planted_reads(0.10)), so that the
# aligner bridges the planted indels inside one alignment: with PLANT_SEED = 21 the oracle's final blocks hold 7 net query gaps and 7 net text gaps above
# 25 (the 14 planted indels, none from the simulated errors); above 10 they hold 8 and 8.
PLANT_SEED = 21
N_PLANTED = 14
CH = [0, 350_000, 800_000]
CHROMS = [b"chrA", b"chrB"]


def planted_reads(err, n_plain=26, seed=PLANT_SEED):
    """-> (genome, reads): n_plain simulated reads of ~6 kb, then N_PLANTED reads of 6 kb with one indel in the middle third -- alternately 40-300 reference
    bases removed and 40-300 random bases inserted, every second pair on the reverse strand."""
    genome = synth.make_genome(800_000, seed=77, repeat_frac=0.2, n_families=3)
    reads, _ = synth.simulate_reads(genome, n_plain, 6000, 1500, err, seed=5)
    rng = np.random.default_rng(seed)
    sim = lambda a, n: synth.simulate_read(rng, genome[a:a + n + 1], n, err * 0.8, (30, 35, 35), False)[0]
    for i in range(N_PLANTED):
        c = i % 2
        a = int(rng.integers(CH[c] + 1000, CH[c + 1] - 8000))
        n1 = int(rng.integers(2000, 4000)); size = int(rng.integers(40, 301))
        if i % 2 == 0:
            rd = np.concatenate([sim(a, n1), sim(a + n1 + size, 6000 - n1)])                   # `size` reference bases removed
        else:
            rd = np.concatenate([sim(a, n1), synth.BASES[rng.integers(0, 4, size)], sim(a + n1, 6000 - n1)])
        reads.append(synth.revcomp(rd) if (i // 2) % 2 else rd)
    return genome, [np.ascontiguousarray(r).tobytes() for r in reads]


def expected_text(mapper, d, num_aln, reads, genome, names, min_len):
    """Per read: the restatement on the final blocks of its alignments in result order (job, then segment)."""
    from lra_amd import mapread
    na = max(int(num_aln), 1)
    jo = d["job_aln_off"]
    gb = genome.tobytes()
    out = []
    for r in range(len(reads)):
        text = b""
        if not d["read_status"][r]:
            for a in range(int(jo[r * na]), int(jo[(r + 1) * na])):
                ci = int(d["chrom"][a])
                rd = reads[r] if not d["strand"][a] else mapread.create_rc(reads[r])
                b = d["blocks"][int(d["block_off"][a]):int(d["block_off"][a + 1])]
                text += signature_lines(mapper.chrom_names[ci], names[r], expected_signatures(rd, gb[mapper.chrom_pos[ci]:mapper.chrom_pos[ci + 1]], b, min_len))
        out.append(text)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["ont", "clr-two-stage", "ccs"])
def test_record_stage_prints_the_signatures(ctx, form):
    import dataclasses
    from lra_amd import mapread, seed, parallel
    genome, reads = planted_reads(0.01 if form == "ccs" else 0.10)
    names = [b"read%d" % i for i in range(len(reads))]
    if form == "ccs":
        mapper = mapread.HighAccMapper(ctx, genome, None, None, CHROMS, CH, "ccs")
    else:
        opts = mapread.clr_options() if form.startswith("clr") else mapread.LowAccOptions()
        ik, ip = synth.build_global_index(genome, opts.globalK, opts.globalW, 100 if opts.read_type == "ont" else opts.globalMaxFreq)
        mapper = mapread.LowAccMapper(ctx, genome, ik, ip, CHROMS, CH, opts)
    batch = seed.ReadBatch(ctx, reads)
    if form == "clr-two-stage":
        mapper.front(batch)
        res, bctx = mapper.back()
        m = mapper.on(bctx)
    else:
        res = mapper.align(batch)
        m = mapper
    try:
        d = m.fetch(res)
        want = expected_text(m, d, res.num_aln, reads, genome, names, 25)
        got = m.sv_signatures(res, names)                                  # lra_map_svsig
        assert got == want
        joined = b"".join(got)
        assert joined.count(b"\tINS\t") >= 1 and joined.count(b"\tDEL\t") >= 1, (joined.count(b"\tINS\t"), joined.count(b"\tDEL\t"))
        # the record text does not change by a byte; the snapshot form prints the same signatures on 1 and 4 threads
        rargs = m.record_args(names, reads)
        plain = m.records_host(m.snapshot(res, md=False), rargs)
        snap = m.snapshot(res, md=False, svsig=True)
        assert m.records_host(snap, rargs, free=False) == plain
        assert m.svsig_host(snap, names, n_threads=1, free=False) == want
        assert m.svsig_host(snap, names, n_threads=4) == want
        # the pack round trip of the multi-GPU path
        packed = parallel.pack_records(m.ctx, res, svsig=True, svsig_len=25)
        assert parallel.svsig_from_packed(ctx.lib, packed, names, m.chrom_names) == want
        assert parallel.records_from_packed(ctx.lib, m.copts, packed, names, reads, m.chrom_names) == plain
        assert np.frombuffer(parallel.pack_records(m.ctx, res)[:128].tobytes(), np.int64)[12:14].tolist() == [0, 0]
        # MD and SV together: both outputs, unchanged
        withmd = m.records_host(m.snapshot(res, md=True), rargs)
        snap = m.snapshot(res, md=True, svsig=True)
        assert m.records_host(snap, rargs, free=False) == withmd != plain
        assert m.svsig_host(snap, names) == want
        # svsigLen = 10: a superset of the default's lines
        if form == "ccs":
            m10 = m; m.svsigLen = 10
        else:
            m10 = m.on(m.ctx); m10.opts = dataclasses.replace(m.opts, svsigLen=10)
        got10 = m10.sv_signatures(res, names)
        assert m.ctx.lib.lra_ctx_svsig_len(m.ctx.h) == 10
        assert got10 == expected_text(m, d, res.num_aln, reads, genome, names, 10)
        for g25, g10 in zip(got, got10):
            assert set(g25.splitlines()) <= set(g10.splitlines())
        if form == "ont":                                                  # (the oracle's count for these reads: 16 lines above 10 against 14 above 25)
            assert sum(len(g.splitlines()) for g in got10) > sum(len(g.splitlines()) for g in got)
    finally:
        m.ctx.lib.lra_ctx_set_svsig_len(m.ctx.h, 25)
        if form == "clr-two-stage":
            mapper.release()


@pytest.mark.gpu
def test_map_files_writes_the_signatures(ctx, tmp_path):
    from lra_amd import mapread, seed
    genome, reads = planted_reads(0.10, n_plain=2)
    reads = reads[:2] + reads[2:8]
    names = [b"read%d" % i for i in range(len(reads))]
    fa = tmp_path / "g.fa"; fq = tmp_path / "r.fq"
    with open(fa, "wb") as f:
        for c in range(2):
            f.write(b">" + CHROMS[c] + b"\n" + genome[CH[c]:CH[c + 1]].tobytes() + b"\n")
    with open(fq, "wb") as f:
        for n, r in zip(names, reads):
            f.write(b"@" + n + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    run = lambda *extra: subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_files.py"), "-ONT", str(fa), str(fq), *extra], check=True, timeout=300,
                                        capture_output=True)
    run("-o", str(tmp_path / "plain.sam"))
    run("-o", str(tmp_path / "sv.sam"), "-SV", "25", str(tmp_path / "out.svsig"))
    strip = lambda p: [l for l in open(p, "rb").read().split(b"\n") if not l.startswith(b"@PG")]
    assert strip(tmp_path / "sv.sam") == strip(tmp_path / "plain.sam")
    opts = mapread.LowAccOptions()
    mapper = mapread.LowAccMapper(ctx, genome, None, None, CHROMS, CH, opts, index_params=(17, 10, 150, 15, 1), staged=False)   # `lra index -ONT`, as the tool builds it
    res = mapper.align(seed.ReadBatch(ctx, reads))
    lib_text = b"".join(mapper.sv_signatures(res, names))
    assert open(tmp_path / "out.svsig", "rb").read() == lib_text and lib_text.count(b"\n") >= 1
