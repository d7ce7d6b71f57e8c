"""lra align -a (opts.storeAll, lra.cpp:182-184; MapRead.h:172-183): the read is sketched with w = 1, every other stage keeps opts.globalW.

CPU: the oracle's StoreMinimizers at w = 1 equals a closed form; the switch's argument checks.  GPU: the w = 1 sketch (sketch_all_kernel) through a1-a4
against the oracle, the drivers with the switch against the oracle pipeline composed with w = 1, and the switch through prefetch, two-stage batches
and the host-buffer boundary."""
import ctypes as C

import numpy as np
import pytest

from lra_amd import synth

M63 = np.uint64((1 << 63) - 1)
B63 = np.uint64(1 << 63)
_BAD = np.ones(256, bool)                 # what code_n (SeqUtils.h:42, seqMapN) classes as > 3: everything but ACGTacgt and the bytes 0..7
_BAD[:8] = False
_CODE = np.zeros(256, np.uint64)
_CODE[:8] = np.arange(8) & 3
for _i, _c in enumerate(b"ACGT"):
    _BAD[_c] = _BAD[_c + 32] = False
    _CODE[_c] = _CODE[_c + 32] = _i


def closed_form(seq: bytes, k):
    """StoreMinimizers(seq, k, 1) (MinCount.h:8-179 with windowSpan = k): nothing if L <= k; else every p < L - k whose k-mer has no non-ACGT byte, and
    p = L - k only if its k-mer is clean and seq[L - k - 1] is ACGT.  Keys canonical with the strand in bit 63 (MinCount.h:60-61)."""
    a = np.frombuffer(seq, np.uint8)
    L = len(a)
    if L <= k:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    n = L - k + 1
    bad = _BAD[a]
    cs = np.concatenate([[0], np.cumsum(bad)])
    em = (cs[k:k + n] - cs[:n]) == 0
    em[n - 1] &= not bad[L - k - 1]
    c = _CODE[a]
    fwd = np.zeros(n, np.uint64)
    rc = np.zeros(n, np.uint64)
    for i in range(k):
        fwd = (fwd << np.uint64(2)) | c[i:i + n]
        rc |= (np.uint64(3) - c[i:i + n]) << np.uint64(2 * i)
    key = np.where((fwd & M63) < (rc & M63), fwd & M63, rc | B63)
    pos = np.nonzero(em)[0]
    return key[pos], pos.astype(np.uint32)


def _crafted(k, rng):
    """Reads at the edges of the closed form (N placement, lengths around k, lower case, the last k-mer's quirk)."""
    R = lambda n: synth.BASES[rng.integers(0, 4, n)].tobytes()
    out = [b"", b"N" * 300, R(k - 1), R(k), R(k + 1), b"N" + R(200), R(5) + b"N" + R(200), R(200) + b"N" + R(k), R(200) + b"N" + R(k - 1) + b"C",
           R(200) + b"N", R(150) + b"NNNNNNN" + R(90) + b"N" * 40 + R(70), b"N" + R(k), b"NN" + R(k), b"N" * 50 + R(k), b"N" * 50 + R(k + 1) + b"N",
           R(300).lower(), R(120) + R(120).lower() + b"n" + R(80), R(k) + b"N" + R(k), bytes(rng.integers(0, 8, 100).astype(np.uint8)) + R(30),
           R(63 - k) + b"N" + R(64), R(64 + 64 - k) + b"N" + R(200), R(64 * 3 + 5), R(1000) + b"X" + R(100) + b"-" + R(50)]
    # N every few bases: short clean runs of every length around k
    s = bytearray(R(4000))
    for p in np.cumsum(rng.integers(k - 3, k + 4, 200)):
        if p < len(s):
            s[p] = ord("N")
    out.append(bytes(s))
    return out


def test_oracle_w1_sketch_is_the_closed_form(oracle):
    rng = np.random.default_rng(11)
    n_last = n_quirk = 0
    for k in (11, 15, 17, 19, 25, 32):
        reads = _crafted(k, rng) + [synth.BASES[rng.integers(0, 4, int(rng.integers(0, 3000)))].tobytes() for _ in range(20)]
        for s in reads:
            kk, pp = oracle.store_minimizers(s, k, 1)
            ek, ep = closed_form(s, k)
            assert np.array_equal(pp, ep) and np.array_equal(kk, ek), (k, s[:40], len(s), pp[:8], ep[:8])
            L = len(s)
            if L > k:
                clean_last = not _BAD[np.frombuffer(s[L - k:], np.uint8)].any()
                n_last += clean_last and len(ep) > 0 and ep[-1] == L - k
                n_quirk += clean_last and not (len(ep) and ep[-1] == L - k)
    assert n_last > 50 and n_quirk >= 12, (n_last, n_quirk)      # both sides of the last k-mer's rule occur


def test_store_all_switch_rejects_bad_arguments_without_gpu():
    import __graft_entry__ as g
    g.build()
    from lra_amd._lib import load_library
    lib = load_library()
    assert lib.lra_ctx_set_store_all(None, 1) == -1                   # LRA_ERR_INVALID
    assert lib.lra_ctx_set_store_all(None, 0) == -1
    assert lib.lra_ctx_store_all(None) == -1


# ---------------------------------------------------------------------------------------------------------------------------------- GPU: a1-a4 at w = 1
def _check_seed(ctx, oracle, genome, reads, k, max_freq, index_w=10):
    """lra_seed_batch(w = 1) against oracle sketch + sort + CompareLists + SeparateMatchesByStrand, field for field (the global index at index_w)."""
    from lra_amd import seed
    from test_seed import _oracle_pipeline
    ik, ip = synth.build_global_index(genome, k, index_w, 50)
    seed.load_reference(ctx, genome, ik, ip)
    batch = seed.ReadBatch(ctx, reads)
    res = seed.seed_batch(ctx, batch, k, 1, max_freq)
    out = seed.fetch(ctx, res)
    gbytes = genome.tobytes() + b"\0" * 64
    n_mm = n_match = n_tied = 0
    for r, rb in enumerate(reads):
        sk, sp, qi, ti, strand = _oracle_pipeline(oracle, rb, gbytes, ik, ip, k, 1, max_freq)
        a, b = int(out["mm_off"][r]), int(out["mm_off"][r + 1])
        assert b - a == len(sk) == len(closed_form(rb, k)[0]), (r, len(rb), b - a, len(sk))
        assert np.array_equal(out["mm_key"][a:b], sk), r
        assert np.array_equal(out["mm_pos"][a:b], sp), r
        m0, m1 = int(out["match_off"][r]), int(out["match_off"][r + 1])
        assert m1 - m0 == len(qi), (r, m1 - m0, len(qi))
        assert np.array_equal(out["match_qi"][m0:m1], qi), r
        assert np.array_equal(out["match_ti"][m0:m1], ti), r
        nf = int((strand == 0).sum())
        assert int(out["n_forward"][r]) == nf, r
        eq, et = sp[qi], ip[ti]
        assert np.array_equal(out["sep_qpos"][m0:m0 + nf], eq[strand == 0]), r
        assert np.array_equal(out["sep_tpos"][m0:m0 + nf], et[strand == 0]), r
        assert np.array_equal(out["sep_qpos"][m0 + nf:m1], eq[strand == 1]), r
        assert np.array_equal(out["sep_tpos"][m0 + nf:m1], et[strand == 1]), r
        n_mm += len(sk); n_match += len(qi)
        n_tied += bool(len(sk) > 1 and np.any((sk[1:] & M63) == (sk[:-1] & M63)))
    assert int(res.n_minimizers) == n_mm
    return n_mm, n_match, n_tied


@pytest.mark.gpu
@pytest.mark.parametrize("k", [17, 19])
def test_hip_seed_w1_matches_oracle(ctx, oracle, k):
    rng = np.random.default_rng(k)
    genome = synth.make_genome(400_000, seed=2, repeat_frac=0.4)
    sim, _ = synth.simulate_reads(genome, 40, 5000, 2500, 0.10, seed=k)
    reads = []
    for i, r in enumerate(sim):                                          # random reads, with the crafted ones and empty reads between them
        reads.append(r.tobytes())
        if i % 8 == 3:
            reads.append(b"")
    reads += _crafted(k, rng)
    # one read longer than 1 Mb (its lists go to the sort for lists beyond 65534 tuples), a second one with N runs, and reads straddling every tile phase
    big = np.concatenate([genome[s:s + 100_000] for s in range(0, 400_000, 100_000)] * 3)[:1_100_003].copy()
    reads.append(big.tobytes())
    reads.append(b"")
    holes = big[:300_000].copy()
    holes[rng.integers(0, len(holes), 200)] = ord("N")
    reads.append(holes.tobytes())
    for L in range(k - 1, k + 70):
        a = int(rng.integers(0, 300_000))
        reads.append(genome[a:a + L].tobytes())
    n_mm, n_match, n_tied = _check_seed(ctx, oracle, genome, reads, k, 150)
    assert n_match > 10_000 and n_mm > 1_400_000, (n_mm, n_match)
    print("w = 1, k = %d: %d reads, %d tuples, %d matches, %d reads with a repeated key (exact sort)" % (k, len(reads), n_mm, n_match, n_tied))


@pytest.mark.gpu
def test_hip_seed_w1_small_batches(ctx, oracle):
    """Batches of one read, of empty reads only, and of a read whose only clean k-mer is the last one (never emitted), back to back on one context."""
    from lra_amd import seed
    rng = np.random.default_rng(3)
    genome = synth.make_genome(200_000, seed=6, repeat_frac=0.2)
    k = 17
    last_only = b"N" * 40 + genome[1000:1000 + k].tobytes()
    for reads in ([genome[5000:5000 + 700].tobytes()], [b"", b"", b""], [last_only], [last_only, genome[9000:9000 + k + 1].tobytes()],
                  [synth.BASES[rng.integers(0, 4, 64 * 5)].tobytes() for _ in range(9)]):
        _check_seed(ctx, oracle, genome, reads, k, 150)
    ik, ip = synth.build_global_index(genome, k, 10, 50)
    seed.load_reference(ctx, genome, ik, ip)
    res = seed.seed_batch(ctx, seed.ReadBatch(ctx, [last_only]), k, 1, 150)
    assert int(res.n_minimizers) == 0


# ---------------------------------------------------------------------------------------------------------------------------------- GPU: the drivers
def _lowacc_case(preset):
    from lra_amd import mapread
    import oracle_pipeline as OP
    genome = synth.make_genome(500_000, seed=31, repeat_frac=0.25, n_families=3)
    o = mapread.clr_options() if preset == "clr" else mapread.LowAccOptions()
    oo = dict(OP.CLR if preset == "clr" else OP.ONT)
    err, mix = (0.15, (20, 30, 50)) if preset == "clr" else (0.12, (30, 35, 35))
    reads, _ = synth.simulate_reads(genome, 12, 7000, 2500, err, mix, seed=13)
    rng = np.random.default_rng(4)
    sim = lambda a, n, rev=False: synth.simulate_read(rng, genome[a:a + n + 1], n, err * 0.8, mix, rev)[0]
    reads.append(np.concatenate([sim(50_000, 4000), sim(60_000, 4000)]))                       # 6 kb deletion
    reads.append(np.concatenate([sim(150_000, 4000), sim(154_000, 2500, True), sim(156_500, 4000)]))   # inversion
    short = sim(210_000, 900, True).copy()
    short[rng.integers(0, len(short), 6)] = ord("N")
    reads.append(short)                                                                        # short, with N
    reads.append(synth.BASES[rng.integers(0, 4, 2000)].copy())                                 # junk
    return genome, o, oo, [r.tobytes() for r in reads]


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["ont", "clr"])
def test_lowacc_store_all_matches_oracle_pipeline(ctx, oracle, preset):
    """-ONT / -CLR with -a: every SegAlignment equals the oracle pipeline run with globalW = 1 (on this path opts.globalW reaches nothing but the sketch:
    the refinement stages take smallOpts, whose globalW is glIndex.w).  The switch reaches the sketch: n_minimizers is the closed form's count with it,
    near 2 / (w + 1) of that without it, and the records differ."""
    import dataclasses
    import oracle_pipeline as OP
    from lra_amd import seed, mapread
    genome, o, oo, raw = _lowacc_case(preset)
    CH = [0, len(genome)]
    ik, ip = synth.build_global_index(genome, o.globalK, o.globalW, 100)
    names = [b"r%d" % i for i in range(len(raw))]
    plain = mapread.LowAccMapper(ctx, genome, ik, ip, [b"chr1"], CH, o)
    batch = seed.ReadBatch(ctx, raw)
    res_w = plain.align(batch)
    texts_w = plain.records(res_w, names, raw)
    n0_w = plain.fetch(res_w)["n0"]
    n_mm_w = plain.stats["n_minimizers"]
    mapper = mapread.LowAccMapper(ctx, genome, ik, ip, [b"chr1"], CH, dataclasses.replace(o, storeAll=True))
    assert ctx.lib.lra_ctx_store_all(ctx.h) == 1
    res = mapper.align(batch)
    out = mapper.fetch(res)
    texts_a = mapper.records(res, names, raw)
    closed = sum(len(closed_form(r, o.globalK)[0]) for r in raw)
    assert mapper.stats["n_minimizers"] == closed, (mapper.stats["n_minimizers"], closed)
    assert closed >= 0.99 * sum(max(0, len(r) - o.globalK + 1) for r in raw) - 200
    assert 0.75 < n_mm_w / (closed * 2 / (o.globalW + 1)) < 1.25, (n_mm_w, closed)
    assert len(out["n0"]) != len(n0_w) or np.any(out["n0"] != n0_w)           # the anchors behind the alignments differ
    n_text_diff = sum(a != b for a, b in zip(texts_a, texts_w))
    g_win, g_bnd, g_tup = mapper.gli.fetch()
    g_index = (mapread.seq_offsets(CH, o.localIndexWindow).astype(np.uint64), g_bnd, g_tup)
    gbytes = genome.tobytes() + b"\0" * 64
    oo1 = dict(oo, globalW=1)
    na = int(res.num_aln)
    n_flagged = n_seg = 0
    for r, rd in enumerate(raw):
        if out["read_status"][r]:
            n_flagged += 1
            continue
        exp, unaligned = OP.map_read_lowacc(rd, gbytes, ik, ip, g_index, oo1, chrom_pos=CH)
        for p in range(na):
            a0, a1 = int(out["job_aln_off"][r * na + p]), int(out["job_aln_off"][r * na + p + 1])
            e = exp[p] if p < len(exp) else []
            assert a1 - a0 == len(e), (r, p, a1 - a0, len(e))
            for a, s in zip(range(a0, a1), e):
                assert (out["strand"][a], out["supp"][a], out["n0"][a], out["n1"][a], out["chrom"][a]) == (s["strand"], s["supp"], s["n0"], s["n1"], s["chrom"]), (r, p, a)
                assert np.float32(out["first_sdp_value"][a]).view(np.uint32) == np.float32(s["value"]).view(np.uint32), (r, p, a)
                b = out["blocks"][int(out["block_off"][a]):int(out["block_off"][a + 1])]
                assert np.array_equal(b, s["blocks"]), (r, p, a, len(b), len(s["blocks"]))
                ec, ev, eruns, _ = s["stats"]
                assert out["counts"][a].tolist() == [ec[k] for k in oracle.STAT_NAMES], (r, p, a)
                assert np.array_equal(out["runs"][int(out["run_off"][a]):int(out["run_off"][a + 1])], eruns), (r, p, a)
                n_seg += 1
    print("-%s -a: %d reads, %d flagged, %d alignments checked, %d tuples (w = %d: %d), %d reads' records differ" % (preset.upper(), len(raw), n_flagged, n_seg, closed,
                                                                                                          o.globalW, n_mm_w, n_text_diff))
    assert n_flagged == int(res.counters.n_flagged_reads)
    assert n_flagged <= 2 and n_seg >= len(raw) - 4, (n_flagged, n_seg)
    # the switch off again: the plain records come back on the same context
    assert plain.records(plain.align(batch), names, raw) == texts_w


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["ccs", "contig"])
def test_highacc_store_all_matches_oracle_pipeline(ctx, oracle, monkeypatch, preset):
    """-CCS / -CONTIG with -a: the driver equals MapRead_highacc composed from the oracle's stages with StoreMinimizers at w = 1 while globalW stays 20 / 10
    (RefineBtwnClusters_chain's W, Map_highacc.h:466-468)."""
    import oracle_pipeline as OP
    from lra_amd import seed, mapread, index as I
    rng = np.random.default_rng(21)
    g = synth.make_genome(500_000, seed=19, repeat_frac=0.2, n_families=3)
    CH = [0, 250_000, len(g)]
    if preset == "contig":
        oo, ip, err, n, ln = dict(OP.CONTIG), (19, 10, 30, 20, 1), 0.003, 4, 40_000
    else:
        oo, ip, err, n, ln = dict(OP.CCS), (17, 10, 150, 15, 1), 0.01, 10, 8000
    reads, _ = synth.simulate_reads(g, n, ln, ln // 4, err, (34, 33, 33), seed=5)
    sim = lambda a, m, rev=False: synth.simulate_read(rng, g[a:a + m + 1], m, err, (34, 33, 33), rev)[0]
    reads.append(np.concatenate([sim(50_000, 4000), sim(60_000, 4000)]))
    reads.append(np.concatenate([sim(300_000, 4500), sim(420_000, 4500, True)]))
    raw = [r.tobytes() for r in reads]
    names = [b"r%d" % i for i in range(len(raw))]
    plain = mapread.HighAccMapper(ctx, g, None, None, [b"chrA", b"chrB"], CH, preset, index_params=ip)
    batch = seed.ReadBatch(ctx, raw)
    n0_w = plain.fetch(plain.align(batch))["n0"]
    mapper = mapread.HighAccMapper(ctx, g, None, None, [b"chrA", b"chrB"], CH, preset, index_params=ip, storeAll=True)
    assert mapper.seed_w == 1 and int(mapper.copts.globalW) == oo["globalW"]
    res = mapper.align(batch)
    out = mapper.fetch(res)
    assert mapper.stats["n_minimizers"] == sum(len(closed_form(r, oo["globalK"])[0]) for r in raw)
    assert len(out["n0"]) != len(n0_w) or np.any(out["n0"] != n0_w)
    ik, ipos = I.global_index(ctx)
    g_index = mapper.fetch_local_index()
    orig = OP.O.store_minimizers
    monkeypatch.setattr(OP.O, "store_minimizers", lambda s, k, w: orig(s, k, 1))
    gb = g.tobytes()
    na = int(res.num_aln)
    n_seg = n_flagged = 0
    for r, rd in enumerate(raw):
        if out["read_status"][r]:
            n_flagged += 1
            continue
        exp, unaligned, note = OP.map_read_highacc(rd, gb, ik, ipos, oo, chrom_pos=CH, g_index=g_index)
        assert note is None, (r, note)
        by_h = {G["h"]: G["segs"] for G in exp}
        for h in range(na):
            a0, a1 = int(out["job_aln_off"][r * na + h]), int(out["job_aln_off"][r * na + h + 1])
            assert bool(out["job_reached"][r * na + h]) == (h in by_h), (r, h)
            e = by_h.get(h, [])
            assert a1 - a0 == len(e), (r, h, a1 - a0, len(e))
            for a, s in zip(range(a0, a1), e):
                assert (out["strand"][a], out["supp"][a], out["secondary"][a], out["n0"][a], out["n1"][a], out["chrom"][a]) == \
                       (s["strand"], s["supp"], s["secondary"], s["n0"], s["n1"], s["chrom"]), (r, h, a)
                assert np.float32(out["first_sdp_value"][a]).view(np.uint32) == np.float32(s["value"]).view(np.uint32), (r, h, a)
                b = out["blocks"][int(out["block_off"][a]):int(out["block_off"][a + 1])]
                assert np.array_equal(b, s["blocks"]), (r, h, a, len(b), len(s["blocks"]))
                ec, ev, eruns, _ = s["stats"]
                assert np.array_equal(out["runs"][int(out["run_off"][a]):int(out["run_off"][a + 1])], eruns), (r, h, a)
                n_seg += 1
    print("-%s -a: %d reads, %d flagged, %d alignments checked" % (preset.upper(), len(raw), n_flagged, n_seg))
    assert n_flagged <= 1 and n_seg >= len(raw) - 2, (n_flagged, n_seg)


# ---------------------------------------------------------------------------------------------------------------------------------- GPU: pipelining
@pytest.mark.gpu
def test_store_all_with_prefetch_two_stage_and_host_buffers(ctx):
    """A seed result prefetched at globalW is not adopted by a store-all batch (it seeds itself), one prefetched at w = 1 is; two-stage front / back with the
    switch equals the one call; lra_map_reads_host with the switch equals the device-buffer call."""
    import dataclasses
    import threading
    from lra_amd import seed, mapread
    from lra_amd.context import Context
    genome = synth.make_genome(500_000, seed=31, repeat_frac=0.3, n_families=3)
    o = dataclasses.replace(mapread.LowAccOptions(), storeAll=True)
    ik, ip = synth.build_global_index(genome, o.globalK, o.globalW, 100)
    reads, _ = synth.simulate_reads(genome, 16, 7000, 3000, 0.10, seed=5)
    raw = [r.tobytes() for r in reads]
    names = [b"q%d" % i for i in range(len(raw))]
    mapper = mapread.LowAccMapper(ctx, genome, ik, ip, [b"chr1"], [0, len(genome)], o)
    assert mapper.seed_w == 1
    batch = seed.ReadBatch(ctx, raw)
    want = mapper.records(mapper.align(batch), names, raw)
    side = Context(0)
    mapread.LowAccMapper.sharing(side, mapper)
    assert side.lib.lra_ctx_store_all(side.h) == 1
    ctx.timing(True)
    for w, adopted in ((o.globalW, False), (mapper.seed_w, True)):
        seed.seed_prefetch(side, batch, o.globalK, w, o.globalMaxFreq)
        seed.adopt_seed(ctx, side)
        ctx.timing_reset()
        assert mapper.records(mapper.align(batch), names, raw) == want, w
        assert ctx.timing_get("sketch_all_count")[1] == (0 if adopted else 1), w
        assert ctx.timing_get("sketch_emit")[1] == 0
    # the reverse: a result prefetched at w = 1 is not adopted by a batch without the switch
    plain = mapread.LowAccMapper.sharing(Context(0), mapper)
    plain.opts = dataclasses.replace(o, storeAll=False)
    want_plain = plain.records(plain.align(batch), names, raw)
    seed.seed_prefetch(side, batch, o.globalK, 1, o.globalMaxFreq)
    seed.adopt_seed(plain.ctx, side)
    plain.ctx.timing(True); plain.ctx.timing_reset()
    assert plain.records(plain.align(batch), names, raw) == want_plain
    assert plain.ctx.timing_get("sketch_emit")[1] == 1 and plain.ctx.timing_get("sketch_all_count")[1] == 0
    assert want_plain != want
    ctx.timing(False)
    # two-stage batches
    got, err = [None, None], []

    def fronts():
        try:
            for _ in range(2):
                mapper.front(batch)
        except BaseException as e:
            err.append(e)

    def backs():
        try:
            for i in range(2):
                res, bctx = mapper.back()
                got[i] = mapper.on(bctx).records(res, names, raw)
                mapper.release()
        except BaseException as e:
            err.append(e)
    tf, tb = threading.Thread(target=fronts), threading.Thread(target=backs)
    tf.start(); tb.start(); tf.join(); tb.join()
    assert not err, err
    assert got == [want, want]
    # the host-buffer boundary
    seqb = b"".join(raw)
    off = np.zeros(len(raw) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in raw])
    res = mapread.MapResult()
    ctx.check(ctx.lib.lra_map_reads_host(ctx.h, len(raw), C.c_char_p(seqb), C.c_void_p(off.ctypes.data), C.byref(mapper.copts), C.byref(res)))
    assert mapper.records(res, names, raw) == want
    assert int(res.counters.n_minimizers) == sum(len(closed_form(r, o.globalK)[0]) for r in raw)
    plain.ctx.close()
    side.close()
