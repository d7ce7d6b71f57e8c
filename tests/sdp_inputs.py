"""Helpers (tests / bench cpu_baseline only): the extended clusters SDP#A sees, produced by the ORACLE's a1-a7; the sparse DP tests' shared driver
(_run_hip), the comparison with the oracle (_compare), random / captured / crafted inputs and the CPU-side shape of a job (sdp_case_shape)."""
import numpy as np


def oracle_ext_clusters(oracle, read: bytes, genome_arr, ik, ip, k=17, w=10, mf=150, preset="ONT"):
    """-> (cluster_off, strands, q, t(global), len) as Map_lowacc.h:77-150 hands them to SparseDP (:188)."""
    g = genome_arr.tobytes() + b"\0" * 64
    keys, pos = oracle.store_minimizers(read, k, w)
    sk, sp = oracle.sort_minimizers(keys, pos)
    qi, ti = oracle.compare_lists(sk, sp, ik, ip, mf)
    q, t, key = sp[qi], ip[ti], sk[qi]
    st = oracle.separate_strand(read, g, k, q, t)
    po = dict(oracle.CLEAN_PRESETS[preset]); po["globalK"] = k
    opts = oracle.CleanOpts(**po)
    offs = [0]; strands = []; Q = []; T = []; L = []
    chrom = genome_arr.tobytes()
    for strand in (0, 1):
        sel = st == strand
        oq, ot, cl = oracle.clean_matches(q[sel], t[sel], key[sel], strand, opts, [0, len(genome_arr)])
        for i in range(len(cl["start"])):
            a, b = int(cl["start"][i]), int(cl["end"][i])
            eq, et, el, _ = oracle.linear_extend(oq[a:b], ot[a:b], strand, k, read, chrom)
            Q.extend(eq.tolist()); T.extend(et.tolist()); L.extend(el.tolist())
            strands.append(strand); offs.append(len(Q))
    return (np.array(offs, np.int32), np.array(strands, np.uint8), np.array(Q, np.uint32), np.array(T, np.uint32), np.array(L, np.int32))


# ---------------------------------------------------------------- HIP SDP#A vs. oracle: inputs, driver, comparison -----
def _random_clusters(rng, n_clusters, per_cluster, span, ties):
    offs = [0]; strands = []; Q = []; T = []; L = []
    for c in range(n_clusters):
        strand = int(rng.random() < 0.4)
        q = int(rng.integers(0, span)); t = int(rng.integers(0, span)) + (span if strand else 0)
        m = int(rng.integers(1, per_cluster + 1))
        for i in range(m):
            ln = int(rng.choice([1, 2, 3])) if ties else int(rng.choice([17, 17, 20, 30, 60, 150]))
            Q.append(q); T.append(t); L.append(ln)
            step = int(rng.integers(0, 3)) if ties else int(rng.integers(0, 200))
            q += ln + step
            if strand:
                t = max(0, t - ln - (int(rng.integers(0, 3)) if ties else int(rng.integers(0, 200))))
            else:
                t += ln + (int(rng.integers(0, 3)) if ties else int(rng.integers(0, 200)))
        strands.append(strand); offs.append(len(Q))
    return (np.array(offs, np.int32), np.array(strands, np.uint8), np.array(Q, np.uint32), np.array(T, np.uint32), np.array(L, np.int32))


def _random_read_mix():
    """162 reads of 0 .. 599 anchors (0 .. 1298 points; 90 of them below 40 points): the oracle accepts every one under each of _MIX_OPTS"""
    rng = np.random.default_rng(77)
    reads_in = []
    for k in range(160):
        if k < 40: reads_in.append(_random_clusters(rng, int(rng.integers(1, 4)), 3, 12, True))        # heavy coordinate ties
        elif k < 80: reads_in.append(_random_clusters(rng, int(rng.integers(1, 5)), 6, 40, True))
        elif k < 140: reads_in.append(_random_clusters(rng, int(rng.integers(1, 8)), 12, 3000, False))
        else: reads_in.append(_random_clusters(rng, int(rng.integers(4, 30)), 40, 30000, False))
    reads_in.insert(5, (np.array([0], np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.int32)))   # read without clusters
    reads_in.insert(9, (np.array([0, 1], np.int32), np.array([1], np.uint8), np.array([5], np.uint32), np.array([100], np.uint32), np.array([17], np.int32)))
    read_lens = [max(300, int(q.max()) + 200) if len(q) else 300 for (_, _, q, _, _) in reads_in]
    return reads_in, read_lens


_MIX_OPTS = (dict(), dict(NumAln=3, alnthres=0.3, rate=3.0), dict(gapopen=4.0, gapextend=20.0, gapCeiling1=3000, gapCeiling2=5000, rate=1.0))


def _run_hip(ctx, reads_in, read_lens, opts_kw, rates=None):
    """reads_in: list of (cluster_off, strands, q, t, len) per read -> fetched result dict.  q and t reach the device with their 32 bits as they are (a t above
    2^31 is the same unsigned number there); rates: one rate per read (the `rate=` tensor of chain.sparse_dp_batch) or None."""
    import torch
    from lra_amd import chain
    dev = ctx.device
    coff = [0]; cstart = []; ccount = []; cstrand = []; Q = []; T = []; L = []
    pad = 0; at = 0
    for (offs, st, q, t, ln) in reads_in:
        for c in range(len(st)):
            a, b = int(offs[c]), int(offs[c + 1])
            Q.append(np.full(pad, 7, np.uint32)); T.append(np.full(pad, 9, np.uint32)); L.append(np.full(pad, 1, np.int32))   # gaps between clusters, as lra_linear_extend_batch leaves them
            at += pad
            cstart.append(at); ccount.append(b - a); cstrand.append(int(st[c]))
            Q.append(np.asarray(q[a:b], np.uint32)); T.append(np.asarray(t[a:b], np.uint32)); L.append(np.asarray(ln[a:b], np.int32))
            at += b - a
            pad = (pad + 1) % 3
        coff.append(len(cstart))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt, copy=False) if at else np.zeros(1, dt)
    roff = np.concatenate([[0], np.cumsum(read_lens)]).astype(np.int64)
    tt = lambda a, dt: torch.tensor(np.asarray(a, dtype=dt), device=dev)
    bits = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev)    # uint32 -> the same 32 bits in an int32 tensor
    d = dict(cluster_off=tt(coff, np.int64), c_start=tt(cstart if cstart else [0], np.int64), c_count=tt(ccount if ccount else [0], np.int32),
             c_strand=tt(cstrand if cstrand else [0], np.int32), q=bits(cat(Q, np.uint32)), t=bits(cat(T, np.uint32)), ln=tt(cat(L, np.int32), np.int32),
             roff=tt(roff, np.int64))
    rate = None if rates is None else tt(rates, np.float32)
    res = chain.sparse_dp_batch(ctx, len(reads_in), d["cluster_off"], d["c_start"], d["c_count"], d["c_strand"], d["q"], d["t"], d["ln"], d["roff"],
                                chain.sdp_opts(**opts_kw), rate=rate)
    return res, chain.fetch(ctx, res)


def _compare(out, num_aln, reads_in, read_lens, opts_kw, must_have_result=False, rates=None, oracle_results=None):
    """HIP result `out` against the oracle, read by read, bit for bit (frag_val and chain_value by their bits).  Without must_have_result a read the oracle has no result for
    (status < 0: the reference reads outside its arrays) must be flagged by the device too and is passed over, and the return value is the number of CHAINS compared.
    With must_have_result such a read -- and any non-zero device status -- fails the test, and the return value is the number of READS compared.
    rates: per-read rates (the oracle runs each read with its own); oracle_results: the reads' oracle results where a caller has them already."""
    import oracle_lib as O
    n_chains = 0; n_reads = 0
    for r, (offs, st, q, t, ln) in enumerate(reads_in):
        if oracle_results is not None:
            exp = oracle_results[r]
        else:
            kw = dict(opts_kw) if rates is None else dict(opts_kw, rate=float(rates[r]))
            exp = O.sdp_chain(offs, st, q, t, ln, O.sdp_opts(read_lens[r], **kw))
        if exp["status"] < 0:
            assert not must_have_result, (r, "the oracle has no result", exp["status"])
            assert out["status"][r] != 0, r
            continue
        assert out["status"][r] == 0, (r, out["status"][r])
        f0, f1 = int(out["frag_off"][r]), int(out["frag_off"][r + 1])
        assert f1 - f0 == len(q)
        assert np.array_equal(out["frag_val"][f0:f1].view(np.uint32), exp["val"].view(np.uint32)), r
        assert int(out["n_chains"][r]) == len(exp["chains"]), (r, out["n_chains"][r], len(exp["chains"]))
        for c, ch in enumerate(exp["chains"]):
            s = r * num_aln + c
            a = int(out["chain_start"][s]); m = int(out["chain_len"][s])
            assert m == len(ch["frags"]), (r, c)
            cl = np.searchsorted(offs, ch["frags"], side="right") - 1
            assert np.array_equal(out["chain_cluster"][a:a + m], cl), (r, c)
            assert np.array_equal(out["chain_anchor"][a:a + m], ch["frags"] - offs[cl]), (r, c)
            assert np.array_equal(out["chain_link"][a:a + m - 1], ch["link"]), (r, c)
            assert out["chain_box"][s].tolist() == ch["box"].tolist(), (r, c)
            assert np.float32(out["chain_value"][s]) == np.float32(ch["value"]), (r, c)
            # what the split-chain stage reads: the chain's anchors themselves and their clusters' strands
            assert np.array_equal(out["chain_q"][a:a + m], np.asarray(q, np.uint32)[ch["frags"]]), (r, c)
            assert np.array_equal(out["chain_t"][a:a + m], np.asarray(t, np.uint32)[ch["frags"]]), (r, c)
            assert np.array_equal(out["chain_alen"][a:a + m], np.asarray(ln, np.int32)[ch["frags"]]), (r, c)
            assert np.array_equal(out["chain_strand"][a:a + m], np.asarray(st, np.uint8)[cl]), (r, c)
            n_chains += 1
        n_reads += 1
    return n_reads if must_have_result else n_chains


def _load_jobs(path):
    """jobs written by LRA_SDP_DUMP (lra_amd/csrc/sdp_diag.hip, diag_dump): header (mode, clusters, anchors, read length), rate, cluster offsets, strands, q, t, len"""
    b = open(path, "rb").read(); at = 0; jobs = []
    while at < len(b):
        mode, nc, total, rl = (int(x) for x in np.frombuffer(b, np.int32, 4, at)); at += 16
        rate = float(np.frombuffer(b, np.float32, 1, at)[0]); at += 4
        off = np.frombuffer(b, np.int32, nc + 1, at).copy(); at += 4 * (nc + 1)
        st = np.frombuffer(b, np.uint8, nc, at).copy(); at += nc
        q = np.frombuffer(b, np.uint32, total, at).copy(); at += 4 * total
        t = np.frombuffer(b, np.uint32, total, at).copy(); at += 4 * total
        ln = np.frombuffer(b, np.int32, total, at).copy(); at += 4 * total
        jobs.append((mode, rate, (off, st, q, t, ln)))
    return jobs


# ---------------------------------------------------------------- crafted inputs ---------------------------------------
def _one_cluster(q, t, ln, strand):
    """One cluster of the anchors (q, t, ln), in the order of the lattice case of test_sdp.py: by the diagonal q - t, then by q."""
    q = np.asarray(q, np.int64); t = np.asarray(t, np.int64); ln = np.broadcast_to(np.asarray(ln, np.int64), q.shape)
    assert q.min() >= 0 and t.min() >= 0 and (q + ln).max() < 2 ** 31 and (t + ln).max() < 2 ** 32
    o = np.lexsort((q, q - t))
    return (np.array([0, len(q)], np.int32), np.array([strand], np.uint8), q[o].astype(np.uint32), t[o].astype(np.uint32), ln[o].astype(np.int32))


def sdp_ladder(n, step=37, length=20, base=5000, jitter=50, strand=0, q0=0):
    """n anchors of one length at q = q0 + i step, t = (q - q0) + base + (i % 3) jitter -- for the reverse strand t runs down as q runs up.  With step 37, length 20 and
    jitter 50 no two corners share a row or a column: 2 n distinct rows and 2 n distinct columns."""
    i = np.arange(n, dtype=np.int64)
    q = q0 + i * step
    t = (i if strand == 0 else n - 1 - i) * step + base + (i % 3) * jitter
    return _one_cluster(q, t, length, strand)


def sdp_lattice(n, seed, strand=0):
    """n anchors on the lattice (171 a + 7 b, 171 c + 7 b) of test_sdp.py's workgroup case, cut to size: heavy ties in rows, columns and diagonals."""
    rng = np.random.default_rng(seed)
    m = 4 * n + 64
    a_ = rng.integers(0, 12, m); c_ = rng.integers(0, 12, m); b_ = rng.integers(0, 8, m)
    q = 171 * a_ + 7 * b_; t = 171 * c_ + 7 * b_ + 5000
    _, u = np.unique(q * 100000 + t, return_index=True)
    u = np.sort(u)[:n]
    assert len(u) == n
    return _one_cluster(q[u], t[u], 12, strand)


def sdp_diag_steps(steps, strand=0, length=20, advance=60, base=20000):
    """Anchors whose consecutive diagonals differ by exactly steps[i] (signed): q advances by `advance`, the diagonal (t - q forward, t + q reverse) by the step."""
    steps = np.asarray(steps, np.int64)
    i = np.arange(len(steps) + 1, dtype=np.int64)
    d = np.concatenate([[0], np.cumsum(steps)])
    q = i * advance
    if strand == 0:
        t = q + base + d - d.min()
    else:
        t = base + q.max() + (d - d.min()) - q                   # t + q = a constant + d
    return _one_cluster(q, t, length, strand)


def sdp_merge(*jobs):
    """The clusters of several jobs as one read."""
    offs = [0]; st = []; Q = []; T = []; L = []
    for (o, s, q, t, ln) in jobs:
        for c in range(len(s)):
            a, b = int(o[c]), int(o[c + 1])
            Q.append(q[a:b]); T.append(t[a:b]); L.append(ln[a:b]); st.append(int(s[c])); offs.append(offs[-1] + b - a)
    return (np.array(offs, np.int32), np.array(st, np.uint8), np.concatenate(Q).astype(np.uint32), np.concatenate(T).astype(np.uint32), np.concatenate(L).astype(np.int32))


def sdp_points(job, mode):
    """The points of a job as k_points (sdp_points.hip) makes them -> (q, t, ind, anchor) arrays in insertion order.  Every anchor gives the start / end pair of its
    cluster's strand (forward: (q, t) / (q + len, t + len); reverse: (q, t + len) / (q + len, t)); in cluster mode (mode 0) the first and the last anchor of a cluster
    give the other family's pair as well (SparseDP.h:2159-2166)."""
    offs, st, q, t, ln = job
    q = np.asarray(q, np.int64); t = np.asarray(t, np.int64); ln = np.asarray(ln, np.int64)
    n = len(q)
    cl = np.searchsorted(np.asarray(offs), np.arange(n), side="right") - 1
    strand = np.asarray(st, np.int64)[cl] if n else np.zeros(0, np.int64)
    first = np.isin(np.arange(n), np.asarray(offs[:-1])); last = np.isin(np.arange(n), np.asarray(offs[1:]) - 1)
    edge = (first | last) if mode == 0 else np.zeros(n, bool)
    PQ = []; PT = []; PI = []; PA = []
    for fam, sel in ((0, (strand == 0) | edge), (1, (strand == 1) | edge)):
        a = np.nonzero(sel)[0]
        ts, te = (t[a], t[a] + ln[a]) if fam == 0 else (t[a] + ln[a], t[a])
        PQ += [q[a], q[a] + ln[a]]; PT += [ts, te]; PI += [np.ones(len(a), np.int64), np.zeros(len(a), np.int64)]; PA += [a, a]
    return np.concatenate(PQ), np.concatenate(PT), np.concatenate(PI), np.concatenate(PA)


def sdp_case_shape(job, mode):
    """What decides a job's path through the sparse DP, computed from the definitions in the code: `points` (k_cluster_counts: 2 n in single mode, 2 n + 4 per cluster of
    n >= 2 anchors in cluster mode), the distinct `rows` and `cols` of the points (GetRowInfo / GetColInfo: the levels of the decompositions), and `span` as
    sdp_process_wg defines it: the largest distance, in (q, t, ind) order of the points, from an anchor's first start point to its last end point."""
    pq, pt, ind, anc = sdp_points(job, mode)
    if len(pq) == 0:
        return dict(points=0, rows=0, cols=0, span=0)
    o = np.lexsort((ind, pt, pq))
    pos = np.empty(len(o), np.int64); pos[o] = np.arange(len(o))
    n = int(anc.max()) + 1
    s0 = np.full(n, len(o), np.int64); e1 = np.full(n, -1, np.int64)
    np.minimum.at(s0, anc[ind == 1], pos[ind == 1]); np.maximum.at(e1, anc[ind == 0], pos[ind == 0])
    return dict(points=len(pq), rows=len(np.unique(pq)), cols=len(np.unique(pt)), span=int(max(0, (e1 - s0).max())))
