"""The device combination of two haplotypes' assembly SV calls, beside the two one-haplotype passes it is made of (needs the GPU):

    python tools/time_bam_svcombine.py [genome_bases=16000000] [contig_bases=1000000] [site_every=4000] [repeats=5] [oracle=1] [genome_seed=1]

Two synthetic contig haplotypes over synth_torch.make_genome(genome_bases, genome_seed): contigs of contig_bases tile the reference with a tenth of overlap;
a site every site_every bases is a deletion or an insertion of 40 - 400 bases; a haplotype carries a site with probability 0.8, and its copy of a shared
site is moved by up to 8 bases and resized by up to a tenth, so that partners are found by the fraction, not by equality.  Each haplotype's contigs are
written as a coordinate-sorted BAM (host zlib, level 1) into a temporary directory and read from the page cache.  Timed `repeats` times after one warm-up,
wall time through the Python wrapper, median and range: two lra_bam_svcalls passes with text, one after the other (what two runs of tools/svcalls_bam.py
do in one process -- the pass without a sink is the parent commit's), and lra_sv_combine from create to the last piece, with its own split
(lra_sv_combine_stats: the two passes, classify, emit, copy).  oracle: tests/svcombine_ref.py over the same records, once, compared with the device's
pieces.  One JSON line at the end."""
import json
import os
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np
import torch

from lra_amd import bgzf, synth_torch as st
from lra_amd.bam import BamSvCalls, SvCombine
from lra_amd.context import Context
from lra_amd.index import load_genome

CODE = np.zeros(256, np.uint8)
for k, c in enumerate(b"=ACMGRSVTWYHKDBN"):
    CODE[c] = k


def med(v):
    return [float(np.median(v)), float(min(v)), float(max(v))]


def timed(reps, fn):
    t, last = [], None
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn()
        if it:
            t.append((time.perf_counter() - t0) * 1e3)
    return med(t), last


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def contig_record(genome, pos, end, sites, name, rng):
    """the contig that aligns to [pos, end) with the sites [(anchor, length, kind)] inside it: M runs of the genome's own bases between the variants"""
    ops, parts, cur = [], [], pos
    for anchor, ln, kind in sites:
        ops.append(((anchor + 1 - cur) << 4) | 0)
        parts.append(genome[cur:anchor + 1])
        cur = anchor + 1
        if kind == "D":
            ops.append((ln << 4) | 2)
            cur += ln
        else:
            ops.append((ln << 4) | 1)
            parts.append(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)])
    ops.append(((end - cur) << 4) | 0)
    parts.append(genome[cur:end])
    seq = np.concatenate(parts)
    nib = CODE[seq]
    if len(nib) & 1:
        nib = np.concatenate([nib, np.zeros(1, np.uint8)])
    packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
    body = struct.pack("<iiBBHHHIiii", 0, pos, len(name) + 1, 60, reg2bin(pos, end), len(ops), 0, len(seq), -1, -1, end - pos) + name + b"\0"
    body += struct.pack("<%dI" % len(ops), *ops) + packed + b"\xff" * len(seq)
    return struct.pack("<I", len(body)) + body


def haplotype(genome, contig, sites, take, jitter, tag, rng):
    """-> the records of one haplotype's contigs in coordinate order"""
    n, recs, c, step = len(genome), [], 0, contig - contig // 10
    for pos in range(1000, n - 1000, step):
        end = min(pos + contig, n - 1000)
        mine = []
        for k, (anchor, ln, kind) in enumerate(sites):
            if not take[k] or anchor < pos + 500 or anchor + 2 * ln + 600 > end:
                continue
            a, l2 = anchor + int(jitter[k][0]), max(40, ln + int(jitter[k][1] * ln / 10))
            mine.append((a, l2, kind))
        recs.append(contig_record(genome, pos, end, mine, b"%s_ctg%d" % (tag, c), rng))
        c += 1
    return recs


def write_bam(path, recs, ref_len):
    head = b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", 1) + struct.pack("<I", 5) + b"chr1\0" + struct.pack("<I", ref_len)
    with open(path, "wb") as f:
        f.write(bgzf.bgzf_compress(head, 6, eof=False) + bgzf.bgzf_compress(b"".join(recs), 1, eof=True))


def main():
    a = [int(x) for x in sys.argv[1:]]
    n, contig, every, reps, oracle, seed = (a + [16_000_000, 1_000_000, 4000, 5, 1, 1][len(a):])[:6]
    ctx = Context(0)
    d_genome = st.make_genome(n, seed, torch.device("cuda", 0))
    load_genome(ctx, d_genome)
    ctx.check(ctx.lib.lra_ctx_load_chromosomes(ctx.h, (C.c_uint64 * 2)(0, n), 1))
    genome = d_genome.cpu().numpy()
    rng = np.random.default_rng(seed)
    sites = [(int(p), int(rng.integers(40, 401)), "D" if rng.integers(0, 2) else "I") for p in range(5000, n - 5000, every)]
    out = dict(genome_bases=n, contig_bases=contig, sites=len(sites), repeats=reps)
    with tempfile.TemporaryDirectory() as tmp:
        path, recs = {}, {}
        for hap in ("maternal", "paternal"):
            take = rng.random(len(sites)) < 0.8
            jitter = rng.integers(-8, 9, (len(sites), 2)) if hap == "paternal" else np.zeros((len(sites), 2), np.int64)
            recs[hap] = haplotype(genome, contig, sites, take, jitter, hap[0].encode(), rng)
            path[hap] = os.path.join(tmp, hap + ".bam")
            write_bam(path[hap], recs[hap], n)
            out[hap] = dict(records=len(recs[hap]), file_bytes=os.path.getsize(path[hap]))

        def two_passes():
            k = nb = 0
            for hap in path:
                d = BamSvCalls(ctx, path[hap], hap=hap, vcf_columns=True)
                for _, _, count, _, text in d.fetch():
                    k += count; nb += len(text)
                d.close()
            return k, nb

        def combine():
            d = SvCombine(ctx, path["maternal"], path["paternal"])
            pieces = [(hap, kind, cls, count, text) for hap, kind, cls, count, _, text in d.fetch()]
            s = d.stats()
            d.close()
            return pieces, s

        t2, (k2, nb2) = timed(reps, two_passes)
        out["two_svcalls"] = dict(ms=t2, rows=k2, text_bytes=nb2)
        print("two lra_bam_svcalls passes, text: %d rows, %.3f MB, %.1f ms (%.1f-%.1f)" % (k2, nb2 / 1e6, *t2), flush=True)
        tc, (pieces, s) = timed(reps, combine)
        flat = {k: v for k, v in s.items() if k != "passes"}
        out["combine"] = dict(ms=tc, stats=flat, passes=s["passes"], pieces=[p[:4] for p in pieces])
        print("lra_sv_combine: %.1f ms (%.1f-%.1f); pass m %.1f  pass p %.1f  classify %.3f  emit %.3f  copy %.3f; het m %d/%d  het p %d/%d  hom %d/%d  partnered p %d/%d "
              "(INS/DEL); %.3f MB of text; the passes kept %d/%d and %d/%d" %
              (*tc, s["ms_pass_m"], s["ms_pass_p"], s["ms_classify"], s["ms_emit"], s["ms_copy"], s["het_m_ins"], s["het_m_del"], s["het_p_ins"], s["het_p_del"], s["hom_ins"],
               s["hom_del"], s["partnered_p_ins"], s["partnered_p_del"], s["bytes_text"] / 1e6, s["passes"][0]["kept_ins"], s["passes"][0]["kept_del"],
               s["passes"][1]["kept_ins"], s["passes"][1]["kept_del"]), flush=True)
        if oracle:
            import bam_text
            import svcalls_ref
            import svcombine_ref
            import vcf_ref
            t0 = time.perf_counter()
            P = {h: [vcf_ref.parse_record(r, bam_text._tags) for r in recs[h]] for h in recs}
            cores = {h: [svcalls_ref.core_of(r) for r in recs[h]] for h in recs}
            want, wst, _, _ = svcombine_ref.run(P["maternal"], cores["maternal"], P["paternal"], cores["paternal"], [b"chr1"], [genome.tobytes()])
            same = [(w[0], w[1], w[2], w[3]) for w in want] == [(p[0], p[1], p[2], p[4]) for p in pieces]
            out["oracle"] = dict(ms=(time.perf_counter() - t0) * 1e3, same=bool(same), stats=wst)
            print("host oracle: %.0f ms; %s; the device's pieces are %s" % (out["oracle"]["ms"], wst, "the same" if same else "DIFFERENT"), flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
