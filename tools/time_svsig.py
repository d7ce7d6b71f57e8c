"""What the SV signatures cost the record stage (LRA_PACK_SVSIG): one batch mapped once, then its snapshot with no flag, with LRA_PACK_MD (the yardstick)
and with LRA_PACK_SVSIG, and the host printer.
  --preset ont     -ONT reads against a synthetic reference (lra_map_reads_lowacc_batch); every --plant-every'th read carries one indel of 40-300 bases
  --preset contig  -CONTIG contigs against a synthetic reference (lra_map_reads_highacc_batch): few alignments of 10^5 blocks and more
One JSON line: snapshot ms (pack + the stage + copy) per flag word, the printer's ms, the signature count and bytes.  For the kernels' own time run it under
`rocprofv3 --kernel-trace --stats` (kernels sv_count, sv_cut, sv_emit, sv_copy and the scans' tile_sum / part_scan / tile_scan)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=["ont", "contig"], default="ont")
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--read-len", type=int, default=0)
    ap.add_argument("--genome", type=int, default=0, help="reference length (bases)")
    ap.add_argument("--plant-every", type=int, default=4)
    ap.add_argument("--svsig-len", type=int, default=25)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from lra_amd.context import Context
    from lra_amd import seed, mapread, synth, parallel
    P = {"ont": dict(reads=4096, read_len=20000, genome=40_000_000, err=0.10, sd=5000),
         "contig": dict(reads=64, read_len=1_000_000, genome=80_000_000, err=0.002, sd=200_000)}[args.preset]
    n_reads, rlen, G = args.reads or P["reads"], args.read_len or P["read_len"], args.genome or P["genome"]
    ctx = Context(0)
    genome = synth.make_genome(G, seed=11, repeat_frac=0.05, n_families=4)
    CH = [0, G // 2, G]
    names = [b"chr1", b"chr2"]
    reads, _ = synth.simulate_reads(genome, n_reads, rlen, P["sd"], P["err"], (34, 33, 33) if args.preset == "contig" else (30, 35, 35), seed=3)
    rng = np.random.default_rng(8)
    for n, i in enumerate(range(0, len(reads), max(1, args.plant_every))):  # one indel in the middle third: bases cut out of the read, or random bases put in
        r = reads[i]
        at = int(rng.integers(len(r) // 3, 2 * len(r) // 3)); size = int(rng.integers(40, 301))
        reads[i] = np.concatenate([r[:at], r[at + size:]]) if n % 2 else np.concatenate([r[:at], synth.BASES[rng.integers(0, 4, size)], r[at:]])
    reads = [np.ascontiguousarray(r).tobytes() for r in reads]
    if args.preset == "ont":
        o = mapread.LowAccOptions(svsigLen=args.svsig_len)
        ik, ip = synth.build_global_index(genome, o.globalK, o.globalW, o.globalMaxFreq)
        mapper = mapread.LowAccMapper(ctx, genome, ik, ip, names, CH, o)
    else:
        mapper = mapread.HighAccMapper(ctx, genome, None, None, names, CH, "contig", svsigLen=args.svsig_len)
    batch = seed.ReadBatch(ctx, reads)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = mapper.align(batch)
    torch.cuda.synchronize()
    t_map = (time.perf_counter() - t0) * 1e3
    rnames = [b"read%d" % i for i in range(len(reads))]
    out = dict(preset=args.preset, reads=len(reads), bases=int(sum(len(r) for r in reads)), alignments=int(res.n_alignments), blocks=int(res.n_blocks),
               map_ms=round(t_map, 1), svsig_len=args.svsig_len)
    forms = (("plain", dict(md=False)), ("md", dict(md=True)), ("svsig", dict(md=False, svsig=True)))
    for k, kw in forms + forms:
        snap_ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            snap = mapper.snapshot(res, **kw)
            snap_ms.append((time.perf_counter() - t0) * 1e3)
            ctx.lib.lra_map_host_free(snap)
        out["snapshot_ms_" + k] = round(min(snap_ms), 2)
    snap = mapper.snapshot(res, md=False, svsig=True)
    t0 = time.perf_counter()
    text = mapper.svsig_host(snap, rnames)
    out["print_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    joined = b"".join(text)
    out["signatures"] = joined.count(b"\n"); out["ins"] = joined.count(b"\tINS\t"); out["del"] = joined.count(b"\tDEL\t"); out["text_bytes"] = len(joined)
    pk = parallel.pack_records(ctx, res, svsig=True)
    hdr = np.frombuffer(pk[:128].tobytes(), np.int64)
    nA, sec = int(res.n_alignments), len(pk) - int(hdr[12])                # the section is the pack's tail: sig_off u64[nA + 1] | 24-byte records | the bases
    n_packed = int(np.frombuffer(pk[sec + 8 * nA:sec + 8 * nA + 8].tobytes(), np.uint64)[0])
    out["packed_signatures"] = n_packed                                    # (those of flagged reads are packed and not printed)
    out["section_bytes"] = int(hdr[12])
    out["sequence_bytes"] = int(hdr[12]) - 8 * (nA + 1) - 24 * n_packed    # (padded to 8)
    out["md_bytes"] = int(np.frombuffer(parallel.pack_records(ctx, res, print_md=True)[:128].tobytes(), np.int64)[10])
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
