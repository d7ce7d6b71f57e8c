"""What --printMD costs the record stage (LRA_PACK_MD): one batch mapped once, then its snapshot and its SAM text with and without the MD strings.
  --preset ont     -ONT reads against a synthetic reference (lra_map_reads_lowacc_batch)
  --preset contig  -CONTIG contigs against a synthetic reference (lra_map_reads_highacc_batch): few alignments of 10^5 blocks and more
One JSON line: snapshot ms (pack + lra_md_strings_batch + copy) and host record ms, each with and without MD, MD bytes, SAM bytes.  For the MD kernels' own
time run it under `rocprofv3 --kernel-trace --stats` (kernels md_segments, md_walk, md_resolve, md_seg_fill)."""
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
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from lra_amd.context import Context
    from lra_amd import seed, mapread, synth
    P = {"ont": dict(reads=4096, read_len=20000, genome=40_000_000, err=0.10, sd=5000),
         "contig": dict(reads=64, read_len=1_000_000, genome=80_000_000, err=0.002, sd=200_000)}[args.preset]
    n_reads, rlen, G = args.reads or P["reads"], args.read_len or P["read_len"], args.genome or P["genome"]
    ctx = Context(0)
    genome = synth.make_genome(G, seed=11, repeat_frac=0.05, n_families=4)
    CH = [0, G // 2, G]
    names = [b"chr1", b"chr2"]
    reads, _ = synth.simulate_reads(genome, n_reads, rlen, P["sd"], P["err"], (34, 33, 33) if args.preset == "contig" else (30, 35, 35), seed=3)
    reads = [r.tobytes() for r in reads]
    if args.preset == "ont":
        o = mapread.LowAccOptions()
        ik, ip = synth.build_global_index(genome, o.globalK, o.globalW, o.globalMaxFreq)
        mapper = mapread.LowAccMapper(ctx, genome, ik, ip, names, CH, o)
    else:
        mapper = mapread.HighAccMapper(ctx, genome, None, None, names, CH, "contig")
    batch = seed.ReadBatch(ctx, reads)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = mapper.align(batch)
    torch.cuda.synchronize()
    t_map = (time.perf_counter() - t0) * 1e3
    rargs = mapper.record_args([b"read%d" % i for i in range(len(reads))], reads)
    out = dict(preset=args.preset, reads=len(reads), bases=int(sum(len(r) for r in reads)), alignments=int(res.n_alignments), blocks=int(res.n_blocks),
               map_ms=round(t_map, 1))
    for md in (False, True, False, True):
        snap_ms, rec_ms = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            snap = mapper.snapshot(res, md=md)
            t1 = time.perf_counter()
            n_text = mapper.records_host(snap, rargs, as_list=False)
            t2 = time.perf_counter()
            snap_ms.append((t1 - t0) * 1e3); rec_ms.append((t2 - t1) * 1e3)
        k = "md" if md else "plain"
        out["snapshot_ms_" + k] = round(min(snap_ms), 2)
        out["records_ms_" + k] = round(min(rec_ms), 2)
        out["sam_bytes_" + k] = int(n_text)
    from lra_amd import parallel
    pk = parallel.pack_records(ctx, res, print_md=True)
    out["md_bytes"] = int(np.frombuffer(pk[:128].tobytes(), np.int64)[10])
    bases = out["bases"]
    for k in ("plain", "md"):
        out["gbps_" + k] = round(bases / ((t_map + out["snapshot_ms_" + k] + out["records_ms_" + k]) * 1e-3) / 1e9, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
