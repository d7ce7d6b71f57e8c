"""Coordinate-sorted, indexed BAM output against the unsorted BAM output of the device record stage, on one bench-like batch (needs the GPU):

    python tools/time_bam_sorted.py [n_reads=2048] [read_len=30000] [alternations=4]

Both forms run on the same lra_map_result in one session, alternating bam, sorted, bam, sorted, ... after one warm-up of each:
  bam     lra_map_records_device_bam with bgzf = 1: the members in read order;
  sorted  lra_map_records_device_bam_to_sorter, then lra_bam_sorter_finish, every piece of lra_bam_sorter_next, lra_bam_sorter_index.
Per form the wall time; for sorted also the wall time of its four steps and the sorter's own split (lra_bam_sorter_stats: keys + span, the sort, the gather
and the index in HIP events, the compress stage as wall time).  Median and range over the alternations, and one JSON line at the end."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lra_amd import mapread, seed, synth_torch as st
from lra_amd.bam import BamSorter
from lra_amd.context import Context


def med(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    rlen = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    genome = st.make_genome(16_000_000, 1, dev)
    sim = st.simulate_batch(genome, n, rlen, rlen // 10, 0.10, (30, 35, 35), 5)
    reads = torch.cat([sim["seq"], torch.zeros(64, dtype=torch.uint8, device=dev)])
    ik, ip = st.build_global_index(genome, 17, 10, 150)
    mapper = mapread.LowAccMapper(ctx, genome, ik, ip, [b"chr1"], [0, int(genome.numel())])
    d_off = sim["off"]
    rb = seed.read_batch_from_device(ctx, reads, d_off)
    off = d_off.cpu().numpy(); h = reads.cpu().numpy()
    rl = [h[off[i]:off[i + 1]].tobytes() for i in range(n)]
    rng = np.random.default_rng(1)
    ql = [bytes(rng.integers(43, 74, len(r)).astype(np.uint8)) for r in rl]
    names = [b"read%d" % i for i in range(n)]
    args = mapper.record_args(names, rl, ql)
    kw = dict(d_qual=torch.from_numpy(np.frombuffer(b"".join(ql), np.uint8).copy()).to(dev),
              d_qual_off=torch.from_numpy(np.concatenate([[0], np.cumsum([len(q) for q in ql])]).astype(np.int64)).to(dev))
    del sim
    torch.cuda.empty_cache()
    res = mapper.align(rb)
    mapper.copts.printFormat = ord("s")
    sorter = BamSorter(ctx, 8 << 30)
    ref_len = [int(genome.numel())]
    keys = ("encode_add", "finish", "next", "index", "total")
    runs = dict(bam=[], **{k: [] for k in keys}, **{"dev_" + k: [] for k in ("keys_span", "sort", "gather", "compress", "index")})
    sizes = {}

    def bam():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = mapper.records_device_bam(res, args, bgzf=True, **kw)
        sizes["bam_members"] = len(r[0])
        return (time.perf_counter() - t0) * 1e3

    def sort():
        torch.cuda.synchronize()
        t = [time.perf_counter()]
        mapper.records_device_bam_to_sorter(res, args, sorter, **kw)
        t.append(time.perf_counter())
        sizes["records"], sizes["stream_bytes"] = sorter.held()
        sorter.finish(1000, ref_len)
        t.append(time.perf_counter())
        sizes["sorted_members"] = sum(len(p) for p in sorter.pieces())
        t.append(time.perf_counter())
        sizes["bai_bytes"] = len(sorter.index())
        t.append(time.perf_counter())
        d = [(b - a) * 1e3 for a, b in zip(t, t[1:])]
        return dict(zip(keys, d + [sum(d)])), sorter.stats()

    bam(); sort()                                                               # warm-up: the kept buffers reach their sizes
    for _ in range(reps):
        runs["bam"].append(bam())
        w, s = sort()
        for k in keys:
            runs[k].append(w[k])
        for k, v in s.items():
            runs["dev_" + k].append(v)
    out = dict(n_reads=n, bases=int(off[-1]), alternations=reps, **sizes, **{k: med(v) for k, v in runs.items()})
    print("bam (bgzf = 1): wall %.1f ms (%.1f-%.1f), %.1f MB of members" % (*out["bam"], sizes["bam_members"] / 1e6), flush=True)
    print("sorted: %d records, stream %.1f MB, members %.1f MB, .bai %d bytes; wall %s"
          % (sizes["records"], sizes["stream_bytes"] / 1e6, sizes["sorted_members"] / 1e6, sizes["bai_bytes"],
             "  ".join("%s %.2f ms (%.2f-%.2f)" % (k, *out[k]) for k in keys)), flush=True)
    print("sorter's split: " + "  ".join("%s %.3f ms (%.3f-%.3f)" % (k[4:], *out[k]) for k in runs if k.startswith("dev_")), flush=True)
    print(json.dumps(out))
    sorter.close()
    ctx.close()


if __name__ == "__main__":
    main()
