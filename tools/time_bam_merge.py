"""The device merge of sorted BAM runs against the device sorter on the same records, on one bench-like batch (needs the GPU):

    python tools/time_bam_merge.py [n_reads=2048] [read_len=30000] [repeats=3] [window_bytes=0]

The batch's BAM records (lra_map_records_device_bam, read order) are cut into k = 2, 8 and 32 consecutive slices; each slice, sorted, becomes a run file
(its members from the device compress stage) in a temporary directory.  Per k: lra_bam_merger over the k files at the given window (0: the default, from
the budget of 8 GiB) -- create, every piece, index -- `repeats` times after one warm-up: the wall time, the merger's own split (lra_bam_merger_stats) and
the MB/s of merged record bytes.  Beside them the sorter on the same records in one run (lra_bam_sorter: add, finish, every piece, index), the yardstick:
the merger's bound + rank + gather against the sorter's sort + gather is what merging by ranks costs at that k.  Median and range, and one JSON line."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lra_amd import bgzf, deflate, mapread, seed, synth_torch as st
from lra_amd.bam import BamMerger, BamSorter
from lra_amd.context import Context

STAGES = ("ms_read_inflate", "ms_frame_keys", "ms_bound_rank", "ms_gather_span", "ms_compress", "ms_index")


def med(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def sort_key(rec):
    ref, pos = np.frombuffer(rec, "<i4", 2, 4)
    flag = int(np.frombuffer(rec, "<u2", 1, 18)[0])
    return (int(ref) & 0xffffffff, int(pos), flag & 16)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    rlen = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    window = int(sys.argv[4]) if len(sys.argv) > 4 else 0
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
    args = mapper.record_args([b"read%d" % i for i in range(n)], rl, ql)
    kw = dict(d_qual=torch.from_numpy(np.frombuffer(b"".join(ql), np.uint8).copy()).to(dev),
              d_qual_off=torch.from_numpy(np.concatenate([[0], np.cumsum([len(q) for q in ql])]).astype(np.int64)).to(dev))
    del sim
    torch.cuda.empty_cache()
    res = mapper.align(rb)
    mapper.copts.printFormat = ord("s")
    raw, _ = mapper.records_device_bam(res, args, **kw)
    recs, at = [], 0
    while at < len(raw):
        bs = int(np.frombuffer(raw, "<u4", 1, at)[0])
        recs.append(raw[at:at + 4 + bs])
        at += 4 + bs
    ref_len = [int(genome.numel())]
    head_raw = mapper.bam_header(b"@HD\tVN:1.6\tSO:coordinate\n")
    head = b"".join(deflate.deflate_members([head_raw[a:a + deflate.IN_MAX] for a in range(0, len(head_raw), deflate.IN_MAX)])[0])
    out = dict(n_reads=n, records=len(recs), stream_bytes=len(raw), repeats=reps, window_bytes=window)

    # the yardstick: the sorter on the same records in one run
    stream = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)
    starts = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)).to(dev)
    sorter = BamSorter(ctx, 8 << 30)
    sruns = {k: [] for k in ("wall", "keys_span", "sort", "gather", "compress", "index")}
    want = None
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sorter.add(stream, starts)
        sorter.finish(len(head), ref_len)
        data = b"".join(sorter.pieces())
        bai = sorter.index()
        w = (time.perf_counter() - t0) * 1e3
        want = (data, bai)
        if it:
            sruns["wall"].append(w)
            for k, v in sorter.stats().items():
                sruns[k].append(v)
    sorter.close()
    out["sorter"] = {k: med(v) for k, v in sruns.items()}
    print("sorter, one run: wall %.1f ms (%.1f-%.1f); " % out["sorter"]["wall"] +
          "  ".join("%s %.3f ms" % (k, out["sorter"][k][0]) for k in ("keys_span", "sort", "gather", "compress", "index")), flush=True)

    with tempfile.TemporaryDirectory() as d:
        for k in (2, 8, 32):
            per = (len(recs) + k - 1) // k
            paths = []
            for i in range(k):
                part = sorted(recs[i * per:(i + 1) * per], key=sort_key)
                paths.append(os.path.join(d, "k%d.run%04d.bam" % (k, i)))
                with open(paths[-1], "wb") as f:
                    f.write(head + (deflate.compress_device(ctx, b"".join(part))[0] if part else b"") + bgzf.EOF_BLOCK)
            runs = {s: [] for s in ("wall",) + STAGES}
            for it in range(reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = BamMerger(ctx, paths, 8 << 30, len(head), window)
                data = b"".join(m.pieces())
                bai = m.index()
                w = (time.perf_counter() - t0) * 1e3
                s = m.stats()
                m.close()
                assert (data, bai) == want, "the merged file is not the sorter's"
                if it:
                    runs["wall"].append(w)
                    for x in STAGES:
                        runs[x].append(s[x])
            r = {x: med(v) for x, v in runs.items()}
            r.update(rounds=s["rounds"], peak_device_bytes=s["peak_device_bytes"], file_bytes=sum(os.path.getsize(p) for p in paths),
                     mb_per_s=len(raw) / 1e6 / (r["wall"][0] / 1e3))
            out["k%d" % k] = r
            print("k = %2d: %d rounds, peak %.1f MB, wall %.1f ms (%.1f-%.1f), %.0f MB/s of records; " % (k, r["rounds"], r["peak_device_bytes"] / 1e6, *r["wall"], r["mb_per_s"]) +
                  "  ".join("%s %.3f" % (x[3:], r[x][0]) for x in STAGES), flush=True)
            print("        bound + rank + gather + span %.3f ms against the sorter's sort + gather (+ its span in keys_span) %.3f ms"
                  % (r["ms_bound_rank"][0] + r["ms_gather_span"][0], out["sorter"]["sort"][0] + out["sorter"]["gather"][0]), flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
