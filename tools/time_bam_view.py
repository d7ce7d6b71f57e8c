"""The device BAM view on the sorted BAM of one bench-like batch (needs the GPU):

    python tools/time_bam_view.py [n_reads=2048] [read_len=30000] [repeats=3] [window_bytes=0] [keep=PATH]

The batch's BAM records (lra_map_records_device_bam) are sorted by the device sorter and written, with their .bai, to a temporary directory: the file
tools/time_bam_sorted.py times the writing of.  Then lra_bam_view, `repeats` times after one warm-up: the whole file as SAM text -- wall time, the view's
own split (lra_bam_view_stats: read + inflate, frame + select, tags + lengths, the floats' round trip, emit, the copy to the host) and the MB/s of text
-- and the latency of a region of 1 kb and of 1 Mb in the middle of the reference (region call to the last piece, on an open view).  Median and
range, and one JSON line.  keep: the sorted file and its index are also written to PATH and PATH.bai (tools/time_bam_depth.py reads them)."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lra_amd import bgzf, deflate, mapread, seed, synth_torch as st
from lra_amd.bam import BamSorter, BamView
from lra_amd.context import Context

STAGES = ("ms_read_inflate", "ms_frame_select", "ms_tags_lengths", "ms_floats", "ms_emit", "ms_copy")


def med(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    rlen = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    window = int(sys.argv[4]) if len(sys.argv) > 4 else 0
    keep = sys.argv[5] if len(sys.argv) > 5 else None
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
    lens, at = [], 0
    while at < len(raw):
        bs = int(np.frombuffer(raw, "<u4", 1, at)[0])
        lens.append(4 + bs)
        at += 4 + bs
    ref_len = [int(genome.numel())]
    head_raw = mapper.bam_header(b"@HD\tVN:1.6\tSO:coordinate\n")
    head = b"".join(deflate.deflate_members([head_raw[a:a + deflate.IN_MAX] for a in range(0, len(head_raw), deflate.IN_MAX)])[0])
    stream = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)
    starts = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
    sorter = BamSorter(ctx, 8 << 30)
    sorter.add(stream, starts)
    sorter.finish(len(head), ref_len)
    data = b"".join(sorter.pieces())
    bai = sorter.index()
    sorter.close()
    del stream, starts
    out = dict(n_reads=n, records=len(lens), stream_bytes=len(raw), repeats=reps, window_bytes=window)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sorted.bam")
        with open(path, "wb") as f:
            f.write(head + data + bgzf.EOF_BLOCK)
        with open(path + ".bai", "wb") as f:
            f.write(bai)
        if keep:
            for suffix, blob in (("", head + data + bgzf.EOF_BLOCK), (".bai", bai)):
                with open(keep + suffix, "wb") as f:
                    f.write(blob)
        out["file_bytes"] = os.path.getsize(path)
        runs = {s: [] for s in ("wall",) + STAGES}
        text_bytes = 0
        for it in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = BamView(ctx, path, None, window)
            text_bytes = sum(len(p) for p in v.fetch())
            w = (time.perf_counter() - t0) * 1e3
            s = v.stats()
            v.close()
            assert s["records"] == len(lens)
            if it:
                runs["wall"].append(w)
                for x in STAGES:
                    runs[x].append(s[x])
        r = {x: med(v) for x, v in runs.items()}
        r.update(text_bytes=text_bytes, windows=s["windows"], mb_per_s=text_bytes / 1e6 / (r["wall"][0] / 1e3))
        out["whole"] = r
        print("whole file: %d records, %.1f MB of BAM -> %.1f MB of text in %d windows; wall %.1f ms (%.1f-%.1f), %.0f MB/s of text; "
              % (len(lens), out["file_bytes"] / 1e6, text_bytes / 1e6, r["windows"], *r["wall"], r["mb_per_s"]) +
              "  ".join("%s %.3f" % (x[3:], r[x][0]) for x in STAGES), flush=True)
        v = BamView(ctx, path, path + ".bai", window)
        mid = ref_len[0] // 2
        for name, span in (("region_1kb", 1000), ("region_1mb", 1_000_000)):
            t, k, b = [], 0, 0
            for it in range(reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                b = sum(len(p) for p in v.fetch(0, mid, mid + span))
                w = (time.perf_counter() - t0) * 1e3
                k = v.last_records
                if it:
                    t.append(w)
            out[name] = dict(ms=med(t), records=k, text_bytes=b)
            print("%s: %d records, %.2f MB of text, %.2f ms (%.2f-%.2f)" % (name, k, b / 1e6, *out[name]["ms"]), flush=True)
        v.close()
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
