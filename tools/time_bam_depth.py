"""The device BAM depth on a coordinate-sorted BAM with its .bai, beside the device view of the same file and the host oracle (needs the GPU):

    python tools/time_bam_depth.py sorted.bam [repeats=3] [oracle=1]

`tools/time_bam_view.py ... keep=sorted.bam` writes the bench-size file.  Each pass `repeats` times after one warm-up, wall time from create to the last
piece through the Python wrapper, median and range: lra_bam_view over the whole file and over 1 Mb in the middle of the first reference (the floor the
two share: read + inflate + frame); lra_bam_depth per base with values only, per base with the text of the covered positions, --bin 1000, and the same
1 Mb region; lra_bam_depth's own split of every whole-file pass (lra_bam_depth_stats).  oracle: tests/depth_ref.py's loop over the same records (parsed
on the host from the inflated file), once, and its values compared with the device's.  One JSON line at the end."""
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from lra_amd.bam import BamDepth, BamView
from lra_amd.context import Context

STAGES = ("ms_read_inflate", "ms_frame_select", "ms_ops", "ms_accumulate", "ms_finish", "ms_text", "ms_copy")


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


def main():
    path = sys.argv[1]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    oracle = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    bai = path + ".bai"
    ctx = Context(0)
    out = dict(file_bytes=os.path.getsize(path), repeats=reps)

    def view(region):
        v = BamView(ctx, path, bai)
        n = sum(len(p) for p in v.fetch(*region))
        v.close()
        return n

    def depth(region, **kw):
        d = BamDepth(ctx, path, bai, **kw)
        n = k = 0
        for _, _, count, _, text in d.fetch(*region):
            n += len(text); k += count
        s = d.stats()
        d.close()
        return n, k, s

    d0 = BamDepth(ctx, path, bai)
    names, lens = d0.header()
    d0.close()
    mid = lens[0] // 2
    reg = (0, mid, mid + 1_000_000)
    for name, region in (("whole", ()), ("region_1mb", reg)):
        out["view_" + name], n = timed(reps, lambda: view(region))
        print("view %s: %.1f MB of text, %.1f ms (%.1f-%.1f)" % (name, n / 1e6, *out["view_" + name]), flush=True)
        for label, kw in (("values", dict(text=False, values=True)), ("text", dict()), ("bin1000", dict(bin=1000))):
            t, (n, k, s) = timed(reps, lambda: depth(region, **kw))
            out["depth_%s_%s" % (label, name)] = dict(ms=t, text_bytes=n, count=k, stats=s)
            print("depth %s %s: %d positions / bins, %.2f MB of text, %.1f ms (%.1f-%.1f); " % (label, name, k, n / 1e6, *t) +
                  "  ".join("%s %.3f" % (x[3:], s[x]) for x in STAGES) + "; windows %d slides %d covered %d max %d" %
                  (s["windows"], s["slides"], s["covered"], s["depth_max"]), flush=True)
    if oracle:
        import bam_text
        import depth_ref
        from test_bam_depth_device import parse
        t0 = time.perf_counter()
        raw = bam_text.inflate(open(path, "rb").read())
        _, refs, at = bam_text.parse_header(raw)
        recs = []
        while at < len(raw):
            (bs,) = struct.unpack_from("<I", raw, at)
            recs.append(parse(raw[at:at + 4 + bs]))
            at += 4 + bs
        t1 = time.perf_counter()
        want = depth_ref.depth(recs, lens)
        t2 = time.perf_counter()
        d = BamDepth(ctx, path, bai, text=False, values=True)
        got = [np.zeros(n, np.uint32) for n in lens]
        for ref, first, count, v, _ in d.fetch():
            got[ref][first:first + count] = v
        d.close()
        same = all(np.array_equal(a, b) for a, b in zip(got, want))
        out["oracle"] = dict(parse_ms=(t1 - t0) * 1e3, loop_ms=(t2 - t1) * 1e3, records=len(recs), ops=sum(len(r[4]) for r in recs), same=bool(same))
        print("host oracle: %d records, %d ops: inflate + parse %.0f ms, the loop %.0f ms; the device's values are %s" %
              (len(recs), out["oracle"]["ops"], out["oracle"]["parse_ms"], out["oracle"]["loop_ms"], "the same" if same else "DIFFERENT"), flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
