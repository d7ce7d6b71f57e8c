"""The device BAM-to-VCF pass on a coordinate-sorted BAM with its .bai, beside the device view of the same file and the host oracle (needs the GPU):

    python tools/time_bam_vcf.py sorted.bam [repeats=3] [oracle=1] [genome_seed=1]

`tools/time_bam_view.py ... keep=sorted.bam` writes the bench-size file; its genome is synth_torch.make_genome(<the reference's length>, genome_seed),
made again here and loaded into the context.  Each pass `repeats` times after one warm-up, wall time from create to the last piece through the Python
wrapper, median and range: lra_bam_view over the whole file and over 1 Mb in the middle of the first reference; lra_bam_vcf with text, with values
only, with --minLength 20, and the same 1 Mb region; lra_bam_vcf's own split of every pass (lra_bam_vcf_stats) and the view's.  oracle:
tests/vcf_ref.py's walk over the same records (parsed on the host from the inflated file), once, and its text compared with the device's.  One JSON
line at the end."""
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np
import torch

from lra_amd import synth_torch as st
from lra_amd.bam import BamVcf, BamView
from lra_amd.context import Context
from lra_amd.index import load_genome

STAGES = ("ms_read_inflate", "ms_frame_select", "ms_ops", "ms_walk", "ms_lengths", "ms_emit", "ms_copy")
VIEW_STAGES = ("ms_read_inflate", "ms_frame_select", "ms_tags_lengths", "ms_floats", "ms_emit", "ms_copy")


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
    seed = int(sys.argv[4]) if len(sys.argv) > 4 else 1
    bai = path + ".bai"
    ctx = Context(0)
    out = dict(file_bytes=os.path.getsize(path), repeats=reps)
    v0 = BamView(ctx, path, bai)
    _, names, lens = v0.header()
    v0.close()
    assert len(lens) == 1, "the bench-size file has one reference"
    genome = st.make_genome(int(lens[0]), seed, torch.device("cuda", 0))
    load_genome(ctx, genome)
    ctx.check(ctx.lib.lra_ctx_load_chromosomes(ctx.h, (C.c_uint64 * 2)(0, int(lens[0])), 1))

    def view(region):
        v = BamView(ctx, path, bai)
        n = sum(len(p) for p in v.fetch(*region))
        s = v.stats()
        v.close()
        return n, s

    def vcf(region, **kw):
        d = BamVcf(ctx, path, bai, **kw)
        n = k = 0
        for count, _, text in d.fetch(*region):
            n += len(text); k += count
        s = d.stats()
        d.close()
        return n, k, s

    mid = int(lens[0]) // 2
    reg = (0, mid, mid + 1_000_000)
    for name, region in (("whole", ()), ("region_1mb", reg)):
        t, (n, s) = timed(reps, lambda: view(region))
        out["view_" + name] = dict(ms=t, text_bytes=n, stats=s)
        print("view %s: %.1f MB of text, %.1f ms (%.1f-%.1f); " % (name, n / 1e6, *t) + "  ".join("%s %.3f" % (x[3:], s[x]) for x in VIEW_STAGES), flush=True)
        for label, kw in (("text", dict()), ("values", dict(text=False, values=True)), ("min20", dict(min_length=20))):
            t, (n, k, s) = timed(reps, lambda: vcf(region, **kw))
            out["vcf_%s_%s" % (label, name)] = dict(ms=t, text_bytes=n, variants=k, stats=s)
            print("vcf %s %s: %d variants, %.2f MB of text, %.1f ms (%.1f-%.1f); " % (label, name, k, n / 1e6, *t) +
                  "  ".join("%s %.3f" % (x[3:], s[x]) for x in STAGES) + "; windows %d records %d walked %d ins %d del %d" %
                  (s["windows"], s["records_read"], s["records_walked"], s["n_ins"], s["n_del"]), flush=True)
    if oracle:
        import bam_text
        import vcf_ref
        t0 = time.perf_counter()
        raw = bam_text.inflate(open(path, "rb").read())
        _, refs, at = bam_text.parse_header(raw)
        recs = []
        while at < len(raw):
            (bs,) = struct.unpack_from("<I", raw, at)
            recs.append(vcf_ref.parse_record(raw[at:at + 4 + bs], bam_text._tags))
            at += 4 + bs
        t1 = time.perf_counter()
        want = vcf_ref.call(recs, [n for n, _ in refs], [genome.cpu().numpy().tobytes()])[0]
        t2 = time.perf_counter()
        d = BamVcf(ctx, path, bai)
        got = b"".join(p[2] for p in d.fetch())
        d.close()
        out["oracle"] = dict(parse_ms=(t1 - t0) * 1e3, walk_ms=(t2 - t1) * 1e3, records=len(recs), ops=sum(len(r[4]) for r in recs), same=bool(got == want))
        print("host oracle: %d records, %d ops: inflate + parse %.0f ms, the walk %.0f ms; the device's text is %s" %
              (len(recs), out["oracle"]["ops"], out["oracle"]["parse_ms"], out["oracle"]["walk_ms"], "the same" if got == want else "DIFFERENT"), flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
