"""The device assembly-SV pass on a coordinate-sorted BAM with its .bai, beside lra_bam_vcf's pass of the same file and the host oracle (needs the GPU):

    python tools/time_bam_svcalls.py sorted.bam [repeats=3] [oracle=1] [genome_seed=1] [min_size=40]

`tools/time_bam_view.py ... keep=sorted.bam` writes the bench-size file; its genome is synth_torch.make_genome(<the reference's length>, genome_seed),
made again here and loaded into the context.  Each pass `repeats` times after one warm-up, wall time from create to the last piece through the Python
wrapper, median and range: lra_bam_svcalls over the whole file (min_size as given, drop_contained 1, an empty mask) with text and with values only, the
same with drop_contained 0, and lra_bam_vcf with values only at min_length = min_size, with and without drop_contained; each pass's own split
(lra_bam_svcalls_stats, lra_bam_vcf_stats) and the merge's rounds.  oracle: tests/svcalls_ref.py over the same records (parsed on the host from the
inflated file), once, and its tables compared with the device's.  One JSON line at the end."""
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
from lra_amd.bam import BamSvCalls, BamVcf, BamView
from lra_amd.context import Context
from lra_amd.index import load_genome

SV_STAGES = ("ms_read_inflate", "ms_frame_select", "ms_ops", "ms_walk", "ms_lengths", "ms_rows", "ms_merge", "ms_emit", "ms_copy")
VCF_STAGES = ("ms_read_inflate", "ms_frame_select", "ms_ops", "ms_walk", "ms_lengths", "ms_emit", "ms_copy")


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
    min_size = int(sys.argv[5]) if len(sys.argv) > 5 else 40
    bai = path + ".bai"
    ctx = Context(0)
    out = dict(file_bytes=os.path.getsize(path), repeats=reps, min_size=min_size)
    v0 = BamView(ctx, path, bai)
    _, names, lens = v0.header()
    v0.close()
    assert len(lens) == 1, "the bench-size file has one reference"
    genome = st.make_genome(int(lens[0]), seed, torch.device("cuda", 0))
    load_genome(ctx, genome)
    ctx.check(ctx.lib.lra_ctx_load_chromosomes(ctx.h, (C.c_uint64 * 2)(0, int(lens[0])), 1))

    def svcalls(**kw):
        d = BamSvCalls(ctx, path, bai, min_size=min_size, **kw)
        n = k = 0
        for _, _, count, _, text in d.fetch():
            n += len(text); k += count
        s = d.stats()
        d.close()
        return n, k, s

    def vcf(**kw):
        d = BamVcf(ctx, path, bai, text=False, values=True, min_length=min_size, **kw)
        k = sum(p[0] for p in d.fetch())
        s = d.stats()
        d.close()
        return k, s

    for label, kw in (("text", dict()), ("values", dict(text=False, values=True)), ("text_all_records", dict(drop_contained=False))):
        t, (n, k, s) = timed(reps, lambda: svcalls(**kw))
        out["svcalls_" + label] = dict(ms=t, text_bytes=n, rows=k, stats=s)
        print("svcalls %s: %d rows, %.3f MB of text, %.1f ms (%.1f-%.1f); " % (label, k, n / 1e6, *t) + "  ".join("%s %.3f" % (x[3:], s[x]) for x in SV_STAGES) +
              "; windows %d records %d contained %d walked %d; small %d/%d masked %d/%d merged %d/%d kept %d/%d (INS/DEL); rounds %d" %
              (s["windows"], s["records_read"], s["records_contained"], s["records_walked"], s["small_ins"], s["small_del"], s["masked_ins"], s["masked_del"],
               s["merged_ins"], s["merged_del"], s["kept_ins"], s["kept_del"], s["merge_rounds"]), flush=True)
    for label, kw in (("values", dict()), ("values_drop_contained", dict(drop_contained=True))):
        t, (k, s) = timed(reps, lambda: vcf(**kw))
        out["vcf_" + label] = dict(ms=t, variants=k, stats=s)
        print("vcf %s, min_length %d: %d variants, %.1f ms (%.1f-%.1f); " % (label, min_size, k, *t) + "  ".join("%s %.3f" % (x[3:], s[x]) for x in VCF_STAGES) +
              "; windows %d records %d contained %d walked %d" % (s["windows"], s["records_read"], s["records_contained"], s["records_walked"]), flush=True)
    if oracle:
        import bam_text
        import svcalls_ref
        import vcf_ref
        t0 = time.perf_counter()
        raw = bam_text.inflate(open(path, "rb").read())
        _, refs, at = bam_text.parse_header(raw)
        recs, cores = [], []
        while at < len(raw):
            (bs,) = struct.unpack_from("<I", raw, at)
            recs.append(vcf_ref.parse_record(raw[at:at + 4 + bs], bam_text._tags))
            cores.append(svcalls_ref.core_of(raw[at:at + 4 + bs]))
            at += 4 + bs
        t1 = time.perf_counter()
        want = svcalls_ref.calls(recs, cores, [n for n, _ in refs], [genome.cpu().numpy().tobytes()], min_size=min_size)
        t2 = time.perf_counter()
        d = BamSvCalls(ctx, path, bai, min_size=min_size)
        got = {"DEL": b"", "INS": b""}
        for _, kind, _, _, text in d.fetch():
            got[kind] += text
        d.close()
        same = got["DEL"] == want["DEL"][0] and got["INS"] == want["INS"][0]
        out["oracle"] = dict(parse_ms=(t1 - t0) * 1e3, calls_ms=(t2 - t1) * 1e3, records=len(recs), stats=want["stats"], same=bool(same))
        print("host oracle: %d records: inflate + parse %.0f ms, the calls %.0f ms; %s; the device's tables are %s" %
              (len(recs), out["oracle"]["parse_ms"], out["oracle"]["calls_ms"], want["stats"], "the same" if same else "DIFFERENT"), flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
