"""BAM output against BGZF-compressed SAM output of the device record stage, on one bench-like batch (needs the GPU):

    python tools/time_bam_output.py [n_reads=2048] [read_len=30000] [alternations=4]

Both forms run on the same lra_map_result in one session, alternating sam, bam, sam, bam, ... after one warm-up call of each:
  sam   lra_map_records_device_bgzf, format s -- the parent's compressed output;
  bam   lra_map_records_device_bam with bgzf = 1.
Per form: the stream's bytes (the deflate kernel's input), the members' bytes (what crosses to the host), the compress stage's wall time
(lra_bgzf_compress_stats), the call's wall time and the process's CPU seconds over the call (user + system, every host thread); for bam also the three
encode kernels' HIP-event times from the context's kernel timing (one more call).  Median and range over the alternations, the ratio bam / sam of every
figure pair by pair (median and range), and one JSON line at the end."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lra_amd import deflate, mapread, seed, synth_torch as st
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
    forms = dict(sam=lambda: mapper.records_device_bgzf(res, args, **kw), bam=lambda: mapper.records_device_bam(res, args, bgzf=True, **kw))
    keys = ("stream_bytes", "member_bytes", "d2h_bytes", "ms_deflate", "wall_ms", "cpu_s")
    runs = {f: {k: [] for k in keys} for f in forms}

    def one(f):
        torch.cuda.synchronize()
        c0 = os.times(); t0 = time.perf_counter()
        r = forms[f]()
        wall = (time.perf_counter() - t0) * 1e3
        c1 = os.times()
        s = mapper.records_device_stats()
        return dict(stream_bytes=int(s["text_bytes"]), member_bytes=len(r[0]), d2h_bytes=int(s["bytes_d2h"]), ms_deflate=deflate.compress_stats(ctx)[0], wall_ms=wall,
                    cpu_s=(c1.user - c0.user) + (c1.system - c0.system))

    for f in forms:
        one(f)                                                                  # warm-up: the kept buffers reach their sizes
    for _ in range(reps):
        for f in ("sam", "bam"):
            m = one(f)
            for k in keys:
                runs[f][k].append(m[k])
    out = dict(n_reads=n, bases=int(off[-1]), alternations=reps)
    for f in forms:
        out[f] = {k: med(runs[f][k]) for k in keys}
    out["bam_over_sam"] = {k: med([b / max(a, 1e-12) for a, b in zip(runs["sam"][k], runs["bam"][k])]) for k in keys}
    ctx.timing(True); ctx.timing_reset()
    forms["bam"]()
    out["bam_kernels_ms"] = {k: ctx.timing_get(k)[0] for k in ("bam_cigar", "bam_pack_seq", "bam_phred", "records_copy", "bgzf_deflate")}
    ctx.timing_reset()
    forms["sam"]()
    out["sam_kernels_ms"] = {k: ctx.timing_get(k)[0] for k in ("cigar_text", "records_copy", "bgzf_deflate")}
    ctx.timing(False)
    for f in forms:
        print("%s: stream %.1f MB  members %.1f MB  d2h %.1f MB  compress stage %.1f ms (%.1f-%.1f)  wall %.1f ms (%.1f-%.1f)  cpu %.3f s (%.3f-%.3f)"
              % (f, out[f]["stream_bytes"][0] / 1e6, out[f]["member_bytes"][0] / 1e6, out[f]["d2h_bytes"][0] / 1e6, *out[f]["ms_deflate"], *out[f]["wall_ms"], *out[f]["cpu_s"]), flush=True)
    print("bam / sam: " + "  ".join("%s %.3f (%.3f-%.3f)" % (k, *out["bam_over_sam"][k]) for k in keys), flush=True)
    print("bam kernels (ms): %s;  sam kernels (ms): %s" % (out["bam_kernels_ms"], out["sam_kernels_ms"]), flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
