"""What BGZF output costs the device record stage on one bench-like batch (needs the GPU):

    python tools/time_bgzf_output.py [n_reads=2048] [read_len=30000] [repeats=5] [kernel-only]

  plain   lra_map_records_device (format s, the qualities on the device): wall ms per batch, device-to-host bytes;
  bgzf    lra_map_records_device_bgzf on the same result: wall ms, the compress stage's share (lra_bgzf_compress_stats), device-to-host bytes, and
          the bgzf_deflate kernel's HIP-event time and input GB/s from the context's kernel timing (one more call);
  sizes   the members' bytes against zlib levels 1 and 6 on the same 65280-byte cuts (lra_amd.bgzf), over the first 64 MB of the text;
  host    Python zlib level 1 over the same cuts of the whole text on 16 threads (zlib releases the GIL): the host alternative's wall ms.
A library without lra_map_records_device_bgzf (the parent commit) runs the plain form only.  kernel-only: one bgzf call and nothing else, for a
profiler run of its own (rocprofv3 --kernel-trace --stats).  Median and range over the repeats after one warm-up call; one JSON line at the end."""
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lra_amd import bgzf, mapread, seed, synth_torch as st
from lra_amd.context import Context


def med(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    rlen = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    kernel_only = len(sys.argv) > 4 and sys.argv[4] == "kernel-only"
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    has_bgzf = hasattr(ctx.lib, "lra_map_records_device_bgzf") and hasattr(mapread.LowAccMapper, "records_device_bgzf")
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
    out = dict(n_reads=n, bases=int(off[-1]), repeats=reps, has_bgzf=has_bgzf)
    if kernel_only:
        r = mapper.records_device_bgzf(res, args, **kw)
        print(json.dumps(dict(out, bgzf_bytes=len(r[0]))))
        ctx.close()
        return

    def timed(fn):
        fn()
        wall = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
        return med(wall)

    got = {}
    def plain():
        got["plain"] = mapper.records_device(res, args, as_list=False, **kw)
        got["plain_stats"] = mapper.records_device_stats()
    out["plain_wall_ms"] = timed(plain)
    out["text_bytes"] = got["plain"]; out["plain_d2h_bytes"] = got["plain_stats"]["bytes_d2h"]
    print("plain: wall %.1f ms (%.1f-%.1f)  text %.1f MB  d2h %.1f MB" % (*out["plain_wall_ms"], got["plain"] / 1e6, out["plain_d2h_bytes"] / 1e6), flush=True)
    if has_bgzf:
        from lra_amd import deflate
        ms = []
        def zf():
            got["bgzf"] = mapper.records_device_bgzf(res, args, **kw)
            got["bgzf_stats"] = mapper.records_device_stats()
            ms.append(deflate.compress_stats(ctx)[0])
        out["bgzf_wall_ms"] = timed(zf)
        out["bgzf_compress_stage_ms"] = med(ms[1:])
        data = got["bgzf"][0]
        out["bgzf_bytes"] = len(data); out["bgzf_d2h_bytes"] = got["bgzf_stats"]["bytes_d2h"]
        ctx.timing(True); ctx.timing_reset()
        mapper.records_device_bgzf(res, args, **kw)
        k_ms = ctx.timing_get("bgzf_deflate")[0]; p_ms = ctx.timing_get("bgzf_pack")[0]
        ctx.timing(False)
        out["bgzf_deflate_kernel_ms"] = k_ms; out["bgzf_pack_kernel_ms"] = p_ms; out["bgzf_deflate_input_GBps"] = got["plain"] / max(k_ms, 1e-6) / 1e6
        print("bgzf:  wall %.1f ms (%.1f-%.1f)  compress stage %.1f ms  deflate kernel %.2f ms = %.1f GB/s of input  pack %.2f ms  members %.1f MB  d2h %.1f MB"
              % (*out["bgzf_wall_ms"], out["bgzf_compress_stage_ms"][0], k_ms, out["bgzf_deflate_input_GBps"], p_ms, len(data) / 1e6, out["bgzf_d2h_bytes"] / 1e6), flush=True)
        import gzip
        text = gzip.decompress(data + bgzf.EOF_BLOCK)
        assert len(text) == got["plain"]
        moff = got["bgzf"][2]
        nm = min(len(moff) - 1, (64 << 20) // 65280)
        part = text[:nm * 65280]
        z1, z6 = len(bgzf.bgzf_compress(part, 1, eof=False)), len(bgzf.bgzf_compress(part, 6, eof=False))
        out.update(sample_text_bytes=len(part), sample_ours=int(moff[nm]), sample_zlib1=z1, sample_zlib6=z6)
        print("sizes over the first %.1f MB: ours %d  zlib level 1 %d  level 6 %d  (ours / level 1 %.3f, ours / level 6 %.3f)"
              % (len(part) / 1e6, int(moff[nm]), z1, z6, int(moff[nm]) / z1, int(moff[nm]) / z6), flush=True)
        cuts = [text[a:a + 65280] for a in range(0, len(text), 65280)]
        def one(d):
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            return len(c.compress(d) + c.flush())
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(one, cuts[:64]))
            wall = []
            for _ in range(max(reps, 3)):
                t0 = time.perf_counter()
                total = sum(ex.map(one, cuts, chunksize=16))
                wall.append((time.perf_counter() - t0) * 1e3)
        out["host_zlib1_16_threads_ms"] = med(wall)
        print("host zlib level 1, 16 threads: %.1f ms (%.1f-%.1f) = %.2f GB/s" % (*out["host_zlib1_16_threads_ms"], len(text) / out["host_zlib1_16_threads_ms"][0] / 1e6), flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
