"""Time the two forms of the record stage on one bench-like batch (needs the GPU):

    python tools/time_records_device.py [n_reads=28672] [read_len=30000] [preset=ont|contig] [repeats=5] [format=s|P|a]

  host    lra_map_snapshot + lra_map_records_host at 4 and 12 threads (the CIGAR runs copied to the host, the text written by host threads);
  device  lra_map_records_device (a snapshot without the runs, the piece table on host threads, the long fields and the assembly on the device),
          split as lra_map_records_device_last reports it, with the qualities uploaded from the host, with the qualities already on the device, and
          (format s / P) with the batch read back through a device reader with LRA_READS_DEV_QUAL | LRA_READS_DEV_NO_HOST from a FASTQ of the same reads
          and qualities: records_device on the READER's d_qual / d_qual_off, stub quals and no host reads ("device_quals_from_reader").
Per form: wall ms and host CPU-seconds per batch (time.process_time: every thread of the process), median and range over the repeats after one
warm-up call; device-to-host bytes; the copy pass's GB/s (bytes read + bytes written over its HIP-event time).  One JSON line at the end.
format a (pairwise): the host form is the snapshot with every block and one copy per alignment of the bases under it; the device form builds the rows with
lra_pairwise_text_batch, whose kernels' times (one more call under the context's kernel timing) and whose emit kernel's written bytes per second are added;
the qualities play no part, so the device form is timed once."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lra_amd import mapread, seed, synth_torch as st
from lra_amd.context import Context


def med(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def pairwise_kernels(ctx, mapper, res, args, text_bytes):
    """One more device call under the context's kernel timing: the pairwise stage's kernels (count + scans, emit) and the assembly's, and the emit kernel's
    written bytes per second (the rows' text: the record text less the name and Interval lines, a few dozen bytes per alignment) against the 8 TB/s peak."""
    ctx.timing(True)
    ctx.timing_reset()
    mapper.records_device(res, args, as_list=False)
    ms = {k: ctx.timing_get(k)[0] for k in ("pairwise_count", "pairwise_emit", "records_resolve", "records_copy")}
    ctx.timing(False)
    rows = text_bytes - 60 * int(res.n_alignments)
    gbps = rows / max(ms["pairwise_emit"], 1e-6) / 1e6
    out = dict(ms=ms, emit_written_GBps=gbps, emit_fraction_of_8TBps=gbps / 8000)
    print("pairwise kernels (ms): %s; pw_emit writes %.0f GB/s = %.1f %% of 8 TB/s" % (ms, gbps, 100 * gbps / 8000), flush=True)
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 28672
    rlen = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
    preset = sys.argv[3] if len(sys.argv) > 3 else "ont"
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    fmt = sys.argv[5] if len(sys.argv) > 5 else "s"
    assert fmt in ("s", "P", "a"), fmt
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    genome = st.make_genome(16_000_000, 1, dev)
    err = 0.10 if preset == "ont" else 0.003
    sim = st.simulate_batch(genome, n, rlen, rlen // 10, err, (30, 35, 35), 5)
    reads = torch.cat([sim["seq"], torch.zeros(64, dtype=torch.uint8, device=dev)])
    if preset == "ont":
        ik, ip = st.build_global_index(genome, 17, 10, 150)
        mapper = mapread.LowAccMapper(ctx, genome, ik, ip, [b"chr1"], [0, int(genome.numel())])
    else:
        mapper = mapread.HighAccMapper(ctx, genome, None, None, [b"chr1"], [0, int(genome.numel())], preset="contig", index_params=(19, 10, 30, 20, 1))
    d_off = sim["off"]
    rb = seed.read_batch_from_device(ctx, reads, d_off)
    off = d_off.cpu().numpy(); h = reads.cpu().numpy()
    rl = [h[off[i]:off[i + 1]].tobytes() for i in range(n)]
    rng = np.random.default_rng(1)
    ql = [bytes(rng.integers(43, 74, len(r)).astype(np.uint8)) for r in rl]
    names = [b"read%d" % i for i in range(n)]
    args = mapper.record_args(names, rl, ql)
    qoff = torch.from_numpy(np.concatenate([[0], np.cumsum([len(q) for q in ql])]).astype(np.int64)).to(dev)
    dq = torch.from_numpy(np.frombuffer(b"".join(ql), np.uint8).copy()).to(dev)
    del sim
    torch.cuda.empty_cache()                                                # (the simulation's temporaries: the library allocates beside torch's cache)
    res = mapper.align(rb)
    mapper.copts.printFormat = ord(fmt)
    out = dict(format=fmt, n_reads=n, bases=int(off[-1]), preset=preset, n_runs=int(res.n_runs), n_alignments=int(res.n_alignments), repeats=reps)

    def timed(fn):
        fn()                                                                # warm-up: buffers sized, pages touched
        wall, cpu = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            c0, t0 = time.process_time(), time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3); cpu.append(time.process_time() - c0)
        return dict(wall_ms=med(wall), cpu_s=med(cpu))

    for T in (4, 12):
        nb = []
        def host():
            snap = mapper.snapshot(res, with_blocks=fmt == "a")
            nb.append(mapper.records_host(snap, args, n_threads=T, as_list=False))
        r = timed(host)
        r["text_bytes"] = nb[-1]; r["d2h_bytes"] = int(res.n_runs) * 4 + int(res.n_alignments) * 140      # the pack: the runs + the per-alignment arrays
        if fmt == "a":                                                      # + every block, and the chromosome bases under every alignment (one copy each)
            fo = mapper.fetch(res)
            r["d2h_bytes"] += int(res.n_blocks) * 12 + int(sum(int(c[17]) - int(c[16]) for c in fo["counts"]))
            r["d2h_copies_per_alignment"] = 1
        out["host_%d" % T] = r
        print("host  %2d threads: wall %.1f ms (%.1f-%.1f)  cpu %.3f s (%.3f-%.3f)  text %.3f GB" % (T, *r["wall_ms"], *r["cpu_s"], nb[-1] / 1e9), flush=True)
    forms = (("device_quals_from_host", {}), ("device_quals_on_device", dict(d_qual=dq, d_qual_off=qoff))) if fmt != "a" else (("device", {}),)
    rf = tmp = None
    if fmt != "a":                                                          # the same reads and qualities through a device reader that keeps them on the device
        import tempfile
        from lra_amd import reads_io
        tmp = tempfile.TemporaryDirectory()
        fq = os.path.join(tmp.name, "reads.fq")
        with open(fq, "wb", buffering=1 << 24) as f:
            for i in range(n):
                f.write(b"@%s\n%s\n+\n%s\n" % (names[i], rl[i], ql[i]))
        rf = reads_io.ReadsFile([fq], ctx=ctx, device_quals=True, no_host_copy=True)
        b = rf.next_batch(int(off[-1]))
        assert b["n"] == n and b["seqs"] is None and b["names"] == names
        stub = mapper.record_args(names, None, b["quals"], lens=b["read_len"])
        forms += (("device_quals_from_reader", dict(d_qual=b["d_qual"], d_qual_off=b["d_qual_off"], _args=stub)),)
    texts = {}
    for label, kw in forms:
        kw = dict(kw)
        a = kw.pop("_args", args)
        for T in (4, 12):
            parts = []
            got = []
            def devf():
                got.append(mapper.records_device(res, a, n_threads=T, as_list=False, **kw))
                parts.append(mapper.records_device_stats())
            r = timed(devf)
            last = parts[-1]
            for k in last:
                if k.startswith("ms_"):
                    r[k] = med([p[k] for p in parts[1:]])
            r.update(returned_bytes=got[-1], fell_through=last["text_bytes"] == 0 and got[-1] > 0, text_bytes=last["text_bytes"], d2h_bytes=last["bytes_d2h"], h2d_bytes=last["bytes_h2d"], n_pieces=last["n_pieces"])
            ck = r["ms_copy_kernel"][0]
            r["copy_GBps"] = 2 * last["text_bytes"] / max(ck, 1e-6) / 1e6
            out["%s_%d" % (label, T)] = r
            texts[label] = got[-1]
            print("%s %2d threads: wall %.1f ms (%.1f-%.1f)  cpu %.3f s (%.3f-%.3f)  snapshot %.1f  cigar+md %.1f  pieces %.1f  upload %.1f  kernels %.1f (copy %.2f = %.0f GB/s)  "
                  "text copy %.1f ms  d2h %.3f GB  h2d %.3f GB" % (label, T, *r["wall_ms"], *r["cpu_s"], r["ms_snapshot"][0], r["ms_cigar_md"][0], r["ms_pieces"][0], r["ms_upload"][0],
                                                                   r["ms_kernels"][0], ck, r["copy_GBps"], r["ms_text_copy"][0], last["bytes_d2h"] / 1e9, last["bytes_h2d"] / 1e9), flush=True)
    if rf is not None:
        assert texts["device_quals_from_reader"] == texts["device_quals_from_host"], texts   # the same number of bytes (the tests compare the bytes)
        rf.close(); tmp.cleanup()
    if fmt == "a" and not out["device_4"]["fell_through"]:
        out["pairwise_kernels"] = pairwise_kernels(ctx, mapper, res, args, out["device_4"]["text_bytes"])
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
