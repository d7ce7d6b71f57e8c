"""Time the two forms of the read-file input on a FASTQ or BAM of bench size (needs the GPU): lra_reads_next_batch (host parsing) against
lra_reads_next_batch_device (parsing on the device), in Mbases/s of whole batches, from the page cache.

    python tools/time_input.py [--format fastq|bam|fastq-bgzf|fastq-gz] [--level 6] [--n-reads 28672] [--read-len 30000] [--out profiles/device_input.json]
    python tools/time_input.py --format fastq-bgzf --inflate-kernel serial|lut      # the inflate stage alone over the file's member table
    python tools/time_input.py --resident 0,1,3 --device-only --warm-reader         # lra_reads_set_device_resident's modes side by side

--resident: the device form once per listed mode (0: as before; 1: LRA_READS_DEV_QUAL; 3: | LRA_READS_DEV_NO_HOST), each with the batch's device-to-host
bytes (the tool's own count of what the reader copies: names always, bases and qualities unless mode 3, one byte per read in mode 3) and the page-locked
bytes the reader holds for its batch arrays (what the batch's host arrays need, before the buffers' growth headroom).  --warm-reader times the SECOND
pass of one reader over the file list given twice (FASTA / FASTQ only: nothing is read behind a BAM file), so the first pass has sized every buffer:
the time per batch of a reader that maps many batches.

--format fastq-bgzf / fastq-gz: the FASTQ of --format fastq (random per-read qualities) as BGZF members of htslib's size, or as one gzip member, at zlib
level --level, opened with compressed_text.  --inflate-kernel times one of the two inflate kernels alone (bgzf_inflate: lra_bgzf_inflate_batch; bgzf_inflate_lut:
lra_bgzf_inflate_lut_batch) over the SAME member table, twice, and prints a CRC-32 of the output so that two runs can be compared byte for byte.

The BAM (--format bam) holds the same reads with random per-read qualities (a constant quality string compresses unrealistically well), in BGZF members of
htslib's size at zlib level --level; its device form is broken down into the file read, host-to-device copies, inflate, framing, record decoding and
device-to-host copies.

The file (28672 reads of 30 kb by default, ~1.7 GB: bases, '+', qualities) is written under a temporary directory and read once before timing so that
both forms read from the page cache.  The device form is broken down into the file read (a plain read of the file into one buffer, the same bytes the
reader reads), host-to-device copies, the parser's kernels and the device-to-host copies of each batch (device events: lra_ctx_timing)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from lra_amd import reads_io, synth
from lra_amd.context import Context


def write_fastq(path, n_reads, read_len, seed=1):
    """reads cut from a synthetic genome (lra_amd.synth), 1 in 8 of them lower case, Phred+33 qualities"""
    rng = np.random.default_rng(seed)
    genome = synth.make_genome(4_000_000, seed=seed, repeat_frac=0.2, n_families=3)
    g = genome.tobytes()
    qual = bytes(rng.integers(35, 74, read_len).astype(np.uint8))
    with open(path, "wb", buffering=1 << 24) as f:
        for i in range(n_reads):
            a = int(rng.integers(0, len(g) - read_len))
            s = g[a:a + read_len]
            f.write(b"@read%d pos=%d\n%s\n+\n%s\n" % (i, a, s.lower() if i % 8 == 0 else s, qual))


def write_bam(path, n_reads, read_len, level, seed=1):
    """the reads of write_fastq as an unaligned BAM: numpy packs the records, zlib compresses the members on 16 threads"""
    from concurrent.futures import ThreadPoolExecutor
    from lra_amd import bgzf
    rng = np.random.default_rng(seed)
    genome = synth.make_genome(4_000_000, seed=seed, repeat_frac=0.2, n_families=3)
    code = np.full(256, 15, np.uint8)
    for i, c in enumerate(bgzf.NT16):
        code[c] = i
    g = code[genome]
    parts = [bgzf.bam_bytes([])]
    for i in range(n_reads):
        a = int(rng.integers(0, len(g) - read_len))
        s = g[a:a + read_len]
        if read_len % 2:
            s = np.append(s, 0)
        packed = ((s[0::2] << 4) | s[1::2]).astype(np.uint8).tobytes()
        q = rng.integers(2, 41, read_len).astype(np.uint8).tobytes()
        name = b"read%d\0" % i
        body = np.array([-1, -1], "<i4").tobytes() + bytes([len(name), 255]) + np.array([4680, 0, 4], "<u2").tobytes() + \
            np.array([read_len, -1, -1, 0], "<i4").tobytes() + name + packed + q + b"RGZrun1\0"
        parts.append(np.array([len(body)], "<u4").tobytes() + body)
    raw = b"".join(parts)
    del parts
    cuts = range(0, len(raw), 65280)
    with ThreadPoolExecutor(16) as ex:
        members = list(ex.map(lambda a: bgzf.member(raw[a:a + 65280], level), cuts))
    with open(path, "wb") as f:
        f.write(b"".join(members) + bgzf.EOF_BLOCK)
    return len(raw)


def write_fastq_compressed(path, n_reads, read_len, level, bgzf_members, seed=1):
    """write_fastq's reads with random qualities, BGZF (members of 65280 bytes, compressed on 16 threads) or one gzip member"""
    from concurrent.futures import ThreadPoolExecutor
    from lra_amd import bgzf
    rng = np.random.default_rng(seed)
    g = synth.make_genome(4_000_000, seed=seed, repeat_frac=0.2, n_families=3).tobytes()
    parts = []
    for i in range(n_reads):
        a = int(rng.integers(0, len(g) - read_len))
        s = g[a:a + read_len]
        parts.append(b"@read%d pos=%d\n%s\n+\n%s\n" % (i, a, s.lower() if i % 8 == 0 else s, (33 + rng.integers(2, 41, read_len)).astype(np.uint8).tobytes()))
    raw = b"".join(parts)
    del parts
    if bgzf_members:
        with ThreadPoolExecutor(16) as ex:
            members = list(ex.map(lambda a: bgzf.member(raw[a:a + 65280], level), range(0, len(raw), 65280)))
        data = b"".join(members) + bgzf.EOF_BLOCK
    else:
        data = bgzf.gzip_compress(raw, level)
    with open(path, "wb") as f:
        f.write(data)
    return len(raw)


def time_inflate(ctx, path, kernel, repeats=2):
    """one inflate kernel alone over the BGZF file's member table: seconds per run (device events), GB/s of output, the output's CRC-32"""
    import ctypes as C
    import zlib
    import torch
    from lra_amd import bgzf
    data = open(path, "rb").read()
    in_off, out_off = bgzf.blocks(data)
    n = len(in_off) - 1
    dev = lambda a: torch.from_numpy(a.view(np.uint8)).cuda()
    t_in, t_io, t_oo = dev(np.frombuffer(data, np.uint8).copy()), dev(np.array(in_off, np.uint64)), dev(np.array(out_off, np.uint64))
    t_out, t_st = torch.zeros(out_off[-1] + 64, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    fn = ctx.lib.lra_bgzf_inflate_batch if kernel == "serial" else ctx.lib.lra_bgzf_inflate_lut_batch
    secs = []
    for _ in range(repeats + 1):                                # the first run warms the code object up
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc = fn(ctx.h, n, t_in.data_ptr(), t_io.data_ptr(), t_oo.data_ptr(), t_out.data_ptr(), t_st.data_ptr())
        secs.append(time.perf_counter() - t)
        assert rc == 0 and int(t_st.abs().sum()) == 0, "a member failed"
    crc = zlib.crc32(t_out[:out_off[-1]].cpu().numpy().tobytes()) & 0xffffffff
    return dict(kernel=kernel, members=n, out_bytes=out_off[-1], seconds=secs[1:], gb_per_s=[out_off[-1] / s / 1e9 for s in secs[1:]], crc32="%08x" % crc)


def run(files, max_bases, ctx=None, chunk=None, resident=0, warm=False):
    kw = dict(device_quals=bool(resident & 1), no_host_copy=bool(resident & 2)) if resident else {}      # (mode 0 runs on a library without the setter too)
    rf = reads_io.ReadsFile(files * 2 if warm else files, ctx=ctx, chunk=chunk, compressed_text=True, **kw)
    lib = rf.lib
    b = reads_io.ReadBatchC()
    import ctypes as C
    n_reads = n_bases = n_batches = 0
    d2h = pinned = 0
    if warm:                                                    # the first pass over the file sizes the reader's buffers
        tot = 0
        while tot < sum_bases(files):
            d_seq, d_off = C.c_void_p(), C.c_void_p()
            rc = lib.lra_reads_next_batch_device(rf.h, ctx.h, C.c_uint64(max_bases), C.byref(b), C.byref(d_seq), C.byref(d_off))
            assert rc == 0 and b.n_reads, rc
            tot += int(b.total_bases)
    t = time.perf_counter()
    while True:
        if ctx is None:
            rc = lib.lra_reads_next_batch(rf.h, C.c_uint64(max_bases), C.byref(b))
        else:
            d_seq, d_off = C.c_void_p(), C.c_void_p()
            rc = lib.lra_reads_next_batch_device(rf.h, ctx.h, C.c_uint64(max_bases), C.byref(b), C.byref(d_seq), C.byref(d_off))
        assert rc == 0, rc
        if b.n_reads == 0:
            break
        n_reads += b.n_reads; n_bases += int(b.total_bases); n_batches += 1
        if ctx is not None:                                     # what this batch brought to the host, and the page-locked bytes under its host arrays
            t_acc = time.perf_counter()                         # (this bookkeeping is taken out of the time)
            qp = C.cast(b.quals, C.POINTER(C.c_void_p))
            names = sum(len(b.names[i]) + 1 for i in range(b.n_reads))
            quals = sum(b.read_len[i] + 1 if qp[i] else 1 for i in range(b.n_reads))
            nb = names + (b.n_reads if resident & 2 else int(b.total_bases) + 64 + quals)
            d2h += nb; pinned = max(pinned, nb)
            t += time.perf_counter() - t_acc
    dt = time.perf_counter() - t
    rf.close()
    out = dict(seconds=dt, reads=n_reads, bases=n_bases, batches=n_batches, mbases_per_s=n_bases / dt / 1e6, ms_per_batch=dt * 1e3 / max(n_batches, 1))
    if ctx is not None:
        out.update(resident=resident, warm_reader=warm, d2h_bytes_per_batch=d2h // max(n_batches, 1), pinned_batch_bytes=pinned)
    return out


_BASES = {}


def sum_bases(files):
    return sum(_BASES[f] for f in files)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", choices=["fastq", "bam", "fastq-bgzf", "fastq-gz"], default="fastq")
    ap.add_argument("--level", type=int, default=6, help="zlib level of the compressed formats")
    ap.add_argument("--inflate-kernel", choices=["serial", "lut"], default=None, help="time this inflate kernel alone over the BGZF file's members")
    ap.add_argument("--n-reads", type=int, default=28672)
    ap.add_argument("--read-len", type=int, default=30000)
    ap.add_argument("--max-bases", type=int, default=0, help="bases per batch (0: the whole bench batch, n-reads x read-len)")
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--device-only", action="store_true", help="skip the host form (for a profiler run)")
    ap.add_argument("--resident", default="0", help="comma-separated lra_reads_set_device_resident modes to time (0, 1, 3)")
    ap.add_argument("--warm-reader", action="store_true", help="time the second pass of one reader over the file (its buffers sized by the first)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    max_bases = args.max_bases or args.n_reads * args.read_len
    ctx = Context(0)
    with tempfile.TemporaryDirectory() as tmp:
        fq = os.path.join(tmp, {"fastq": "reads.fq", "bam": "reads.bam", "fastq-bgzf": "reads.fq.bgz", "fastq-gz": "reads.fq.gz"}[args.format])
        t = time.perf_counter()
        raw = None
        if args.format == "fastq":
            write_fastq(fq, args.n_reads, args.read_len)
        elif args.format == "bam":
            raw = write_bam(fq, args.n_reads, args.read_len, args.level)
        else:
            raw = write_fastq_compressed(fq, args.n_reads, args.read_len, args.level, args.format == "fastq-bgzf")
        size = os.path.getsize(fq)
        _BASES[fq] = args.n_reads * args.read_len
        sys.stderr.write("wrote %s: %.2f GB in %.1f s\n" % (fq, size / 1e9, time.perf_counter() - t))
        buf = bytearray(size)
        reads = []
        for _ in range(args.repeats + 1):                      # the first pass fills the page cache
            t = time.perf_counter()
            with open(fq, "rb", buffering=0) as f:
                got = f.readinto(buf)
            reads.append(time.perf_counter() - t)
            assert got == size
        del buf
        if args.inflate_kernel:
            res = dict(format=args.format, level=args.level, file_bytes=size, inflate=time_inflate(ctx, fq, args.inflate_kernel, args.repeats))
            print(json.dumps(res))
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(res, f, indent=1)
            ctx.close()
            return
        res = dict(format=args.format, level=args.level if raw else None, decompressed_bytes=raw, file_bytes=size, n_reads=args.n_reads, read_len=args.read_len, max_bases=max_bases, chunk=args.chunk,
                   file_read_s=min(reads[1:]), file_read_gb_per_s=size / min(reads[1:]) / 1e9)
        if not args.device_only:
            res["host"] = min((run([fq], max_bases) for _ in range(args.repeats)), key=lambda r: r["seconds"])
        modes = [int(m) for m in args.resident.split(",")]
        res["device_resident"] = {}
        for mode in modes[1:] if modes[0] == 0 else modes:      # the new modes; mode 0 is the "device" entry below
            runs = []
            for _ in range(args.repeats):
                ctx.timing(True); ctx.timing_reset()
                r = run([fq], max_bases, ctx=ctx, chunk=args.chunk, resident=mode, warm=args.warm_reader)
                r["breakdown_ms"] = {k: ctx.timing_get(k)[0] for k in ("input_h2d", "input_parse", "input_decode", "input_d2h", "input_pack_quals")}
                ctx.timing(False)
                runs.append(r)
            best_m = min(runs, key=lambda r: r["seconds"])
            best_m["all_seconds"] = [r["seconds"] for r in runs]
            res["device_resident"][str(mode)] = best_m
        best = None
        all_s = []
        for _ in range(args.repeats):
            ctx.timing(True); ctx.timing_reset()
            r = run([fq], max_bases, ctx=ctx, chunk=args.chunk, warm=args.warm_reader)
            all_s.append(r["seconds"])
            keys = {"fastq": ("input_h2d", "input_parse", "input_d2h"), "bam": ("input_h2d", "input_inflate", "input_frame", "input_decode", "input_d2h"),
                    "fastq-bgzf": ("input_h2d", "input_inflate", "input_parse", "input_d2h"), "fastq-gz": ("input_h2d", "input_parse", "input_d2h")}[args.format]
            r["breakdown_ms"] = {k: ctx.timing_get(k)[0] for k in keys}
            ctx.timing(False)
            if best is None or r["seconds"] < best["seconds"]:
                best = r
        res["device"] = best
        res["device"]["all_seconds"] = all_s
        bd = best["breakdown_ms"]
        res["device"]["breakdown_ms"]["file_read"] = res["file_read_s"] * 1e3
        res["device"]["breakdown_ms"]["other_host"] = best["seconds"] * 1e3 - res["file_read_s"] * 1e3 - sum(v for k, v in bd.items() if k != "file_read")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
