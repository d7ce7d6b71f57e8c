"""Time the two forms of the read-file input on a FASTQ or BAM of bench size (needs the GPU): lra_reads_next_batch (host parsing) against
lra_reads_next_batch_device (parsing on the device), in Mbases/s of whole batches, from the page cache.

    python tools/time_input.py [--format fastq|bam] [--level 6] [--n-reads 28672] [--read-len 30000] [--out profiles/device_input.json]

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


def run(files, max_bases, ctx=None, chunk=None):
    rf = reads_io.ReadsFile(files, ctx=ctx, chunk=chunk)
    lib = rf.lib
    b = reads_io.ReadBatchC()
    import ctypes as C
    n_reads = n_bases = n_batches = 0
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
    dt = time.perf_counter() - t
    rf.close()
    return dict(seconds=dt, reads=n_reads, bases=n_bases, batches=n_batches, mbases_per_s=n_bases / dt / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", choices=["fastq", "bam"], default="fastq")
    ap.add_argument("--level", type=int, default=6, help="zlib level of the BAM's members")
    ap.add_argument("--n-reads", type=int, default=28672)
    ap.add_argument("--read-len", type=int, default=30000)
    ap.add_argument("--max-bases", type=int, default=0, help="bases per batch (0: the whole bench batch, n-reads x read-len)")
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--device-only", action="store_true", help="skip the host form (for a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    max_bases = args.max_bases or args.n_reads * args.read_len
    ctx = Context(0)
    with tempfile.TemporaryDirectory() as tmp:
        fq = os.path.join(tmp, "reads.fq" if args.format == "fastq" else "reads.bam")
        t = time.perf_counter()
        raw = None
        if args.format == "fastq":
            write_fastq(fq, args.n_reads, args.read_len)
        else:
            raw = write_bam(fq, args.n_reads, args.read_len, args.level)
        size = os.path.getsize(fq)
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
        res = dict(format=args.format, level=args.level if raw else None, decompressed_bytes=raw, file_bytes=size, n_reads=args.n_reads, read_len=args.read_len, max_bases=max_bases, chunk=args.chunk,
                   file_read_s=min(reads[1:]), file_read_gb_per_s=size / min(reads[1:]) / 1e9)
        if not args.device_only:
            res["host"] = min((run([fq], max_bases) for _ in range(args.repeats)), key=lambda r: r["seconds"])
        best = None
        for _ in range(args.repeats):
            ctx.timing(True); ctx.timing_reset()
            r = run([fq], max_bases, ctx=ctx, chunk=args.chunk)
            keys = ("input_h2d", "input_parse", "input_d2h") if raw is None else ("input_h2d", "input_inflate", "input_frame", "input_decode", "input_d2h")
            r["breakdown_ms"] = {k: ctx.timing_get(k)[0] for k in keys}
            ctx.timing(False)
            if best is None or r["seconds"] < best["seconds"]:
                best = r
        res["device"] = best
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
