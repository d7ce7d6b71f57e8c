"""Time the genome input from open to install on a synthetic genome of GRCh38's shape (needs the GPU): the device form (lra_genome_read_device), the
host form (lra_genome_read_host) and the Python yardstick (read_genome() of tools/map_files.py + lra_ctx_load_genome) on the plain file; both forms on
its gzip -6 and BGZF copies.

    python tools/time_genome.py [--bases 3100000000] [--gzip-bases N] [--records 300] [--out profiles/genome_input.json]

The genome is cut from a 16 Mb synthetic sequence (lra_amd.synth) at random offsets -- DEFLATE sees 32 KiB, so the copies compress like fresh sequence --
in 60-base lines.  --gzip-bases times the serial gzip decoder on a shorter prefix-sized genome of its own (0: skip it).  Files are written under a
temporary directory and read once before timing, so every form reads from the page cache.  The device form is broken down by device events
(lra_ctx_timing): host-to-device copies, BGZF inflate, the parser's kernels; the rest is host time (file read, page-locked allocation, gzip inflate)."""
import argparse
import ctypes as C
import gzip
import importlib.util
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from lra_amd import bgzf, index, synth
from lra_amd.context import Context


def write_genome(path, bases, records, seed=1):
    rng = np.random.default_rng(seed)
    src = synth.make_genome(16_000_000, seed=seed, repeat_frac=0.2, n_families=3)
    share = rng.dirichlet(np.full(records, 0.6)) * bases
    with open(path, "wb", buffering=1 << 24) as f:
        for i, n in enumerate(share):
            n = max(60, int(n))
            f.write(b">chr%d  synthetic record %d\n" % (i + 1, i))
            left = n
            while left > 0:
                m = min(left, 6_000_000)
                a = int(rng.integers(0, len(src) - m))
                s = src[a:a + m]
                if i % 7 == 3:
                    s = s | 0x20                                     # a soft-masked record
                rows = m // 60
                block = np.empty((rows, 61), np.uint8)
                block[:, :60] = s[:rows * 60].reshape(rows, 60); block[:, 60] = 10
                f.write(block.tobytes())
                if m % 60:
                    f.write(s[rows * 60:].tobytes() + b"\n")
                left -= m


def write_bgzf(src, dst, level=6):
    from concurrent.futures import ThreadPoolExecutor
    with open(src, "rb") as f, open(dst, "wb") as out, ThreadPoolExecutor(16) as ex:
        while True:
            raw = f.read(65280 * 4096)
            if not raw:
                break
            out.write(b"".join(ex.map(lambda a: bgzf.member(raw[a:a + 65280], level), range(0, len(raw), 65280))))
        out.write(bgzf.EOF_BLOCK)


def write_gzip(src, dst, level=6):
    with open(src, "rb") as f, gzip.open(dst, "wb", compresslevel=level) as out:
        while True:
            raw = f.read(1 << 26)
            if not raw:
                break
            out.write(raw)


def warm(path):
    with open(path, "rb", buffering=0) as f:
        while f.read(1 << 28):
            pass


def time_form(lib, ctx, path, device):
    g = C.c_void_p()
    if device:
        ctx.timing(True); ctx.timing_reset()
    t = time.perf_counter()
    assert lib.lra_genome_open(path.encode(), C.byref(g)) == 0
    rc = lib.lra_genome_read_device(g, ctx.h) if device else lib.lra_genome_read_host(g)
    assert rc == 0, lib.lra_genome_last_error(g)
    t_read = time.perf_counter() - t
    ctx.check(lib.lra_genome_install(g, ctx.h))
    dt = time.perf_counter() - t
    n, nl, total = C.c_int32(0), C.c_uint64(0), C.c_uint64(0)
    lib.lra_genome_info(g, C.byref(n), C.byref(nl), C.byref(total))
    lib.lra_genome_close(g)
    r = dict(seconds=dt, read_seconds=t_read, records=n.value, bases=total.value, gbases_per_s=total.value / dt / 1e9)
    if device:
        r["device_ms"] = {k: ctx.timing_get(k)[0] for k in ("genome_h2d", "genome_inflate", "genome_parse")}
        ctx.timing(False)
    return r


def time_python(ctx, path):
    spec = importlib.util.spec_from_file_location("map_files_tool", os.path.join(os.path.dirname(os.path.abspath(__file__)), "map_files.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    t = time.perf_counter()
    names, pos, seq = m.read_genome(path)
    index.load_genome(ctx, seq)
    cp = (C.c_uint64 * len(pos))(*pos)
    ctx.check(ctx.lib.lra_ctx_load_chromosomes(ctx.h, cp, len(pos) - 1))
    dt = time.perf_counter() - t
    return dict(seconds=dt, records=len(names), bases=pos[-1], gbases_per_s=pos[-1] / dt / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=3_100_000_000)
    ap.add_argument("--gzip-bases", type=int, default=None, help="size of the genome the gzip forms are timed on (default: --bases; 0: skip)")
    ap.add_argument("--records", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--skip-python", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gz_bases = args.bases if args.gzip_bases is None else args.gzip_bases
    ctx = Context(0)
    lib = ctx.lib
    res = dict(bases=args.bases, records=args.records, gzip_bases=gz_bases)
    best = lambda runs: min(runs, key=lambda r: r["seconds"])
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "genome.fa")
        t = time.perf_counter()
        write_genome(fa, args.bases, args.records)
        bg = os.path.join(tmp, "genome.bgzf.fa.gz")
        write_bgzf(fa, bg)
        sys.stderr.write("wrote %.2f GB plain, %.2f GB BGZF in %.1f s\n" % (os.path.getsize(fa) / 1e9, os.path.getsize(bg) / 1e9, time.perf_counter() - t))
        res["file_bytes"] = dict(plain=os.path.getsize(fa), bgzf=os.path.getsize(bg))
        for key, path in (("plain", fa), ("bgzf", bg)):
            warm(path)
            res[key] = dict(device=best([time_form(lib, ctx, path, True) for _ in range(args.repeats)]), host=time_form(lib, ctx, path, False))
            sys.stderr.write("%s: %s\n" % (key, json.dumps(res[key])))
        if not args.skip_python:
            res["plain"]["python_read_genome"] = time_python(ctx, fa)
            sys.stderr.write("python: %s\n" % json.dumps(res["plain"]["python_read_genome"]))
        if gz_bases:
            small = fa
            if gz_bases != args.bases:
                small = os.path.join(tmp, "small.fa")
                write_genome(small, gz_bases, max(1, args.records * gz_bases // max(1, args.bases)))
            gz = os.path.join(tmp, "genome.fa.gz")
            t = time.perf_counter()
            write_gzip(small, gz)
            sys.stderr.write("wrote %.2f GB gzip in %.1f s\n" % (os.path.getsize(gz) / 1e9, time.perf_counter() - t))
            res["file_bytes"]["gzip"] = os.path.getsize(gz)
            warm(gz)
            res["gzip"] = dict(device=time_form(lib, ctx, gz, True), host=time_form(lib, ctx, gz, False))
            sys.stderr.write("gzip: %s\n" % json.dumps(res["gzip"]))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
