"""`lra index`: a genome FASTA (plain text, gzip or BGZF) into its index files genome.mms and genome.gli (needs the GPU):

    python tools/index_files.py -ONT|-CLR|-CCS|-CONTIG genome.fa[.gz] [-K k] [-W w] [-F freq] [-N n] [--globalWinsize s] [-k k] [-w w] [-f freq]
                                [--localIndexWindow s]

The option letters and values are those of RunStoreGlobal and RunStoreLocal (lra.cpp:867-, :780-865): -K / -W / -F / -N / --globalWinsize override the
preset's global index parameters (index.INDEX_PRESETS); the local index is k = 10, w = 5, windows of 2048, max frequency 15 under every preset unless
-k / -w / --localIndexWindow / -f say otherwise.  The genome is read and parsed on the device (lra_genome_read_device), both indexes are built there
(lra_ctx_build_global_index, lra_ctx_build_local_index) and written with lra_write_mms / lra_write_gli.  Stage times go to stderr."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lra_amd import genome_io, index
from lra_amd.context import Context

LOCAL_INDEX = (10, 5, 2048, 15)                                                   # k, w, localIndexWindow, localMaxFreq of `lra index`


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    pre = ap.add_mutually_exclusive_group(required=True)
    for p in ("ONT", "CLR", "CCS", "CONTIG"):
        pre.add_argument("-" + p, dest="preset", action="store_const", const=p)
    ap.add_argument("genome")
    ap.add_argument("-K", dest="K", type=int, default=None, help="global k")
    ap.add_argument("-W", dest="W", type=int, default=None, help="global w")
    ap.add_argument("-F", dest="F", type=int, default=None, help="global max frequency")
    ap.add_argument("-N", dest="N", type=int, default=None, help="minimizers kept per window")
    ap.add_argument("--globalWinsize", type=int, default=None)
    ap.add_argument("-k", dest="k", type=int, default=None, help="local k")
    ap.add_argument("-w", dest="w", type=int, default=None, help="local w")
    ap.add_argument("-f", dest="f", type=int, default=None, help="local max frequency")
    ap.add_argument("--localIndexWindow", type=int, default=None)
    ap.add_argument("--chunk", type=int, default=None, help="bytes of the genome file read and parsed per step (default: the library's)")
    args = ap.parse_args()
    K, W, F, S, N = index.INDEX_PRESETS[args.preset.lower()]
    K, W, F, S, N = [d if v is None else v for v, d in ((args.K, K), (args.W, W), (args.F, F), (args.globalWinsize, S), (args.N, N))]
    k, w, win, f = [d if v is None else v for v, d in zip((args.k, args.w, args.localIndexWindow, args.f), LOCAL_INDEX)]
    ctx = Context(0)
    t0 = time.perf_counter()
    gf = genome_io.GenomeFile(args.genome, ctx=ctx, chunk=args.chunk)
    try:
        gf.read()
    except IOError as e:
        raise SystemExit("index_files: %s" % e)
    if not gf.names:
        raise SystemExit("%s: no FASTA records" % args.genome)
    gf.install(ctx)
    t_read = time.perf_counter() - t0
    t = time.perf_counter()
    st = index.build_global_index(ctx, gf.chrom_pos, K, W, F, S, N)
    key, pos = index.global_index(ctx)
    index.write_mms(args.genome + ".mms", K, gf.names, gf.chrom_pos, key, pos)
    t_global = time.perf_counter() - t
    t = time.perf_counter()
    ctx.check(ctx.lib.lra_ctx_build_local_index(ctx.h, k, w, win, f))
    li = index.local_index(ctx)
    index.write_gli(args.genome + ".gli", li["k"], li["w"], li["window"], li["seq_offsets"], li["tuple_bnd"], li["tuples"])
    t_local = time.perf_counter() - t
    sys.stderr.write("index_files: %d sequences, %d bases; read+parse (device) %.2f s, global index %.2f s (%d of %d minimizers kept), local index %.2f s (%d windows, "
                     "%d minimizers)\n" % (len(gf.names), gf.chrom_pos[-1], t_read, t_global, st["n_index"], st["n_minimizers"], t_local, len(li["tuple_bnd"]) - 1,
                                           len(li["tuples"])))
    gf.close()
    ctx.close()


if __name__ == "__main__":
    main()
