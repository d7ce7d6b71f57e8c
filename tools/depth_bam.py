"""Print the coverage of a coordinate-sorted BAM file, per base or per bin, whole or for regions reached through its .bai index (needs the GPU):

    python tools/depth_bam.py in.bam [REGION ...] [-a] [-J] [-Q INT] [-f INT] [-F INT] [--bin N] [-o out.tsv] [--window BYTES] [--span BASES]

The file is inflated, framed, filtered and turned into depth on the device (lra_bam_depth).  Without --bin a line is `RNAME POS DEPTH` (POS 1-based) for
every position with depth > 0, with -a for every position; with --bin N a line is `RNAME START END MEAN` (0-based, half-open) for every bin of N bases.
A REGION is `name` or `name:beg-end`, 1-based and inclusive, as samtools takes it; regions need in.bam.bai and print one after the other.  Records that
are unmapped, secondary, QC-fail or duplicate are dropped (-F, default 0x704); -f keeps the records with all of these bits, -Q those with at least this
MAPQ; -J counts deletions as covered.  --window: compressed bytes per step; --span: reference positions held on the device at once (defaults: the
library's).  A file the pass refuses is named on stderr; the lines in front of a fault are printed first."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lra_amd._lib import LraError
from lra_amd.bam import BamDepth, parse_region
from lra_amd.context import Context


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("bam", help="the BAM file")
    ap.add_argument("regions", nargs="*", metavar="REGION", help="name or name:beg-end (1-based, inclusive)")
    ap.add_argument("-a", dest="all_positions", action="store_true", help="print every position, those of depth 0 too")
    ap.add_argument("-J", dest="count_deletions", action="store_true", help="count deletions as covered")
    ap.add_argument("-Q", dest="min_mapq", type=int, default=0, metavar="INT", help="keep records with at least this MAPQ")
    ap.add_argument("-f", dest="require", type=lambda s: int(s, 0), default=0, metavar="INT", help="keep records with all of these flag bits")
    ap.add_argument("-F", dest="exclude", type=lambda s: int(s, 0), default=None, metavar="INT", help="keep records with none of these flag bits (default 0x704)")
    ap.add_argument("--bin", type=int, default=0, metavar="N", help="print the mean depth of bins of N bases")
    ap.add_argument("-o", dest="out", default=None, help="write to this file instead of stdout")
    ap.add_argument("--window", type=int, default=0, metavar="BYTES", help="compressed bytes per step (at least 65536)")
    ap.add_argument("--span", type=int, default=0, metavar="BASES", help="reference positions held on the device at once (at least 65536)")
    args = ap.parse_args()
    bai = args.bam + ".bai" if os.path.exists(args.bam + ".bai") else None
    if args.regions and bai is None:
        sys.stderr.write("depth_bam: %s has no index (%s.bai): regions need one\n" % (args.bam, args.bam))
        sys.exit(1)
    out = open(args.out, "wb") if args.out else sys.stdout.buffer
    ctx = Context(0)
    rc = 0
    try:
        d = BamDepth(ctx, args.bam, bai, require=args.require, exclude=args.exclude, min_mapq=args.min_mapq, count_deletions=args.count_deletions,
                     bin=args.bin, all_positions=args.all_positions, window_bytes=args.window, span_bases=args.span)
        try:
            names, lens = d.header()
            passes = [parse_region(r, names, lens) for r in args.regions] or [(None, 0, None)]
            for ref, beg, end in passes:
                for piece in d.fetch(ref, beg, end):
                    out.write(piece[4])
        finally:
            d.close()
    except (LraError, ValueError) as e:
        sys.stderr.write("depth_bam: %s\n" % e)
        rc = 1
    out.flush()
    if args.out:
        out.close()
    ctx.close()
    sys.exit(rc)


if __name__ == "__main__":
    main()
