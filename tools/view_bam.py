"""Print a BAM file as SAM text, whole or for regions reached through its .bai index (needs the GPU):

    python tools/view_bam.py in.bam [REGION ...] [-h | -H] [-c] [-f INT] [-F INT] [-o out.sam] [--window BYTES]

The file is inflated, framed, filtered and printed on the device (lra_bam_view).  A REGION is `name` or `name:beg-end`, 1-based and inclusive, as
samtools view takes it; regions need in.bam.bai, which is used when it exists, and print one after the other (a record that overlaps two regions prints
twice).  -h prints the header in front of the records, -H the header alone, -c the number of records instead of the records; -f / -F keep the records
that have all of / none of the flag bits.  --window: compressed bytes per step (default: the library's).  A file or an index the view refuses is named
on stderr; the records in front of a fault are printed first."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lra_amd._lib import LraError
from lra_amd.bam import BamView, parse_region
from lra_amd.context import Context


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, add_help=False)
    ap.add_argument("--help", action="help", help="show this help and exit")
    ap.add_argument("bam", help="the BAM file")
    ap.add_argument("regions", nargs="*", metavar="REGION", help="name or name:beg-end (1-based, inclusive)")
    ap.add_argument("-h", dest="with_header", action="store_true", help="print the header in front of the records")
    ap.add_argument("-H", dest="header_only", action="store_true", help="print the header only")
    ap.add_argument("-c", dest="count", action="store_true", help="print the number of records only")
    ap.add_argument("-f", dest="require", type=lambda s: int(s, 0), default=0, metavar="INT", help="keep records with all of these flag bits")
    ap.add_argument("-F", dest="exclude", type=lambda s: int(s, 0), default=0, metavar="INT", help="keep records with none of these flag bits")
    ap.add_argument("-o", dest="out", default=None, help="write to this file instead of stdout")
    ap.add_argument("--window", type=int, default=0, metavar="BYTES", help="compressed bytes per step (at least 65536)")
    args = ap.parse_args()
    bai = args.bam + ".bai" if os.path.exists(args.bam + ".bai") else None
    if args.regions and bai is None and not args.header_only:
        sys.stderr.write("view_bam: %s has no index (%s.bai): regions need one\n" % (args.bam, args.bam))
        sys.exit(1)
    out = open(args.out, "wb") if args.out else sys.stdout.buffer
    ctx = Context(0)
    rc = 0
    try:
        v = BamView(ctx, args.bam, bai, args.window)
        try:
            text, names, lens = v.header()
            passes = [parse_region(r, names, lens) for r in args.regions] or [(None, 0, None)]
            if args.header_only or (args.with_header and not args.count):
                out.write(text)
            if not args.header_only:
                v.set_flags(args.require, args.exclude)
                n = 0
                for ref, beg, end in passes:
                    for piece in v.fetch(ref, beg, end):
                        if not args.count:
                            out.write(piece)
                    n += v.last_records
                if args.count:
                    out.write(b"%d\n" % n)
        finally:
            v.close()
    except (LraError, ValueError) as e:
        sys.stderr.write("view_bam: %s\n" % e)
        rc = 1
    out.flush()
    if args.out:
        out.close()
    ctx.close()
    sys.exit(rc)


if __name__ == "__main__":
    main()
