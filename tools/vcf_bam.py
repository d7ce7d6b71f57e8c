"""Print the insertions and deletions of a BAM file's alignments as VCF, whole or for regions reached through its .bai index (needs the GPU):

    python tools/vcf_bam.py in.bam --ref genome.fa[.gz] [--sample S] [--minLength N] [--chrom NAME | REGION ...] [-f INT] [-F INT] [-Q INT] [--one-based]
                            [--drop-contained] [-o out.vcf] [--window BYTES]

What the reference's call_assembly_SVs/SamToVCF.py prints, walked and printed on the device (lra_bam_vcf; include/lra_hip.h states the rules and the
three places where the script is not followed): the script's header lines, then one line per insertion and deletion of every mapped record, in the
file's order.  The genome is read with the device reader (plain, gzip or BGZF FASTA; no .fai needed) and must list the chromosomes in the order of the
BAM header's reference table; the ##contig lines are that table's.  POS is the 0-based position of the anchor base, as the script prints it;
--one-based prints that + 1, as VCF means it.  --chrom NAME is the pass over one reference; a REGION is `name` or `name:beg-end`, 1-based and inclusive,
and prints the variants whose anchor lies inside; both need in.bam.bai.  -F drops records with any of these flag bits (default 0x4: unmapped), -f keeps
those with all of them, -Q those with at least this MAPQ.  --drop-contained does not walk a record that lies inside an earlier one of its reference (the
reference's ParseAlignment.py, for a coordinate-sorted BAM of contig alignments: a nested alignment's indels are not called again); with it a REGION begins
at the reference's first base.  A file the pass refuses is named on stderr; the lines in front of a fault are printed first."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lra_amd._lib import LraError
from lra_amd.bam import BamVcf, parse_region, vcf_header
from lra_amd.context import Context
from lra_amd.genome_io import GenomeFile


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("bam", help="the BAM file")
    ap.add_argument("regions", nargs="*", metavar="REGION", help="name or name:beg-end (1-based, inclusive)")
    ap.add_argument("--ref", required=True, help="the genome FASTA (plain, gzip or BGZF)")
    ap.add_argument("--sample", default="unknown", help="the sample's name in the column line")
    ap.add_argument("--minLength", type=int, default=1, metavar="N", help="print variants with |len(ALT) - len(REF)| >= N")
    ap.add_argument("--chrom", default=None, metavar="NAME", help="process this reference only")
    ap.add_argument("-f", dest="require", type=lambda s: int(s, 0), default=0, metavar="INT", help="keep records with all of these flag bits")
    ap.add_argument("-F", dest="exclude", type=lambda s: int(s, 0), default=None, metavar="INT", help="keep records with none of these flag bits (default 0x4)")
    ap.add_argument("-Q", dest="min_mapq", type=int, default=0, metavar="INT", help="keep records with at least this MAPQ")
    ap.add_argument("--one-based", dest="one_based", action="store_true", help="print POS + 1")
    ap.add_argument("--drop-contained", dest="drop_contained", action="store_true", help="skip records that lie inside an earlier record of their reference")
    ap.add_argument("-o", dest="out", default=None, help="write to this file instead of stdout")
    ap.add_argument("--window", type=int, default=0, metavar="BYTES", help="compressed bytes per step (at least 65536)")
    args = ap.parse_intermixed_args()                                          # (regions may stand behind the options)
    regions = ([args.chrom] if args.chrom is not None else []) + args.regions
    bai = args.bam + ".bai" if os.path.exists(args.bam + ".bai") else None
    if regions and bai is None:
        sys.stderr.write("vcf_bam: %s has no index (%s.bai): --chrom and regions need one\n" % (args.bam, args.bam))
        sys.exit(1)
    out = open(args.out, "wb") if args.out else sys.stdout.buffer
    ctx = Context(0)
    rc = 0
    try:
        g = GenomeFile(args.ref, ctx)
        try:
            g.read().install(ctx)
        finally:
            g.close()
        d = BamVcf(ctx, args.bam, bai, require=args.require, exclude=args.exclude, min_mapq=args.min_mapq, min_length=max(args.minLength, 0),
                   pos_one_based=args.one_based, window_bytes=args.window, drop_contained=args.drop_contained)
        try:
            names, lens = d.header()
            passes = [parse_region(r, names, lens) for r in regions] or [(None, 0, None)]
            out.write(vcf_header(args.ref, names, lens, args.sample))
            for ref, beg, end in passes:
                for piece in d.fetch(ref, beg, end):
                    out.write(piece[2])
        finally:
            d.close()
    except (LraError, ValueError, IOError) as e:
        sys.stderr.write("vcf_bam: %s\n" % e)
        rc = 1
    out.flush()
    if args.out:
        out.close()
    ctx.close()
    sys.exit(rc)


if __name__ == "__main__":
    main()
