"""Call assembly SVs from a coordinate-sorted BAM of one haplotype's contig alignments: the merged DEL and INS tables (needs the GPU):

    python tools/svcalls_bam.py sorted.bam --ref genome.fa[.gz] [--mask centromere.bed] [--minSize 40] [--aligner aligner] [--hap maternal] [--chrom NAME]
                                [--no-drop-contained] [-f INT] [-F INT] [-Q INT] [--one-based] [--vcf] [--sample S] [--window BYTES] -o PREFIX

The one-haplotype half of the reference's call_assembly_SVs/callassemblysv.snakefile -- ParseAlignment.py, SamToVCF.py, the size filter, the centromere
mask, the IDs and mergeSV.py -- on the device (lra_bam_svcalls; include/lra_hip.h states the rules and the two places where the snakefile is not what it
seems).  It writes PREFIX.DEL.merge.vcf and PREFIX.INS.merge.vcf: one line per kept call,

    RNAME  START  END  ID  REF  ALT  60  PASS  INFO  GT  1/1

with START the anchor's 0-based position, END = START + |SVLEN| and ID = <aligner>.<DEL|INS>.<hap>.<NR>.  --aligner defaults to the literal word "aligner",
which is what the snakefile's awk prints.  --vcf writes PREFIX.vcf instead: the header of tools/vcf_bam.py, then ten columns per call with the ID in the third
and no END -- the lines in the order they are delivered, a reference's DEL calls in front of its INS calls, not sorted by position.  --one-based prints
START (and END) + 1, as tools/vcf_bam.py does for POS.  --mask is a BED file (0-based, half-open) parsed here; its names are matched to the BAM header's and
unknown names are ignored.  --chrom NAME is the pass over one reference (it needs sorted.bam.bai); its calls are numbered from 1.  -F drops records with any
of these flag bits (default 0x4), -f keeps those with all of them, -Q those with at least this MAPQ.  The genome must list the chromosomes in the order of
the BAM header's reference table.  A file the pass refuses is named on stderr; the calls of the references finished in front of the fault are written first."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lra_amd._lib import LraError
from lra_amd.bam import BamSvCalls, parse_bed, vcf_header
from lra_amd.context import Context
from lra_amd.genome_io import GenomeFile


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("bam", help="the coordinate-sorted BAM file")
    ap.add_argument("--ref", required=True, help="the genome FASTA (plain, gzip or BGZF)")
    ap.add_argument("--mask", default=None, metavar="BED", help="drop calls that share a base with an interval of this BED file")
    ap.add_argument("--minSize", type=int, default=40, metavar="N", help="keep calls with |SVLEN| >= N")
    ap.add_argument("--aligner", default="aligner", help="the first word of the IDs")
    ap.add_argument("--hap", default="maternal", help="the third word of the IDs")
    ap.add_argument("--chrom", default=None, metavar="NAME", help="process this reference only")
    ap.add_argument("--no-drop-contained", dest="drop_contained", action="store_false", help="keep the alignments that lie inside an earlier one")
    ap.add_argument("-f", dest="require", type=lambda s: int(s, 0), default=0, metavar="INT", help="keep records with all of these flag bits")
    ap.add_argument("-F", dest="exclude", type=lambda s: int(s, 0), default=None, metavar="INT", help="keep records with none of these flag bits (default 0x4)")
    ap.add_argument("-Q", dest="min_mapq", type=int, default=0, metavar="INT", help="keep records with at least this MAPQ")
    ap.add_argument("--one-based", dest="one_based", action="store_true", help="print START and END + 1")
    ap.add_argument("--vcf", action="store_true", help="write PREFIX.vcf: a header and ten columns, in delivery order")
    ap.add_argument("--sample", default="unknown", help="the sample's name in the column line of --vcf")
    ap.add_argument("--window", type=int, default=0, metavar="BYTES", help="compressed bytes per step (at least 65536)")
    ap.add_argument("-o", dest="prefix", required=True, metavar="PREFIX", help="the output files' prefix")
    args = ap.parse_args()
    bai = args.bam + ".bai" if os.path.exists(args.bam + ".bai") else None
    if args.chrom is not None and bai is None:
        sys.stderr.write("svcalls_bam: %s has no index (%s.bai): --chrom needs one\n" % (args.bam, args.bam))
        sys.exit(1)
    out = {}
    ctx = Context(0)
    rc = 0
    try:
        g = GenomeFile(args.ref, ctx)
        try:
            g.read().install(ctx)
        finally:
            g.close()
        d = BamSvCalls(ctx, args.bam, bai, require=args.require, exclude=args.exclude, min_mapq=args.min_mapq, min_size=max(args.minSize, 0),
                       drop_contained=args.drop_contained, aligner=args.aligner, hap=args.hap, pos_one_based=args.one_based, vcf_columns=args.vcf,
                       window_bytes=args.window)
        try:
            names, lens = d.header()
            if args.mask is not None:
                with open(args.mask, "rb") as f:
                    d.set_mask(parse_bed(f, names))
            if args.vcf:
                out["DEL"] = out["INS"] = open(args.prefix + ".vcf", "wb")
                out["DEL"].write(vcf_header(args.ref, names, lens, args.sample))
            else:
                out = {k: open("%s.%s.merge.vcf" % (args.prefix, k), "wb") for k in ("DEL", "INS")}
            for _, kind, _, _, text in d.fetch(args.chrom):
                out[kind].write(text)
        finally:
            d.close()
    except (LraError, ValueError, IOError) as e:
        sys.stderr.write("svcalls_bam: %s\n" % e)
        rc = 1
    for f in set(out.values()):
        f.close()
    ctx.close()
    sys.exit(rc)


if __name__ == "__main__":
    main()
