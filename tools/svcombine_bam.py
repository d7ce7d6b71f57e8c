"""Combine two haplotypes' assembly SV calls into the diploid call set, from two coordinate-sorted BAMs of contig alignments (needs the GPU):

    python tools/svcombine_bam.py maternal.bam paternal.bam --ref genome.fa[.gz] [--mask BED] [--minSize 40] [--aligner aligner] [--frac 3/10] [--pass-filter]
                                  [--chrom NAME] [--one-based] [--sample S] [--window BYTES] -o PREFIX

The reference's call_assembly_SVs/callassemblysv.snakefile from the two sorted BAMs to the files of its `rule all`: each haplotype's calls as
tools/svcalls_bam.py makes them, then the rules Homcalls, Hetcalls and combineHet, on the device (lra_sv_combine; include/lra_hip.h states the rules).  A
maternal and a paternal call of one kind are partners when they share at least --frac of both (bedtools intersect -f 0.3 -r).  It writes seven files:

    PREFIX.maternal.INS.het.vcf  PREFIX.maternal.DEL.het.vcf     the maternal calls without a paternal partner
    PREFIX.paternal.INS.het.vcf  PREFIX.paternal.DEL.het.vcf     the paternal calls without a maternal partner
    PREFIX.INS.hom.vcf           PREFIX.DEL.hom.vcf              the maternal calls with one, once each
    PREFIX.vcf                                                   the header of tools/vcf_bam.py, then the six bodies in that order

one line per call:  RNAME  START  ID  REF  ALT  60  INFO  INFO  GT  1/1  -- the snakefile's awk prints INFO in the FILTER column too, and 1/1 in the het files
as well; this tool prints what it prints.  --pass-filter writes PASS there, and --frac 1/10 --pass-filter is combinehapSV.snakefile's output.  An empty
class gives an empty file.  --mask, --minSize, --aligner, --chrom (both files need their .bai), --one-based and --window are tools/svcalls_bam.py's.  The
genome must list the chromosomes in the order of both BAM headers' reference tables, which must be equal.  A file a pass refuses is named on stderr with its
haplotype, and nothing is written into the seven files."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lra_amd._lib import LraError
from lra_amd.bam import SVCOMBINE_FILES, SvCombine, parse_bed, parse_frac, vcf_header
from lra_amd.context import Context
from lra_amd.genome_io import GenomeFile


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("maternal", help="the maternal haplotype's coordinate-sorted BAM file")
    ap.add_argument("paternal", help="the paternal haplotype's coordinate-sorted BAM file")
    ap.add_argument("--ref", required=True, help="the genome FASTA (plain, gzip or BGZF)")
    ap.add_argument("--mask", default=None, metavar="BED", help="drop calls that share a base with an interval of this BED file")
    ap.add_argument("--minSize", type=int, default=40, metavar="N", help="keep calls with |SVLEN| >= N")
    ap.add_argument("--aligner", default="aligner", help="the first word of the IDs")
    ap.add_argument("--frac", default="3/10", metavar="NUM/DEN", help="partners share at least this fraction of both calls")
    ap.add_argument("--pass-filter", dest="filter_pass", action="store_true", help="print PASS in the FILTER column, not INFO a second time")
    ap.add_argument("--chrom", default=None, metavar="NAME", help="process this reference only")
    ap.add_argument("--one-based", dest="one_based", action="store_true", help="print START + 1")
    ap.add_argument("--sample", default="unknown", help="the sample's name in the column line of PREFIX.vcf")
    ap.add_argument("--window", type=int, default=0, metavar="BYTES", help="compressed bytes per step (at least 65536)")
    ap.add_argument("-o", dest="prefix", required=True, metavar="PREFIX", help="the output files' prefix")
    args = ap.parse_args()
    try:
        frac = parse_frac(args.frac)
    except ValueError as e:
        sys.stderr.write("svcombine_bam: %s\n" % e)
        sys.exit(1)
    bai = [b + ".bai" if os.path.exists(b + ".bai") else None for b in (args.maternal, args.paternal)]
    if args.chrom is not None and None in bai:
        b = (args.maternal, args.paternal)[bai.index(None)]
        sys.stderr.write("svcombine_bam: %s has no index (%s.bai): --chrom needs one\n" % (b, b))
        sys.exit(1)
    ctx = Context(0)
    rc = 0
    try:
        g = GenomeFile(args.ref, ctx)
        try:
            g.read().install(ctx)
        finally:
            g.close()
        d = SvCombine(ctx, args.maternal, args.paternal, bai[0], bai[1], min_size=max(args.minSize, 0), aligner=args.aligner, pos_one_based=args.one_based,
                      frac=frac, filter_pass=args.filter_pass, window_bytes=args.window)
        try:
            names, lens = d.header()
            if args.mask is not None:
                with open(args.mask, "rb") as f:
                    d.set_mask(parse_bed(f, names))
            body = {key: b"" for key, _ in SVCOMBINE_FILES}
            for hap, kind, cls, _, _, text in d.fetch(args.chrom):                  # (nothing comes before both passes have ended: a refusal writes no file)
                body[hap, kind, cls] += text
            for key, suffix in SVCOMBINE_FILES:
                with open(args.prefix + suffix, "wb") as f:
                    f.write(body[key])
            with open(args.prefix + ".vcf", "wb") as f:
                f.write(vcf_header(args.ref, names, lens, args.sample) + b"".join(body[key] for key, _ in SVCOMBINE_FILES))
        finally:
            d.close()
    except (LraError, ValueError, IOError) as e:
        sys.stderr.write("svcombine_bam: %s\n" % e)
        rc = 1
    ctx.close()
    sys.exit(rc)


if __name__ == "__main__":
    main()
