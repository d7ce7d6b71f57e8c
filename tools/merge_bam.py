"""Merge coordinate-sorted BAM files with equal reference tables into one sorted, indexed file (needs the GPU):

    python tools/merge_bam.py a.bam b.bam ... -o out.bam [--mem BYTES]

The files are streamed through the device merger (lra_bam_merger: 1 .. 256 files, at most --mem bytes of device memory, default 8 GiB).  out.bam gets the
first file's header, the merged records -- ties in the order of the files, then in file order -- and the EOF member; out.bam.bai is written beside it.
A file that is not sorted by coordinate, has another reference table or a bad BGZF member is named on stderr and nothing is left behind."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lra_amd import bgzf, deflate
from lra_amd._lib import LraError
from lra_amd.bam import BamMerger
from lra_amd.context import Context


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="+", help="coordinate-sorted BAM files")
    ap.add_argument("-o", dest="out", required=True, help="the merged file; its index is written to OUT.bai")
    ap.add_argument("--mem", type=int, default=8 << 30, metavar="BYTES", help="device memory the merger may use (default 8 GiB)")
    args = ap.parse_args()
    ctx = Context(0)
    try:
        m = BamMerger(ctx, args.files, args.mem, 0)                                # the header first: its compressed length is where the first member starts
        raw = m.header()[0]
        m.close()
        head = b"".join(deflate.deflate_members([raw[a:a + deflate.IN_MAX] for a in range(0, len(raw), deflate.IN_MAX)])[0])
        m = BamMerger(ctx, args.files, args.mem, len(head))
        try:
            with open(args.out, "wb") as f:
                f.write(head)
                for piece in m.pieces():
                    f.write(piece)
                f.write(bgzf.EOF_BLOCK)
            bai = m.index()
            with open(args.out + ".bai", "wb") as f:
                f.write(bai)
            st = m.stats()
        finally:
            m.close()
    except LraError as e:
        for p in (args.out, args.out + ".bai"):
            if os.path.exists(p):
                os.remove(p)
        sys.stderr.write("merge_bam: %s\n" % e)
        ctx.close()
        sys.exit(1)
    sys.stderr.write("merge_bam: %d files, %d records, %d bytes of records in %d rounds; at most %d bytes of device memory\n"
                     % (len(args.files), st["records"], st["bytes"], st["rounds"], st["peak_device_bytes"]))
    ctx.close()


if __name__ == "__main__":
    main()
