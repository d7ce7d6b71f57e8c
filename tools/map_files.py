"""Map read files against a genome FASTA and print the records as `lra align` would (needs the GPU):

    python tools/map_files.py -ONT genome.fa reads.fq [more.fa ...] [-p s|p|pc|b|a] [-H] [--printMD] [-a] [--PrintNumAln N] [--refineBreakpoints] [-o out.sam] [--device-records] [--bgzf | --bam [--sort [--sort-mem BYTES] [--merge-runs]]]

The reads are parsed on the device (lra_reads_next_batch_device) and mapped from the reader's device arrays; --host-input parses them on the host
(lra_reads_next_batch) and maps through lra_map_reads_host, the same records.  The index: genome.fa.mms / genome.fa.gli when both exist (lra_read_mms /
lra_read_gli), else built on the device with the preset's `lra index` parameters.  The genome (plain text, gzip or BGZF) is parsed on the device too
(lra_genome_read_device); --host-genome parses it on the host (lra_genome_read_host).  --bgzf writes the output BGZF-compressed: the header through
lra_bgzf_deflate_host, every batch's records deflated on the device, the EOF member at the end.  --bam writes a BAM file (in read order, not indexed):
lra_bam_header's bytes as BGZF members, every batch's BAM records encoded and deflated on the device (lra_map_records_device_bam), the EOF member.
--bam --sort writes a coordinate-sorted BAM file and its index, out.bam and out.bam.bai (-o is required): the header text gets "@HD VN:1.6 SO:coordinate"
in front, every batch's records go to a device sorter (lra_bam_sorter, at most --sort-mem bytes of device memory), which gives back the sorted members and
the .bai bytes.  When the records do not fit one run, every run becomes a complete sorted, indexed file of its own -- out.run0000.bam, out.run0000.bam.bai,
out.run0001.bam, ... -- and the tool says so on stderr.  --merge-runs then merges the runs on the device (lra_bam_merger, under the same --sort-mem) into
out.bam and out.bam.bai, the bytes one run of a large enough budget would have given, and removes the run files; if the merge fails they stay and the
tool says why.  The SV signatures (-SV) stay per batch, in read order.
Per-stage times go to stderr."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from lra_amd import bgzf, deflate, genome_io, index, mapread, reads_io
from lra_amd.context import Context

INDEX_PARAMS = {"ONT": (17, 10, 150, 15, 1), "CLR": (15, 10, 250, 12, 1), "CCS": (17, 10, 150, 15, 1), "CONTIG": (19, 10, 30, 20, 1)}   # `lra index -<preset>`
PRESET_BATCH = 500_000_000                                                        # bases per batch: about the bench batch's device footprint


def read_genome(path):
    """-> (names, chrom_pos, upper-case bases back to back) of a plain FASTA file (Genome::Read: the name is the header's first token).  main reads the
    genome through lra_amd.genome_io; this stays as the tests' independent yardstick."""
    names, parts, pos = [], [], [0]
    cur = []
    with open(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if names:
                    s = b"".join(cur).upper(); parts.append(s); pos.append(pos[-1] + len(s)); cur = []
                tok = line[1:].split()
                names.append(tok[0] if tok else b"")
            elif line:
                cur.append(line)
    if names:
        s = b"".join(cur).upper(); parts.append(s); pos.append(pos[-1] + len(s))
    if not names:
        raise SystemExit("%s: no FASTA records" % path)
    return names, pos, np.frombuffer(b"".join(parts), np.uint8).copy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    pre = ap.add_mutually_exclusive_group(required=True)
    for p in ("ONT", "CLR", "CCS", "CONTIG"):
        pre.add_argument("-" + p, dest="preset", action="store_const", const=p)
    ap.add_argument("genome")
    ap.add_argument("reads", nargs="+")
    ap.add_argument("-p", dest="fmt", default="s", choices=["s", "p", "pc", "b", "a"], help="print format: SAM, PAF, PAF with cigar, BED, pairwise")
    ap.add_argument("-H", dest="hard_clip", action="store_true", help="hard-clip SAM records")
    ap.add_argument("--printMD", action="store_true", help="MD:Z in SAM records")
    ap.add_argument("-a", dest="store_all", action="store_true", help="seed from every k-mer of a read")
    ap.add_argument("-SV", dest="sv", nargs=2, metavar=("LEN", "PATH"), default=None,
                    help="write the SV signatures (net gaps inside an alignment longer than LEN) of every read to PATH")
    ap.add_argument("--PrintNumAln", type=int, default=1)
    ap.add_argument("--refineBreakpoints", action="store_true")
    ap.add_argument("-o", dest="out", default=None, help="output file (default stdout)")
    ap.add_argument("--host-input", action="store_true", help="parse the read files on the host (lra_reads_next_batch)")
    ap.add_argument("--batch-bases", type=int, default=PRESET_BATCH, help="bases per batch (a batch ends with the read that crosses this)")
    ap.add_argument("--host-genome", action="store_true", help="parse the genome file on the host (lra_genome_read_host)")
    ap.add_argument("--chunk", type=int, default=None, help="bytes the device reader reads and parses per step (default: the library's)")
    ap.add_argument("-Flag", dest="flag", type=int, default=0, help="SAM / BAM input: skip records whose flag meets this mask")
    ap.add_argument("--passthrough", action="store_true", help="SAM / BAM input: append each read's aux fields to its SAM records")
    ap.add_argument("--device-records", action="store_true",
                    help="build the record text on the device (lra_map_records_device; formats s, pc and a, the others fall through to the host path)")
    ap.add_argument("--bgzf", action="store_true",
                    help="write the output as BGZF: the records are deflated on the device (with --device-records before they leave it: lra_map_records_device_bgzf)")
    ap.add_argument("--bam", action="store_true",
                    help="write BAM: the records are encoded and deflated on the device (lra_map_records_device_bam); implies --device-records and -p s")
    ap.add_argument("--sort", action="store_true", help="with --bam and -o: sort the records by coordinate on the device and write out.bam.bai beside the file")
    ap.add_argument("--sort-mem", type=int, default=8 << 30, metavar="BYTES", help="device memory the sorter may use (default 8 GiB); more records make several sorted files")
    ap.add_argument("--merge-runs", action="store_true", help="with --sort: when the records made several sorted runs, merge them on the device into -o and its index")
    args = ap.parse_args()
    if args.merge_runs and not args.sort:
        ap.error("--merge-runs merges the runs --sort made: it needs --sort")
    if args.sort and not (args.bam and args.out):
        ap.error("--sort sorts BAM output into a file and its index: it needs --bam and -o")
    if args.bam:
        if args.fmt != "s" or args.bgzf:
            ap.error("--bam writes SAM records (-p s) as BAM; it does not go with another format or with --bgzf")
        args.device_records = True
    P = args.preset
    t0 = time.perf_counter()
    ctx = Context(0)
    gf = genome_io.GenomeFile(args.genome, ctx=None if args.host_genome else ctx)
    try:
        gf.read()
    except IOError as e:
        raise SystemExit("map_files: %s" % e)
    if not gf.names:
        raise SystemExit("%s: no FASTA records" % args.genome)
    names, chrom_pos, genome = gf.names, gf.chrom_pos, gf.seq
    gf.close()                                                                   # (the bases are a copy: a numpy array or a device tensor)
    mms, gli = args.genome + ".mms", args.genome + ".gli"
    ik = ipos = None
    gli_params = None
    if os.path.exists(mms) and os.path.exists(gli):
        m = index.read_mms(mms)
        assert [int(x) for x in m["chrom_pos"]] == chrom_pos, "the .mms file is of another genome"
        ik, ipos = m["key"], m["pos"]
        g = index.read_gli(gli)
        gli_params = (g["k"], g["w"], g["window"])
    fmt = {"s": "s", "p": "p", "pc": "c", "b": "b", "a": "a"}[args.fmt]
    if P in ("ONT", "CLR"):
        o = mapread.LowAccOptions() if P == "ONT" else mapread.clr_options()
        if gli_params:
            o = mapread.with_gli(o, *gli_params)
        o.printFormat = fmt; o.PrintNumAln = args.PrintNumAln; o.printMD = args.printMD; o.storeAll = args.store_all
        o.refineBreakpoint = args.refineBreakpoints
        if args.sv:
            o.svsigLen = int(args.sv[0])
        if args.hard_clip:
            o.hardClip = True
        mapper = mapread.LowAccMapper(ctx, genome, ik, ipos, names, chrom_pos, o, index_params=INDEX_PARAMS[P], staged=False)
    else:
        ov = dict(printFormat=ord(fmt), PrintNumAln=args.PrintNumAln, refineBreakpoint=int(args.refineBreakpoints), printMD=args.printMD, storeAll=args.store_all)
        if args.hard_clip:
            ov["hardClip"] = 1
        if args.sv:
            ov["svsigLen"] = int(args.sv[0])
        mapper = mapread.HighAccMapper(ctx, genome, ik, ipos, names, chrom_pos, preset=P.lower(), index_params=INDEX_PARAMS[P], gli=gli_params, **ov)
    t_index = time.perf_counter() - t0
    out = None if args.sort else open(args.out, "wb") if args.out else sys.stdout.buffer
    if fmt == "s":
        cl = ["lra", "align", "-" + P, args.genome, *args.reads, "-p", args.fmt] + (["-H"] if args.hard_clip else []) + (["--printMD"] if args.printMD else []) + \
             (["-a"] if args.store_all else []) + ["--PrintNumAln", str(args.PrintNumAln)] + (["--refineBreakpoints"] if args.refineBreakpoints else []) + \
             (["-Flag", str(args.flag)] if args.flag else []) + (["--passthrough"] if args.passthrough else []) + (["-SV", *args.sv] if args.sv else [])       # (--device-records is no lra option: the same records)
        head = mapread.LowAccMapper.sam_header(mapper, b"lra_amd", " ".join(cl).encode())     # the lra command line: the same for either reader
        if args.sort:
            head = b"@HD\tVN:1.6\tSO:coordinate\n" + head
        if args.bam:
            head = mapper.bam_header(head)
        if args.bgzf or args.bam:
            head = b"".join(deflate.deflate_members([head[a:a + deflate.IN_MAX] for a in range(0, len(head), deflate.IN_MAX)])[0])
        if out:
            out.write(head)
    sorter = run_no = None
    if args.sort:
        from lra_amd.bam import BamSorter, SorterFull
        from lra_amd._lib import LraError
        sorter, run_no = BamSorter(ctx, args.sort_mem), 0
        stem = args.out[:-4] if args.out.endswith(".bam") else args.out

        def write_run(last):
            """the sorter's records as a sorted file with its index: args.out when everything fitted one run, else stem.runNNNN.bam"""
            nonlocal run_no
            path = args.out if last and run_no == 0 else "%s.run%04d.bam" % (stem, run_no)
            n_held = sorter.held()[0]
            try:
                sorter.finish(len(head), np.diff(np.asarray(chrom_pos, np.int64)))
            except LraError as e:
                raise SystemExit("map_files: --sort-mem %d is too small to sort and index the %d records held: %s" % (args.sort_mem, n_held, e))
            with open(path, "wb") as f:
                f.write(head)
                for piece in sorter.pieces():
                    f.write(piece)
                f.write(bgzf.EOF_BLOCK)
            try:
                bai = sorter.index()
                with open(path + ".bai", "wb") as f:
                    f.write(bai)
            except LraError as e:
                sys.stderr.write("map_files: %s is not indexed: %s\n" % (path, e))
            if path != args.out:
                sys.stderr.write("map_files: the records do not fit one sorted run of %d bytes (--sort-mem): %s holds %d records, sorted and indexed on its own; "
                                 "%s\n" % (args.sort_mem, path, n_held, "--merge-runs merges the runs at the end" if args.merge_runs else "the runs are not merged"))
            run_no += 1

        def merge_runs():
            """the runs into args.out and its index, under the sorter's budget; the run files go when that worked"""
            from lra_amd.bam import BamMerger
            paths = ["%s.run%04d.bam" % (stem, i) for i in range(run_no)]
            try:
                m = BamMerger(ctx, paths, args.sort_mem, len(head))
                try:
                    with open(args.out, "wb") as f:
                        f.write(head)
                        for piece in m.pieces():
                            f.write(piece)
                        f.write(bgzf.EOF_BLOCK)
                    bai = m.index()
                    with open(args.out + ".bai", "wb") as f:
                        f.write(bai)
                finally:
                    m.close()
            except LraError as e:
                for p in (args.out, args.out + ".bai"):
                    if os.path.exists(p):
                        os.remove(p)
                sys.stderr.write("map_files: the %d runs are not merged and stay as they are: %s\n" % (run_no, e))
                return
            for p in paths:
                for q in (p, p + ".bai"):
                    if os.path.exists(q):
                        os.remove(q)
            sys.stderr.write("map_files: %d runs merged into %s\n" % (run_no, args.out))
    # --device-records with device input: the qualities stay on the device from the reader to the record text; the host copies of bases and qualities
    # are switched off where nothing reads them (the formats the device builds; with them -SV is built on the device too, from the result's own arrays)
    dev_quals = args.device_records and not args.host_input
    no_host = dev_quals and fmt in ("s", "c", "a")
    rf = reads_io.ReadsFile(args.reads, ctx=None if args.host_input else ctx, chunk=None if args.host_input else args.chunk, flag_remove=args.flag, compressed_text=True,
                            passthrough=args.passthrough, device_quals=dev_quals, no_host_copy=no_host)
    sv_out = open(args.sv[1], "wb") if args.sv else None
    t_read = t_map = t_rec = 0.0
    n_reads = n_bases = n_batches = 0
    failed = None
    while True:
        t = time.perf_counter()
        try:
            b = rf.next_batch(args.batch_bases)
        except IOError as e:                                                # a corrupt record or file: map the reads in front of it, then fail
            b, failed = e.partial, e
        t_read += time.perf_counter() - t
        if b is None:
            break
        t = time.perf_counter()
        res = reads_io.map_reads_host(mapper, b["raw"]) if args.host_input else reads_io.map_reads_device(mapper, b)
        t_map += time.perf_counter() - t
        t = time.perf_counter()
        tags = b["tags"] if args.passthrough else None
        if args.sort:                                                       # BAM records that stay on the device, in the sorter; the signatures stay plain, per batch
            rargs = mapper.record_args(b["names"], b["seqs"], b["quals"], lens=b.get("read_len"))
            while True:
                try:
                    r = mapper.records_device_bam_to_sorter(res, rargs, sorter, passthrough=tags, d_qual=b.get("d_qual"), d_qual_off=b.get("d_qual_off"), svsig=bool(sv_out))
                    break
                except SorterFull as e:
                    if sorter.held()[0] == 0:
                        raise SystemExit("map_files: --sort-mem %d does not hold one batch: %s" % (args.sort_mem, e))
                    write_run(False)
            texts = []
            for sig in (r[1] if sv_out else []):
                sv_out.write(sig)
        elif args.bam:                                                      # BAM records, BGZF members when they leave the device; the signatures stay plain
            r = mapper.records_device_bam(res, mapper.record_args(b["names"], b["seqs"], b["quals"], lens=b.get("read_len")), passthrough=tags,
                                          d_qual=b.get("d_qual"), d_qual_off=b.get("d_qual_off"), svsig=bool(sv_out), bgzf=True)
            texts = [r[0]]
            for sig in (r[3] if sv_out else []):
                sv_out.write(sig)
        elif args.bgzf and args.device_records:                             # the text leaves the device as BGZF members; the signatures stay plain
            r = mapper.records_device_bgzf(res, mapper.record_args(b["names"], b["seqs"], b["quals"], lens=b.get("read_len")), passthrough=tags,
                                           d_qual=b.get("d_qual"), d_qual_off=b.get("d_qual_off"), svsig=bool(sv_out))
            texts = [r[0]]
            for sig in (r[3] if sv_out else []):
                sv_out.write(sig)
        elif sv_out and args.device_records:                                # one call: the records and the signatures of the same batch, both in read order
            texts, sigs = mapper.records_device(res, mapper.record_args(b["names"], b["seqs"], b["quals"], lens=b.get("read_len")), passthrough=tags,
                                                d_qual=b.get("d_qual"), d_qual_off=b.get("d_qual_off"), svsig=True)
            for sig in sigs:
                sv_out.write(sig)
        elif sv_out:                                                        # one snapshot: the same from the host
            snap = mapper.snapshot(res, with_blocks=fmt == "a", svsig=True)
            texts = mapper.records_host(snap, mapper.record_args(b["names"], b["seqs"], b["quals"]), passthrough=tags, free=False)
            for sig in mapper.svsig_host(snap, b["names"]):
                sv_out.write(sig)
        elif args.device_records:
            texts = mapper.records_device(res, mapper.record_args(b["names"], b["seqs"], b["quals"], lens=b.get("read_len")), passthrough=tags,
                                          d_qual=b.get("d_qual"), d_qual_off=b.get("d_qual_off"))
        else:
            texts = mapper.records(res, b["names"], b["seqs"], quals=b["quals"], passthrough=tags)
        if args.bgzf and not args.device_records:                           # the host text, deflated on the device
            texts = [deflate.compress_device(ctx, b"".join(texts))[0]]
        for txt in texts:
            out.write(txt)
        t_rec += time.perf_counter() - t
        n_reads += len(b["names"]); n_bases += int(b["off"][-1]); n_batches += 1
        if failed:
            break
    rf.close()
    if sorter:
        write_run(True)
        sorter.close()
        if args.merge_runs and run_no > 1:
            merge_runs()
    elif args.bgzf or args.bam:
        out.write(bgzf.EOF_BLOCK)
    if sv_out:
        sv_out.close()
    if out and args.out:
        out.close()
    elif out:
        out.flush()
    sys.stderr.write("map_files: %d reads, %d bases, %d batches; genome + index %.2f s, %s %.2f s (%.1f Mbases/s), map %.2f s, records %.2f s\n"
                     % (n_reads, n_bases, n_batches, t_index, "read+parse (host)" if args.host_input else "read+parse (device)", t_read,
                        n_bases / max(t_read, 1e-9) / 1e6, t_map, t_rec))
    ctx.close()
    if failed:
        sys.stderr.write("map_files: %s\n" % failed)
        sys.exit(1)


if __name__ == "__main__":
    main()
