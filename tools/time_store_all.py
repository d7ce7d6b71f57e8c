"""What lra align -a (lra_ctx_set_store_all: the read sketched with w = 1) costs, on bench-shaped inputs: the synthetic GRCh38-like reference with its N gaps
(lra_amd/synth_genome.py, scaled), -ONT reads of 30 kb, and -CCS reads of 15 kb.  Three comparisons, each alternated in one process, --reps rounds:
  seed    the seed stage a1-a4 at w = 1 (lra_seed_batch): this tree's position-parallel sketch against --parent-lib's (a liblra_hip.so built from the commit
          before the w = 1 path: the window machine, and for reads with N the lane-per-read kernel), and this tree at w = globalW for scale
  ont     the one-call low-accuracy step (lra_map_reads_lowacc_batch) with and without -a
  ccs     a -CCS batch (lra_map_reads_highacc_batch) with and without -a
One JSON line: per comparison the wall ms of every round and their median, the seed stage's kernel times (lra_ctx_timing_get), the counters (tuples, matches,
n_flagged_reads), the reads whose tuple list has a repeated key (the exact sort takes those), and the device memory in use after each step (the library's work
buffers are kept from call to call: what the largest step needed).  Size --reads so that it fits: at w = 1 the tuple and match arrays are ~5x those at w = 10.
For the kernels of one -a step run it under `rocprofv3 --kernel-trace --stats` with --only ont_a --reps 1 (two -a steps: the first grows the buffers)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED_KERNELS = ("sketch_all_count", "sketch_all_emit", "sketch_emit", "sketch_serial", "sketch_compact", "sort", "sort_fallback", "index_bounds", "compare", "strand")


def parent_context(path, device):
    """A context of the library at `path` (another build of liblra_hip.so, loaded beside this tree's in the same process and the same HIP runtime)."""
    from lra_amd._lib import SYMBOLS
    from lra_amd.context import Context
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res; fn.argtypes = args
    c = Context.__new__(Context)
    c.lib = lib
    import torch
    c.device = torch.device("cuda", device)
    h = C.c_void_p()
    if lib.lra_ctx_create(device, C.byref(h)):
        raise RuntimeError("parent library: lra_ctx_create failed")
    c.h = h
    c.bind_stream()
    return c


def used_gb():
    import torch
    free, total = torch.cuda.mem_get_info()
    return round((total - free) / 1e9, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-scale", type=float, default=0.25, help="1.0 = GRCh38-sized (3.09 Gb)")
    ap.add_argument("--reads", type=int, default=4096, help="-ONT reads of the seed and ont comparisons")
    ap.add_argument("--read-len", type=int, default=30000)
    ap.add_argument("--ccs-reads", type=int, default=2048)
    ap.add_argument("--ccs-len", type=int, default=15000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default="", help="liblra_hip.so of the parent commit (seed comparison); without it the parent's leg is left out")
    ap.add_argument("--only", choices=["seed", "ont", "ont_a", "ccs"], default=None, help="ont_a: the -a leg of ont alone (for a profiler's kernel table)")
    args = ap.parse_args()
    import torch
    from lra_amd.context import Context
    from lra_amd import seed, mapread, index as I, synth_genome as sg
    dev = 0
    out = dict(genome_scale=args.genome_scale, reads=args.reads, read_len=args.read_len, reps=args.reps)
    sync = lambda: torch.cuda.synchronize()
    with torch.no_grad():
        torch.use_deterministic_algorithms(True, warn_only=True)
        genome, chrom_pos, chrom_names = sg.make_grch38_like("cuda:0", scale=args.genome_scale, seed=3)
        sim = sg.simulate_reads_sv(genome, chrom_pos, args.reads, args.read_len, args.read_len / 10, 0.10, (30, 35, 35), 1000)
        torch.use_deterministic_algorithms(False)
    out["genome_bases"] = int(genome.numel())
    off_h = sim["off"].cpu().numpy()
    out["read_bases"] = int(off_h[-1])
    o = mapread.LowAccOptions(localIndexWindow=2048)
    ctx = Context(dev)
    plain = mapread.LowAccMapper(ctx, genome, None, None, chrom_names, chrom_pos, o, index_params=(o.globalK, o.globalW, o.globalMaxFreq, 15, 1), staged=False)
    rbatch = seed.read_batch_from_device(ctx, sim["seq"], sim["off"])

    def timed(fn):
        sync(); t0 = time.perf_counter(); r = fn(); sync()
        return (time.perf_counter() - t0) * 1e3, r

    if args.only in (None, "seed"):
        ik, ipos = I.global_index(ctx)
        seeders = [("new_w1", ctx, 1), ("w%d" % o.globalW, ctx, o.globalW)]
        if args.parent_lib:
            pc = parent_context(args.parent_lib, dev)
            gh = genome.cpu().numpy()
            pc.check(pc.lib.lra_ctx_load_genome(pc.h, C.c_void_p(gh.ctypes.data), C.c_uint64(len(gh))))
            k_ = np.ascontiguousarray(ik).view(np.uint64); p_ = np.ascontiguousarray(ipos, dtype=np.uint32)
            pc.check(pc.lib.lra_ctx_load_global_index(pc.h, C.c_void_p(k_.ctypes.data), C.c_void_p(p_.ctypes.data), C.c_uint64(len(k_))))
            del gh
            seeders.insert(1, ("parent_w1", pc, 1))
        res = {}
        for name, c, _ in seeders:
            c.timing(True)
        for rep in range(args.reps + 1):                                  # (round 0 grows the buffers: not counted)
            for name, c, w in seeders:
                c.timing_reset()
                ms, sr = timed(lambda: seed.seed_batch(c, rbatch, o.globalK, w, o.globalMaxFreq))
                d = res.setdefault(name, dict(ms=[], kernels_ms={}))
                if rep == 0:
                    d.update(n_minimizers=int(sr.n_minimizers), n_matches=int(sr.n_matches))
                    mo = c.to_host(sr.d_mm_off, rbatch.n + 1, np.uint64)
                    if name != "w%d" % o.globalW:
                        keys = c.to_host(sr.d_mm_key, int(sr.n_minimizers), np.uint64) & np.uint64((1 << 63) - 1)
                        eq = np.zeros(len(keys), bool)
                        eq[1:] = keys[1:] == keys[:-1]
                        eq[mo[1:-1].astype(np.int64)[mo[1:-1] < len(keys)]] = False      # (a read's first tuple is not a repeat of the read before)
                        d["reads_with_repeated_key"] = int(len(np.unique(np.searchsorted(mo.astype(np.int64), np.nonzero(eq)[0], side="right"))))
                        d["mm_checksum"] = int(np.bitwise_xor.reduce(keys)) if len(keys) else 0
                    continue
                d["ms"].append(round(ms, 1))
                for kn in SEED_KERNELS:
                    t, n = c.timing_get(kn)
                    if n:
                        d["kernels_ms"].setdefault(kn, []).append(round(t, 2))
        for name, d in res.items():
            d["median_ms"] = float(np.median(d["ms"]))
            d["kernels_ms"] = {k: float(np.median(v)) for k, v in d["kernels_ms"].items()}
        if "parent_w1" in res:
            res["same_tuples_as_parent"] = res["parent_w1"]["mm_checksum"] == res["new_w1"]["mm_checksum"] and \
                res["parent_w1"]["n_matches"] == res["new_w1"]["n_matches"]
        out["seed"] = res
        for _, c, _ in seeders:
            c.timing(False)
        out["device_used_gb_after_seed"] = used_gb()

    if args.only in (None, "ont", "ont_a"):
        import copy
        import dataclasses
        ra = copy.copy(plain)                                              # (the same context: align() sets the switch from the mapper's options every call)
        ra.opts = dataclasses.replace(o, storeAll=True)
        res = {}
        for rep in range(args.reps + 1):
            for name, m in (("plain", plain), ("store_all", ra))[1 if args.only == "ont_a" else 0:]:
                ms, r = timed(lambda: m.align(rbatch))
                d = res.setdefault(name, dict(ms=[]))
                if rep == 0:
                    d.update({k: int(m.stats[k]) for k in ("n_minimizers", "n_matches", "n_clusters", "n_sdp_anchors", "n_flagged_reads", "n_alignments")})
                    d["device_used_gb_after"] = used_gb()
                    continue
                d["ms"].append(round(ms, 1))
        for d in res.values():
            d["median_ms"] = float(np.median(d["ms"]))
            d["gbps"] = round(out["read_bases"] / (d["median_ms"] * 1e-3) / 1e9, 3)
        out["ont"] = res

    if args.only in (None, "ccs"):
        del plain
        with torch.no_grad():
            torch.use_deterministic_algorithms(True, warn_only=True)
            cs = sg.simulate_reads_sv(genome, chrom_pos, args.ccs_reads, args.ccs_len, args.ccs_len / 10, 0.01, (34, 33, 33), 2000)
            torch.use_deterministic_algorithms(False)
        cctx = Context(dev)
        hp = mapread.HighAccMapper(cctx, genome, None, None, chrom_names, chrom_pos, "ccs", index_params=(17, 10, 150, 15, 1), gli=True)
        cb = seed.read_batch_from_device(cctx, cs["seq"], cs["off"])
        res = {}
        for rep in range(args.reps + 1):
            for name, on in (("plain", False), ("store_all", True)):
                hp.storeAll = on
                ms, r = timed(lambda: hp.align(cb))
                d = res.setdefault(name, dict(ms=[]))
                if rep == 0:
                    d.update({k: int(hp.stats[k]) for k in ("n_minimizers", "n_matches", "n_clusters", "n_flagged_reads", "n_alignments")})
                    d["device_used_gb_after"] = used_gb()
                    continue
                d["ms"].append(round(ms, 1))
        for d in res.values():
            d["median_ms"] = float(np.median(d["ms"]))
        out["ccs"] = dict(res, reads=args.ccs_reads, read_len=args.ccs_len, read_bases=int(cs["off"][-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
