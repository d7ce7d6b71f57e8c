"""The record stage with SV signatures, from the host snapshot and on the device: the batch of tools/time_svsig.py (-ONT, 4096 reads x 20 kb, an indel planted in
every --plant-every'th read) mapped once, then per --svsig-len value, --reps times each, alternating:
  host           snapshot(LRA_PACK_SVSIG) + lra_map_records_host + lra_map_svsig_host
  device         lra_map_records_device with LRA_PACK_SVSIG (when the library has lra_map_records_device_svsig)
  device_noflag  lra_map_records_device with no flag
One JSON line: per form the wall ms and the host CPU ms (all threads) of every repetition, the bytes that crossed to the host, the text's bytes.  Runs
unchanged on a build without the device form (it then reports `host` and `device_noflag` only), which is how two commits are compared.  For the kernels' own
time run it under `rocprofv3 --kernel-trace --stats` (kernels svt_count, svt_head, svt_copy)."""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--read-len", type=int, default=20000)
    ap.add_argument("--genome", type=int, default=40_000_000, help="reference length (bases)")
    ap.add_argument("--plant-every", type=int, default=4)
    ap.add_argument("--svsig-len", type=int, nargs="+", default=[25, 1])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--forms", nargs="+", default=["host", "device", "device_noflag"])
    args = ap.parse_args()
    import torch
    from lra_amd.context import Context
    from lra_amd import seed, mapread, synth, parallel
    ctx = Context(0)
    lib = ctx.lib
    has_device = hasattr(lib, "lra_map_records_device_svsig")
    G = args.genome
    genome = synth.make_genome(G, seed=11, repeat_frac=0.05, n_families=4)
    CH = [0, G // 2, G]
    reads, _ = synth.simulate_reads(genome, args.reads, args.read_len, 5000, 0.10, (30, 35, 35), seed=3)
    rng = np.random.default_rng(8)
    for n, i in enumerate(range(0, len(reads), max(1, args.plant_every))):  # as tools/time_svsig.py plants them
        r = reads[i]
        at = int(rng.integers(len(r) // 3, 2 * len(r) // 3)); size = int(rng.integers(40, 301))
        reads[i] = np.concatenate([r[:at], r[at + size:]]) if n % 2 else np.concatenate([r[:at], synth.BASES[rng.integers(0, 4, size)], r[at:]])
    reads = [np.ascontiguousarray(r).tobytes() for r in reads]
    o = mapread.LowAccOptions()
    ik, ip = synth.build_global_index(genome, o.globalK, o.globalW, o.globalMaxFreq)
    mapper = mapread.LowAccMapper(ctx, genome, ik, ip, [b"chr1", b"chr2"], CH, o)
    res = mapper.align(seed.ReadBatch(ctx, reads))
    torch.cuda.synchronize()
    n = len(reads)
    rnames = [b"read%d" % i for i in range(n)]
    rargs = mapper.record_args(rnames, reads)
    a_names = (C.c_char_p * n)(*rnames); a_chr = (C.c_char_p * len(mapper.chrom_names))(*mapper.chrom_names)
    out = dict(reads=n, bases=int(sum(len(r) for r in reads)), alignments=int(res.n_alignments), blocks=int(res.n_blocks), device_form=has_device, lengths={})

    def host():
        snap = mapper.snapshot(res, md=False, svsig=True)
        rec = mapper.records_host(snap, rargs, free=False, as_list=False)
        ln = C.c_uint64(0)
        assert lib.lra_map_svsig_host(snap, a_names, a_chr, 0, None, C.byref(ln), None) == 0
        lib.lra_map_host_free(snap)
        return rec, int(ln.value)

    def device():
        return mapper.records_device(res, rargs, md=False, as_list=False, svsig=True)

    def device_noflag():
        return mapper.records_device(res, rargs, md=False, as_list=False), 0

    forms = [(k, f) for k, f in (("host", host), ("device", device), ("device_noflag", device_noflag)) if k in args.forms and (k != "device" or has_device)]
    for L in args.svsig_len:
        mapper.opts = dataclasses.replace(mapper.opts, svsigLen=L)
        mapread.set_svsig_len(ctx, L)
        rep = {k: dict(wall_ms=[], cpu_ms=[]) for k, _ in forms}
        for k, f in forms:                                                  # (once unmeasured: the kept buffers grow to their size)
            f()
        for _ in range(args.reps):
            for k, f in forms:                                              # the forms alternate inside a repetition
                c0 = time.process_time(); t0 = time.perf_counter()
                rec, sig = f()
                rep[k]["wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 2)); rep[k]["cpu_ms"].append(round((time.process_time() - c0) * 1e3, 2))
                rep[k]["record_bytes"], rep[k]["signature_bytes"] = rec, sig
                if k.startswith("device"):
                    st = mapper.records_device_stats()
                    rep[k]["bytes_to_host"] = int(st["bytes_d2h"]) + int(st.get("svsig_bytes_d2h", 0))
                    rep[k]["ms_svsig"] = round(st.get("ms_svsig", 0.0), 3)
        if "host" in rep:
            rep["host"]["bytes_to_host"] = len(parallel.pack_records(ctx, res, svsig=True, svsig_len=L))
        for k in rep:
            rep[k]["wall_ms_median"] = float(np.median(rep[k]["wall_ms"])); rep[k]["cpu_ms_median"] = float(np.median(rep[k]["cpu_ms"]))
        out["lengths"][str(L)] = rep
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
