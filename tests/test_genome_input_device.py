"""The genome reader's device form (lra_genome_read_device) against its host form on the corpora of tests/genome_cases.py -- names, chrom_pos, every
byte and the padding, at steps that put headers, "\\r\\n" pairs and the leading junk on step edges --, the index files built from an installed genome,
and the two tools as child processes."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genome_cases as gc   # noqa: E402

pytestmark = pytest.mark.gpu
STEPS = (None, 4096, 4099, 6007)


def read(path, ctx=None, chunk=None):
    from lra_amd.genome_io import GenomeFile
    g = GenomeFile(str(path), ctx=ctx, chunk=chunk).read()
    padded = g.padded.cpu().numpy() if ctx is not None else g.padded
    out = (g.names, g.chrom_pos, padded.tobytes())
    g.close()
    return out


def same_in_both_forms(ctx, path, data, steps=STEPS):
    names, pos, seq = gc.parse_rules(data)
    host = read(path)
    assert host == (names, pos, seq + bytes(64))
    for chunk in steps:
        dev = read(path, ctx, chunk)
        assert dev[0] == host[0], chunk
        assert dev[1] == host[1], chunk
        assert dev[2] == host[2], chunk


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return p


def encodings(data, seed=0):
    from lra_amd.bgzf import bgzf_compress
    r = np.random.default_rng(seed)
    return {"plain.fa": data, "gzip.fa.gz": gzip.compress(data, 6), "two.fa.gz": gc.gzip_variants(data)["two_members"],
            "bgzf.fa.gz": bgzf_compress(data), "bgzf_small.fa.gz": bgzf_compress(data, block=int(r.integers(500, 9000)), level=1, eof=bool(seed & 1))}


@pytest.mark.parametrize("name", sorted(gc.fixed_cases()))
def test_fixed_cases(ctx, tmp_path, name):
    data = gc.fixed_cases()[name]
    for fn, z in encodings(data).items():
        same_in_both_forms(ctx, write(tmp_path, fn, z), data)


@pytest.mark.parametrize("seed", range(12))
def test_random_corpora(ctx, tmp_path, seed):
    data = gc.corpus(seed, eol=b"\r\n" if seed % 3 == 1 else b"\n", n_rec=12)
    for fn, z in encodings(data, seed).items():
        same_in_both_forms(ctx, write(tmp_path, fn, z), data)


def test_record_several_steps_long(ctx, tmp_path):
    data = gc.corpus(50, n_rec=4, big=True, eol=b"\r\n") + b"\n" + gc.fixed_cases()["unwrapped"]
    data = b"junk " * 1000 + data                                # the leading junk is longer than a step
    for fn, z in encodings(data, 3).items():
        same_in_both_forms(ctx, write(tmp_path, fn, z), data, steps=(None, 4096, 6007, 100_003))


def test_gzip_across_window_and_steps(ctx, tmp_path):
    data = gc.repetitive(9)
    same_in_both_forms(ctx, write(tmp_path, "rep.fa.gz", gzip.compress(data, 9)), data, steps=(None, 4096, 70_001))


@pytest.mark.parametrize("name", sorted(gc.refused_cases()))
def test_refused_input_same_text(ctx, tmp_path, name):
    from lra_amd.genome_io import GenomeFile
    data = gc.refused_cases()[name][0]
    for fn, z in encodings(b"x\n" + data + (b"\n>z\nAC\n" if not data.endswith(b"\r") else b"")).items():
        p = write(tmp_path, fn, z)
        texts = []
        for c, chunk in ((None, None), (ctx, None), (ctx, 4096)):
            g = GenomeFile(str(p), ctx=c, chunk=chunk)
            with pytest.raises(IOError) as e:
                g.read()
            assert e.value.rc == -1
            texts.append(g.last_error())
            with pytest.raises(IOError):
                g.read()
            assert g.last_error() == texts[-1]
            g.close()
        assert texts[0] and texts[0] == texts[1] == texts[2]


def test_bad_members_same_text(ctx, tmp_path):
    from lra_amd.bgzf import bgzf_compress, blocks
    from lra_amd.genome_io import GenomeFile
    data = gc.corpus(60, n_rec=5, big=True)
    z = bgzf_compress(data, block=20000)
    in_off, _ = blocks(z)
    bad = bytearray(z); bad[in_off[len(in_off) // 2] + 30] ^= 0xff
    gz = gzip.compress(data, 6)
    flipped = bytearray(gz); flipped[len(gz) // 2] ^= 0x55
    for fn, blob in (("bad.fa.gz", bytes(bad)), ("cut.fa.gz", z[:in_off[3] + 50]), ("trunc.fa.gz", gz[:len(gz) // 2]), ("flip.fa.gz", bytes(flipped))):
        p = write(tmp_path, fn, blob)
        texts = []
        for c, chunk in ((None, None), (ctx, None), (ctx, 4096)):
            g = GenomeFile(str(p), ctx=c, chunk=chunk)
            with pytest.raises(IOError) as e:
                g.read()
            assert e.value.rc == -1
            texts.append(g.last_error())
            g.close()
        assert "compressed offset" in texts[0] and texts[0] == texts[1] == texts[2], (fn, texts)


def small_genome(tmp_path):
    from lra_amd import synth
    genome = synth.make_genome(300_000, seed=3, repeat_frac=0.2, n_families=2)
    s = genome.tobytes()
    data = (b">chr1 first\n" + b"\n".join(s[x:x + 70] for x in range(0, 200_000, 70)) + b"\n>chr2\n" +
            b"\n".join(s[x:x + 70] for x in range(200_000, len(s), 70)) + b"\n")
    return genome, data, write(tmp_path, "genome.fa", data)


def test_install_builds_the_same_index_files(ctx, tmp_path):
    """install + build_global_index + lra_ctx_build_local_index == the same build on lra_ctx_load_genome of the Python-parsed bytes"""
    import ctypes as C
    from lra_amd import index
    from lra_amd.genome_io import GenomeFile
    _, data, path = small_genome(tmp_path)
    names, pos, seq = gc.parse_rules(data)

    def build(tag):
        st = index.build_global_index(ctx, pos, *index.INDEX_PRESETS["ont"])
        key, p = index.global_index(ctx)
        index.write_mms(tmp_path / (tag + ".mms"), 17, names, pos, key, p)
        ctx.check(ctx.lib.lra_ctx_build_local_index(ctx.h, 10, 5, 2048, 15))
        li = index.local_index(ctx)
        index.write_gli(tmp_path / (tag + ".gli"), li["k"], li["w"], li["window"], li["seq_offsets"], li["tuple_bnd"], li["tuples"])
        assert st["n_index"] > 0 and (li["k"], li["w"], li["window"]) == (10, 5, 2048) and len(li["tuples"]) > 0
        return (tmp_path / (tag + ".mms")).read_bytes(), (tmp_path / (tag + ".gli")).read_bytes()

    index.load_genome(ctx, np.frombuffer(seq, np.uint8))
    cp = (C.c_uint64 * len(pos))(*pos)
    ctx.check(ctx.lib.lra_ctx_load_chromosomes(ctx.h, cp, len(pos) - 1))
    want = build("python")
    for tag, c in (("device", ctx), ("host", None)):
        g = GenomeFile(str(path), ctx=c, chunk=4099 if c else None).read()
        assert g.names == names and g.chrom_pos == pos
        g.install(ctx)
        g.close()
        assert build(tag) == want


def test_install_refuses_a_genome_without_records(ctx, tmp_path):
    from lra_amd._lib import LraError
    from lra_amd.genome_io import GenomeFile
    g = GenomeFile(str(write(tmp_path, "junk.fa", b"nothing here\n")), ctx=ctx).read()
    assert g.names == [] and g.chrom_pos == [0] and g.padded.cpu().numpy().tobytes() == bytes(64)
    with pytest.raises(LraError):
        g.install(ctx)
    g.close()


def run_tool(tool, *args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), *[str(a) for a in args]], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p


def test_index_files_tool(tmp_path):
    """tools/index_files.py on genome.fa, its gzip copy and its bgzip copy: identical index files, and lra_read_mms / lra_read_gli read them back"""
    from lra_amd import index
    from lra_amd.bgzf import bgzf_compress
    _, data, path = small_genome(tmp_path)
    os.makedirs(tmp_path / "gz"); os.makedirs(tmp_path / "bgzf")
    gz = write(tmp_path / "gz", "genome.fa.gz", gzip.compress(data, 6))
    bg = write(tmp_path / "bgzf", "genome.fa.gz", bgzf_compress(data))
    outs = []
    for f, extra in ((path, []), (gz, []), (bg, ["--chunk", "8192"])):
        p = run_tool("index_files.py", "-ONT", f, *extra)
        assert b"read+parse (device)" in p.stderr
        outs.append((open(str(f) + ".mms", "rb").read(), open(str(f) + ".gli", "rb").read()))
    assert outs[0] == outs[1] == outs[2]
    m = index.read_mms(str(path) + ".mms")
    names, pos, _ = gc.parse_rules(data)
    assert m["globalK"] == 17 and m["names"] == names and [int(x) for x in m["chrom_pos"]] == pos and len(m["key"]) > 0
    g = index.read_gli(str(path) + ".gli")
    assert (g["k"], g["w"], g["window"]) == (10, 5, 2048) and len(g["tuples"]) > 0
    run_tool("index_files.py", "-CLR", path, "-K", "13", "-k", "8", "--localIndexWindow", "1024")
    assert index.read_mms(str(path) + ".mms")["globalK"] == 13
    g = index.read_gli(str(path) + ".gli")
    assert (g["k"], g["w"], g["window"]) == (8, 5, 1024)


def test_map_files_tool_reads_compressed_genomes(tmp_path):
    """tools/map_files.py on genome.fa and genome.fa.gz (and with --host-genome): the same SAM records, the @PG line aside"""
    from lra_amd import synth
    genome, data, path = small_genome(tmp_path)
    gz = write(tmp_path, "genome.fa.gz", gzip.compress(data, 6))
    reads, _ = synth.simulate_reads(genome, 30, 5000, 1500, 0.08, seed=11)
    fq = write(tmp_path, "r.fq", b"".join(b"@m%d\n%s\n+\n%s\n" % (i, r.tobytes(), b"5" * len(r)) for i, r in enumerate(reads)))
    outs = []
    for k, (g, extra) in enumerate(((path, []), (gz, []), (path, ["--host-genome"]))):
        o = tmp_path / ("out%d.sam" % k)
        run_tool("map_files.py", "-ONT", g, fq, "-o", o, "--batch-bases", "40000", *extra)
        outs.append([l for l in o.read_bytes().split(b"\n") if not l.startswith(b"@PG")])
    assert outs[0] == outs[1] == outs[2]
    assert len({l.split(b"\t")[0] for l in outs[0] if l and not l.startswith(b"@")}) == 30
