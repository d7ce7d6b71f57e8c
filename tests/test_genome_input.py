"""The genome reader's host form (lra_genome_read_host) against the Python restatement of its rules (tests/genome_cases.py): names, chrom_pos and
every byte, for plain, gzip and BGZF input; the inputs it refuses; the ABI.  No GPU."""
import gzip
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genome_cases as gc   # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from lra_amd._lib import load_library
    return load_library()


def read_host(path, chunk=None):
    from lra_amd.genome_io import GenomeFile
    g = GenomeFile(str(path), chunk=chunk).read()
    out = (g.names, g.chrom_pos, g.seq.tobytes(), g.padded[len(g.seq):].tobytes())
    g.close()
    return out


def check(path, data, chunk=None):
    names, pos, seq = gc.parse_rules(data)
    got = read_host(path, chunk)
    assert got[0] == names
    assert got[1] == pos
    assert got[2] == seq
    assert got[3] == bytes(64)


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return p


def map_files_module():
    spec = importlib.util.spec_from_file_location("map_files_tool", os.path.join(ROOT, "tools", "map_files.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("name", sorted(gc.fixed_cases()))
def test_fixed_cases(lib, tmp_path, name):
    data = gc.fixed_cases()[name]
    check(write(tmp_path, "g.fa", data), data)
    check(write(tmp_path, "g2.fa", data), data, chunk=4096)


@pytest.mark.parametrize("seed", range(24))
def test_random_corpora(lib, tmp_path, seed):
    eol = b"\r\n" if seed % 3 == 1 else b"\n"
    data = gc.corpus(seed, eol=eol)
    check(write(tmp_path, "g.fa", data), data)
    check(write(tmp_path, "g2.fa", data), data, chunk=4096 + seed)


@pytest.mark.parametrize("seed", range(8))
def test_ordinary_fasta_equals_read_genome(lib, tmp_path, seed):
    data = gc.corpus(100 + seed, plain=True)
    p = write(tmp_path, "g.fa", data)
    check(p, data)
    names, pos, seq = map_files_module().read_genome(str(p))
    got = read_host(p)
    assert got[0] == names and got[1] == pos and got[2] == seq.tobytes()


@pytest.mark.parametrize("seed", range(4))
def test_gzip_variants(lib, tmp_path, seed):
    data = gc.corpus(200 + seed, n_rec=6, eol=b"\r\n" if seed == 1 else b"\n")
    for name, z in gc.gzip_variants(data).items():
        assert gzip.decompress(z) == data, name
        p = write(tmp_path, name + ".fa.gz", z)
        check(p, data)
        check(p, data, chunk=4096 + 7 * seed)


def test_gzip_distances_across_window_and_steps(lib, tmp_path):
    data = gc.repetitive(7)
    assert len(data) > (1 << 20)
    for name, z in gc.gzip_variants(data).items():
        if name == "level1":
            continue
        p = write(tmp_path, name + ".fa.gz", z)
        check(p, data, chunk=4096 if name in ("level9", "two_members") else 50_000)
    check(write(tmp_path, "default_step.fa.gz", gzip.compress(data, 6)), data)


@pytest.mark.parametrize("seed", range(4))
def test_bgzf(lib, tmp_path, seed):
    from lra_amd.bgzf import bgzf_compress
    data = gc.corpus(300 + seed, n_rec=5, big=seed == 0)
    r = np.random.default_rng(seed)
    cuts = sorted(set(int(x) for x in r.integers(1, max(2, len(data)), size=12)))
    cuts = [c for a, c in zip([0] + cuts, cuts) if c - a <= 60000]
    if len(data) - (cuts[-1] if cuts else 0) > 60000 or (cuts and cuts[0] > 60000):
        cuts = list(range(50000, len(data), 50000)) + [len(data) - 1]
        cuts = sorted(set(c for c in cuts if 0 < c < len(data)))
    check(write(tmp_path, "default.fa.gz", bgzf_compress(data)), data)
    check(write(tmp_path, "cuts.fa.gz", bgzf_compress(data, cuts=cuts, eof=False)), data)
    check(write(tmp_path, "small.fa.gz", bgzf_compress(data, block=997, level=1)), data, chunk=4096)


def expect_invalid(path, chunk=None):
    from lra_amd.genome_io import GenomeFile
    g = GenomeFile(str(path), chunk=chunk)
    with pytest.raises(IOError) as e:
        g.read()
    assert e.value.rc == -1                                    # LRA_ERR_INVALID
    text = g.last_error()
    assert text and str(path) in text
    with pytest.raises(IOError) as e2:                         # sticky
        g.read()
    assert e2.value.rc == -1 and g.last_error() == text
    assert g.lib.lra_genome_info(g.h, None, None, None) == -1
    g.close()
    return text


@pytest.mark.parametrize("name", sorted(gc.refused_cases()))
def test_refused_input(lib, tmp_path, name):
    data, kind, idx, rname = gc.refused_cases()[name]
    with pytest.raises(gc.Refused) as e:
        gc.parse_rules(data)
    assert (e.value.kind, e.value.record) == (kind, idx)
    for chunk in (None, 4096):
        text = expect_invalid(write(tmp_path, "g.fa", data), chunk)
        assert "record %d ('%s')" % (idx, rname.decode()) in text
        assert ("FASTQ" in text) == (kind == "plus") and ("\\r" in text) == (kind == "cr")
    text = expect_invalid(write(tmp_path, "g.fa.gz", gzip.compress(data)))
    assert "record %d " % idx in text


def test_bad_gzip(lib, tmp_path):
    data = gc.corpus(400, n_rec=6)
    z = gzip.compress(data, 6)
    text = expect_invalid(write(tmp_path, "truncated.fa.gz", z[:len(z) // 2]))
    assert "compressed offset 0" in text and "ends inside" in text
    bad = bytearray(z); bad[len(z) // 2] ^= 0x55
    text = expect_invalid(write(tmp_path, "flipped.fa.gz", bytes(bad)), chunk=4096)
    assert "compressed offset 0" in text
    bad = bytearray(z); bad[-4] ^= 1
    text = expect_invalid(write(tmp_path, "isize.fa.gz", bytes(bad)))
    assert "compressed offset 0" in text and "ISIZE" in text
    z2 = gzip.compress(data[:1000]) + z[:len(z) - 9]           # the second member is cut
    text = expect_invalid(write(tmp_path, "second.fa.gz", z2))
    assert "compressed offset %d" % len(gzip.compress(data[:1000])) in text
    text = expect_invalid(write(tmp_path, "garbage.fa.gz", z + b"garbage"))
    assert "compressed offset %d" % len(z) in text


def test_bad_bgzf_member_in_the_middle(lib, tmp_path):
    from lra_amd.bgzf import bgzf_compress, blocks
    data = gc.corpus(401, n_rec=4, big=True)
    z = bgzf_compress(data, block=20000)
    in_off, _ = blocks(z)
    k = len(in_off) // 2
    bad = bytearray(z); bad[in_off[k] + 30] ^= 0xff
    for chunk in (None, 4096):
        text = expect_invalid(write(tmp_path, "bad.fa.gz", bytes(bad)), chunk)
        assert "compressed offset %d" % in_off[k] in text
    text = expect_invalid(write(tmp_path, "cut.fa.gz", z[:in_off[k] + 100]))
    assert "compressed offset %d" % in_off[k] in text and "ends inside" in text


def test_first_fault_in_file_order(lib, tmp_path):
    """a '+' line in front of a bad member is the fault reported; behind it, the member is"""
    from lra_amd.bgzf import bgzf_compress, blocks
    body = b">a\nACGT\n+\nIIII\n" + gc.corpus(402, n_rec=3, plain=True, big=True)
    z = bgzf_compress(body, block=30000)
    in_off, _ = blocks(z)
    bad = bytearray(z); bad[in_off[2] + 40] ^= 0xff
    assert "FASTQ" in expect_invalid(write(tmp_path, "a.fa.gz", bytes(bad)))
    body = gc.corpus(402, n_rec=3, plain=True, big=True) + b"+\n"
    z = bgzf_compress(body, block=30000)
    bad = bytearray(z); bad[in_off[2] + 40] ^= 0xff
    assert "compressed offset" in expect_invalid(write(tmp_path, "b.fa.gz", bytes(bad)))


def test_abi_and_forms(lib, tmp_path):
    import ctypes as C
    assert lib.lra_abi_version() == 9
    for n in ("open", "read_host", "read_device", "info", "names", "host_seq", "device_seq", "install", "last_error", "set_device_chunk", "close"):
        assert hasattr(lib, "lra_genome_" + n)
    h = C.c_void_p()
    assert lib.lra_genome_open(str(tmp_path / "absent.fa").encode(), C.byref(h)) == -1 and not h
    p = write(tmp_path, "g.fa", b">a\nAC\n")
    assert lib.lra_genome_open(str(p).encode(), C.byref(h)) == 0
    assert lib.lra_genome_set_device_chunk(h, 4095) == -1 and lib.lra_genome_set_device_chunk(h, 4096) == 0
    assert lib.lra_genome_info(h, None, None, None) == -1      # not read yet
    assert lib.lra_genome_read_host(h) == 0 and lib.lra_genome_read_host(h) == 0
    assert lib.lra_genome_set_device_chunk(h, 8192) == -1      # only before the read
    assert lib.lra_genome_read_device(h, None) == -1
    assert lib.lra_genome_host_seq(h) and not lib.lra_genome_device_seq(h)
    lib.lra_genome_close(h)


def test_no_records_is_ok_and_install_refuses(lib, tmp_path):
    names, pos, seq, pad = read_host(write(tmp_path, "junk.fa", b"nothing\nhere\n"))
    assert names == [] and pos == [0] and seq == b"" and pad == bytes(64)
