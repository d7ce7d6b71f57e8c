"""Shared by test_genome_input.py and test_genome_input_device.py: the Python restatement of the genome reader's rules (kseq_read's FASTA branch as
Genome::Read uses it, htslib 1.11) and the seeded corpora both test files read.  Not a test module."""
import gzip
import struct
import zlib

import numpy as np

SPACE = b" \t\n\v\f\r"


class Refused(Exception):
    """the two inputs the reader refuses: kind in ("plus", "cr"), record = its index"""

    def __init__(self, kind, record):
        Exception.__init__(self, kind, record)
        self.kind, self.record = kind, record


def parse_rules(data: bytes):
    """-> (names, chrom_pos, bases) under rules 1-8 of the issue; Refused for a '+' line in a record and for rule 4's lone "\\r" first line"""
    first = min((i for i in (data.find(b">"), data.find(b"@")) if i >= 0), default=-1)
    names, pos, out = [], [0], bytearray()
    if first < 0:
        return names, pos, bytes(out)
    lines = data[first:].split(b"\n")                       # rule 1: the byte opens the first header; rule 5: the last line needs no '\n'
    cur = None
    for k, line in enumerate(lines):
        if k == 0 or line[:1] in (b">", b"@"):              # rule 2
            if cur is not None:
                out += cur; pos.append(len(out))
            body = line[1:]
            e = next((i for i, c in enumerate(body) if c in SPACE), len(body))
            names.append(bytes(body[:e]))                   # rule 3
            cur = bytearray()
            continue
        if line[:1] == b"+":
            raise Refused("plus", len(names) - 1)           # rule 7
        if line == b"":
            continue                                        # rule 4: an empty line is skipped
        if line.endswith(b"\r"):
            if line == b"\r" and len(cur) == 0:
                raise Refused("cr", len(names) - 1)         # kseq would keep it (str->l > 1 fails): the port refuses
            line = line[:-1]
        cur += line.upper() if not any(c >= 0x80 for c in line) else bytes(c - 32 if 97 <= c <= 122 else c for c in line)   # rule 6, C locale
    out += cur; pos.append(len(out))
    return names, pos, bytes(out)


ALPHABETS = [b"ACGT", b"acgt", b"ACGTacgtNn", b"ACGTNRYKMSWBDHVacgtnrykmswbdhv"]


def corpus(seed, n_rec=None, eol=b"\n", width=None, plain=False, big=False):
    """a FASTA-like file from a seeded generator.  plain: only what read_genome() of tools/map_files.py reads the same way ('>' headers at line
    starts, no blanks in sequence lines, '\\n' line ends, no junk in front)."""
    r = np.random.default_rng(seed)
    if n_rec is None:
        n_rec = int(r.integers(1, 9))
    if width is None:
        width = int(r.choice([0, 1, 2, 7, 60, 61, 80, 200]))   # 0: unwrapped
    alpha = np.frombuffer(ALPHABETS[int(r.integers(0, len(ALPHABETS)))], np.uint8)
    out = bytearray()
    if not plain and r.random() < 0.4:
        out += [b"junk in front\n", b"# no header yet", b"\n\n  \t", b"x" * 37][int(r.integers(0, 4))]   # rule 1 (the 2nd and 4th: the header mid-line)
    empties = set(int(x) for x in r.choice(n_rec, size=min(n_rec, int(r.integers(0, 3))), replace=False)) if n_rec > 1 or r.random() < 0.2 else set()
    for i in range(n_rec):
        hc = b">" if plain or r.random() < 0.8 else b"@"
        name = b"" if (not plain and r.random() < 0.1) else b"chr%d_%d" % (i, int(r.integers(0, 1000)))
        tail = [b"", b" a comment", b"\tlen=12 x", b"  two  blanks ", b"\tAC>GT @x"][int(r.integers(0, 5))]
        if plain and not name:
            name = b"c%d" % i
        out += hc + name + tail + eol
        if i in empties:
            if r.random() < 0.5 and eol == b"\n":             # (an "empty" line that ends in "\r\n" would be a first line of "\r" alone: refused)
                out += eol
            continue
        L = int(r.integers(1, 3000)) if not big else int(r.integers(200_000, 400_000))
        seq = alpha[r.integers(0, len(alpha), size=L)].tobytes()
        if not plain:
            seq = bytearray(seq)
            for _ in range(int(r.integers(0, 4))):           # blanks, tabs, digits, '>' and '@' inside sequence lines: they stay
                seq[int(r.integers(0, L))] = b" \t7>@\r"[int(r.integers(0, 6))]
            seq = bytes(seq)
        w = width or L
        for a in range(0, L, w):
            line = seq[a:a + w]
            if not plain and line[:1] in (b">", b"@", b"+", b"\r"):
                line = b"A" + line[1:]                      # (a sequence line's first byte decides what the line is)
            out += line + eol
            if not plain and r.random() < 0.03:
                out += eol                                  # an empty line
    if r.random() < 0.3 and len(out) >= len(eol):
        del out[len(out) - len(eol):]                       # rule 5
    return bytes(out)


def fixed_cases():
    """name -> bytes: the edges the issue lists, spelled out"""
    return {
        "empty_file": b"",
        "junk_only": b"no record here\nnor here\n",
        "single": b">one\nACGT\n",
        "single_no_nl": b">one\nACGT",
        "header_only": b">one",
        "header_only_nl": b">one\n",
        "empty_name": b"> chr1 with the empty name\nAC\nGT\n",
        "at_headers": b"@r1 x\nACGT\n@r2\nTTTT\n",
        "mid_line_markers": b">a\nAC>GT\nAC@GT\nA+C\n",
        "junk_then_header_mid_line": b"xxxx>a b\nACGT\n>b\nAA\n",
        "junk_with_at": b"mail me@home\nACGT\n>b\nAA\n",
        "blanks_inside": b">a\nAC GT\tAC\n 12 \n",
        "crlf": b">a c\r\nACGT\r\nAC\r\n>b\r\nTT\r\n\r\nG\r\n",
        "cr_mid_line": b">a\nAC\rGT\r\r\nA\r",
        "lone_cr_later": b">a\nAC\n\r\nGT\n",
        "cr_at_end": b">a\nACGT\r",
        "empty_records": b">a\n>b\n\n>c\nAC\n>d\n>e",
        "empty_lines": b">a\n\n\nAC\n\nGT\n\n",
        "lower_mixed": b">a\nacgtnNrykm\xe9\xff\n",
        "unwrapped": b">a\n" + b"ACGT" * 5000 + b"\n>b\n" + b"TG" * 3000,
    }


def refused_cases():
    """name -> (bytes, kind, record index, the record's name)"""
    return {
        "plus_line": (b">a\nACGT\n>b x\nAC\n+\nIIII\n", "plus", 1, b"b"),
        "plus_first": (b"@r\nAC\n+r\nII\n", "plus", 0, b"r"),
        "lone_cr_first": (b">a\nAC\n>bb\n\r\nGT\n", "cr", 1, b"bb"),
        "lone_cr_after_empty": (b">a\n\n\r\nGT\n", "cr", 0, b"a"),
        "lone_cr_at_end": (b">a\nAC\n>b\n\r", "cr", 1, b"b"),
        "crlf_blank_line_first": (b">a\r\nAC\r\n>b\r\n\r\nTT\r\n", "cr", 1, b"b"),
    }


def gzip_variants(data: bytes):
    """name -> bytes: the gzip encodings the issue lists"""
    def raw(level, strategy=zlib.Z_DEFAULT_STRATEGY):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        return c.compress(data) + c.flush()

    def wrap(body, flg=0, extra=b""):
        return b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff" + extra + body + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data) & 0xffffffff)

    half = len(data) // 2
    return {
        "level1": gzip.compress(data, 1),
        "level6": gzip.compress(data, 6),
        "level9": gzip.compress(data, 9),
        "two_members": gzip.compress(data[:half], 6) + gzip.compress(data[half:], 9),
        "fname_fextra": wrap(raw(6), 4 | 8 | 16 | 2, struct.pack("<H", 5) + b"XY\x01\x00z" + b"genome.fa\0" + b"a comment\0" + b"\x12\x34"),
        "fixed": wrap(raw(6, zlib.Z_FIXED)),
        "stored": wrap(raw(0)),
    }


def repetitive(seed, size=1_400_000):
    """above 1 MiB of repetitive sequence in 60-base lines: DEFLATE distances reach across the 32 KiB window"""
    r = np.random.default_rng(seed)
    unit = np.frombuffer(b"ACGT", np.uint8)[r.integers(0, 4, size=31_000)].tobytes()
    seq = bytearray()
    while len(seq) < size:
        seq += unit
        seq += np.frombuffer(b"ACGTN", np.uint8)[r.integers(0, 5, size=int(r.integers(1, 300)))].tobytes()
    out = bytearray(b">rep1 repetitive\n")
    for a in range(0, len(seq), 60):
        out += seq[a:a + 60] + b"\n"
        if a == 60 * 9000:
            out += b">rep2\n"
    return bytes(out)
