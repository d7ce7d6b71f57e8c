#!/usr/bin/env python
"""Golden vectors for tests/svcombine_ref.py's column rule from the REFERENCE's own awk: the programs of the rules Homcalls and Hetcalls in
call_assembly_SVs/callassemblysv.snakefile and combinehapSV.snakefile, read out of the rule text when this runs (the shell block is a Python string and a
snakemake format: its escapes are resolved and its doubled braces undoubled) and run by awk on crafted .merge.vcf rows of eleven columns.  Writes
tests/golden/svcombine_awk_golden.json -- the rows and what awk printed; none of the programs' text.

    python tools/make_golden_svcombine.py [REFERENCE_CHECKOUT]          (default: $REF, else /root/reference, as oracle/Makefile)"""
import codecs
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF", "/root/reference")

ROWS = [
    "chr1\t100\t160\taligner.DEL.maternal.1\tACGTA\tA\t60\tPASS\tSVTYPE=DEL;SVLEN=-60;QNAME=ctg1;QSTART=812;QSTRAND=+\tGT\t1/1",
    "chr1\t5000\t5050\taligner.INS.paternal.7\tC\tCGGTA\t60\tPASS\tSVTYPE=INS;SVLEN=50;QNAME=tig=0001;x;QSTART=3;QSTRAND=-\tGT\t1/1",   # an INFO that holds ; and = of its own
    "chrUn_KI270442v1\t0\t41\tlra.DEL.maternal.1234567\tN\tN\t60\tPASS\tSVTYPE=DEL;SVLEN=-41;QNAME=a/b:c|d;QSTART=1;QSTRAND=+\tGT\t1/1",
    "2\t99999999\t100000040\taligner.INS.maternal.2\tT\tTA\t60\tPASS\tSVTYPE=INS;SVLEN=41;QNAME=q;QSTART=4000000000;QSTRAND=+\tGT\t1/1",
]


def awk_programs(snakefile, rule):
    """the awk programs of the rule's shell block, in order, as the shell hands them to awk"""
    text = open(os.path.join(REF, "call_assembly_SVs", snakefile)).read()
    body = re.search(r"^rule %s:.*?shell:\"\"\"(.*?)\"\"\"" % rule, text, re.S | re.M).group(1)
    body = codecs.decode(body, "unicode_escape").replace("{{", "{").replace("}}", "}")
    return re.findall(r"awk '([^']*)'", body)


gold = {"source": "the awk programs of the rules Homcalls and Hetcalls of the reference's two call_assembly_SVs snakefiles, run by tools/make_golden_svcombine.py",
        "rows": ROWS, "cases": []}
for snakefile, n_want in (("callassemblysv.snakefile", 3), ("combinehapSV.snakefile", 3)):
    n = 0
    for rule in ("Homcalls", "Hetcalls"):
        for k, prog in enumerate(awk_programs(snakefile, rule)):
            out = subprocess.run(["awk", prog], input="".join(r + "\n" for r in ROWS), capture_output=True, text=True, check=True).stdout
            gold["cases"].append({"snakefile": snakefile, "rule": rule, "program": k, "printed": out.splitlines()})
            n += 1
    assert n == n_want, (snakefile, n)
with open(os.path.join(ROOT, "tests", "golden", "svcombine_awk_golden.json"), "w") as f:
    json.dump(gold, f, indent=0)
print(len(gold["cases"]), "programs,", len(ROWS), "rows each")
