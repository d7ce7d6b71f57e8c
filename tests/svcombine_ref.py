"""The two-haplotype oracle: the rules Homcalls, Hetcalls and combineHet of the reference's call_assembly_SVs/callassemblysv.snakefile as plain Python over
svcalls_ref.calls() -- bedtools intersect -f F -r with -u and -v, the awk that picks the columns, the cat.  Input is the two haplotypes' merged tables as
svcalls_ref gives them; output the six classes in delivery order.  The partner test is the brute-force form over all pairs."""
import svcalls_ref as sr

ORDER = (("maternal", "INS", "het"), ("maternal", "DEL", "het"), ("paternal", "INS", "het"), ("paternal", "DEL", "het"), ("maternal", "INS", "hom"),
         ("maternal", "DEL", "hom"))                                             # combineHet's cat: expand() puts hap outside and SVTYPE inside, the het files first


def partner(a, b, num=3, den=10):
    """rows (ref, start, end), half-open, of one kind: bedtools intersect -f num/den -r -- the overlap is at least the fraction of both rows, in integers"""
    ov = min(a[2], b[2]) - max(a[1], b[1])
    return a[0] == b[0] and ov > 0 and den * ov >= num * (a[2] - a[1]) and den * ov >= num * (b[2] - b[1])


def partnered(A, B, num=3, den=10):
    """[has row a of A a partner in B?], all pairs"""
    return [any(partner(a, b, num, den) for b in B) for a in A]


def columns(line, filter_pass=False):
    """the snakefiles' awk over a .merge.vcf line of eleven columns (bytes, no newline): print $1,$2,$4,$5,$6,$7,$9,$9,$10,$11 -- the FILTER column carries
    INFO a second time -- or, in combinehapSV.snakefile, $1,$2,$4,$5,$6,$7,"PASS",$9,$10,$11; OFS a tab"""
    f = line.split(b"\t")
    return b"\t".join([f[0], f[1], f[3], f[4], f[5], f[6], b"PASS" if filter_pass else f[8], f[8], f[9], f[10]])


def combine(calls_m, calls_p, num=3, den=10, filter_pass=False, one_based=False):
    """calls_m, calls_p: svcalls_ref.calls() of the maternal and the paternal file (hap b"maternal" / b"paternal") ->
    ([(hap, kind, cls, text, rows)] for the classes that have rows, in delivery order; stats).  rows: svcalls_ref's tuples + (hap 0 / 1, cls 0 het / 1 hom)"""
    tables = {"maternal": calls_m, "paternal": calls_p}
    flag = {}
    for k in ("INS", "DEL"):
        M, P = [r[:3] for r in calls_m[k][1]], [r[:3] for r in calls_p[k][1]]
        flag["maternal", k], flag["paternal", k] = partnered(M, P, num, den), partnered(P, M, num, den)
    out = []
    st = {"partnered_p": [sum(flag["paternal", "INS"]), sum(flag["paternal", "DEL"])]}
    for hap, k, cls in ORDER:
        text, rows = tables[hap][k]
        lines = text.split(b"\n")[:-1]
        assert len(lines) == len(rows)
        want = cls == "hom"
        t, rs = [], []
        for ln, r, f in zip(lines, rows, flag[hap, k]):
            if f != want:
                continue
            c = columns(ln, filter_pass).split(b"\t")
            if one_based:
                c[1] = b"%d" % (int(c[1]) + 1)
            t.append(b"\t".join(c) + b"\n")
            rs.append(tuple(r) + (0 if hap == "maternal" else 1, 1 if want else 0))
        st[hap[0] + "_" + k + "_" + cls] = len(rs)
        if rs:
            out.append((hap, k, cls, b"".join(t), rs))
    return out, st


def run(recs_m, cores_m, recs_p, cores_p, names, genome, num=3, den=10, filter_pass=False, one_based=False, **kw):
    """both passes and the combination: kw as svcalls_ref.calls() takes them, but hap"""
    m = sr.calls(recs_m, cores_m, names, genome, hap=b"maternal", **kw)
    p = sr.calls(recs_p, cores_p, names, genome, hap=b"paternal", **kw)
    return combine(m, p, num, den, filter_pass, one_based) + (m, p)
