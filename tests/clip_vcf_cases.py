"""Aimed cases for the junction VCF of the clip stages (tiddit_amd/tiddit_clip_vcf.py, csrc/tdt_junction.hip), each with the claim it
makes written down from what the case PLANTED — never computed by the definition, by the restatement of tests/test_clip_vcf_refs_cpu.py
or by the device.

KERNEL CASES (``KERNEL_CASES``): a hand-built evidence store — ``contigs`` = [(LN, [(start, end, bits), ...] sorted by start)] — a list
of ``boundaries`` [(contig row, b)], the flank ``F`` and ``expect`` = [(left, right, span, span_lowq)] per boundary, literal.  ``span``
(optional) replaces a contig's max span in the table (the default is what the pack kernel would have found: max(end - start, 0)).

JUNCTION CASES (``JUNCTION_CASES``): rows in the layouts of ``tiddit_clip_align.summarise``, ``tiddit_clip_far.summarise`` and
``tiddit_clip_ins.file_rows`` in, the record lines and the header counters out, literal.  ``support`` gives (left, right, span,
span_lowq) per boundary in the order of ``tiddit_clip_vcf.boundaries_of`` (default: all zero)."""
import os
import re

import numpy as np

UNMAPPED, MATE_UNMAPPED, DUPLICATE, HAS_SA, LOW_Q, DISCORDANT = 0x04, 0x08, 0x01, 0x02, 0x10, 0x20
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiddit_amd", "csrc", "tdt_junction.hip")).read()


def _define(name):
    """a number from the `#define` lines of csrc/tdt_junction.hip: the cases stay on the kernel's edges when it is retuned"""
    return int(re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+([0-9]+)[ \t]*(?://[^\n]*)?$" % name, _SRC, re.M).group(1))


JS_THREADS, JS_MAX_FLANK = _define("JS_THREADS"), _define("JS_MAX_FLANK")
JS_WAVES = JS_THREADS // 64                     # boundaries per workgroup
EV_RECORD = np.dtype([("start", "<i4"), ("end", "<i4"), ("mate_pos", "<i4"), ("bits", "u1"), ("pad", "u1", (3,))])

KERNEL_CASES = []


def kcase(family, name, claims, contigs, boundaries, F, expect, span=None):
    assert len(boundaries) == len(expect)
    KERNEL_CASES.append({"family": family, "name": family + ": " + name, "claims": claims, "contigs": contigs, "boundaries": boundaries, "F": F,
                         "expect": [tuple(e) for e in expect], "span": span or {}})


def table(case):
    """int64[n][5] (offset, n, max span, tid, length) of the case's store"""
    t = np.zeros((len(case["contigs"]), 5), dtype=np.int64)
    o = 0
    for c, (ln, recs) in enumerate(case["contigs"]):
        sp = max([max(e - s, 0) for s, e, _ in recs] + [0])
        t[c] = (o if recs else 0, len(recs), case["span"].get(c, sp), c, ln)             # (a contig without records keeps offset 0, as the store books it)
        o += len(recs)
    return t


def records(case):
    """the store's records, all contigs back to back, as the device holds them"""
    flat = [r for _, recs in case["contigs"] for r in recs]
    out = np.zeros(len(flat), dtype=EV_RECORD)
    for i, (s, e, b) in enumerate(flat):
        out[i] = (s, e, -1, b, (0, 0, 0))
    return out


# ---- 1. the four comparisons, one base to either side
kcase("edges", "start = b - F and b - F + 1", "b = 500, F = 10: the base 490 is held by the record that starts at 490, not by the one at 491; both hold 509",
      [(1000, [(490, 600, 0), (491, 600, 0)])], [(0, 500)], 10, [(1, 2, 1, 0)])
kcase("edges", "end = b + F and b + F - 1", "the base 509 is held by the record that ends at 510 (exclusive), not by the one that ends at 509; both hold 490",
      [(1000, [(400, 509, 0), (400, 510, 0)])], [(0, 500)], 10, [(2, 1, 1, 0)])
kcase("edges", "b - F = 0 and -1", "b = 10: base 0 is held by both records, base 19 by the long one; b = 9: there is no base -1, left is 0, and nothing spans",
      [(1000, [(0, 5, 0), (0, 100, 0)])], [(0, 10), (0, 9)], 10, [(2, 1, 1, 0), (0, 1, 0, 0)])
kcase("edges", "b + F = LN and LN + 1", "b = 990: base 999 is the contig's last and is held; b = 991: base 1000 does not exist, right is 0",
      [(1000, [(950, 1000, 0)])], [(0, 990), (0, 991)], 10, [(1, 1, 1, 0), (1, 0, 0, 0)])
kcase("edges", "b = 0 and b = LN", "the cut in front of the first base has no left side, the cut behind the last base no right side",
      [(1000, [(0, 100, 0), (900, 1000, 0)])], [(0, 0), (0, 1000)], 10, [(0, 1, 0, 0), (1, 0, 0, 0)])
kcase("edges", "b beyond the contig, end beyond LN", "b = 1015: base 1005 lies beyond LN = 1000; a record whose end field says 1200 is clamped to LN and does not hold it; "
      "b = -3 and b = 1500 count nothing; b = 990: the clamped record holds 980 and 999",
      [(1000, [(900, 1200, 0)])], [(0, 1015), (0, -3), (0, 1500), (0, 990)], 10, [(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (1, 1, 1, 0)])
kcase("edges", "end <= start", "records with end = start and end < start count nowhere; one of one base holds only base 450; the 40-base read spans b = 500",
      [(1000, [(450, 450, 0), (450, 440, 0), (450, 451, 0), (480, 520, 0)])], [(0, 500), (0, 451)], 10, [(1, 1, 1, 0), (0, 0, 0, 0)])
kcase("edges", "F = 1", "the flank of one base: b = 150 inside the read spans, b = 200 at its end has the left base only, b = 100 at its start the right base only",
      [(5000, [(100, 200, 0)])], [(0, 150), (0, 200), (0, 100)], 1, [(1, 1, 1, 0), (1, 0, 0, 0), (0, 1, 0, 0)])
kcase("edges", "F = %d" % JS_MAX_FLANK, "b = 2000: base 1000 and base 2999; a read 1000 ... 2999 spans, one that ends a base earlier or starts a base later does not",
      [(5000, [(1000, 2999, 0), (1000, 3000, 0), (1001, 3000, 0)])], [(0, 2000)], JS_MAX_FLANK, [(2, 2, 1, 0)])

# ---- 2. the read filter
_BITS = (UNMAPPED, DUPLICATE, LOW_Q, UNMAPPED | DUPLICATE, UNMAPPED | LOW_Q, DUPLICATE | LOW_Q, MATE_UNMAPPED, HAS_SA, DISCORDANT,
         MATE_UNMAPPED | HAS_SA | DISCORDANT, LOW_Q | DISCORDANT, 0)
kcase("filter", "each excluding bit alone and in pairs, the three irrelevant bits", "twelve reads over b = 500: the five without an excluding bit (none, 0x08, 0x02, 0x20 "
      "and the three together) count, LOW_Q alone and LOW_Q with DISCORDANT are span_lowq, the others count nowhere",
      [(1000, [(400, 600, x) for x in _BITS])], [(0, 500)], 10, [(5, 5, 5, 2)])
kcase("filter", "low-quality reads that hold one side only", "span_lowq asks for both bases as span does",
      [(1000, [(400, 505, LOW_Q), (400, 600, LOW_Q), (495, 600, LOW_Q)])], [(0, 500)], 10, [(0, 0, 0, 1)])

# ---- 3. the bracket
_HUNDREDS = [(s, s + 100, 0) for s in range(10000, 20001, 50)]
kcase("bracket", "one record of span 5000 far to the left", "b = 10050: the 100-base reads that start at 10000 (both bases) and 10050 (base 10059) and the read 5100 ... 10099, "
      "which starts 4940 bases in front of base 10040 and is found only through the contig's max span",
      [(100000, [(5100, 10100, 0)] + _HUNDREDS)], [(0, 10050)], 10, [(2, 3, 2, 0)])
for _n in (0, 1, 63, 64, 65, 4095, 4096, 4097):
    kcase("bracket", "%d candidates" % _n, "%d equal reads 1000 ... 1099 between ten that end at 20 and ten that start at 5000: every one holds both bases of b = 1050" % _n,
          [(10000, [(10, 20, 0)] * 10 + [(1000, 1100, 0)] * _n + [(5000, 5100, 0)] * 10)], [(0, 1050)], 10, [(_n, _n, _n, 0)], span={0: 100})
kcase("bracket", "a run of equal start across each bracket end", "max span 100, b = 1050: 70 reads start at 940 (just outside the bracket, they end in front of base 1040), 70 at "
      "941 (they hold 1040), 70 at 1059 (they hold 1059), 70 at 1060 (outside)",
      [(10000, [(940, 1040, 0)] * 70 + [(941, 1041, 0)] * 70 + [(1059, 1159, 0)] * 70 + [(1060, 1160, 0)] * 70)], [(0, 1050)], 10, [(70, 70, 0, 0)])


# ---- 4. the search: contig ranges of <= 64, 65 ... 4096 and > 4096 records (0, 1 and 2 rounds of the 64-ary search)
def _tiled(n):
    """n reads of 100 bases, one every 10: base 10 k is held by the ten reads k - 9 ... k"""
    return (10 * n + 200, [(10 * i, 10 * i + 100, 0) for i in range(n)])


_TEN = (10, 10, 9, 0)    # b = 10 k, F = 10: base 10 (k - 1) by reads k - 10 ... k - 1, base 10 k + 9 by reads k - 9 ... k, both by k - 9 ... k - 1
kcase("search", "ranges of 64, 4096 and 5000 records", "one boundary in the middle of each contig, one 5 reads behind the start of the middle one (reads 0 ... 4 and 0 ... 5) "
      "and one at the last read of the third", [_tiled(64), _tiled(4096), _tiled(5000)], [(0, 300), (1, 20000), (1, 50), (2, 49900), (2, 25000)], 10,
      [_TEN, _TEN, (5, 6, 5, 0), _TEN, _TEN])
kcase("search", "three contigs with an empty one in the middle", "the third contig's range starts behind the first one's two records",
      [(1000, [(100, 200, 0)] * 2), (500, []), (1000, [(100, 200, 0)] * 3)], [(0, 150), (1, 150), (2, 150)], 10, [(2, 2, 2, 0), (0, 0, 0, 0), (3, 3, 3, 0)])
kcase("search", "boundaries unsorted and repeated", "every boundary is answered for itself", [_tiled(64), _tiled(4096)], [(1, 20000), (1, 50), (0, 300), (1, 20000), (1, 50), (1, 1000)], 10,
      [_TEN, (5, 6, 5, 0), _TEN, _TEN, (5, 6, 5, 0), _TEN])
for _nb in (1, 3, 4, 5, 3 * JS_WAVES + 1):
    kcase("search", "nb = %d" % _nb, "a workgroup answers %d boundaries: the last one has a partly filled workgroup, or a full one" % JS_WAVES, [_tiled(4096)],
          [(0, 10 * (20 + i)) for i in range(_nb)], 10, [_TEN] * _nb)

# ---- 5. 64-bit positions
_LN = 2 ** 31 - 1
kcase("overflow", "a contig of 2^31 - 1 bases, boundaries at its end", "two reads end at LN.  b = LN: base LN - 10 is held, b + F = LN + 10 is beyond the contig — and beyond int32; "
      "b = LN - 5 the same; b = LN - 10: base LN - 1 is the contig's last and is held",
      [(_LN, [(_LN - 200, _LN, 0)] * 2)], [(0, _LN), (0, _LN - 5), (0, _LN - 10)], 10, [(2, 0, 0, 0), (2, 0, 0, 0), (2, 2, 2, 0)])

N_KERNEL_CASES = len(KERNEL_CASES)

# ---- 6. from sites to boundaries: a deletion of 401 ... 600 on a contig of 1000 bases, R site at P = 400, L site at P = 601 (1-based), F = 10.
# The R cut has 400 bases to its left, the L cut 600.  Of the three reference reads the first holds 390 ... 409, the second ends with base 609 —
# the last base the L cut asks for — and the third starts with base 590, the first it asks for.
SITE_CASE = {"contigs": [(1000, [(300, 410, 0), (500, 610, 0), (590, 700, 0)])], "R": (0, 400), "L": (0, 601), "F": 10, "boundaries": [(0, 400), (0, 600)],
             "expect": [(1, 1, 1, 0), (2, 2, 2, 0)], "span": {}}

# ------------------------------------------------------------------------------------------- junction cases
JUNCTION_CASES = []
NAMES = ["chrA", "chrB"]
L, R = 0, 1
FMT = "GT:RV:RR:LQ:DPF"
ZERO = {"junctions": 0, "both_sources": 0, "sources_disagree": 0, "one_sided": 0, "not_mutual": 0, "inv_rows": 0, "ins_rows": 0, "ins_explained": 0, "records": 0,
        "ambiguous": 0}


def jcase(name, claims, lines, counts, align=None, far=None, ins=None, support=None):
    JUNCTION_CASES.append({"name": name, "claims": claims, "align": align, "far": far, "ins": ins, "support": support, "lines": lines, "counts": dict(ZERO, **counts)})


def a_row(tid, P, side, sup, Q, typ, ln, mate, hom, mm=0, hits=1, strand=0):
    """an ALIGN row: (tid, P, side, SUPPORT, CLEN, PARTNER, strand, mm, HITS, TYPE, LEN, MATE, HOM)"""
    return (tid, P, side, sup, 28, Q, strand, mm, hits, typ, ln, mate, hom)


def f_row(tid, P, side, sup, pt, Q, typ, ln, mt, mate, hom, mm=0, hits=1, strand=0):
    """a FAR row: (tid, P, side, SUPPORT, CLEN, partner contig, PARTNER, strand, mm, HITS, TYPE, LEN, mate contig, MATE, HOM)"""
    return (tid, P, side, sup, 28, pt, Q, strand, mm, hits, typ, ln, mt, mate, hom)


def i_row(tid, PR, tsd, rs, ls, ln, seq, mm=0, closures=1, left="ACGTACGTACGTACGTACGT", right="TTGCATTGCATTGCATTGCA"):
    """an INS row: (tid, P_R, P_L, TSD, R_SUPPORT, L_SUPPORT, R_COLS, L_COLS, status, LEN, MISMATCH, CLOSURES, SEQ, LEFT_SEQ, RIGHT_SEQ)"""
    closed = ln is not None
    return (tid, PR, PR + 1 - tsd, tsd, rs, ls, len(left), len(right), int(closed), ln, mm if closed else None, closures, seq if closed else ".", left, right)


def rec(chrom, pos, rid, alt, flt, info, sample):
    return "\t".join((chrom, str(pos), rid, "N", alt, ".", flt, info, FMT, sample))


# a deletion of bases a + 1 ... b and a tandem duplication of a ... b, both with h bases of microhomology, as the align and far cases plant them:
# DEL: R at a + h with PARTNER b + h + 1, L at b + 1 with PARTNER a.  DUP: R at b + h with PARTNER a + h, L at a with PARTNER b.
_A, _B, _BD = 400, 600, 599
for _h in (0, 1, 5, 28):
    _del_a = [a_row(1, _A + _h, R, 5, _B + _h + 1, "DEL", 200, _B + 1, _h), a_row(1, _B + 1, L, 4, _A, "DEL", 200, _A + _h, _h, mm=1)]
    _del_f = [f_row(1, _A + _h, R, 5, 1, _B + _h + 1, "DEL", 200, 1, _B + 1, _h), f_row(1, _B + 1, L, 4, 1, _A, "DEL", 200, 1, _A + _h, _h, mm=1)]
    _dup_a = [a_row(1, _BD + _h, R, 3, _A + _h, "DUP", 200, _A, _h), a_row(1, _A, L, 6, _BD, "DUP", 200, _BD + _h, _h)]
    _dup_f = [f_row(1, _BD + _h, R, 3, 1, _A + _h, "DUP", 200, 1, _A, _h), f_row(1, _A, L, 6, 1, _BD, "DUP", 200, 1, _BD + _h, _h)]
    for _src, _kw in (("align", {"align": _del_a}), ("far", {"far": _del_f}), ("align,far", {"align": _del_a, "far": _del_f})):
        jcase("DEL of 401 ... 600, HOM %d, from %s" % (_h, _src), "POS 400 is the base in front of the left-most placement, END 600 its last base, whatever the homology",
              [rec("chrB", 400, "CLIP_1", "<DEL>", "PASS", "SVTYPE=DEL;END=600;SVLEN=-200;CIPOS=0,%d;HOMLEN=%d;SRC=%s;MISMATCH=0,1" % (_h, _h, _src), "1/1:5,4:0,0:0,0:0,0,0,0")],
              {"junctions": 1, "records": 1, "both_sources": int(_src == "align,far")}, **_kw)
    for _src, _kw in (("align", {"align": _dup_a}), ("far", {"far": _dup_f}), ("align,far", {"align": _dup_a, "far": _dup_f})):
        jcase("DUP of 400 ... 599, HOM %d, from %s" % (_h, _src), "POS 399 is the base in front of the duplicated stretch, END 599 its last base",
              [rec("chrB", 399, "CLIP_1", "<DUP>", "PASS", "SVTYPE=DUP;END=599;SVLEN=200;CIPOS=0,%d;HOMLEN=%d;SRC=%s;MISMATCH=0,0" % (_h, _h, _src), "1/1:3,6:0,0:0,0:0,0,0,0")],
              {"junctions": 1, "records": 1, "both_sources": int(_src == "align,far")}, **_kw)
jcase("both stages, disagreeing", "FAR calls the same two sites with HOM 4 where ALIGN says 5: one junction, ALIGN's rows, counted as disagreeing",
      [rec("chrB", 400, "CLIP_1", "<DEL>", "PASS", "SVTYPE=DEL;END=600;SVLEN=-200;CIPOS=0,5;HOMLEN=5;SRC=align,far;MISMATCH=0,0", "1/1:5,4:0,0:0,0:0,0,0,0")],
      {"junctions": 1, "records": 1, "both_sources": 1, "sources_disagree": 1},
      align=[a_row(1, 405, R, 5, 606, "DEL", 200, 601, 5), a_row(1, 601, L, 4, 400, "DEL", 200, 405, 5)],
      far=[f_row(1, 405, R, 5, 1, 606, "DEL", 200, 1, 601, 4), f_row(1, 601, L, 4, 1, 400, "DEL", 200, 1, 405, 4)])
# a translocation A[... 400] + B[601 ...] with 5 bases of homology: R on A at 405 with PARTNER B:606, L on B at 601 with PARTNER A:400
jcase("BND with both records", "the record on A at 400 joins to B:601 behind it, the record on B at 601 has A:400 in front of it; they name each other",
      [rec("chrA", 400, "CLIP_1_1", "N[chrB:601[", "PASS", "SVTYPE=BND;MATEID=CLIP_1_2;CIPOS=0,5;HOMLEN=5;SRC=far;MISMATCH=0,2", "1/1:7,8:0,0:0,0:0,0,0,0"),
       rec("chrB", 601, "CLIP_1_2", "]chrA:400]N", "PASS", "SVTYPE=BND;MATEID=CLIP_1_1;CIPOS=0,5;HOMLEN=5;SRC=far;MISMATCH=0,2", "1/1:7,8:0,0:0,0:0,0,0,0")],
      {"junctions": 1, "records": 2}, far=[f_row(0, 405, R, 7, 1, 606, "BND", None, 1, 601, 5), f_row(1, 601, L, 8, 0, 400, "BND", None, 0, 405, 5, mm=2)])
jcase("rows that make no record", "an R row whose chosen mate chose another R row (not mutual, and that mate's own pair is the junction), a DEL row without a mate, a "
      "reverse-strand BND row, a REF row, an INV row, an unaligned row",
      [rec("chrB", 400, "CLIP_1", "<DEL>", "PASS", "SVTYPE=DEL;END=600;SVLEN=-200;CIPOS=0,0;HOMLEN=0;SRC=align;MISMATCH=0,0", "1/1:5,4:0,0:0,0:0,0,0,0")],
      {"junctions": 1, "records": 1, "not_mutual": 1, "one_sided": 2, "inv_rows": 2},
      align=[a_row(1, 400, R, 5, 601, "DEL", 200, 601, 0), a_row(1, 601, L, 4, 400, "DEL", 200, 400, 0), a_row(1, 397, R, 3, 598, "DEL", 200, 601, 3),
             a_row(1, 900, R, 3, 1200, "DEL", 299, None, None), a_row(1, 100, R, 3, 101, "REF", 0, None, None), a_row(1, 700, R, 3, 800, "INV", 100, None, None, strand=1),
             (1, 750, R, 3, 28, 760, 0, 5, 0, None, None, None, None)],
      far=[f_row(0, 400, R, 3, 1, 300, "BND", None, None, None, None, strand=1), f_row(1, 700, R, 3, 1, 800, "INV", 100, None, None, None, strand=1),
           (1, 750, R, 3, 28, None, None, None, None, 0, None, None, None, None, None)])
jcase("HITS > 1", "the L row's consensus places twice: the record is written and filtered",
      [rec("chrB", 400, "CLIP_1", "<DEL>", "Ambiguous", "SVTYPE=DEL;END=600;SVLEN=-200;CIPOS=0,0;HOMLEN=0;SRC=align;MISMATCH=0,0", "1/1:5,4:0,0:0,0:0,0,0,0")],
      {"junctions": 1, "records": 1, "ambiguous": 1}, align=[a_row(1, 400, R, 5, 601, "DEL", 200, 601, 0), a_row(1, 601, L, 4, 400, "DEL", 200, 400, 0, hits=2)])
_SEQ = "ACGTTGCAAC" * 6
for _tsd in (0, 15, 32):
    jcase("INS closed, TSD %d" % _tsd, "60 bases behind base 2000; with a target-site duplication the L site lies TSD bases to the left and POS is the base in front of it",
          [rec("chrA", 2000 - _tsd, "CLIP_1", "<INS>", "PASS", "SVTYPE=INS;END=%d;SVLEN=60;CIPOS=0,%d;TSD=%d;SVINSSEQ=%s;SRC=ins;MISMATCH=1" % (2000 - _tsd, _tsd, _tsd, _SEQ),
               "1/1:4,5:0,0:0,0:0,0,0,0")], {"ins_rows": 1, "records": 1}, ins=[i_row(0, 2000, _tsd, 4, 5, 60, _SEQ, mm=1)])
    jcase("INS open, TSD %d" % _tsd, "no closure: the two flanks, no SVLEN, no MISMATCH",
          [rec("chrA", 2000 - _tsd, "CLIP_1", "<INS>", "PASS", "SVTYPE=INS;END=%d;CIPOS=0,%d;TSD=%d;LEFT_SVINSSEQ=ACGTACGTACGTACGTACGT;RIGHT_SVINSSEQ=TTGCATTGCATTGCATTGCA;SRC=ins"
               % (2000 - _tsd, _tsd, _tsd), "1/1:4,5:0,0:0,0:0,0,0,0")], {"ins_rows": 1, "records": 1}, ins=[i_row(0, 2000, _tsd, 4, 5, None, None)])
# a 20-base tandem duplication of 981 ... 1000 with no homology: R at 1000 with PARTNER 981, L at 981 with PARTNER 1000; the INS stage pairs the same two sites with TSD 20
jcase("an INS pair explained by a DUP", "the two sites are a junction of rule 1: the DUP record stands, the pair row is dropped",
      [rec("chrA", 980, "CLIP_1", "<DUP>", "PASS", "SVTYPE=DUP;END=1000;SVLEN=20;CIPOS=0,0;HOMLEN=0;SRC=align;MISMATCH=0,0", "1/1:3,3:0,0:0,0:0,0,0,0")],
      {"junctions": 1, "records": 1, "ins_explained": 1}, align=[a_row(0, 1000, R, 3, 981, "DUP", 20, 981, 0), a_row(0, 981, L, 3, 1000, "DUP", 20, 1000, 0)],
      ins=[i_row(0, 1000, 20, 3, 3, 40, "ACGT" * 10)])
jcase("a site in two pair rows, and several closures", "the R site at 3000 pairs with the L sites at 3001 and 2991: both rows are records, both filtered; the pair at 5000 closes at "
      "three lengths: filtered",
      [rec("chrA", 2990, "CLIP_1", "<INS>", "Ambiguous", "SVTYPE=INS;END=2990;SVLEN=44;CIPOS=0,10;TSD=10;SVINSSEQ=%s;SRC=ins;MISMATCH=0" % ("ACGTTGCAACG" * 4), "1/1:3,3:0,0:0,0:0,0,0,0"),
       rec("chrA", 3000, "CLIP_2", "<INS>", "Ambiguous", "SVTYPE=INS;END=3000;SVLEN=40;CIPOS=0,0;TSD=0;SVINSSEQ=%s;SRC=ins;MISMATCH=0" % ("ACGT" * 10), "1/1:3,4:0,0:0,0:0,0,0,0"),
       rec("chrA", 5000, "CLIP_3", "<INS>", "Ambiguous", "SVTYPE=INS;END=5000;SVLEN=40;CIPOS=0,0;TSD=0;SVINSSEQ=%s;SRC=ins;MISMATCH=0" % ("ACGT" * 10), "1/1:3,3:0,0:0,0:0,0,0,0")],
      {"ins_rows": 3, "records": 3, "ambiguous": 3},
      ins=[i_row(0, 3000, 10, 3, 3, 44, "ACGTTGCAACG" * 4), i_row(0, 3000, 0, 3, 4, 40, "ACGT" * 10), i_row(0, 5000, 0, 3, 3, 40, "ACGT" * 10, closures=3)])
# the genotype cuts: DEL 4 ALT >= 3 (ALT + REF)  <=>  ALT >= 3 REF;  DUP 12 ALT >= 5 (ALT + REF)  <=>  7 ALT >= 5 REF
_DEL0 = [a_row(1, 400, R, 5, 601, "DEL", 200, 601, 0), a_row(1, 601, L, 4, 400, "DEL", 200, 400, 0)]
_DEL1 = [a_row(1, 400, R, 4, 601, "DEL", 200, 601, 0), a_row(1, 601, L, 4, 400, "DEL", 200, 400, 0)]
_DUP0 = [a_row(1, 599, R, 3, 400, "DUP", 200, 400, 0), a_row(1, 400, L, 2, 599, "DUP", 200, 599, 0)]
for _rows, _typ, _sup, _gt, _why in ((_DEL0, "DEL", [(9, 8, 2, 1), (7, 6, 1, 0)], "1/1", "ALT 9, REF 3: 36 >= 36"), (_DEL1, "DEL", [(9, 8, 2, 1), (7, 6, 1, 0)], "0/1", "ALT 8, REF 3: 32 < 33"),
                                     (_DUP0, "DUP", [(9, 8, 4, 1), (7, 6, 3, 0)], "1/1", "ALT 5, REF 7: 60 >= 60"), (_DUP0, "DUP", [(9, 8, 4, 1), (7, 6, 4, 0)], "0/1", "ALT 5, REF 8: 60 < 65")):
    _sv = "SVTYPE=DEL;END=600;SVLEN=-200" if _typ == "DEL" else "SVTYPE=DUP;END=599;SVLEN=200"
    _rv = "%d,%d" % (_rows[0][3], _rows[1][3])
    jcase("the %s cut, %s" % (_typ, _gt), _why + "; RR, LQ and DPF are the kernel's numbers, R boundary first",
          [rec("chrB", 400 if _typ == "DEL" else 399, "CLIP_1", "<%s>" % _typ, "PASS", _sv + ";CIPOS=0,0;HOMLEN=0;SRC=align;MISMATCH=0,0",
               "%s:%s:%d,%d:%d,%d:%d,%d,%d,%d" % (_gt, _rv, _sup[0][2], _sup[1][2], _sup[0][3], _sup[1][3], _sup[0][0], _sup[0][1], _sup[1][0], _sup[1][1]))],
          {"junctions": 1, "records": 1}, align=_rows, support=_sup)
jcase("the output order and the IDs", "events ascend by (contig, POS, END, type); the BND pair is numbered by its first record and its second record sorts where it lies; an "
      "insertion and a deletion at one POS: END decides",
      [rec("chrA", 400, "CLIP_1_1", "N[chrB:90[", "PASS", "SVTYPE=BND;MATEID=CLIP_1_2;CIPOS=0,0;HOMLEN=0;SRC=far;MISMATCH=0,0", "1/1:3,3:0,0:0,0:0,0,0,0"),
       rec("chrA", 2000, "CLIP_2", "<INS>", "PASS", "SVTYPE=INS;END=2000;SVLEN=40;CIPOS=0,0;TSD=0;SVINSSEQ=%s;SRC=ins;MISMATCH=0" % ("ACGT" * 10), "1/1:3,3:0,0:0,0:0,0,0,0"),
       rec("chrA", 2000, "CLIP_3", "<DEL>", "PASS", "SVTYPE=DEL;END=2100;SVLEN=-100;CIPOS=0,0;HOMLEN=0;SRC=far;MISMATCH=0,0", "1/1:3,3:0,0:0,0:0,0,0,0"),
       rec("chrB", 90, "CLIP_1_2", "]chrA:400]N", "PASS", "SVTYPE=BND;MATEID=CLIP_1_1;CIPOS=0,0;HOMLEN=0;SRC=far;MISMATCH=0,0", "1/1:3,3:0,0:0,0:0,0,0,0"),
       rec("chrB", 399, "CLIP_4", "<DUP>", "PASS", "SVTYPE=DUP;END=599;SVLEN=200;CIPOS=0,0;HOMLEN=0;SRC=far;MISMATCH=0,0", "1/1:3,3:0,0:0,0:0,0,0,0")],
      {"junctions": 3, "ins_rows": 1, "records": 5},
      far=[f_row(1, 599, R, 3, 1, 400, "DUP", 200, 1, 400, 0), f_row(1, 400, L, 3, 1, 599, "DUP", 200, 1, 599, 0), f_row(0, 2000, R, 3, 0, 2101, "DEL", 100, 0, 2101, 0),
           f_row(0, 2101, L, 3, 0, 2000, "DEL", 100, 0, 2000, 0), f_row(0, 400, R, 3, 1, 90, "BND", None, 1, 90, 0), f_row(1, 90, L, 3, 0, 400, "BND", None, 0, 400, 0)],
      ins=[i_row(0, 2000, 0, 3, 3, 40, "ACGT" * 10)])
jcase("an empty job", "all three stages ran and gave no row: the header only", [], {}, align=[], far=[], ins=[])

N_JUNCTION_CASES = len(JUNCTION_CASES)
