"""The genotype rule and the writer of ``TIDDIT_SMALL_VCF`` (tiddit_amd/tiddit_small_vcf.py) on the CPU: the rule equals every literal
claim of tests/pileup_cases.py and an independent restatement, whose two departures (ties to the larger index, GQ uncapped) are noticed
by the named claims; literal lines for each record form (SNV, short DEL, ``<DEL>``, sequence INS, ``<INS>``), an ``N`` reference base,
``no_reference``, two alleles at one position, the merge order, each ``FILTER`` and the joined form, the header's counters, and
``parse_switch`` with every refusal text.

Every test of this file fails on the parent commit: the module does not exist there."""
import numpy as np
import pytest

import pileup_cases as D


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def test_the_rule_equals_every_literal_claim():
    from tiddit_amd import tiddit_small_vcf as V
    for name, alt, dp0, cols in D.RULE:
        assert V.genotype(alt, dp0) == cols, (name, V.genotype(alt, dp0))
    assert V.genotype(D.RULE_BEHIND_THE_END[1], 0) == D.RULE_BEHIND_THE_END[2]
    case, k1, sup, want = D.rule_case()
    depth = D.expected(case)[0]
    rows = [(int(a), 0, int(s), 0) for a, s in zip(k1.tolist(), sup.tolist())]
    got = V.genotype_rows(rows, depth, D.LENGTHS)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(V.genotype_rows((k1, k1, sup, sup), depth, D.LENGTHS), want)             # (the four columns instead of a list of rows)
    # a contig the table does not hold, and P = 0: a depth of 0
    assert V.genotype_rows([(99 << 32 | 5, 0, 4, 0), (D.B << 32, 0, 4, 0)], depth, D.LENGTHS).tolist() == [list(D.RULE_BEHIND_THE_END[2])] * 2


def restated_rule(alt, dp0, ties="smaller", cap=True):
    """the rule on numpy int64 vectors, written independently; ``ties`` / ``cap``: the two departures, built in on purpose"""
    other = np.maximum(np.int64(dp0) - np.int64(alt), 0)
    L = np.array([20 * np.int64(alt), 3 * (np.int64(alt) + other), 20 * other], dtype=object)
    order = sorted(range(3), key=lambda i: (L[i], i if ties == "smaller" else -i))
    pl = [min(int(L[i] - L[order[0]]), 9999) for i in range(3)]
    second = sorted(pl)[1]
    return int(dp0), int(other), pl[0], pl[1], pl[2], order[0], min(second, 99) if cap else second, int(alt > dp0)


def test_the_restated_rule_equals_the_rule_on_the_claims_and_on_a_grid():
    from tiddit_amd import tiddit_small_vcf as V
    for name, alt, dp0, cols in D.RULE:
        assert restated_rule(alt, dp0) == cols, name
    for alt in list(range(0, 70)) + [99, 100, 499, 500, 501, 3000, 2 ** 31, 2 ** 32 - 1]:
        for dp0 in list(range(0, 70)) + [99, 100, 499, 500, 501, 3000, 2 ** 31 - 1]:
            assert V.genotype(alt, dp0) == restated_rule(alt, dp0), (alt, dp0)


@pytest.mark.parametrize("departure,noticed_by", [({"ties": "larger"}, ("(3, 17)", "(17, 3)", "(0, 0)")), ({"cap": False}, ("GQ above 99", "PL at the cap"))])
def test_a_departure_of_the_rule_is_noticed_by_the_named_claims(departure, noticed_by):
    for start in noticed_by:
        hit = [(alt, dp0, cols) for name, alt, dp0, cols in D.RULE if name.startswith(start)]
        assert hit and all(restated_rule(alt, dp0, **departure) != cols for alt, dp0, cols in hit), start


# ---- the file -------------------------------------------------------------------------------------------------------------------
T0 = "ACGTNACGTA" + "GATTACAGGC" * 11                                            # contig 0, loaded; contig 1 (50 bases) is not
NAMES, LENGTHS = ("c0", "c1"), (len(T0), 50)
FMT = "GT:DP:AD:GQ:PL"
DEL_, INS_ = 0, 1 << 63


def k1(tid, P):
    return tid << 32 | P


def snv(ref, alt):
    return "ACGT".index(ref) << 3 | "ACGT".index(alt) << 1


def indel(type_bit, n, kind=0, payload=0):
    return type_bit | n << 47 | kind << 45 | payload << 1


def _made(snv_rows, indel_rows, depth=None):
    from tiddit_amd import refseq, tiddit_small_vcf as V
    ref = refseq.HostReference({0: refseq.codes_of_bases(T0)})
    if depth is None:
        depth = [np.full(LENGTHS[0], 20, dtype=np.uint32), np.zeros(LENGTHS[1], dtype=np.uint32)]
        depth[0][9] = 5
    return V.records_of(snv_rows, V.genotype_rows(snv_rows, depth, LENGTHS), indel_rows, V.genotype_rows(indel_rows, depth, LENGTHS), NAMES, ref)


SNV_ROWS = [(k1(0, 2), snv("C", "T"), 10, 4), (k1(0, 12), snv("A", "G"), 2, 1), (k1(0, 12), snv("A", "T"), 2, 1), (k1(1, 5), snv("A", "C"), 4, 2)]
INDEL_ROWS = [(k1(0, 4), indel(DEL_, 2), 3, 0),                                   # over the N
              (k1(0, 10), indel(INS_, 30, 1, 0x123), 5, 2),                       # a hashed insertion, where the depth is 5
              (k1(0, 12), indel(DEL_, 3), 20, 10),
              (k1(0, 12), indel(INS_, 2, 0, 2), 8, 8),                            # GA
              (k1(0, 21), indel(DEL_, 60), 6, 0),
              (k1(0, 30), indel(INS_, 7, 2), 2, 1),                               # SEQ *
              (k1(0, 118), indel(DEL_, 5), 9, 4),                                 # its six bases run past the end
              (k1(0, 120), indel(INS_, 1, 0, 3), 2, 1),                           # T behind the last base: written
              (k1(0, 121), indel(DEL_, 70), 2, 1),                                # a symbolic deletion whose anchor lies behind the end
              (k1(1, 7), indel(DEL_, 1), 5, 2)]                                   # a contig that is not loaded
WANT = [
    "c0\t2\t.\tC\tT\t140\tPASS\tTYPE=SNV;AS=10;FWD=6;REV=4\t" + FMT + "\t0/1:20:10,10:99:140,0,140",
    "c0\t4\t.\tTNA\tT\t0\tRefCall;LowGQ\tTYPE=DEL;AS=3;FWD=3;REV=0\t" + FMT + "\t0/0:20:17,3:0:0,0,280",
    "c0\t10\t.\tA\t<INS>\t100\tLowGQ\tTYPE=INS;AS=5;FWD=3;REV=2;SVLEN=30\t" + FMT + "\t1/1:5:0,5:15:100,15,0",
    "c0\t12\t.\tA\tG\t0\tRefCall\tTYPE=SNV;AS=2;FWD=1;REV=1\t" + FMT + "\t0/0:20:18,2:20:0,20,320",
    "c0\t12\t.\tA\tT\t0\tRefCall\tTYPE=SNV;AS=2;FWD=1;REV=1\t" + FMT + "\t0/0:20:18,2:20:0,20,320",
    "c0\t12\t.\tATTA\tA\t400\tPASS\tTYPE=DEL;AS=20;FWD=10;REV=10\t" + FMT + "\t1/1:20:0,20:60:400,60,0",
    "c0\t12\t.\tA\tAGA\t100\tOneStrand\tTYPE=INS;AS=8;FWD=0;REV=8\t" + FMT + "\t0/1:20:12,8:99:100,0,180",
    "c0\t21\t.\tG\t<DEL>\t60\tOneStrand\tTYPE=DEL;AS=6;FWD=6;REV=0;END=81;SVLEN=-60\t" + FMT + "\t0/1:20:14,6:60:60,0,220",
    "c0\t30\t.\tC\t<INS>\t0\tRefCall\tTYPE=INS;AS=2;FWD=1;REV=1;SVLEN=7\t" + FMT + "\t0/0:20:18,2:20:0,20,320",
    "c0\t120\t.\tC\tCT\t0\tRefCall\tTYPE=INS;AS=2;FWD=1;REV=1\t" + FMT + "\t0/0:20:18,2:20:0,20,320",
    "c1\t5\t.\tA\tC\t80\tLowGQ\tTYPE=SNV;AS=4;FWD=2;REV=2\t" + FMT + "\t1/1:4:0,4:12:80,12,0",
]


def test_every_record_form_is_the_literal_line_in_the_merge_order():
    """SNV < DEL < INS at one position, two SNV alleles at one position as two records by K2, an N in the reference written N, three
    indel rows without reference bases skipped and counted, an SNV on a contig that is not loaded written all the same"""
    assert T0[3:6] == "TNA" and T0[11:15] == "ATTA" and T0[20] == "G" and T0[29] == "C" and T0[119] == "C" and T0[9] == "A"
    lines, above, no_ref = _made(SNV_ROWS, INDEL_ROWS)
    assert lines == WANT
    assert (above, no_ref) == (1, 3)                                              # (above: the SNV on c1, whose depth is 0)
    # either table alone, rows in any order, and the four columns instead of a list
    assert _made(SNV_ROWS[::-1], None)[0] == [l for l in WANT if "TYPE=SNV" in l]
    assert _made(None, INDEL_ROWS[::-1])[0] == [l for l in WANT if "TYPE=SNV" not in l]
    cols = lambda rows: tuple(np.array(c, dtype=dt) for c, dt in zip(zip(*rows), (np.uint64, np.uint64, np.uint32, np.uint32)))
    assert _made(cols(SNV_ROWS), cols(INDEL_ROWS))[0] == WANT
    assert _made(None, None) == ([], 0, 0)


def test_each_filter_alone_and_joined():
    from tiddit_amd import tiddit_small_vcf as V
    assert V.filter_of(1, 20, 5, 0) == "PASS" and V.filter_of(2, 99, 6, 3) == "PASS"
    assert V.filter_of(0, 20, 5, 2) == "RefCall" and V.filter_of(1, 19, 5, 2) == "LowGQ"
    assert V.filter_of(1, 20, 6, 0) == "OneStrand" and V.filter_of(1, 20, 6, 6) == "OneStrand" and V.filter_of(1, 20, 5, 5) == "PASS"
    assert V.filter_of(0, 0, 3, 0) == "RefCall;LowGQ" and V.filter_of(1, 3, 7, 7) == "LowGQ;OneStrand" and V.filter_of(0, 25, 9, 0) == "RefCall;OneStrand"
    assert V.filter_of(0, 0, 6, 0) == "RefCall;LowGQ;OneStrand"
    # ... and in a record: ALT above the depth with all reads on one strand and a low GQ
    depth = [np.full(LENGTHS[0], 1, dtype=np.uint32), np.zeros(50, dtype=np.uint32)]
    assert _made([(k1(0, 2), snv("C", "G"), 6, 6)], None, depth) == (["c0\t2\t.\tC\tG\t120\tLowGQ;OneStrand\tTYPE=SNV;AS=6;FWD=0;REV=6\t" + FMT + "\t1/1:6:0,6:18:120,18,0"], 1, 0)


def test_the_header_carries_the_cut_the_normalisation_and_every_counter(tmp_path):
    from tiddit_amd import tiddit_clip_vcf, tiddit_pileup, tiddit_small_vcf as V
    assert V.SN == D.SN + ("support_above_depth", "no_reference", "written_records")
    lines, above, no_ref = _made(SNV_ROWS, INDEL_ROWS)
    counts = V.counts_of(np.arange(11, 18, dtype=np.uint64), above, no_ref, len(lines))
    parts = tiddit_clip_vcf.header_parts({"SQ": [{"SN": n, "LN": ln} for n, ln in zip(NAMES, LENGTHS)]}, "sample", "3.9.5")
    path = str(tmp_path / "x.small.vcf")
    V.write_file(path, parts, 20, True, counts, lines)
    text = open(path).read().split("\n")
    assert text[-1] == "" and text[-1 - len(WANT):-1] == WANT
    head = text[:-1 - len(WANT)]
    assert head[0] == "##fileformat=VCFv4.1" and head[1] == "##source=TIDDIT-3.9.5 small_vcf v1"
    assert head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample" and head[-2].startswith("##TIDDITcmd=")
    assert head[-14:-2] == ["##small_vcf_min_mapq=20", "##small_vcf_left_normalised=1", "##small_vcf_records=11", "##small_vcf_eligible=12",
                            "##small_vcf_malformed=13", "##small_vcf_no_cigar=14", "##small_vcf_spans=15", "##small_vcf_covered_bases=16",
                            "##small_vcf_clamped_spans=17", "##small_vcf_support_above_depth=1", "##small_vcf_no_reference=3", "##small_vcf_written_records=11"]
    assert ["##contig=<ID=c0,length=120>", "##contig=<ID=c1,length=50>"] == [l for l in head if l.startswith("##contig")]
    for kind, ids in (("ALT", ("DEL", "INS")), ("INFO", ("TYPE", "AS", "FWD", "REV", "END", "SVLEN")), ("FILTER", ("RefCall", "LowGQ", "OneStrand")),
                      ("FORMAT", ("GT", "DP", "AD", "GQ", "PL"))):
        assert [l.split("ID=")[1].split(",")[0] for l in head if l.startswith("##%s=" % kind)] == list(ids)
    V.write_file(path, parts, 0, False, counts, [])
    text = open(path).read().split("\n")
    assert "##small_vcf_min_mapq=0" in text and "##small_vcf_left_normalised=0" in text and text[-2].startswith("#CHROM")
    assert V.summary_line(counts) == ("small vcf: 11 records written, 15 spans, 16 covered bases, 17 clamped spans, support above depth 1, no reference 3, "
                                      "malformed records 13")


def test_parse_switch_and_every_refusal_text():
    from tiddit_amd import tiddit_small_vcf as V
    assert V.parse_switch(None) is None and V.parse_switch("") is None and V.parse_switch("", (3, 20, 20), (2, 20)) is None
    assert V.parse_switch("1", (3, 20, 20), None) == 20 and V.parse_switch("1", None, (2, 7)) == 7 and V.parse_switch("1", (3, 0, 20), (2, 0)) == 0
    for value in ("0", "2", "yes", "1:20", " 1", "01"):
        with pytest.raises(ValueError, match=r"^the switch is 1$"):
            V.parse_switch(value, (3, 20, 20), (2, 20))
    with pytest.raises(ValueError, match=r"^the switch genotypes the rows of TIDDIT_SNVS and TIDDIT_INDELS, neither of which is set$"):
        V.parse_switch("1")
    with pytest.raises(ValueError, match=r"^TIDDIT_SNVS and TIDDIT_INDELS have different minimum MAPQ \(30 and 20\): the depth is counted at one$"):
        V.parse_switch("1", (3, 30, 20), (2, 20))
    with pytest.raises(ValueError, match=r"^the switch is 1$"):                   # (the value is judged first)
        V.parse_switch("2")
