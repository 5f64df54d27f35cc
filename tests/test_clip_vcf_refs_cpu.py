"""The junction VCF of the clip stages without a GPU: the loop definition of the boundary support (tiddit_amd/tiddit_clip_vcf.py rule 4), an
independent numpy restatement (sorted starts, one ``searchsorted`` pair per boundary, as the device brackets its candidates) and the
literal claims of tests/clip_vcf_cases.py agree on every kernel case; one-line departures of the restatement are each noticed by a claim
of the family listed for them; every junction case's records and header counters equal its literal text; events planted through the real
``tiddit_clip_align`` / ``tiddit_clip_far`` definitions come out at their left-aligned coordinates for every microhomology; and the switch.

Every test of this file fails on the parent commit: the module does not exist there."""
import numpy as np
import pytest

import clip_align_cases as CA
import clip_far_cases as CF
import clip_vcf_cases as X
from tiddit_amd import tiddit_clip_vcf as V

BAM_HEADER = {"SQ": [{"SN": "chrA", "LN": 12000}, {"SN": "chrB", "LN": 8000}]}


# ---- the two readings of rule 4 -----------------------------------------------------------------------------------------------
def definition(case):
    tab, recs = X.table(case), X.records(case)
    out = []
    for row, b in case["boundaries"]:
        o, n, _, _, ln = (int(v) for v in tab[row])
        r = recs[o:o + n]
        out.append(V.boundary_support(zip(r["start"].tolist(), r["end"].tolist(), r["bits"].tolist()), ln, b, case["F"]))
    return out


def restated(case, mutant=None):
    """sorted starts, searchsorted; ``mutant``: one line changed"""
    tab, recs = X.table(case), X.records(case)
    F, out = case["F"], []
    keep_mask = (0x04 | 0x10) if mutant == "bit_dropped" else (0x04 | 0x01 | 0x10)
    for row, b in case["boundaries"]:
        o, n, span, _, ln = (int(v) for v in tab[row])
        r = recs[o:o + n]
        start, end, bits = r["start"].astype(np.int64), r["end"].astype(np.int64), r["bits"].astype(np.int64)
        pl, pr1 = b - F, b + F                                                   # the left base, and one past the right base
        if mutant == "int32":
            pr1 = (pr1 + 2 ** 31) % 2 ** 32 - 2 ** 31
        if mutant == "span_ignored":
            span = 100                                                           # (the read length instead of the table's max span)
        i0, i1 = np.searchsorted(start, pl - span + 1, "left"), np.searchsorted(start, pr1, "left")
        s, e, x = start[i0:i1], end[i0:i1], bits[i0:i1] & (0x04 | 0x01 | 0x10)
        kept = (bits[i0:i1] & keep_mask) == 0
        real = e > s
        if mutant != "no_clamp":
            e = np.minimum(e, ln)
        l = real & ((s < pl) if mutant == "left_lt" else (s <= pl)) & (pl < e) & (pl >= 0)
        rr = real & ((s < pr1 - 1) if mutant == "right_lt" else (s <= pr1 - 1)) & (pr1 - 1 < e) & (pr1 <= ln)
        left, right = int((kept & l).sum()), int((kept & rr).sum())
        span_n = min(left, right) if mutant == "span_min" else int((kept & l & rr).sum())
        out.append((left, right, span_n, int(((x == 0x10) & l & rr).sum())))
    return out


@pytest.mark.parametrize("case", X.KERNEL_CASES, ids=[c["name"] for c in X.KERNEL_CASES])
def test_kernel_cases_definition_restatement_and_claim_agree(case):
    assert definition(case) == case["expect"], case["claims"]
    assert restated(case) == case["expect"], case["claims"]


def test_the_stated_kernel_cases():
    assert X.N_KERNEL_CASES == 30 and X.JS_WAVES == 4 and X.JS_MAX_FLANK == 1000
    assert max(len(X.records(c)) for c in X.KERNEL_CASES) < 10000
    # the starts of every contig ascend, as a coordinate-sorted file gives them
    for c in X.KERNEL_CASES:
        for _, recs in c["contigs"]:
            assert all(a[0] <= b[0] for a, b in zip(recs, recs[1:])), c["name"]


MUTANTS = [("left_lt", "edges"), ("right_lt", "edges"), ("no_clamp", "edges"), ("span_min", "edges"), ("span_ignored", "bracket"), ("bit_dropped", "filter"),
           ("int32", "overflow"), ("right_lt", "bracket")]


@pytest.mark.parametrize("mutant,family", MUTANTS, ids=["%s in %s" % m for m in MUTANTS])
def test_a_departure_of_the_restatement_is_noticed_in_its_family(mutant, family):
    cases = [c for c in X.KERNEL_CASES if c["family"] == family]
    assert cases and any(restated(c, mutant) != c["expect"] for c in cases)


def test_the_l_boundary_at_P_is_noticed():
    """an R site at P cuts behind base P (b = P), an L site at P in front of it (b = P - 1): the definition's boundaries are the claimed ones and give
    the claimed counts; with the L boundary at P the read that ends with the last base asked for no longer spans"""
    c = X.SITE_CASE
    event = {"tid_r": c["R"][0], "P_r": c["R"][1], "tid_l": c["L"][0], "P_l": c["L"][1]}
    assert V.boundaries_of([event]) == c["boundaries"]
    assert definition(c) == c["expect"] and restated(c) == c["expect"]
    wrong = dict(c, boundaries=[c["R"], c["L"]])
    assert definition(wrong) != c["expect"] and definition(wrong)[1] == (2, 1, 1, 0)


# ---- rows in, records out --------------------------------------------------------------------------------------------------
def _file(case, tmp_path):
    counts, events = V.events_of(case["align"], case["far"], case["ins"])
    support = case["support"] or [(0, 0, 0, 0)] * (2 * len(events))
    assert len(support) == len(V.boundaries_of(events))
    records = V.records_of(events, support, X.NAMES)
    path = str(tmp_path / "out.clips.vcf")
    V.write_file(path, V.header_parts(BAM_HEADER, "sample", "test"), 10, V.finish_counts(counts, events, records), records)
    return counts, open(path).read().split("\n")


@pytest.mark.parametrize("case", X.JUNCTION_CASES, ids=[c["name"] for c in X.JUNCTION_CASES])
def test_junction_cases_records_and_counters_equal_the_literal_text(case, tmp_path):
    counts, lines = _file(case, tmp_path)
    assert lines[-1] == ""
    body = [l for l in lines[:-1] if not l.startswith("#")]
    assert body == case["lines"], case["claims"]
    assert counts == case["counts"]
    assert [l for l in lines if l.startswith("##clips_vcf_")] == ["##clips_vcf_flank=10"] + ["##clips_vcf_%s=%d" % (k, case["counts"][k]) for k in V.SN]


def test_the_stated_junction_cases_and_the_header(tmp_path):
    assert X.N_JUNCTION_CASES == 42
    _, lines = _file(X.JUNCTION_CASES[-1], tmp_path)
    assert X.JUNCTION_CASES[-1]["name"] == "an empty job" and lines[0] == "##fileformat=VCFv4.1" and lines[-1] == "" and all(l.startswith("#") for l in lines[:-1])
    assert [l for l in lines if l.startswith("##contig=")] == ["##contig=<ID=chrA,length=12000>", "##contig=<ID=chrB,length=8000>"]
    assert lines[-2] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample" and lines[-3].startswith('##TIDDITcmd="')
    # a header line for every key a record can use
    used_info = {kv.split("=")[0] for c in X.JUNCTION_CASES for l in c["lines"] for kv in l.split("\t")[7].split(";")}
    declared = {l.split("ID=")[1].split(",")[0] for l in lines if l.startswith("##INFO=")}
    assert used_info <= declared
    assert {l.split("ID=")[1].split(",")[0] for l in lines if l.startswith("##FORMAT=")} == set(X.FMT.split(":"))
    assert {l.split("ID=")[1].split(",")[0] for l in lines if l.startswith("##FILTER=")} == {"Ambiguous"}
    assert {l.split("ID=")[1].split(",")[0] for l in lines if l.startswith("##ALT=")} == {"DEL", "DUP", "INS", "BND"}


# ---- planted events through the real definitions --------------------------------------------------------------------------------------
def _info(line):
    return dict(kv.split("=") for kv in line.split("\t")[7].split(";"))


def _planted(cases, word):
    out = [c for c in cases if c["family"] == "events" and word in c["name"]]
    assert len(out) == 4                                                        # HOM 0, 1, 5 and 28
    return out


@pytest.mark.parametrize("source", ["align", "far"])
def test_planted_deletions_come_out_left_aligned(source):
    """clip_align_cases / clip_far_cases cut bases 401 ... 600 out of the sample, with 0, 1, 5 and 28 bases of microhomology: POS 400, END 600"""
    mod = CA if source == "align" else CF
    for c, h in zip(_planted(mod.CASES, "deletion"), (0, 1, 5, 28)):
        _, _, rows = mod.definition(c)
        counts, events = V.events_of(**{source + "_rows": rows})
        assert counts["junctions"] == 1 and len(events) == 1, c["name"]
        (_, line), = V.records_of(events, [(0, 0, 0, 0)] * 2, ["c0", "c1"])
        f, info = line.split("\t"), _info(line)
        assert (f[0], f[1], f[4]) == ("c1", "400", "<DEL>") and info["END"] == "600" and info["SVLEN"] == "-200" and info["HOMLEN"] == str(h) and info["CIPOS"] == "0,%d" % h
        assert int(info["END"]) - int(f[1]) == 200 and info["SRC"] == source


def test_planted_duplications_come_out_left_aligned():
    """clip_align_cases duplicates bases 400 ... 599 in tandem: POS 399 (the base in front), END 599"""
    for c, h in zip(_planted(CA.CASES, "duplication"), (0, 1, 5, 28)):
        _, _, rows = CA.definition(c)
        counts, events = V.events_of(align_rows=rows)
        assert counts["junctions"] == 1 and len(events) == 1, c["name"]
        (_, line), = V.records_of(events, [(0, 0, 0, 0)] * 2, ["c0", "c1"])
        f, info = line.split("\t"), _info(line)
        assert (f[0], f[1], f[4]) == ("c1", "399", "<DUP>") and info["END"] == "599" and info["SVLEN"] == "200" and info["HOMLEN"] == str(h)


def test_planted_translocations_come_out_left_aligned():
    """clip_far_cases joins A[... 400] to B[601 ...]: the record on A at 400 with B:601 behind it, the record on B at 601 with A:400 in front; the decoy
    row of the HOM 5 case has no mate"""
    for c, h in zip(_planted(CF.CASES, "translocation"), (0, 1, 5, 28)):
        _, _, rows = CF.definition(c)
        counts, events = V.events_of(far_rows=rows)
        assert counts["junctions"] == 1 and counts["one_sided"] == (1 if h == 5 else 0) and counts["not_mutual"] == 0, c["name"]
        (_, a), (_, b) = V.records_of(events, [(0, 0, 0, 0)] * 2, ["A", "B"])
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:5] == ["A", "400", "CLIP_1_1", "N", "N[B:601["] and fb[:5] == ["B", "601", "CLIP_1_2", "N", "]A:400]N"]
        assert _info(a)["HOMLEN"] == str(h) and _info(a)["MATEID"] == "CLIP_1_2" and _info(b)["MATEID"] == "CLIP_1_1"


# ---- the genotype rule and the switch --------------------------------------------------------------------------------------------
def test_the_genotype_cuts():
    assert [V.genotype("DEL", a, r) for a, r in ((9, 3), (8, 3), (3, 1), (3, 2), (6, 0))] == ["1/1", "0/1", "1/1", "0/1", "1/1"]
    assert [V.genotype(t, 9, 3) for t in ("BND", "INS")] == ["1/1", "1/1"] and [V.genotype(t, 8, 3) for t in ("BND", "INS")] == ["0/1", "0/1"]
    assert [V.genotype("DUP", a, r) for a, r in ((5, 7), (5, 8), (10, 14), (10, 15))] == ["1/1", "0/1", "1/1", "0/1"]


def test_the_switch():
    assert V.parse_switch(None) is None and V.parse_switch("") is None
    assert V.parse_switch("1") == 10 and V.parse_switch("2") == 2 and V.parse_switch("25") == 25 and V.parse_switch("1000") == 1000
    for bad, text in (("0", "the switch is 1 or F"), ("1001", "the flank is 2 ... 1000"), ("01", "the switch is 1 or F"), ("yes", "the switch is 1 or F"),
                      ("10:2", "the switch is 1 or F"), ("-5", "the switch is 1 or F"), ("1" * 10, "the switch is 1 or F"), ("١٠", "the switch is 1 or F")):
        with pytest.raises(ValueError, match=text):
            V.parse_switch(bad)
    with pytest.raises(ValueError, match="TIDDIT_CLIPS, which is not set"):
        V.parse_switch("1", clips=False, stages=False)
    with pytest.raises(ValueError, match="none of which is set"):
        V.parse_switch("1", clips=True, stages=False)
    assert V.parse_switch("", clips=False, stages=False) is None


def test_the_summary_line():
    counts = dict(X.ZERO, junctions=3, both_sources=1, ins_rows=2, records=6, one_sided=4)
    assert V.summary_line(counts) == ("clips vcf: 3 junctions (1 from both stages, 0 disagree), 2 insertions (0 explained by a junction), 6 records (0 events ambiguous), "
                                      "rows without a record: 4 one-sided, 0 not mutual, 0 inv")
