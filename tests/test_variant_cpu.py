"""The variant stage's host layer without a GPU: the VCF header, and the typing / filter / genotype / QUAL layer of
tiddit_amd.tiddit_variant fed the evidence the compiled reference recorded (tests/golden/sv_vcf*.json, made by
tests/golden/make_golden_vcf.py: every get_region call with its result, the three coverage means of every candidate) —
the VCF body must come out byte for byte.  Small hand-built cases pin the reference's visible quirks."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import pytest

FIXTURES = ["sv_vcf_small.json", "sv_vcf.json", "sv_vcf_grch38.json"]


def body_of(fx):
    return "".join(l + "\n" for l in fx["vcf_records"])


def evidence_of(fx):
    """the fixture -> (candidates as tiddit_cluster.main shapes them, the fields define_variant reads; means keyed like
    tiddit_region.candidate_means; get_region results keyed (chrom, start, end, bp))"""
    cols = fx["meta"]["candidate_columns"]
    sample = fx["meta"]["sample_id"]
    cand, means = {}, {}
    for row in fx["candidates"]:
        r = dict(zip(cols, row))
        c = {k: r[k] for k in ("posA", "posB", "startA", "endA", "startB", "endB", "N_discordants", "N_splits", "N_contigs")}
        for side in ("A", "B"):
            c["positions_" + side] = {k: r["%s_%s" % (k, side)] for k in ("orientation_discordants", "orientation_splits", "orientation_contigs")}
        c["sample_splits"] = {sample: set(range(r["n_sample_splits"]))}           # (only their sizes are read)
        c["sample_discordants"] = {sample: set(range(r["n_sample_discordants"]))}
        c["contigs"] = []
        cand.setdefault(r["chrA"], {}).setdefault(r["chrB"], {})[r["cluster"]] = c
        means[(r["chrA"], r["chrB"], r["cluster"])] = {"avg_a": np.float64(r["avg_a"]), "avg_b": np.float64(r["avg_b"]), "covM": r["covM"]}
    regions = {(c[0], c[1], c[2], c[3]): tuple(c[6]) for c in fx["get_region_calls"]}
    return cand, means, regions


def args_of(fx, **over):
    a = dict(fx["meta"]["args"])
    a.update(over)
    return argparse.Namespace(**a)


def contigs_of(fx):
    from tiddit_amd import synth_bam
    return synth_bam.contigs_for(fx["meta"]["params"])


@pytest.fixture(scope="module", params=FIXTURES)
def fx(request, golden_dir):
    return json.load(open(os.path.join(golden_dir, request.param)))


def test_fixture_is_consistent(fx):
    body = body_of(fx)
    assert hashlib.sha256(body.encode()).hexdigest() == fx["vcf_body_sha256"]
    assert len(fx["vcf_records"]) == fx["meta"]["n_records"] > 0


def test_header_equals_reference(fx):
    from tiddit_amd import tiddit_vcf_header
    m = fx["meta"]
    header = {"SQ": [{"SN": n, "LN": ln} for n, ln in contigs_of(fx)]}
    lines = tiddit_vcf_header.main(header, m["library"], m["sample_id"], m["version"]).split("\n")
    cmd = [l for l in lines if l.startswith("##TIDDITcmd=")]
    assert cmd == ['##TIDDITcmd="' + " ".join(sys.argv) + '"']
    head = [l for l in lines if not l.startswith("##TIDDITcmd=")]
    assert [l for l in head if not l.startswith("##contig=")] == fx["vcf_header_other_lines"]
    assert hashlib.sha256("\n".join(head).encode()).hexdigest() == fx["vcf_header_sha256"]


def test_typing_layer_reproduces_the_body(fx):
    from tiddit_amd import tiddit_variant
    m = fx["meta"]
    cand, means, regions = evidence_of(fx)
    variants = tiddit_variant.type_variants(cand, args_of(fx), m["library"], [m["sample_id"]], m["max_ins_len"], {}, means, regions)
    assert tiddit_variant.vcf_body([n for n, _ in contigs_of(fx)], variants) == body_of(fx)


def test_queries_are_the_reference_calls(fx):
    """the pre-filters pick exactly the get_region calls the reference made, in its order (duplicates included)"""
    from tiddit_amd import tiddit_variant
    m = fx["meta"]
    cand, means, regions = evidence_of(fx)
    args = args_of(fx)
    q = []
    for chrA in cand:
        for chrB, cid, c, posA, posB, _, _ in tiddit_variant.survivors(chrA, cand, args, m["library"], means):
            q += tiddit_variant.region_queries(chrA, chrB, c, posA, posB)
    assert q == [tuple(c[:4]) for c in fx["get_region_calls"]]
    assert all(c[4] == m["min_mapq"] and int(c[5]) == int(m["max_ins_len"]) for c in fx["get_region_calls"])   # (get_region truncates: int max_ins)


# ---- hand-built cases ----------------------------------------------------------------------------------------------------
LIB = {"avg_coverage": 30.0, "avg_coverage_chr1": 30.0, "avg_coverage_chr2": 30.0, "contig_ploidy_chr1": 2, "contig_ploidy_chr2": 2}


def _args(**over):
    a = dict(p=3, r=3, z=50, n=2, max_coverage=4.0, p_ratio=0.1, r_ratio=0.1, skip_assembly=True)
    a.update(over)
    return argparse.Namespace(**a)


def _cand(posA, posB, startA, endA, startB, endB, nd=6, ns=0, oa=None, ob=None):
    oa = oa if oa is not None else ["+"] * nd
    ob = ob if ob is not None else ["-"] * nd
    return {"posA": posA, "posB": posB, "startA": startA, "endA": endA, "startB": startB, "endB": endB, "N_discordants": nd, "N_splits": ns,
            "N_contigs": 0, "positions_A": {"orientation_discordants": oa, "orientation_splits": [], "orientation_contigs": []},
            "positions_B": {"orientation_discordants": ob, "orientation_splits": [], "orientation_contigs": []},
            "sample_splits": {"S": set()}, "sample_discordants": {"S": set(range(nd))}, "contigs": []}


def _run(cands, means, regions, **argover):
    from tiddit_amd import tiddit_variant
    return tiddit_variant.type_variants(cands, _args(**argover), LIB, ["S"], 500, {}, means, regions)


def test_bnd_lfb_repeats_a_and_not_inverted_and_covm_int_zero():
    c = _cand(1000, 5000, 900, 1000, 5000, 5100, oa=["+"] * 6, ob=["+"] * 6)       # all pairs "inverted": still no inverted alt form
    cands = {"chr1": {"chr2": {"0": c}}}
    means = {("chr1", "chr2", "0"): {"avg_a": np.float64(30.0), "avg_b": np.float64(30.0), "covM": 0}}
    regions = {("chr1", 900, 1000, 1000): (30.0, 0.0, 7, 1, 20, 25), ("chr2", 5000, 5100, 5000): (31.0, 0.01, 9, 2, 21, 26)}
    v = _run(cands, means, regions)
    a, b = v["chr1"][0][1], v["chr2"][0][1]
    assert a[4] == "N[chr2:5000[" and b[4] == "]chr1:1000]N"            # posA == endA: "not before"
    assert "LFA=7,1;LFB=7,1;" in a[7] and a[7] == b[7]
    assert a[9].split(":")[2] == "30.0,0,31.0"                           # covM is the int 0
    assert a[2] == "SV_1_1" and b[2] == "SV_1_2" and a[1] == "1000" and b[1] == "5000"


def test_zero_mean_divides_to_inf_not_an_error():
    c = _cand(1000, 9000, 900, 1000, 9000, 9100)
    cands = {"chr1": {"chr1": {"0": c}}}
    means = {("chr1", "chr1", "0"): {"avg_a": np.float64(0.0), "avg_b": np.float64(30.0), "covM": np.float64(15.0)}}
    regions = {("chr1", 900, 1000, 1000): (30.0, 0, 7, 1, 20, 25), ("chr1", 9000, 9100, 9000): (30.0, 0, 7, 1, 20, 25)}
    with np.errstate(divide="ignore"):
        v = _run(cands, means, regions)
    assert len(v["chr1"]) == 1
    assert v["chr1"][0][1][9].split(":")[5] == "0,0"                    # frac_low_q is the int 0 without reads


def test_stable_order_and_chra_order():
    c1, c2 = _cand(2000, 9000, 1900, 2000, 9000, 9100), _cand(2000, 12000, 1900, 2000, 12000, 12100)
    cands = {"chr1": {"chr1": {"0": c1, "1": c2}}}
    m = {"avg_a": np.float64(30.0), "avg_b": np.float64(30.0), "covM": np.float64(14.0)}
    means = {("chr1", "chr1", "0"): m, ("chr1", "chr1", "1"): m}
    r = (30.0, 0.0, 7, 1, 20, 25)
    regions = {("chr1", 1900, 2000, 2000): r, ("chr1", 9000, 9100, 9000): r, ("chr1", 12000, 12100, 12000): r}
    from tiddit_amd import tiddit_variant
    v = _run(cands, means, regions)
    body = tiddit_variant.vcf_body(["chr1"], v).splitlines()
    assert [l.split("\t")[2] for l in body] == ["SV_1_1", "SV_2_1"]       # equal positions keep the candidates' order
    assert all(l.split("\t")[4] == "<DEL>" for l in body)


def test_percentiles_empty_and_scoring():
    from tiddit_amd import tiddit_variant
    assert tiddit_variant.percentile([], [1, 50, 99]) == [0, 0, 0]
    assert tiddit_variant.percentile([0.5, 0.1, 0.9], [1, 50, 99]) == [0.1, 0.5, 0.9]
    zero = {k: [0] * 16 for k in ("FA", "FB", "RA", "RB")}
    d = {"n_contigs": 0, "n_discordants": 3, "n_splits": 0, "refFA": 0, "refFB": 3, "refRA": 0, "refRB": 0}
    assert tiddit_variant.scoring(d, zero) == 80
    assert tiddit_variant.finish({"chr1": {}}, []) == {"chr1": []}


def test_skip_assembly_ctg_dot(fx):
    assert all("CTG=.\t" in l or ";CTG=." in l for l in fx["vcf_records"])
