"""TIDDIT_GENOTYPE without a GPU: the sites parser (every ALT form, END, regions present / absent / not matching the breakpoints,
windows clipped at 1 and at the contig length, the refused files), the pure evidence-to-column function pinned to every record of
the compiled reference's VCFs (tests/golden/sv_vcf*.json: the get_region results and means the fixture recorded, DV / RV from LTE),
the two link-count references against each other and against their four mutants, the flip of sites, the header."""
import argparse
import json
import os

import numpy as np
import pytest

import genotype_cases as GC

FIXTURES = ["sv_vcf_small.json", "sv_vcf.json", "sv_vcf_grch38.json"]
NUM = {"chr1": 0, "chr2": 1, "chr10": 2}
LEN = {"chr1": 100_000, "chr2": 50_000, "chr10": 80_000}
W = 500


def _rec(chrom, pos, alt, info, no=1):
    return (no, [chrom, str(pos), "SV_1_1", "N", alt, "10", "PASS", info, "GT", "./."])


def _site(chrom, pos, alt, info, w=W):
    from tiddit_amd import tiddit_genotype as G
    return G.site_of(*_rec(chrom, pos, alt, info), NUM, LEN, w)


# ---- the parser -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alt", ["N[chr2:2000[", "]chr2:2000]N", "N]chr2:2000]", "[chr2:2000[N"])
def test_every_break_end_form_names_the_mate(alt):
    site, rule = _site("chr1", 5000, alt, "SVTYPE=BND")
    assert rule == "window"
    assert site == ("chr1", 5000, "chr2", 2000, 4500, 5500, 1500, 2500, "BND")


def test_symbolic_alt_takes_end():
    site, rule = _site("chr1", 5000, "<DUP:TANDEM>", "SVTYPE=DUP:TANDEM;SVLEN=3000;END=8000")
    assert (site, rule) == (("chr1", 5000, "chr1", 8000, 4500, 5500, 7500, 8500, "DUP:TANDEM"), "window")


def test_regions_present_keep_the_info_orientation_on_both_records_of_a_pair():
    info = "SVTYPE=BND;REGIONA=4800,5000;REGIONB=2000,2300;LFA=3,1"
    first = _site("chr1", 5000, "N[chr2:2000[", info)
    second = _site("chr2", 2000, "]chr1:5000]N", info)
    assert first == second == (("chr1", 5000, "chr2", 2000, 4800, 5000, 2000, 2300, "BND"), "regions")


def test_regions_on_one_contig_with_the_own_breakpoint_in_region_b():
    info = "SVTYPE=BND;REGIONA=4800,5000;REGIONB=9000,9300"
    assert _site("chr1", 9100, "]chr1:4900]N", info) == (("chr1", 4900, "chr1", 9100, 4800, 5000, 9000, 9300, "BND"), "regions")
    # either assignment fits (overlapping regions): the record's own breakpoint is A
    info = "SVTYPE=DEL;END=5100;REGIONA=4800,5200;REGIONB=4900,5300"
    assert _site("chr1", 5000, "<DEL>", info)[0][:4] == ("chr1", 5000, "chr1", 5100)


def test_regions_on_two_contigs_fitting_both_ways_follow_the_name_order():
    info = "SVTYPE=BND;REGIONA=1000,3000;REGIONB=1500,3500"
    a = _site("chr10", 2000, "N[chr2:2500[", info)
    b = _site("chr2", 2500, "]chr10:2000]N", info)
    assert a == b and a[0][:4] == ("chr10", 2000, "chr2", 2500) and "chr10" < "chr2"


def test_regions_not_matching_the_breakpoints_fall_back_to_the_window():
    info = "SVTYPE=BND;REGIONA=100,200;REGIONB=2000,2300"
    site, rule = _site("chr1", 5000, "N[chr2:2000[", info)
    assert rule == "missed" and site == ("chr1", 5000, "chr2", 2000, 4500, 5500, 1500, 2500, "BND")
    # one region alone is no pair of regions
    assert _site("chr1", 5000, "N[chr2:2000[", "SVTYPE=BND;REGIONA=4800,5000")[1] == "window"


def test_windows_are_clipped_at_one_and_at_the_contig_length():
    site, _ = _site("chr1", 300, "N[chr2:49800[", "SVTYPE=BND")
    assert site[4:8] == (1, 800, 49_300, 50_000)
    site, _ = _site("chr1", 300, "N[chr2:49800[", "SVTYPE=BND", w=534.0)            # (the library's percentile is a float)
    assert site[4:8] == (1, 834, 49_266, 50_000)


def test_read_sites_from_a_file(tmp_path):
    from tiddit_amd import tiddit_genotype as G
    p = tmp_path / "s.vcf"
    p.write_text("##fileformat=VCFv4.1\n##INFO=<ID=FOO,Number=1,Type=String,Description=\"x\">\n#CHROM\tPOS\n"
                 + "\t".join(_rec("chr1", 5000, "<DEL>", "SVTYPE=DEL;END=9000")[1]) + "\n\n"
                 + "\t".join(_rec("chr2", 70, "[chr10:600[N", "SVTYPE=BND")[1][:8]) + "\n")
    assert G.read_sites(str(p), NUM, LEN, W) == [("chr1", 5000, "chr1", 9000, 4500, 5500, 8500, 9500, "DEL"),
                                                ("chr2", 70, "chr10", 600, 1, 570, 100, 1100, "BND")]
    meta, records = G.parse_vcf(str(p))
    assert len(meta) == 2 and [no for no, _ in records] == [4, 6]


@pytest.mark.parametrize("cols, word", [
    (["chr1", "5000", "x", "N", "<DEL>", ".", "PASS"], "columns"),
    (["chr1", "5000", "x", "N", "<DEL>", ".", "PASS", "SVTYPE=DEL"], "END"),
    (["chr1", "5000", "x", "N", "<DEL>", ".", "PASS", "SVTYPE=DEL;END=9k"], "END"),
    (["chr1", "pos", "x", "N", "<DEL>", ".", "PASS", "SVTYPE=DEL;END=9000"], "POS"),
    (["chr1", "5000", "x", "N", "<DEL>", ".", "PASS", "END=9000"], "SVTYPE"),
    (["chr1", "5000", "x", "N", "ACGT", ".", "PASS", "SVTYPE=INS;END=5000"], "ALT"),
    (["chr1", "5000", "x", "N", "N[chr2:2000]", ".", "PASS", "SVTYPE=BND"], "ALT"),
    (["chr1", "5000", "x", "N", "N[chr2:2000[", ".", "PASS", "SVTYPE=BND;REGIONA=1;REGIONB=2,3"], "REGIONA"),
    (["chr1", "5000", "x", "N", "N[chr2:2000[", ".", "PASS", "SVTYPE=BND;REGIONA=9,1;REGIONB=2,3"], "REGIONA"),
    (["chr1", "5000", "x", "N", "N[chr2:60000[", ".", "PASS", "SVTYPE=BND"], "outside"),
    (["chr3", "5000", "x", "N", "N[chr2:2000[", ".", "PASS", "SVTYPE=BND"], "chr3"),
    (["chr1", "5000", "x", "N", "N[chrUn:2000[", ".", "PASS", "SVTYPE=BND"], "chrUn"),
])
def test_a_malformed_record_is_an_error_that_names_its_line(tmp_path, cols, word):
    from tiddit_amd import tiddit_genotype as G
    p = tmp_path / "bad.vcf"
    good = "\t".join(_rec("chr1", 5000, "<DEL>", "SVTYPE=DEL;END=9000")[1])
    p.write_text("##fileformat=VCFv4.1\n#CHROM\n" + good + "\n" + "\t".join(cols) + "\n" + good + "\n")
    with pytest.raises(G.SitesError) as e:
        G.read_sites(str(p), NUM, LEN, W)
    assert "line 4" in str(e.value) and word in str(e.value) and "\n" not in str(e.value)


def test_gz_and_missing_files_are_refused_in_one_line(tmp_path):
    from tiddit_amd import tiddit_genotype as G
    (tmp_path / "s.vcf.gz").write_bytes(b"\x1f\x8b")
    for name in ("s.vcf.gz", "nothing.vcf"):
        with pytest.raises(G.SitesError) as e:
            G.read_sites(str(tmp_path / name), NUM, LEN, W)
        assert "\n" not in str(e.value) and name in str(e.value)


# ---- the column, pinned to the compiled reference ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=FIXTURES)
def fx(request, golden_dir):
    return json.load(open(os.path.join(golden_dir, request.param)))


def test_sample_column_equals_every_record_of_the_reference(fx):
    """every record, none excluded: the site the parser makes of the record, the get_region results and the mean the fixture recorded
    for it, DV / RV from the record's LTE (one sample, no contigs: the sample's counts are the candidate's) -> the record's own
    sample column, byte for byte"""
    from tiddit_amd import tiddit_genotype as G
    m = fx["meta"]
    number, length, records, regions, between = GC.golden_evidence(fx)
    sites, rules = G.sites_of(records, number, length, m["max_ins_len"])
    assert len(sites) == len(fx["vcf_records"]) == m["n_records"] and set(rules) == {"regions"}
    args = argparse.Namespace(**m["args"])
    pair = {}
    for (no, cols), site in zip(records, sites):
        assert all(q in regions for q in G.site_queries(site)), (no, site)           # the reference made exactly these calls
        dv, rv = (int(x) for x in G._info(cols[7])["LTE"].split(","))
        got = G.sample_column(site, regions, between[(site[0], site[2]) + site[4:8]], dv, rv, args, m["library"])
        assert got == cols[9], (no, cols[:5])
        assert cols[8] == "GT:CN:COV:DV:RV:LQ:RR:DR"
        pair.setdefault(cols[2].rsplit("_", 1)[0], []).append(site)
    assert any(len(v) == 2 for v in pair.values())
    assert all(v[0] == v[1] for v in pair.values() if len(v) == 2)                   # both records of a break-end pair: one site


def test_sample_column_overrides_and_interchromosomal_cn():
    from tiddit_amd import tiddit_genotype as G
    lib = {"avg_coverage": 30.0, "avg_coverage_chr1": 30.0, "avg_coverage_chr2": 0.0, "contig_ploidy_chr1": 2, "contig_ploidy_chr2": 2}
    args = argparse.Namespace(p=3, r=3, n=2)
    r = (30.0, 0.0, 7, 1, 20, 25)
    site = ("chr1", 2000, "chr1", 9000, 1900, 2000, 9000, 9100, "DEL")
    regions = {("chr1", 1900, 2000, 2000): r, ("chr1", 9000, 9100, 9000): r}
    assert G.sample_column(site, regions, 14.0, 0, 0, args, lib).startswith("0/1:1:30.0,14.0,30.0:0:0:")     # DEL: by the copy number
    assert G.sample_column(site, regions, 1.0, 9, 9, args, lib).startswith("1/1:0:")
    assert G.sample_column(site[:8] + ("DUP:TANDEM",), regions, 61.0, 0, 0, args, lib).startswith("1/1:4:")
    assert G.sample_column(site[:8] + ("INV",), regions, 30.0, 0, 0, args, lib).startswith("./.:2:")         # no support, no override
    assert G.sample_column(site[:8] + ("INV",), regions, 30.0, 3, 0, args, lib).startswith("0/1:2:")
    assert G.sample_column(site[:8] + ("INV",), regions, 30.0, 300, 0, args, lib).startswith("1/1:2:")       # refFA < 0.1 * DV
    bnd = ("chr1", 2000, "chr2", 9000, 1900, 2000, 9000, 9100, "DEL")                 # (a foreign type on two contigs: CN '.', no override)
    regions[("chr2", 9000, 9100, 9000)] = r
    assert G.sample_column(bnd, regions, None, 0, 4, args, lib).startswith("0/1:.:30.0,0,30.0:0:4:")
    near = ("chr2", 2000, "chr2", 2500, 1900, 2000, 2500, 2600, "BND")                # covM from the middle region; avg 0: the -n branch
    regions.update({("chr2", 1900, 2000, 2000): r, ("chr2", 2500, 2600, 2500): r, ("chr2", 2000, 2500, 2000): (45.0, 0, 0, 0, 0, 0)})
    assert G.sample_column(near, regions, None, 0, 0, args, lib).startswith("./.:3:30.0,45.0,30.0:")
    assert G.site_queries(near)[2] == ("chr2", 2000, 2500, 2000)


# ---- the link-count references ------------------------------------------------------------------------------------------------
def test_loop_and_numpy_references_agree_and_every_mutant_is_told_apart():
    posA, posB, kind, off, sites = GC.small_table()
    want = GC.link_counts_loop(posA, posB, kind, off, sites)
    assert np.array_equal(GC.link_counts_numpy(posA, posB, kind, off, sites), want)
    assert want.sum() > 0 and (want[:, 0] > 0).any() and (want[:, 1] > 0).any()
    assert not want[0].any()                                                         # bucket -1
    for b in GC.BOUNDS:
        loop = GC.link_counts_loop(posA, posB, kind, off, sites, strict=(b,))
        assert np.array_equal(GC.link_counts_numpy(posA, posB, kind, off, sites, strict=(b,)), loop)
        assert not np.array_equal(loop, want), b                                     # `<` for `<=` in this one comparison shows


def test_numpy_reference_on_the_large_table_tells_the_mutants_apart_too():
    posA, posB, kind, off, sites = GC.large_table(n_big=200_003)
    want = GC.link_counts_numpy(posA, posB, kind, off, sites)
    few = sites[:4] + sites[4:40:7]
    assert np.array_equal(GC.link_counts_loop(posA, posB, kind, off, few)[4:], GC.link_counts_numpy(posA, posB, kind, off, few)[4:])
    assert int(want[0].sum()) == 200_003 and want[1].sum() == 65 and want[2].sum() == 1 and not want[3].any()
    for b in GC.BOUNDS:
        assert not np.array_equal(GC.link_counts_numpy(posA, posB, kind, off, sites, strict=(b,)), want), b


def test_contig_kind_rows_count_in_neither():
    posA, posB = np.array([10, 10, 10], dtype=np.int32), np.array([20, 20, 20], dtype=np.int32)
    kind, off = np.array([0, 1, 2], dtype=np.uint8), np.array([0, 3])
    for f in (GC.link_counts_loop, GC.link_counts_numpy):
        assert f(posA, posB, kind, off, [(0, 10, 10, 20, 20)]).tolist() == [[1, 1]]


def test_link_rows_flip_sites_to_the_table_order():
    from tiddit_amd import tiddit_genotype as G
    bucket = {(0, 1): 0, (2, 2): 1}
    sites = [("chr1", 5, "chr2", 9, 1, 6, 7, 10, "BND"), ("chr2", 9, "chr1", 5, 7, 10, 1, 6, "BND"), ("chr10", 5, "chr10", 9, 1, 6, 7, 10, "DEL"),
             ("chr2", 5, "chr10", 9, 1, 6, 7, 10, "BND")]
    assert G.link_rows(sites, bucket, NUM) == [(0, 1, 6, 7, 10), (0, 1, 6, 7, 10), (1, 1, 6, 7, 10), (-1, 1, 6, 7, 10)]
    turned = G._lower_first([("chr1", 900, "chr1", 100, 400, 1400, 1, 600, "BND")] * 2, ["window", "regions"])
    assert turned[0] == ("chr1", 100, "chr1", 900, 1, 600, 400, 1400, "BND") and turned[1][1] == 900


def test_header_takes_the_inputs_unknown_lines_and_states_the_rule():
    from tiddit_amd import tiddit_genotype as G
    own = "##fileformat=VCFv4.1\n##ALT=<ID=DEL,Description=\"Deletion\">\n##INFO=<ID=END,Number=1,Type=Integer,Description=\"e\">\n#CHROM\tPOS\tID\tS1"
    meta = ["##fileformat=VCFv4.2", "##INFO=<ID=END,Number=1,Type=Integer,Description=\"other\">", "##INFO=<ID=VARID,Number=1,Type=String,Description=\"v\">",
            "##ALT=<ID=INS,Description=\"Insertion\">", "##FILTER=<ID=Mine,Description=\"f\">", "##contig=<ID=zz,length=3>",
            "##INFO=<ID=VARID,Number=1,Type=String,Description=\"again\">"]
    lines = G.header(own, meta, "sites.vcf", 534.0).split("\n")
    assert lines[:3] == own.split("\n")[:3] and lines[-1] == "#CHROM\tPOS\tID\tS1"
    assert lines[3:6] == [meta[2], meta[3], meta[4]]
    assert lines[6].startswith("##TIDDITgenotype=<sites=sites.vcf,window=") and "534" in lines[6] and len(lines) == 8
