"""The allele counts without a GPU: the definition (tiddit_alleles.count_read) and the numpy restatement of tests/alleles_cases.py
agree on every case, every claimed property holds, every one-line mutant of the restatement is caught inside the family that claims
it, and the host side — site reader, writer, switch parser — does what its docstrings say.

This file fails on the parent commit, which has no such module."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import alleles_cases as AC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_case_list():
    assert len(AC.CASES) == AC.N_CASES and len({c["name"] for c in AC.CASES}) == AC.N_CASES
    assert AC.FAMILIES == ["cigar", "contention", "filters", "malformed", "nibbles", "qualities", "sizes", "state", "tables"]
    assert sum(not c["reader_ok"] for c in AC.CASES) == 4 and all(c["family"] == "malformed" for c in AC.CASES if not c["reader_ok"])


@pytest.fixture(scope="module")
def results():
    return {c["name"]: (AC.expected(c), AC.reference(c), AC.definition(c)) for c in AC.CASES}


@pytest.mark.parametrize("case", AC.CASES, ids=[c["name"] for c in AC.CASES])
def test_definition_restatement_and_claim_agree(case, results):
    claim, ref, dfn = results[case["name"]]
    assert claim[0].any() or case["expect"] == {}
    for who, got in (("restatement", ref), ("definition", dfn)):
        bad = np.argwhere(got[0] != claim[0])
        assert not len(bad), (who, [(int(k), int(c), int(got[0][k, c]), int(claim[0][k, c])) for k, c in bad[:8]])
        assert got[1:] == claim[1:], (who, got[1:], claim[1:])


def test_padding_changes_nothing_for_well_formed_cases():
    """the records back to back (as a BAM holds them) count like the records with 64 KB behind the malformed one"""
    for c in AC.CASES:
        if c["family"] == "malformed" and c["reader_ok"]:
            a, b = AC.reference(c, padding=False), AC.reference(c, padding=True)
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
            assert len(AC.build(c, True).raw) - len(AC.build(c, False).raw) == AC.PAD


@pytest.mark.parametrize("mutant", sorted(AC.MUTANTS))
def test_every_mutant_is_caught_inside_its_family(mutant):
    family = AC.MUTANTS[mutant]
    caught = []
    for c in AC.CASES:
        if c["family"] == family:
            got, want = AC.reference(c, mutant), AC.expected(c)
            if not np.array_equal(got[0], want[0]) or got[1:] != want[1:]:
                caught.append(c["name"])
    assert caught, (mutant, family)


def test_malformed_padding_would_count_as_good_g():
    """what a missing bound would read: the padding byte is G G as sequence and a quality no min_bq refuses"""
    assert AC.PAD_BYTE >> 4 == 4 and AC.PAD_BYTE & 0xf == 4 and 93 >= AC.PAD_BYTE >= 13 and AC.PAD_BYTE != 0xff
    for c in AC.CASES:
        if c["family"] == "malformed":
            assert "G" not in c["expect"][(0, 105)] and "T" not in c["expect"][(0, 105)]


# ---- the site reader ------------------------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["chr1", "chr2", "chrM"], [1000, 500, 100]
VCF = "\n".join([
    "##fileformat=VCFv4.2",
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO",
    "chr2\t500\t.\tA\tg\t.\t.\t.",              # the last base of chr2, lower-case ALT
    "chr1\t10\trs1\tc\tT",                      # five columns are enough
    "chrX\t10\t.\tA\tC",                        # unknown contig
    "chr1\t0\t.\tA\tC",                         # POS < 1
    "chr2\t501\t.\tA\tC",                       # POS > LN
    "chr1\t20\t.\tA\tA",                        # REF == ALT
    "chr1\t20\t.\tAT\tA",                       # an indel
    "chr1\t20\t.\tA\tC,G",                      # multi-allelic
    "chr1\t20\t.\tN\tA",                        # not ACGT
    "chr1\t10\t.\tC\tA",                        # the same position again: shares the device site
    "chr1\t5\t.\tG\tC",
    "chrM\t1\t.\tT\tC",
    "chrX\t0\t.\tA\tA",                         # unknown contig is tested first
    ""])


@pytest.mark.parametrize("zipped", [False, True])
def test_site_reader(tmp_path, zipped):
    from tiddit_amd import tiddit_alleles
    path = str(tmp_path / ("sites.vcf.gz" if zipped else "sites.vcf"))
    with (gzip.open(path, "wt") if zipped else open(path, "w")) as f:
        f.write(VCF)
    s = tiddit_alleles.read_sites(path, NAMES, LENGTHS)
    assert s.skipped == {"unknown contig": 2, "position outside the contig": 2, "not a biallelic SNV": 4}
    assert [r[:4] for r in s.rows] == [("chr2", 500, "A", "G"), ("chr1", 10, "C", "T"), ("chr1", 10, "C", "A"), ("chr1", 5, "G", "C"),
                                       ("chrM", 1, "T", "C")]
    assert s.site_pos.dtype == np.int32 and s.site_pos.tolist() == [4, 9, 499, 0]
    assert s.site_off.dtype == np.int64 and s.site_off.tolist() == [0, 2, 3, 4]
    assert [r[4] for r in s.rows] == [2, 1, 1, 0, 3] and len(s) == 4


def test_site_reader_on_an_empty_file(tmp_path):
    from tiddit_amd import tiddit_alleles
    path = str(tmp_path / "none.vcf")
    open(path, "w").write("##fileformat=VCFv4.2\n")
    s = tiddit_alleles.read_sites(path, NAMES, LENGTHS)
    assert s.rows == [] and len(s) == 0 and s.site_off.tolist() == [0, 0, 0, 0]


# ---- the writer -----------------------------------------------------------------------------------------------------------------
def test_writer_bytes(tmp_path):
    from tiddit_amd import tiddit_alleles
    rows = [("chr2", 500, "A", "G", 2), ("chr1", 10, "C", "T", 1), ("chr1", 10, "C", "A", 1), ("chr1", 5, "G", "C", 0), ("chrM", 1, "T", "C", 3)]
    table = np.array([[0, 0, 0, 0, 3, 1, 2, 4],             # chr1:5    no G, no C: BAF .
                      [0, 7, 0, 0, 0, 0, 0, 0],             # chr1:10   all C: C>T 0.000000, C>A 0.000000
                      [0, 0, 5, 0, 0, 0, 0, 0],             # chr2:500  A>G all G: 1.000000
                      [0, 2, 0, 1, 0, 0, 0, 9]],            # chrM:1    T>C 2 / 3
                     dtype=np.uint32)
    path = str(tmp_path / "x.alleles.tab")
    tiddit_alleles.write_file(path, rows, table)
    assert open(path, "rb").read() == (
        b"#CHROM\tPOS\tREF\tALT\tA\tC\tG\tT\tN\tDEL\tSKIP\tLOWBQ\tREF_N\tALT_N\tBAF\n"
        b"chr2\t500\tA\tG\t0\t0\t5\t0\t0\t0\t0\t0\t0\t5\t1.000000\n"
        b"chr1\t10\tC\tT\t0\t7\t0\t0\t0\t0\t0\t0\t7\t0\t0.000000\n"
        b"chr1\t10\tC\tA\t0\t7\t0\t0\t0\t0\t0\t0\t7\t0\t0.000000\n"
        b"chr1\t5\tG\tC\t0\t0\t0\t0\t3\t1\t2\t4\t0\t0\t.\n"
        b"chrM\t1\tT\tC\t0\t2\t0\t1\t0\t0\t0\t9\t1\t2\t0.666667\n")


def test_summary_line(tmp_path):
    from tiddit_amd import tiddit_alleles
    path = str(tmp_path / "sites.vcf")
    open(path, "w").write(VCF)
    s = tiddit_alleles.read_sites(path, NAMES, LENGTHS)
    assert tiddit_alleles.summary_line(s, 12, 1) == ("allele counts: 5 sites accepted (4 device sites), rows skipped: 2 unknown contig, "
                                                     "2 position outside the contig, 4 not a biallelic SNV; reads used 12, malformed records 1")


# ---- the switch -----------------------------------------------------------------------------------------------------------------
def test_switch_parser(tmp_path):
    from tiddit_amd import tiddit_alleles
    path = str(tmp_path / "sites.vcf")
    open(path, "w").write(VCF)
    assert tiddit_alleles.parse_switch(None, None) is None and tiddit_alleles.parse_switch("", "7") is None
    assert tiddit_alleles.parse_switch(path, None) == (path, 13) and tiddit_alleles.parse_switch(path, "") == (path, 13)
    assert tiddit_alleles.parse_switch(path, "0") == (path, 0) and tiddit_alleles.parse_switch(path, "93") == (path, 93)
    with pytest.raises(ValueError):
        tiddit_alleles.parse_switch(str(tmp_path / "missing.vcf"), None)
    for bad in ("-1", "94", "x", "1.5", "0x10"):
        with pytest.raises(ValueError) as e:
            tiddit_alleles.parse_switch(path, bad)
        assert "TIDDIT_ALLELES_MIN_BQ" in str(e.value)


@pytest.mark.parametrize("env", [{"TIDDIT_ALLELES": "/nonexistent/sites.vcf"}, {"TIDDIT_ALLELES": "SITES", "TIDDIT_ALLELES_MIN_BQ": "94"}])
def test_the_job_refuses_a_bad_switch_before_any_work(tmp_path, env):
    """status 1 and one error line before the BAM is opened (the job is given files that do not exist) and before the library is loaded"""
    sites = str(tmp_path / "sites.vcf")
    open(sites, "w").write(VCF)
    e = dict(os.environ, **{k: (sites if v == "SITES" else v) for k, v in env.items()})
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", "tiddit_amd", "--sv", "--bam", str(tmp_path / "no.bam"), "--ref", str(tmp_path / "no.fa"), "-o", out,
                        "--skip_assembly"], cwd=REPO, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    errors = [l for l in r.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_ALLELES=")
    assert not os.path.exists(out + "_tiddit")
