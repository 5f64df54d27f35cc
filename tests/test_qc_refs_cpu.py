"""The read-level QC tables without a GPU: the definition (tiddit_qc.count_read), the numpy restatement of tests/qc_cases.py and the
hand-written claims agree on every case, every one-line mutant of the restatement is caught inside the family that claims it, and the
host side — layout, writer, switch parser — does what its docstrings say.

This file fails on the parent commit, which has no such module."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import qc_cases as QC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_case_list():
    assert len(QC.CASES) == QC.N_CASES and len({c["name"] for c in QC.CASES}) == QC.N_CASES
    assert QC.FAMILIES == ["cigar", "flags", "gcr", "insert", "length", "malformed", "nibbles", "qualities", "shape"]
    assert sum(not c["reader_ok"] for c in QC.CASES) == 5 and all((c["family"] == "malformed") == (not c["reader_ok"]) for c in QC.CASES)
    assert all(any(c["cuts"] for c in QC.CASES if c["family"] == f) for f in QC.FAMILIES)          # batches cut inside every family


def test_the_layout_is_the_headers_and_the_modules():
    from tiddit_amd import tiddit_qc
    assert (QC.CY, QC.IM, QC.IDM) == (tiddit_qc.QC_CYCLES, tiddit_qc.QC_IS_MAX, tiddit_qc.QC_ID_MAX) == (512, 2000, 64)
    assert QC.SECTIONS == tiddit_qc.LAYOUT and QC.SIZE == tiddit_qc.SIZE and QC.SN == tiddit_qc.SN
    header = open(os.path.join(REPO, "include", "tiddit_hip.h")).read()
    macro = lambda k: int(re.search(r"^#define TDT_QC_%s (\d+)$" % k, header, re.M).group(1))
    assert {k: macro("OFF_" + k) for k in QC.SECTIONS} == {k: v[0] for k, v in QC.SECTIONS.items()}
    assert macro("TOTAL") == QC.SIZE and macro("SN_N") == len(QC.SN)
    # what a workgroup of the base pass adds to a 32-bit word between its zeroing and its flush cannot wrap
    assert 65535 * QC.BT < 2 ** 32 and 255 * QC.BT < 2 ** 32


@pytest.fixture(scope="module")
def results():
    return {c["name"]: (QC.expected(c), QC.reference(c), QC.definition(c)) for c in QC.CASES}


def _differences(got, want):
    return [(int(k), int(got[k]), int(want[k])) for k in np.flatnonzero(got != want)[:8]]


@pytest.mark.parametrize("case", QC.CASES, ids=[c["name"] for c in QC.CASES])
def test_definition_restatement_and_claim_agree(case, results):
    claim, ref, dfn = results[case["name"]]
    assert claim.any()
    for who, got in (("restatement", ref), ("definition", dfn)):
        assert np.array_equal(got, claim), (who, _differences(got, claim))


@pytest.mark.parametrize("chunk", [1 << 22, 7])
def test_the_column_form_of_the_definition_equals_it_on_every_case(results, chunk):
    """tiddit_qc.count_batch_columns (what the end to end test runs over a whole file) against count_read"""
    from tiddit_amd import tiddit_qc
    for c in QC.CASES:
        if chunk == 7 and len(c["reads"]) > 300:
            continue
        got = np.zeros(QC.SIZE, dtype=np.int64)
        for b in QC.batches(c):
            tiddit_qc.count_batch_columns(got, b, chunk_bases=chunk)
        assert np.array_equal(got.astype(np.uint64), results[c["name"]][2]), (c["name"], _differences(got.astype(np.uint64), results[c["name"]][2]))


def test_every_record_is_counted_once():
    for c in QC.CASES:
        assert QC.expected(c)[QC.index(("SN", "records"))] == len(c["reads"]), c["name"]


def test_padding_changes_nothing_for_well_formed_cases():
    for c in QC.CASES:
        if c["family"] in ("nibbles", "cigar"):
            assert np.array_equal(QC.reference(c, padding=False), QC.reference(c, padding=True))


@pytest.mark.parametrize("mutant", sorted(QC.MUTANTS))
def test_every_mutant_is_caught_inside_its_family(mutant):
    family = QC.MUTANTS[mutant]
    caught = [c["name"] for c in QC.CASES if c["family"] == family and not np.array_equal(QC.reference(c, mutant), QC.expected(c))]
    assert caught, (mutant, family)


def test_malformed_padding_would_count_as_g_with_a_quality():
    """what a missing bound would read: the padding byte is G G as sequence and a quality; the malformed record itself carries T"""
    assert QC.PAD_BYTE >> 4 == 4 and QC.PAD_BYTE & 0xf == 4 and QC.PAD_BYTE != 0xff
    n = 0
    for c in QC.CASES:
        if c["family"] == "malformed":
            n += 1
            assert c["expect"][("SN", "malformed")] == 1 and c["expect"][("SN", "records")] == 3 and c["expect"][("MAPQ", 60)] == 3
            assert not [k for k in c["expect"] if k[0] == "QUAL" or (k[0] == "CYC" and k[2] != "A")]
            if not c.get("truncate_last"):
                assert len(QC.build(c, True).raw) - len(QC.build(c, False).raw) == QC.PAD
    assert n == 5


# ---- the writer -----------------------------------------------------------------------------------------------------------------
def test_writer_bytes(tmp_path):
    from tiddit_amd import tiddit_qc
    case = next(c for c in QC.CASES if c["name"] == "length 2 forward and reverse")
    path = str(tmp_path / "x.qc.tab")
    tiddit_qc.write_file(path, QC.expected(case))
    zero = {"secondary", "supplementary", "qc_fail", "duplicate", "unmapped", "paired", "read1", "read2", "proper_pair", "mate_unmapped", "both_mapped",
            "mate_other_contig", "mate_other_contig_mapq5", "mapq0", "malformed", "reads_no_seq", "reads_no_qual", "aligned_bases", "soft_clipped_bases",
            "hard_clipped_bases", "inserted_bases", "deleted_bases", "skipped_bases", "insertions", "deletions", "reads_clipped"}
    value = {"records": 2, "primary": 2, "mapped": 2, "reverse": 1, "bases": 4, "bases_q20": 2, "bases_q30": 2}
    assert zero | set(value) == set(QC.SN)
    want = "# tiddit_amd qc v1\n" + "".join("SN\t%s\t%d\n" % (k, value.get(k, 0)) for k in QC.SN) + (
        "MAPQ\t60\t2\n"
        "RL\t2\t2\n"
        "CYC\t0\t0\t1\t0\t1\t0\t40\t2\n"
        "CYC\t1\t1\t0\t1\t0\t0\t40\t2\n"
        "QUAL\t10\t2\n"
        "QUAL\t30\t2\n"
        "GCR\t50\t2\n")
    assert open(path).read() == want
    ins = next(c for c in QC.CASES if c["name"] == "insert who is counted")
    tiddit_qc.write_file(path, QC.expected(ins))
    lines = open(path).read().split("\n")
    assert "IS\t100\t0\t0\t1" in lines and lines[1] == "SN\trecords\t8" and len(lines) == 1 + 33 + 3 + 1
    ind = next(c for c in QC.CASES if c["name"] == "cigar ops in pairs")
    tiddit_qc.write_file(path, QC.expected(ind))
    assert "ID\t2\t1\t1" in open(path).read().split("\n")


def test_summary_line():
    from tiddit_amd import tiddit_qc
    case = next(c for c in QC.CASES if c["name"] == "malformed an op code of 9")
    assert tiddit_qc.summary_line(QC.expected(case)) == "qc tables: 3 records, 3 primary, 3 mapped, 2 bases, malformed records 1"


# ---- the switch -----------------------------------------------------------------------------------------------------------------
def test_switch_parser():
    from tiddit_amd import tiddit_qc
    assert tiddit_qc.parse_switch(None) is False and tiddit_qc.parse_switch("") is False and tiddit_qc.parse_switch("1") is True
    for bad in ("0", "2", "yes", " 1", "1 ", "01"):
        with pytest.raises(ValueError):
            tiddit_qc.parse_switch(bad)


def test_the_job_refuses_a_bad_switch_before_any_work(tmp_path):
    """status 1 and one error line before the BAM is opened (the job is given files that do not exist) and before the library is loaded"""
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", "tiddit_amd", "--sv", "--bam", str(tmp_path / "no.bam"), "--ref", str(tmp_path / "no.fa"), "-o", out,
                        "--skip_assembly"], cwd=REPO, env=dict(os.environ, TIDDIT_QC="2"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    errors = [l for l in r.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_QC=2")
    assert not os.path.exists(out + "_tiddit")
