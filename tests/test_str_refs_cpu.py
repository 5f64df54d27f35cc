"""`TIDDIT_STR` without a GPU: every aimed case's claim (tests/str_cases.py) equals the definition (``tiddit_str.keys_of_read`` /
``rows_of_keys``) and the independent restatement (a reference-to-query map and string matching); each stated one-line departure of the
restatement is noticed inside its family; the genotype rule on its literal cases; the loci reader's refusals; the cuts; the file's text;
and the definition ignores where batches are cut."""
import gzip

import numpy as np
import pytest

import str_cases as D
from tiddit_amd import tiddit_str


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_the_claim_equals_the_definition_and_the_restatement(case):
    claim, defn, ref = D.expected(case), D.definition(case), D.reference(case)
    assert D.same(claim, defn), (case["name"], claim[1].tolist(), defn[1].tolist(), claim[0].tolist()[:12], defn[0].tolist()[:12])
    assert D.same(claim, ref), (case["name"], claim[1].tolist(), ref[1].tolist(), claim[0].tolist()[:12], ref[0].tolist()[:12])


def test_the_stated_number_of_cases_and_families():
    assert D.N_CASES == len(D.CASES) == 30
    assert D.FAMILIES == ["bad", "cigar", "flank", "gate", "merge", "motif", "run", "table"]
    assert len({c["name"] for c in D.CASES}) == D.N_CASES


@pytest.mark.parametrize("mutant", sorted(D.MUTANTS))
def test_a_departure_of_the_restatement_is_noticed_inside_its_family(mutant):
    family = [c for c in D.CASES if c["family"] == D.MUTANTS[mutant]]
    assert family and any(not D.same(D.expected(c), D.reference(c, mutant)) for c in family), mutant


@pytest.mark.parametrize("case", [c for c in D.CASES if len(c["reads"]) >= 4 and len(c["reads"]) <= 40], ids=lambda c: c["name"])
def test_the_definition_ignores_where_batches_are_cut(case):
    n = len(case["reads"])
    whole = D.definition(case, cuts=())
    for cuts in ((1,), (n // 2,), (1, 2, n - 1), tuple(range(1, n))):
        assert D.same(whole, D.definition(case, cuts=cuts)), (case["name"], cuts)


@pytest.mark.parametrize("name,spans,flanks,S,want", D.GENOTYPES, ids=[g[0] for g in D.GENOTYPES])
def test_the_genotype_rule(name, spans, flanks, S, want):
    loci = tiddit_str.loci_of_rows([list(map(str, D.STD))], D.NAMES, D.LENGTHS)
    rows = D.genotype_rows(spans, flanks)
    got = tiddit_str.summarise(loci, rows, S)
    assert got == [(12,) + want]
    # ... and from the four columns, as the handle gives the rows
    assert tiddit_str.summarise(loci, D.row_columns(rows), S) == got


def test_summarise_keeps_loci_apart_and_in_table_order():
    loci = tiddit_str.loci_of_rows([["c0", "2000", "2010", "CAG", "second"], ["c0", "1000", "1012", "cag"], ["c1", "50", "56", "AC"]], D.NAMES, D.LENGTHS)
    assert [r[:2] for r in loci.rows] == [("c0", 1000), ("c0", 2000), ("c1", 50)]
    rows = D.genotype_rows({12: 5}, [], 0) + D.genotype_rows({13: 2, 10: 3}, [(2, 30, 1)], 1)
    got = tiddit_str.summarise(loci, rows, 5)
    assert got == [(12, 5, (12, 5, 12, 5, "0/0"), 0, 0, 0, "12:5"), (10, 5, (10, 3, 13, 2, "0/1"), 1, 30, 1, "10:3,13:2"), (6, 0, None, 0, 0, 0, ".")]


def test_the_file_text(tmp_path):
    loci = tiddit_str.loci_of_rows([["c0", "1000", "1012", "cag", "HTT"], ["c0", "2000", "2010", "CAG"], ["c9", "1", "5", "A"]], D.NAMES, D.LENGTHS)
    rows = D.genotype_rows({12: 3, 15: 3}, [(2, 16, 1)], 0)
    table = tiddit_str.summarise(loci, rows, 5)
    counts = np.arange(1, 12, dtype=np.uint64)
    p = str(tmp_path / "x.str.tab")
    tiddit_str.write_file(p, loci, counts, table, 5, 5, 20)
    want = ("# tiddit_amd str v1 flank=5 min_reads=5 min_mapq=20\n"
            + "".join("SN\t%s\t%d\n" % (k, i + 1) for i, k in enumerate(D.SN))
            + "SN\tloci\t2\nSN\tskipped_columns\t0\nSN\tskipped_contig\t1\nSN\tskipped_range\t0\nSN\tskipped_long\t0\nSN\tskipped_motif\t0\n"
            + "SN\tskipped_overlap\t0\nSN\tskipped_cap\t0\n"
            + "#CHROM\tSTART\tEND\tMOTIF\tID\tREF_LEN\tSPAN_N\tA1\tA1_N\tA2\tA2_N\tGT\tFLANK_N\tFLANK_MAX\tLONGER\tHIST\n"
            + "c0\t1000\t1012\tCAG\tHTT\t12\t6\t12\t3\t15\t3\t0/1\t1\t16\t1\t12:3,15:3\n"
            + "c0\t2000\t2010\tCAG\t.\t10\t0\t.\t.\t.\t.\t.\t0\t0\t0\t.\n")
    assert open(p).read() == want


def test_the_loci_reader_refuses_by_reason_in_the_stated_order(tmp_path):
    text = "\n".join([
        "# a comment", "track name=x", "browser position c0:1-2", "",
        "c0\t3000\t3012\tCAG\tthird",                   # accepted (sorted behind the next one)
        "c0\t1000\t1012\tcag",                          # accepted, lower case, no id
        "c0\t1012\t1020\tAC",                           # overlaps: start must be >= 1013
        "c0\t1013\t1020\tAC\tnext",                     # accepted: one base apart
        "c0\t10",                                       # fewer than four columns
        "c7\t0\t0\tNNNNNNNN",                           # unknown contig (tested first)
        "c0\t0\t10\tA",                                 # start 0: no neighbour base
        "c0\t99990\t100000\tA",                         # end == LN: no neighbour base
        "c0\t99989\t99999\tA\tlast",                    # accepted: end == LN - 1
        "c0\t10\t10\tA",                                # empty
        "c0\tx\t10\tA",                                 # not a number
        "c1\t1\t1000002\tNNNNNNN",                      # outside the contig comes before too long and before the motif
        "c2\t1\t8\tACGTACG",                            # seven letters
        "c2\t1\t8\tACN",                                # not ACGT
        "c2\t1\t8\t",                                   # empty motif
        "c2\t1\t8\tACGTAC\tsix",                        # accepted
    ]) + "\n"
    names, lengths = D.NAMES, D.LENGTHS
    want_rows = [("c0", 1000, 1012, "CAG", "."), ("c0", 1013, 1020, "AC", "next"), ("c0", 3000, 3012, "CAG", "third"), ("c0", 99989, 99999, "A", "last"),
                 ("c2", 1, 8, "ACGTAC", "six")]
    want_skipped = {"fewer than four columns": 1, "unknown contig": 1, "coordinates outside the contig": 5, "longer than 10^6": 0,
                    "not a motif of 1 to 6 ACGT": 3, "overlaps the locus in front": 1, "over 2^24 loci": 0}
    for zipped in (False, True):
        p = str(tmp_path / ("loci.bed.gz" if zipped else "loci.bed"))
        with (gzip.open(p, "wt") if zipped else open(p, "w")) as f:
            f.write(text)
        loci = tiddit_str.read_loci(p, names, lengths)
        assert loci.rows == want_rows and loci.skipped == want_skipped
        assert loci.loc_off.tolist() == [0, 4, 4, 5] and loci.lstart.tolist() == [1000, 1013, 3000, 99989, 1] and loci.lend.tolist() == [1012, 1020, 3012, 99999, 8]
        assert loci.lstart.dtype == loci.lend.dtype == np.int32 and loci.motif.dtype == np.uint32 and loci.loc_off.dtype == np.int64
        assert loci.motif.tolist() == [0x4123, 0x212, 0x4123, 0x11, 0x2184216]


def test_the_loci_reader_too_long_the_stable_sort_and_the_cap(monkeypatch):
    long_names, long_lengths = ("big",), (3000000,)
    loci = tiddit_str.loci_of_rows([["big", "1", "1000002", "A"], ["big", "1", "1000001", "A", "ok"], ["big", "2000000", "2000010", "AC", "b"],
                                    ["big", "2000000", "2000020", "AC", "a"]], long_names, long_lengths)
    # (equal starts: the row that stands first in the file wins — the sort is stable — and the other one overlaps it)
    assert loci.rows == [("big", 1, 1000001, "A", "ok"), ("big", 2000000, 2000010, "AC", "b")]
    assert loci.skipped["longer than 10^6"] == 1 and loci.skipped["overlaps the locus in front"] == 1
    monkeypatch.setattr(tiddit_str, "MAX_LOCI", 2)
    loci = tiddit_str.loci_of_rows([["big", str(10 * k), str(10 * k + 5), "A"] for k in range(1, 5)], long_names, long_lengths)
    assert len(loci) == 2 and loci.skipped["over 2^24 loci"] == 2 and tiddit_str.MAX_LOCI == 2


def test_the_cuts_and_the_switch():
    assert tiddit_str.parse_switch(None, None) is None and tiddit_str.parse_switch("", "") is None
    assert tiddit_str.parse_switch("l.bed", None) == ("l.bed", 5, 5, 20) and tiddit_str.parse_switch("l.bed", "") == ("l.bed", 5, 5, 20)
    assert tiddit_str.parse_switch("l.bed", "7") == ("l.bed", 7, 5, 20) and tiddit_str.parse_switch("l.bed", "1:1") == ("l.bed", 1, 1, 20)
    assert tiddit_str.parse_switch("l.bed", "100:1000000:255") == ("l.bed", 100, 10 ** 6, 255) and tiddit_str.parse_switch("l.bed", "3:2:0") == ("l.bed", 3, 2, 0)
    for bad in ("0", "101", "5:0", "5:1000001", "5:5:256", "5:5:5:5", "a", "5:", ":5", "-1", "5.0", " 5", "1" * 10):
        with pytest.raises(ValueError):
            tiddit_str.parse_switch("l.bed", bad)
    with pytest.raises(ValueError, match="TIDDIT_STR not set"):
        tiddit_str.parse_switch(None, "5")
    with pytest.raises(ValueError, match="TIDDIT_STR not set"):
        tiddit_str.parse_switch("", "5:5:20")


def test_the_packed_motif():
    assert tiddit_str.pack_motif("A") == 0x11 and tiddit_str.pack_motif("CAG") == 0x4123 and tiddit_str.pack_motif("ACGTAC") == 0x2184216
