"""`TIDDIT_PHASE` without a GPU: the definition (tiddit_amd/tiddit_phase.py) against the independent restatement of tests/phase_cases.py
on every read, fragment, threshold and graph case; every case's literal claims; the one-line departures of the restatement, each noticed
inside the family listed for it; the het rule against the REF_N / ALT_N that tiddit_alleles.write_file prints; the FNV-1a literals; the
switch parser and its refusals.

Every test of this file fails on the parent commit: the module does not exist there."""
import numpy as np
import pytest

import phase_cases as D
from tiddit_amd import tiddit_alleles, tiddit_phase


@pytest.fixture(scope="module")
def defined():
    return {c["name"]: D.definition(c) for c in D.CASES}


def test_the_stated_counts_of_cases():
    assert len(D.CASES) == D.N_CASES and len(D.GRAPHS) == D.N_GRAPHS
    assert len({c["name"] for c in D.CASES}) == D.N_CASES and set(D.MUTANTS.values()) <= set(D.FAMILIES) | {"graphs"}


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_definition_restatement_and_claims_agree(case, defined):
    keys, sn, table, het, result = defined[case["name"]]
    rkeys, rsn = D.restate_keys(case)
    assert np.array_equal(D.key_rows(keys), D.key_rows(rkeys)) and sn == rsn, (sn, rsn)
    assert D.same_result(result, D.restate(rkeys, het, D.sites_of(case)[0].site_off, case["S"]))
    assert case["claims"] and not D.claim_problems(case, keys, sn, het, result), D.claim_problems(case, keys, sn, het, result)


def test_padding_and_batch_cuts_change_nothing(defined):
    for c in D.CASES:
        if c["family"] in ("malformed", "state"):
            keys, sn, _, het, result = D.definition(dict((k, v) for k, v in c.items() if not isinstance(k, tuple)), padding=False) if c["reader_ok"] else defined[c["name"]]
            assert sorted(keys) == sorted(defined[c["name"]][0]) and sn == defined[c["name"]][1]


@pytest.mark.parametrize("graph", D.GRAPHS, ids=[g["name"] for g in D.GRAPHS])
def test_forest_definition_restatement_and_claims_agree(graph):
    f = tiddit_phase.forest(graph["n_sites"], graph["j"], graph["i"], graph["n"], graph["trans"], graph["S"])
    r = D.restate_forest(graph["n_sites"], graph["j"], graph["i"], graph["n"], graph["trans"], graph["S"])
    assert D.same_forest(f, r), graph["name"]
    assert not D.graph_problems(graph, f), D.graph_problems(graph, f)
    assert f["sn"]["forest_edges"] == f["sn"]["phased_sites"] - f["sn"]["blocks"]


@pytest.mark.parametrize("mutant", list(D.MUTANTS), ids=list(D.MUTANTS))
def test_every_departure_of_the_restatement_is_noticed_in_its_family(mutant, defined):
    family, noticed = D.MUTANTS[mutant], []
    if family == "graphs":
        for g in D.GRAPHS[:12]:
            f = tiddit_phase.forest(g["n_sites"], g["j"], g["i"], g["n"], g["trans"], g["S"])
            if not D.same_forest(f, D.restate_forest(g["n_sites"], g["j"], g["i"], g["n"], g["trans"], g["S"], mutant)):
                noticed.append(g["name"])
    else:
        for c in (c for c in D.CASES if c["family"] == family):
            keys, sn, _, het, result = defined[c["name"]]
            rkeys, rsn = D.restate_keys(c, mutant)
            if sorted(rkeys) != sorted(keys) or rsn != sn or not D.same_result(result, D.restate(rkeys, het, D.sites_of(c)[0].site_off, c["S"], mutant)):
                noticed.append(c["name"])
    assert noticed, (mutant, family)
    assert len(D.MUTANTS) >= 10


def test_fnv1a_literals():
    for name, want in D.FNV_LITERALS.items():
        assert tiddit_phase.fnv1a64(name.encode()) == want == D.fnv(name)
    assert tiddit_phase.fnv1a64(b"ab") != tiddit_phase.fnv1a64(b"ac")


def test_the_het_rule_reads_the_counts_the_allele_file_prints(tmp_path):
    """REF_N / ALT_N of rule 6 are the two columns of {o}.alleles.tab, row by row, and the rule's three tests hold at their edges"""
    case = next(c for c in D.CASES if c["name"] == "thresholds 4 min = max")
    sites, codes = D.sites_of(case)
    table = D.definition(case)[2]
    path = str(tmp_path / "a.alleles.tab")
    tiddit_alleles.write_file(path, sites.rows, table)
    het, ref_n, alt_n = tiddit_phase.het_flags(table, codes, 3)
    rows = [l.split("\t") for l in open(path).read().split("\n")[1:] if l]
    assert len(rows) == len(sites.rows) == 5
    for (chrom, pos, ref, alt, k), l in zip(sites.rows, rows):
        assert (int(l[12]), int(l[13])) == (int(ref_n[k]), int(alt_n[k]))
    t = np.zeros((6, 8), dtype=np.uint32)
    c6 = np.array([0 | 1 << 2] * 5 + [0xff], dtype=np.uint8)                    # A > C five times, one site that is not phaseable
    t[:, 0], t[:, 1] = [3, 2, 3, 12, 13, 50], [3, 3, 2, 3, 3, 50]                # REF_N, ALT_N
    assert tiddit_phase.het_flags(t, c6, 3)[0].tolist() == [1, 0, 0, 1, 0, 0]   # H on either side; 5 x 3 = 15 >= 15 but < 16; never a 0xff site
    assert tiddit_phase.het_flags(t, c6, 2)[0].tolist() == [1, 1, 1, 1, 0, 0]


def test_site_codes_and_positions_with_two_rows():
    case = next(c for c in D.CASES if c["family"] == "bases")
    sites, codes = D.sites_of(case)
    assert codes.tolist() == [0 | 1 << 2, 1 | 2 << 2, 2 | 3 << 2, 3 | 0 << 2, 0xff] and len(sites.rows) == 6


def test_the_switch_parser_and_its_refusals():
    P = tiddit_phase.parse_switch
    assert P(None, True) is None and P("", True) is None and P(None, False) is None and P("", False) is None
    assert P("1", True) == (2, 3) and P("2", True) == (2, 3) and P("7", True) == (7, 3) and P("1:3", True) == (1, 3) and P("1000000:1000000", True) == (10 ** 6, 10 ** 6)
    for bad in ("0", "-1", "1000001", "01", "1:", ":3", "2:0", "2:3:4", "x", "2.0", " 2", "1:1000001", "+2"):
        with pytest.raises(ValueError):
            P(bad, True)
    with pytest.raises(ValueError) as e:
        P("2", False)
    assert "TIDDIT_ALLELES not set" in str(e.value)
    with pytest.raises(ValueError) as e:
        P("x", False)                                                             # (the value form is judged first)
    assert "TIDDIT_ALLELES" not in str(e.value)


def test_the_file_text_of_a_case(defined):
    case = next(c for c in D.CASES if c["name"] == "thresholds equal w decided by row")
    keys, sn, table, het, result = defined[case["name"]]
    sites, codes = D.sites_of(case)
    _, ref_n, alt_n = tiddit_phase.het_flags(table, codes, case["H"])
    text, blocks, all_sn = tiddit_phase.file_text(sites, codes, het, ref_n, alt_n, result, sn, D.NAMES, 2, 1, 13)
    lines = text.split("\n")
    assert lines[0] == "# tiddit_amd phase v1 min_link=2 min_allele=1 min_bq=13 hash=fnv1a64"
    assert [l.split("\t")[1] for l in lines[1:1 + len(tiddit_phase.SN)]] == list(tiddit_phase.SN)
    assert lines[1 + len(tiddit_phase.SN)] == "#CHROM\tPOS\tREF\tALT\tREF_N\tALT_N\tGT\tPS"
    assert lines[2 + len(tiddit_phase.SN):] == ["c0\t101\tA\tC\t4\t2\t0|1\t101", "c0\t201\tC\tG\t4\t2\t0|1\t101", "c0\t301\tT\tA\t3\t3\t1|0\t101", ""]   # (REF ALT REF per trio of pairs)
    assert blocks == "#CHROM\tSTART\tEND\tSITES\tEDGES\tAGREE\tCONFLICT\nc0\t101\t301\t3\t3\t0\t1\n"
    assert all_sn["phaseable_sites"] == 5 and all_sn["het_sites"] == 3
