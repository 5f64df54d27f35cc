"""The duplicate metrics without a GPU: the definition (tiddit_dup.key_of_read + summarise), the struct / Counter restatement of
tests/dup_cases.py and the hand-written claims agree on every case — keys and counters —, every one-line mutant of the restatement is
caught inside the family that claims it, the column form that the end to end test runs over a whole file equals the per-read
definition, the library-size bisection is pinned and monotone, and the host side — layout, writer, switch parser — does what its
docstrings say.

This file fails on the parent commit, which has no such module."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dup_cases as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_case_list():
    assert len(D.CASES) == D.N_CASES == 45 and len({c["name"] for c in D.CASES}) == D.N_CASES
    assert D.FAMILIES == ["carrier", "clips", "malformed", "mc", "range", "sets", "shape", "sizes"]
    assert sum(not c["reader_ok"] for c in D.CASES) == 14 and all(not c["reader_ok"] for c in D.CASES if c["family"] == "malformed")
    assert D.RS_TILE == 4096 and D.DUP_TILE % D.DUP_BLOCK == 0 and D.DUP_K_TILE % D.DUP_BLOCK == 0 and D.DUP_BLOCK == 256
    assert set(D.MUTANTS.values()) <= set(D.FAMILIES)


def test_the_layout_is_the_headers_and_the_modules():
    from tiddit_amd import tiddit_dup
    assert D.SN == tiddit_dup.SN and D.SIZE == tiddit_dup.SIZE == 2060 and D.OFF_HIST == tiddit_dup.OFF_HIST
    assert (D.BIAS, D.HIST_MAX, D.TOP) == (tiddit_dup.DUP_BIAS, tiddit_dup.DUP_HIST_MAX, tiddit_dup.E_LIMIT) == (1 << 28, 1024, 1 << 33)
    header = open(os.path.join(REPO, "include", "tiddit_hip.h")).read()
    macro = lambda k: int(re.search(r"^#define TDT_DUP_%s (\d+)$" % k, header, re.M).group(1))
    assert (macro("SN_N"), macro("OFF_HIST"), macro("HIST_MAX"), macro("TOTAL")) == (len(D.SN), D.OFF_HIST, D.HIST_MAX, D.SIZE)
    # the fields of a key do not overlap: strand, 33 bits of end, 24 bits of contig, the pair bit
    assert D.K1(2 ** 24 - 1, D.TOP - 1 - D.BIAS, 1) == 2 ** 58 - 1 and D.K2(0, -D.BIAS, 0) == 2 ** 58


@pytest.fixture(scope="module")
def results():
    return {c["name"]: (D.expected(c), D.reference(c), D.definition(c)) for c in D.CASES}


def _same(got, want):
    return got[0].shape == want[0].shape and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _differences(got, want):
    return got[0].shape, want[0].shape, [(int(k), int(got[1][k]), int(want[1][k])) for k in np.flatnonzero(got[1] != want[1])[:8]]


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_definition_restatement_and_claim_agree(case, results):
    claim, ref, dfn = results[case["name"]]
    assert claim[1].any() and claim[1].dtype == np.uint64
    for who, got in (("restatement", ref), ("definition", dfn)):
        assert _same(got, claim), (who, _differences(got, claim))


def test_the_column_form_of_the_definition_equals_it_on_every_case(results):
    """tiddit_dup.keys_of_batch + summarise_columns (what the end to end test runs over a whole file) against key_of_read + summarise"""
    from tiddit_amd import tiddit_dup
    for c in D.CASES:
        sn, cols = {}, []
        for b in D.batches(c):
            cols.append(tiddit_dup.keys_of_batch(b, sn))
        k1, k2, m = (np.concatenate([x[k] for x in cols]) for k in range(3))
        assert k1.dtype == k2.dtype == np.uint64 and m.dtype == np.uint8
        got = (D.rows_of(list(zip(k1.tolist(), k2.tolist(), m.tolist()))), tiddit_dup.summarise_columns(k1, k2, sn))
        assert _same(got, results[c["name"]][2]), (c["name"], _differences(got, results[c["name"]][2]))


def test_every_record_is_counted_once_and_the_counters_add_up():
    for c in D.CASES:
        e = dict(zip(D.SN, D.expected(c)[1][:12].tolist()))
        assert e["records"] == len(c["reads"]) * c["repeat"], c["name"]
        assert e["eligible"] == e["malformed"] + e["fragments"] + e["pairs"] + e["pair_mates"], c["name"]
        assert e["fragments"] == e["fragment_sets"] + e["fragment_duplicates"] and e["pairs"] == e["pair_sets"] + e["pair_duplicates"], c["name"]


def test_the_order_of_the_reads_changes_nothing():
    from tiddit_amd import tiddit_dup
    c = next(c for c in D.CASES if c["name"] == "carrier mates that make a fragment, records that are not eligible")
    want = D.definition(c)
    rng = np.random.default_rng(11)
    for order in (list(range(len(c["reads"])))[::-1], rng.permutation(len(c["reads"])).tolist()):
        keys, sn = [], {}
        tiddit_dup.keys_of_batch_by_read(D.build_reads([c["reads"][k] for k in order]), keys, sn)
        assert _same((D.rows_of(keys), tiddit_dup.summarise(keys[::-1], sn)), want)


def test_padding_changes_nothing():
    for c in D.CASES:
        if any(r["pad"] for r in c["reads"]) and not c.get("truncate_last"):
            assert _same(D.reference(c, padding=False), D.reference(c, padding=True)), c["name"]


@pytest.mark.parametrize("mutant", sorted(D.MUTANTS))
def test_every_mutant_is_caught_inside_its_family(mutant):
    family = D.MUTANTS[mutant]
    caught = [c["name"] for c in D.CASES if c["family"] == family and not _same(D.reference(c, mutant), D.expected(c))]
    assert caught, (mutant, family)


# ---- the derived rows -----------------------------------------------------------------------------------------------------------
def test_library_size_is_pinned_and_brackets_the_root():
    from tiddit_amd import tiddit_dup
    pins = {(2, 1): 1, (10, 9): 46, (100, 90): 466, (1000, 500): 627, (1000000, 900000): 4660793, (300000000, 270000000): 1398238043, (1025, 1): 1}
    for (pairs, sets), want in pins.items():
        got = tiddit_dup.library_size(pairs, sets)
        assert got == want, (pairs, sets, got)
        f = lambda L: L * -math.expm1(-pairs / L)
        assert f(got) <= sets * (1 + 1e-12) and f(got + 1) >= sets * (1 - 1e-12)              # floor of the root
    for pairs, sets in ((5, 5), (5, 6), (0, 0), (7, 0)):
        assert tiddit_dup.library_size(pairs, sets) is None


def test_library_size_is_monotone():
    from tiddit_amd import tiddit_dup
    by_sets = [tiddit_dup.library_size(10000, s) for s in range(1, 10000, 97)]
    assert all(a <= b for a, b in zip(by_sets, by_sets[1:])) and by_sets[0] == 1 and by_sets[-1] > 10000      # more distinct pairs: a larger library
    by_pairs = [tiddit_dup.library_size(p, 5000) for p in range(5001, 50000, 997)]
    assert all(a >= b for a, b in zip(by_pairs, by_pairs[1:])) and by_pairs[-1] == 5000                     # the same sets from more pairs: a smaller one


def test_derived_rows():
    from tiddit_amd import tiddit_dup
    c = np.zeros(D.SIZE, dtype=np.uint64)
    assert tiddit_dup.derived(c) == []
    for k, v in (("fragments", 3), ("fragment_duplicates", 1)):
        c[D.SN.index(k)] = v
    assert tiddit_dup.derived(c) == [("duplication_ppm", 333333)]
    for k, v in (("pairs", 8), ("pair_sets", 7), ("pair_duplicates", 1)):
        c[D.SN.index(k)] = v
    assert tiddit_dup.derived(c) == [("duplication_ppm", 10 ** 6 * 3 // 19), ("estimated_library_size", 29)]


# ---- the writer -----------------------------------------------------------------------------------------------------------------
def test_writer_bytes(tmp_path):
    from tiddit_amd import tiddit_dup
    case = next(c for c in D.CASES if c["name"] == "sets pairs that differ in one field")
    path = str(tmp_path / "x.dup.tab")
    tiddit_dup.write_file(path, D.expected(case)[1])
    value = {"records": 9, "eligible": 9, "fragments": 1, "pairs": 8, "pairs_no_mc": 8, "fragment_sets": 1, "pair_sets": 7, "pair_duplicates": 1}
    want = "# tiddit_amd dup v1\n" + "".join("SN\t%s\t%d\n" % (k, value.get(k, 0)) for k in D.SN) + (
        "SN\tduplication_ppm\t117647\n"
        "SN\testimated_library_size\t29\n"
        "HIST\t1\t6\t1\n"
        "HIST\t2\t1\t0\n")
    assert open(path).read() == want
    big = next(c for c in D.CASES if c["name"] == "sizes sets of 1 2 63 64 65 and round DUP_HIST_MAX")
    tiddit_dup.write_file(path, D.expected(big)[1])
    lines = open(path).read().split("\n")
    assert "HIST\t1024\t1\t2" in lines and "HIST\t1023\t0\t1" in lines and "HIST\t65\t1\t1" in lines and not [l for l in lines if l.startswith("HIST\t1025")]
    none = next(c for c in D.CASES if c["name"] == "shape a batch of 1 reads")
    tiddit_dup.write_file(path, D.expected(none)[1])
    assert open(path).read().split("\n")[13:] == ["SN\tduplication_ppm\t0", "HIST\t1\t0\t1", ""]


def test_summary_line():
    from tiddit_amd import tiddit_dup
    case = next(c for c in D.CASES if c["name"] == "sets pairs that differ in one field")
    assert tiddit_dup.summary_line(D.expected(case)[1]) == ("duplicates: 9 records, 1 fragments, 8 pairs, 0 fragment duplicates, 1 pair duplicates, 117647 ppm, "
                                                            "library size 29, malformed records 0")
    assert tiddit_dup.summary_line(np.zeros(D.SIZE, dtype=np.uint64)).endswith("- ppm, library size -, malformed records 0")


# ---- the switch -----------------------------------------------------------------------------------------------------------------
def test_switch_parser():
    from tiddit_amd import tiddit_dup
    assert tiddit_dup.parse_switch(None) is False and tiddit_dup.parse_switch("") is False and tiddit_dup.parse_switch("1") is True
    for bad in ("0", "2", "yes", " 1", "1 ", "01"):
        with pytest.raises(ValueError):
            tiddit_dup.parse_switch(bad)


def test_the_job_refuses_a_bad_switch_before_any_work(tmp_path):
    """status 1 and one error line before the BAM is opened (the job is given files that do not exist) and before the library is loaded"""
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", "tiddit_amd", "--sv", "--bam", str(tmp_path / "no.bam"), "--ref", str(tmp_path / "no.fa"), "-o", out,
                        "--skip_assembly"], cwd=REPO, env=dict(os.environ, TIDDIT_DUPS="2"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    assert [l for l in r.stdout.split("\n") if l.startswith("error")] == ["error, TIDDIT_DUPS=2: the switch is 1 or unset"]
    assert not os.path.exists(out + "_tiddit") and not os.path.exists(out + ".dup.tab")
