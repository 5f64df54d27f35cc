"""The definition of ``TIDDIT_INDELS_NORM`` (tiddit_indels.left_normalise, events_of_read / keys_of_batch with ``ref``) against the
independent restatement and the written claims of tests/indel_norm_cases.py — no GPU.  The GPU tests compare the kernel with the
definition; this file is what pins the definition."""
import numpy as np
import pytest

import indel_cases as D
import indel_norm_cases as N

IDS = [c["name"] for c in N.CASES]


@pytest.fixture(scope="module")
def defined():
    return {c["name"]: N.definition(c) for c in N.CASES}


@pytest.mark.parametrize("case", N.CASES, ids=IDS)
def test_the_definition_equals_the_restatement_and_the_claim(case, defined):
    d = defined[case["name"]]
    assert N.same(d, N.restate(case)), case["name"]
    if case["want"] is not None:
        assert [(k1 >> 32, k1 & 0xffffffff) for k1, _ in d[0]] == case["want"]
    if case["norm"] is not None:
        assert d[2] == case["norm"]


@pytest.mark.parametrize("case", N.CASES, ids=IDS)
def test_the_whole_column_form_agrees_with_the_read_by_read_form(case, defined):
    from tiddit_amd import tiddit_indels
    ref = N.host_reference(case["loaded"])
    keys, sn = [], {}
    for b in D.batches(case):
        keys.extend(tiddit_indels.keys_of_batch(b, sn, case["Q"], ref))
    assert keys == defined[case["name"]][0] and tuple(sn.get(k, 0) for k in N.NORM_SN) == defined[case["name"]][2]


def test_placements_of_one_event_give_one_key_and_one_rotation(defined):
    from tiddit_amd import tiddit_indels
    keys = defined[next(c["name"] for c in N.CASES if c["family"] == "ins_repeat")][0]
    assert {(k1, k2 >> 1) for k1, k2 in keys[:41]} == {(D.K1(0, 6000), D.INS("CA") >> 1)} and tiddit_indels.seq_text(keys[0][1]) == "CA"
    assert {(k1, k2 >> 1) for k1, k2 in keys[41:]} == {(D.K1(1, 300), D.INS("CACA") >> 1)}
    sets = next(c for c in N.CASES if c["family"] == "sets")
    with_ref, without = defined[sets["name"]], N.definition(sets, ref=None)
    assert [len(with_ref[1][S][1][0]) for S in (1, 2, 3)] == [2, 2, 2] and [len(without[1][S][1][0]) for S in (1, 2, 3)] == [6, 0, 0]
    assert with_ref[1][3][1][2].tolist() == [3, 3] and with_ref[1][3][1][3].tolist() == [2, 1]


def test_a_rotated_allele_has_the_key_of_that_allele_inserted_directly():
    """also across the packed / hashed border: n = 22 packs, n = 23 hashes"""
    from tiddit_amd import tiddit_indels as T
    ref = N.host_reference()
    seen = set()
    for unit, at in (("ACGTTGCAAGCTTCGATCGGAT", 8400), ("ACGTTGCAAGCTTCGATCGGATC", 8200)):
        n = len(unit)
        for j in (1, 5, n - 1, n, n + 3, 3 * n):
            codes = [D.BASES.index(c) for c in (unit * 2)[j % n:j % n + n]]
            P2, allele, k, status = T.left_normalise(ref, 0, at + j, n, True, codes)
            assert (P2, k, status) == (at, j, T.NORM_OK) and allele == [D.BASES.index(c) for c in unit]
            assert T.left_normalise(ref, 0, P2, n, True, allele) == (P2, allele, 0, T.NORM_OK)
            kind, payload = T.payload_of_codes(allele)
            assert kind == (0 if n == 22 else 1)
            seen.add((n, kind, payload))
    assert len(seen) == 2 and {(n, p) for n, _, p in seen} == {(22, D.INS("ACGTTGCAAGCTTCGATCGGAT") >> 1 & (1 << 44) - 1),
                                                                (23, D.INSH("ACGTTGCAAGCTTCGATCGGATC") >> 1 & (1 << 44) - 1)}


def test_without_a_reference_the_functions_are_what_they_were():
    from tiddit_amd import tiddit_indels
    assert len(D.CASES) == D.N_CASES
    for case in D.CASES:
        want = D.reference(case)
        keys, sn = [], {}
        for b in D.batches(case):
            tiddit_indels.keys_of_batch_by_read(b, keys, sn, case["Q"], None)
        assert not set(sn) & set(N.NORM_SN)
        assert np.array_equal(D.key_rows(keys), want[0]), case["name"]
        for S in case["S"]:                                      # ... and the eleven counters and the rows
            counts, rows = tiddit_indels.summarise(keys, sn, S)
            assert np.array_equal(counts, want[1][S][0]), (case["name"], S)
            assert all(np.array_equal(x, y) for x, y in zip(D.row_columns(rows), want[1][S][1])), (case["name"], S)
        b = D.build(case)
        r = tiddit_indels.events_of_read(int(b.flag[0]), int(b.tid[0]), int(b.pos[0]), int(b.mapq[0]), int(b.rec_off[0]), bytes(b.raw), case["Q"])
        assert len(r) == 4
        assert len(tiddit_indels.events_of_read(int(b.flag[0]), int(b.tid[0]), int(b.pos[0]), int(b.mapq[0]), int(b.rec_off[0]), bytes(b.raw), case["Q"],
                                                ref=N.host_reference())) == 5


@pytest.mark.parametrize("mutant", sorted(N.MUTANTS))
def test_each_departure_changes_the_output_inside_its_family(mutant, defined):
    """The departures are made in the RESTATEMENT (the cases file), not in the package: this is a check that the case set is sensitive to
    each of them.  It bears on the package through what it compares with — ``left_normalise``'s output on the family's cases must differ
    from the departed restatement, while test_the_definition_equals_the_restatement_and_the_claim holds it equal to the faithful one — so a
    ``left_normalise`` that made one of these departures would fail here or there."""
    family = N.MUTANTS[mutant]
    hit = [c["name"] for c in N.CASES if c["family"] == family and not N.same(defined[c["name"]], N.restate(c, mutant=mutant))]
    assert hit, (mutant, family)


def test_the_switch_needs_its_partner():
    from tiddit_amd import tiddit_indels as T
    assert T.parse_norm_switch(None, None) is False and T.parse_norm_switch("", (2, 20)) is False and T.parse_norm_switch("1", (2, 20)) is True
    with pytest.raises(ValueError, match="TIDDIT_INDELS not set"):
        T.parse_norm_switch("1", None)
    with pytest.raises(ValueError, match="the switch is 1"):
        T.parse_norm_switch("0", (2, 20))


def test_the_file_gains_the_mark_and_three_rows_only_with_the_switch(tmp_path):
    from tiddit_amd import tiddit_indels as T
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    T.write_file(a, np.arange(11), [], [], None, 2, 20)
    T.write_file(b, np.arange(11), [], [], None, 2, 20, [5, 1, 2])
    la, lb = open(a).read().split("\n"), open(b).read().split("\n")
    assert la[0] == "# tiddit_amd indels v1 min_support=2 min_mapq=20" and lb[0] == la[0] + " left_normalised=1024"
    assert lb[1:12] == la[1:12] and lb[12:15] == ["SN\tshifted_events\t5", "SN\tshift_capped\t1", "SN\toff_reference\t2"] and lb[15:] == la[12:]
