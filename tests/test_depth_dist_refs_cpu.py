"""The references of the depth-distribution tests pinned on the CPU (tests/depth_dist_cases.py): the numpy reference the GPU test
compares with equals a literal per-read, per-base loop on every case; every case's claims about itself hold; the tile-by-tile
restatement of the kernel equals both, and each of its one-line mutants is told apart by a case of the family listed for it.  Also the
text of the two files, which needs no GPU."""
import numpy as np
import pytest

import depth_dist_cases as D

N_CASES = 11


def test_constants_are_read_from_the_source():
    from tiddit_amd import tiddit_depth_dist
    assert D.CAP == tiddit_depth_dist.DD_CAP == 1000
    assert D.T >= 64 and D.T % 256 == 0
    assert D.parse_constants("#define DD_CAP 7   // x\n  #define DD_TILE 128\n") == {"DD_TILE": 128, "DD_CAP": 7}
    with pytest.raises(KeyError):
        D.parse_constants("#define DD_CAP (7)\n#define DD_TILE 128\n")


def test_case_list():
    assert len(D.CASES) == N_CASES
    assert {c["family"] for c in D.CASES} == {"tile", "ends", "records", "values", "multi", "state"} == set(D.MUTANTS.values()) | {"multi", "state"}
    for c in D.CASES:
        assert max(c["lengths"]) <= 4 * D.T + 3 and len(c["records"]) <= 4000, c["name"]
        keys = [(r[0], r[1]) for r in c["records"]]
        assert keys == sorted(keys), c["name"]                       # a coordinate-sorted file
        assert all(0 <= r[0] < len(c["lengths"]) for r in c["records"])
        if c["order"] is not None:
            assert sorted(c["order"]) == list(range(len(c["lengths"])))
    assert any(c["order"] for c in D.CASES) and any(c["batches"] and c["capacity"] for c in D.CASES)
    assert any(0 in c["lengths"] for c in D.CASES)


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_reference_equals_the_literal_loop_and_the_claims_hold(case):
    lengths, records = case["lengths"], case["records"]
    lit = D.literal(lengths, records)
    dep = D.depths(lengths, records)
    for t in range(len(lengths)):
        assert np.array_equal(dep[t], np.array(lit[t], dtype=np.int64)), (case["name"], t)
    ref = D.reference(lengths, records)
    assert ref.shape == (len(lengths), D.CAP + 4) and ref.dtype == np.int64
    for t, LN in enumerate(lengths):
        d = np.array(lit[t], dtype=np.int64)
        assert ref[t, :D.CAP + 1].sum() == LN
        assert ref[t, D.CAP + 1] == d.sum() and ref[t, D.CAP + 2] == (d.max() if LN else 0) and ref[t, D.CAP + 3] == (d.min() if LN else 0)
        for k in range(D.CAP):
            if ref[t, k]:
                assert ref[t, k] == (d == k).sum()
        assert ref[t, D.CAP] == (d >= D.CAP).sum()
    assert np.array_equal(D.restatement(lengths, records), ref)
    sp = D.spans(lengths, records)
    assert case["claims"]
    for claim in case["claims"]:
        kind = claim[0]
        if kind == "start":
            assert records[claim[1]][1] == claim[2], claim
        elif kind == "end":
            assert records[claim[1]][2] == claim[2], claim
        elif kind == "depth":
            assert lit[claim[1]][claim[2]] == claim[3], claim
        elif kind == "max":
            assert max(lit[claim[1]]) == claim[2], claim
        elif kind == "min":
            assert min(lit[claim[1]]) == claim[2], claim
        elif kind == "bin":
            assert ref[claim[1], claim[2]] == claim[3], claim
        elif kind == "tiles":
            assert -(-lengths[claim[1]] // D.T) == claim[2], claim
        elif kind == "span_over_tile":
            assert sp[claim[1]] > D.T, claim
        else:
            raise AssertionError(claim)


def test_edges_named_by_the_families_are_really_there():
    """reads on lo-1, lo, lo+1, hi-1, hi of a tile as starts and as ends; contigs of 1, T-1, T, T+1 bases; overhangs of 1 and of more
    than a tile; both degenerate records; every filter combination; both sides of min_q; depths CAP-1, CAP, CAP+1"""
    T, CAP = D.T, D.CAP
    by = {}
    for c in D.CASES:
        by.setdefault(c["family"], []).append(c)
    starts = {r[1] for c in by["tile"] for r in c["records"]}
    ends = {r[2] for c in by["tile"] for r in c["records"]}
    assert {T - 1, T, T + 1, 2 * T - 1, 2 * T} <= starts and {T - 1, T, T + 1, 2 * T - 1, 2 * T} <= ends
    assert any((r[1], r[2]) == (2 * T, 3 * T) for c in by["tile"] for r in c["records"])
    assert any(len(c["records"]) == 1 and c["records"][0][1] < T and c["records"][0][2] > 3 * T for c in by["tile"])
    assert {1, T - 1, T, T + 1} <= {n for c in by["ends"] for n in c["lengths"]}
    over = {r[2] - c["lengths"][r[0]] for c in by["ends"] for r in c["records"]}
    assert 0 in over and 1 in over and any(o > T for o in over)
    rs = [r for c in by["records"] for r in c["records"]]
    assert any(r[2] == r[1] for r in rs) and any(r[2] < r[1] for r in rs)
    combos = {(bool(r[4] & D.UNMAPPED), bool(r[4] & D.DUPLICATE), r[3] < D.MIN_Q) for r in rs if r[2] > r[1]}
    assert len(combos) == 8
    assert {D.MIN_Q - 1, D.MIN_Q} <= {r[3] for r in rs}
    assert any(n and not any(r[0] == t for r in c["records"]) and 0 < t < len(c["lengths"]) - 1
               for c in by["records"] for t, n in enumerate(c["lengths"]))
    reached = {int(v) for c in by["values"] for d in D.depths(c["lengths"], c["records"]) for v in np.unique(d)}
    assert {CAP - 1, CAP, CAP + 1} <= reached
    assert any(D.reference(c["lengths"], c["records"])[0, CAP + 3] > 0 for c in by["values"])
    multi = by["multi"][0]
    assert {-(-n // T) for n in multi["lengths"]} >= {1, 2, 3, 4}


@pytest.mark.parametrize("mutant", sorted(D.MUTANTS))
def test_every_mutant_is_told_apart_by_its_family(mutant):
    family = D.MUTANTS[mutant]
    told = [c["name"] for c in D.CASES if c["family"] == family and
            not np.array_equal(D.restatement(c["lengths"], c["records"], mutant=mutant), D.reference(c["lengths"], c["records"]))]
    assert told, (mutant, family)


def test_the_two_files(tmp_path):
    """write_files on a table small enough to read: rows only for bases > 0, `1000+` for the last bin, fractions at or above over the
    contig's length, the total block the element-wise sum, mean = sum of depths / length"""
    from tiddit_amd import tiddit_depth_dist as M
    table = np.zeros((3, M.DD_CAP + 4), dtype=np.int64)
    table[0, 0], table[0, 2], table[0, M.DD_CAP] = 6, 3, 1
    table[0, M.SUM], table[0, M.MAX], table[0, M.MIN] = 6 + 1500, 1500, 0
    table[1, 0] = 7
    table[2, 3] = 3
    table[2, M.SUM], table[2, M.MAX], table[2, M.MIN] = 9, 3, 3
    prefix = str(tmp_path / "o")
    M.write_files(prefix, ["a", "b", "c"], [10, 7, 3], table)
    assert open(prefix + ".depth_dist.tab").read() == (
        "#contig\tdepth\tbases\tfraction_at_or_above\n"
        "a\t0\t6\t1.000000\na\t2\t3\t0.400000\na\t1000+\t1\t0.100000\n"
        "b\t0\t7\t1.000000\n"
        "c\t3\t3\t1.000000\n"
        "total\t0\t13\t1.000000\ntotal\t2\t3\t0.350000\ntotal\t3\t3\t0.200000\ntotal\t1000+\t1\t0.050000\n")
    assert open(prefix + ".depth_summary.tab").read() == (
        "#contig\tlength\tbases\tmean\tmin\tmax\n"
        "a\t10\t1506\t150.60\t0\t1500\nb\t7\t0\t0.00\t0\t0\nc\t3\t9\t3.00\t3\t3\ntotal\t20\t1515\t75.75\t0\t1500\n")
    assert M.parse_switch(None) is False and M.parse_switch("") is False and M.parse_switch("1") is True
    for bad in ("2", "0", "yes", " 1"):
        with pytest.raises(ValueError):
            M.parse_switch(bad)
