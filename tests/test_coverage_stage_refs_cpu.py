"""CPU pin of tests/coverage_stage_cases.py: the constant parser, the two references against each other and against the real
update_coverage's bins (tests/golden/coverage_edges.npz), the claims of every case against what its family promises, and the
departures of the restatement that the cases must notice.  No GPU."""
import os

import numpy as np
import pytest

import coverage_stage_cases as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coverage_edges.npz")


def test_the_case_set_is_the_one_the_gpu_file_states():
    assert (cc.N_CASES, cc.N_PAIRS) == (377, 2100)
    fam = {f: len(cc.case_names(f)) for f in "ABCDEFGH"}
    assert fam == {"A": 30, "B": 14, "C": 28, "D": 21, "E": 189, "F": 20, "G": 72, "H": 3}, fam
    big = [n for n in cc.case_names() if max(cc.nbins_of(LN, cc.CASES[n]["z"]) for _, LN in cc.CASES[n]["contigs"]) > 1 << 24]
    assert len(big) <= 4                                           # at most one contig above 2^24 bins per bin-size class
    assert all(l in cc.ALL_LAYOUTS for n in cc.case_names() for l in cc.CASES[n]["layouts"])


def test_constants_are_read_from_the_sources():
    c = cc.CONSTANTS
    assert c["COV_THREADS"] % 64 == 0 and c["COV_READS_PER_BLOCK"] % (c["COV_THREADS"] * c["COV_RPL"]) == 0
    assert c["COV_PK_SPAN"] == 0xffffff
    hip = ("#define COV_THREADS 256\n#ifndef COV_RPL\n#define COV_RPL 8   // reads (4 or 8)\n#endif\n#define COV_RPL 4\n#define COV_RPL1 (COV_RPL / 2)\n"
           "#define COV_READS_PER_BLOCK (4u << 12)\n#define COV_WIN 2048\n#define COV_WIN1 COV_WIN\n#define COV_DQMAX 256\n"
           "#define COV_LUT_LDS_MAX 1024\n#define COV_KEPT_SLOTS 512\n")
    rec = "#define COV_PK_SPAN 0xffffffu\n"
    got = cc.parse_constants({"tdt_coverage.hip": hip, "tdt_cov_record.h": rec})
    assert got == {"COV_THREADS": 256, "COV_RPL": 8, "COV_RPL1": 4, "COV_READS_PER_BLOCK": 16384, "COV_WIN": 2048, "COV_WIN1": 2048,
                   "COV_DQMAX": 256, "COV_LUT_LDS_MAX": 1024, "COV_KEPT_SLOTS": 512, "COV_PK_SPAN": 0xffffff}
    with pytest.raises(KeyError):                                  # a constant that moved to the other file
        cc.parse_constants({"tdt_coverage.hip": hip + rec, "tdt_cov_record.h": ""})
    with pytest.raises(KeyError):                                  # ... that is gone
        cc.parse_constants({"tdt_coverage.hip": hip.replace("#define COV_DQMAX 256\n", ""), "tdt_cov_record.h": rec})
    with pytest.raises(KeyError):                                  # ... that is no longer an integer expression
        cc.parse_constants({"tdt_coverage.hip": hip.replace("COV_WIN 2048", "COV_WIN (sizeof(long) * 256)"), "tdt_cov_record.h": rec})


def test_dispatch_restates_the_host():
    for z, kind in ((1, "z1"), (2, "mode1"), (128, "mode1"), (129, "tabled"), (1023, "tabled"), (1024, "global"), (1 << 20, "global")):
        assert cc.dispatch(z)["kind"] == kind, z
    assert cc.dispatch(128, "binned", True)["flavour"] == "tabled/rec2" and cc.dispatch(128)["xmax"] == 256 * 128 == 32768
    assert cc.dispatch(50)["margin"] == cc.DQMAX + 8 and cc.dispatch(500)["margin"] == 5 and cc.dispatch(1)["margin"] == 644
    assert cc.dispatch(50)["TILE"] == cc.THREADS * cc.RPL1 and cc.dispatch(50, "packed", True)["TILE"] == cc.THREADS * cc.RPL0
    for z in (1, 1024):
        with pytest.raises(ValueError):
            cc.dispatch(z, "binned")


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("family", "ABCDEFGH")
def test_oracle_equals_restatement_equals_fixture(golden, family):
    names = list(golden["names"])
    seen = 0
    for name in cc.case_names(family):
        c = cc.get(name)
        if c["expect"] == cc.TDT_E_RANGE:
            # a kept read that leaves the contig's bins: the reference's IndexError.  start < 0 and end <= start are refused by the
            # library alone (include/tiddit_hip.h); the reference's arithmetic wraps or runs backwards there, and so does the oracle's
            with pytest.raises(cc.CoverageRangeError):
                cc.restatement(c)
            if "beyond" in name or name == "h_state_bad":
                with pytest.raises(IndexError):
                    cc.reference(c)
            continue
        want, kept = cc.restatement(c)
        ref, rkept = cc.reference(c)
        assert _same(ref, want) and rkept == kept, name
        assert all(v.dtype == np.float64 for _, v in want)
        if name in names:
            k = names.index(name)
            assert golden["hashes"][k] == cc.input_hash(c), (name, "the generator drifted: regenerate with tests/golden/make_golden.py")
            fix = [(golden["k%d_c%d_idx" % (k, ci)], golden["k%d_c%d_val" % (k, ci)]) for ci in range(len(c["contigs"]))]
            assert _same(fix, want), name
            seen += 1
        else:
            assert not cc.in_golden(c), name
    assert seen >= 1, family


def test_fixture_covers_every_class_and_is_small(golden):
    names = list(golden["names"])
    assert {cc.z_class(cc.CASES[n]["z"]) for n in names} == {1, 2, 3, 4}
    assert {cc.CASES[n]["family"] for n in names} == set("ABCDEFGH")
    assert names == [n for n in cc.case_names() if cc.in_golden(cc.CASES[n])]
    here = os.path.dirname(GOLDEN)
    assert os.path.getsize(GOLDEN) < max(os.path.getsize(os.path.join(here, f)) for f in os.listdir(here) if f != "coverage_edges.npz")


# ================================================================================================== claims
def test_every_case_lands_on_the_paths_it_names():
    for name in cc.case_names():
        c = cc.get(name)
        cl = c["claim"]
        assert cl["flavour"].startswith(cc.dispatch(c["z"])["kind"]), name
        for p in c["paths"]:
            assert cl[p] > 0, (name, p, cl["flavour"])
        if c["expect"] == "bins":
            assert cl["refused"] == 0, name
        elif c["expect"] == cc.TDT_E_RANGE:
            assert cl["refused"] >= 1, name
        for layout in c["layouts"]:                               # the model runs under every entry and flavour the GPU file uses
            for mode0 in ((False, True) if c["mode0"] else (False,)):
                m = cc.model(c, layout, mode0)
                assert m["refused"] == cl["refused"] or c["min_q"] > 63 or c["min_q"] < 0, (name, layout)


def test_family_a_has_every_geometry_in_every_slot():
    for z in cc.ALL_Z:
        c = cc.get("a_geometry_z%d" % z)
        d = cc.dispatch(z)
        geo = cc.a_geometries(z, d)
        assert set(c["claim"]["slots"]) == set(geo), z
        for g, at in c["claim"]["slots"].items():
            assert {s for s, _ in at} == set(range(d["RPL"])), (z, g)
            assert all(p in (1, 2, 3) for _, p in at), (z, g)
        slots = c["claim"]["slots"]
        if d["mode"] == 1:                                         # the register path ends exactly at xmax and at COV_DQMAX bins after K
            assert {p for s, p in slots["re1_xmax"] if s <= 1} == {1} and 1 not in {p for _, p in slots["re1_xmax_plus1"]}, z
            assert (0, 1) in slots["s0_e0_b%d" % (cc.DQMAX - 1)] and 1 not in {p for _, p in slots["s0_e0_b%d" % cc.DQMAX]}, z
            assert 1 not in {p for _, p in slots["s%d_e%d_b%d" % (z - 1, z - 1, cc.DQMAX + 1)]}, z
        elif z > 1:
            assert {p for s, p in slots["s0_e0_b1"] if s <= 2} == {1} and 1 not in {p for _, p in slots["s0_e0_b2"]}, z
        runs = cc.get("a_runs_z%d" % z)
        K = (runs["cols"][0][0][::d["RPL"]].astype(np.int64)) // z
        lengths = np.diff(np.flatnonzero(np.concatenate([[True], K[1:] != K[:-1], [True]])))
        assert lengths.tolist() == [1, 2, 63, 64, 65, 3], z


def test_family_b_meets_every_window_edge():
    for z in cc.B_Z:
        c = cc.get("b_window_z%d" % z)
        cl, d = c["claim"], cc.dispatch(z)
        assert len(cl["bases"]) == 1 and len(cl["bases"][0]) == 3, (z, cl["bases"])          # two re-bases in one workgroup
        assert 0 in cl["slack"] and -1 in cl["slack"] and cl["same_base"] == 1, (z, cl["slack"])
        assert cl["register"] and cl["literal_window"] and cl["literal_global"], z
        s, e = (a.astype(np.int64) for a in c["cols"][0][:2])
        m = cc.model_item(s, e, np.ones(len(s), bool), cc.nbins_of(c["contigs"][0][1], z), z, d)
        K = (s // z)[(np.arange(len(s)) // d["RPL"]) * d["RPL"]]
        base0 = cl["bases"][0][0]
        first_tile = np.arange(len(s)) < d["TILE"]
        for ko, path in ((d["safe_ko"] - 1, 1), (d["safe_ko"], 2), (d["safe_ko"] + 1, 2)):     # one below, on and above the limit
            sel = first_tile & (K - base0 == ko)
            assert sel.any(), (z, ko)
            if d["kind"] in ("tabled", "mode1"):                   # (bin size 1 and >= 1024 have no `safe`: every sum goes through `contribute`)
                assert ((m["path"][sel] == 1) if path == 1 else (m["path"][sel] >= 2)).all(), (z, ko)
        eb = (e - 1) // z
        for last, path in ((base0 + d["WIN"] - 1, 2), (base0 + d["WIN"], 3), (base0 + d["WIN"] + 5, 3)):
            sel = first_tile & (eb == last) & (s // z == base0 + d["WIN"] - 3)
            assert sel.any() and (m["path"][sel] == path).all(), (z, last)
        front = first_tile & (s // z < base0)                      # in front of the window: whole lanes, and one sibling of a lane inside it
        assert front.sum() >= d["RPL"] + 1 and (m["path"][front] >= (3 if d["kind"] in ("tabled", "mode1") else 1)).all(), z
        assert m["path"][front][-1] == 3, z
        behind = ~first_tile & (s // z == base0)                   # reads after a re-base that lie behind the new window
        assert behind.sum() >= 2 * d["RPL"] and (m["path"][behind & (np.arange(len(s)) >= 2 * d["TILE"])] >= (3 if d["kind"] in ("tabled", "mode1") else 1)).all(), z
        lim = cc.get("b_last_bin_limit_z%d" % z)
        paths = cc.model(lim, "arrays")
        if d["kind"] in ("tabled", "mode1"):
            assert (paths["register"], paths["literal_window"]) == (2 * d["RPL"], d["RPL"]), (z, paths)


# ================================================================================================== mutants
@pytest.mark.parametrize("mutant", cc.MUTANTS)
def test_every_departure_is_noticed_in_every_family_it_is_listed_for(mutant):
    for family in cc.MUTANT_FAMILIES[mutant]:
        hit = 0
        for name in cc.case_names(family):
            c = cc.get(name)
            if c["expect"] != "bins" or c["n"] > 200_000:
                continue
            try:
                got = cc.restatement(c, mutant)
            except cc.CoverageRangeError:
                hit += 1
                continue
            want = cc.restatement(c)
            hit += not (_same(got[0], want[0]) and got[1] == want[1])
        assert hit >= 1, (mutant, family)


def test_no_departure_is_equivalent():
    """every listed departure changes some result, so none had to be asserted equivalent; the two that cannot show at bin size 1 (a read
    never has a last bin apart from its first there... it has: bases in the last bin are then 0 of 1) are checked on that class too"""
    c = cc.get("d_contig_end_z1")
    assert not _same(cc.restatement(c, "no_one_short")[0], cc.restatement(c)[0])
    # bin size 1: end_bin_size is always 1 == z, so the two last-bin denominators cannot differ
    for mutant in ("z_in_last_bin", "end_bin_size_for_single"):
        assert _same(cc.restatement(c, mutant)[0], cc.restatement(c)[0]), mutant
