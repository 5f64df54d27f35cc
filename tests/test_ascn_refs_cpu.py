"""`TIDDIT_ASCN` on the CPU: the definition of tiddit_amd/tiddit_ascn.py (``define_contig``) against the three references of
tests/ascn_cases.py — the literal loops, the dense 16 x 16 chain, the enumeration of all paths — on every case the GPU tests use; every
one-line mutant of the loops told apart inside the family listed for it; the planted stage input yields its plants and nothing else;
the host-side segment former, the file text, the switch parser and its "needs both switches" error.  Nothing here needs a GPU.

Every test of this file fails on the parent commit: tiddit_amd/tiddit_ascn.py does not exist there."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import ascn_cases as C
from tiddit_amd import tiddit_ascn, tiddit_cnv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constants_and_states():
    assert (tiddit_ascn.BU, tiddit_ascn.ACAP, tiddit_ascn.HOM, tiddit_ascn.MIN_N, tiddit_ascn.S) == (C.BU, C.ACAP, C.HOM, C.MIN_N, 16)
    assert (tiddit_cnv.UNIT, tiddit_cnv.CAP, tiddit_cnv.LAMBDA) == (C.UNIT, C.CAP, C.LAMBDA)
    assert list(tiddit_ascn.STATES) == C.CM and list(tiddit_ascn.MU) == C.MU_OF and tiddit_ascn.HEADER == C.HEADER
    assert [tiddit_ascn.home_of(P) for P in range(1, 7)] == [1, 3, 5, 8, 11, 15]
    assert C.CHUNK == 256


@pytest.mark.parametrize("case", C.VITERBI_CASES, ids=[c["name"] for c in C.VITERBI_CASES])
def test_loop_equals_dense_equals_brute_force(case):
    for (E, home), (s, cost, ties, args) in zip(case["contigs"], C.viterbi_reference(case)):
        if not len(E):
            continue
        d, dcost = C.dense_viterbi(E, home, case["lam"])
        assert np.array_equal(d, s) and dcost == cost == C.path_cost(E, home, s, case["lam"])
        if len(E) <= 4:
            assert C.brute_force_cost(E, home, case["lam"]) == cost
    cl = case["claims"]
    s0, cost0, ties0, args0 = C.viterbi_reference(case)[0]
    if "path" in cl:
        assert s0.tolist() == cl["path"]
    if "tie" in cl:
        assert cl["tie"] in ties0
    if "arg" in cl:
        assert args0 == {cl["arg"]} and s0[cl["jump_at"] - 1] != s0[cl["jump_at"]]
    if cl.get("all_home"):
        assert all((s == h).all() for (E, h), (s, _, _, _) in zip(case["contigs"], C.viterbi_reference(case)))
    if "cost_above" in cl:
        assert cost0 > cl["cost_above"]


def test_the_viterbi_cases_cover_what_they_claim():
    by = {}
    for c in C.VITERBI_CASES:
        by.setdefault(c["family"], []).append(c)
    assert sorted(len(E) for c in by["size"] for E, _ in c["contigs"]) == [1, 2, 255, 256, 257, 511, 512, 513, 65 * 256 + 1]
    assert sorted(len(c["contigs"]) for c in by["multi"]) == [9, 9, 300] and sum(len(E) == 1 for E, _ in by["multi"][2]["contigs"]) >= 150
    assert [h for _, h in by["home"][0]["contigs"]] == list(range(16))
    assert {c["claims"]["arg"] for c in by["argmin"]} == set(range(15)) and {c["claims"]["jump_at"] for c in by["argmin"]} == {255, 256}
    # (state 15 is the argmin wherever a run at 15 is left)
    used = set()
    for c in by["home"] + by["size"]:
        for r in C.viterbi_reference(c):
            used |= r[3]
    assert 15 in used
    assert sorted(c["lam"] for c in by["lambda"]) == [0, 1 << 28]
    assert max(int(E.max()) for c in C.VITERBI_CASES for E, _ in c["contigs"] if len(E)) == 1 << 28
    assert min(int(E.min()) for c in C.VITERBI_CASES for E, _ in c["contigs"] if len(E)) >= 0


@pytest.mark.parametrize("mutant", ["bp_lt", "argmin_high"])
def test_a_viterbi_mutant_is_told_apart_inside_its_family(mutant):
    family = [c for c in C.VITERBI_CASES if c["family"] == C.MUTANTS[mutant]]
    differs = [c["name"] for c in family
               if any(C.ref_viterbi(E.tolist(), h, c["lam"], mutant=mutant) != s.tolist() for (E, h), (s, _, _, _) in zip(c["contigs"], C.viterbi_reference(c)) if len(E))]
    assert len(differs) >= 3, differs


@pytest.mark.parametrize("case", C.EMISSIONS_CASES, ids=[c["name"] for c in C.EMISSIONS_CASES])
def test_the_definition_s_emissions_equal_the_loop(case):
    E, ns, sb = C.emissions_reference(case)
    at = 0
    for c in case["contigs"]:
        if not c["processed"]:
            continue
        T = len(c["x"])
        e, n, b, s, _ = tiddit_ascn.define_contig(c["x"], 2, c["W"], T * c["W"], "c", c["pos"], c["ref_n"], c["alt_n"])
        assert np.array_equal(np.array(e).reshape(-1, 16), E[at:at + T]) and n == ns[at:at + T].tolist() and b == sb[at:at + T].tolist()
        assert s == C.ref_viterbi(e, 3) and np.array_equal(C.dense_viterbi(e, 3)[0], s)
        at += T
    assert at == len(E) and 0 <= E.min() and E.max() < 1 << 28


def test_the_emissions_cases_cover_what_they_claim():
    by = {c["name"]: c for c in C.EMISSIONS_CASES}
    E, ns, sb = C.emissions_reference(by["0, 1 and 3200 sites at the largest scores"])
    assert ns.tolist() == [0, 1, 3200] and E[2].max() == C.CAP + 3200 * C.ACAP and sb[2] == 3200 * 256
    E, ns, sb = C.emissions_reference(by["n = MIN_N - 1 and MIN_N"])
    assert ns.sum() == 5
    E, ns, sb = C.emissions_reference(by["masked bins with and without sites"])
    assert ns.tolist() == [1, 0, 1, 1] and not E[1].any() and E[0].any()
    E, ns, sb = C.emissions_reference(by["a site behind the last bin"])
    assert ns.tolist() == [0, 1]
    c = by["bin edges, short last bin"]["contigs"][0]
    assert set(c["pos"].tolist()) >= {499, 500, 501, 1729} and len(c["x"]) * c["W"] > 1730
    cols = by["all 12 (REF, ALT) column pairs"]["contigs"][0]["cols"]
    assert len({tuple(r) for r in cols.tolist()}) == 12
    pairs = by["every pair with n <= 64"]["contigs"][0]
    assert len(pairs["pos"]) == 65 * 66 // 2
    assert any(v == (1 << 32) - 1 for v in by["ref_n == alt_n, alt_n == 0, counters of 2^32 - 1"]["contigs"][0]["ref_n"])


@pytest.mark.parametrize("mutant", ["no_hom", "beta_round", "bin_edge", "min_n"])
def test_an_emissions_mutant_is_told_apart_inside_its_family(mutant):
    family = [c for c in C.EMISSIONS_CASES if c["family"] == C.MUTANTS[mutant]]
    assert family and all(any(not np.array_equal(a, b) for a, b in zip(C.emissions_reference(c), C.emissions_reference(c, mutant))) for c in family)


def _overlap(seg, lo, hi):
    return max(0, min(seg[2], hi) - max(seg[1], lo))


def test_the_planted_stage_yields_its_plants_and_nothing_else():
    text, skipped, tracks, detail = C.planted_reference()
    (coverage, gcs, library, contigs, length, min_contig, W), table, sites, number = C.planted_job()
    assert skipped == ["tiny"] and set(tracks) == {"chrA", "chrN", "chrH"}
    lines = [l.split("\t") for l in text.split("\n")[1:] if l]
    on_a = [(l[0], int(l[1]), int(l[2]), l[3], int(l[4]), int(l[5])) for l in lines if l[0] == "chrA"]
    assert len(on_a) == len(C.PLANTED["plants"]) and len(lines) == len(on_a), text
    for seg, (kind, c, m, lo, hi) in zip(on_a, C.PLANTED["plants"]):
        assert seg[3:] == (kind, c, m) and _overlap(seg, lo * W, hi * W) >= 0.9 * (hi - lo) * W and seg[2] - seg[1] <= 1.1 * (hi - lo) * W, seg
    # the definition of the module on the same input: the same file
    cols = tiddit_ascn.site_columns(sites)
    segs = []
    for c in contigs:
        if c in tracks:
            lo, hi = int(sites.site_off[number[c]]), int(sites.site_off[number[c] + 1])
            k = np.arange(lo, hi)
            out = tiddit_ascn.define_contig(tracks[c][0], library["contig_ploidy_" + c], W, length[c], c, sites.site_pos[lo:hi],
                                            table[k, cols[lo:hi, 0]], table[k, cols[lo:hi, 1]])
            assert out[0] == detail[c][0] and out[3] == detail[c][3]
            segs += out[4]
    assert tiddit_ascn.text_of(segs) == text
    # ... and the numpy segment former on the definition's states
    used = [c for c in contigs if c in tracks]
    ploidy = [library["contig_ploidy_" + c] for c in used]
    chains = tiddit_cnv.chain_table([(len(tracks[c][0]), 0) for c in used])
    chains[:, 2] = [tiddit_ascn.home_of(P) for P in ploidy]
    cat = lambda i: np.concatenate([np.asarray(detail[c][i]) for c in used])
    got = tiddit_ascn.segments_of(cat(3).astype(np.int8), np.concatenate([np.asarray(tracks[c][0]) for c in used]), cat(1), cat(2), chains, ploidy, W,
                                  [length[c] for c in used], used)
    assert tiddit_ascn.text_of(got) == text


def test_the_segment_former_trims_empty_bins_and_types_every_kind():
    """runs of every type, EMPTY bins at both ends of a run, a run of only EMPTY bins, a masked bin with sites, runs that end with
    their contig — against the loop"""
    P = [4, 2]
    home = [tiddit_ascn.home_of(p) for p in P]
    s0 = [8] * 3 + [7] * 5 + [8] * 2 + [6] * 4 + [3] * 3 + [12] * 4 + [8] + [2] * 3
    x0 = [1024] * 3 + [-1, -1, 1000, -1, -1] + [1024] * 2 + [-1] * 4 + [700, -1, 800] + [-1, 1500, 1600, -1] + [1024] + [-1, 512, -1]
    n0 = [0] * 3 + [0, 2, 1, 0, 0] + [1, 0] + [0, 2, 0, 0] + [0, 1, 0] + [0, 0, 3, 0] + [0] + [0, 0, 4]
    s1 = [2] * 2 + [3] * 2 + [1] * 3 + [3] + [4] * 2
    x1 = [500, -1, 512, 512, 260, 250, -1, 512, -1, -1]
    n1 = [0, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    sb0, sb1 = [37 * v for v in n0], [11 * v for v in n1]
    want = C.ref_segments(s0, x0, n0, sb0, 4, 500, len(s0) * 500 - 7, "a") + C.ref_segments(s1, x1, n1, sb1, 2, 500, len(s1) * 500 - 100, "b")
    assert [w[3] for w in want] == ["AI", "LOH", "DEL", "DUP", "DEL", "LOH", "DEL"]        # (the last run of b is all EMPTY)
    chains = np.array([(0, len(s0), home[0]), (len(s0), len(s1), home[1])], dtype=np.int64)
    got = tiddit_ascn.segments_of(np.array(s0 + s1, dtype=np.int8), np.array(x0 + x1), np.array(n0 + n1), np.array(sb0 + sb1), chains, P, 500,
                                  [len(s0) * 500 - 7, len(s1) * 500 - 100], ["a", "b"])
    assert got == want
    assert any(w[8] == "." for w in want) and any(w[9] == "." for w in want)
    assert tiddit_ascn.segments_of(np.zeros(0, dtype=np.int8), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 3)), [], 500, [], []) == []


def test_the_file_text(tmp_path):
    seg = [("chr1", 0, 1500, "LOH", 2, 0, 3, 2, "1.992", "0.012"), ("chr2", 500, 730, "AI", 4, 1, 0, 5, ".", "0.250")]
    tiddit_ascn.write_bed(str(tmp_path / "o.ascn.bed"), seg)
    assert open(str(tmp_path / "o.ascn.bed")).read() == C.HEADER + "chr1\t0\t1500\tLOH\t2\t0\t3\t2\t1.992\t0.012\nchr2\t500\t730\tAI\t4\t1\t0\t5\t.\t0.250\n"
    tiddit_ascn.write_bed(str(tmp_path / "e.ascn.bed"), [])
    assert open(str(tmp_path / "e.ascn.bed")).read() == C.HEADER


def test_the_columns_of_a_site_are_those_of_its_first_row():
    sites = types.SimpleNamespace(rows=[("c", 5, "G", "T", 1), ("c", 2, "A", "C", 0), ("c", 5, "T", "G", 1), ("c", 9, "C", "A", 2)], site_pos=[1, 4, 8])
    sites_len = type("S", (), {"__len__": lambda self: 3, "rows": sites.rows})()
    assert tiddit_ascn.site_columns(sites_len).tolist() == [[0, 1], [2, 3], [1, 0]]


def test_the_switch_parser():
    on = ("sites.vcf", 13)
    assert tiddit_ascn.parse_switch(None, 500, on) is False and tiddit_ascn.parse_switch("", None, None) is False
    assert tiddit_ascn.parse_switch("1", 500, on) is True
    for value, cnv, alleles, word in (("1", None, on, "TIDDIT_CNV is not set"), ("1", 500, None, "TIDDIT_ALLELES is not set"),
                                      ("1", None, None, "TIDDIT_CNV and TIDDIT_ALLELES are not set"), ("0", 500, on, "the switch is 1"),
                                      ("yes", 500, on, "the switch is 1")):
        with pytest.raises(ValueError) as e:
            tiddit_ascn.parse_switch(value, cnv, alleles)
        assert word in str(e.value)


@pytest.mark.parametrize("env", [{"TIDDIT_ASCN": "1"}, {"TIDDIT_ASCN": "1", "TIDDIT_CNV": "1"}, {"TIDDIT_ASCN": "2", "TIDDIT_CNV": "1"}])
def test_the_switch_without_its_partners_is_refused_before_anything_is_made(tmp_path, env):
    """the command line, before it looks at its files: one error line, exit status 1, nothing made (no GPU is touched)"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("TIDDIT_")}
    e.update(env)
    out = str(tmp_path / "o")
    r = subprocess.run([sys.executable, "-m", "tiddit_amd", "--sv", "--bam", str(tmp_path / "no.bam"), "--ref", str(tmp_path / "no.fa"), "-o", out,
                        "--skip_assembly"], cwd=REPO, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    errors = [l for l in r.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_ASCN=%s:" % env["TIDDIT_ASCN"])
    assert os.listdir(str(tmp_path)) == []
