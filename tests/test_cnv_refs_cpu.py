"""The references and cases of tests/cnv_cases.py, checked without a GPU: the literal definition, the numpy restatement and (for five
bins and fewer) the enumeration of all paths agree on every case; every property a case claims holds in the reference; every
one-line misreading of the definition is caught inside the family listed for it; and the planted depth track yields exactly its two
segments.  tests/test_gpu_cnv.py then holds the device to the same references.

Every test of this file fails on the parent commit: tiddit_amd/tiddit_cnv.py and csrc/tdt_cnv.hip (whose CNV_CHUNK the cases read)
do not exist there."""
import numpy as np
import pytest

import cnv_cases as C

U, L = C.UNIT, C.CHUNK


def test_the_constants_are_the_product_s():
    from tiddit_amd import tiddit_cnv
    assert (tiddit_cnv.UNIT, tiddit_cnv.STATES, tiddit_cnv.CAP, tiddit_cnv.LAMBDA, tiddit_cnv.MIN_CLASS) == (C.UNIT, C.STATES, C.CAP, C.LAMBDA, C.MIN_CLASS)
    assert tiddit_cnv.HEADER == C.HEADER and L >= 16 and (C.CAP, C.LAMBDA) == (4 * U * U, 2 * U * U)


def test_the_case_lists_are_the_ones_the_gpu_tests_count():
    assert len(C.VITERBI_CASES) == 57 and len(C.BINS_CASES) == 18
    assert len({c["name"] for c in C.VITERBI_CASES}) == 57 and len({c["name"] for c in C.BINS_CASES}) == 18
    assert sorted({c["contigs"][0][0].shape[0] for c in C.VITERBI_CASES if c["family"] == "size"}) == [1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 1, 300 * L + 1]
    multi = [c for c in C.VITERBI_CASES if c["family"] == "multi"]
    assert [len(x) for x, _ in multi[0]["contigs"]] == [0, 1, L, L + 1, 3, 2 * L]
    assert sorted(len(x) for x, _ in multi[1]["contigs"]) == sorted([0, 1, L, L + 1, 3, 2 * L]) and [len(x) for x, _ in multi[1]["contigs"]] != [0, 1, L, L + 1, 3, 2 * L]


@pytest.mark.parametrize("case", C.VITERBI_CASES, ids=[c["name"] for c in C.VITERBI_CASES])
def test_the_three_references_agree(case):
    for (x, P), (s, cost, ties) in zip(case["contigs"], C.viterbi_reference(case)):
        if not len(x):
            assert len(s) == 0
            continue
        s2, cost2 = C.numpy_viterbi(x, P)
        assert np.array_equal(s, s2) and cost == cost2
        assert C.path_cost([int(v) for v in x], P, [int(v) for v in s]) == cost        # the path is worth what the forward pass says
        if len(x) <= 5:
            assert C.brute_force_cost(x, P) == cost


def test_enumeration_on_every_short_track_of_extreme_values():
    """all tracks of up to three bins over a handful of values (masked, state centres, midpoints, the clamp) and three ploidies"""
    import itertools
    values = (-1, 0, U // 2, U, U + U // 2, 2 * U, 3 * U, 8 * U)
    n = 0
    for T in (1, 2, 3):
        for x in itertools.product(values, repeat=T):
            for P in (1, 2, 6):
                d = {}
                s = C.ref_viterbi(list(x), P, details=d)
                assert d["cost"] == C.brute_force_cost(x, P) == C.path_cost(list(x), P, s)
                assert np.array_equal(C.numpy_viterbi(x, P)[0], s)
                n += 1
    assert n == 3 * (8 + 64 + 512)


@pytest.mark.parametrize("case", C.VITERBI_CASES, ids=[c["name"] for c in C.VITERBI_CASES])
def test_every_claim_of_a_case_holds(case):
    claims = case["claims"]
    (x, P), (s, cost, ties) = case["contigs"][0], C.viterbi_reference(case)[0]
    if "T" in claims:
        assert len(x) == claims["T"] and (len(x) < 20 or len(set(s.tolist())) > 1)
    if "change_at" in claims:
        p = claims["change_at"]
        assert s[p - 1] != s[p], "a change point between bins %d and %d" % (p - 1, p)
        assert p in (L - 2, L - 1, L, L + 1)          # L - 1 is the last bin of chunk 0, L the first of chunk 1
    if claims.get("all_P"):
        assert (s == P).all()
    if "run" in claims:
        lo, hi, cn = claims["run"]
        assert (s[lo:hi] == cn).all() and cn != P and (lo == 0 or s[lo - 1] != cn) and (hi == len(s) or s[hi] != cn)
    if "tie" in claims:
        t, k = claims["tie"]
        assert (t, k) in ties and s[t] == k, "V_{t-1}(k) == m + LAMBDA on the path"
    if "midway" in claims:
        lo, hi = claims["midway"]
        assert all(C.emission(int(v), 1) == C.emission(int(v), 2) == (U // 2) ** 2 for v in x[lo:hi])
    if "capped_at" in claims:
        t = claims["capped_at"]
        assert (int(x[t]) - U * P) ** 2 > C.CAP == C.emission(int(x[t]), P)
    if "cap_edges" in claims:
        a, b, c = claims["cap_edges"]
        assert [(int(x[t]) - U * P) ** 2 - C.CAP for t in (a, b, c)] == [1 - 4 * U, 0, 4 * U + 1]
    if "cost_above" in claims:
        assert cost > claims["cost_above"]
    if case["family"] == "masked":
        assert (x < 0).any()
    if case["family"] == "seam" or "seam" in case["name"]:
        assert len(x) > L


@pytest.mark.parametrize("case", C.BINS_CASES, ids=[c["name"] for c in C.BINS_CASES])
def test_the_bins_reference_against_numpy(case):
    """the same bins with numpy's own left-to-right accumulation (cumsum) and rint"""
    for (cov, gc, K, P, E), want in zip(case["contigs"], C.bins_reference(case)):
        got = []
        for t in range(-(-len(cov) // K)):
            g = gc[t * K:(t + 1) * K]
            use = g != -1
            if 2 * use.sum() < K:
                got.append(-1)
                continue
            obs = np.cumsum(cov[t * K:(t + 1) * K][use])[-1]
            exp = np.cumsum(E[g[use]])[-1]
            got.append(min(8 * case["unit"], int(np.rint(obs / exp * float(P * case["unit"])))))
        assert got == want.tolist()


def test_the_claims_of_the_bins_cases():
    by = {c["name"]: c for c in C.BINS_CASES}
    assert C.bins_reference(by["2^53, 1, 1"])[0].tolist() == [0] and C.bins_reference(by["2^53, 1, 1"])[1].tolist() == [1]
    x = C.bins_reference(by["rint ties, P=2"])[0]
    assert x.tolist() == [n + (n & 1) for n in range(40)]                    # n + 0.5 goes to the even neighbour: both parities
    x = C.bins_reference(by["the clamp at 8 UNIT"])[0]
    assert x.tolist() == [8 * U, 8 * U - 1, 8 * U, 8 * U, int(np.rint(7.998 * U)), 8 * U, 0]
    for K in (1, 2, 10, 64):
        c = by["half usable, K=%d" % K]
        cov, gc, _, _, _ = c["contigs"][0]
        x = C.bins_reference(c)[0]
        n = (gc.reshape(-1, K) != -1).sum(axis=1)
        assert ((x == -1) == (2 * n < K)).all() and (2 * n == K).any() == (K % 2 == 0) and (x == -1).any() and (x >= 0).any()
        if K > 2:
            assert (2 * n == K - 1).any() or (2 * n == K - 2).any()
    assert [a.tolist() for a in C.bins_reference(by["short last bin"])] == [[2 * U, 2 * U, 2 * U], [2 * U, 2 * U, -1], [2 * U] * 4]
    assert sorted(c[3] for c in by["P = 1 .. 6 in one call"]["contigs"]) == [1, 2, 3, 4, 5, 6]
    assert {c[2] for c in C.BINS_CASES[0]["contigs"] + C.BINS_CASES[1]["contigs"] + C.BINS_CASES[2]["contigs"] + C.BINS_CASES[3]["contigs"]} == {1, 2, 10, 64}
    assert all(len(c["contigs"][0][0]) % c["contigs"][0][2] for c in C.BINS_CASES[1:4])         # nb is no multiple of K


@pytest.mark.parametrize("mutant", sorted(C.MUTANTS))
def test_every_misreading_is_caught_inside_its_family(mutant):
    family = C.MUTANTS[mutant]
    caught = []
    for case in C.VITERBI_CASES:
        if case["family"] != family:
            continue
        for (x, P), (s, _, _) in zip(case["contigs"], C.viterbi_reference(case)):
            if len(x) and C.ref_viterbi([int(v) for v in x], P, mutant=mutant) != s.tolist():
                caught.append(case["name"])
    for case in C.BINS_CASES:
        if case["family"] != family:
            continue
        for (cov, gc, K, P, E), want in zip(case["contigs"], C.bins_reference(case)):
            if C.ref_bins(cov, gc, K, P, E, unit=case["unit"], mutant=mutant) != want.tolist():
                caught.append(case["name"])
    assert caught, "no case of family %r tells %r from the definition" % (family, mutant)


def test_segments_of_equals_the_literal_loop():
    from tiddit_amd import tiddit_cnv
    rng = np.random.default_rng(3)
    for trial in range(200):
        T = int(rng.integers(1, 60))
        P = int(rng.integers(1, 7))
        s = np.repeat(rng.integers(0, 8, T), rng.integers(1, 6, T))[:T].astype(np.int8)
        x = rng.integers(0, 8 * U + 1, T).astype(np.int32)
        x[rng.random(T) < 0.3] = -1
        W = int(rng.choice([50, 500, 3200]))
        length = T * W - int(rng.integers(0, W))
        assert tiddit_cnv.segments_of(s, x, P, W, length, "c") == C.ref_segments(s.tolist(), x.tolist(), P, W, length, "c")
    assert tiddit_cnv.segments_of(np.zeros(0, dtype=np.int8), np.zeros(0, dtype=np.int32), 2, 500, 0, "c") == []


def test_parse_switch():
    from tiddit_amd import tiddit_cnv
    assert tiddit_cnv.parse_switch(None) is None and tiddit_cnv.parse_switch("") is None
    assert tiddit_cnv.parse_switch("1") == 500
    assert [tiddit_cnv.parse_switch(str(w)) for w in (50, 100, 500, 3200)] == [50, 100, 500, 3200]
    for bad in ("0", "75", "3250", "x", "-500", "500.0", " 500", "25", "2"):
        with pytest.raises(ValueError):
            tiddit_cnv.parse_switch(bad)


def test_tables():
    from tiddit_amd import tiddit_cnv
    assert tiddit_cnv.bin_table([(0, 25, 10, 2), (25, 0, 10, 1), (25, 64, 64, 3)]).tolist() == [[0, 25, 10, 2, 0], [25, 0, 10, 1, 3], [25, 64, 64, 3, 3]]
    assert tiddit_cnv.chain_table([(3, 2), (0, 1), (1, 3)]).tolist() == [[0, 3, 2], [3, 0, 1], [3, 1, 3]]
    lower, upper = np.full((2, 101), 10.0), np.full((2, 101), 12.0)
    count = np.zeros((2, 101), dtype=np.int64)
    count[0, 40], count[0, 41], count[1, 40] = 100, 99, 101
    E = tiddit_cnv.expected_depth(lower, upper, count, [30.0, 50.0])
    assert E[0, 40] == 11.0 and E[0, 41] == 30.0 and E[1, 40] == 11.0 and E[1, 0] == 50.0 and E.shape == (2, 101)


def test_the_planted_track_yields_its_two_segments():
    """seed and sizes chosen here, on the reference: a half-depth and a 1.5x interval in Poisson depth are the only two segments of
    chrA, each boundary within one CNV bin; chrB (one copy) shows its uncovered run as CN 0, and the skipped contigs are named"""
    coverage, gcs, library, contigs, length, min_contig, W = C.planted_job()
    text, skipped, tracks = C.ref_job(coverage, gcs, library, contigs, length, min_contig, W)
    rows = [l.split("\t") for l in text.split("\n")[1:] if l]
    a = [r for r in rows if r[0] == "chrA"]
    assert len(a) == 2, a
    p = C.PLANTED
    for r, (lo, hi), kind, cn in zip(a, (p["del"], p["dup"]), ("DEL", "DUP"), ("1", "3")):
        assert r[3] == kind and r[4] == cn
        assert abs(int(r[1]) - lo * 50) <= W and abs(int(r[2]) - hi * 50) <= W
        assert abs(float(r[6]) - int(cn)) < 0.1
    assert skipped == ["absent", "tiny", "empty", "odd", "none"]
    b, c = [r for r in rows if r[0] == "chrB"], [r for r in rows if r[0] == "chrC"]
    assert [r[0] for r in rows] == ["chrA"] * 2 + ["chrB"] * len(b) + ["chrC"] * len(c) and len(b) == 1
    assert b[0][1:6] == ["20000", "24000", "DEL", "0", "8"]
    # the class fallback on both sides of MIN_CLASS: 101 and 100 bins take their own median, 99 the contig's — and read as a duplication
    Cm = C.ref_contig_median(coverage["chrC"], gcs["chrC"])
    E = C.ref_expected(coverage["chrC"], gcs["chrC"], Cm)
    assert E[60] > 1.9 * Cm and E[61] > 1.9 * Cm and E[62] == Cm
    assert len(c) == 1 and c[0][3:5] == ["DUP", "4"] and abs(int(c[0][1]) - 2100 * 50) <= W and abs(int(c[0][2]) - 2199 * 50) <= W
