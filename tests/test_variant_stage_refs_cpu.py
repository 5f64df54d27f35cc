"""Pins the plain references of tests/variant_stage_cases.py on the CPU, and shows that its inputs hold the edges they claim:
  * get_region_loop == get_region_numpy == the C oracle (oracle.get_region_counts, orc_get_region) on every query of the small
    families, numpy == the C oracle on the large ones;
  * adequacy: every one-comparison mutant of the loop (MUTANTS) gives other counts than the loop on at least one predicate-edge query,
    and every comparison of the chain meets operand differences -1, 0 and +1 on a live read;
  * the search, span, pack and means generators really produce the shapes test_gpu_variant_stages.py relies on;
  * pack_reference agrees with the independent statement of the bits in tests/test_gpu_variant.py."""
import warnings

import numpy as np
import pytest

import oracle
import variant_stage_cases as vc

EDGE = vc.edge_case()
SMALL = vc.counts_cases(large=False)


def _tables(case):
    return {t: vc.contig_table(case["cols"], t) for t in range(len(case["lengths"]))}


def _args(case, q):
    t, s, e, bp = (int(x) for x in q)
    return t, case["lengths"][t], s, e, bp, case["min_q"], case["max_ins"]


# ================================================================================================== the three statements agree
def test_case_counts():
    assert [c["name"] for c in SMALL] == ["predicate_edges", "search_small_increasing", "search_small_runs", "search_small_equal",
                                          "search_nq1", "search_nq3", "search_nq4", "search_nq5"]
    assert [len(c["queries"]) for c in SMALL[4:]] == list(vc.NQ_TAILS)
    assert all(len(c["queries"]) > 300 for c in SMALL[1:3]) and len(SMALL[3]["queries"]) > 100      # (one stored value per all-equal contig)
    assert len(vc.MUTANTS) == len(set(vc.MUTANTS)) == 28


@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_loop_numpy_and_c_oracle_agree(case):
    """the pure-Python loop runs where reads x queries stays small (contigs of up to 129 reads, and the whole edge family)"""
    tabs = _tables(case)
    looped = 0
    for q in case["queries"]:
        a = _args(case, q)
        tab = tabs[a[0]]
        want = vc.get_region_numpy(tab, *a)
        got_c = oracle.get_region_counts(tab, *a)
        assert np.array_equal(want, got_c), (case["name"], q, want, got_c)
        if case["family"] == "edges" or len(tab["start"]) <= 129:
            assert np.array_equal(vc.get_region_loop(tab, *a), want), (case["name"], q)
            looped += 1
    assert looped >= (len(case["queries"]) if case["family"] == "edges" else 1)
    if case["family"] == "edges":                                  # the multi-contig form of the arguments selects the contig itself
        a = _args(case, case["queries"][0])
        assert np.array_equal(vc.get_region_loop(case["cols"], *a), vc.get_region_numpy(case["cols"], *a))


def test_numpy_and_c_oracle_agree_on_the_large_cases():
    for case in vc.search_cases(large=True)[len(SMALL) - 1:] + [vc.span_case()]:
        assert case["large"]
        tabs = _tables(case)
        some = 0
        for q in case["queries"]:
            a = _args(case, q)
            want = vc.get_region_numpy(tabs[a[0]], *a)
            assert np.array_equal(want, oracle.get_region_counts(tabs[a[0]], *a)), (case["name"], q)
            some += int(want[1] > 0)
        assert some > len(case["queries"]) // 4, case["name"]


# ================================================================================================== adequacy of the edge family
def test_columns_are_legal():
    for case in SMALL:
        c = case["cols"]
        tid = c["tid"].astype(np.int64)
        placed = tid >= 0
        assert (np.diff(np.where(placed, tid, 1 << 40)) >= 0).all()
        L = np.array(case["lengths"] + [0])[tid]
        assert ((c["pos"][placed] >= 0) & (c["pos"][placed] < L[placed]) & (c["end"][placed] >= c["pos"][placed]) & (c["end"][placed] <= L[placed])).all()
        assert (c["mate_pos"] >= -1).all()
        for t in range(len(case["lengths"])):
            assert (np.diff(c["pos"][tid == t].astype(np.int64)) >= 0).all()
        assert min(case["lengths"]) >= 10


@pytest.mark.parametrize("mutant", vc.MUTANTS)
def test_every_mutant_is_told_apart(mutant):
    """A mutant that no predicate-edge query separates from the loop fails here: the cases are extended, the mutant stays."""
    tabs = _tables(EDGE)
    for q in EDGE["queries"]:
        a = _args(EDGE, q)
        if not np.array_equal(vc.get_region_loop(tabs[a[0]], *a), vc.get_region_loop(tabs[a[0]], *a, mutant=mutant)):
            return
    pytest.fail("no predicate-edge query tells mutant %r from get_region_loop" % mutant)


def test_every_comparison_meets_minus_one_zero_and_plus_one():
    trace = {}
    tabs = _tables(EDGE)
    for q in EDGE["queries"]:
        a = _args(EDGE, q)
        vc.get_region_loop(tabs[a[0]], *a, trace=trace)
    assert set(trace) == set(vc.COMPARISONS)
    for name in vc.COMPARISONS:
        assert {-1, 0, 1} <= trace[name], (name, sorted(trace[name]))


def test_edge_family_holds_the_listed_values():
    c, q = EDGE["cols"], EDGE["queries"]
    placed = c["tid"] >= 0
    assert placed.all() and len(c["tid"]) > 5000
    assert set(vc.MAPQ_VALUES) <= set(c["mapq"].tolist()) and set(vc.TLEN_VALUES) <= set(c["tlen"].tolist())
    for t in (0, 1, 2, 4):
        m = c["tid"] == t
        assert {t, vc.EDGE_OTHER, -1} <= set(c["mate_tid"][m].tolist()) and {-1, 0} <= set(c["mate_pos"][m].tolist())
        combos = {(int(f) & 0x40c, bool(s >= 0)) for f, s in zip(c["flag"][m], c["sa_off"][m])}
        assert combos == {(b, s) for b in vc.FLAG_BITS for s in (False, True)}
    assert not (c["tid"] == vc.EDGE_OTHER).any()
    L = np.array(EDGE["lengths"])[q[:, 0]]
    assert (q[:, 1] == q[:, 2]).sum() >= 10                                                 # start == end
    assert set(vc.BP_NEAR_ORIGIN) <= set(q[q[:, 0] == 1, 3].tolist())
    assert ((q[:, 3] < q[:, 1]).sum() >= 5) and ((q[:, 3] > q[:, 2]).sum() >= 5)            # bp outside [start, end]
    assert {-1, 0, 1} <= set((q[:, 2] + vc.MAX_INS - L).tolist())                           # end + max_ins at the contig length
    assert {0, 1, 5} <= set((q[:, 1] - L).tolist())                                         # start >= contig length: the fallback
    top = q[q[:, 0] == 4]
    assert EDGE["lengths"][4] == vc.I32_MAX and (top[:, 2] + vc.MAX_INS > vc.I32_MAX).sum() >= 5
    assert c["pos"][c["tid"] == 4].min() > vc.I32_MAX - 10_000


# ================================================================================================== search, span
def test_search_model_is_a_lower_bound():
    rng = np.random.default_rng(5)
    for n in (0, 1, 64, 65, 4097, 4160, 4225, 300_000):
        a = np.sort(rng.integers(0, max(1, n // 3), n))
        for v in [-1, 0, 1, n // 6, n] + a[:: max(1, n // 7)].tolist():
            assert vc.search_probes(a, v)[1] == np.searchsorted(a, v, side="left")
    assert [len(vc.search_probes(np.arange(n), 1)[0]) for n in (64, 65, 4223, 4224, 262144, 270_399, 270_400)] == [0, 1, 1, 2, 2, 2, 3]


def test_search_shapes_hold_what_they_claim():
    assert set(vc.SEARCH_SMALL) | set(vc.SEARCH_LARGE) == set(vc.SEARCH_N) and len(vc.SEARCH_LARGE) == 4
    for n in vc.SEARCH_N:
        inc, runs, eq = (vc.search_starts(n, p) for p in vc.SEARCH_PATTERNS)
        assert len(inc) == len(runs) == len(eq) == n
        assert (np.diff(inc) > 0).all() and (np.diff(runs) >= 0).all() and (np.diff(eq) == 0).all()
        spec = vc.search_runs(n)
        assert len(spec) == (0 if n < 127 else 1 if n < 4224 else 2)
        for rnd, (lo, r) in enumerate(spec):
            assert 65 <= r <= 5000 and lo >= 0 and lo + r <= n
            v = runs[lo]
            assert (runs[lo:lo + r] == v).all() and (runs == v).sum() == r
            probes = vc.search_probes(runs, v)[0]
            assert len(probes) > rnd
            inside = [p for p in probes[rnd] if lo < p < lo + r - 1]              # a probed index with the run on both sides of it
            assert inside, (n, rnd, lo, r)
        # the aimed keys: stored starts and both neighbours, one below the first and one above the last start
        if n:
            vals = set(vc.search_query_values(inc))
            assert {int(inc[0]) - 5, int(inc[0]), int(inc[-1]), int(inc[-1]) + 1, int(inc[-1]) + 5} <= vals
            c1 = n >> 6
            if c1:
                assert {int(inc[32 * c1 - 1]) + d for d in (-1, 0, 1)} <= vals
    case = SMALL[2]                                                  # both keys of a query pair are the aimed value
    a = vc.search_starts(*case["shape"][7])
    for t, s, e, bp in vc.search_queries(7, a)[:8:2]:
        assert e + vc.MAX_INS in vc.search_query_values(a) and e + vc.MAX_INS < vc.SEARCH_LENGTH
    for t, s, e, bp in vc.search_queries(7, a)[1:8:2]:
        assert s - vc.SEARCH_SPAN in vc.search_query_values(a)
    for case in SMALL[1:4]:                                          # ... and the maximum span of every contig with reads is SEARCH_SPAN
        for t, (n, p) in enumerate(case["shape"]):
            tab = vc.contig_table(case["cols"], t)
            assert len(tab["start"]) == n and np.array_equal(tab["start"], vc.search_starts(n, p))
            if n:
                assert (tab["end"].astype(np.int64) - tab["start"]).max() == vc.SEARCH_SPAN


def test_span_case_reaches_back():
    case = vc.span_case()
    tab = vc.contig_table(case["cols"], 1)
    x, i = case["at"], case["far_index"]
    q0, q1 = case["queries"][0], case["queries"][1]
    assert len(tab["start"]) == vc.SPAN_N and tab["start"][vc.SPAN_AT] == x and vc.SPAN_AT - i > 300_000
    assert tab["end"][i] == q0[1] + 1 == q1[1] and tab["end"][i + 2] == q0[1]            # passes q_start by 1 / misses by 0
    span = (tab["end"].astype(np.int64) - tab["start"])
    assert span.argmax() == i and np.sort(span)[-3] <= 60
    a0, a1 = _args(case, q0), _args(case, q1)
    without = {k: np.delete(v, i) for k, v in tab.items()}
    assert vc.get_region_numpy(tab, *a0)[1] == vc.get_region_numpy(without, *a0)[1] + 1      # the far read is counted there ...
    assert np.array_equal(vc.get_region_numpy(tab, *a1), vc.get_region_numpy(without, *a1))  # ... and not one base further
    assert np.array_equal(vc.get_region_numpy(tab, *a0), vc.get_region_numpy({k: np.delete(v, i + 2) for k, v in tab.items()}, *a0))


# ================================================================================================== pack
def test_pack_reference_equals_the_bits_of_test_gpu_variant():
    from test_gpu_variant import _bits
    from tiddit_amd import tiddit_region as R
    assert vc.EV_RECORD == R.EV_RECORD
    assert (vc.EV_UNMAPPED, vc.EV_MATE_UNMAPPED, vc.EV_DUPLICATE, vc.EV_HAS_SA, vc.EV_LOW_Q, vc.EV_DISCORDANT) == \
        (R.EV_UNMAPPED, R.EV_MATE_UNMAPPED, R.EV_DUPLICATE, R.EV_HAS_SA, R.EV_LOW_Q, R.EV_DISCORDANT)
    assert vc.COLS == R._EV_COLUMNS and tuple(vc._DT[k] for k in vc.COLS) == R._EV_TYPES
    rng = np.random.default_rng(77)
    cols = vc._pack_contigs(rng, np.sort(rng.integers(0, 4, 5000)).tolist() + [-1] * 7, 4)
    cols["tlen"][:9] = vc.TLEN_VALUES
    cols["mapq"][9:14] = vc.MAPQ_VALUES
    rec, spans = vc.pack_reference(cols, vc.MIN_Q, vc.MAX_INS, 4)
    assert len(rec) == 5000 and not rec["pad"].any()
    o = 0
    for t in range(4):
        tab = vc.contig_table(cols, t)
        n = len(tab["start"])
        assert np.array_equal(rec["bits"][o:o + n], _bits(tab, vc.MIN_Q, vc.MAX_INS, t))
        assert np.array_equal(rec["start"][o:o + n], tab["start"]) and np.array_equal(rec["end"][o:o + n], tab["end"])
        assert np.array_equal(rec["mate_pos"][o:o + n], tab["mate_pos"])
        assert spans[t] == (tab["end"].astype(np.int64) - tab["start"]).max()
        o += n
    assert rec["bits"][0] & vc.EV_DISCORDANT == 0 and rec["bits"][2] & vc.EV_DISCORDANT     # |tlen| == max_ins is not discordant ...
    assert {int(b) & vc.EV_DISCORDANT for b in rec["bits"][7:9]} == {vc.EV_DISCORDANT}      # ... INT32_MIN and INT32_MAX are


def test_pack_cases_hold_what_they_claim():
    cases = {c["name"]: c for c in vc.pack_cases(large=True)}
    assert [len(cases["n%d" % n]["batches"][0]["tid"]) for n in vc.PACK_SIZES] == list(vc.PACK_SIZES)
    for n in vc.PACK_SIZES:
        tl = cases["n%d" % n]["batches"][0]["tlen"]
        assert tl[-1] == vc.I32_MAX and (n == 1 or tl[0] == vc.I32_MIN)
        b = cases["n%d" % n]["batches"][0]
        assert b["mate_tid"][0] == b["tid"][0] and b["mate_tid"][-1] == b["tid"][-1]          # discordant by |tlen| alone
        rec = vc.pack_reference(b, vc.MIN_Q, vc.MAX_INS, 3)[0]
        assert rec["bits"][0] & vc.EV_DISCORDANT and rec["bits"][-1] & vc.EV_DISCORDANT

    def wave_contigs(c, w):
        return c["batches"][0]["tid"][64 * w:64 * w + 64]
    c = cases["wave_of_2_contigs"]
    assert len(set(wave_contigs(c, 1).tolist())) == 2
    c5 = cases["wave_of_5_contigs"]
    assert len(set(wave_contigs(c5, 0).tolist())) == 5 and 2 not in set(c5["batches"][0]["tid"].tolist())
    for c in (c, c5):                                              # the widest read of a contig: not lane 0, not the wave's first contig
        b = c["batches"][0]
        span = b["end"].astype(np.int64) - b["pos"]
        w = c["wave"]
        hit = [i for i in c["wide"] if 64 * w <= i < 64 * w + 64 and i % 64 and b["tid"][i] != b["tid"][64 * w]]
        assert hit
        for i in c["wide"]:
            assert span[i] == span[b["tid"] == b["tid"][i]].max() and (span[b["tid"] == b["tid"][i]] == span[i]).sum() == 1
    c = cases["three_appends"]
    tids = [b["tid"] for b in c["batches"]]
    assert all((t == 1).any() for t in tids) and (tids[0] == 0).any() and (tids[2] == 3).any() and (tids[2][-5:] == -1).all()
    assert not any((t == 2).any() for t in tids)
    allc = vc.concat_cols(c["batches"])
    span = allc["end"].astype(np.int64) - allc["pos"]
    i = c["wide"][0]
    assert len(tids[0]) <= i < len(tids[0]) + len(tids[1]) and span[i] == span[allc["tid"] == 1].max() > 10_000
    # the two stores that grow: both rules of the reserve run, with records already in the store
    g0, g1 = cases["grow_from_0"], cases["grow_from_1000"]
    assert vc.expected_capacities(0, g0["sizes"]) == ([1 << 20, 1 << 20, 3 << 19], ["floor", None, "x1.5"])
    caps, why = vc.expected_capacities(1000, g1["sizes"])
    assert why == [None, "floor", None, "x1.5", "exact"] and caps[-1] == sum(g1["sizes"]) > caps[-2] == 3 << 19
    for g in (g0, g1):
        assert [len(b["tid"]) for b in g["batches"]] == list(g["sizes"]) and sum(g["sizes"]) > 1 << 20
        assert all((np.diff(b["tid"]) >= 0).all() for b in g["batches"])


# ================================================================================================== means
@pytest.mark.parametrize("family", vc.VALUE_FAMILIES)
def test_means_cases_hold_what_they_claim(family):
    cov, gc, segs, masked, kept = vc.means_case(family)
    seen = {}
    for (name, s, e), m, k in zip(segs, masked, kept):
        kind, kk, off = name.rsplit("_", 2)
        assert s == int(off) and k == int(kk) and e == len(cov[name]) == len(gc[name])
        g = gc[name][s:e]
        assert ((g > -1).sum() if m else len(g)) == k
        if kind in ("lane0", "lane63") and k:
            assert set((np.flatnonzero(g > -1) % 64).tolist()) == {0 if kind == "lane0" else 63}
        seen.setdefault((kind, m), set()).add((k, s))
    for kind in vc.MASK_KINDS:
        offs = (0, 5) if kind in ("lane0", "lane63") else vc.MEAN_OFFSETS
        ks = (0,) if kind == "none" else vc.KEPT_COUNTS
        assert seen[(kind, 1)] == {(k, o) for k in ks for o in offs}, kind
    assert seen[("all", 0)] == {(k, o) for k in vc.KEPT_COUNTS for o in vc.MEAN_OFFSETS}
    a = cov["all_8193_1"][1:]
    if family == "cancel":                                          # another order of the same terms gives another sum, by far
        assert abs(np.average(a) - np.average(a[::-1])) > 1e-6 * abs(np.average(a)) or np.average(a) != np.average(np.sort(a))
        assert np.average(a) != np.sum(np.sort(a)) / len(a)
    if family == "special":
        vals = np.concatenate([v for v in cov.values()])
        assert not np.isfinite(vals[vals != 0]).any() and np.signbit(vals[vals == 0]).all() and np.isnan(vals).any()
    with warnings.catch_warnings():                                 # the restated pairwise mean of the oracle on these values too
        warnings.simplefilter("ignore")
        for (name, s, e), m in list(zip(segs, masked))[::7]:
            x, g = cov[name][s:e], gc[name][s:e]
            want = np.average(x[g > -1] if m else x) if ((g > -1).sum() if m else len(x)) else np.nan
            got = oracle.np_masked_mean(x, g)[0] if m else oracle.np_mean(x)
            assert got == want or (np.isnan(got) and np.isnan(want)), (family, name, m)
