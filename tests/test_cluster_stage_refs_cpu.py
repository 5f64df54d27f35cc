"""CPU pin of tests/cluster_stage_cases.py (no GPU): the three references of the clustering cases agree — the literal state machine
in C, its closed form, and the labels the real DBSCAN.py gave (tests/golden/dbscan_edges.npz) — every case sits on the edge it
claims, and a plain Python restatement of both passes with named one-line mutants shows that the cases would notice: the unmutated
restatement equals the literal oracle on every small case, every mutant differs from it inside every family listed for it."""
import os

import numpy as np
import pytest

import cluster_stage_cases as cc


# ================================================================================================== the constants
def test_constants_are_parsed_from_the_sources():
    c = cc.parse_constants()
    assert set(c) == {"DT_NW", "DT_T", "DT_S", "DT_GRP", "DB_SMALL", "DBF_M_MAX", "DBF_TILE", "DBM_INLINE_PREFIX_MAX"}
    assert all(isinstance(v, int) and v > 0 for v in c.values())
    assert c["DT_S"] == c["DT_NW"] * 64 and c["DT_T"] == c["DT_S"] - 128
    # what the case builders rely on: a cluster of DB_SMALL members fits the halo, word starts and seam offsets do not collide
    assert c["DB_SMALL"] <= 128 and c["DT_T"] > 15 * 64 + c["DB_SMALL"] + 66 and c["DBF_M_MAX"] < cc.EPS
    assert c["DBF_TILE"] % 64 == 0 and c["DT_GRP"] >= 2


def test_constant_parser_fails_when_a_define_goes():
    src = {fn: open(os.path.join(cc._CSRC, fn)).read() for fn in set(cc._CONST_FILES.values())}
    assert cc.parse_constants(src) == cc.CONSTANTS
    for name, fn in cc._CONST_FILES.items():
        broken = dict(src)
        broken[fn] = src[fn].replace("#define %s " % name, "#define X%s " % name)
        assert broken[fn] != src[fn], name
        with pytest.raises(KeyError):
            cc.parse_constants(broken)
    retuned = dict(src)
    retuned["tdt_dbscan_tile.h"] = src["tdt_dbscan_tile.h"].replace("#define DT_NW 24", "#define DT_NW 16")
    got = cc.parse_constants(retuned)
    assert (got["DT_NW"], got["DT_S"], got["DT_T"]) == (16, 1024, 896)


# ================================================================================================== the registry
def test_registry_counts():
    names = cc.case_names()
    assert len(names) == len(set(names)) == cc.N_CASES
    assert sum(len(cc.get(n)["entries"]) for n in names) == cc.N_PAIRS
    for n in names:
        c = cc.get(n)
        assert c["family"] == cc.family_of(n) and c["entries"], n
        assert ("sort" in c["entries"]) <= c["sorted_x"], n                    # unsorted x: no sorting entries
        assert ("host" in c["entries"]) <= (c["nb"] == 1), n
    large = [n for n in names if cc.get(n)["n"] > cc.LITERAL_MAX]
    assert large == [cc.B_LARGE] and cc.get(cc.B_LARGE)["n"] > cc.DBM_INLINE_PREFIX_MAX * cc.DBF_TILE
    assert set(cc.MUTANT_FAMILIES) | set(cc.EQUIVALENT_MUTANTS) == set(MUTANTS)


def test_family_a_is_the_whole_cross():
    names = set(cc.case_names("A"))
    for m in (2, 3, 4, 5, 63, 64):
        ks = cc.a_member_counts(m)
        assert {m, m + 1, 127, 128} <= set(ks) and (m > 63 or {63, 64, 65} <= set(ks))
        for k in ks:
            for o in (-65, -64, -2, -1, 0, 1):
                for tw in ("", "_nb3"):
                    assert "a_seam_m%d_k%d_o%+d%s" % (m, k, o, tw) in names
    c = cc.get("a_seam_m3_k128_o-1")
    want = {s % cc.DT_T for s in c["claim"]["starts"]}
    assert {cc.DT_T - 1} <= want and {s % 64 for s in cc.A_WORD_STARTS} == {0, 1, 62, 63}
    assert cc.DT_T - 1 in c["claim"]["starts"] and 2 * cc.DT_T - 1 in c["claim"]["starts"]
    assert cc.DT_T - 1 + 128 == cc.DT_S - 1                      # 128 members from DT_T - 1: the cluster ends on the last staged position
    assert {cc.get("a_n%d_m3" % n)["n"] for n in cc.A_NS} == {cc.DT_T - 1, cc.DT_T, cc.DT_T + 1, cc.DT_S, cc.DT_S + 1, cc.DT_GRP * cc.DT_T - 1,
                                                             cc.DT_GRP * cc.DT_T, cc.DT_GRP * cc.DT_T + 1}


# ================================================================================================== references agree, claims hold
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_literal_equals_closed_form_and_claims_hold(family):
    """every case up to LITERAL_MAX points: literal == closed form (labels and last ids, and the x pass alone), and the properties
    computed from the literal labels are the claimed ones"""
    seen_routes = set()
    for name in cc.case_names(family):
        c = cc.get(name)
        if c["n"] > cc.LITERAL_MAX:
            continue
        lit, closed = cc.reference(c, literal=True), cc.reference(c, literal=False)
        assert np.array_equal(lit[0], closed[0]) and np.array_equal(lit[1], closed[1]), name
        assert lit[0].dtype == np.float64 and lit[1].dtype == np.int64
        prop, claim = cc.properties(c), c["claim"]
        for k in ("largest", "route"):
            assert claim[k] is None or claim[k] == prop[k], (name, k, claim[k], prop[k])
        assert set(claim["starts"]) <= prop["starts"], (name, sorted(set(claim["starts"]) - prop["starts"]))
        assert claim["tiles"] == prop["tiles"] and claim["groups"] == prop["groups"], name
        xl, xid = cc.reference(c, literal=True, mode=1)
        for b in range(c["nb"]):                                    # -1 for empty buckets and for buckets without a cluster
            seg, xseg = lit[0][c["off"][b]:c["off"][b + 1]], xl[c["off"][b]:c["off"][b + 1]]
            assert (lit[1][b] == -1) == (xid[b] == -1) == (not (xseg >= 0).any()), (name, b)
            assert lit[1][b] >= (seg.max() if len(seg) else -1) and lit[1][b] >= xid[b], (name, b)
        seen_routes.add(prop["route"])
    assert seen_routes >= {"A": {1}, "B": {1, 2, 3}, "C": {1, 2, 3}, "D": {1, 2}}[family]


def test_the_large_case_is_reached_on_purpose():
    """the one case above LITERAL_MAX uses the closed form alone; its generator is pinned to the literal reference on the smaller
    members of the same family (above), and it does hold the 129-member cluster that sends the call to route 2"""
    c = cc.get(cc.B_LARGE)
    xl, _ = cc.reference(c, literal=False, mode=1)
    at = c["claim"]["starts"][0]
    assert xl[at] >= 0 and xl[at - 1] != xl[at]
    assert int(np.bincount(xl[xl >= 0].astype(np.int64)).max()) == cc.DB_SMALL + 1 == c["claim"]["largest"]
    assert -(-c["n"] // cc.DBF_TILE) > cc.DBM_INLINE_PREFIX_MAX
    small = cc.get("b_tiles3")
    assert small["claim"]["largest"] == c["claim"]["largest"] and -(-small["n"] // cc.DBF_TILE) <= cc.DBM_INLINE_PREFIX_MAX


def test_family_specific_aims():
    # B: the 128 | 129 twins differ by one point, and everything outside the big cluster keeps its labels up to one renumbering
    for where in ("start", "end", "seam"):
        a, b = cc.get("b_switch_%s_%d" % (where, cc.DB_SMALL)), cc.get("b_switch_%s_%d" % (where, cc.DB_SMALL + 1))
        assert b["n"] == a["n"] + 1 and cc.properties(a)["route"] == 1 and cc.properties(b)["route"] == 2
        la, lb = cc.reference(a)[0], cc.reference(b)[0]
        at = a["claim"]["starts"][0]
        ia = np.concatenate([np.arange(at), np.arange(at + cc.DB_SMALL + (where != "end"), a["n"])])
        ib = np.where(ia < at, ia, ia + 1)
        assert same_up_to_renumbering(la[ia], lb[ib]), where
    # B: m = 64 and m = 65 on the same points (routes 2 and 3): the x-clusters of at least 65 members are the same index ranges
    for big in cc.B_BIGS:
        a, b = cc.get("b_mixed_%d_m%d" % (big, cc.DBF_M_MAX)), cc.get("b_mixed_%d_m%d" % (big, cc.DBF_M_MAX + 1))
        assert cc.properties(a)["route"] == 2 and cc.properties(b)["route"] == 3
        xa, xb = cc.reference(a, mode=1)[0], cc.reference(b, mode=1)[0]
        at = a["claim"]["starts"][0]
        for xl in (xa, xb):
            assert (xl[at:at + big] == xl[at]).all() and xl[at] >= 0 and xl[at + big] != xl[at] and xl[at - 1] != xl[at]
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"])          # the same points on routes 2 and 3
        assert (xa != xb).any()                                                            # (the 64-member stretches: clusters at m = 64 only)
    # C: the windows stop at the bucket's end, ids restart, and the packed case holds many boundaries per 64 positions
    for m in (2, 3, 5):
        c = cc.get("c_many_m%d_mode0" % m)
        assert c["nb"] >= 300 and c["n"] <= cc.DT_T and set(np.diff(c["off"]).tolist()) >= {0, 1, 2, m - 1, m, m + 1, m + 2}
        assert max(np.histogram(c["off"], bins=np.arange(0, c["n"] + 64, 64))[0]) >= 8
    c = cc.get("c_empty_mode0")
    size = np.diff(c["off"])
    assert size[0] == 0 and size[-1] == 0 and (size[4:8] == [1, 0, 0, 0]).all() and cc.DT_T - 1 in c["off"] and 2 * cc.DT_T in c["off"]
    for pos in cc.C_CUT_POSITIONS:
        c = cc.get("c_cut_p%d_m3_mode0" % pos)
        assert c["off"][1] == pos and (np.diff(c["x"][pos - 20:pos + 20]) == 1).all()    # one stretch, cut
    # D: the window distances sit on eps - 1, eps and eps + 1 in both passes
    for name, E in (("d_dist_r1_m2", 60), ("d_dist_r1_m3", 60), ("d_dist_r2_m3", 60), ("d_dist_f395_m2", 40), ("d_dist_f400_m3", 40)):
        dx, dy = cc.window_distances(cc.get(name))
        assert {E - 1, E, E + 1} <= dx and {E - 1, E, E + 1} <= dy, name
    assert cc.properties(cc.get("d_dist_r2_m3"))["route"] == 2 and cc.properties(cc.get("d_dist_r1_m3"))["route"] == 1
    for n in (100, 300):
        c = cc.get("d_wide_n%d_eps%d" % (n, (1 << 32) - 1))
        assert c["x"].min() == 0 == c["y"].min() and c["x"].max() == (1 << 32) - 2 == c["y"].max()
        assert (cc.reference(c, mode=1)[0] == 0).all()
    assert cc.reference(cc.get("d_wide_below"), mode=1)[0].tolist() == [-1.0, 0.0, 0.0]
    # D: 0, 1, 2 and many sub-runs, so that later clusters' ids are shifted by earlier extras
    for m in (2, 3, 5):
        c = cc.get("d_subruns_m%d" % m)
        xl, xid = cc.reference(c, mode=1)
        lab, last = cc.reference(c)
        per = [len(set(lab[xl == k].tolist()) - {-1.0}) for k in range(int(xid[0]) + 1)]
        assert {0, 1, 2} <= set(per) and max(per) >= 4 and last[0] > xid[0]
        for kind in ("equal", "two", "desc"):
            c = cc.get("d_ties_%s_m%d" % (kind, m))
            assert (cc.reference(c)[0] >= 0).any()


def same_up_to_renumbering(a, b):
    if not np.array_equal(a < 0, b < 0):
        return False
    fwd, back = {}, {}
    for u, v in zip(a[a >= 0].tolist(), b[b >= 0].tolist()):
        if fwd.setdefault(u, v) != v or back.setdefault(v, u) != u:
            return False
    return True


# ================================================================================================== the real DBSCAN.py
def test_golden_labels_of_the_real_dbscan(golden_dir):
    z = np.load(os.path.join(golden_dir, "dbscan_edges.npz"))
    names = z["names"].tolist()
    assert names == [n for n in cc.case_names() if cc.in_golden(cc.get(n))] and len(names) > 150
    assert all(any(cc.in_golden(cc.get(n)) for n in cc.case_names(f)) for f in cc.FAMILIES)
    for m in cc.A_MS:
        for k in cc.a_member_counts(m):
            assert "a_seam_m%d_k%d_o-1" % (m, k) in names
    size = os.path.getsize(os.path.join(golden_dir, "dbscan_edges.npz"))
    assert size < max(os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir) if f != "dbscan_edges.npz")
    hashes, xids, at = z["hashes"].tolist(), z["xid"], 0
    for k, name in enumerate(names):
        c = cc.get(name)
        assert hashes[k] == cc.input_hash(c), name                          # the case module still generates the fixture's inputs
        assert z["c%d_x" % k].dtype == np.int32
        xl, xid = cc.reference(c, literal=True, mode=1)
        assert np.array_equal(xl, z["c%d_x" % k].astype(np.float64)) and np.array_equal(xid, xids[at:at + c["nb"]]), name
        at += c["nb"]
        if c["mode"] == 0:
            assert np.array_equal(cc.reference(c, literal=True)[0], z["c%d_main" % k].astype(np.float64)), name
    assert at == len(xids)


# ================================================================================================== restatement and mutants
MUTANTS = tuple(cc.MUTANT_FAMILIES) + cc.EQUIVALENT_MUTANTS


def restate(case, mut=None):
    """DBSCAN.py:33-129 bucket by bucket in plain Python, with exactly one line changed when `mut` names a mutant"""
    x, y, off, eps, m, mode = case["x"].tolist(), case["y"].tolist(), case["off"].tolist(), case["eps"], case["m"], case["mode"]
    n = len(x)
    lab, last = [-1.0] * n, [-1] * (len(off) - 1)
    lt = (lambda d: d <= eps) if mut == "x_le_eps" else (lambda d: d < eps)
    lty = (lambda d: d <= eps) if mut == "y_le_eps" else (lambda d: d < eps)
    wx = m + {"x_window_m_minus_1": -1, "x_window_m_plus_1": 1}.get(mut, 0)
    wy = m - 1 + {"y_window_m_minus_2": -1, "y_window_m": 1}.get(mut, 0)
    sx = m + {"x_stretch_longer": 1, "x_stretch_shorter": -1}.get(mut, 0)
    sy = m + {"y_stretch_longer": 1, "y_stretch_shorter": -1}.get(mut, 0)
    carry = -1
    for b in range(len(off) - 1):
        lo, hi = off[b], off[b + 1]
        k = hi - lo
        if not k:
            continue
        reach = n if mut == "bucket_boundaries_ignored" else hi
        cid = carry if mut == "ids_not_restarted" else -1
        active = False
        for i in range(lo, lo + k - m + 1 + {"x_last_window_minus_1": -1, "x_last_window_plus_1": 1}.get(mut, 0)):      # :40
            pts = x[i + 1:min(i + wx + 1, reach)]                                                                       # :44
            if pts and lt(max(abs(p - x[i]) for p in pts)):                                                             # :51
                if active:
                    if i + m - 1 < hi:
                        lab[i + m - 1] = float(cid)                                                                     # :54
                else:
                    cid += 1
                    active = True
                    for j in range(i, min(i + sx, hi)):                                                                 # :59
                        lab[j] = float(cid)
            else:
                active = False
        if mode == 0:
            for c in sorted(set(lab[lo:hi]) - {-1.0}):                                                                  # :68-70
                idx = [i for i in range(lo, hi) if lab[i] == c]                                                         # :72
                yc = sorted(((y[i], i) for i in idx), key=(lambda t: (t[0], -t[1])) if mut == "y_ties_reversed" else (lambda t: t[0]))   # :81
                sub = [-1] * len(yc)
                active, sid = False, 0
                for i in range(0, len(yc) - m + 1 + (-1 if mut == "y_last_window_minus_1" else 0)):                      # :90
                    nxt = yc[i + 1:i + 1 + wy]                                                                          # :93
                    if not nxt or lty(max(abs(p[0] - yc[i][0]) for p in nxt)):                                          # :100
                        if active:
                            if i + m - 1 < len(sub):
                                sub[i + m - 1] = sid
                        else:
                            sid += 1
                            active = True
                            for j in range(i, min(i + sy, len(sub))):                                                   # :107
                                sub[j] = sid
                    else:
                        active = False
                for i, s in enumerate(sub):                                                                             # :112-119
                    if s == 1 and mut != "subrun1_renumbered":
                        lab[yc[i][1]] = c
                    elif s > -1:
                        lab[yc[i][1]] = float(s + cid - 1)
                    else:
                        lab[yc[i][1]] = -1.0
                if sid > 1 and mut != "extra_offset_dropped":                                                           # :121
                    cid += sid - 1
        last[b] = cid
        carry = cid
    return np.array(lab, dtype=np.float64), np.array(last, dtype=np.int64)


def _small(family):
    return [n for n in cc.case_names(family) if cc.in_golden(cc.get(n)) and cc.get(n)["m"] <= 5]


def _differs(case, mut):
    want = cc.reference(case, literal=True)
    got = restate(case, mut)
    return not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_restatement_equals_the_literal_oracle(family):
    """on every small case — the ones the real DBSCAN.py was run on (all m: the m = 63 / 64 layouts too)"""
    names = [n for n in cc.case_names(family) if cc.in_golden(cc.get(n))]
    assert len(names) >= 20
    for name in names:
        assert not _differs(cc.get(name), None), name


@pytest.mark.parametrize("mut", sorted(cc.MUTANT_FAMILIES))
def test_every_mutant_is_caught_in_every_listed_family(mut):
    for family in cc.MUTANT_FAMILIES[mut]:
        assert any(_differs(cc.get(n), mut) for n in _small(family)), (mut, family)


def test_tie_order_cannot_change_the_labels():
    """the one mutant of the issue's list that no case can catch (see EQUIVALENT_MUTANTS in the case module): held to be equivalent
    on every small case of family D and on the tie-heavy layouts of A, and on an exhaustive sweep of tiny clusters"""
    for name in _small("D") + [n for n in _small("A") if "_o-1" in n and "_nb3" not in n]:
        assert not _differs(cc.get(name), "y_ties_reversed"), name
    import itertools
    for m in (2, 3):
        for ys in itertools.product(range(4), repeat=6):
            c = cc._case("t", "D", np.arange(6), np.array(ys) * 2, 3, m)
            assert np.array_equal(restate(c, "y_ties_reversed")[0], restate(c)[0]), (m, ys)
