"""The realignment of clip-site consensus without a GPU: the definition of tiddit_amd/tiddit_clip_align.py (a Python loop per site), an
independent numpy restatement (sliding comparisons over arrays of codes, the mates by sorting) and the literal claims of
tests/clip_align_cases.py agree on every case; each one-line departure of the restatement is noticed inside the family that is listed
for it; the switch's four forms and its refusals; the file's bytes on a literal example."""
import numpy as np
import pytest

import clip_align_cases as C
from tiddit_amd import tiddit_clip_align as A

PAD = 64
_LUT = np.full(16, 4, dtype=np.int8)          # a 4-bit reference code -> 0 ... 3, or 4 for what is no base
_LUT[[1, 2, 4, 8]] = [0, 1, 2, 3]


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def restate_sites(c, bug=None):
    """every site's (status, PARTNER, strand, mm, HITS) by sliding comparisons; ``bug``: one departure from the definition"""
    ref = C.host_reference(c)
    W, K, M = c["W"], c["K"], c["M"]
    padded = {t: np.concatenate([np.full(PAD, 4, np.int8), _LUT[codes], np.full(PAD, 4, np.int8)]) for t, codes in ref.contigs.items()}
    out = []
    for x in c["sites"]:
        tid, P, side, cl = x["tid"], x["P"], x["side"], x["clen"]
        if cl < K:
            out.append((C.SHORT, 0, 0, C.NO_MM, 0))
            continue
        if tid not in padded or not 1 <= P <= len(padded[tid]) - 2 * PAD:
            out.append((C.OFF, 0, 0, C.NO_MM, 0))
            continue
        g, ln = padded[tid], len(padded[tid]) - 2 * PAD
        cols = np.array([(x["cons"] >> (2 * j)) & 3 for j in range(cl)], dtype=np.int8)
        Q = np.arange(max(1, P - W), min(ln, P + W) + 1, dtype=np.int64)
        keys, hits = [], 0
        for strand in (0, 1):
            ascending = (side == C.R_SIDE) == (strand == 0)
            if bug == "swap_L" and side == C.L_SIDE:
                ascending = not ascending
            step = 1 if ascending else -1
            want = 3 - cols if strand and bug != "no_comp" else cols
            last = Q + step * (cl - 1)
            ok = (last >= 1) & (last <= ln) if bug != "guard" else np.ones(len(Q), dtype=bool)
            mm = np.zeros(len(Q), dtype=np.int64)
            for j in range(cl):
                mm += g[Q + step * j + PAD - 1] != want[j]
            mm, q = mm[ok], Q[ok]
            hits += int(((mm < M) if bug == "lt" else (mm <= M)).sum())
            dist = np.abs(q - P)
            keys.append(np.stack([mm, dist, np.full(len(q), strand), q], axis=1))
        keys = np.concatenate(keys)
        if not len(keys):
            out.append((C.SEARCHED, 0, 0, C.NO_MM, 0))
            continue
        order = (keys[:, 3], keys[:, 2], keys[:, 1], keys[:, 0]) if bug != "tie" else (keys[:, 2], keys[:, 3], keys[:, 1], keys[:, 0])
        mm, _, strand, q = keys[np.lexsort(order)[0]].tolist()
        out.append((C.SEARCHED, q, strand, mm, hits))
    return out


def restate_rows(c, placed, bug=None):
    """the counters and rows of summarise, restated over arrays"""
    M = c["M"]
    sn = dict.fromkeys(A.SN, 0)
    rows = []
    for x, (status, Q, strand, mm, hits) in zip(c["sites"], placed):
        sn["sites"] += 1
        sn[("short_consensus", "off_reference", "searched")[status]] += 1
        if status != C.SEARCHED:
            continue
        P, side = x["P"], x["side"]
        typ = ln = None
        if mm != C.NO_MM and mm <= M:
            d = Q - P if side == C.R_SIDE else P - Q          # the partner's offset away from the aligned part
            if strand:
                typ, ln = "INV", abs(d) + (bug == "len_inv")
            elif d == 1:
                typ, ln = "REF", 0
            elif d > 1:
                typ, ln = "DEL", d - 1 + (bug == "len_del")
            else:
                typ, ln = "DUP", 1 - d + (bug == "len_dup")
            sn["aligned"] += 1
            sn["ambiguous"] += hits > 1
            sn[typ.lower()] += 1
        else:
            sn["unaligned"] += 1
        none = mm == C.NO_MM
        rows.append([x["tid"], P, side, 3, x["clen"], None if none else Q, None if none else strand, None if none else mm, hits, typ, ln, None, None])
    top = A.MAX_HOM - (bug == "hom")
    for i, r in enumerate(rows):
        if r[9] not in ("DEL", "DUP"):
            continue
        cand = sorted(((R[5] - L[1]), o[1]) for o in rows if o[0] == r[0] and o[2] != r[2] and o[9] == r[9] and o[10] == r[10]
                      for R, L in [(r, o) if r[2] == C.R_SIDE else (o, r)] if 0 <= R[5] - L[1] <= top)
        if cand:
            r[12], r[11] = cand[0]
            sn["mated"] += 1
    return np.array([sn[k] for k in A.SN], dtype=np.uint64), [tuple(r) for r in rows]


@pytest.fixture(scope="module")
def defined():
    """the definition over every case, computed once: {name: (placed, counters, rows)}"""
    return {c["name"]: C.definition(c) for c in C.CASES}


# ---- the three agree ----------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_families():
    assert {c["family"] for c in C.CASES} == {"events", "zero", "phase", "bounds", "order", "bases", "status", "structure"}
    assert C.N_CASES == len({c["name"] for c in C.CASES}) == 32
    assert all(c["W"] <= 300 for c in C.CASES)
    assert C.CA_STRIDE == C.CA_BLOCK and C.CA_GRID >= 1


def test_definition_restatement_and_claims_agree(defined):
    for c in C.CASES:
        placed, counts, rows = defined[c["name"]]
        assert C.agrees_with_claim(c, placed, rows) is None, c["name"]
        again = restate_sites(c)
        assert again == [tuple(int(v) for v in p) for p in placed], c["name"]
        counts2, rows2 = restate_rows(c, again)
        assert np.array_equal(counts, counts2) and rows == rows2, c["name"]
        assert C.agrees_with_claim(c, again, rows2) is None, c["name"]


def test_the_big_window_is_restated_where_it_was_planted():
    c = C.big_case()
    placed = restate_sites(c)
    _, rows = restate_rows(c, placed)
    assert C.agrees_with_claim(c, placed, rows) is None
    assert placed[0][1] == c["sites"][0]["P"] + (1 << 20)


DEPARTURES = {"tie": "order", "lt": "order", "guard": "bounds", "swap_L": "events", "no_comp": "events", "len_del": "events", "len_dup": "events",
              "len_inv": "events", "hom": "events"}


@pytest.mark.parametrize("bug", sorted(DEPARTURES))
def test_each_departure_is_noticed_in_its_family(bug):
    noticed = []
    for c in C.CASES:
        if c["family"] != DEPARTURES[bug]:
            continue
        placed = restate_sites(c, bug)
        _, rows = restate_rows(c, placed, bug)
        if C.agrees_with_claim(c, placed, rows) is not None:
            noticed.append(c["name"])
    assert noticed, bug


# ---- the switch -------------------------------------------------------------------------------------------------------------------
def test_parse_switch():
    assert A.parse_switch(None) is None and A.parse_switch("") is None and A.parse_switch(None, clips=False) is None
    assert A.parse_switch("1") == (10000, 20, 2)
    assert A.parse_switch("500") == (500, 20, 2)
    assert A.parse_switch("1:20") == (1, 20, 2)
    assert A.parse_switch("1048576:28:27") == (1 << 20, 28, 27)
    assert A.parse_switch("300:1:0") == (300, 1, 0)
    form = "the switch is 1, W, W:K or W:K:M (window 1 ... 2^20, minimum consensus columns 1 ... 28, maximum mismatches 0 ... 27)"
    for bad, text in (("0", "the window is 1 ... 2^20"), ("1048577", "the window is 1 ... 2^20"), ("5:40", "the minimum consensus columns are 1 ... 28"),
                      ("5:0", "the minimum consensus columns are 1 ... 28"), ("5:20:28", "the maximum mismatches are 0 ... 27"), ("yes", form), ("1:2:3:4", form),
                      ("-1", form), ("1:", form), ("1.5", form), ("1234567890", form), (" 1", form), ("١", form)):
        with pytest.raises(ValueError) as e:
            A.parse_switch(bad)
        assert str(e.value) == text, bad
    with pytest.raises(ValueError) as e:
        A.parse_switch("1", clips=False)
    assert str(e.value) == "the switch realigns the sites of TIDDIT_CLIPS, which is not set"


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def test_the_file_bytes(tmp_path):
    sites = [(0 << 32 | 428, 1, 7, 28), (0 << 32 | 601, 0, 5, 28), (1 << 32 | 50, 1, 3, 12), (1 << 32 | 90, 0, 4, 25), (1 << 32 | 95, 1, 3, 22)]
    placed = [(2, 629, 0, 0, 1), (2, 400, 0, 1, 2), (0, 0, 0, A.NO_MM, 0), (2, 300, 1, 5, 0), (2, 0, 0, A.NO_MM, 0)]
    counts, rows = A.summarise(sites, placed, 2)
    path = str(tmp_path / "x.clips.align.tab")
    A.write_file(path, counts, rows, ["chrA", "chrB"], 300, 20, 2)
    assert open(path, "rb").read() == (
        b"# tiddit_amd clips_align v1 window=300 min_cols=20 max_mismatch=2\n"
        b"SN\tsites\t5\nSN\tshort_consensus\t1\nSN\toff_reference\t0\nSN\tsearched\t4\nSN\taligned\t2\nSN\tambiguous\t1\nSN\tunaligned\t2\n"
        b"SN\tref\t0\nSN\tdel\t2\nSN\tdup\t0\nSN\tinv\t0\nSN\tmated\t2\n"
        b"#CHROM\tPOS\tSIDE\tSUPPORT\tCLEN\tPARTNER\tSTRAND\tMISMATCH\tHITS\tTYPE\tLEN\tMATE\tHOM\n"
        b"chrA\t428\tR\t7\t28\t629\t+\t0\t1\tDEL\t200\t601\t28\n"
        b"chrA\t601\tL\t5\t28\t400\t+\t1\t2\tDEL\t200\t428\t28\n"
        b"chrB\t90\tL\t4\t25\t300\t-\t5\t0\t.\t.\t.\t.\n"
        b"chrB\t95\tR\t3\t22\t.\t.\t.\t0\t.\t.\t.\t.\n")
