"""The genome-wide placement of clip-site consensus without a GPU: the definition of tiddit_amd/tiddit_clip_far.py (per site, the seed
looked up with ``bytes.find``), an independent numpy restatement (every 16-mer of the reference as an integer, joined on the sites' seeds
through a sort; the other columns compared over arrays; the mates by sorting) and the literal claims of tests/clip_far_cases.py agree on
every case; each one-line departure of the restatement is noticed inside the family that is listed for it; the switch's three forms and
its refusals; the file's bytes on a literal example."""
import numpy as np
import pytest

import clip_far_cases as C
from tiddit_amd import tiddit_clip_far as F

_LUT = np.full(16, 4, dtype=np.int64)          # a 4-bit reference code -> 0 ... 3, or 4 for what is no base
_LUT[[1, 2, 4, 8]] = [0, 1, 2, 3]
PAD = 32


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _index(c, bug=None):
    """per loaded contig: the padded bases and all its 16-mers as integers (-1 where a window holds what is no base), sorted"""
    ref = C.host_reference(c)
    out = {}
    for t, codes in sorted(ref.contigs.items()):
        pad = np.full(PAD, 0 if bug == "guard_a" else 4, dtype=np.int64)
        g = np.concatenate([pad, _LUT[codes], pad])                # base q (1-based) is g[q + PAD - 1]
        n = len(g) - 15
        kmers = np.zeros(n, dtype=np.int64)
        bad = np.zeros(n, dtype=bool)
        for j in range(16):
            kmers |= (g[j:j + n] & 3) << (30 - 2 * j)
            bad |= g[j:j + n] > 3
        kmers[bad] = -1
        order = np.argsort(kmers, kind="stable")
        out[t] = (g, len(codes), kmers, order, kmers[order])
    return out


def restate_sites(c, bug=None, index=None):
    """every site's (status, contig, PARTNER, strand, mm, HITS) by a join of the sites' seeds on the reference's 16-mers; ``bug``: one
    departure from the definition"""
    index = index or _index(c, bug)
    K, M = c["K"], c["M"]
    seed = 15 if bug in ("seed15", "tail15") else 16
    tail_from = 15 if bug == "tail15" else 16
    out = []
    for x in c["sites"]:
        tid, P, side, cl = x["tid"], x["P"], x["side"], x["clen"]
        if cl < K:
            out.append((C.SHORT, 0, 0, 0, C.NO_MM, 0))
            continue
        if tid not in index or not 1 <= P <= index[tid][1]:
            out.append((C.OFF, 0, 0, 0, C.NO_MM, 0))
            continue
        cols = np.array([(x["cons"] >> (2 * j)) & 3 for j in range(cl)], dtype=np.int64)
        keys = []
        for t, (g, ln, kmers, order, skm) in index.items():
            for strand in (0, 1):
                step = 1 if (side == C.R_SIDE) == (strand == 0) else -1
                want = 3 - cols if strand and bug != "no_comp" else cols
                # the seed's bases over ascending reference positions, and where Q lies in its window
                asc = want[:16] if step == 1 else want[:16][::-1]
                key = int(sum(int(b) << (30 - 2 * j) for j, b in enumerate(asc)))
                if seed == 16:
                    at = order[np.searchsorted(skm, key, "left"):np.searchsorted(skm, key, "right")]
                else:                                              # column 15 is free: the last base ascending, the first descending
                    mask = ~(3 << (0 if step == 1 else 30))
                    at = np.flatnonzero((kmers >= 0) & ((kmers & mask) == (key & mask)))
                Q = (at - PAD + 1) + (0 if step == 1 else 15)      # `at` indexes g: base at - PAD + 1 is the window's first
                last = Q + step * (cl - 1)
                lo, hi = (0 if bug == "bounds_lo" else 1), (ln + 1 if bug == "bounds_hi" else ln)
                ok = (last >= lo) & (last <= hi) if bug != "guard_a" else (Q >= 1) & (Q <= ln)
                Q = Q[ok]
                mm = np.zeros(len(Q), dtype=np.int64)
                for j in range(tail_from, cl):
                    mm += g[Q + step * j + PAD - 1] != want[j]
                good = (mm < M) if bug == "lt" else (mm <= M)
                Q, mm = Q[good], mm[good]
                other = 0 if bug == "no_own" else int(t != tid)
                dist = np.abs(Q - P) if t == tid and bug != "no_own" else np.zeros(len(Q), dtype=np.int64)
                keys.append(np.stack([mm, np.full(len(Q), other), dist, np.full(len(Q), strand), np.full(len(Q), t), Q], axis=1))
        keys = np.concatenate(keys)
        if not len(keys):
            out.append((C.SEARCHED, 0, 0, 0, C.NO_MM, 0))
            continue
        mm, _, _, strand, t, q = keys[np.lexsort(tuple(keys[:, k] for k in (5, 4, 3, 2, 1, 0)))[0]].tolist()
        out.append((C.SEARCHED, t, q, strand, mm, len(keys)))
    return out


def restate_rows(c, placed, bug=None):
    """the counters and rows of summarise, restated: the mates by a sort of the admissible pairs"""
    sn = dict.fromkeys(F.SN, 0)
    rows = []
    for x, (status, pt, Q, strand, mm, hits) in zip(c["sites"], placed):
        sn["sites"] += 1
        sn[("short_consensus", "off_reference", "searched")[status]] += 1
        if status != C.SEARCHED:
            continue
        P, side, tid = x["P"], x["side"], x["tid"]
        if mm == C.NO_MM:
            sn["unplaced"] += 1
            rows.append([tid, P, side, 3, x["clen"], None, None, None, None, 0, None, None, None, None, None])
            continue
        sn["placed"] += 1
        sn["ambiguous"] += hits > 1
        sn["same_contig" if pt == tid else "other_contig"] += 1
        sn["reverse"] += strand
        if pt != tid:
            typ, ln = "BND", None
        else:
            d = Q - P if side == C.R_SIDE else P - Q               # the partner's offset away from the aligned part
            typ, ln = ("INV", abs(d)) if strand else ("REF", 0) if d == 1 else ("DEL", d - 1) if d > 1 else ("DUP", 1 - d)
        rows.append([tid, P, side, 3, x["clen"], pt, Q, strand, mm, hits, typ, ln, None, None, None])
    fwd = [r for r in rows if r[10] is not None and r[7] == 0]
    for r in fwd:
        cand = sorted((R[6] - L[1], o[0], o[1]) for o in fwd if o[2] != r[2] and o[0] == r[5] and o[5] == r[0]
                      for R, L in [(r, o) if r[2] == C.R_SIDE else (o, r)]
                      if 0 <= R[6] - L[1] <= F.MAX_HOM and (bug == "mate_eq" or R[6] - L[1] == R[1] - L[6]))
        if cand:
            r[14], r[12], r[13] = cand[0]
            sn["mated"] += 1
    return np.array([sn[k] for k in F.SN], dtype=np.uint64), [tuple(r) for r in rows]


@pytest.fixture(scope="module")
def defined():
    """the definition over every case, computed once: {name: (placed, counters, rows)}"""
    return {c["name"]: C.definition(c) for c in C.CASES}


# ---- the three agree ----------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_families():
    assert {c["family"] for c in C.CASES} == {"phase", "bounds", "unloaded", "bases", "mismatch", "order", "hits", "filter", "structure", "zero", "events", "random"}
    assert C.N_CASES == len({c["name"] for c in C.CASES}) == len(C.CASES) == 43
    assert len(next(c for c in C.CASES if c["family"] == "phase")["sites"]) == 16 * 13 * 2 * 2
    assert len(C.CASES[-1]["sites"]) == 2000 and sum(len(s) for s in C.CASES[-1]["contigs"]) == 100000
    assert C.FAR_TILE == C.FAR_BLOCK * C.FAR_RUN and C.FAR_RUN == 32 and C.FAR_GRID >= 1 and 10 <= C.FAR_FILTER_LOG2 <= 21
    assert C.FAR_HASH_MUL % 2 == 1 and C.FAR_HASH_MUL < 1 << 32


def test_definition_restatement_and_claims_agree(defined):
    for c in C.CASES:
        placed, counts, rows = defined[c["name"]]
        assert C.agrees_with_claim(c, placed, rows) is None, (c["name"], C.agrees_with_claim(c, placed, rows))
        again = restate_sites(c)
        assert again == [tuple(int(v) for v in p) for p in placed], c["name"]
        counts2, rows2 = restate_rows(c, again)
        assert np.array_equal(counts, counts2) and rows == rows2, c["name"]
        assert C.agrees_with_claim(c, again, rows2) is None, c["name"]


def test_the_large_references_are_restated_where_they_were_planted():
    for c in C.big_cases():
        placed = restate_sites(c)
        counts, rows = restate_rows(c, placed)
        assert C.agrees_with_claim(c, placed, rows) is None, (c["name"], C.agrees_with_claim(c, placed, rows))
        again, counts2, rows2 = C.definition(c)
        assert [tuple(int(v) for v in p) for p in again] == placed and np.array_equal(counts, counts2) and rows == rows2, c["name"]


DEPARTURES = {"seed15": "mismatch", "tail15": "mismatch", "lt": "mismatch", "bounds_lo": "bounds", "bounds_hi": "bounds", "guard_a": "bounds",
              "no_own": "order", "no_comp": "phase", "mate_eq": "events"}


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
    assert F.parse_switch(None) is None and F.parse_switch("") is None and F.parse_switch(None, clips=False) is None
    assert F.parse_switch("1") == (20, 2)
    assert F.parse_switch("16") == (16, 2) and F.parse_switch("28") == (28, 2)
    assert F.parse_switch("24:0") == (24, 0) and F.parse_switch("16:12") == (16, 12) and F.parse_switch("028:02") == (28, 2)
    form = "the switch is 1, K or K:M (minimum consensus columns 16 ... 28, maximum mismatches 0 ... 12)"
    for bad, text in (("0", "the minimum consensus columns are 16 ... 28"), ("15", "the minimum consensus columns are 16 ... 28"),
                      ("29", "the minimum consensus columns are 16 ... 28"), ("20:13", "the maximum mismatches are 0 ... 12"), ("yes", form), ("20:2:1", form),
                      ("-1", form), ("20:", form), ("1.5", form), ("1234567890", form), (" 1", form), ("١", form)):
        with pytest.raises(ValueError) as e:
            F.parse_switch(bad)
        assert str(e.value) == text, bad
    with pytest.raises(ValueError) as e:
        F.parse_switch("1", clips=False)
    assert str(e.value) == "the switch places the sites of TIDDIT_CLIPS, which is not set"


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def test_the_file_bytes(tmp_path):
    sites = [(0 << 32 | 405, 1, 7, 28), (1 << 32 | 601, 0, 5, 28), (1 << 32 | 50, 1, 3, 12), (1 << 32 | 90, 0, 4, 25), (1 << 32 | 95, 1, 3, 22), (0 << 32 | 700, 1, 3, 20)]
    placed = [(2, 1, 606, 0, 0, 1), (2, 0, 400, 0, 1, 2), (0, 0, 0, 0, F.NO_MM, 0), (2, 1, 300, 1, 2, 3), (2, 0, 0, 0, F.NO_MM, 0), (2, 0, 900, 0, 0, 1)]
    counts, rows = F.summarise(sites, placed, 2)
    path = str(tmp_path / "x.clips.far.tab")
    F.write_file(path, counts, rows, ["chrA", "chrB"], 20, 2)
    assert open(path, "rb").read() == (
        b"# tiddit_amd clips_far v1 seed=16 min_cols=20 max_mismatch=2\n"
        b"SN\tsites\t6\nSN\tshort_consensus\t1\nSN\toff_reference\t0\nSN\tsearched\t5\nSN\tplaced\t4\nSN\tambiguous\t2\nSN\tunplaced\t1\n"
        b"SN\tsame_contig\t2\nSN\tother_contig\t2\nSN\treverse\t1\nSN\tmated\t2\n"
        b"#CHROM\tPOS\tSIDE\tSUPPORT\tCLEN\tPCHROM\tPARTNER\tSTRAND\tMISMATCH\tHITS\tTYPE\tLEN\tMATE_CHROM\tMATE\tHOM\n"
        b"chrA\t405\tR\t7\t28\tchrB\t606\t+\t0\t1\tBND\t.\tchrB\t601\t5\n"
        b"chrB\t601\tL\t5\t28\tchrA\t400\t+\t1\t2\tBND\t.\tchrA\t405\t5\n"
        b"chrB\t90\tL\t4\t25\tchrB\t300\t-\t2\t3\tINV\t210\t.\t.\t.\n"
        b"chrB\t95\tR\t3\t22\t.\t.\t.\t.\t0\t.\t.\t.\t.\t.\n"
        b"chrA\t700\tR\t3\t20\tchrA\t900\t+\t0\t1\tDEL\t199\t.\t.\t.\n")
    assert F.summary_line(counts) == "clips far: 6 sites, 5 searched, 4 placed (2 ambiguous), 1 unplaced, same contig 2, other contig 2, reverse 1, mated 2"
