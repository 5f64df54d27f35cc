"""The definition of ``TIDDIT_CLIPS_MEI`` (tiddit_amd/tiddit_clip_mei.py) on the CPU: it meets every literal claim of
tests/clip_mei_cases.py; its two implementations (cell by cell, and by anti-diagonals over many queries) agree; two independent
restatements agree with it — Smith-Waterman by numpy ROWS with the gap along the query as a running maximum, for the score and the end
cell on every case, the 500 generated queries included, and a plain enumeration of every START cell with (score, start, end) tuples on
problems under 40 x 40 (drawn from two-letter alphabets, where ties are everywhere, and those of the aimed cases); ten departures from
the definition are each noticed by a named family of cases; ``parse_switch`` in every accepted form and every refusal; the file's text for a literal table; and the VCF
text of a named and of an unnamed pair.

Every test of this file fails on the parent commit: the module does not exist there."""
import functools

import numpy as np
import pytest

import clip_mei_cases as X

OPEN_, EXT_, MIS_, OTH_ = 7, 1, 4, 1                             # a gap's first base costs 6 + 1, every further one 1


@functools.lru_cache(maxsize=None)
def _definition(k):
    c = X.CASES[k] if k >= 0 else X.random_case()
    return (c,) + X.definition(c)


@pytest.mark.parametrize("k", range(X.N_AIMED), ids=[c["name"] for c in X.CASES])
def test_the_definition_meets_every_literal_claim(k):
    c, res, counts, calls = _definition(k)
    assert X.agrees_with_claim(c, res, counts, calls) is None
    assert all(w is not None for w in c["want"]) or c["family"] in ("pairs",)


def test_the_case_families_are_all_there():
    assert X.N_AIMED >= 50
    assert {c["family"] for c in X.CASES} == {"planted", "gap", "ties", "strand", "named", "library", "edges", "lengths", "lanes", "small", "pairs"}
    lengths = next(c for c in X.CASES if c["family"] == "lengths")
    assert [len(q) for q in lengths["queries"]] == list(range(1, X.QMAX + 1))


# ---- the two implementations of rule 3 ---------------------------------------------------------------------------------------------------
def test_cell_by_cell_and_by_anti_diagonals_are_the_same_integers():
    from tiddit_amd import tiddit_clip_mei as M
    n = 0
    for c in X.CASES:
        if c["family"] in ("lengths", "lanes"):
            continue
        lib = X.library_codes(c)
        for q in X.query_codes(c):
            for s in (q, M.reverse_complement(q)):
                for fam in lib:
                    assert M.align(s, fam) == M.align_batch([s], fam)[0], c["name"]
                    n += 1
    assert n >= 100


# ---- restatement 1: rows in numpy, score and end cell ------------------------------------------------------------------------------------
def _rows_scores(queries, fam):
    """score-only local alignment of many queries against one family, row by row: E from the row above, F as a running maximum along the
    row (a gap that opens from a cell reached by F is never better than extending that F) -> (best score, the cells that have it) per query"""
    B, N = len(queries), max(len(q) for q in queries)
    qq = np.full((B, N), -1, dtype=np.int64)
    for b, q in enumerate(queries):
        qq[b, :len(q)] = q
    live = qq >= 0
    onehot = np.where(live, 1 << np.maximum(qq, 0), 0)
    H = np.zeros((B, N + 1), dtype=np.int64)                      # column 0 is the border
    E = np.zeros((B, N), dtype=np.int64)
    best = np.zeros(B, dtype=np.int64)
    cells = [[] for _ in range(B)]
    j = np.arange(N, dtype=np.int64)
    for i, fc in enumerate(np.asarray(fam).tolist()):
        s = np.where(onehot == fc, 1, -(MIS_ if fc in (1, 2, 4, 8) else OTH_))
        E = np.maximum(np.maximum(H[:, 1:] - OPEN_, E - EXT_), 0)
        h0 = np.maximum(np.maximum(H[:, :-1] + s, E), 0)         # without F
        # F[j] = max over k < j of h[k] - 6 - (j - k), and h[k] >= h0[k] only through F itself
        run = np.maximum.accumulate(h0 + j, axis=1)
        F = np.concatenate([np.zeros((B, 1), dtype=np.int64), run[:, :-1] - (OPEN_ - EXT_)], axis=1) - j
        h = np.where(live, np.maximum(h0, F), 0)
        H = np.concatenate([np.zeros((B, 1), dtype=np.int64), h], axis=1)
        top = h.max(axis=1)
        for b in np.nonzero(top >= np.maximum(best, 1))[0]:
            if top[b] > best[b]:
                best[b], cells[b] = top[b], []
            cells[b] += [(i, int(x)) for x in np.nonzero(h[b] == top[b])[0]]
    return best, cells


def _check_rows(c, res):
    from tiddit_amd import tiddit_clip_mei as M
    qs = X.query_codes(c)
    both = qs + [M.reverse_complement(q) for q in qs]
    per = [_rows_scores(both, fam) for fam in X.library_codes(c)]
    for qi, (q, r) in enumerate(zip(qs, res)):
        scores = {(f, s): int(per[f][0][s * len(qs) + qi]) for f in range(len(per)) for s in (0, 1)}
        top = max(scores.values())
        assert int(r[2]) == top, (c["name"], qi)
        if not top:
            assert r[0] == X.NONE
            continue
        f, s = int(r[0]), int(r[1])
        assert (f, s) == min(k for k, v in scores.items() if v == top), (c["name"], qi)
        qend0 = len(q) - int(r[3]) if s else int(r[4]) - 1        # (the end cell in the strand's own coordinates)
        assert (int(r[6]) - 1, qend0) in per[f][1][s * len(qs) + qi], (c["name"], qi)
        others = [v for (f2, _), v in scores.items() if f2 != f]
        assert int(r[7]) == (max(others) if others else 0), (c["name"], qi)


@pytest.mark.parametrize("k", range(X.N_AIMED), ids=[c["name"] for c in X.CASES])
def test_the_restatement_by_rows_agrees_on_every_aimed_case(k):
    c, res, _, _ = _definition(k)
    _check_rows(c, res)


def test_the_restatement_by_rows_agrees_on_the_500_generated_queries():
    c, res, counts, _ = _definition(-1)
    assert len(res) == 500 and int(counts[4]) + int(counts[5]) == 500 and int(counts[4]) >= 400 and int(counts[6]) >= 100
    _check_rows(c, res)


# ---- restatement 2: every start cell, tuples ---------------------------------------------------------------------------------------------
def _from_start(q, fam, i0, j0, open_=OPEN_, ext=EXT_, other=OTH_, empty_below=1):
    """the best (score, i, j) per end cell of the alignments that START with the pair (i0, j0) and never fall below ``empty_below``"""
    n, m = len(q), len(fam)
    sc = lambda i, j: 1 if fam[i] == 1 << q[j] else -(MIS_ if fam[i] in (1, 2, 4, 8) else other)
    keep = lambda v: v if v is not None and v >= empty_below else None
    mx = lambda *v: max([x for x in v if x is not None], default=None)
    H, E, F, out = {}, {}, {}, []
    for i in range(i0, m):
        for j in range(j0, n):
            d = sc(i, j) if (i, j) == (i0, j0) else (H.get((i - 1, j - 1)) + sc(i, j) if H.get((i - 1, j - 1)) is not None else None)
            e = mx(keep(H[(i - 1, j)] - open_) if H.get((i - 1, j)) is not None else None, keep(E[(i - 1, j)] - ext) if E.get((i - 1, j)) is not None else None)
            f = mx(keep(H[(i, j - 1)] - open_) if H.get((i, j - 1)) is not None else None, keep(F[(i, j - 1)] - ext) if F.get((i, j - 1)) is not None else None)
            H[(i, j)], E[(i, j)], F[(i, j)] = mx(keep(d), e, f), e, f
            if H[(i, j)] is not None:
                out.append((H[(i, j)], i, j))
    return out


def enumerate_starts(q, fam, later_start=False, **knobs):
    """rule 3 by enumeration -> (score, fstart, qstart, fend, qend) or None: the larger score, then the smaller start, then the smaller end"""
    best = None
    for i0 in range(len(fam)):
        for j0 in range(len(q)):
            for score, i, j in _from_start(q, fam, i0, j0, **knobs):
                cand = (score, (i0, j0) if later_start else (-i0, -j0), -i, -j)
                if best is None or cand > best[0]:
                    best = (cand, (score, i0, j0, i, j))
    return None if best is None else best[1]


def _unpack(r):
    from tiddit_amd import tiddit_clip_mei as M
    key, fend, qend = r
    if not key:
        return None
    start = M.NONE - (key & M.NONE)
    return (key >> 32, start >> M.POS_BITS, start & 511, fend, qend)


def test_the_enumeration_of_start_cells_agrees_where_ties_are_everywhere():
    from tiddit_amd import tiddit_clip_mei as M
    rs = np.random.RandomState(5)
    n = 0
    for k in range(60):
        letters = (1, 2) if k % 3 else (1, 2, 4, 15)             # two-letter families: ties everywhere; every third with other bases
        fam = [letters[x] for x in rs.randint(0, len(letters), int(rs.randint(1, 40)))]
        q = [int(x) for x in rs.randint(0, 2, int(rs.randint(1, 25)))]
        if k % 5 == 0:
            q = [{1: 0, 2: 1, 4: 2}.get(x, 3) for x in fam[2:20]] or q   # a long copy, so that gaps pay
            q = q[:len(q) // 2] + q[len(q) // 2 + 2:] if len(q) > 16 else q
        assert _unpack(M.align(q, fam)) == enumerate_starts(q, fam), (k, q, fam)
        n += 1
    assert n == 60
    # ... and every problem of the aimed cases that is under 40 x 40, on both strands
    for c in X.CASES:
        for q in X.query_codes(c):
            for fam in X.library_codes(c):
                if len(q) <= 40 and len(fam) <= 40:
                    for s in (q, M.reverse_complement(q)):
                        assert _unpack(M.align(s, fam)) == enumerate_starts(s, [int(x) for x in fam]), c["name"]
                        n += 1
    assert n >= 60 + 12


# ---- departures ---------------------------------------------------------------------------------------------------------------------------
def _variant_results(c, strand_first=0, family_order=1, second_same_family=False, concatenated=False, convert_minus=True, **knobs):
    """rules 3 and 4 by enumeration is too slow for 60 x 300: rule 3 here is the definition's recurrence on (score, -fstart, -qstart) tuples
    with the knobs of a departure -> the nine columns per query"""
    from tiddit_amd import tiddit_clip_mei as M
    lib = X.library_codes(c)
    if concatenated:                                             # every family runs on into the next one's bases
        lib = [np.concatenate(lib[f:]) for f in range(len(lib))]
    out = []
    for q in X.query_codes(c):
        probs = {}
        for f, fam in enumerate(lib):
            for s in (0, 1):
                r = _tuple_align(M.reverse_complement(q) if s else q, [int(x) for x in fam], **knobs)
                probs[(f, s)] = r
        live = {k: v for k, v in probs.items() if v is not None}
        if not live:
            out.append((X.NONE, 0, 0, 0, 0, 0, 0, 0, X.NONE))
            continue
        f, s = min(live, key=lambda k: (-live[k][0], family_order * k[0], k[1] if strand_first == 0 else -k[1]))
        score, fs, qs, fe, qe = live[(f, s)]
        others = [(v[0], f2) for (f2, s2), v in live.items() if (f2 != f or (second_same_family and s2 != s))]
        second = max((v for v, _ in others), default=0)
        sf = min((f2 for v, f2 in others if v == second), default=X.NONE)
        n = len(q)
        qa, qb = (n - qe, n - qs) if s and convert_minus else (qs + 1, qe + 1)
        out.append((f, s, score, qa, qb, fs + 1, fe + 1, second, sf))
    return out


def _tuple_align(q, fam, open_=OPEN_, ext=EXT_, other=OTH_, empty_below=1, later_start=False):
    sgn = 1 if later_start else -1
    n, m = len(q), len(fam)
    keep = lambda v: v if v is not None and v[0] >= empty_below else None
    less = lambda v, p: keep((v[0] - p,) + v[1:]) if v is not None else None
    mx = lambda *v: max([x for x in v if x is not None], default=None)
    Hp, Ep, best = [None] * n, [None] * n, None
    for i in range(m):
        H, E, f, left = [None] * n, [None] * n, None, None
        acgt = fam[i] in (1, 2, 4, 8)
        for j in range(n):
            e = mx(less(Hp[j], open_), less(Ep[j], ext))
            f = mx(less(left, open_), less(f, ext))
            d0 = (Hp[j - 1] if j else None) or (0, sgn * i, sgn * j)
            s = 1 if fam[i] == 1 << q[j] else -(MIS_ if acgt else other)
            h = mx(keep((d0[0] + s,) + d0[1:]), e, f)
            H[j], E[j], left = h, e, h
            if h is not None and (best is None or h > best[0]):
                best = (h, i, j)
        Hp, Ep = H, E
    if best is None:
        return None
    (score, a, b), i, j = best
    return score, sgn * a, sgn * b, i, j


def _noticed(family, **knobs):
    """how many cases of ``family`` contradict the departure's results (and, first, none contradicts the results without a departure)"""
    cases = [c for c in X.CASES if c["family"] == family]
    assert cases and all(X.agrees_with_claim(c, _variant_results(c)) is None for c in cases), family
    return sum(X.agrees_with_claim(c, _variant_results(c, **knobs)) is not None for c in cases)


DEPARTURES = [("the gap extension charged twice on the opening base", "gap", {"open_": OPEN_ + 1}),
              ("the gap opening forgotten", "gap", {"open_": EXT_}),
              ("ties to the later start", "ties", {"later_start": True}),
              ("strand - in front of strand +", "strand", {"strand_first": 1}),
              ("a strand - span left in the reverse complement's coordinates", "strand", {"convert_minus": False}),
              ("another base scores 0", "library", {"other": 0}),
              ("EMPTY at < 0 rather than <= 0", "planted", {"empty_below": 0}),
              ("SECOND taken from the same family's other strand", "strand", {"second_same_family": True}),
              ("ties to the larger family index", "ties", {"family_order": -1}),
              ("the bases behind a family's end read", "edges", {"concatenated": True})]


@pytest.mark.parametrize("what,family,knobs", DEPARTURES, ids=[d[0] for d in DEPARTURES])
def test_a_departure_is_noticed_by_its_family_of_cases(what, family, knobs):
    if what.startswith("SECOND"):
        # (the palindrome's strand - is the same family at the same score: SECOND would be 34, and the case claims 0)
        pal = next(c for c in X.CASES if "palindrome" in c["name"])
        assert pal["second"] is None
        pal = dict(pal, second=[(0, X.NONE)])
        assert X.agrees_with_claim(pal, _variant_results(pal)) is None and X.agrees_with_claim(pal, _variant_results(pal, **knobs)) is not None
        return
    assert _noticed(family, **knobs) >= 1


# ---- the switch ---------------------------------------------------------------------------------------------------------------------------
def _library(tmp_path, name="lib.fa", library=X.JOB_LIBRARY):
    from tiddit_amd import fasta
    p = str(tmp_path / name)
    X.write_library(p, library)
    fasta.build_fai(p)
    return p


def test_parse_switch_accepts_the_library_with_and_without_a_minimum(tmp_path):
    from tiddit_amd import tiddit_clip_mei as M
    p = _library(tmp_path)
    assert M.parse_switch(None) is None and M.parse_switch("") is None and M.parse_switch(None, "") is None and M.parse_switch("", None, False, False) is None
    assert M.parse_switch(p) == (p, 30) and M.parse_switch(p, "") == (p, 30)
    assert M.parse_switch(p, "12") == (p, 12) and M.parse_switch(p, "280") == (p, 280) and M.parse_switch(p, "045") == (p, 45)
    fa, names, lengths = M.library_index(p)
    assert names == ["AluX", "L1X", "SvaX"] and lengths == [300, 900, 500]


def test_parse_switch_refuses_everything_else(tmp_path):
    from tiddit_amd import tiddit_clip_mei as M
    p = _library(tmp_path)
    for args, text in (((p, None, False, True), "TIDDIT_CLIPS is not set"), ((p, None, True, False), "TIDDIT_CLIPS_INS, which is not set"),
                       ((None, "30"), "TIDDIT_CLIPS_MEI, which is not set"), (("", "30"), "TIDDIT_CLIPS_MEI, which is not set"),
                       ((p, "11"), "12 ... 280"), ((p, "281"), "12 ... 280"), ((p, "x"), "12 ... 280"), ((p, "-30"), "12 ... 280"), ((p, "3" * 10), "12 ... 280"),
                       ((str(tmp_path / "missing.fa"),), "cannot be read"), ((str(tmp_path),), "cannot be read")):
        with pytest.raises(ValueError) as e:
            M.parse_switch(*args)
        assert text in str(e.value), (args, str(e.value))
    for name, lib, text in (("none.fa", [], "0 sequences"), ("many.fa", [("s%d" % k, "ACGT") for k in range(4097)], "4097 sequences"),
                            ("long.fa", [("a", "A" * ((1 << 20) + 1))], "2^20"), ("sum.fa", [("a", "A" * (1 << 19)), ("b", "C" * (1 << 19)), ("c", "G")], "at most 2^20"),
                            ("twice.fa", [("a", "ACGT"), ("a", "ACGT")], "one name")):
        with pytest.raises(ValueError) as e:
            M.parse_switch(_library(tmp_path, name, lib))
        assert text in str(e.value), (name, str(e.value))
    empty = str(tmp_path / "empty.fa")
    open(empty, "w").write(">a\n\n>b\nACGT\n")
    from tiddit_amd import fasta
    fasta.build_fai(empty)
    with pytest.raises(ValueError) as e:
        M.parse_switch(empty)
    assert "0 bases" in str(e.value)


# ---- the file and the VCF -------------------------------------------------------------------------------------------------------------------
INS_ROWS = [(0, 2000, 2001, 0, 7, 7, 140, 140, 1, 130, 0, 1, "ACGT" * 32 + "AC", "A" * 140, "C" * 140),
            (0, 4000, 3986, 15, 7, 7, 140, 140, 0, None, None, 0, ".", "G" * 140, "T" * 140),
            (1, 500, 501, 0, 3, 4, 40, 50, 1, 60, 1, 1, "ACGT" * 15, "A" * 40, "C" * 50)]
MEI_ROWS = [(0, 2000, 2001, 1, 0, 130, 1, 1, 118, 3, 130, 51, 178, 118, 0), (0, 4000, 3986, 0, 1, 140, 0, 0, 140, 1, 140, 101, 240, 17, 2),
            (0, 4000, 3986, 0, 2, 140, 0, 0, 29, 5, 33, 600, 628, 0, 0xffffffff), (1, 500, 501, 1, 0, 60, 0xffffffff, 0, 0, 0, 0, 0, 0, 0, 0xffffffff)]
MEI_TEXT = ("# tiddit_amd clips_mei v1 match=1 mismatch=4 gap_open=6 gap_extend=1 other=1 min_score=30 families=3 bases=1700\n"
            "SN\tqueries\t4\nSN\tclosed_queries\t2\nSN\tleft_queries\t1\nSN\tright_queries\t1\nSN\tnamed\t2\nSN\tunnamed\t2\nSN\treverse\t1\nSN\tambiguous\t1\n"
            "SN\tpairs_named\t2\nSN\tpairs_conflict\t0\n"
            "#CHROM\tPOS\tEND\tSTATUS\tPART\tQLEN\tFAMILY\tSTRAND\tSCORE\tQSTART\tQEND\tFSTART\tFEND\tSECOND\tSECOND_FAMILY\n"
            "chrA\t2000\t2001\tCLOSED\tSEQ\t130\tL1X\t-\t118\t3\t130\t51\t178\t118\tAluX\n"
            "chrA\t4000\t3986\tOPEN\tLEFT\t140\tAluX\t+\t140\t1\t140\t101\t240\t17\tSvaX\n"
            "chrA\t4000\t3986\tOPEN\tRIGHT\t140\t.\t.\t.\t.\t.\t.\t.\t.\t.\n"
            "chrB\t500\t501\tCLOSED\tSEQ\t60\t.\t.\t.\t.\t.\t.\t.\t.\t.\n")


def test_the_file_text_of_a_literal_table(tmp_path):
    from tiddit_amd import tiddit_clip_mei as M
    res, parts = [r[6:] for r in MEI_ROWS], [r[4] for r in MEI_ROWS]
    counts, calls = M.summarise(res, parts, 30, [0, 1, 1, 2])
    assert counts.tolist() == [4, 2, 1, 1, 2, 2, 1, 1, 2, 0] and calls == {0: (1, 1, 118, 51, 178), 1: (0, 0, 140, 101, 240)}
    p = str(tmp_path / "t.clips.mei.tab")
    M.write_file(p, counts, MEI_ROWS, ["chrA", "chrB"], ["AluX", "L1X", "SvaX"], 1700, 30)
    assert open(p).read() == MEI_TEXT
    assert M.file_rows(INS_ROWS, [0, 1, 1, 2], parts, [r[5] for r in MEI_ROWS], list(zip(*res))) == MEI_ROWS
    assert M.queries_of_rows(INS_ROWS) == [(0, 0, INS_ROWS[0][12]), (1, 1, "G" * 140), (1, 2, "T" * 140), (2, 0, "ACGT" * 15)]
    assert M.calls_for_vcf(MEI_ROWS, 30, ["AluX", "L1X", "SvaX"]) == {0: ("L1X", "-", 118, 51, 178), 1: ("AluX", "+", 140, 101, 240)}
    assert M.summary_line(counts) == "clips mei: 4 queries (2 closed, 1 left, 1 right), 2 named (1 reverse, 1 ambiguous), 2 unnamed, 2 pairs named, 0 in conflict"


def test_the_vcf_text_of_a_named_and_of_an_unnamed_pair(tmp_path):
    from tiddit_amd import tiddit_clip_vcf as V
    parts = (["##contig=<ID=chrA,length=12000>", "##contig=<ID=chrB,length=8000>"], "##TIDDITcmd=x", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts", "3.9.5")
    of = lambda t: []
    plain, named = str(tmp_path / "plain.vcf"), str(tmp_path / "named.vcf")
    V.definition_file(plain, parts, ["chrA", "chrB"], [12000, 8000], 10, of, ins_rows=INS_ROWS)
    V.definition_file(named, parts, ["chrA", "chrB"], [12000, 8000], 10, of, ins_rows=INS_ROWS, mei=(30, MEI_ROWS, ["AluX", "L1X", "SvaX"]))
    a, b = open(plain).read().split("\n"), open(named).read().split("\n")
    extra = [l for l in b if l not in a]
    assert [l for l in a if l not in b] == [x for x in a if x.startswith("chrA")] and len(b) == len(a) + 5
    assert extra[:5] == ['##INFO=<ID=MEI,Number=1,Type=String,Description="Family of the library that the inserted sequence aligns to best">',
                         '##INFO=<ID=MEISTRAND,Number=1,Type=String,Description="Strand of the family the inserted sequence lies on">',
                         '##INFO=<ID=MEISCORE,Number=1,Type=Integer,Description="Local alignment score against the family (match 1, mismatch 4, gap 6 + length)">',
                         '##INFO=<ID=MEISPAN,Number=2,Type=Integer,Description="First and last base of the family that the alignment covers">',
                         "##clips_vcf_mei_min_score=30"]
    assert b.index("##clips_vcf_mei_min_score=30") == b.index("##clips_vcf_flank=10") + 1
    rec = lambda lines, chrom, pos: next(l for l in lines if l.startswith("%s\t%d\t" % (chrom, pos)))
    assert rec(b, "chrA", 2000) == rec(a, "chrA", 2000).replace("SRC=ins;MISMATCH=0", "SRC=ins;MISMATCH=0;MEI=L1X;MEISTRAND=-;MEISCORE=118;MEISPAN=51,178")
    assert rec(b, "chrA", 3985) == rec(a, "chrA", 3985).replace("SRC=ins", "SRC=ins;MEI=AluX;MEISTRAND=+;MEISCORE=140;MEISPAN=101,240")
    assert rec(b, "chrB", 500) == rec(a, "chrB", 500) and "MEI" not in rec(b, "chrB", 500)
    assert rec(b, "chrA", 2000).split("\t")[7] == ("SVTYPE=INS;END=2000;SVLEN=130;CIPOS=0,0;TSD=0;SVINSSEQ=%s;SRC=ins;MISMATCH=0;MEI=L1X;MEISTRAND=-;MEISCORE=118;"
                                                   "MEISPAN=51,178" % INS_ROWS[0][12])
