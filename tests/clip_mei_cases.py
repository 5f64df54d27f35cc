"""Aimed cases for the naming of inserted sequences (tiddit_amd/tiddit_clip_mei.py, csrc/tdt_swalign.hip), each with the literal result
it claims, written down from what the case PLANTED — never computed by the definition or by the restatement of
tests/test_clip_mei_refs_cpu.py.

A case is a library ``[(name, text)]``, queries (texts, in reference direction) and per query the claim ``(family, strand, score,
qstart, qend, fstart, fend)`` (1-based, ``None`` where the case claims nothing: a base or two of a very short query can sit anywhere),
optionally the claim ``(second, second_family)`` and the counters that follow.  The backgrounds are seeded random bases: a chance
alignment in them scores a dozen at the most, the planted ones 24 or more.  PAIR cases add every query's part and pair row.  The JOB is
a generated reference of two contigs and 20 kb with insertions cut from a library of three families and the sample's reads over them."""
import os
import re

import numpy as np

import clip_cases as D
import clip_ins_cases as C
from clip_align_cases import Seq, fasta_raw, other, rc, seeded

NONE = 0xffffffff
PLUS, MINUS = 0, 1
SEQ, LEFT, RIGHT = 0, 1, 2
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(_ROOT, "tiddit_amd", "csrc", "tdt_swalign.hip")).read()
FAM_BLOCK = int(re.search(r"^#define SW_FAM_BLOCK (\d+)\b", _SRC, re.M).group(1))       # family codes a wave takes at a time: the only block size
MAX_COLS = int(re.search(r"^#define SW_MAX_COLS (\d+)\b", _SRC, re.M).group(1))         # query columns of a lane at most
_HDR = open(os.path.join(_ROOT, "include", "tiddit_hip.h")).read()
QMAX = int(re.search(r"^#define TDT_SW_QMAX (\d+)\b", _HDR, re.M).group(1))
SCORES = {k: int(re.search(r"^#define TDT_SW_%s (\d+)\b" % k, _HDR, re.M).group(1)) for k in ("MATCH", "MISMATCH", "GAP_OPEN", "GAP_EXTEND", "OTHER")}
assert (FAM_BLOCK, MAX_COLS, QMAX) == (64, 5, 280) and SCORES == {"MATCH": 1, "MISMATCH": 4, "GAP_OPEN": 6, "GAP_EXTEND": 1, "OTHER": 1}

CASES = []
_R = lambda n, seed: seeded(n, 11000 + seed)


def case(family, name, claims, library, queries, want, second=None, sn=None, A=30, parts=None, pairs=None, calls=None):
    assert len(want) == len(queries) and all(1 <= len(q) <= QMAX for q in queries)
    CASES.append({"family": family, "name": family + ": " + name, "claims": claims, "library": [(n, t) for n, t in library], "queries": list(queries),
                  "want": list(want), "second": second, "sn": sn, "A": A, "parts": parts, "pairs": pairs, "calls": calls})


def sub(s, j, ch=None):
    """base j (0-based) of s replaced by ch, or by a base that differs from it"""
    return s[:j] + (ch or other(s[j])) + s[j + 1:]


def unlike(*chs):
    """a base that differs from all of ``chs``"""
    return next(b for b in "ACGT" if b not in chs)


def library_codes(c):
    from tiddit_amd import refseq
    return [refseq.codes_of_bases(t) for _, t in c["library"]]


def query_codes(c):
    return [["ACGT".index(ch) for ch in q] for q in c["queries"]]


def definition(c):
    """the definition over the case -> (the nine columns per query, the counters, the pair calls)"""
    from tiddit_amd import tiddit_clip_mei as M
    res = M.results(query_codes(c), library_codes(c))
    counts, calls = M.summarise(res, c["parts"] or [SEQ] * len(res), c["A"], c["pairs"])
    return res, counts, calls


def agrees_with_claim(c, res, counts=None, calls=None):
    """the nine columns per query (of the definition, of the restatement, of the device) against the claims -> None or what differs"""
    from tiddit_amd import tiddit_clip_mei as M
    for qi, (r, w) in enumerate(zip(res, c["want"])):
        if w is None:
            continue
        got = tuple(int(v) for v in r[:7])
        if any(x is not None and x != g for x, g in zip(w, got)):
            return "query %d: %s / %s" % (qi, got, w)
    for qi, w in enumerate(c["second"] or ()):
        if w is not None and (int(res[qi][7]), int(res[qi][8])) != w:
            return "query %d: second %s / %s" % (qi, (int(res[qi][7]), int(res[qi][8])), w)
    if counts is not None and c["sn"] is not None:
        got = {k: int(counts[M.SN_INDEX[k]]) for k in c["sn"]}
        if got != c["sn"]:
            return "counters %s / %s" % (got, c["sn"])
    if calls is not None and c["calls"] is not None and dict(calls) != c["calls"]:
        return "pair calls %s / %s" % (dict(calls), c["calls"])
    return None


# ------------------------------------------------------------------------------------------- planted alignments and ties
_BG = _R(300, 1)                                                # a family: 300 background bases
_P = _BG[100:160]                                               # a piece of 60 bases at family bases 101 ... 160
_LIB = [("FamA", _BG)]
case("planted", "an exact copy", "60 bases of the family: score 60, the whole query at 101 ... 160", _LIB, [_P], [(0, PLUS, 60, 1, 60, 101, 160)],
     second=[(0, NONE)], sn={"queries": 1, "closed_queries": 1, "named": 1, "unnamed": 0, "reverse": 0, "ambiguous": 0, "pairs_named": 1, "pairs_conflict": 0})
case("planted", "one interior mismatch", "base 31 of the copy differs: 59 matches and one mismatch, 59 - 4 = 55 = n - 5, the full span", _LIB, [sub(_P, 30)],
     [(0, PLUS, 55, 1, 60, 101, 160)])
for _p in (1, 2, 3, 4, 5):
    # kept: n - 5; clipped: the n - p - 1 bases on the far side.  p = 4: behind four matches the mismatch leaves a score of 0, which is EMPTY, so
    # the alignment from the left end ends there and the clipped one is the only one of 55; from the right end the two share their start and key
    case("planted", "a mismatch %d bases from the left end" % _p,
         "kept it scores 55, clipped 60 - %d - 1 = %d: %s" % (_p, 59 - _p, "clipped" if _p < 4 else "4 - 4 = 0 is EMPTY: clipped" if _p == 4 else "kept"),
         _LIB, [sub(_P, _p)], [(0, PLUS, 59 - _p, _p + 2, 60, 102 + _p, 160) if _p <= 4 else (0, PLUS, 55, 1, 60, 101, 160)])
    case("planted", "a mismatch %d bases from the right end" % _p,
         "kept it scores 55, clipped %d: %s" % (59 - _p, "clipped" if _p < 4 else "a tie of one start and one key: the smaller end, clipped" if _p == 4 else "kept"),
         _LIB, [sub(_P, 59 - _p)], [(0, PLUS, 59 - _p, 1, 59 - _p, 101, 159 - _p) if _p <= 4 else (0, PLUS, 55, 1, 60, 101, 160)])
_BIG = _R(400, 2)
_Q120 = _BIG[100:220]                                           # 120 bases at 101 ... 220
for _k in (1, 3, 20):
    # the query lacks k family bases behind its 60th base: a gap that skips family bases
    _q = _Q120[:60] + _Q120[60 + _k:]
    case("gap", "the query lacks %d family bases" % _k, "%d matches and a gap of %d: %d - 6 - %d = %d, the family span is %d longer" %
         (len(_q), _k, len(_q), _k, len(_q) - 6 - _k, _k), [("FamB", _BIG)], [_q], [(0, PLUS, len(_q) - 6 - _k, 1, len(_q), 101, 220)])
    # the query carries k bases the family lacks, each unlike the family bases around them
    _x = "".join(unlike(_Q120[59], _Q120[60], "ACGT"[j % 4]) for j in range(_k))
    _q = _Q120[:60] + _x + _Q120[60:120 - _k]
    case("gap", "the query carries %d bases more" % _k, "%d matches and a gap of %d on the other side: %d" % (120 - _k, _k, 120 - _k - 6 - _k),
         [("FamB", _BIG)], [_q], [(0, PLUS, 120 - _k - 6 - _k, 1, 120, 101, 220 - _k)])
# gap open against two mismatches: X = 10 units of ACGT, then g = ACTA (two of four differ from a unit), then a tail T.  From family base 1:
# X exact, a gap over g (10), T.  From family base 5: X against X[4:] + g, two mismatches (10), T.  Equal scores: the smaller start.
_X, _G, _T = "ACGT" * 10, "ACTA", _R(40, 3)
case("ties", "gap open against two mismatches at equal score",
     "40 + 40 - 10 = 70 either way; the key decides for the alignment that starts at family base 1 (the gapped one), not for the later start", [("FamC", _X + _G + _T + _R(30, 4))],
     [_X + _T], [(0, PLUS, 70, 1, 80, 1, 84)])
case("strand", "a copy on strand -", "the family holds the reverse complement of the query at 201 ... 260: strand -, the whole query",
     [("FamR", _R(200, 50) + rc(_P) + _R(40, 51))], [_P], [(0, MINUS, 60, 1, 60, 201, 260)], sn={"named": 1, "reverse": 1})
case("strand", "a part of the query on strand -",
     "10 + 40 + 6 bases, the 40 reverse-complemented in the family at 51 ... 90 with unlike bases around them: strand -, and QSTART / QEND are the query's own 11 ... 50",
     [("FamD", _R(50, 5) + rc(_P[:40]) + _R(60, 6))],
     [_R(9, 7) + unlike(_P[0], rc(_R(60, 6))[-1]) + _P[:40] + unlike(_P[39], rc(_R(50, 5))[0]) + _R(5, 8)], [(0, MINUS, 40, 11, 50, 51, 90)])
_PAL = "ACGTTGCAAGGCCTTAATTAAGGCCTTGCAACGT"                        # its own reverse complement
assert rc(_PAL) == _PAL
case("strand", "a reverse-complement palindrome", "both strands align the 34 bases alike: strand + wins", [("FamE", _R(80, 9) + _PAL + _R(80, 10))], [_PAL],
     [(0, PLUS, 34, 1, 34, 81, 114)])
case("ties", "the same piece twice in one family", "at 51 ... 110 and at 201 ... 260: the smaller FSTART", [("FamF", _R(50, 11) + _P + _R(90, 12) + _P + _R(40, 13))], [_P],
     [(0, PLUS, 60, 1, 60, 51, 110)], second=[(0, NONE)])
case("ties", "the same piece in two families", "the smaller index; SECOND is the other family's equal score: ambiguous",
     [("FamG", _R(70, 14)), ("FamH", _R(30, 15) + _P + _R(30, 16)), ("FamI", _R(10, 17) + _P + _R(10, 18))], [_P], [(1, PLUS, 60, 1, 60, 31, 90)], second=[(60, 2)],
     sn={"named": 1, "ambiguous": 1})
case("ties", "the second family on the other strand", "SECOND looks at both strands of the other families", [("FamH", _R(30, 15) + _P + _R(30, 16)), ("FamJ", _R(20, 19) + unlike(rc(_P[45])) + rc(_P[:45]) + _R(20, 20))],
     [_P], [(0, PLUS, 60, 1, 60, 31, 90)], second=[(45, 1)], sn={"named": 1, "ambiguous": 0})
case("named", "a score of exactly A - 1 and of exactly A", "29 and 30 bases of the family at A = 30: unnamed and named",
     _LIB, [_P[:29], _P[:30]], [(0, PLUS, 29, 1, 29, 101, 129), (0, PLUS, 30, 1, 30, 101, 130)], sn={"queries": 2, "named": 1, "unnamed": 1, "pairs_named": 1})
case("named", "no positive cell at all", "A against C and N: no family, score 0", [("FamK", "CCCCNNCCCC"), ("FamL", "GGNGG")], ["AAAAAAAAAAAA"], [(NONE, 0, 0, 0, 0, 0, 0)],
     second=[(0, NONE)], sn={"queries": 1, "named": 0, "unnamed": 1, "pairs_named": 0})

# ------------------------------------------------------------------------------------------- library bases
case("library", "an N inside the copy", "59 matches and one other base: 59 - 1 = 58, the full span", [("FamA", sub(_BG, 130, "N"))], [_P], [(0, PLUS, 58, 1, 60, 101, 160)])
case("library", "IUPAC codes inside the copy", "R and y are not A C G T: 58 - 2 = 56", [("FamA", sub(sub(_BG, 120, "R"), 140, "y"))], [_P], [(0, PLUS, 56, 1, 60, 101, 160)])
case("library", "a lower-case family", "letters map in either case: the exact copy", [("FamA", _BG.lower())], [_P], [(0, PLUS, 60, 1, 60, 101, 160)])
case("library", "a byte that is no letter", "'-' and '*' map to 15 like N", [("FamA", sub(sub(_BG, 120, "-"), 140, "*"))], [_P], [(0, PLUS, 56, 1, 60, 101, 160)])

# ------------------------------------------------------------------------------------------- position, length and block edges
case("edges", "an alignment that begins at a family's first base and one that ends at its last", "1 ... 60 and 241 ... 300", _LIB, [_BG[:60], _BG[240:]],
     [(0, PLUS, 60, 1, 60, 1, 60), (0, PLUS, 60, 1, 60, 241, 300)])
case("edges", "a neighbouring family's bases that would extend it",
     "the first family ends with the first 30 bases of the query, the second begins with the other 30: 30 each, never 60; a family before and behind hold nothing",
     [("FamM", _R(5, 21)), ("FamN", _R(41, 22) + _P[:30]), ("FamO", _P[30:] + _R(37, 23)), ("FamP", _R(7, 24))], [_P], [(1, PLUS, 30, 1, 30, 42, 71)], second=[(30, 2)])
_Q100 = _R(100, 25)
case("edges", "a family of one base", "score 1 at the base's first place in the query, strand +", [("One", _Q100[40])], [_Q100], [(0, PLUS, 1, _Q100.index(_Q100[40]) + 1, _Q100.index(_Q100[40]) + 1, 1, 1)], A=12)
for _n in (FAM_BLOCK - 1, FAM_BLOCK, FAM_BLOCK + 1):
    case("edges", "a family of %d bases inside the query" % _n, "the whole family: score %d" % _n, [("Whole", _R(_n, 26))], [_R(20, 27) + _R(_n, 26) + _R(20, 28)],
         [(0, PLUS, _n, 21, 20 + _n, 1, _n)])
for _n in [b * FAM_BLOCK + d for b in (1, 2, 3, 5) for d in (-1, 0, 1)]:
    _f = _R(_n, 30 + _n)
    case("edges", "a family of %d bases whose last 50 are the query" % _n, "the alignment ends at the family's last base, one base in front of, at and behind a block edge",
         [("Pad", _R(33, 29)), ("Tail", _f)], [_f[-50:]], [(1, PLUS, 50, 1, 50, _n - 49, _n)])
for _e in (FAM_BLOCK, 2 * FAM_BLOCK, 4 * FAM_BLOCK):
    case("edges", "a copy across the block edge at %d" % _e, "50 bases from %d: 25 on either side of the edge" % (_e - 24), [("FamB", _BIG)], [_BIG[_e - 25:_e + 25]],
         [(0, PLUS, 50, 1, 50, _e - 24, _e + 25)])
_F320 = _R(20, 31) + _R(QMAX, 32) + _R(20, 33)
case("lengths", "every query length 1 ... %d" % QMAX, "the first n bases of a piece at 21 ...: score n; from 16 bases on the span too (shorter ones can sit elsewhere as well)",
     [("FamQ", _F320)], [_F320[20:20 + n] for n in range(1, QMAX + 1)],
     [(0, None, n, None, None, None, None) if n < 16 else (0, PLUS, n, 1, n, 21, 20 + n) for n in range(1, QMAX + 1)], A=12,
     sn={"queries": QMAX, "named": QMAX - 11, "unnamed": 11})
# a mismatch, a gap opening and a gap extension at every column offset of a lane: the lanes of a query of n bases hold ceil(n / 64) columns
_EDITS_Q, _EDITS_W = [], []
for _n in (60, 100, 140, 200, 272):
    _c = (_n + 63) // 64
    _piece = _F320[20:20 + _n]
    for _o in range(MAX_COLS):
        _at = (_n // 2 // _c) * _c + _o                           # a column with offset o % c in its lane, in the middle of the query
        _EDITS_Q.append(sub(_piece, _at))
        _EDITS_W.append((0, PLUS, _n - 5, 1, _n, 21, 20 + _n))
        _EDITS_Q.append(_piece[:_at] + _F320[20 + _at + 3:20 + _n + 3])            # three family bases skipped in front of column _at
        _EDITS_W.append((0, PLUS, _n - 9, 1, _n, 21, 23 + _n))
        _ins3 = "".join(unlike(_piece[_at - 1], _piece[_at], "ACGT"[j]) for j in range(3))
        _EDITS_Q.append(_piece[:_at] + _ins3 + _piece[_at:_n - 3])               # three query bases the family lacks, columns _at ... _at + 2
        _EDITS_W.append((0, PLUS, _n - 3 - 9, 1, _n, 21, 17 + _n))
case("lanes", "a mismatch, a gap over the family and a gap over the query at every column offset of a lane", "n - 5, n - 9 and n - 12 for n = 60, 100, 140, 200, 272",
     [("FamQ", _F320)], _EDITS_Q, _EDITS_W)

# ------------------------------------------------------------------------------------------- problems under 40 x 40 (every start cell can be enumerated)
_S40 = _R(40, 60)
case("small", "an exact copy of 20 bases in a family of 30", "at 6 ... 25", [("S", _S40[:30])], [_S40[5:25]], [(0, PLUS, 20, 1, 20, 6, 25)], A=12)
case("small", "12 bases twice in a family of 34", "at 1 ... 12 and at 19 ... 30: the smaller FSTART", [("S", _S40[:12] + "ACGTAC" + _S40[:12] + "TTGA")], [_S40[:12]],
     [(0, PLUS, 12, 1, 12, 1, 12)], A=12)
case("small", "a query of 36 that lacks two family bases", "18 + 18 matches and a gap of 2: 36 - 8 = 28 over family bases 1 ... 38", [("S", _S40)], [_S40[:18] + _S40[20:38]],
     [(0, PLUS, 28, 1, 36, 1, 38)], A=12)
case("small", "16 bases on strand - in a family of 30", "the reverse complement at 8 ... 23", [("S", _R(7, 61) + rc(_S40[:16]) + _R(7, 62))], [_S40[:16]],
     [(0, MINUS, 16, 1, 16, 8, 23)], A=12)

# ------------------------------------------------------------------------------------------- the pair rule
_F1, _F2 = _R(200, 40), _R(200, 41)
_PLIB = [("Alu", _F1), ("L1", _F2)]
_NOISE = _R(40, 42)
case("pairs", "OPEN pairs with agreeing, disagreeing and half-named parts, and a CLOSED one between them",
     "pair 0: both flanks from Alu +: named, the larger score and the union of the spans; pair 1: Alu and L1: a conflict; pair 2 is CLOSED and named; pair 3: one flank "
     "names nothing: named by the other; pair 4: Alu + and Alu -: a conflict; pair 5: nothing named",
     _PLIB, [_F1[10:60], _F1[120:190], _F1[10:60], _F2[100:150], _F2[20:80], _NOISE, _F2[100:140], _F1[10:60], rc(_F1[100:150]), _NOISE[:20], _NOISE[20:]],
     [(0, PLUS, 50, 1, 50, 11, 60), (0, PLUS, 70, 1, 70, 121, 190), (0, PLUS, 50, 1, 50, 11, 60), (1, PLUS, 50, 1, 50, 101, 150), (1, PLUS, 60, 1, 60, 21, 80), None,
      (1, PLUS, 40, 1, 40, 101, 140), (0, PLUS, 50, 1, 50, 11, 60), (0, MINUS, 50, 1, 50, 101, 150), None, None],
     parts=[LEFT, RIGHT, LEFT, RIGHT, SEQ, LEFT, RIGHT, LEFT, RIGHT, LEFT, RIGHT], pairs=[0, 0, 1, 1, 2, 3, 3, 4, 4, 5, 5],
     sn={"queries": 11, "closed_queries": 1, "left_queries": 5, "right_queries": 5, "named": 8, "unnamed": 3, "reverse": 1, "pairs_named": 3, "pairs_conflict": 2},
     calls={0: (0, PLUS, 70, 11, 190), 2: (1, PLUS, 60, 21, 80), 3: (1, PLUS, 40, 101, 140)})
N_AIMED = len(CASES)


# ------------------------------------------------------------------------------------------- generated input
def random_case(n=500, seed=77):
    """500 queries of 20 ... 150 bases cut from a library of three families and 2 kb, on either strand, with random substitutions,
    deletions and insertions; no literal claim"""
    rs = np.random.RandomState(seed)
    lib = [("Ra", seeded(700, 12001)), ("Rb", seeded(600, 12002)), ("Rc", seeded(700, 12003))]
    lib[2] = ("Rc", lib[2][1][:300] + lib[0][1][200:400] + lib[2][1][500:])        # (a stretch two families share: ties between families)
    queries = []
    for _ in range(n):
        t = lib[rs.randint(3)][1]
        ln = int(rs.randint(20, 151))
        at = int(rs.randint(0, len(t) - ln + 1))
        q = list(t[at:at + ln])
        for _ in range(int(rs.randint(0, 6))):
            kind, j = rs.randint(3), int(rs.randint(0, len(q)))
            if kind == 0:
                q[j] = "ACGT"[rs.randint(4)]
            elif kind == 1 and len(q) > 12:
                del q[j:j + int(rs.randint(1, 6))]
            else:
                q[j:j] = list(seeded(int(rs.randint(1, 6)), int(rs.randint(1 << 30))))
        q = "".join(q)[:QMAX]
        queries.append(rc(q) if rs.randint(2) else q)
    return {"family": "random", "name": "random: %d queries cut from a 3-family library of 2 kb, with random edits" % n, "claims": "the definition, the restatement and the device agree",
            "library": lib, "queries": queries, "want": [None] * n, "second": None, "sn": None, "A": 30, "parts": None, "pairs": None, "calls": None}


# ------------------------------------------------------------------------------------------- the job
JOB_A = 30
JOB_LIBRARY = [("AluX", seeded(300, 13001)), ("L1X", seeded(900, 13002)), ("SvaX", seeded(500, 13003))]
# (contig, P_R, TSD, the inserted bases, what the file names: family, strand, FSTART, FEND — None: nothing)
_L1 = JOB_LIBRARY[1][1]
JOB_PLANTED = ((0, 2000, 0, JOB_LIBRARY[0][1][50:180], ("AluX", "+", 51, 180)), (0, 4000, 15, rc(JOB_LIBRARY[2][1][100:230]), ("SvaX", "-", 101, 230)),
               (0, 6000, 0, _L1[300:550], ("L1X", "+", 301, 550)), (0, 8000, 15, rc(_L1[600:850]), ("L1X", "-", 601, 850)),
               (0, 10000, 0, seeded(250, 13004), None), (1, 3000, 0, _L1[100:700], ("L1X", "+", 101, 700)))


def job_genome():
    """two contigs of 12 and 8 kb; no base of homology at either junction of a planted insertion, as in clip_ins_cases.job_genome"""
    g = (Seq(seeded(C.LEN_A, 13010)), Seq(seeded(C.LEN_B, 13011)))
    for t, P, tsd, s, _ in JOB_PLANTED:
        PL = P + 1 - tsd
        if g[t][P + 1] == s[0]:
            g[t].b[P] = other(s[0])
        if g[t][PL - 1] == s[-1]:
            g[t].b[PL - 2] = other(s[-1])
    return g


def job_reads(g):
    """the reads of clip_ins_cases.job_reads over JOB_PLANTED: per junction side one read each with 30, 60, 90 and 120 clipped bases
    and three with 140, and plain reads every 75 bases"""
    reads = []
    for t, P, tsd, s, _ in JOB_PLANTED:
        PL = P + 1 - tsd
        for j, k in enumerate(C.JOB_CLIPS):
            m = C.READ - k
            clip = (s + g[t].get(PL, PL + C.READ))[:k]
            reads.append(D.rd(tid=t, pos=P - m, m=m, trail=clip, seq=g[t].get(P - m + 1, P) + clip, flag=D.REV * (j % 2)))
            clip = (g[t].get(P - C.READ, P) + s)[-k:]
            reads.append(D.rd(tid=t, pos=PL - 1, m=m, lead=clip, seq=clip + g[t].get(PL, PL + m - 1), flag=D.REV * (j % 2)))
    for t, s in enumerate(g):
        for p in range(1, len(s.b) - C.READ, 75):
            reads.append(D.rd(tid=t, pos=p - 1, m=C.READ, seq=s.get(p, p + C.READ - 1), flag=D.REV * (p % 150 == 1)))
    return sorted(reads, key=lambda r: (r["tid"], r["pos"]))


def write_library(path, library=JOB_LIBRARY):
    with open(path, "wb") as f:
        f.write(b"".join(b">" + n.encode() + b"\n" + fasta_raw(t) + b"\n" for n, t in library))
