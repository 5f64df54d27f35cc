"""Aimed cases for the insertion candidates from facing clip sites (tiddit_amd/tiddit_clip_ins.py, csrc/tdt_clip_ins.hip and
clip_ext_keys of csrc/tdt_clip.hip), each with the literal result it claims, written down from what the case PLANTED — never computed by
the definition or by the restatement of tests/test_clip_ins_refs_cpu.py.

KEY cases are reads built byte by byte with ``clip_cases.rd``: the claim (:func:`claimed_keys`) is the extension keys and the four push
counters that follow from the bases planted into each clip.  CONSENSUS cases are reads too, with the sites they claim at a stated
minimum support: ``(tid, P, side, SUPPORT, ECLEN, consensus outward)``.  PAIR and CLOSURE cases are site lists
``(tid, P, side, SUPPORT, consensus outward)`` with the rows they claim: ``(R index, L index, TSD, status, LEN, MISMATCH, CLOSURES,
SEQ)``.  The JOB is a generated reference of two contigs and 20 kb with planted insertions and the sample's reads over them."""
import collections
import os
import re

import numpy as np

import clip_cases as D
from clip_align_cases import Seq, fasta_raw, seeded

COLS, EXT_COLS, MAX_TSD = 28, 140, 32
L_SIDE, R_SIDE = D.L_SIDE, D.R_SIDE
OPEN, CLOSED = 0, 1
PUSH_SN = ("ext_left_events", "ext_right_events", "ext_keys", "cut_beyond_28")
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiddit_amd", "csrc", "tdt_clip.hip")).read()
K_TILE = int(re.search(r"^#define CLIP_K_TILE (\d+)\b", _SRC, re.M).group(1))           # the reads of a clip_ext_keys workgroup
_HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tiddit_hip.h")).read()
MAX_PER_READ = int(re.search(r"^#define TDT_CLIP_EXT_MAX_PER_READ (\d+)\b", _HDR, re.M).group(1))


def codes(text):
    return ["ACGT".index(ch) for ch in text]


def ext_outward(clip, side):
    """what rule 1 keeps of a clip given in read order: outward from the breakpoint, up to the first base that is not A C G T, 140 at most"""
    s = clip[::-1] if side == L_SIDE else clip
    keep = ""
    for ch in s[:EXT_COLS]:
        if ch not in "ACGT":
            break
        keep += ch
    return keep


def XK1(c, tid, P):
    return c * 2 ** 56 + tid * 2 ** 32 + P


# ------------------------------------------------------------------------------------------- key cases
KEY_CASES, CONS_CASES, PAIR_CASES = [], [], []


def key_case(family, name, claims, batches_, Q=20, L=10, capacity=1 << 12):
    bs = [(b, 0) if isinstance(b, list) else b for b in batches_]
    KEY_CASES.append({"family": family, "name": family + ": " + name, "claims": claims, "batches": bs, "Q": Q, "L": L, "capacity": capacity, "S": (1,),
                      "rows": None})


def planted_events(case):
    """-> [(tid, P, side, rev, kept bases outward, cliplen)] of every clip the case planted in a read that is OK and whose clip is an event"""
    out = []
    for reads, _ in case["batches"]:
        for r in reads:
            if r["kind"] != D.OK:
                continue
            rev = 1 if r["flag"] & D.REV else 0
            for side, clip, P in ((L_SIDE, r["lead"], r["pos"] + 1), (R_SIDE, r["trail"], r["pos"] + r["m"])):
                if clip and len(clip) >= case["L"]:
                    out.append((r["tid"], P, side, rev, ext_outward(clip, side), len(clip)))
    return out


def claimed_keys(case):
    """-> (extension keys [(K1, K2)], {push counter: n}) from the planted clips: one key per further chunk of 28 kept bases"""
    keys, sn = [], collections.Counter()
    for tid, P, side, rev, kept, cliplen in planted_events(case):
        sn["cut_beyond_28"] += COLS <= len(kept) < min(cliplen, EXT_COLS)
        if len(kept) > COLS:
            sn["ext_right_events" if side else "ext_left_events"] += 1
        for c in range(1, 5):
            chunk = kept[COLS * c:COLS * (c + 1)]
            if chunk:
                keys.append((XK1(c, tid, P), D.K2(side, chunk, rev)))
    sn["ext_keys"] = len(keys)
    return keys, +sn


def key_definition(case):
    """the definition over the case's batches -> (sorted extension key rows, {push counter: n}, events)"""
    from tiddit_amd import tiddit_clip_ins as I
    events, keys, sn = [], [], {}
    for b in D.batches(case):
        I.events_of_batch_by_read(b, events, keys, sn, case["Q"], case["L"])
    return D.key_rows(keys), sn, events


def key_agrees_with_claim(case, rows, sn):
    keys, want = claimed_keys(case)
    if not np.array_equal(rows, D.key_rows(keys)):
        return "keys"
    if dict(sn) != dict(want):
        return "push counters %s / %s" % (dict(sn), dict(want))
    return None


_R = lambda n, seed: seeded(n, 7000 + seed)
_N = lambda clip, j, side: (clip[:len(clip) - 1 - j] + "N" + clip[len(clip) - j:]) if side == L_SIDE else clip[:j] + "N" + clip[j + 1:]
LENGTHS = (28, 29, 55, 56, 57, 84, 85, 112, 113, 139, 140, 141, 150)
key_case("length", "clips of 28 ... 150 bases on both sides",
         "28 bases give no key; 29 one key of 1 base; 56 one full chunk, 57 a second of 1 base; ... 140, 141 and 150 four full chunks: the 141st base is not "
         "stored and nothing is cut",
         [[D.rd(pos=1000 + 10 * k, lead=_R(n, k)) for k, n in enumerate(LENGTHS)] + [D.rd(pos=2000 + 10 * k, trail=_R(n, 50 + k), flag=D.REV) for k, n in enumerate(LENGTHS)]])
key_case("phase", "extension chunks starting on an even and on an odd query index, on both sides",
         "a leading clip is read backwards from query index cliplen - 1 (chunk 1 starts at cliplen - 29: odd for 60, even for 61 bases); a trailing clip "
         "forwards (chunk 1 at l_seq - cliplen + 28: even and odd with m = 20 and 21)",
         [[D.rd(pos=100, lead=_R(60, 1)), D.rd(pos=150, lead=_R(61, 2)), D.rd(pos=200, m=20, trail=_R(60, 3)), D.rd(pos=200, m=21, trail=_R(60, 4)),
           D.rd(pos=300, lead=_R(90, 5), m=21, trail=_R(91, 6), flag=D.REV)]])
key_case("hard", "H outside the S on both sides",
         "an S behind a leading H and in front of a trailing H is the clip and is extended like any other; H alone gives nothing",
         [[D.rd(pos=100, hl=5, lead=_R(70, 7)), D.rd(pos=100, trail=_R(71, 8), ht=7), D.rd(pos=100, hl=3, lead=_R(100, 9), trail=_R(45, 10), ht=4), D.rd(pos=100, hl=30)]])
key_case("other", "a base that is not A C G T at columns 27, 28, 29, 55, 56 and 139",
         "column 27: no key (the first chunk is not full; the cut is the base store's, not counted here); 28: no key, cut_beyond_28; 29: a key of 1 base; "
         "55: a key of 27; 56: one full key and no second; 139: three full keys and one of 27; all but the first are cut_beyond_28; on both sides",
         [[D.rd(pos=100 + j, lead=_N(_R(150, 11), j, L_SIDE)) for j in (27, 28, 29, 55, 56, 139)] +
          [D.rd(pos=400 + j, trail=_N(_R(150, 12), j, R_SIDE), flag=D.REV) for j in (27, 28, 29, 55, 56, 139)]])
key_case("both", "a read with two clips of 140 bases or more",
         "S M S with 140 and 150 clipped bases: four keys per clip, eight for the read",
         [[D.rd(pos=100, lead=_R(140, 13), trail=_R(150, 14)), D.rd(pos=100, lead=_R(9, 15), trail=_R(141, 16)), D.rd(pos=100, lead=_R(30, 17), trail=_R(8, 18))]])
_bad = lambda **kw: D.rd(kind=D.MALFORMED, **kw)
key_case("malformed", "malformed, unsequenced, unaligned and filtered reads with long clips",
         "an op code of 9, tid = 2^24, pos = -1, a query length that differs from l_seq, a body beyond block_size, a CIGAR of S alone, a MAPQ below Q, a "
         "duplicate: none gives a key or is counted; one well-formed read among them gives two",
         [[_bad(pos=100, lead=_R(90, 19), patch=((D.cig_at(1), "<I", 20 << 4 | 9),)), _bad(tid=2 ** 24, pos=100, lead=_R(90, 20)), _bad(pos=-1, lead=_R(90, 21)),
           _bad(pos=100, lead=_R(90, 22), patch=((D.cig_at(0), "<I", 91 << 4 | 4),)), _bad(pos=100, lead=_R(90, 23), bs_delta=-1),
           D.rd(pos=100, ops=[(4, 90)], seq=_R(90, 24), kind=D.NO_ALIGNMENT), D.rd(pos=100, lead=_R(90, 25), mapq=19, kind=D.NOT_ELIGIBLE),
           D.rd(pos=100, lead=_R(90, 26), flag=0x400, kind=D.NOT_ELIGIBLE), D.rd(pos=100, lead=_R(80, 27))]])
key_case("malformed", "a block that reaches beyond the raw bytes",
         "the last record's block ends one byte behind raw_len: it is malformed and gives nothing, the read in front of it gives its keys",
         [([D.rd(pos=100, trail=_R(100, 28)), _bad(pos=100, trail=_R(100, 29))], 1)])
key_case("length", "L above 28", "with L = 100 a clip of 99 bases is short and gives no key, one of 100 gives three",
         [[D.rd(pos=100, lead=_R(99, 30)), D.rd(pos=100, trail=_R(100, 31))]], L=100)
key_case("store", "%d reads with one long clip each" % (K_TILE + 1),
         "two workgroups, the second with a single read; every seventh read is below the MAPQ cut, so the compaction moves the reads behind it; clip "
         "lengths 20 ... 150, so reads with 0, 1, 2, 3 and 4 keys lie side by side in the stage",
         [[D.rd(pos=2000 + 3 * (k % 50), lead=_R(20 + (k * 37) % 131, k) if k % 2 else "", trail="" if k % 2 else _R(20 + (k * 41) % 131, k), flag=D.REV * (k % 3 == 0),
                mapq=3 if k % 7 == 3 else 60, kind=D.NOT_ELIGIBLE if k % 7 == 3 else D.OK) for k in range(K_TILE + 1)]])
key_case("store", "every read of a tile gives %d keys" % MAX_PER_READ,
         "%d reads with two clips of 140 bases: the LDS stage of the workgroup is full, and the store, made for exactly that many keys, is full too" % K_TILE,
         [[D.rd(pos=3000 + k % 20, lead=_R(140, k % 5), trail=_R(140, 100 + k % 7), flag=D.REV * (k & 1)) for k in range(K_TILE)]], capacity=MAX_PER_READ * K_TILE)
_many = [D.rd(tid=k % 3, pos=1000 + 7 * (k % 41), lead=_R(10 + (k * 29) % 140, k % 9) if k % 3 else "", trail=_R(10 + (k * 31) % 140, 20 + k % 8) if k % 2 else "",
              flag=D.REV if k % 5 == 0 else 0, mapq=19 + k % 4, kind=D.OK if k % 4 else D.NOT_ELIGIBLE) for k in range(300)]
key_case("store", "300 reads in three pushes, a store made for 64 keys",
         "20 reads need 160 slots of a store of 64 (it grows), the next 220 need 1760 more (it grows again), the last 60 fit behind the real count",
         [_many[:20], _many[20:240], _many[240:]], capacity=64)
N_KEY_CASES = len(KEY_CASES)


# ------------------------------------------------------------------------------------------- consensus cases
def cons_case(name, claims, reads, S, sites, L=10):
    CONS_CASES.append({"family": "consensus", "name": "consensus: " + name, "claims": claims, "batches": [(reads, 0)], "Q": 20, "L": L, "S": (S,), "min_support": S,
                       "capacity": 1 << 12, "sites": sites, "rows": None})


_X = _R(150, 40)
for _c in (28, 29, 56, 57):
    cons_case("the depth falls below S at column %d" % _c,
              "three reads at S = 3: two keep 140 bases, one keeps %d: ECLEN = %d; at S = 2 it is 140" % (_c, _c),
              [D.rd(pos=100, trail=_X), D.rd(pos=100, trail=_X, flag=D.REV), D.rd(pos=100, trail=_X[:_c])], 3, [(0, 120, R_SIDE, 3, _c, _X[:_c])])
    cons_case("the depth falls below S at column %d, left side" % _c, "the same on the L side: the columns are counted from the clip's LAST base",
              [D.rd(pos=100, lead=_X), D.rd(pos=100, lead=_X, flag=D.REV), D.rd(pos=100, lead=_X[150 - _c:])], 3, [(0, 101, L_SIDE, 3, _c, _X[::-1][:_c])])
cons_case("S = 2 reaches all 140 columns", "the same three reads at S = 2: two reads reach column 139",
          [D.rd(pos=100, trail=_X), D.rd(pos=100, trail=_X, flag=D.REV), D.rd(pos=100, trail=_X[:29])], 2, [(0, 120, R_SIDE, 3, 140, _X[:140])])
_T = _R(100, 41)
_sub = lambda s, j, ch: s[:j] + ch + s[j + 1:]
cons_case("ties in extension chunks",
          "four reads: at columns 30 and 90 two carry A/C and two carry G/T: the smaller code wins (A at 30, G at 90); at column 60 three carry T and one C",
          [D.rd(pos=100, trail=_sub(_sub(_sub(_T, 30, "A"), 90, "T"), 60, "T")), D.rd(pos=100, trail=_sub(_sub(_sub(_T, 30, "C"), 90, "G"), 60, "T")),
           D.rd(pos=100, trail=_sub(_sub(_sub(_T, 30, "C"), 90, "T"), 60, "C")), D.rd(pos=100, trail=_sub(_sub(_sub(_T, 30, "A"), 90, "G"), 60, "T"))], 4,
          [(0, 120, R_SIDE, 4, 100, _sub(_sub(_sub(_T, 30, "A"), 90, "G"), 60, "T"))])
cons_case("a site whose chunk 1 has less than S support",
          "one read keeps 28 bases (its column 28 is an N) and two keep more: at S = 3 chunk 1 has two events, no row, ECLEN = 28; "
          "a second site with SUPPORT 2 is not reported at all",
          [D.rd(pos=100, trail=_X[:100]), D.rd(pos=100, trail=_X[:90]), D.rd(pos=100, trail=_N(_X[:80], 28, R_SIDE)), D.rd(pos=300, trail=_X[:100]),
           D.rd(pos=300, trail=_X[:100])], 3, [(0, 120, R_SIDE, 3, 28, _X[:28])])
cons_case("a chunk with a row but a short CLEN ends the consensus",
          "three reads keep 100, 100 and 40 bases, a fourth 130: at S = 3 columns 0 ... 39 have depth 4, 40 ... 99 depth 3, 100 ... 129 depth 1: ECLEN = 100, and "
          "chunk 4's single event is not looked at",
          [D.rd(pos=100, trail=_X[:100]), D.rd(pos=100, trail=_X[:100]), D.rd(pos=100, trail=_X[:40]), D.rd(pos=100, trail=_X[:130])], 3,
          [(0, 120, R_SIDE, 4, 100, _X[:100])])


def cons_definition(case):
    from tiddit_amd import tiddit_clip_ins as I
    _, _, events = key_definition(case)
    return I.extended_sites(events, case["min_support"])


def literal_sites(case):
    return [(D.K1(tid, P), side, sup, eclen, codes(cons)) for tid, P, side, sup, eclen, cons in case["sites"]]


# ------------------------------------------------------------------------------------------- pair and closure cases
def pair_case(family, name, claims, sites, rows, K=20, O=12, M=1):
    PAIR_CASES.append({"family": family, "name": family + ": " + name, "claims": claims, "sites": sites, "rows": rows, "K": K, "O": O, "M": M})


def sites_of(case):
    """-> [(K1, side, SUPPORT, ECLEN, codes)] ascending by (K1, side), as the definition's extended_sites gives them"""
    s = [(D.K1(tid, P), side, sup, len(cons), codes(cons)) for tid, P, side, sup, cons in case["sites"]]
    assert s == sorted(s, key=lambda x: (x[0], x[1])), case["name"]
    return s


def literal_rows(case):
    return [(r, l, tsd, status, ln, mm, closures, codes(seq)) for r, l, tsd, status, ln, mm, closures, seq in case["rows"]]


def flanks(ins, a, b):
    """an insertion's two consensus: x = its first a bases, y = its last b bases outward (reversed)"""
    return ins[:a], ins[::-1][:b]


_I60 = _R(60, 60)
_x, _y = flanks(_I60, 40, 40)
for _d in (0, 1, 32, 33):
    pair_case("pairs", "d = %d" % _d,
              "an R site at 1000 and an L site at %d: TSD %d%s" % (1001 - _d, _d, "" if _d <= 32 else " is beyond the 32 bases: no pair"),
              sorted([(0, 1000, R_SIDE, 5, _x), (0, 1001 - _d, L_SIDE, 4, _y)], key=lambda s: (s[1], s[2])),
              [] if _d == 33 else [(0 if _d == 0 else 1, 1 if _d == 0 else 0, _d, CLOSED, 60, 0, 1, _I60)])
pair_case("pairs", "L at P_R + 2", "an L site two bases right of the R site is a deletion with an insertion: not a pair here",
          [(0, 1000, R_SIDE, 5, _x), (0, 1002, L_SIDE, 4, _y)], [])
pair_case("pairs", "equal positions on neighbouring contigs",
          "the R site at (0, 1000) and the L site at (1, 1001), and the R site at (1, 2^32 - 1) whose P_R + 1 is no position: no pair; (1, 1000) R "
          "with (1, 1001) L is one",
          [(0, 1000, R_SIDE, 5, _x), (1, 1000, R_SIDE, 5, _x), (1, 1001, L_SIDE, 4, _y), (1, 2 ** 32 - 1, R_SIDE, 3, _x), (2, 0, L_SIDE, 3, _y)],
          [(1, 2, 0, CLOSED, 60, 0, 1, _I60)])
_I70 = _R(70, 61)
_x2, _y2 = flanks(_I70, 45, 45)
pair_case("pairs", "two L sites for one R, two R sites for one L",
          "R at 1000 faces L at 990 and at 1001 (rows ascend by P_L); R at 1000 and R at 995 both face L at 990: the R consensus of the first insertion "
          "does not close with the L consensus of the second, which is OPEN",
          [(0, 990, L_SIDE, 3, _y2), (0, 995, R_SIDE, 3, _x2), (0, 1000, R_SIDE, 5, _x), (0, 1001, L_SIDE, 4, _y)],
          [(1, 0, 6, CLOSED, 70, 0, 1, _I70), (2, 0, 11, OPEN, 0, 0, 0, ""), (2, 3, 0, CLOSED, 60, 0, 1, _I60)])
pair_case("pairs", "a side with ECLEN = K - 1",
          "with K = 40 an L site of 39 columns is no partner and an R site of 39 columns has no row; the pair of 40 and 40 is one",
          [(0, 1000, R_SIDE, 5, _x), (0, 1001, L_SIDE, 4, _y[:39]), (0, 2000, R_SIDE, 5, _x[:39]), (0, 2001, L_SIDE, 4, _y), (0, 3000, R_SIDE, 5, _x),
           (0, 3001, L_SIDE, 4, _y)], [(4, 5, 0, CLOSED, 60, 0, 1, _I60)], K=40)
pair_case("pairs", "the rows in front of an R site that are full of sites",
          "an L and an R site at every position 969 ... 1000 (64 rows): the R site at 1000 faces the 32 L sites at 969 ... 1000 (TSD 32 ... 1) and the one "
          "at 1001 (TSD 0); all OPEN (their consensus are one base repeated, of another base each side)",
          [(0, p, s, 3, ("A" if s == R_SIDE else "C") * 30) for p in range(969, 1001) for s in (L_SIDE, R_SIDE)] + [(0, 1001, L_SIDE, 3, "C" * 30)],
          sorted([(2 * (pr - 969) + 1, 2 * (pl - 969), pr + 1 - pl, OPEN, 0, 0, 0, "") for pr in range(969, 1001) for pl in range(969, 1002) if 0 <= pr + 1 - pl <= 32]))

# closure: l at the edges of the candidate range, of the shorter and of the longer consensus
_A, _B, _O = 50, 70, 12
for _l, _what in ((_O - 1, "O - 1"), (_O, "O"), (_A - 1, "min(a, b) - 1"), (_A + 1, "min(a, b) + 1"), (_B - 1, "max(a, b) - 1"), (_B + 1, "max(a, b) + 1"),
                  (_A + _B - _O, "a + b - O"), (_A + _B - _O + 1, "a + b - O + 1")):
    _ins = _R(_l, 70 + _l)
    _open = _l < _O or _l > _A + _B - _O
    # (an insertion shorter than a consensus: the consensus runs on into the reference behind it, here bases unlike anything else)
    _xx = (_ins + _R(200, 300 + _l))[:_A]
    _yy = (_ins[::-1] + _R(200, 500 + _l))[:_B]
    pair_case("closure", "l = %s = %d with a = %d, b = %d" % (_what, _l, _A, _B),
              "the overlap is min(a, l) - max(0, l - b) = %d columns: %s" % (min(_A, _l) - max(0, _l - _B), "no candidate, OPEN" if _open else "CLOSED, SEQ is the insertion"),
              [(0, 1000, R_SIDE, 3, _xx), (0, 1001, L_SIDE, 3, _yy)], [(0, 1, 0, OPEN, 0, 0, 0, "") if _open else (0, 1, 0, CLOSED, _l, 0, 1, _ins)])
    pair_case("closure", "l = %s = %d with a = %d, b = %d" % (_what, _l, _B, _A), "the same with the longer consensus on the R side",
              [(0, 1000, R_SIDE, 3, (_ins + _R(200, 300 + _l))[:_B]), (0, 1001, L_SIDE, 3, (_ins[::-1] + _R(200, 500 + _l))[:_A])],
              [(0, 1, 0, OPEN, 0, 0, 0, "") if _open else (0, 1, 0, CLOSED, _l, 0, 1, _ins)])
_I90 = _R(90, 80)
_x3, _y3 = flanks(_I90, 60, 60)                                  # the overlap is x[30:60]
_mut = lambda s, at: "".join(("ACGT"[("ACGT".index(ch) + 1) % 4] if j in at else ch) for j, ch in enumerate(s))
pair_case("closure", "mm = M", "two of the 30 overlapping columns differ, M = 2: CLOSED with MISMATCH 2; SEQ takes the R consensus up to min(a, l)",
          [(0, 1000, R_SIDE, 3, _mut(_x3, (35, 50))), (0, 1001, L_SIDE, 3, _y3)], [(0, 1, 0, CLOSED, 90, 2, 1, _mut(_I90, (35, 50)))], M=2)
pair_case("closure", "mm = M + 1", "three differ, M = 2: OPEN", [(0, 1000, R_SIDE, 3, _mut(_x3, (35, 50, 59))), (0, 1001, L_SIDE, 3, _y3)],
          [(0, 1, 0, OPEN, 0, 0, 0, "")], M=2)
pair_case("closure", "M = 0 and one mismatch at the overlap's last column", "a mismatch at column 59 of x, the overlap's last: OPEN at M = 0",
          [(0, 1000, R_SIDE, 3, _mut(_x3, (59,))), (0, 1001, L_SIDE, 3, _y3)], [(0, 1, 0, OPEN, 0, 0, 0, "")], M=0)
pair_case("closure", "the overlap's first column", "a mismatch at column 30 of x, the overlap's first: CLOSED with MISMATCH 1 at M = 1",
          [(0, 1000, R_SIDE, 3, _mut(_x3, (30,))), (0, 1001, L_SIDE, 3, _y3)], [(0, 1, 0, CLOSED, 90, 1, 1, _mut(_I90, (30,)))], M=1)
pair_case("closure", "a mismatch outside the overlap does not count", "column 29 of x lies in front of the overlap: MISMATCH 0, and SEQ carries it",
          [(0, 1000, R_SIDE, 3, _mut(_x3, (29,))), (0, 1001, L_SIDE, 3, _y3)], [(0, 1, 0, CLOSED, 90, 0, 1, _mut(_I90, (29,)))], M=0)
_U = "ACGGT"                                                     # a periodic insertion: 16 copies of a unit of 5
_P80 = _U * 16
_xp, _yp = flanks(_P80, 50, 50)
pair_case("closure", "a periodic insertion with several closures",
          "80 bases of a 5-base unit, a = b = 50, O = 12, M = 0: every l = 80 - 5 k with an overlap of 12 or more closes without a mismatch: l = 15, 20, ... 85 "
          "(15 closures); the best is the smallest, 15, whose SEQ is three units",
          [(0, 1000, R_SIDE, 3, _xp), (0, 1001, L_SIDE, 3, _yp)], [(0, 1, 0, CLOSED, 15, 0, 15, _U * 3)], M=0)
pair_case("closure", "O above the shorter consensus", "a = 20, b = 140, O = 30: no l has 30 overlapping columns: OPEN",
          [(0, 1000, R_SIDE, 3, _R(140, 81)[:20]), (0, 1001, L_SIDE, 3, _R(140, 81)[::-1])], [(0, 1, 0, OPEN, 0, 0, 0, "")], O=30)
_I250 = _R(250, 82)
pair_case("closure", "250 bases from two consensus of 140",
          "the overlap is 30 columns; SEQ has 250 bases, nine words of 28",
          [(0, 1000, R_SIDE, 3, _I250[:140]), (0, 1001, L_SIDE, 3, _I250[::-1][:140])], [(0, 1, 0, CLOSED, 250, 0, 1, _I250)])
N_PAIR_CASES = len(PAIR_CASES)


def every_length_case(O=12):
    """every l from O to 268 at a = b = 140, one pair per l on its own contig position: every word phase of the shift occurs"""
    sites, rows = [], []
    for k, l in enumerate(range(O, 2 * EXT_COLS - O + 1)):
        ins = seeded(l, 9000 + l)
        x = (ins + seeded(200, 9500 + l))[:EXT_COLS]
        y = (ins[::-1] + seeded(200, 9800 + l))[:EXT_COLS]
        sites += [(0, 1000 + 100 * k, R_SIDE, 3, x), (0, 1001 + 100 * k, L_SIDE, 3, y)]
        rows.append((2 * k, 2 * k + 1, 0, CLOSED, l, 0, 1, ins))
    return {"family": "closure", "name": "closure: every l from %d to %d at a = b = 140" % (O, 2 * EXT_COLS - O), "sites": sites, "rows": rows, "K": 20, "O": O, "M": 0,
            "claims": "each pair closes at its own l and nowhere else"}


def pair_definition(case):
    from tiddit_amd import tiddit_clip_ins as I
    return I.pairs_of_sites(sites_of(case), case["K"], case["O"], case["M"])


def pair_agrees_with_claim(case, counts, rows):
    want = literal_rows(case)
    if [tuple(r) for r in rows] != want:
        return "rows %s / %s" % ([r[:7] for r in rows][:6], [r[:7] for r in want][:6])
    s = sites_of(case)
    expect = {"sites_extended": sum(1 for x in s if x[3] > COLS), "left_sites": sum(1 for x in s if x[1] == L_SIDE and x[3] >= case["K"]),
              "right_sites": sum(1 for x in s if x[1] == R_SIDE and x[3] >= case["K"]), "pairs": len(want), "closed": sum(1 for r in want if r[3] == CLOSED),
              "open": sum(1 for r in want if r[3] == OPEN), "closed_multi": sum(1 for r in want if r[6] > 1)}
    from tiddit_amd import tiddit_clip_ins as I
    got = {k: int(counts[I.SN_INDEX[k]]) for k in expect}
    return None if got == expect else "counters %s / %s" % (got, expect)


# ------------------------------------------------------------------------------------------- the job
READ, JOB_S, JOB_Q, JOB_L, JOB_K, JOB_O, JOB_M = 150, 3, 20, 10, 20, 12, 1
CLIPS, INS = "%d:%d:%d" % (JOB_S, JOB_Q, JOB_L), "%d:%d:%d" % (JOB_K, JOB_O, JOB_M)
LEN_A, LEN_B = 12000, 8000
JOB_CLIPS = (30, 60, 90, 120, 140, 140, 140)                     # the clipped bases of the reads over each side of a junction
# (contig, P_R, TSD, inserted bases): the sample carries the insertion behind base P_R, and the TSD bases up to P_R a second time behind it
PLANTED = ((0, 2000, 0, 60), (0, 4000, 15, 60), (0, 6000, 0, 130), (0, 8000, 15, 130), (0, 10000, 0, 250), (1, 2000, 15, 250), (1, 5000, 0, 600))


def job_genome():
    g = (Seq(seeded(LEN_A, 921)), Seq(seeded(LEN_B, 922)))
    ins = [seeded(n, 930 + k) for k, (_, _, _, n) in enumerate(PLANTED)]
    for (t, P, tsd, _), s in zip(PLANTED, ins):
        # no base of homology at either junction: an aligner clips exactly there (the insertion's first base differs from the reference base behind
        # P_R, its last from the base in front of P_L)
        PL = P + 1 - tsd
        if g[t][P + 1] == s[0]:
            g[t].b[P] = "ACGT"[("ACGT".index(s[0]) + 1) % 4]
        if g[t][PL - 1] == s[-1]:
            g[t].b[PL - 2] = "ACGT"[("ACGT".index(s[-1]) + 1) % 4]
    return g, ins


def job_reads(g, ins):
    """150-bp reads over both junctions of every planted insertion, clipped where the sample leaves the reference: per side one read
    each with 30, 60, 90 and 120 clipped bases and three with 140 (so S = 3 reads reach all 140 columns), and plain reads every 75
    bases of both contigs"""
    reads = []
    for (t, P, tsd, n), s in zip(PLANTED, ins):
        PL = P + 1 - tsd
        # the sample around the insertion: ... ref[.. P] + s + ref[PL ..] ...
        for j, k in enumerate(JOB_CLIPS):
            m = READ - k
            clip = (s + g[t].get(PL, PL + READ))[:k]                # a read that ends k bases into the insertion (or through it)
            reads.append(D.rd(tid=t, pos=P - m, m=m, trail=clip, seq=g[t].get(P - m + 1, P) + clip, flag=D.REV * (j % 2)))
            clip = (g[t].get(P - READ, P) + s)[-k:]                 # a read that starts k bases in front of the insertion's end
            reads.append(D.rd(tid=t, pos=PL - 1, m=m, lead=clip, seq=clip + g[t].get(PL, PL + m - 1), flag=D.REV * (j % 2)))
    for t, s in enumerate(g):
        for p in range(1, len(s.b) - READ, 75):
            reads.append(D.rd(tid=t, pos=p - 1, m=READ, seq=s.get(p, p + READ - 1), flag=D.REV * (p % 150 == 1)))
    return sorted(reads, key=lambda r: (r["tid"], r["pos"]))


def job_expected_rows(ins):
    """the planted rows as the file holds them: [CHROM, POS, END, TSD, STATUS, LEN, SEQ] (the 600-base one OPEN)"""
    out = []
    for (t, P, tsd, n), s in zip(PLANTED, ins):
        closed = n <= 2 * EXT_COLS - JOB_O
        out.append(["chr" + "AB"[t], str(P), str(P + 1 - tsd), str(tsd), "CLOSED" if closed else "OPEN", str(n) if closed else ".", s if closed else "."])
    return out
