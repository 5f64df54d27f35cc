"""Aimed cases for the realignment of clip-site consensus (tiddit_amd/tiddit_clip_align.py, csrc/tdt_clip_align.hip): designed references
of at most a few thousand bases over two or three contigs (so that contig offsets and guards matter) and clip sites whose consensus is
cut from them, each with the claim it makes, written down from what the case PLANTED (which bases were copied from where, which event
was cut into the sample) — never computed by the definition or by the restatement of tests/test_clip_align_refs_cpu.py.

A case is a dict: ``contigs`` (the reference: one string of letters per contig, None for a contig that is not loaded), ``lengths``,
``sites`` (see :func:`site`), ``W`` / ``K`` / ``M``, ``family``, ``claims`` (a sentence).  A site's ``claim`` is a dict with any of
``status partner strand mm hits`` (the five columns of the device) and ``type len mate hom`` (of the definition's summarise; ``type``
None: unaligned) — only what the case planted is claimed.  Positions are 1-based, as in the definition."""
import os
import re

import numpy as np

from tiddit_amd import refseq

L_SIDE, R_SIDE = 0, 1
SHORT, OFF, SEARCHED = 0, 1, 2
NO_MM = 0xffffffff
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiddit_amd", "csrc", "tdt_clip_align.hip")).read()


def _define(name):
    """a number from the `#define` lines of csrc/tdt_clip_align.hip: the cases stay on the kernel's edges when it is retuned"""
    return int(re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+([0-9]+)[ \t]*(?://[^\n]*)?$" % name, _SRC, re.M).group(1))


CA_BLOCK, CA_STRIDE, CA_GRID = _define("CA_BLOCK"), _define("CA_STRIDE"), _define("CA_GRID")


def seeded(n, seed):
    """n bases from a seeded generator"""
    return "".join("ACGT"[i] for i in np.random.RandomState(seed).randint(0, 4, n))


def rc(s):
    return s.translate(_COMP)[::-1]


def other(ch):
    """a base that differs from ``ch``"""
    return "ACGT"[("ACGT".index(ch.upper()) + 1) % 4]


class Seq:
    """a contig under construction, addressed 1-based and inclusive as the definition does"""

    def __init__(self, text):
        self.b = list(text)

    def __getitem__(self, q):
        return self.b[q - 1]

    def get(self, lo, hi):
        return "".join(self.b[lo - 1:hi])

    def down(self, hi, n):
        """n bases descending from ``hi``: what an L site's columns hold when its clip continues at ``hi``"""
        return "".join(self.b[hi - n:hi])[::-1]

    def put(self, lo, text):
        self.b[lo - 1:lo - 1 + len(text)] = list(text)

    def differ(self, q, from_q):
        """make base q differ from base from_q (so that an aligner's extension stops there)"""
        if self[q].upper() == self[from_q].upper():
            self.b[q - 1] = other(self[from_q])

    def text(self):
        return "".join(self.b)


def pack(bases):
    """columns outward from the breakpoint -> the packed consensus of a clip row"""
    return sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(bases))


def site(tid, P, side, bases, **claim):
    """a clip site: ``bases`` = its consensus columns OUTWARD from the breakpoint (CLEN = their number)"""
    return {"tid": tid, "P": P, "side": side, "clen": len(bases), "cons": pack(bases), "bases": bases, "claim": claim}


CASES = []


def case(family, name, claims, contigs, sites, W, K=20, M=2, lengths=None):
    CASES.append({"family": family, "name": family + ": " + name, "claims": claims, "contigs": [c.text() if isinstance(c, Seq) else c for c in contigs],
                  "sites": sites, "W": W, "K": K, "M": M,
                  "lengths": lengths or [len(c.text() if isinstance(c, Seq) else c) for c in contigs]})


def host_reference(c):
    return refseq.HostReference({t: refseq.codes_of_bases(s) for t, s in enumerate(c["contigs"]) if s is not None})


def fasta_raw(text, linebases=60, eol=b"\n"):
    """a contig's bytes as a FASTA file holds them (no line end behind the last base)"""
    return eol.join(text[i:i + linebases].encode() for i in range(0, len(text), linebases))


def columns(c):
    """the four site columns as tdt_clip_rows gives them"""
    s = c["sites"]
    return (np.array([(x["tid"] << 32) | x["P"] for x in s], dtype=np.uint64), np.array([x["side"] for x in s], dtype=np.uint32),
            np.array([x["clen"] for x in s], dtype=np.uint32), np.array([x["cons"] for x in s], dtype=np.uint64))


def definition(c):
    """the definition over the case -> (placed: [(status, PARTNER, strand, mm, HITS)], counters, rows of summarise)"""
    from tiddit_amd import tiddit_clip_align as A
    ref = host_reference(c)
    placed = [A.place_site(ref, x["tid"], x["P"], x["side"], x["clen"], x["cons"], c["W"], c["K"], c["M"]) for x in c["sites"]]
    counts, rows = A.summarise([((x["tid"] << 32) | x["P"], x["side"], 3, x["clen"]) for x in c["sites"]], placed, c["M"])
    return placed, counts, rows


def agrees_with_claim(c, placed, rows):
    """``placed`` / ``rows`` (of the definition, of the restatement, of the device + summarise) against the claims -> None or what differs"""
    searched = iter(rows)
    for i, (x, p) in enumerate(zip(c["sites"], placed)):
        row = next(searched) if p[0] == SEARCHED else None
        for k, v in x["claim"].items():
            if k in ("status", "partner", "strand", "mm", "hits"):
                got = p[("status", "partner", "strand", "mm", "hits").index(k)]
            else:
                got = None if row is None else row[{"type": 9, "len": 10, "mate": 11, "hom": 12}[k]]
            if got != v:
                return "site %d (%s %d): %s is %r, claimed %r" % (i, "LR"[x["side"]], x["P"], k, got, v)
    return None


# ---- 1. events: a sample with one planted event; the two junction sites as an aligner clips the reads over them
HOMS = (0, 1, 5, 28)
for _h in HOMS:
    # a deletion of bases a + 1 ... b (D = b - a) whose first h bases equal the h bases behind it
    _g, _a, _b = Seq(seeded(1200, 100 + _h)), 400, 600
    _g.put(_a + 1, _g.get(_b + 1, _b + _h))
    _g.differ(_a, _b)                                  # (the right-anchored read cannot extend to the left)
    _g.differ(_a + _h + 1, _b + _h + 1)                # (the left-anchored read stops behind the homology)
    case("events", "a 200-bp deletion with %d bases of microhomology" % _h,
         "the left-anchored reads align through the homology to a + h and clip G[b + h + 1 ...]: R, PARTNER b + h + 1, DEL 200; the right-anchored "
         "reads start at b + 1 and clip G[a], G[a - 1] ...: L, PARTNER a, DEL 200; the two are mates with HOM h",
         [seeded(37, 1), _g], [site(1, _a + _h, R_SIDE, _g.get(_b + _h + 1, _b + _h + 28), partner=_b + _h + 1, strand=0, mm=0, hits=1, type="DEL", len=200, mate=_b + 1, hom=_h),
                               site(1, _b + 1, L_SIDE, _g.down(_a, 28), partner=_a, strand=0, mm=0, hits=1, type="DEL", len=200, mate=_a + _h, hom=_h)], W=300)
    # a tandem duplication of a ... b (D = b - a + 1) whose first h bases also follow it
    _g, _a, _b = Seq(seeded(1200, 200 + _h)), 400, 599
    _g.put(_b + 1, _g.get(_a, _a + _h - 1))
    _g.differ(_b + _h + 1, _a + _h)
    _g.differ(_a - 1, _b)
    case("events", "a 200-bp tandem duplication with %d bases of microhomology" % _h,
         "the left-anchored reads end at b + h and clip G[a + h ...]: R, PARTNER a + h, DUP 200; the right-anchored reads start at a and clip G[b], "
         "G[b - 1] ...: L, PARTNER b, DUP 200; mates with HOM h",
         [seeded(37, 1), _g], [site(1, _b + _h, R_SIDE, _g.get(_a + _h, _a + _h + 27), partner=_a + _h, strand=0, mm=0, hits=1, type="DUP", len=200, mate=_a, hom=_h),
                               site(1, _a, L_SIDE, _g.down(_b, 28), partner=_b, strand=0, mm=0, hits=1, type="DUP", len=200, mate=_b + _h, hom=_h)], W=300)
    # an inversion of a ... b (D = b - a + 1) whose first h bases are the reverse complement of its last h
    _g, _a, _b = Seq(seeded(1200, 300 + _h)), 400, 599
    _g.put(_a, rc(_g.get(_b - _h + 1, _b)))
    if _g[_a + _h] == rc(_g[_b - _h]):                 # (both extensions stop behind the inverted repeat)
        _g.put(_a + _h, other(_g[_a + _h]))
    case("events", "a 200-bp inversion whose ends are an inverted repeat of %d bases" % _h,
         "the left-anchored reads align through the repeat to a - 1 + h and clip the complement of G[b - h], G[b - h - 1] ...: R, reverse, PARTNER "
         "b - h; the right-anchored reads align back to b + 1 - h and clip, outward, the complement of G[a + h], G[a + h + 1] ...: L, reverse, PARTNER "
         "a + h; both INV 200 - 2 h; INV rows are not mated",
         [seeded(37, 1), _g], [site(1, _a - 1 + _h, R_SIDE, rc(_g.get(_b - _h - 27, _b - _h)), partner=_b - _h, strand=1, mm=0, hits=1, type="INV", len=200 - 2 * _h, mate=None, hom=None),
                               site(1, _b + 1 - _h, L_SIDE, rc(_g.get(_a + _h, _a + _h + 27))[::-1], partner=_a + _h, strand=1, mm=0, hits=1, type="INV", len=200 - 2 * _h, mate=None,
                                    hom=None)], W=300)

# ---- 2. a clip that continues the reference
_g = Seq(seeded(900, 7))
case("zero", "clips that continue the reference", "R: the columns are G[P + 1 ...], Q = P + 1; L: they are G[P - 1], G[P - 2] ..., Q = P - 1: REF, LEN 0, no mate",
     [_g, seeded(50, 2)], [site(0, 500, R_SIDE, _g.get(501, 528), partner=501, strand=0, mm=0, hits=1, type="REF", len=0, mate=None),
                           site(0, 500, L_SIDE, _g.down(499, 28), partner=499, strand=0, mm=0, hits=1, type="REF", len=0, mate=None)], W=300)

# ---- 3. every nibble phase of the window start, CLEN around one and two 64-bit words
_g = Seq(seeded(700, 11))
_sites = []
for _p in range(16):
    for _cl in (1, 15, 16, 17, 27, 28):
        _q = 161 + _p                                  # (base q is nibble q - 1 of the contig, whose store offset is a multiple of 16 bases)
        _claim = lambda q: dict(partner=q, strand=0, mm=0, type="DEL", len=10) if _cl >= 15 else {}
        _sites.append(site(1, _q - 11, R_SIDE, _g.get(_q, _q + _cl - 1), **_claim(_q)))       # the window starts at q
        _q = 400 + _p + _cl                            # (read descending from q: the window starts at q - cl + 1 = 401 + p)
        _sites.append(site(1, _q + 11, L_SIDE, _g.down(_q, _cl), **_claim(_q)))
case("phase", "16 phases x CLEN 1, 15, 16, 17, 27, 28, read ascending and descending",
     "a consensus cut from the reference at every nibble phase of its window (one, two and three 64-bit words of the store) is found where it was "
     "cut, 10 bases from the breakpoint, with no mismatch; CLEN = 1 is left to the definition", [seeded(37, 1), _g], _sites, W=40, K=1, M=0)

# ---- 4. bounds
_t = Seq("C" + "A" * 60 + "G")                         # 62 bases: the only C is the first base, the only G the last
case("bounds", "Q at len and Q at 1, CLEN = 1",
     "R with the column G at P = 57: the only forward candidate without mismatch is Q = 62 = len (a window of one base); the C at base 1 would match "
     "on the reverse strand and is outside W = 10.  L with the column C at P = 6: Q = 1",
     [seeded(37, 1), _t, seeded(40, 3)], [site(1, 57, R_SIDE, "G", partner=62, strand=0, mm=0, hits=1, type="DEL", len=4),
                                         site(1, 6, L_SIDE, "C", partner=1, strand=0, mm=0, hits=1, type="DEL", len=4)], W=10, K=1, M=0)
_t = Seq(seeded(120, 21))
case("bounds", "windows cut by both contig ends, W larger than the contig",
     "R at P = 30 with G[1 ... 20]: Q = 1, DUP 30; L at P = 90 with G[120], G[119] ...: Q = 120 = len, DUP 31; W = 300 reaches far beyond both ends",
     [seeded(37, 1), _t, seeded(40, 3)], [site(1, 30, R_SIDE, _t.get(1, 20), partner=1, strand=0, mm=0, hits=1, type="DUP", len=30),
                                         site(1, 90, L_SIDE, _t.down(120, 20), partner=120, strand=0, mm=0, hits=1, type="DUP", len=31)], W=300)
case("bounds", "the best placement lies one base outside the contig",
     "19 columns cut from the contig's last / first 19 bases and a 20th that would lie at len + 1 / at 0: with the guard nibble counted as one mismatch "
     "they would be placed at Q = 102 / Q = 19 with MISMATCH 1; there is no such candidate, and every real one has more than M = 2 mismatches: unaligned, "
     "HITS 0.  On all four readings (ascending and descending, forward and reverse)",
     [seeded(37, 1), _t, seeded(40, 3)],
     [site(1, 40, R_SIDE, _t.get(102, 120) + "A", hits=0, type=None),                      # forward, ascending from 102: the last column at len + 1
      site(1, 40, L_SIDE, _t.get(102, 120).translate(_COMP) + "A", hits=0, type=None),     # reverse, ascending
      site(1, 40, L_SIDE, _t.down(19, 19) + "A", hits=0, type=None),                       # forward, descending from 19: the last column at 0
      site(1, 40, R_SIDE, _t.down(19, 19).translate(_COMP) + "A", hits=0, type=None)],     # reverse, descending
     W=300)
case("bounds", "a contig shorter than CLEN", "12 bases cannot hold 20 columns: searched, no candidate, PARTNER `.`",
     [seeded(37, 1), seeded(12, 5), seeded(40, 3)], [site(1, 5, R_SIDE, seeded(20, 6), status=SEARCHED, partner=0, mm=NO_MM, hits=0, type=None),
                                                    site(1, 5, L_SIDE, seeded(20, 6), status=SEARCHED, partner=0, mm=NO_MM, hits=0, type=None)], W=300)
_g = Seq(seeded(900, 31))
for _w, _found in ((100, True), (99, False)):
    _c = dict(strand=0, mm=0, hits=1, type="DEL", len=99) if _found else dict(hits=0, type=None)
    case("bounds", "the planted partner at P + W and P - W" if _found else "the planted partner one base beyond P + W and P - W",
         "R at P = 500 with G[600 ...] and L at P = 400 with G[300], G[299] ...: the partner is exactly W = 100 away and found" if _found else
         "the same sites with W = 99: the partner is no candidate, nothing else is within M", [seeded(37, 1), _g],
         [site(1, 500, R_SIDE, _g.get(600, 627), **dict(_c, partner=600) if _found else _c), site(1, 400, L_SIDE, _g.down(300, 28), **dict(_c, partner=300) if _found else _c)], W=_w)

# ---- 5. the order of rule 3
_x28 = seeded(28, 41)
_g = Seq(seeded(600, 42))
_g.put(170, _x28), _g.put(230, _x28)
case("order", "equal mm at equal distance on both sides", "the 28-mer lies at 170 and at 230, P = 200: both forward, both 30 away; the smaller Q wins, HITS 2",
     [_g, seeded(37, 1)], [site(0, 200, R_SIDE, _x28, partner=170, strand=0, mm=0, hits=2, type="DUP", len=31)], W=300)
_pal = seeded(10, 43) + rc(seeded(10, 43))
_g = Seq(seeded(600, 44))
_g.put(100, _pal), _g.put(161, _pal)
case("order", "a palindromic consensus: forward and reverse tie",
     "a 20-mer that is its own reverse complement lies at 100 ... 119 and 161 ... 180; for R at P = 140 the forward candidate Q = 161 and the reverse "
     "candidate Q = 119 are both 21 away with no mismatch: forward wins; the four placements are HITS 4",
     [_g, seeded(37, 1)], [site(0, 140, R_SIDE, _pal, partner=161, strand=0, mm=0, hits=4, type="DEL", len=20)], W=300)
_g = Seq(seeded(600, 45))
_g.put(150, _x28), _g.put(230, _x28)
case("order", "equal mm at different distances", "the 28-mer lies 50 below and 30 above P = 200: the nearer wins",
     [_g, seeded(37, 1)], [site(0, 200, R_SIDE, _x28, partner=230, strand=0, mm=0, hits=2, type="DEL", len=29)], W=300)
_g = Seq(seeded(600, 46))
_m2, _m3 = list(_x28), list(_x28)
for _k in (3, 20):
    _m2[_k] = other(_m2[_k])
for _k in (0, 13, 27):
    _m3[_k] = other(_m3[_k])
_g.put(150, "".join(_m2)), _g.put(400, "".join(_m3))
case("order", "mm of exactly M and of M + 1",
     "the reference holds the 28-mer with two substitutions at 150 and with three at 400: at M = 2 the first site is aligned with MISMATCH 2 and HITS 1, "
     "the second is unaligned and still reports its best candidate, MISMATCH 3",
     [_g, seeded(37, 1)], [site(0, 100, R_SIDE, _x28, partner=150, strand=0, mm=2, hits=1, type="DEL", len=49),
                          site(0, 450, R_SIDE, _x28, partner=400, strand=0, mm=3, hits=0, type=None)], W=120)
_g = Seq(seeded(300, 47))
_g.put(100, "T" + "ACG" * 20 + "T")                    # the repeat is bases 101 ... 160
case("order", "HITS in a tandem repeat", "(ACG) x 20 at 101 ... 160 and the consensus (ACG) x 7: the windows at 101, 104 ... 140 match, fourteen of them; the "
     "nearest to P = 91 is 101; the reverse complement (CGT) x 7 occurs nowhere",
     [_g, seeded(37, 1)], [site(0, 91, R_SIDE, "ACG" * 7, partner=101, strand=0, mm=0, hits=14, type="DEL", len=9)], W=300, M=0)

# ---- 6. reference letters that are no base
_g = Seq(seeded(600, 51))
_y = list(_g.get(300, 327))
_g.put(303, "N"), _g.put(310, "r"), _g.put(320, _g[320].lower()), _g.put(321, _g[321].lower())
_z = list(_g.get(400, 427))
_g.put(400, "n"), _g.put(405, "M"), _g.put(427, "y")
case("bases", "N, IUPAC codes and lower-case letters under a column",
     "N and r under two columns are two mismatches whatever the column holds, lower-case a c g t are the bases themselves: MISMATCH 2; n, M and y under "
     "three columns are three: unaligned at M = 2.  On the reverse strand too (the complement of N is no base)",
     [_g, seeded(37, 1)], [site(0, 250, R_SIDE, "".join(_y), partner=300, strand=0, mm=2, hits=1, type="DEL", len=49),
                          site(0, 350, R_SIDE, "".join(_z), partner=400, strand=0, mm=3, hits=0, type=None),
                          site(0, 250, R_SIDE, rc("".join(_y)), partner=327, strand=1, mm=2, hits=1, type="INV", len=77),
                          site(0, 350, L_SIDE, "".join(_y)[::-1], partner=327, strand=0, mm=2, hits=1, type="DEL", len=22)], W=100)

# ---- 7. status
_g = Seq(seeded(400, 61))
case("status", "CLEN = K - 1, a contig that is not loaded, a tid outside the table, P = 0, P = len + 1, P = 1 and P = len",
     "19 columns at K = 20: short_consensus, also where the contig is not loaded; 20 columns on contig 1 (not loaded) and on tid 5: off_reference; P = 0 and "
     "P = 401 on contig 0: off_reference; P = 1 and P = 400 are searched",
     [_g, None, seeded(37, 1)], [site(0, 100, R_SIDE, _g.get(150, 168), status=SHORT, partner=0, mm=NO_MM, hits=0),
                                site(1, 100, R_SIDE, _g.get(150, 168), status=SHORT), site(1, 100, R_SIDE, _g.get(150, 169), status=OFF, partner=0, mm=NO_MM, hits=0),
                                site(5, 100, R_SIDE, _g.get(150, 169), status=OFF), site(0, 0, R_SIDE, _g.get(1, 20), status=OFF),
                                site(0, 401, L_SIDE, _g.down(400, 20), status=OFF),
                                site(0, 1, R_SIDE, _g.get(2, 21), status=SEARCHED, partner=2, type="REF", len=0),
                                site(0, 400, L_SIDE, _g.down(399, 20), status=SEARCHED, partner=399, type="REF", len=0)], W=300, lengths=[400, 500, 37])

# ---- 8. structure: site counts around the grid, window lengths around the workgroup's stride
_g = Seq(seeded(2000, 71))
for _n in (CA_GRID - 1, CA_GRID, CA_GRID + 1):
    case("structure", "%d sites" % _n, "one site fewer than the grid has workgroups, exactly as many, and one more (the first workgroup takes a second site); "
         "every site continues the reference at its own P", [seeded(37, 1), _g],
         [site(1, 10 + k % 1900, R_SIDE, _g.get(11 + k % 1900, 18 + k % 1900), status=SEARCHED) for k in range(_n)], W=2, K=4, M=1)
for _rounds in (1, 2):
    # 2 W + CLEN window starts: CLEN = 19, 20, 21 at this W is one start fewer than the rounds hold, exactly as many, and one more
    _w = (_rounds * CA_STRIDE - 20) // 2
    _sites = []
    for _cl in (19, 20, 21):
        _P = 1000
        _sites.append(site(1, _P, R_SIDE, _g.get(_P + _w, _P + _w + _cl - 1), partner=_P + _w, strand=0, mm=0, type="DEL", len=_w - 1))      # the last start
        _sites.append(site(1, _P, L_SIDE, _g.down(_P - _w, _cl), partner=_P - _w, strand=0, mm=0, type="DEL", len=_w - 1))                   # the first start
    case("structure", "window starts around %d round(s) of the workgroup" % _rounds,
         "W = %d: a site of 19, 20 and 21 columns has %d, %d and %d window starts; the partner is planted at P + W (the last start, read ascending) "
         "and at P - W (the first start, read descending)" % (_w, 2 * _w + 19, 2 * _w + 20, 2 * _w + 21), [seeded(37, 1), _g], _sites, W=_w, K=19, M=0)

N_CASES = len(CASES)


def big_case():
    """one site with W = 2^20 on a contig of 2.2 Mb of seeded bases, its partner planted exactly W above P: for the numpy restatement only"""
    text = seeded(2200000, 81)
    P, W = 1100000, 1 << 20
    g = Seq(text)
    return {"family": "structure", "name": "structure: W = 2^20 on 2.2 Mb", "claims": "the consensus is G[P + W ...]: PARTNER P + W, DEL W - 1",
            "contigs": [seeded(37, 1), text], "lengths": [37, len(text)], "W": W, "K": 20, "M": 2,
            "sites": [site(1, P, R_SIDE, g.get(P + W, P + W + 27), partner=P + W, strand=0, mm=0, type="DEL", len=W - 1)]}
