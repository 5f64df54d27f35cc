"""Aimed cases for the genome-wide placement of clip-site consensus (tiddit_amd/tiddit_clip_far.py, csrc/tdt_clip_far.hip): designed
references of a few thousand bases over two to four contigs (so that contig offsets, guards and the contig lookup matter) and clip sites
whose consensus is cut from them, each with the claim it makes, written down from what the case PLANTED (which bases were copied from
where, which junction was cut into the sample) — never computed by the definition or by the restatement of
tests/test_clip_far_refs_cpu.py.

A case is a dict: ``contigs`` (one string of letters per contig, None for a contig that is not loaded), ``lengths``, ``sites``
(:func:`site`), ``K`` / ``M``, ``family``, ``claims`` (a sentence).  A site's ``claim`` is a dict with any of ``status ptid partner
strand mm hits`` (the six columns of the device) and ``type len mate_chrom mate hom`` (of the definition's summarise; ``type`` None:
unplaced) — only what the case planted is claimed.  Positions are 1-based, as in the definition."""
import os
import re

import numpy as np

from clip_align_cases import L_SIDE, NO_MM, OFF, R_SIDE, SEARCHED, SHORT, Seq, fasta_raw, other, pack, rc, seeded  # noqa: F401
from tiddit_amd import refseq

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiddit_amd", "csrc", "tdt_clip_far.hip")).read()
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def _define(name):
    """a number from the `#define` lines of csrc/tdt_clip_far.hip: the cases stay on the kernel's edges when it is retuned"""
    return int(re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+([0-9]+)[ \t]*(?://[^\n]*)?$" % name, _SRC, re.M).group(1))


FAR_BLOCK, FAR_RUN, FAR_TILE, FAR_GRID = _define("FAR_BLOCK"), _define("FAR_RUN"), _define("FAR_TILE"), _define("FAR_GRID")
FAR_FILTER_LOG2, FAR_HASH_MUL = _define("FAR_FILTER_LOG2"), _define("FAR_HASH_MUL")
GUARD = 16                                             # bytes of zeros in front of and behind every contig of the store (tdt_refseq.h)


def filter_bit(key):
    """the filter bit of a 32-bit seed key, as the source's comment defines it"""
    return ((key * FAR_HASH_MUL) & 0xffffffff) >> (32 - FAR_FILTER_LOG2)


def key_of(bases16):
    """16 bases -> the 32-bit key: 2 bits per base, the first base on top"""
    return sum("ACGT".index(ch) << (30 - 2 * j) for j, ch in enumerate(bases16))


def bases_of(key):
    return "".join("ACGT"[(key >> (30 - 2 * j)) & 3] for j in range(16))


def first_nibble(lengths, t):
    """the store nibble of base 1 of contig t: every contig starts on an 8-byte boundary behind GUARD bytes (refseq.RefSeq.layout)"""
    off = GUARD
    for c in range(t):
        off += (lengths[c] + 15) // 16 * 8 + GUARD
    return 2 * off


def cut(g, Q, side, strand, clen):
    """the consensus columns of a site on ``side`` whose placement is (Q, strand) on the contig ``g`` (a Seq): rule 2 read backwards"""
    step = 1 if (side == R_SIDE) == (strand == 0) else -1
    s = "".join(g[Q + step * j] for j in range(clen))
    return s.translate(_COMP) if strand else s


def site(tid, P, side, bases, **claim):
    return {"tid": tid, "P": P, "side": side, "clen": len(bases), "cons": pack(bases.upper()), "bases": bases, "claim": claim}


CASES = []


def case(family, name, claims, contigs, sites, K=20, M=2, lengths=None, add=True):
    c = {"family": family, "name": family + ": " + name, "claims": claims, "contigs": [x.text() if isinstance(x, Seq) else x for x in contigs],
         "sites": sites, "K": K, "M": M, "lengths": lengths or [len(x.text() if isinstance(x, Seq) else x) for x in contigs]}
    if add:
        CASES.append(c)
    return c


def host_reference(c):
    return refseq.HostReference({t: refseq.codes_of_bases(s) for t, s in enumerate(c["contigs"]) if s is not None})


def columns(c):
    """the four site columns as tdt_clip_rows gives them"""
    s = c["sites"]
    return (np.array([(x["tid"] << 32) | x["P"] for x in s], dtype=np.uint64), np.array([x["side"] for x in s], dtype=np.uint32),
            np.array([x["clen"] for x in s], dtype=np.uint32), np.array([x["cons"] for x in s], dtype=np.uint64))


def sites_of(c):
    return [((x["tid"] << 32) | x["P"], x["side"], 3, x["clen"]) for x in c["sites"]]


def definition(c):
    """the definition over the case -> (placed: [(status, contig, PARTNER, strand, mm, HITS)], counters, rows of summarise)"""
    from tiddit_amd import tiddit_clip_far as F
    ref = host_reference(c)
    placed = [F.place_site(ref, x["tid"], x["P"], x["side"], x["clen"], x["cons"], c["K"], c["M"]) for x in c["sites"]]
    counts, rows = F.summarise(sites_of(c), placed, c["M"])
    return placed, counts, rows


_PLACED = ("status", "ptid", "partner", "strand", "mm", "hits")
_ROW = {"type": 10, "len": 11, "mate_chrom": 12, "mate": 13, "hom": 14}


def agrees_with_claim(c, placed, rows):
    """``placed`` / ``rows`` (of the definition, of the restatement, of the device + summarise) against the claims -> None or what differs"""
    searched = iter(rows)
    for i, (x, p) in enumerate(zip(c["sites"], placed)):
        row = next(searched) if p[0] == SEARCHED else None
        for k, v in x["claim"].items():
            got = p[_PLACED.index(k)] if k in _PLACED else None if row is None else row[_ROW[k]]
            if got != v:
                return "site %d (%s %d): %s is %r, claimed %r" % (i, "LR"[x["side"]], x["P"], k, got, v)
    return None


def _differ(g, q, ch):
    """make base q of g differ from the letter ch (so that an aligner's extension stops there)"""
    if g[q].upper() == ch.upper():
        g.put(q, other(ch))


# ---- 1. every nibble phase of the seed start x CLEN 16 ... 28 x both sides x both strands, on another contig
_g = Seq(seeded(2200, 1001))
_sites, _n = [], 0
for _cl in range(16, 29):
    for _side in (L_SIDE, R_SIDE):
        for _strand in (0, 1):
            for _p in range(16):
                _s = 161 + 32 * _n + _p                # the seed's first base, ascending: nibble phase p (contig 1 starts on a word)
                _asc = (_side == R_SIDE) == (_strand == 0)
                _Q = _s if _asc else _s + 15
                _sites.append(site(0, 20, _side, cut(_g, _Q, _side, _strand, _cl), status=SEARCHED, ptid=1, partner=_Q, strand=_strand, mm=0, type="BND", len=None))
            _n += 1
case("phase", "16 phases x CLEN 16 ... 28 x both sides x both strands",
     "a consensus cut from contig 1 with its seed at every nibble phase (the other columns behind the seed when read ascending, in front of it "
     "when read descending) is placed where it was cut, by a site of contig 0: BND", [seeded(48, 1), _g], _sites, K=16, M=0)

# ---- 2. bounds
_t = Seq(seeded(200, 1011))
case("bounds", "windows that touch the first and the last base of a contig",
     "28 columns read ascending from Q = 1 and from Q = len - 27, descending from Q = 28 and from Q = len: all four are candidates",
     [seeded(48, 1), _t, seeded(40, 3)],
     [site(0, 20, R_SIDE, cut(_t, 1, R_SIDE, 0, 28), ptid=1, partner=1, strand=0, mm=0, hits=1, type="BND"),
      site(0, 20, R_SIDE, cut(_t, 173, R_SIDE, 0, 28), ptid=1, partner=173, strand=0, mm=0, hits=1, type="BND"),
      site(0, 20, L_SIDE, cut(_t, 28, L_SIDE, 0, 28), ptid=1, partner=28, strand=0, mm=0, hits=1, type="BND"),
      site(0, 20, L_SIDE, cut(_t, 200, L_SIDE, 0, 28), ptid=1, partner=200, strand=0, mm=0, hits=1, type="BND"),
      site(0, 20, L_SIDE, cut(_t, 1, L_SIDE, 1, 28), ptid=1, partner=1, strand=1, mm=0, hits=1, type="BND"),
      site(0, 20, R_SIDE, cut(_t, 200, R_SIDE, 1, 28), ptid=1, partner=200, strand=1, mm=0, hits=1, type="BND")])
case("bounds", "the same one base further: the seed inside the contig, the last column outside it",
     "27 columns cut from the contig's last / first 27 bases and a 28th that would lie at len + 1 / at 0: the seed matches inside the contig, "
     "the window does not fit: no candidate, on all four readings; and a seed whose own first base would lie at 0 / len + 1",
     [seeded(48, 1), _t, seeded(40, 3)],
     [site(0, 20, R_SIDE, _t.get(174, 200) + "A", status=SEARCHED, ptid=0, partner=0, mm=NO_MM, hits=0, type=None),
      site(0, 20, L_SIDE, _t.get(174, 200).translate(_COMP) + "A", hits=0, type=None),
      site(0, 20, L_SIDE, _t.down(27, 27) + "A", hits=0, type=None),
      site(0, 20, R_SIDE, _t.down(27, 27).translate(_COMP) + "A", hits=0, type=None),
      site(0, 20, L_SIDE, "A" + _t.down(200, 27), hits=0, type=None),
      site(0, 20, R_SIDE, "A" + _t.get(1, 27), hits=0, type=None)])
_c15, _c16, _c20 = Seq(seeded(15, 1021)), Seq(seeded(16, 1022)), Seq(seeded(20, 1023))
case("bounds", "contigs of 15, 16 and CLEN bases",
     "a contig of 15 bases holds no seed; one of 16 holds exactly the window of a 16-column site, read either way; one of 20 the window of a "
     "20-column site and not that of a 21-column one",
     [seeded(48, 1), _c15, _c16, _c20],
     [site(0, 20, R_SIDE, _c15.get(1, 15) + "A", hits=0, type=None), site(0, 20, R_SIDE, "A" + _c15.get(1, 15), hits=0, type=None),
      site(0, 20, R_SIDE, _c16.get(1, 16), ptid=2, partner=1, strand=0, mm=0, hits=1, type="BND"),
      site(0, 20, L_SIDE, _c16.down(16, 16), ptid=2, partner=16, strand=0, mm=0, hits=1, type="BND"),
      site(0, 20, R_SIDE, _c20.get(1, 20), ptid=3, partner=1, strand=0, mm=0, hits=1, type="BND"),
      site(0, 20, L_SIDE, cut(_c20, 1, L_SIDE, 1, 20), ptid=3, partner=1, strand=1, mm=0, hits=1, type="BND"),
      site(0, 20, R_SIDE, _c20.get(1, 20) + "A", hits=0, type=None), site(0, 20, L_SIDE, _c20.down(20, 20) + "A", hits=0, type=None)], K=16)
_a, _b = Seq(seeded(64, 1031)), Seq(seeded(64, 1032))
case("bounds", "a seed that would only match across the guard between two contigs",
     "the last 8 bases of contig 1 and the first 8 of contig 2 (which follows it in the store), then 12 more of contig 2: no contig holds them",
     [seeded(48, 1), _a, _b], [site(0, 20, R_SIDE, _a.get(57, 64) + _b.get(1, 20), status=SEARCHED, hits=0, type=None),
                               site(0, 20, R_SIDE, _a.get(50, 64) + _b.get(1, 13), hits=0, type=None)])

# ---- 3. contigs that are not loaded
_u, _l = Seq(seeded(300, 1041)), Seq(seeded(300, 1042))
case("unloaded", "a site on a contig that is not loaded, and a consensus that lies on one",
     "contig 1 is not loaded: its own site is off_reference; a site of contig 0 whose consensus is cut from contig 1's bases finds nothing, "
     "one cut from contig 2 is placed there; a tid outside the table is off_reference",
     [seeded(48, 1), None, _l],
     [site(1, 100, R_SIDE, _l.get(100, 127), status=OFF, ptid=0, partner=0, mm=NO_MM, hits=0), site(0, 20, R_SIDE, _u.get(100, 127), status=SEARCHED, hits=0, type=None),
      site(0, 20, R_SIDE, _l.get(100, 127), ptid=2, partner=100, mm=0, hits=1, type="BND"), site(7, 20, R_SIDE, _l.get(100, 127), status=OFF),
      site(0, 0, R_SIDE, _l.get(100, 127), status=OFF), site(0, 49, R_SIDE, _l.get(100, 127), status=OFF), site(0, 48, L_SIDE, _l.get(100, 118), status=SHORT)],
     lengths=[48, 300, 300])

# ---- 4. reference letters that are no base
_g = Seq(seeded(900, 1051))
_w = [_g.get(100 + 100 * k, 127 + 100 * k) for k in range(7)]
_g.put(103, _g[103].lower()), _g.put(120, _g[120].lower())          # lower case in the seed and behind it: the bases themselves
_g.put(205, "N")                                                     # N in the seed
_g.put(310, "r")                                                     # an IUPAC code in the seed
_g.put(420, "N"), _g.put(425, "y")                                   # two in the other columns
_g.put(517, "n"), _g.put(520, "M"), _g.put(527, "K")                 # three
_g.put(616, "N")                                                     # column 16 itself
case("bases", "N, IUPAC codes and lower-case letters under the seed and under the other columns",
     "lower-case a c g t are the bases themselves; N or r under a seed column: no candidate (on the reverse strand too: the complement of N is "
     "no base); N and y under two other columns are two mismatches, n, M and K three: refused at M = 2",
     [seeded(48, 1), _g],
     [site(0, 20, R_SIDE, _w[0], ptid=1, partner=100, strand=0, mm=0, hits=1), site(0, 20, R_SIDE, _w[1], hits=0, type=None),
      site(0, 20, R_SIDE, _w[2], hits=0, type=None), site(0, 20, L_SIDE, _w[2].translate(_COMP), hits=0, type=None),
      site(0, 20, R_SIDE, _w[3], ptid=1, partner=400, strand=0, mm=2, hits=1), site(0, 20, R_SIDE, _w[4], hits=0, type=None),
      site(0, 20, R_SIDE, _w[5], ptid=1, partner=600, strand=0, mm=1, hits=1),
      # (L on the reverse strand reads ascending from Q too, against the complement)
      site(0, 20, L_SIDE, _w[3].translate(_COMP), ptid=1, partner=400, strand=1, mm=2, hits=1), site(0, 20, L_SIDE, _w[1].translate(_COMP), hits=0, type=None),
      # (R on the reverse strand reads descending from 427: the N at 420 lies under its column 7, inside the seed)
      site(0, 20, R_SIDE, rc(_w[3]), hits=0, type=None)])

# ---- 5. mismatches: the seed is exact, the other columns count
_g = Seq(seeded(1200, 1061))
_x = [_g.get(100 + 100 * k, 127 + 100 * k) for k in range(8)]


def _sub(q, *cols):
    for _k in cols:
        _g.put(q + _k, other(_g[q + _k]))


_sub(100, 16, 27), _sub(200, 16, 20, 27), _sub(300, 15), _sub(400, 16), _sub(500, 0), _sub(600, 15, 16)
case("mismatch", "mm = M accepted, M + 1 refused; column 15 against column 16",
     "two substitutions under columns 16 and 27: MISMATCH 2 = M, placed, HITS 1; three: refused; ONE under column 15 (or column 0) is no "
     "candidate although 1 <= M; one under column 16 is a candidate with MISMATCH 1; read descending too",
     [seeded(48, 1), _g],
     [site(0, 20, R_SIDE, _x[0], ptid=1, partner=100, strand=0, mm=2, hits=1, type="BND"), site(0, 20, R_SIDE, _x[1], ptid=0, partner=0, mm=NO_MM, hits=0, type=None),
      site(0, 20, R_SIDE, _x[2], hits=0, type=None), site(0, 20, R_SIDE, _x[3], ptid=1, partner=400, strand=0, mm=1, hits=1),
      site(0, 20, R_SIDE, _x[4], hits=0, type=None), site(0, 20, R_SIDE, _x[5], hits=0, type=None),
      # read descending (L forward) column j lies at Q - j: the substitutions at bases 116 and 127 are columns 11 and 0 from Q = 127, inside the seed
      site(0, 20, L_SIDE, _x[0][::-1], hits=0, type=None),
      site(0, 20, L_SIDE, _x[6][::-1], ptid=1, partner=727, strand=0, mm=0, hits=1)])
_g2 = Seq(seeded(400, 1062))
_y = _g2.get(100, 127)
_g2.put(100 + 11, other(_g2[111])), _g2.put(100 + 0, other(_g2[100]))                # under columns 16 and 27 of the descending reading from 127
_z = _g2.get(200, 227)
_g2.put(200 + 12, other(_g2[212]))                                                   # under column 15 of the descending reading from 227
case("mismatch", "read descending: columns 16 and 27 lie in FRONT of the seed",
     "an L site reads descending from Q: substitutions at Q - 16 and Q - 27 are MISMATCH 2; one at Q - 15 is inside the seed: no candidate",
     [seeded(48, 1), _g2], [site(0, 20, L_SIDE, _y[::-1], ptid=1, partner=127, strand=0, mm=2, hits=1, type="BND"),
                            site(0, 20, L_SIDE, _z[::-1], hits=0, type=None)])

# ---- 6. the order of rule 3
_x28 = seeded(28, 1071)
_own, _o1, _o2 = Seq(seeded(3000, 1072)), Seq(seeded(500, 1073)), Seq(seeded(500, 1074))
_own.put(2000, _x28), _o1.put(100, _x28)
case("order", "the site's own contig against another", "the 28-mer lies 1500 bases away on the site's contig 1 and on contig 0 (a smaller t): the own contig "
     "wins, HITS 2, DEL", [_o1, _own, _o2], [site(1, 500, R_SIDE, _x28, ptid=1, partner=2000, strand=0, mm=0, hits=2, type="DEL", len=1499)])
_own = Seq(seeded(3000, 1075))
_m1 = list(_x28)
_m1[20] = other(_m1[20])
_own.put(2000, "".join(_m1))
case("order", "fewer mismatches on another contig beat the own contig", "one substitution on the site's own contig, none on contig 0: BND, HITS 2",
     [_o1, _own, _o2], [site(1, 500, R_SIDE, _x28, ptid=0, partner=100, strand=0, mm=0, hits=2, type="BND", len=None)])
_own = Seq(seeded(3000, 1076))
_own.put(300, _x28), _own.put(2000, _x28), _own.put(1200, _x28)
case("order", "nearer against farther, and equal distances", "on the own contig at 300, 1200 and 2000: from P = 1000 the nearest is 1200; from P = 1150 both "
     "300 and 2000 are 850 away and 1200 is nearer; from P = 750 the windows at 300 and 1200 are both 450 away: the smaller Q",
     [_o2, _own], [site(1, 1000, R_SIDE, _x28, ptid=1, partner=1200, strand=0, mm=0, hits=3, type="DEL", len=199),
                   site(1, 1150, R_SIDE, _x28, ptid=1, partner=1200, mm=0, hits=3), site(1, 750, R_SIDE, _x28, ptid=1, partner=300, mm=0, hits=3, type="DUP", len=451)])
_pal = seeded(14, 1077) + rc(seeded(14, 1077))
_own, _o1 = Seq(seeded(600, 1078)), Seq(seeded(600, 1079))
_own.put(100, _pal), _own.put(173, _pal)
_o1.put(200, _pal)
case("order", "a palindromic consensus: forward against reverse",
     "a 28-mer that is its own reverse complement at 100 ... 127 and 173 ... 200 of the own contig: from P = 150 forward Q = 173 and reverse Q = 127 are "
     "both 23 away: forward wins; with the two placements of contig 1, HITS 6",
     [_own, _o1], [site(0, 150, R_SIDE, _pal, ptid=0, partner=173, strand=0, mm=0, hits=6, type="DEL", len=22)])
case("order", "a palindromic consensus on another contig alone", "forward Q = 200 and reverse Q = 227 on contig 1: forward wins, HITS 2",
     [seeded(48, 1), _o1], [site(0, 20, R_SIDE, _pal, ptid=1, partner=200, strand=0, mm=0, hits=2, type="BND")])
_o1, _o2, _o3 = Seq(seeded(600, 1080)), Seq(seeded(600, 1081)), Seq(seeded(600, 1082))
_o1.put(300, _x28), _o1.put(100, _x28), _o2.put(50, _x28), _o3.put(10, rc(_x28))
case("order", "the smaller t, then the smaller Q; a forward placement before a reverse one",
     "forward on contig 1 at 100 and 300 and on contig 2 at 50, reverse on contig 3: forward on contig 1 at 100 wins, HITS 4; a site of contig 1 itself takes "
     "its own contig's nearer placement",
     [seeded(48, 1), _o1, _o2, _o3], [site(0, 20, R_SIDE, _x28, ptid=1, partner=100, strand=0, mm=0, hits=4, type="BND"),
                                      site(1, 250, R_SIDE, _x28, ptid=1, partner=300, strand=0, mm=0, hits=4, type="DEL", len=49)])
_o1, _o2 = Seq(seeded(600, 1083)), Seq(seeded(600, 1084))
_o1.put(300, rc(_x28)), _o2.put(50, _x28)
case("order", "strand before contig", "reverse on contig 1, forward on contig 2: the forward one wins although its t is larger",
     [seeded(48, 1), _o1, _o2], [site(0, 20, R_SIDE, _x28, ptid=2, partner=50, strand=0, mm=0, hits=2, type="BND")])

# ---- 7. HITS
_unit = seeded(28, 1091)
for _n in (1, 2, 64, 65, 300):
    _sp = seeded(5 * _n + 100, 1092)
    _text = _sp[-100:] + "".join(_unit + _sp[5 * k:5 * k + 5] for k in range(_n))
    case("hits", "%d copies" % _n, "the 28-mer lies %d times on contig 1, 33 bases apart: HITS %d, the first copy wins" % (_n, _n),
         [seeded(48, 1), _text], [site(0, 20, R_SIDE, _unit, ptid=1, partner=101, strand=0, mm=0, hits=_n, type="BND")], M=0)
_far_tail = _unit[16:].translate(_COMP)
_sp = seeded(1000, 1093)
case("hits", "a seed that occurs 1000 times with other columns beyond M",
     "the 16 seed bases 1000 times, each followed by the complement of the site's other 12 columns: 12 mismatches each, HITS 0, unplaced",
     [seeded(48, 1), "".join(_unit[:16] + _far_tail + _sp[k] for k in range(1000))],
     [site(0, 20, R_SIDE, _unit, status=SEARCHED, ptid=0, partner=0, mm=NO_MM, hits=0, type=None)])
for _n in (1, 2, 64, 65):
    _tails, _seed = [], 1100
    while len(_tails) < _n:                                        # other columns that differ from each other in more than M places
        _c, _seed = seeded(12, _seed), _seed + 1
        if all(sum(a != b for a, b in zip(_c, _o)) > 2 for _o in _tails):
            _tails.append(_c)
    _sp = seeded(4 * _n + 100, 1094)
    _text = _sp[-100:] + "".join(_unit[:16] + _tails[k] + _sp[4 * k:4 * k + 4] for k in range(_n))
    case("hits", "%d sites sharing one seed" % _n, "%d sites with the same 16 seed columns and other columns of their own, each planted once, 32 bases "
         "apart: every site finds its own copy, HITS 1" % _n, [seeded(48, 1), _text],
         [site(0, 1 + k % 48, R_SIDE, _unit[:16] + _tails[k], ptid=1, partner=101 + 32 * k, strand=0, mm=0, hits=1) for k in range(_n)])
_ps = seeded(8, 1095) + rc(seeded(8, 1095))
_g = Seq(seeded(600, 1096))
_g.put(300, _ps + seeded(12, 1097))
case("hits", "a palindromic seed: both of the site's entries carry one key",
     "the 16 seed bases are their own reverse complement: the ascending and the descending entry of the site are equal keys; the placement "
     "read ascending at 300 has no mismatch, the one read descending from 315 on the reverse strand has the wrong bases in front of it: HITS 1",
     [seeded(48, 1), _g], [site(0, 20, R_SIDE, _g.get(300, 327), ptid=1, partner=300, strand=0, mm=0, hits=1, type="BND")])

# ---- 8. the filter: a seed that is absent and falls on the bit of one that is present
_g = Seq(seeded(600, 1101))
_present = key_of(_g.get(300, 315))
_inv = pow(FAR_HASH_MUL, -1, 1 << 32)
_absent = next(k for k in ((_inv * ((filter_bit(_present) << (32 - FAR_FILTER_LOG2)) | low)) & 0xffffffff for low in range(1, 64)) if k != _present)
assert filter_bit(_absent) == filter_bit(_present) and _absent != _present
_g.put(100, bases_of(_absent) + _g.get(316, 327))                  # the absent seed in the reference, with the site's other columns behind it
case("filter", "two seeds on one filter bit, one present and one absent",
     "the reference holds at 100 a 16-mer whose key falls on the filter bit of the site's seed and is another key: the filter passes it, the "
     "table does not hold it: HITS stays 1", [seeded(48, 1), _g], [site(0, 20, R_SIDE, _g.get(300, 327), ptid=1, partner=300, strand=0, mm=0, hits=1, type="BND")])


# ---- 9. structure: windows that straddle a lane's run, a workgroup's tile (and, in big_cases, the grid's stride)
def _straddle(g, lengths, t, boundary, clen=28):
    """sites whose window starts ``k`` nibbles in front of the store nibble ``boundary``, k = 0 ... clen, read ascending (R forward) and
    descending (L forward)"""
    out = []
    first = first_nibble(lengths, t)
    for k in range(clen + 1):
        s = boundary - k - first + 1                               # the window's first base, 1-based in contig t
        out.append(site(0, 20, R_SIDE, cut(g, s, R_SIDE, 0, clen), ptid=t, partner=s, strand=0, mm=0, type="BND"))
        out.append(site(0, 20, L_SIDE, cut(g, s + clen - 1, L_SIDE, 0, clen), ptid=t, partner=s + clen - 1, strand=0, mm=0, type="BND"))
    return out


_g = Seq(seeded(FAR_TILE + 2000, 1111))
_lens = [48, FAR_TILE + 2000]
case("structure", "windows over the end of a lane's run and of a workgroup's tile, at every offset 0 ... CLEN",
     "a lane takes FAR_RUN starts and the words behind them, a workgroup FAR_TILE: a window that starts k = 0 ... 28 nibbles in front of such a "
     "boundary of the store is found like any other, read ascending and descending", [seeded(48, 1), _g],
     _straddle(_g, _lens, 1, FAR_RUN * 40) + _straddle(_g, _lens, 1, FAR_TILE) + _straddle(_g, _lens, 1, FAR_TILE - FAR_RUN * 64, clen=20))

# ---- 10. no sites, no searched sites, K = 16 and 28
_g = Seq(seeded(600, 1121))
case("zero", "no site at all", "nothing in, nothing out: every counter is 0", [seeded(48, 1), _g], [])
case("zero", "no searched site", "every consensus is shorter than K, or the site is off the reference: nothing is searched",
     [seeded(48, 1), _g], [site(0, 20, R_SIDE, _g.get(100, 118), status=SHORT, hits=0), site(0, 99, R_SIDE, _g.get(100, 127), status=OFF, hits=0)])
for _k in (16, 28):
    case("zero", "K = %d" % _k, "CLEN = K is searched and placed, CLEN = K - 1 is short_consensus", [seeded(48, 1), _g],
         [site(0, 20, R_SIDE, _g.get(100, 99 + _k), status=SEARCHED, ptid=1, partner=100, mm=0), site(0, 20, R_SIDE, _g.get(100, 98 + _k), status=SHORT)], K=_k)

# ---- 11. junctions seen from both sides, with microhomology
HOMS = (0, 1, 5, 28)
for _h in HOMS:
    # a translocation: the sample joins A[... a] to B[b + 1 ...]; the h bases behind a on A equal the h bases behind b on B
    _A, _B, _a, _b = Seq(seeded(1200, 1200 + _h)), Seq(seeded(900, 1300 + _h)), 400, 600
    _A.put(_a + 1, _B.get(_b + 1, _b + _h))
    _differ(_B, _b, _A[_a])                            # (the read anchored on B cannot extend to the left)
    _differ(_A, _a + _h + 1, _B[_b + _h + 1])          # (the read anchored on A stops behind the homology)
    _s = [site(0, _a + _h, R_SIDE, _B.get(_b + _h + 1, _b + _h + 28), ptid=1, partner=_b + _h + 1, strand=0, mm=0, hits=1, type="BND", len=None, mate_chrom=1, mate=_b + 1, hom=_h),
          site(1, _b + 1, L_SIDE, _A.down(_a, 28), ptid=0, partner=_a, strand=0, mm=0, hits=1, type="BND", len=None, mate_chrom=0, mate=_a + _h, hom=_h)]
    if _h == 5:
        # a decoy: an L site of B two bases in front of the junction whose clip lies 100 bases further down A — r.PARTNER - o.POS is 2, a
        # smaller HOM than the true mate's, and r.POS - o.PARTNER is 105: no mate
        _s.insert(1, site(1, _b + 4, L_SIDE, _A.down(_a - 100, 28), ptid=0, partner=_a - 100, strand=0, mm=0, type="BND", mate=None, hom=None))
    case("events", "a translocation with %d bases of microhomology" % _h,
         "the reads anchored on A align through the homology to a + h and clip B[b + h + 1 ...]: R, PARTNER B:b + h + 1; the reads anchored on B start "
         "at b + 1 and clip A[a], A[a - 1] ...: L, PARTNER A:a; both BND, mates with HOM h", [_A, _B], _s)
    # a deletion of bases a + 1 ... b whose first h bases equal the h bases behind it (the construction of clip_align_cases)
    _g, _a, _b = Seq(seeded(1200, 1400 + _h)), 400, 600
    _g.put(_a + 1, _g.get(_b + 1, _b + _h))
    _g.differ(_a, _b)
    _g.differ(_a + _h + 1, _b + _h + 1)
    case("events", "a 200-bp deletion with %d bases of microhomology" % _h,
         "R at a + h with PARTNER b + h + 1, L at b + 1 with PARTNER a, on the sites' own contig: DEL 200, mates with HOM h",
         [seeded(48, 1), _g], [site(1, _a + _h, R_SIDE, _g.get(_b + _h + 1, _b + _h + 28), ptid=1, partner=_b + _h + 1, strand=0, mm=0, hits=1, type="DEL", len=200, mate_chrom=1, mate=_b + 1, hom=_h),
                               site(1, _b + 1, L_SIDE, _g.down(_a, 28), ptid=1, partner=_a, strand=0, mm=0, hits=1, type="DEL", len=200, mate_chrom=1, mate=_a + _h, hom=_h)])
# a reverse-strand pair is not mated
_A, _B = Seq(seeded(800, 1501)), Seq(seeded(800, 1502))
case("events", "reverse-strand rows are not mated", "an R site of A whose clip is the reverse complement of B[... 300] and an L site of B that points back: both "
     "placed on the reverse strand, neither mated", [_A, _B],
     [site(0, 400, R_SIDE, cut(_B, 300, R_SIDE, 1, 28), ptid=1, partner=300, strand=1, mm=0, type="BND", mate=None, hom=None),
      site(1, 300, L_SIDE, cut(_A, 400, L_SIDE, 1, 28), ptid=0, partner=400, strand=1, mm=0, type="BND", mate=None, hom=None)])


# ---- 12. one random reference of 100 kb over four contigs, 2000 sites cut from it
def _random_case():
    rs = np.random.RandomState(1601)
    contigs = [Seq(seeded(n, 1602 + i)) for i, n in enumerate((40000, 30000, 20000, 10000))]
    sites = []
    for _ in range(2000):
        t, side, strand, cl = rs.randint(0, 4), rs.randint(0, 2), rs.randint(0, 2), rs.randint(14, 29)
        Q = rs.randint(40, len(contigs[t].b) - 40)
        bases = list(cut(contigs[t], Q, side, strand, cl))
        nsub = rs.randint(0, 4) if cl > 17 else 0
        for j in set(rs.randint(16, cl, nsub).tolist()) if nsub else ():
            bases[j] = other(bases[j])
        own = rs.randint(0, 4)
        sites.append(site(own, rs.randint(1, len(contigs[own].b) + 1), side, "".join(bases), status=SEARCHED if cl >= 20 else SHORT))
    return case("random", "100 kb over four contigs, 2000 sites", "consensus of 14 ... 28 columns cut anywhere, on either strand, with 0 ... 3 substitutions "
                "outside the seed: the status is claimed, the rest is the definition's against the restatement's and the device's", contigs, sites, add=False)


CASES.append(_random_case())
N_CASES = len(CASES)


# ---- 13. large references (built on demand)
def _seeded_big(n, seed):
    return np.array(list(b"ACGT"), dtype=np.uint8)[np.random.RandomState(seed).randint(0, 4, n)].tobytes().decode()


def big_cases():
    """(a) four dispersed duplications on one contig of 2.2 Mb, the copy inserted more than 2^20 bases behind its source, each junction
    seen from both sides, with microhomology 0, 1, 5 and 28; (b) windows that straddle the grid's stride — the first start of the
    second round of workgroup 0 — at every offset 0 ... 28, on a contig of FAR_GRID * FAR_TILE bases and a little"""
    out = []
    g = Seq(_seeded_big(2200000, 1701))
    sites = []
    for i, h in enumerate(HOMS):
        a = 20000 + 10000 * i                          # the source starts at a; the copy is inserted behind c
        c = a + (1 << 20) + 777
        g.put(c + 1, g.get(a, a + h - 1))              # h bases of homology: G[c + 1 ... c + h] = G[a ... a + h - 1]
        g.differ(c + h + 1, a + h)
        g.differ(a - 1, c)
        sites.append(site(1, c + h, R_SIDE, g.get(a + h, a + h + 27), ptid=1, partner=a + h, strand=0, mm=0, hits=1, type="DUP", len=c - a + 1, mate_chrom=1, mate=a, hom=h))
        sites.append(site(1, a, L_SIDE, g.down(c, 28), ptid=1, partner=c, strand=0, mm=0, hits=1, type="DUP", len=c - a + 1, mate_chrom=1, mate=c + h, hom=h))
    out.append(case("events", "dispersed duplications 2^20 + 777 bases away on 2.2 Mb",
                    "the reads anchored in front of the insertion align to c + h and clip G[a + h ...]: R, PARTNER a + h; the reads anchored in the source "
                    "start at a and clip G[c], G[c - 1] ...: L, PARTNER c; DUP c - a + 1, mates with HOM h; beyond TIDDIT_CLIPS_ALIGN's largest window",
                    [seeded(48, 1), g], sites, add=False))
    n = FAR_GRID * FAR_TILE + 4000
    g = Seq(_seeded_big(n, 1702))
    out.append(case("structure", "windows over the grid's stride at every offset 0 ... CLEN",
                    "the store nibble FAR_GRID * FAR_TILE is the first start of workgroup 0's second round: a window that starts k = 0 ... 28 nibbles in "
                    "front of it is found like any other", [seeded(48, 1), g], _straddle(g, [48, n], 1, FAR_GRID * FAR_TILE), add=False))
    return out
