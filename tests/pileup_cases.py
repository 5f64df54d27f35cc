"""Aimed cases for the exact per-base depth (tiddit_amd/tiddit_pileup.py, csrc/tdt_pileup.hip) and the genotype rule of
tiddit_amd/tiddit_small_vcf.py: records built byte by byte with ``bamio.encode_record``, each read with the kind and the KEPT SPANS it is
stated to have — written down by hand from its position and CIGAR, never computed by the definition or by the restatement of
tests/test_pileup_refs_cpu.py.  :func:`expected` adds the stated spans up into per-contig depth arrays and the seven counters.

The contigs (``LENGTHS``): ``TILE - 1``, ``TILE``, ``TILE + 1``, 1, 2, 63, 64, 65 and ``BIG`` = about 20 000 bases (at least three tiles and
a bit, so that one span can cross three tile borders), ``TILE`` read from the source's ``#define PILE_TILE``.  In that order the guard slot
of contig 0 is the LAST slot of tile 0 and the guard slot of contig 1 the FIRST slot of tile 2 (:func:`offsets`).  The ``carry`` family
has a table of its own: one contig of 257 tiles and a bit, so the carry kernel loops.

A case is a dict: ``batches`` (the pushes, in order: lists of reads, each list over its own raw buffer, ``cut`` bytes short), ``Q``,
``lengths``, ``family`` and what it claims (``claims``, a sentence).  ``RULE`` holds the genotype rule's literal claims:
(SUPPORT, DP0) -> the eight columns."""
import os
import re
import struct

import numpy as np

from tiddit_amd import bamio

SN = ("records", "eligible", "malformed", "no_cigar", "spans", "covered_bases", "clamped_spans")
SIZE = 7
COLUMNS = ("flag", "tid", "pos", "mapq", "rec_off")
NOT_ELIGIBLE, MALFORMED, NO_CIGAR, OK = "not_eligible", "malformed", "no_cigar", "ok"
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiddit_amd", "csrc", "tdt_pileup.hip")
TILE = int(re.search(r"^#define PILE_TILE (\d+)", open(_SRC).read(), re.M).group(1))
BIG = max(20000, 3 * TILE + 1000)
LENGTHS = (TILE - 1, TILE, TILE + 1, 1, 2, 63, 64, 65, BIG)
NAMES = tuple("p%d" % t for t in range(len(LENGTHS)))
B = 8                                          # the big contig
CARRY_LENGTHS = (257 * TILE + 5, 100)
Q = 20


def offsets(lengths=LENGTHS):
    """the first slot of every contig: a slot per base and one guard behind each contig"""
    out, at = [], 0
    for n in lengths:
        out.append(at)
        at += n + 1
    return out


assert offsets()[0] + LENGTHS[0] == TILE - 1 and offsets()[1] + LENGTHS[1] == 2 * TILE        # the two guards at a tile's last and first slot


# ------------------------------------------------------------------------------------------- a read and what it is stated to give
def rd(tid=B, pos=0, cigar="20M", spans=(), clamped=0, kind=OK, flag=0, mapq=60, ops=None, seq=None, patch=(), bs_delta=0, col_tid=None):
    """one read.  ``spans``: the kept [(start, end)] the case STATES for it; ``clamped``: the spans stated as cut or dropped; ``kind``: what
    the definition is stated to make of it.  ``ops``: [(op, len)] instead of a CIGAR string; ``seq``: the bases instead of one ``A`` per
    query base; ``patch``: ((byte offset in the record, struct format, value), ...); ``bs_delta``: added to block_size; ``col_tid``: the
    tid of the batch's column (and of the record) where ``encode_record`` would not take it"""
    cig = list(ops) if ops is not None else bamio.parse_cigar(cigar) if cigar else []
    qlen = sum(ln for op, ln in cig if op in (0, 1, 4, 7, 8))
    assert kind == OK or not spans
    return {"cigar": cig, "flag": flag, "tid": tid if col_tid is None else col_tid, "pos": pos, "mapq": mapq, "seq": "A" * qlen if seq is None else seq,
            "patch": tuple(patch), "bs_delta": bs_delta, "kind": kind, "spans": [tuple(s) for s in spans], "clamped": clamped}


def _record(i, r):
    ok_tid = r["tid"] if -1 <= r["tid"] < 2 ** 15 else 0
    rec = bytearray(bamio.encode_record("r%d" % i, r["flag"], ok_tid, r["pos"] if 0 <= r["pos"] < 2 ** 29 else 0, r["mapq"], r["cigar"], -1, -1, 0, seq=r["seq"]))
    struct.pack_into("<i", rec, 4, r["tid"])
    struct.pack_into("<i", rec, 8, r["pos"])
    if r["bs_delta"]:
        struct.pack_into("<I", rec, 0, len(rec) - 4 + r["bs_delta"])
    for off, fmt, val in r["patch"]:
        struct.pack_into(fmt, rec, off, val)
    return bytes(rec)


class Batch:
    """the columns of a run of reads over one raw buffer — what tdt_pile_push and the definition take"""

    def __init__(self, raw, **cols):
        self.raw = raw
        for k in COLUMNS:
            setattr(self, k, cols[k])

    def __len__(self):
        return len(self.tid)


def build_batch(reads, cut=0):
    """the reads back to back, as a BAM file holds them; ``cut``: that many bytes fewer in the raw buffer"""
    parts, offs, o = [], [], 0
    for i, r in enumerate(reads):
        rec = _record(i, r)
        offs.append(o)
        parts.append(rec)
        o += len(rec)
    col = lambda k, dt: np.array([r[k] for r in reads], dtype=dt)
    raw = np.frombuffer(b"".join(parts), dtype=np.uint8)
    b = Batch(raw[:len(raw) - cut].copy(), flag=col("flag", np.uint16), tid=col("tid", np.int32), pos=col("pos", np.int32), mapq=col("mapq", np.uint8),
              rec_off=np.array(offs, dtype=np.uint64))
    # (not a column of tdt_pile_push: the end of the read on the reference as the decoder gives it, for tiddit_alleles.count_batch)
    b.end = np.array([r["pos"] + (sum(ln for op, ln in r["cigar"] if op in (0, 2, 3, 7, 8)) or 1) for r in reads], dtype=np.int64)
    return b


def batches(case):
    if "built" not in case:
        case["built"] = [build_batch(reads, cut) for reads, cut in case["batches"]]
    return case["built"]


def expected(case):
    """THE CLAIM: ([uint32[length] per contig], uint64[SIZE]) from the stated kinds and spans"""
    depth = [np.zeros(n, dtype=np.uint32) for n in case["lengths"]]
    c = dict.fromkeys(SN, 0)
    for reads, _ in case["batches"]:
        for r in reads:
            c["records"] += 1
            if r["kind"] == NOT_ELIGIBLE:
                continue
            c["eligible"] += 1
            c["malformed"] += r["kind"] == MALFORMED
            c["no_cigar"] += r["kind"] == NO_CIGAR
            c["clamped_spans"] += r["clamped"]
            for s, e in r["spans"]:
                assert 0 <= s < e <= case["lengths"][r["tid"]], (case["name"], r["tid"], s, e)
                depth[r["tid"]][s:e] += 1
                c["spans"] += 1
                c["covered_bases"] += e - s
    return depth, np.array([c[k] for k in SN], dtype=np.uint64)


def definition(case):
    """the same from tiddit_pileup's definition"""
    from tiddit_amd import tiddit_pileup
    spans, sn = [], {}
    for b in batches(case):
        tiddit_pileup.spans_of_batch(b, spans, sn, case["lengths"], case["Q"])
    return tiddit_pileup.depth_of(spans, case["lengths"]), tiddit_pileup.counters_of(sn)


def same(a, b):
    return len(a[0]) == len(b[0]) and all(x.dtype == y.dtype == np.uint32 and np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------- the cases
CASES = []


def case(name, family, claims, *pushes, lengths=LENGTHS, q=Q):
    CASES.append({"name": name, "family": family, "claims": claims, "lengths": tuple(lengths), "Q": q,
                  "batches": [(list(p[0]), p[1]) if isinstance(p, tuple) else (list(p), 0) for p in pushes]})


L8 = LENGTHS[B]
case("edges: base 0, the last base, past the end", "edges",
     "a read at base 0 covers it; a span that ends at the contig's length puts its -1 into the guard; a read running past the end is cut there "
     "(clamped); one that starts at or behind the length is dropped (clamped); the contigs of 1 and 2 bases hold their reads",
     [rd(pos=0, cigar="20M", spans=[(0, 20)]),
      rd(pos=L8 - 20, cigar="20M", spans=[(L8 - 20, L8)]),
      rd(pos=L8 - 10, cigar="20M", spans=[(L8 - 10, L8)], clamped=1),
      rd(pos=L8, cigar="10M", clamped=1),
      rd(pos=L8 + 10, cigar="10M", clamped=1),
      rd(pos=L8 - 5, cigar="10M5D10M", spans=[(L8 - 5, L8)], clamped=2),         # (the first span is cut, the second dropped)
      rd(tid=3, pos=0, cigar="1M", spans=[(0, 1)]),
      rd(tid=3, pos=0, cigar="3M", spans=[(0, 1)], clamped=1),
      rd(tid=3, pos=1, cigar="1M", clamped=1),
      rd(tid=4, pos=0, cigar="2M", spans=[(0, 2)]),
      rd(tid=4, pos=1, cigar="1M", spans=[(1, 2)]),
      rd(tid=5, pos=60, cigar="10M", spans=[(60, 63)], clamped=1),
      rd(tid=6, pos=0, cigar="64M", spans=[(0, 64)]),
      rd(tid=6, pos=64, cigar="4M", clamped=1),
      rd(tid=7, pos=1, cigar="64M", spans=[(1, 65)])])

_200 = [(0, 2), (2, 1)] * 100
case("cigar: every operation", "cigar",
     "M, = and X cover; an I or a P between two Ms leaves ONE span; D and N split; S and H do nothing; operations of length 0 change nothing "
     "(a 0D between two Ms leaves one span); a read that is all soft clip is eligible and covers nothing; 200 operations give 100 spans; a "
     "record with a CIGAR and no sequence counts",
     [rd(pos=100, cigar="5M5=5X", spans=[(100, 115)]),
      rd(pos=200, cigar="10M2I10M", spans=[(200, 220)]),
      rd(pos=300, cigar="10M3D10M", spans=[(300, 310), (313, 323)]),
      rd(pos=400, cigar="10M100N10M", spans=[(400, 410), (510, 520)]),
      rd(pos=600, cigar="5S10M5S", spans=[(600, 610)]),
      rd(pos=700, cigar="5H10M5H", spans=[(700, 710)]),
      rd(pos=800, cigar="10M2P10M", spans=[(800, 820)]),
      rd(pos=900, cigar="10M0D10M", spans=[(900, 920)]),
      rd(pos=1000, cigar="10M0M5D0I0N10M0S", spans=[(1000, 1010), (1015, 1025)]),
      rd(pos=1100, cigar="0M"),
      rd(pos=1200, cigar="20S"),
      rd(pos=1300, cigar="3I4D5M", spans=[(1304, 1309)]),
      rd(pos=2000, ops=_200, spans=[(2000 + 3 * k, 2002 + 3 * k) for k in range(100)]),
      rd(pos=3000, cigar="10M", seq="", spans=[(3000, 3010)]),
      rd(pos=3005, cigar="4M2D4M2I4M", flag=0x10 | 0x1 | 0x80, spans=[(3005, 3009), (3011, 3019)])])

case("gate: the flag bits, tid -1, MAPQ at the cut", "gate",
     "every bit of 0xF04 alone makes a record not eligible, the other flag bits do not; tid -1 is not eligible; MAPQ Q - 1 is not, Q is (>=)",
     [rd(pos=100, flag=f, kind=NOT_ELIGIBLE) for f in (0x4, 0x100, 0x200, 0x400, 0x800)]
     + [rd(pos=100, flag=f, spans=[(100, 120)]) for f in (0x1, 0x2, 0x8, 0x10, 0x20, 0x40, 0x80, 0xfb)]
     + [rd(pos=100, col_tid=-1, kind=NOT_ELIGIBLE), rd(pos=100, mapq=Q - 1, kind=NOT_ELIGIBLE), rd(pos=100, mapq=Q, spans=[(100, 120)]),
        rd(pos=100, mapq=0, kind=NOT_ELIGIBLE), rd(pos=100, mapq=255, spans=[(100, 120)])])

case("gate: a cut of 0 lets MAPQ 0 in", "gate", "with Q = 0 a read of MAPQ 0 is eligible",
     [rd(pos=50, mapq=0, spans=[(50, 70)]), rd(pos=50, flag=0x400, mapq=0, kind=NOT_ELIGIBLE)], q=0)

_ok = rd(pos=10, cigar="10M", spans=[(10, 20)])
case("malformed: op code, pos, tid, lengths, no CIGAR", "malformed",
     "op code 9; pos < 0; tid = n_contigs (and beyond); a query length that differs from l_seq; pos + the reference length above 2^31 - 1; "
     "l_seq < 0; a body larger than block_size — each is malformed and adds nothing else; n_cigar_op = 0 is no_cigar",
     [_ok,
      rd(pos=10, ops=[(0, 5), (9, 5), (0, 5)], kind=MALFORMED),
      rd(pos=10, ops=[(15, 10)], kind=MALFORMED),
      rd(pos=-1, cigar="10M", kind=MALFORMED),
      rd(pos=10, cigar="10M", col_tid=len(LENGTHS), kind=MALFORMED),
      rd(pos=10, cigar="10M", col_tid=len(LENGTHS) + 7, kind=MALFORMED),
      rd(pos=10, cigar="10M", seq="A" * 9, kind=MALFORMED),
      rd(pos=10, cigar="5S10M", seq="A" * 16, kind=MALFORMED),
      rd(pos=2 ** 31 - 11, cigar="20M", kind=MALFORMED),
      rd(pos=2 ** 31 - 21, cigar="20M", clamped=1),                              # (ends at 2^31 - 1: well formed, and wholly past the end)
      rd(pos=10, cigar="10M", patch=((20, "<i", -1),), kind=MALFORMED),
      rd(pos=10, cigar="10M", bs_delta=-1, kind=MALFORMED),
      rd(pos=10, cigar="", seq="ACGT", kind=NO_CIGAR),
      rd(pos=10, cigar="", seq="", kind=NO_CIGAR),
      _ok])

for _name, _cut, _why in (("the header ends behind raw", None, "rec_off + 36 > raw_len"), ("the block ends behind raw", 1, "rec_off + 4 + block_size > raw_len")):
    _last = rd(pos=40, cigar="10M", kind=MALFORMED)
    _n = len(_record(1, _last))
    case("malformed: " + _name, "malformed", "the last record of the buffer is cut (%s): malformed, nothing of it is read; the one in front counts" % _why,
         ([_ok, _last], _n - 30 if _cut is None else _cut))
case("malformed: a block_size that reaches behind raw", "malformed", "block_size + 1000: the block does not fit raw",
     [_ok, rd(pos=40, cigar="10M", bs_delta=1000, kind=MALFORMED)])

for _n in (64, 65, 300):
    case("same position: %d reads" % _n, "merge", "%d reads with the same start and end: the wave merges them, the depth is %d" % (_n, _n),
         [rd(pos=1000, cigar="50M", spans=[(1000, 1050)]) for _ in range(_n)])
case("same position: a depth of 3000 at one base", "merge", "3000 reads of 1M at one base, 7 of 10M over it",
     [rd(pos=5000, cigar="1M", spans=[(5000, 5001)]) for _ in range(3000)] + [rd(pos=4995, cigar="10M", spans=[(4995, 5005)]) for _ in range(7)])
case("same position: runs of equal starts beside other starts, unsorted ends", "merge",
     "neighbouring lanes with equal starts and unequal ends, the same start again in lanes that are not neighbours, eligible reads between "
     "reads that are not",
     [rd(pos=p, cigar="%dM" % n, spans=[(p, p + n)], flag=f) if f != 0x400 else rd(pos=p, cigar="%dM" % n, flag=f, kind=NOT_ELIGIBLE)
      for k in range(200) for p, n, f in ((700 + k // 7, 30 + k % 5, 0x400 if k % 11 == 0 else 0x10 * (k & 1)), (700, 10, 0), (705 + k % 3, 31, 0))])


def _mixed():
    out = []
    for k in range(310):
        p = 37 * k
        if k % 13 == 5:
            out.append(rd(pos=p, cigar="30M", flag=0x100, kind=NOT_ELIGIBLE))
        elif k % 13 == 7:
            out.append(rd(pos=p, cigar="20M10D20M", spans=[(p, p + 20), (p + 30, p + 50)]))
        elif k % 13 == 9:
            out.append(rd(tid=k % 8, pos=0, cigar="1M", spans=[(0, 1)]))
        else:
            out.append(rd(pos=p, cigar="40M", spans=[(p, p + 40)]))
    return out


_M = _mixed()
case("batches: one push", "batches", "310 reads in one batch", _M)
case("batches: two pushes", "batches", "the same reads in two batches give the same", _M[:129], _M[129:])
case("batches: seven pushes, one of them empty", "batches", "the same reads in seven batches, the third one empty, give the same",
     _M[:1], _M[1:65], [], _M[65:66], _M[66:130], _M[130:300], _M[300:])

_o = offsets()
_b1, _b2, _b3 = (k * TILE - _o[B] for k in range(_o[B] // TILE + 1, _o[B] // TILE + 4))
assert 0 < _b1 < _b2 < _b3 < L8                # the big contig's bases that are the first slot of a tile
case("tiles: spans across one, two and three borders, the guards at a tile's edges", "tiles",
     "a span over one, two and three tile borders carries its depth across them; contig 0 filled to its last base puts its -1 into the LAST slot of "
     "tile 0, contig 1 into the FIRST slot of tile 2, and neither leaks into the next contig; spans that start and end exactly on a border",
     [rd(pos=_b1 - 10, cigar="20M", spans=[(_b1 - 10, _b1 + 10)]),
      rd(pos=_b1 - 5, ops=[(0, TILE + 10)], seq="", spans=[(_b1 - 5, _b2 + 5)]),
      rd(pos=_b1 - 1, ops=[(0, 2 * TILE + 2)], seq="", spans=[(_b1 - 1, _b3 + 1)]),
      rd(pos=_b1, ops=[(0, TILE)], seq="", spans=[(_b1, _b2)]),
      rd(pos=_b2 - 1, cigar="1M", spans=[(_b2 - 1, _b2)]),
      rd(pos=_b2, cigar="1M", spans=[(_b2, _b2 + 1)]),
      rd(tid=0, pos=0, ops=[(0, TILE - 1)], seq="", spans=[(0, TILE - 1)]),
      rd(tid=0, pos=TILE - 2, cigar="5M", spans=[(TILE - 2, TILE - 1)], clamped=1),
      rd(tid=1, pos=0, ops=[(0, TILE)], seq="", spans=[(0, TILE)]),
      rd(tid=1, pos=TILE - 1, cigar="1M", spans=[(TILE - 1, TILE)]),
      rd(tid=2, pos=0, ops=[(0, TILE + 1)], seq="", spans=[(0, TILE + 1)]),
      rd(tid=2, pos=TILE, cigar="3M", spans=[(TILE, TILE + 1)], clamped=1)])

_C0 = CARRY_LENGTHS[0]
case("carry: a depth carried over more than 256 tiles", "carry",
     "one span over 257 tiles: the carry kernel loops, and the depth 1 (2 and 3 where short reads lie) holds from the first tile to the last; the "
     "small contig behind it starts at 0 again",
     [rd(tid=0, pos=10, ops=[(0, 257 * TILE - 20)], seq="", spans=[(10, 257 * TILE - 10)]),
      rd(tid=0, pos=100 * TILE - 3, cigar="6M", spans=[(100 * TILE - 3, 100 * TILE + 3)]),
      rd(tid=0, pos=256 * TILE - 1, cigar="2M", spans=[(256 * TILE - 1, 256 * TILE + 1)]),
      rd(tid=0, pos=256 * TILE, cigar="1M", spans=[(256 * TILE, 256 * TILE + 1)]),
      rd(tid=0, pos=_C0 - 1, cigar="1M", spans=[(_C0 - 1, _C0)]),
      rd(tid=1, pos=0, cigar="10M", spans=[(0, 10)]),
      rd(tid=1, pos=95, cigar="10M", spans=[(95, 100)], clamped=1)],
     lengths=CARRY_LENGTHS)

N_CASES = len(CASES)
FAMILIES = ("edges", "cigar", "gate", "malformed", "merge", "batches", "tiles", "carry")
assert {c["family"] for c in CASES} == set(FAMILIES)

# ------------------------------------------------------------------------------------------- the genotype rule: literal claims
# (SUPPORT, DP0) -> (DP0, OTHER, PL0, PL1, PL2, GT index, GQ, 1 when SUPPORT > DP0), each worked out by hand from
# L = (20 ALT, 3 (ALT + OTHER), 20 OTHER)
RULE = (
    ("(0, 0): nothing at all, all three tie", 0, 0, (0, 0, 0, 0, 0, 0, 0, 0)),
    ("(1, 0)", 1, 1, (1, 0, 20, 3, 0, 2, 3, 0)),
    ("(3, 17): L = 60, 60, 340, the tie goes to 0/0", 3, 20, (20, 17, 0, 0, 280, 0, 0, 0)),
    ("(17, 3): L = 340, 60, 60, the tie goes to 0/1", 17, 20, (20, 3, 280, 0, 0, 1, 0, 0)),
    ("(5, 5)", 5, 10, (10, 5, 70, 0, 70, 1, 70, 0)),
    ("(10, 0)", 10, 10, (10, 0, 200, 30, 0, 2, 30, 0)),
    ("(3, 27)", 3, 30, (30, 27, 0, 30, 480, 0, 30, 0)),
    ("support above the depth: OTHER is 0", 5, 2, (2, 0, 100, 15, 0, 2, 15, 1)),
    ("GQ 19: L = 40, 21, 100", 2, 7, (7, 5, 19, 0, 79, 1, 19, 0)),
    ("GQ 20: L = 80, 60, 320", 4, 20, (20, 16, 20, 0, 260, 1, 20, 0)),
    ("GQ 99 exactly: L = 180, 81, 360", 9, 27, (27, 18, 99, 0, 279, 1, 99, 0)),
    ("GQ above 99 is 99: L = 200, 60, 200", 10, 20, (20, 10, 140, 0, 140, 1, 99, 0)),
    ("PL at the cap: L = 20000, 3000, 0", 1000, 1000, (1000, 0, 9999, 3000, 0, 2, 99, 0)),
    ("PL at the cap on the other side: L = 0, 3000, 20000", 0, 1000, (1000, 1000, 0, 3000, 9999, 0, 99, 0)),
    ("a support of 2^32 - 1 needs 64 bits", 2 ** 32 - 1, 0, (0, 0, 9999, 9999, 0, 2, 99, 1)),
)
RULE_BEHIND_THE_END = ("P - 1 equal to the contig's length: DP0 is 0", 4, (0, 0, 80, 12, 0, 2, 12, 1))


def rule_case():
    """the rule's claims as a depth to push and rows to genotype: claim k sits at base 100 + 50 k of the big contig, where DP0 reads of
    1M lie; the last row is RULE_BEHIND_THE_END at P = 65 of the contig of 64 bases -> (case, K1 uint64[], SUPPORT uint32[], uint32[n][8])"""
    reads, k1, sup, want = [], [], [], []
    for k, (_, alt, dp0, cols) in enumerate(RULE):
        p = 100 + 50 * k
        reads += [rd(pos=p, cigar="1M", spans=[(p, p + 1)]) for _ in range(dp0)]
        k1.append(B << 32 | (p + 1))
        sup.append(alt)
        want.append(cols)
    reads.append(rd(tid=6, pos=0, cigar="64M", spans=[(0, 64)]))
    k1.append(6 << 32 | 65)
    sup.append(RULE_BEHIND_THE_END[1])
    want.append(RULE_BEHIND_THE_END[2])
    c = {"name": "rule", "family": "rule", "claims": "the depth the rule's claims are gathered from", "lengths": LENGTHS, "Q": Q, "batches": [(reads, 0)]}
    return c, np.array(k1, dtype=np.uint64), np.array(sup, dtype=np.uint32), np.array(want, dtype=np.uint32)
