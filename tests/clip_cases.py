"""Aimed cases for the clipped-read breakpoint sites (tiddit_amd/tiddit_clips.py, csrc/tdt_clip.hip): records built byte by byte with
``bamio.encode_record``, each case with the keys and counters it claims, written down from what the case PLANTED (which bases were put
into which clip, on which strand, at which position) and from the kind each read is stated to have — never computed by the definition
or by the restatement of tests/test_clip_refs_cpu.py.  Cases aimed at the vote also state their rows literally.

A case is a dict: ``batches`` (the pushes, in order: lists of reads, each list over its own raw buffer, optionally ``(reads, cut)`` with
that many bytes fewer in the buffer), ``capacity`` (of the store at its creation), ``Q`` / ``L`` (of the handle), ``S`` (the minimum
supports the finish is asked for), ``family``, ``claims`` (a sentence) and ``rows`` ({S: literal rows} or None).  A read (:func:`rd`) is
``[H hl] [S lead] M m [S trail] [H ht]`` with the clips' bases given in read order; its claim follows from them (:func:`outward`), or is
stated by the read itself (``events`` / ``short`` / ``cut``) where the record is patched.  A literal row is
``(tid, P, side, SUPPORT, REV, SEQS, CLEN, consensus outward from the breakpoint, AGREE, TOTAL)``."""
import collections
import os
import re
import struct

import numpy as np

from tiddit_amd import bamio

SN = ("records", "eligible", "malformed", "no_sequence", "no_alignment", "short_clips", "left_clips", "right_clips", "clipped_reads",
      "cut_at_other_base", "distinct_sequences", "distinct_sites", "reported_sites")
SIZE = 13
PUSH_SN = SN[:10]
COLUMNS = ("flag", "tid", "pos", "mapq", "rec_off")
REV = 0x10
COLS = 28
NOT_ELIGIBLE, MALFORMED, NO_SEQUENCE, NO_ALIGNMENT, OK = "not_eligible", "malformed", "no_sequence", "no_alignment", "ok"
L_SIDE, R_SIDE = 0, 1
NAME_LEN = 5                                  # "r000" and its NUL: CIGAR word j of a record lies at byte 36 + 5 + 4 j
MAX_TID, MAX_END = 2 ** 24 - 1, 2 ** 31 - 1
ROW_DTYPES = (np.uint64, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint64, np.uint64, np.uint64)


def cig_at(j):
    return 36 + NAME_LEN + 4 * j


def bases(n, start=0):
    """n bases cycling A C G T from ``start``"""
    return "".join("ACGT"[(start + k) % 4] for k in range(n))


def outward(clip, side):
    """what the definition's rule 5 keeps of a clip given in read order: outward from the breakpoint, up to the first base that is not
    A C G T, 28 at most"""
    s = clip[::-1] if side == L_SIDE else clip
    keep = ""
    for ch in s[:COLS]:
        if ch not in "ACGT":
            break
        keep += ch
    return keep


# ------------------------------------------------------------------------------------------- a read and what is planted in it
def rd(tid=0, pos=100, lead="", m=20, trail="", hl=0, ht=0, flag=0, mapq=60, kind=OK, ops=None, seq=None, patch=(), bs_delta=0, events=None, short=None,
       cut=None):
    """``lead`` / ``trail``: the clips' bases in read order; ``hl`` / ``ht``: hard clips outside them; ``ops`` / ``seq``: the CIGAR [(op, len)]
    and the bases instead of the built ones; ``patch``: ((byte offset in the record, struct format, value), ...); ``bs_delta``: added to
    block_size; ``kind``: what the case STATES the definition makes of the read; ``events`` [(side, P, kept bases outward)], ``short``,
    ``cut``: stated by the read instead of following from its clips"""
    cig = [(5, hl)] * bool(hl) + [(4, len(lead))] * bool(lead) + [(0, m)] * bool(m) + [(4, len(trail))] * bool(trail) + [(5, ht)] * bool(ht)
    return {"cigar": cig if ops is None else list(ops), "flag": flag, "tid": tid, "pos": pos, "mapq": mapq,
            "seq": lead + bases(m, 1) + trail if seq is None else seq, "patch": tuple(patch), "bs_delta": bs_delta, "kind": kind, "lead": lead, "trail": trail,
            "m": m, "events": events, "short": short, "cut": cut}


def _record(i, r):
    near = 0 <= r["pos"] < 2 ** 29 and 0 <= r["tid"] < 2 ** 15       # (a far pos or tid does not fit the helper's fields: written afterwards)
    rec = bytearray(bamio.encode_record("r%03d" % (i % 1000), r["flag"], r["tid"] if near else 0, r["pos"] if near else 0, r["mapq"], r["cigar"], -1, -1, 0,
                                        seq=r["seq"]))
    struct.pack_into("<ii", rec, 4, r["tid"], r["pos"])
    if r["bs_delta"]:
        struct.pack_into("<I", rec, 0, len(rec) - 4 + r["bs_delta"])
    for off, fmt, val in r["patch"]:
        struct.pack_into(fmt, rec, off, val)
    return bytes(rec)


class Batch:
    """the columns of a run of reads over one raw buffer — what tdt_clip_push and the definition take"""

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
    return Batch(raw[:len(raw) - cut].copy(), flag=col("flag", np.uint16), tid=col("tid", np.int32), pos=col("pos", np.int32), mapq=col("mapq", np.uint8),
                 rec_off=np.array(offs, dtype=np.uint64))


def batches(case):
    if "built" not in case:
        case["built"] = [build_batch(reads, cut) for reads, cut in case["batches"]]
    return case["built"]


# ------------------------------------------------------------------------------------------- the claim
def K1(tid, P):
    return tid * 2 ** 32 + P


def K2(side, kept, rev=0):
    return side * 2 ** 63 + len(kept) * 2 ** 58 + sum("ACGT".index(ch) * 4 ** j for j, ch in enumerate(kept)) * 4 + rev


def key_rows(keys):
    """[(K1, K2)] -> the sorted rows, uint64[n][2]"""
    return np.array(sorted(keys), dtype=np.uint64).reshape(-1, 2)


def row_columns(rows):
    """[(K1, side, SUPPORT, REV, SEQS, CLEN, consensus, AGREE, TOTAL)] -> the nine columns as tdt_clip_rows gives them"""
    return tuple(np.array([r[k] for r in rows], dtype=dt) for k, dt in enumerate(ROW_DTYPES))


def literal_rows(rows):
    """literal rows (see the module docstring) -> row tuples as the definition's summarise gives them"""
    return [(K1(tid, P), side, sup, rev, seqs, clen, sum("ACGT".index(ch) * 4 ** j for j, ch in enumerate(cons)), agree, total)
            for tid, P, side, sup, rev, seqs, clen, cons, agree, total in rows]


def claimed(case):
    """-> (keys [(K1, K2)], sn {name: n}: the push counters) from what the case planted and states"""
    keys, sn = [], collections.Counter()
    for reads, _ in case["batches"]:
        for r in reads:
            sn["records"] += 1
            if r["kind"] == NOT_ELIGIBLE:
                continue
            sn["eligible"] += 1
            if r["kind"] != OK:
                sn[{MALFORMED: "malformed", NO_SEQUENCE: "no_sequence", NO_ALIGNMENT: "no_alignment"}[r["kind"]]] += 1
                continue
            events, short, cut = r["events"], r["short"], r["cut"]
            if events is None:
                events, short, cut = [], 0, 0
                for side, clip, P in ((L_SIDE, r["lead"], r["pos"] + 1), (R_SIDE, r["trail"], r["pos"] + r["m"])):
                    if clip and len(clip) < case["L"]:
                        short += 1
                    elif clip:
                        kept = outward(clip, side)
                        cut += len(kept) < min(len(clip), COLS)
                        events.append((side, P, kept))
            sn["short_clips"] += short
            sn["cut_at_other_base"] += cut
            sn["left_clips"] += sum(1 for e in events if e[0] == L_SIDE)
            sn["right_clips"] += sum(1 for e in events if e[0] == R_SIDE)
            sn["clipped_reads"] += bool(events)
            rev = 1 if r["flag"] & REV else 0
            keys += [(K1(r["tid"], P), K2(side, kept, rev)) for side, P, kept in events]
    return keys, +sn


def push_counters(sn):
    c = np.zeros(SIZE, dtype=np.uint64)
    for k, v in sn.items():
        c[SN.index(k)] = v
    return c


def definition(case):
    """the definition over the case's batches -> (sorted key rows, {S: (counters, row columns)})"""
    from tiddit_amd import tiddit_clips
    keys, sn = [], {}
    for b in batches(case):
        tiddit_clips.keys_of_batch_by_read(b, keys, sn, case["Q"], case["L"])
    out = {}
    for S in case["S"]:
        c, rows = tiddit_clips.summarise(keys, sn, S)
        out[S] = (c, row_columns(rows))
    return key_rows(keys), out


def same(a, b):
    return (a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and set(a[1]) == set(b[1]) and
            all(np.array_equal(a[1][S][0], b[1][S][0]) and all(np.array_equal(x, y) for x, y in zip(a[1][S][1], b[1][S][1])) for S in a[1]))


def agrees_with_claim(case, got):
    """``got`` (of :func:`definition`, of the restatement, of the device) against the claim: the keys as a multiset, the ten push counters
    for every S, the literal rows where the case states them -> None or what differs"""
    keys, sn = claimed(case)
    if not np.array_equal(got[0], key_rows(keys)):
        return "keys"
    want = push_counters(sn)
    for S in case["S"]:
        c, cols = got[1][S]
        if not np.array_equal(c[:10], want[:10]):
            return "push counters at S=%d: %s / %s" % (S, c[:10].tolist(), want[:10].tolist())
        if c[10] != len({(k1, k2 >> 1) for k1, k2 in keys}) or c[11] != len({(k1, k2 >> 63) for k1, k2 in keys}) or c[12] != len(cols[0]):
            return "set counters at S=%d: %s" % (S, c[10:].tolist())
        if case["rows"] is not None and S in case["rows"]:
            lit = row_columns(literal_rows(case["rows"][S]))
            for name, x, y in zip(("K1", "SIDE", "SUPPORT", "REV", "SEQS", "CLEN", "CONSENSUS", "AGREE", "TOTAL"), cols, lit):
                if x.shape != y.shape or not np.array_equal(x, y):
                    return "rows at S=%d, %s: %s / %s" % (S, name, x.tolist(), y.tolist())
    return None


# ------------------------------------------------------------------------------------------- the cases
CASES = []


def case(family, name, claims, batches_, Q=20, L=10, S=(1, 2, 3), capacity=1 << 12, rows=None):
    bs = [(b, 0) if isinstance(b, list) else b for b in batches_]
    CASES.append({"family": family, "name": family + ": " + name, "claims": claims, "batches": bs, "Q": Q, "L": L, "S": S, "capacity": capacity, "rows": rows})


A28, C28 = "A" * 28, "C" * 28

# ---- clip lengths around L and around the 28 columns
case("length", "clips of L - 1, L and L + 1 bases on both sides",
     "a clip of 9 bases is short and no event; 10 and 11 are events with n = 10 and 11; on both sides",
     [[rd(pos=100 + 10 * k, lead=bases(n, k)) for k, n in enumerate((9, 10, 11))] + [rd(pos=300 + 10 * k, trail=bases(n, k)) for k, n in enumerate((9, 10, 11))]])
case("length", "clips of 27, 28, 29 and 65535 bases on both sides",
     "n is min(cliplen, 28); the 29th base and everything beyond are not stored, so 28, 29 and 65535 A's are one sequence; nothing is cut",
     [[rd(pos=500, lead="A" * n) for n in (27, 28, 29, 65535)] + [rd(pos=500, trail="A" * n, flag=REV) for n in (27, 28, 29, 65535)]],
     rows={2: [(0, 501, L_SIDE, 4, 0, 2, 28, A28, 3 + 4 * 27, 3 + 4 * 27), (0, 520, R_SIDE, 4, 4, 2, 28, A28, 3 + 4 * 27, 3 + 4 * 27)]})
case("length", "L = 1",
     "with L = 1 a clip of one base is an event; G and A tie at column 0 of the L site (A wins), column 1 is reached by one read",
     [[rd(pos=40, lead="G"), rd(pos=40, trail="T"), rd(pos=40, lead="GA", trail="TC")]], L=1,
     rows={1: [(0, 41, L_SIDE, 2, 0, 2, 2, "AG", 2, 3), (0, 60, R_SIDE, 2, 0, 2, 2, "TC", 3, 3)]})
case("length", "L = 65535", "a clip of 65534 bases is short, one of 65535 is an event",
     [[rd(pos=40, lead="C" * 65534), rd(pos=40, trail="C" * 65535)]], L=65535, S=(1,),
     rows={1: [(0, 60, R_SIDE, 1, 0, 1, 28, C28, 28, 28)]})

# ---- nibble phases
case("phase", "a clip starting on an even and on an odd query index, on both sides",
     "a leading clip is read backwards from query index cliplen - 1 (odd for 12, even for 13 bases); a trailing clip forwards from l_seq - cliplen "
     "(even and odd with m = 20 and 21): the kept bases are the planted ones outward from the breakpoint whatever the nibble",
     [[rd(pos=100, lead="ACGTTGCAACGT"), rd(pos=150, lead="ACGTTGCAACGTC"), rd(pos=200, m=20, trail="CATGGTACCATG"), rd(pos=200, m=21, trail="CATGGTACCATG"),
       rd(pos=300, lead="TTGCAACGTTGC", m=21, trail="GGATCCAATTGG", flag=REV)]],
     rows={1: [(0, 101, L_SIDE, 1, 0, 1, 12, "TGCAACGTTGCA", 12, 12), (0, 151, L_SIDE, 1, 0, 1, 13, "CTGCAACGTTGCA", 13, 13), (0, 220, R_SIDE, 1, 0, 1, 12, "CATGGTACCATG", 12, 12),
               (0, 221, R_SIDE, 1, 0, 1, 12, "CATGGTACCATG", 12, 12), (0, 301, L_SIDE, 1, 1, 1, 12, "CGTTGCAACGTT", 12, 12),
               (0, 321, R_SIDE, 1, 1, 1, 12, "GGATCCAATTGG", 12, 12)]})

# ---- other bases
_N = lambda clip, j, side: (clip[:len(clip) - 1 - j] + "N" + clip[len(clip) - j:]) if side == L_SIDE else clip[:j] + "N" + clip[j + 1:]
case("other", "a non-ACGT base at column 0, 1 and 27, and none",
     "the kept bases end in front of the first base that is not A C G T: n = 0 (still an event), 1, 27 and 28; the first three are cut; a clip of "
     "12 bases with an N at its column 11 keeps 11 and is cut",
     [[rd(pos=100, lead=_N(bases(30), j, L_SIDE)) for j in (0, 1, 27)] + [rd(pos=100, lead=bases(30))] +
      [rd(pos=100, trail=_N(bases(30), j, R_SIDE), flag=REV) for j in (0, 1, 27)] + [rd(pos=100, trail=bases(30), flag=REV), rd(pos=100, trail=_N(bases(12), 11, R_SIDE))]])
case("other", "every code that is not A C G T ends the kept bases",
     "= M R S V W Y H K D B N at column 3 of a trailing clip: n = 3 each, one distinct sequence, twelve cut clips",
     [[rd(pos=700, trail="ACG" + ch + "ACGTACGT") for ch in "=MRSVWYHKDBN"]],
     rows={3: [(0, 720, R_SIDE, 12, 0, 1, 3, "ACG", 36, 36)]})

# ---- hard clips, all-S, which operation is the clip
case("hard", "H S M, M S H, H M, M H and S alone",
     "an S behind a leading H and in front of a trailing H is the clip; H alone is no clip; a CIGAR of S alone has no reference length",
     [[rd(pos=100, hl=5, lead=bases(12)), rd(pos=100, trail=bases(12), ht=7), rd(pos=100, hl=30), rd(pos=100, ht=30), rd(pos=100, hl=3, lead=bases(11), trail=bases(13, 2), ht=4),
       rd(pos=100, ops=[(4, 20)], seq=bases(20), kind=NO_ALIGNMENT), rd(pos=100, ops=[(5, 3), (4, 20), (5, 3)], seq=bases(20), kind=NO_ALIGNMENT),
       rd(pos=100, ops=[(4, 12), (1, 8)], seq=bases(20), kind=NO_ALIGNMENT)]])
case("hard", "an S that is not at the edge is no clip",
     "M S M (index 1 behind an M), S S M (only index 0) and H H S M (index 2): the inner S is neither a clip nor short",
     [[rd(pos=100, ops=[(0, 10), (4, 12), (0, 10)], seq=bases(32), events=[], short=0, cut=0),
       rd(pos=100, ops=[(4, 12), (4, 11), (0, 10)], seq="A" * 12 + "C" * 11 + bases(10), events=[(L_SIDE, 101, "A" * 12)], short=0, cut=0),
       rd(pos=100, ops=[(0, 10), (4, 11), (4, 12)], seq=bases(10) + "C" * 11 + "G" * 12, events=[(R_SIDE, 110, "G" * 12)], short=0, cut=0),
       rd(pos=100, ops=[(5, 2), (5, 2), (4, 12), (0, 10)], seq="T" * 12 + bases(10), events=[], short=0, cut=0)]])
case("both", "S M S with both clips kept, with one kept and one short, with both short",
     "a read gives at most two events; clipped_reads counts the read once; a short clip beside a kept one is counted as short",
     [[rd(pos=100, lead=bases(12), trail=bases(14, 1)), rd(pos=100, lead=bases(9), trail=bases(14, 1)), rd(pos=100, lead=bases(12), trail=bases(3)),
       rd(pos=100, lead=bases(2), trail=bases(3))]])

# ---- records without sequence or CIGAR, malformed records
case("nothing", "l_seq == 0 and n_cigar_op == 0",
     "no_sequence, no event: a CIGAR without bases, and bases without a CIGAR",
     [[rd(pos=100, ops=[(4, 12), (0, 20)], seq="", kind=NO_SEQUENCE), rd(pos=100, ops=[], seq=bases(32), kind=NO_SEQUENCE), rd(pos=100, lead=bases(12))]])
_bad = lambda **kw: rd(kind=MALFORMED, **kw)
case("malformed", "each condition",
     "an op code of 9; tid = 2^24 in the column; pos = -1; a reference end of 2^31; a query length that differs from l_seq (too long, too short); a negative "
     "l_seq; a body beyond block_size; one well-formed clipped read among them",
     [[_bad(pos=100, lead=bases(12), patch=((cig_at(1), "<I", 20 << 4 | 9),)), _bad(tid=2 ** 24, pos=100, lead=bases(12)), _bad(pos=-1, lead=bases(12)),
       _bad(pos=MAX_END - 19, lead=bases(12)), _bad(pos=100, lead=bases(12), patch=((cig_at(0), "<I", 13 << 4 | 4),)),
       _bad(pos=100, lead=bases(12), patch=((cig_at(1), "<I", 19 << 4 | 0),)), _bad(pos=100, lead=bases(12), patch=((20, "<i", -1),)),
       _bad(pos=100, lead=bases(12), bs_delta=-1), rd(pos=100, lead=bases(12))]])
case("malformed", "a block that reaches beyond the raw bytes, a header that does",
     "the last record's block ends one byte behind raw_len (first push); only 35 bytes of the last record's header are inside (second push)",
     [([rd(pos=100, lead=bases(12)), _bad(pos=100, lead=bases(12))], 1),
      ([rd(pos=100, lead=bases(12)), _bad(pos=100, lead=bases(12))], len(bamio.encode_record("r001", 0, 0, 100, 60, [(4, 12), (0, 20)], -1, -1, 0, seq=bases(32))) - 35)])

# ---- filters
case("filter", "each filter bit, tid = -1, mapq at Q - 1 and at Q",
     "0x4, 0x100, 0x200, 0x400 and 0x800 each make a record not eligible, and so do tid = -1 and mapq = 19; mapq = 20 is eligible; the paired and "
     "strand bits do not matter",
     [[rd(pos=100, lead=bases(12), flag=f, kind=NOT_ELIGIBLE) for f in (0x4, 0x100, 0x200, 0x400, 0x800, 0x904)] +
      [rd(tid=-1, pos=100, lead=bases(12), kind=NOT_ELIGIBLE), rd(pos=100, lead=bases(12), mapq=19, kind=NOT_ELIGIBLE), rd(pos=100, lead=bases(12), mapq=20),
       rd(pos=100, lead=bases(12), flag=0x1 | 0x2 | 0x20 | 0x40), rd(pos=100, lead=bases(12), flag=0x1 | 0x10 | 0x80)]])
case("filter", "Q = 0 and Q = 255", "with Q = 0 a MAPQ of 0 is eligible; with Q = 255 only 255 is",
     [[rd(pos=100, lead=bases(12), mapq=0), rd(pos=100, lead=bases(12), mapq=255)]], Q=0)
case("filter", "Q = 255", "with Q = 255 only a MAPQ of 255 is eligible",
     [[rd(pos=100, lead=bases(12), mapq=254, kind=NOT_ELIGIBLE), rd(pos=100, lead=bases(12), mapq=255)]], Q=255)

# ---- strands, sides, contigs, the largest keys
case("strand", "both strands at one site",
     "REV counts the reverse reads of a site; two reads with one sequence on two strands are ONE distinct sequence",
     [[rd(pos=100, lead=bases(12)), rd(pos=100, lead=bases(12), flag=REV), rd(pos=100, lead=bases(12), flag=REV), rd(pos=100, lead=bases(12, 1), flag=REV)]],
     rows={1: [(0, 101, L_SIDE, 4, 3, 2, 12, bases(12)[::-1], 36, 48)], 3: [(0, 101, L_SIDE, 4, 3, 2, 12, bases(12)[::-1], 36, 48)]})
case("site", "an L and an R site on one P, equal P on two contigs",
     "P = 120 is the first aligned base of two reads and the last aligned base of two others: two sites, L first; the same on contig 3 is two more",
     [[rd(tid=t, pos=119, lead="G" * 12) for t in (0, 3) for _ in range(2)] + [rd(tid=t, pos=100, trail="T" * 12) for t in (3, 0) for _ in range(2)]],
     rows={2: [(0, 120, L_SIDE, 2, 0, 1, 12, "G" * 12, 24, 24), (0, 120, R_SIDE, 2, 0, 1, 12, "T" * 12, 24, 24),
               (3, 120, L_SIDE, 2, 0, 1, 12, "G" * 12, 24, 24), (3, 120, R_SIDE, 2, 0, 1, 12, "T" * 12, 24, 24)]})
case("site", "the largest legal tid and P",
     "tid = 2^24 - 1 and a reference end of 2^31 - 1: the trailing clip's P is 2^31 - 1, the leading clip's 2^31 - 20",
     [[rd(tid=MAX_TID, pos=MAX_END - 20, lead="C" * 12, trail="A" * 12)]], S=(1,),
     rows={1: [(MAX_TID, MAX_END - 19, L_SIDE, 1, 0, 1, 12, "C" * 12, 12, 12), (MAX_TID, MAX_END, R_SIDE, 1, 0, 1, 12, "A" * 12, 12, 12)]})

# ---- the vote
case("vote", "a tie of 2 against 2",
     "column 0 holds 2 x C and 2 x A, column 1 2 x T and 2 x G: the smaller code wins (A, G); column 2 holds 3 x T and 1 x C",
     [[rd(pos=100, trail="CTT" + "A" * 9), rd(pos=100, trail="AGT" + "A" * 9), rd(pos=100, trail="CGT" + "A" * 9), rd(pos=100, trail="ATC" + "A" * 9)]], S=(1, 4),
     rows={1: [(0, 120, R_SIDE, 4, 0, 4, 12, "AGT" + "A" * 9, 2 + 2 + 3 + 36, 48)], 4: [(0, 120, R_SIDE, 4, 0, 4, 12, "AGT" + "A" * 9, 2 + 2 + 3 + 36, 48)]})
case("vote", "a tie of 2 against 2 on the left side, the larger code seen first",
     "the same with the reads in another order and on the L side: T and G tie at column 0 (G wins), the consensus is written outward",
     [[rd(pos=100, lead="A" * 11 + "T"), rd(pos=100, lead="A" * 11 + "G"), rd(pos=100, lead="A" * 11 + "T"), rd(pos=100, lead="A" * 11 + "G")]], S=(2,),
     rows={2: [(0, 101, L_SIDE, 4, 0, 2, 12, "G" + "A" * 11, 2 + 44, 48)]})
_OUT = bases(30)[::-1]                        # a leading clip of bases(30), outward from the breakpoint
for _c in (1, 14, 27):
    case("depth", "depth falls from S to S - 1 at column %d" % _c,
         "three reads at S = 3: two keep 28 bases, one keeps %d: CLEN = %d at S = 3, 28 at S = 2" % (_c, _c),
         [[rd(pos=100, trail=bases(30)), rd(pos=100, trail=bases(30), flag=REV), rd(pos=100, trail=_N(bases(30), 1, R_SIDE) if _c == 1 else bases(_c))]],
         rows={3: [(0, 120, R_SIDE, 3, 1, 2, _c, bases(_c), 3 * _c, 3 * _c)], 2: [(0, 120, R_SIDE, 3, 1, 2, 28, bases(28), 56 + _c, 56 + _c)]})
    case("depth", "depth falls from S to S - 1 at column %d, left side" % _c,
         "the same on the L side: the columns are counted from the breakpoint, that is from the clip's LAST base",
         [[rd(pos=100, lead=bases(30)), rd(pos=100, lead=bases(30), flag=REV), rd(pos=100, lead=_N(bases(30), 1, L_SIDE) if _c == 1 else bases(30)[30 - _c:])]],
         rows={3: [(0, 101, L_SIDE, 3, 1, 2, _c, _OUT[:_c], 3 * _c, 3 * _c)], 2: [(0, 101, L_SIDE, 3, 1, 2, 28, _OUT[:28], 56 + _c, 56 + _c)]})
case("support", "a site whose SUPPORT is reached only by adding distinct sequences",
     "three reads with three different clips at one site: three distinct sequences of support 1 each, one site of SUPPORT 3, reported at S = 3; at "
     "S = 3 only the columns all three reach count (10)",
     [[rd(pos=100, trail="ACGTACGTAC"), rd(pos=100, trail="ACGTACGTACG"), rd(pos=100, trail="ACGTTCGTACGT")]],
     rows={3: [(0, 120, R_SIDE, 3, 0, 3, 10, "ACGTACGTAC", 29, 30)], 2: [(0, 120, R_SIDE, 3, 0, 3, 11, "ACGTACGTACG", 31, 32)],
           1: [(0, 120, R_SIDE, 3, 0, 3, 12, "ACGTACGTACGT", 32, 33)]})
case("support", "a site with SUPPORT = S - 1",
     "two reads at one site and three at another: at S = 3 the first is a distinct site and not a reported one",
     [[rd(pos=100, trail="G" * 12), rd(pos=100, trail="G" * 12), rd(pos=200, trail="G" * 12), rd(pos=200, trail="G" * 12), rd(pos=200, trail="G" * 12)]],
     rows={3: [(0, 220, R_SIDE, 3, 0, 1, 12, "G" * 12, 36, 36)], 2: [(0, 120, R_SIDE, 2, 0, 1, 12, "G" * 12, 24, 24), (0, 220, R_SIDE, 3, 0, 1, 12, "G" * 12, 36, 36)]})

# ---- the store: more than one push, more than one workgroup, growth
_many = [rd(tid=k % 3, pos=1000 + 7 * (k % 41), lead=bases(10 + k % 23, k % 4) if k % 3 else "", trail=bases(10 + k % 19, k % 3) if k % 2 else "",
            flag=REV if k % 5 == 0 else 0, mapq=19 + k % 4, kind=OK if k % 4 else NOT_ELIGIBLE) for k in range(700)]
case("store", "700 reads in three pushes, a store made for 64 keys",
     "40 reads need 80 slots of a store of 64 (it grows), the next 560 (three workgroups of reads) need 1120 more (it grows again), the last 100 "
     "fit behind the real count; lengths 10 ... 32, both sides, both strands, every fourth read below the MAPQ cut",
     [_many[:40], _many[40:600], _many[600:]], capacity=64)

# ---- the workgroup of clip_keys: the compaction, the staging and the emit on their edges
# the reads of a clip_keys workgroup, from the `#define` line of csrc/tdt_clip.hip: the cases stay on its edges when it is retuned
CLIP_BLOCK = int(re.search(r"^[ \t]*#[ \t]*define[ \t]+CLIP_K_TILE[ \t]+([0-9]+)[ \t]*(?://[^\n]*)?$",
                           open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiddit_amd", "csrc", "tdt_clip.hip")).read(), re.M).group(1))
for _n in (CLIP_BLOCK - 1, CLIP_BLOCK, CLIP_BLOCK + 1):
    case("store", "%d reads with one clip each" % _n,
         "a batch of one workgroup less one read, of exactly one, and of one read more (a second workgroup with a single read); every seventh read "
         "is below the MAPQ cut, so the compaction moves the reads behind it; leading and trailing clips alternate",
         [[rd(pos=2000 + 3 * (k % 50), lead=bases(12, k % 4) if k % 2 else "", trail="" if k % 2 else bases(11 + k % 3, k % 3), flag=REV * (k % 3 == 0),
              mapq=3 if k % 7 == 3 else 60, kind=NOT_ELIGIBLE if k % 7 == 3 else OK) for k in range(_n)]])
case("store", "every read of two workgroups has both clips",
     "512 reads with a leading and a trailing clip of at least L bases: the staging of both workgroups is full at two keys per read, and the "
     "store, made for exactly 2 x 512 keys, is full too",
     [[rd(pos=3000 + k % 20, lead=bases(10 + k % 5, k % 4), trail=bases(10 + k % 4, k % 3), flag=REV * (k & 1)) for k in range(2 * CLIP_BLOCK)]],
     S=(1, 3), capacity=2 * 2 * CLIP_BLOCK)
case("store", "only the last lane of each workgroup holds an eligible read",
     "513 reads, read k eligible only for k % 256 == 255: the compaction hands that read to lane 0, three waves of each workgroup emit nothing, and "
     "the third workgroup holds one ineligible read and emits no key",
     [[rd(pos=4000, lead=bases(12), trail=bases(12, 1), mapq=60 if k % CLIP_BLOCK == CLIP_BLOCK - 1 else 3,
          kind=OK if k % CLIP_BLOCK == CLIP_BLOCK - 1 else NOT_ELIGIBLE) for k in range(2 * CLIP_BLOCK + 1)]],
     rows={2: [(0, 4001, L_SIDE, 2, 0, 1, 12, bases(12)[::-1], 24, 24), (0, 4020, R_SIDE, 2, 0, 1, 12, bases(12, 1), 24, 24)]})

N_CASES = len(CASES)
