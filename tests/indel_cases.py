"""Aimed cases for the small-indel candidates (tiddit_amd/tiddit_indels.py, csrc/tdt_indel.hip): records built byte by byte, each case
with the keys, counters and rows it claims, and a second, independent reference: a restatement that unpacks a record with one ``struct``
format, finds the flanked operations with a regular expression over the CIGAR's letters, takes positions from ``itertools.accumulate``,
reads the inserted bases as TEXT (a decode of the whole sequence, then a slice; the packed payload is a base-4 number read from the
reversed text) and counts the sets with ``collections.Counter``.  The definition (``tiddit_indels.events_of_read`` / ``summarise``) walks
operation by operation and shifts nibbles; the two share no code.

A case is a dict: ``reads`` (see :func:`R`), ``cuts`` (where the reads are cut into batches), ``repeat`` (the batches are pushed that many
times), ``capacity`` (of the store at its creation), ``Q`` (the minimum MAPQ of the handle), ``S`` (the minimum supports the finish is
asked for), and its claim, written down from the case's own numbers, never computed by either reference:
  ``keys``  [((K1, K2), how many)]: the keyed events, spelled with :func:`K1`, :func:`DEL`, :func:`INS`, :func:`INSH`, :func:`INSX`;
  ``sn``    {name: n}: EVERY non-zero counter of the push;
  ``rows``  {S: [(K1, K2 with bit 0 clear, SUPPORT, REV)]} in key order — literal in the ``sets`` family; elsewhere None, and
            :func:`expected` counts the claimed keys (a ``Counter`` over the claim, not over any reference's output).
:func:`expected` turns a claim into the sorted key rows, and per S the counter array and the four row columns.

``RS_TILE`` is read from the `#define` lines of csrc/tdt_sort.hip and ``INDEL_TILE`` / ``INDEL_BLOCK`` / ``INDEL_K_TILE`` from those of
csrc/tdt_indel.hip, so the shape cases stay on their edges when a constant is retuned.

``reader_ok``: the case's records can also travel through a BAM file and the device reader.  Malformed records, contig ids outside the
header, reference spans beyond 2^31, records larger than a BGZF block and sequences shorter than their CIGAR cannot, or need not: those
go through ``tdt_indel_push`` only.

Mutants of the restatement (``reference(case, mutant=...)``), each caught inside the family named beside it:
  ``p_after``      P taken after the operation's own advance     -> walk
  ``one_flank``    the flank test on the left side only          -> walk
  ``cap5``         a cap of 5 keyed events                       -> cap
  ``nostrand``     the strand bit left out of the keys           -> sets
  ``nibble_swap``  the two bases of a sequence byte swapped      -> sequence
  ``gt_support``   ``>`` for ``>=`` at the minimum support           -> sets
  ``q_off``        ``mapq > Q`` for ``mapq >= Q``                    -> filters
  ``dup_ok``       0x400 not filtered                            -> filters
"""
import collections
import itertools
import os
import re
import struct

import numpy as np

from tiddit_amd import bamio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(src, name):
    text = open(os.path.join(REPO, "tiddit_amd", "csrc", src)).read()
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+([0-9]+)[ \t]*(?://[^\n]*)?$" % name, text, re.M)
    if not m:
        raise KeyError("cannot parse #define %s" % name)
    return int(m.group(1))


RS_TILE = _define("tdt_sort.hip", "RS_THREADS") * _define("tdt_sort.hip", "RS_ROUNDS")
INDEL_TILE, INDEL_BLOCK, INDEL_K_TILE = (_define("tdt_indel.hip", k) for k in ("INDEL_TILE", "INDEL_BLOCK", "INDEL_K_TILE"))
SN = ("records", "eligible", "malformed", "unanchored", "too_long", "noisy_reads", "reads_with_events", "insertions", "deletions",
      "distinct_events", "reported_events")
SIZE = 11
MUTANTS = {"p_after": "walk", "one_flank": "walk", "cap5": "cap", "nostrand": "sets", "nibble_swap": "sequence", "gt_support": "sets",
           "q_off": "filters", "dup_ok": "filters"}
LENGTHS = (100000, 50000, 1000)
PAD_BYTE = 0x11                              # padding behind a record reads as "AA" bases / as M operations of length 1118481
L_NAME = 9                                   # "r%07d" and its NUL
REV = 0x10
MAXLEN = 2 ** 28 - 1                         # the longest CIGAR operation
BASES = "=ACMGRSVTWYHKDBN"
COLUMNS = ("flag", "tid", "pos", "mapq", "rec_off")


# ------------------------------------------------------------------------------------------- the claim's spelling of a key
def K1(tid, P):
    return tid * 2 ** 32 + P


def DEL(length, rev=0):
    return length * 2 ** 47 + rev


def INS(text, rev=0):
    """an insertion of at most 22 bases, all of A C G T: the bases two bits each, the first one lowest"""
    assert len(text) <= 22 and set(text) <= set("ACGT")
    return 2 ** 63 + len(text) * 2 ** 47 + sum("ACGT".index(c) * 4 ** i for i, c in enumerate(text)) * 2 + rev


def INSH(text, rev=0):
    """any other insertion: FNV-1a over the 4-bit codes, folded to 44 bits"""
    h = 0xcbf29ce484222325
    for c in text:
        h = (h ^ BASES.index(c)) * 0x100000001b3 % 2 ** 64
    return 2 ** 63 + len(text) * 2 ** 47 + 2 ** 45 + ((h ^ (h >> 44)) % 2 ** 44) * 2 + rev


def INSX(length, rev=0):
    """an insertion whose span is not inside the sequence"""
    return 2 ** 63 + length * 2 ** 47 + 2 * 2 ** 45 + rev


def pattern(n, phase=0):
    """the default sequence: ACGT repeated"""
    return ("ACGT" * (n // 4 + 2))[phase:phase + n]


def R(cigar="10M", flag=0, tid=0, pos=100, mapq=60, seq=None, patch=(), pad=0, bs_delta=0):
    """one read.  cigar: string, [(op, len)] or None (no operations); seq: the bases (None: :func:`pattern` over the CIGAR's query length,
    or nothing when that is 100 000 or more); patch: ((byte offset in the record, struct format, value), ...) applied to the encoded
    record; bs_delta: added to block_size; pad: bytes of PAD_BYTE behind the record in the push entry's buffer"""
    cig = [] if cigar is None else bamio.parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    if seq is None:
        qlen = sum(l for op, l in cig if op in (0, 1, 4, 7, 8))
        seq = pattern(qlen) if qlen < 100000 else ""
    return {"cigar": cig, "flag": flag, "tid": tid, "pos": pos, "mapq": mapq, "seq": seq, "patch": tuple(patch), "pad": pad, "bs_delta": bs_delta}


def _record(i, r):
    rec = bytearray(bamio.encode_record("r%07d" % i, r["flag"], r["tid"], r["pos"], r["mapq"], r["cigar"], -1, -1, 0, seq=r["seq"]))
    if r["bs_delta"]:
        struct.pack_into("<I", rec, 0, len(rec) - 4 + r["bs_delta"])
    for off, fmt, val in r["patch"]:
        struct.pack_into(fmt, rec, off, val)
    return bytes(rec)


class Batch:
    """the columns of a run of reads over one raw buffer — what tdt_indel_push and the definition take"""

    def __init__(self, raw, **cols):
        self.raw = raw
        for k in COLUMNS:
            setattr(self, k, cols[k])

    def __len__(self):
        return len(self.tid)

    def cut(self, lo, hi):
        return Batch(self.raw, **{k: getattr(self, k)[lo:hi] for k in COLUMNS})


def build_reads(reads, padding=True, truncate_last=False):
    """-> the reads as one Batch (padding=False: the records back to back, as a BAM file holds them)"""
    parts, offs, o = [], [], 0
    cache = {}
    for i, r in enumerate(reads):
        rec = _record(i, r)
        offs.append(o)
        parts.append(rec)
        o += len(rec)
        if padding and r["pad"]:
            parts.append(cache.setdefault(r["pad"], bytes([PAD_BYTE]) * r["pad"]))
            o += r["pad"]
    col = lambda k, dt: np.array([r[k] for r in reads], dtype=dt)
    b = Batch(np.frombuffer(b"".join(parts), dtype=np.uint8), flag=col("flag", np.uint16), tid=col("tid", np.int32), pos=col("pos", np.int32),
              mapq=col("mapq", np.uint8), rec_off=np.array(offs, dtype=np.uint64))
    if truncate_last:
        b.raw = b.raw[:offs[-1] + 35]
    return b


def build(case, padding=True):
    if ("built", padding) not in case:
        case[("built", padding)] = build_reads(case["reads"], padding, case.get("truncate_last", False))
    return case[("built", padding)]


def batches(case, padding=True):
    """the pushes of the case, in order (``repeat`` times the cut batches)"""
    b = build(case, padding)
    cuts = [0] + list(case["cuts"]) + [len(b)]
    return [b.cut(lo, hi) for lo, hi in zip(cuts, cuts[1:]) if hi > lo] * case["repeat"]


def key_rows(keys):
    """[(K1, K2)] -> the sorted rows, uint64[n][2]"""
    return np.array(sorted(keys), dtype=np.uint64).reshape(-1, 2)


def row_columns(rows):
    """[(K1, K2e, SUPPORT, REV)] -> the four columns as tdt_indel_rows gives them"""
    return (np.array([r[0] for r in rows], dtype=np.uint64), np.array([r[1] for r in rows], dtype=np.uint64),
            np.array([r[2] for r in rows], dtype=np.uint32), np.array([r[3] for r in rows], dtype=np.uint32))


def _sets_of(keys, S, strict=False):
    """every set of a multiset of keys -> (how many sets, the kept rows in key order)"""
    size = collections.Counter((k1, k2 - k2 % 2) for k1, k2 in keys)
    rev = collections.Counter((k1, k2 - k2 % 2) for k1, k2 in keys if k2 % 2)
    return len(size), [(k1, k2, n, rev[(k1, k2)]) for (k1, k2), n in sorted(size.items()) if (n > S if strict else n >= S)]


def counters_of(sn, distinct, reported):
    c = np.zeros(SIZE, dtype=np.uint64)
    for k, v in sn.items():
        assert v > 0, k
        c[SN.index(k)] = v
    c[9], c[10] = distinct, reported
    return c


def expected(case):
    """the claim -> (sorted key rows, {S: (counters, row columns)})"""
    keys = [k for k, n in case["keys"] for _ in range(n)]
    out = {}
    for S in case["S"]:
        distinct, rows = _sets_of(keys, S)
        if case["rows"] is not None:
            assert [tuple(r) for r in case["rows"][S]] == rows, (case["name"], S)           # (the literal rows are the claim; the count agrees)
            rows = [tuple(r) for r in case["rows"][S]]
        out[S] = (counters_of(case["sn"], distinct, len(rows)), row_columns(rows))
    return key_rows(keys), out


def definition(case, numpy_form=False):
    from tiddit_amd import tiddit_indels
    keys, sn = [], {}
    for b in batches(case):
        if numpy_form:
            keys.extend(tiddit_indels.keys_of_batch(b, sn, case["Q"]))
        else:
            tiddit_indels.keys_of_batch_by_read(b, keys, sn, case["Q"])
    out = {}
    for S in case["S"]:
        c, rows = tiddit_indels.summarise(keys, sn, S)
        out[S] = (c, row_columns(rows))
    return key_rows(keys), out


# ------------------------------------------------------------------------------------------- the restatement
_FLANKED = re.compile(r"(?<=[M=X])[ID](?=[M=X])")
_ONE_FLANK = re.compile(r"(?<=[M=X])[ID]")


def reference_batch(b, keys, sn, Q, mutant=None):
    raw = bytes(np.asarray(b.raw, dtype=np.uint8))
    cap = 5 if mutant == "cap5" else 4
    for i in range(len(b)):
        f, tid, pos, mapq, ro = (int(getattr(b, k)[i]) for k in COLUMNS)
        sn["records"] += 1
        dup = f & 0x400 and mutant != "dup_ok"
        if f & 0x4 or f & 0x100 or f & 0x200 or f & 0x800 or dup or tid < 0 or (mapq <= Q if mutant == "q_off" else mapq < Q):
            continue
        sn["eligible"] += 1
        if tid >= 2 ** 24 or pos < 0 or len(raw) - ro < 36:
            sn["malformed"] += 1
            continue
        bs, _, _, l_name, _, _, n_cig, _, l_seq, _, _, _ = struct.unpack_from("<IiiBBHHHiiii", raw, ro)
        if l_seq < 0 or 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs or ro + 4 + bs > len(raw):
            sn["malformed"] += 1
            continue
        words = struct.unpack_from("<%dI" % n_cig, raw, ro + 36 + l_name)
        if any(w % 16 > 8 for w in words):
            sn["malformed"] += 1
            continue
        letters = "".join("MIDNSHP=X"[w % 16] for w in words)
        lens = [w // 16 for w in words]
        # where each operation starts, on the reference and in the read
        r_at = [pos + x for x in [0] + list(itertools.accumulate(l if c in "MDN=X" else 0 for c, l in zip(letters, lens)))]
        q_at = [0] + list(itertools.accumulate(l if c in "MIS=X" else 0 for c, l in zip(letters, lens)))
        if mutant == "p_after":
            r_at = r_at[1:]
        flanked = {m.start() for m in (_ONE_FLANK if mutant == "one_flank" else _FLANKED).finditer(letters)}
        indels = [j for j, c in enumerate(letters) if c in "ID"]
        keyed = [j for j in indels if j in flanked and 0 < lens[j] < 65536]
        if any(not 1 <= r_at[j] < 2 ** 31 for j in keyed):
            sn["malformed"] += 1
            continue
        sn["unanchored"] += sum(1 for j in indels if j not in flanked or lens[j] == 0)
        sn["too_long"] += sum(1 for j in indels if j in flanked and lens[j] >= 65536)
        if len(keyed) > cap:
            sn["noisy_reads"] += 1
            continue
        sn["reads_with_events"] += bool(keyed)
        packed = raw[ro + 36 + l_name + 4 * n_cig:ro + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2]
        if mutant == "nibble_swap":
            text = "".join(BASES[x % 16] + BASES[x // 16] for x in packed)[:l_seq]
        else:
            text = "".join(BASES[x // 16] + BASES[x % 16] for x in packed)[:l_seq]
        rev = 0 if mutant == "nostrand" else (f // 16) % 2
        for j in keyed:
            if letters[j] == "D":
                sn["deletions"] += 1
                keys.append((K1(tid, r_at[j]), DEL(lens[j], rev)))
                continue
            sn["insertions"] += 1
            ins = text[q_at[j]:q_at[j] + lens[j]]
            if q_at[j] + lens[j] > l_seq:
                k2 = INSX(lens[j], rev)
            elif lens[j] <= 22 and set(ins) <= set("ACGT"):
                k2 = 2 ** 63 + lens[j] * 2 ** 47 + int("".join(str("ACGT".index(c)) for c in reversed(ins)), 4) * 2 + rev
            else:
                k2 = INSH(ins, rev)
            keys.append((K1(tid, r_at[j]), k2))


def reference(case, mutant=None, padding=True):
    """-> (sorted key rows, {S: (counters, row columns)}) of the whole case"""
    keys, sn = [], collections.Counter()
    for b in batches(case, padding):
        reference_batch(b, keys, sn, case["Q"], mutant)
    out = {}
    for S in case["S"]:
        distinct, rows = _sets_of(keys, S, strict=mutant == "gt_support")
        out[S] = (counters_of({k: v for k, v in sn.items() if v}, distinct, len(rows)), row_columns(rows))
    return key_rows(keys), out


def same(a, b):
    """two (key rows, {S: (counters, row columns)}) results are equal"""
    if a[0].shape != b[0].shape or not np.array_equal(a[0], b[0]) or set(a[1]) != set(b[1]):
        return False
    return all(np.array_equal(a[1][S][0], b[1][S][0]) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a[1][S][1], b[1][S][1]))
               for S in a[1])


# ------------------------------------------------------------------------------------------- the cases
CASES = []


def case(family, name, reads, keys, sn, cuts=(), repeat=1, capacity=None, reader_ok=True, Q=20, S=(1,), rows=None, **more):
    ins = sum(n for (_, k2), n in keys if k2 >= 2 ** 63)
    assert ins == sn.get("insertions", 0) and sum(n for _, n in keys) - ins == sn.get("deletions", 0), name
    CASES.append(dict(more, family=family, name=family + " " + name, reads=reads, keys=keys, sn=sn, cuts=tuple(cuts), repeat=repeat, capacity=capacity,
                      reader_ok=reader_ok, Q=Q, S=tuple(S), rows=rows, lengths=LENGTHS))


def plain(n, **more):
    """the push counters of n eligible reads"""
    return dict({"records": n, "eligible": n}, **more)


# ---- walk: the operations, the flank test, where P and q are taken
case("walk", "every op code alone", [R("10" + c) for c in "MIDNSHP=X"], [], plain(9, unanchored=2))
# (code c before and behind a 2I and a 2D: keyed between M, = and X only; between I or D all three are unanchored; P = 100 + 3, q = 3)
case("walk", "every op code before and behind an I and a D", [R([(c, 3), (mid, 2), (c, 3)]) for c in range(9) for mid in (1, 2)],
     [((K1(0, 103), INS("TA")), 3), ((K1(0, 103), DEL(2)), 3)], plain(18, unanchored=3 * 4 + 2 * 4, reads_with_events=6, insertions=3, deletions=3))
case("walk", "flanks of mixed match codes, one-sided flanks, ends, I beside D",
     [R("3M2I3="), R("3X2D3M"), R("3=2D3X"), R("3M2I3S"), R("3S2D3M"), R("3M2D3N3M"), R("3M2I3H"), R("3M2D3P3M"), R("3M2I"), R("2D3M"), R("3M2I2D3M")],
     [((K1(0, 103), INS("TA")), 1), ((K1(0, 103), DEL(2)), 2)], plain(11, unanchored=9, reads_with_events=3, insertions=1, deletions=2))
# (a length of 0 is no event; a flank of length 0 is a flank)
case("walk", "operations of length 0", [R("3M0I3M"), R("3M0D3M"), R("0M2D3M"), R("3M2D0M")], [((K1(0, 100), DEL(2)), 1), ((K1(0, 103), DEL(2)), 1)],
     plain(4, unanchored=2, reads_with_events=2, deletions=2))
# (N moves r, S moves q, H and P move neither; 3M1D3M5N3M1I3M: the I at r = 100 + 3 + 1 + 3 + 5 + 3, q = 9, base 9 of ACGTACGTACGTA)
case("walk", "N between events, S in front, H and P change nothing", [R("3M1D3M5N3M1I3M"), R("2H3M1D3M2H"), R("3M2P3M1D3M"), R("4S3M1I3M")],
     [((K1(0, 103), DEL(1)), 2), ((K1(0, 115), INS("C")), 1), ((K1(0, 106), DEL(1)), 1), ((K1(0, 103), INS("T")), 1)],
     plain(4, reads_with_events=4, insertions=2, deletions=3), cuts=(2,))
case("walk", "0 1 2 and 3 operations", [R(None), R("5M"), R("5M2D"), R("5M2D5M")], [((K1(0, 105), DEL(2)), 1)],
     plain(4, unanchored=1, reads_with_events=1, deletions=1))
# (65535 operations: 32767 flanked deletions are a noisy read; 4 of them and 32763 N are not)
case("walk", "65535 operations", [R([(0, 1), (2, 1)] * 32767 + [(0, 1)]), R([(0, 1), (2, 1)] * 4 + [(0, 1), (3, 1)] * 32763 + [(0, 1)])],
     [((K1(0, 101 + 2 * k), DEL(1)), 1) for k in range(4)], plain(2, noisy_reads=1, reads_with_events=1, deletions=4), reader_ok=False)
# ---- cap: INDEL_MAX_PER_READ
_D4 = [(0, 2), (2, 1)] * 4
case("cap", "0 1 4 and 5 keyed events; unanchored and too long ones do not count towards the cap",
     [R("20M"), R("5M1D5M", pos=200), R(_D4 + [(0, 2)], pos=300), R(_D4 + [(0, 2), (2, 1), (0, 2), (1, 1)], pos=400),
      R(_D4 + [(0, 2), (2, 65536), (0, 2), (1, 3)], pos=500)],
     [((K1(0, 205), DEL(1)), 1)] + [((K1(0, p + 2 + 3 * k), DEL(1)), 1) for p in (300, 500) for k in range(4)],
     plain(5, noisy_reads=1, reads_with_events=3, deletions=9, too_long=1, unanchored=2))
case("cap", "noisy reads beside clean ones in one wave", [R("2M1D" * 5 + "2M" if i % 2 else "5M1D5M", pos=1000 + 10 * i) for i in range(64)],
     [((K1(0, 1005 + 10 * i), DEL(1)), 1) for i in range(0, 64, 2)], plain(64, noisy_reads=32, reads_with_events=32, deletions=32))
# ---- sequence: the inserted bases
_G = "GATTACACATTAGGATTACACAT"


def ins_read(text, lead=5, **kw):
    return R("%dM%dI5M" % (lead, len(text)), seq=pattern(lead) + text + "TTTTT", **kw)


case("sequence", "1 21 and 22 bases are packed, 23 are hashed", [ins_read(_G[:n], pos=100 * n) for n in (1, 21, 22, 23)],
     [((K1(0, 100 * n + 5), INS(_G[:n])), 1) for n in (1, 21, 22)] + [((K1(0, 2305), INSH(_G[:23])), 1)], plain(4, reads_with_events=4, insertions=4))
case("sequence", "each base first and last, at even and odd query offsets", [ins_read(b + "G" + b, lead=lead) for b in "ACGT" for lead in (4, 5)],
     [((K1(0, 100 + lead), INS(b + "G" + b)), 1) for b in "ACGT" for lead in (4, 5)], plain(8, reads_with_events=8, insertions=8))
case("sequence", "an N or = base is hashed", [ins_read("ANA"), ins_read("A=A"), ins_read("N"), ins_read("ACA")],
     [((K1(0, 105), INSH("ANA")), 1), ((K1(0, 105), INSH("A=A")), 1), ((K1(0, 105), INSH("N")), 1), ((K1(0, 105), INS("ACA")), 1)],
     plain(4, reads_with_events=4, insertions=4))
case("sequence", "insertions that differ in one base are distinct", [ins_read("ACGTA"), ins_read("ACGTC"), ins_read("ACGTA"), ins_read(_G), ins_read(_G[:22] + "A"),
                                                                     ins_read(_G)],
     [((K1(0, 105), INS("ACGTA")), 2), ((K1(0, 105), INS("ACGTC")), 1), ((K1(0, 105), INSH(_G)), 2), ((K1(0, 105), INSH(_G[:22] + "A")), 1)],
     plain(6, reads_with_events=6, insertions=6), S=(1, 2))
_LONG = pattern(65535, 1)
case("sequence", "65535 bases are hashed, 65536 are too long", [ins_read(_LONG), R("5M65536I5M", seq=""), R("5M65535D5M"), R("5M65536D5M")],
     [((K1(0, 105), INSH(_LONG)), 1), ((K1(0, 105), DEL(65535)), 1)], plain(4, too_long=2, reads_with_events=2, insertions=1, deletions=1), reader_ok=False)
case("sequence", "no sequence: SEQ *", [R("5M3I5M", seq=""), R("5M3I5M", seq="", flag=REV)], [((K1(0, 105), INSX(3)), 1), ((K1(0, 105), INSX(3, 1)), 1)],
     plain(2, reads_with_events=2, insertions=2))
case("sequence", "a span that ends one base behind the sequence, and one that ends on it", [R("5M3I5M", seq="ACGTACG"), R("5M3I5M", seq="ACGTACGT")],
     [((K1(0, 105), INSX(3)), 1), ((K1(0, 105), INS("CGT")), 1)], plain(2, reads_with_events=2, insertions=2), reader_ok=False)
case("sequence", "the query offset behind a soft clip", [R("3S5M2I5M"), R("3S2H5M2I5M"), R("5M2I5M")],
     [((K1(0, 105), INS("AC")), 2), ((K1(0, 105), INS("CG")), 1)], plain(3, reads_with_events=3, insertions=3))
# ---- filters
_F = "5M1D5M"
case("filters", "each bit of 0xF04 alone, the other bits, tid -1",
     [R(_F, flag=f) for f in (0x4, 0x100, 0x200, 0x400, 0x800, 0x1, 0x2, 0x8, 0x10, 0x20, 0x40, 0x80)] + [R(_F, tid=-1)],
     [((K1(0, 105), DEL(1)), 6), ((K1(0, 105), DEL(1, 1)), 1)], {"records": 13, "eligible": 7, "reads_with_events": 7, "deletions": 7}, cuts=(5,))
case("filters", "mapq round a minimum of 0", [R(_F, mapq=0), R(_F, mapq=1)], [((K1(0, 105), DEL(1)), 2)], plain(2, reads_with_events=2, deletions=2), Q=0)
case("filters", "mapq round a minimum of 20", [R(_F, mapq=19), R(_F, mapq=20), R(_F, mapq=21)], [((K1(0, 105), DEL(1)), 2)],
     {"records": 3, "eligible": 2, "reads_with_events": 2, "deletions": 2}, Q=20)
case("filters", "mapq round a minimum of 255", [R(_F, mapq=254), R(_F, mapq=255)], [((K1(0, 105), DEL(1)), 1)],
     {"records": 2, "eligible": 1, "reads_with_events": 1, "deletions": 1}, Q=255)
# ---- malformed: each bound, op codes, tid, pos, P.  The padding behind a record reads as bases and operations: a missing bound finds them.
_GOOD = [R(_F, pos=50), R(_F, pos=60)]
_BAD_SN = plain(3, malformed=1, reads_with_events=2, deletions=2)
_BAD_KEYS = [((K1(0, 55), DEL(1)), 1), ((K1(0, 65), DEL(1)), 1)]
case("malformed", "the fixed fields end behind the buffer", _GOOD + [R(_F)], _BAD_KEYS, _BAD_SN, reader_ok=False, truncate_last=True)
case("malformed", "the fields are longer than block_size", [_GOOD[0], R(_F, bs_delta=-1, pad=64), _GOOD[1]], _BAD_KEYS, _BAD_SN, reader_ok=False)
case("malformed", "block_size ends behind the buffer (the last record)", _GOOD + [R(_F, bs_delta=1)], _BAD_KEYS, _BAD_SN, reader_ok=False)
case("malformed", "a negative l_seq", [_GOOD[0], R(_F, patch=((4 + 16, "<i", -1),), pad=64), _GOOD[1]], _BAD_KEYS, _BAD_SN, reader_ok=False)
case("malformed", "op codes 9 and 15", [_GOOD[0], R(_F, patch=((4 + 32 + L_NAME + 8, "<I", 5 << 4 | 9),), pad=64),
                                        R(_F, patch=((4 + 32 + L_NAME, "<I", 5 << 4 | 15),), pad=64), _GOOD[1]], _BAD_KEYS,
     plain(4, malformed=2, reads_with_events=2, deletions=2), reader_ok=False)
case("malformed", "tid 2^24 - 1 and 2^24, pos -1", [R(_F, tid=2 ** 24 - 1), R(_F, tid=2 ** 24), R(_F, pos=-1)], [((K1(2 ** 24 - 1, 105), DEL(1)), 1)],
     plain(3, malformed=2, reads_with_events=1, deletions=1), reader_ok=False)
# (a deletion at r = 100 + 5 + the N operations + 1: P = 2^31 - 1 is an event, 2^31 makes the record malformed, also as a sixth keyed event)
_NS = [(3, MAXLEN)] * 7
_LAST = 2 ** 31 - 1 - 106 - 7 * MAXLEN
assert 0 < _LAST < MAXLEN
case("malformed", "P 0 and 1, 2^31 - 1 and 2^31 through long N operations",
     [R("0M1D5M", pos=0), R("1M1D5M", pos=0), R([(0, 5)] + _NS + [(3, _LAST), (0, 1), (2, 1), (0, 5)]), R([(0, 5)] + _NS + [(3, _LAST + 1), (0, 1), (2, 1), (0, 5)]),
      R([(0, 1), (2, 1)] * 5 + [(0, 1)] + _NS + [(3, MAXLEN), (0, 1), (2, 1), (0, 5)])],
     [((K1(0, 1), DEL(1)), 1), ((K1(0, 2 ** 31 - 1), DEL(1)), 1)], plain(5, malformed=3, reads_with_events=2, deletions=2), reader_ok=False)
# ---- sets
_E = lambda p, n_f, n_r: [R(_F, pos=p)] * n_f + [R(_F, pos=p, flag=REV)] * n_r
_ROWS = [(K1(0, 105), DEL(1), 1, 0), (K1(0, 205), DEL(1), 2, 0), (K1(0, 305), DEL(1), 2, 2), (K1(0, 405), DEL(1), 3, 2), (K1(0, 505), DEL(1), 4, 1)]
case("sets", "forward only, reverse only and mixed; supports round 1 2 and 3", _E(100, 1, 0) + _E(200, 2, 0) + _E(300, 0, 2) + _E(400, 1, 2) + _E(500, 3, 1),
     [((K1(0, 105), DEL(1)), 1), ((K1(0, 205), DEL(1)), 2), ((K1(0, 305), DEL(1, 1)), 2), ((K1(0, 405), DEL(1)), 1), ((K1(0, 405), DEL(1, 1)), 2),
      ((K1(0, 505), DEL(1)), 3), ((K1(0, 505), DEL(1, 1)), 1)], plain(12, reads_with_events=12, deletions=12), S=(1, 2, 3), cuts=(4, 9),
     rows={1: _ROWS, 2: _ROWS[1:], 3: _ROWS[3:]})
_ROWS2 = [(K1(0, 105), DEL(1), 2, 1), (K1(0, 105), DEL(2), 1, 0), (K1(0, 105), INS("A"), 1, 1), (K1(1, 105), DEL(1), 1, 0)]
case("sets", "an INS and a DEL at one P, two lengths at one P, two contigs",
     [R("5M1I5M", seq="ACGTAACGTA", flag=REV), R(_F, tid=1), R("5M2D5M"), R(_F), R(_F, flag=REV)],
     [((K1(0, 105), INS("A", 1)), 1), ((K1(1, 105), DEL(1)), 1), ((K1(0, 105), DEL(2)), 1), ((K1(0, 105), DEL(1)), 1), ((K1(0, 105), DEL(1, 1)), 1)],
     plain(5, reads_with_events=5, insertions=1, deletions=4), S=(1, 2), rows={1: _ROWS2, 2: _ROWS2[:1]})
assert (2 * INDEL_TILE + 1) % 3 == 0
_THIRD = (2 * INDEL_TILE + 1) // 3
case("sets", "one event over more keys than two tiles hold, through repeated pushes", [R(_F, flag=REV)] * 1000 + [R(_F)] * (_THIRD - 1000),
     [((K1(0, 105), DEL(1)), 3 * (_THIRD - 1000)), ((K1(0, 105), DEL(1, 1)), 3000)], plain(3 * _THIRD, reads_with_events=3 * _THIRD, deletions=3 * _THIRD),
     repeat=3, reader_ok=False, S=(2, 3 * _THIRD, 3 * _THIRD + 1),
     rows={2: [(K1(0, 105), DEL(1), 3 * _THIRD, 3000)], 3 * _THIRD: [(K1(0, 105), DEL(1), 3 * _THIRD, 3000)], 3 * _THIRD + 1: []})
case("sets", "an empty store", [R("10M"), R("10M", flag=REV)], [], plain(2), S=(1, 2), rows={1: [], 2: []})
case("sets", "a single key", [R("10M"), R(_F, flag=REV)], [((K1(0, 105), DEL(1, 1)), 1)], plain(2, reads_with_events=1, deletions=1), S=(1, 2),
     rows={1: [(K1(0, 105), DEL(1), 1, 1)], 2: []})


def _runs(sizes, seed):
    """reads whose sorted store holds runs of these sizes in this order (run r at P = 15 + r; its members forward and reverse in turn, a
    single one by r's parity), pushed shuffled"""
    reads, keys = [], []
    for r, s in enumerate(sizes):
        n_rev = s // 2 if s > 1 else r % 2
        reads += [R(_F, pos=10 + r)] * (s - n_rev) + [R(_F, pos=10 + r, flag=REV)] * n_rev
        keys += [((K1(0, 15 + r), DEL(1, v)), n) for v, n in ((0, s - n_rev), (1, n_rev)) if n]
    order = np.random.default_rng(seed).permutation(len(reads))
    return [reads[k] for k in order], keys, plain(len(reads), reads_with_events=len(reads), deletions=len(reads))


for _t in sorted({RS_TILE, INDEL_TILE}):
    case("sets", "a store of %d - 1 keys, a run that ends the store" % _t, *_runs([1] * (_t - 3) + [2], 1), cuts=(1000,), reader_ok=False, S=(1, 2))
    case("sets", "a store of %d keys, a run that ends on the tile boundary" % _t, *_runs([1] * (_t - 2) + [2], 2), reader_ok=False, S=(1, 2))
    case("sets", "a store of %d + 1 keys, a run that crosses the boundary" % _t, *_runs([1] * (_t - 1) + [2], 3), reader_ok=False, S=(1, 2))
    case("sets", "a store of %d + 1 keys, a run that starts on the boundary" % _t, *_runs([2] + [1] * (_t - 2) + [1], 4), reader_ok=False, S=(1, 2))
    case("sets", "a store of %d + 2 keys, a run of three round the boundary" % _t, *_runs([1] * (_t - 2) + [3] + [1], 6), reader_ok=False, S=(1, 2, 3))
    # (the second tile holds no run head at all: the carry of the first one reaches the third)
    case("sets", "a store of 2 x %d + 1 keys, a run over a whole tile" % _t, *_runs([1] * (_t - 2) + [_t + 2] + [1], 5), cuts=(_t, _t + 7), reader_ok=False,
         S=(1, 2, _t + 2, _t + 3))
    case("sets", "a store of exactly %d keys" % _t, *_runs([1] * _t, 7), reader_ok=False, S=(1, 2))
    case("sets", "a store of %d + 1 keys" % _t, *_runs([1] * (_t + 1), 8), reader_ok=False, S=(1, 2))


# ---- shape: batches round the wave, the round and the tile of the push kernel; the LDS staging at its bound; a store that grows
def _mix(n):
    """read i by i % 4: a deletion at 10 i + 5; no event; an unmapped read; an insertion of the base C or G at 10 i + 5 (reverse)"""
    reads = [(R(_F, pos=10 * i), R("10M", pos=10 * i), R(_F, flag=0x4, pos=10 * i), ins_read("CG"[i // 4 % 2], pos=10 * i, flag=REV))[i % 4] for i in range(n)]
    keys = [((K1(0, 10 * i + 5), DEL(1)), 1) for i in range(0, n, 4)] + [((K1(0, 10 * i + 5), INS("CG"[i // 4 % 2], 1)), 1) for i in range(3, n, 4)]
    nd, nn, nu, ni = (len(range(k, n, 4)) for k in range(4))
    sn = {k: v for k, v in (("records", n), ("eligible", n - nu), ("reads_with_events", nd + ni), ("insertions", ni), ("deletions", nd)) if v}
    return reads, keys, sn


for _n in (1, 63, 64, 65, INDEL_BLOCK + 1, INDEL_K_TILE - 1, INDEL_K_TILE, INDEL_K_TILE + 1):
    case("shape", "a batch of %d reads" % _n, *_mix(_n))
_N4 = INDEL_K_TILE + 1
case("shape", "every read of a workgroup gives 4 events", [R(_D4 + [(0, 2)], pos=20 * i) for i in range(_N4)],
     [((K1(0, 20 * i + 2 + 3 * k), DEL(1)), 1) for i in range(_N4) for k in range(4)], plain(_N4, reads_with_events=_N4, deletions=4 * _N4))
# (room for 4 keys per read is reserved: 10 reads fit a store of 64; 20 more do not, and the 10 keys there are leave no room either: it
#  grows to 96; 30 more need 30 + 120: it grows again)
_ONE = lambda n: ([R(_F, pos=10 * i) for i in range(n)], [((K1(0, 10 * i + 5), DEL(1)), 1) for i in range(n)], plain(n, reads_with_events=n, deletions=n))
case("shape", "a store that grows once from a capacity of 64", *_ONE(30), cuts=(10,), capacity=64, grows=1, asks=1)
case("shape", "a store that grows twice from a capacity of 64", *_ONE(60), cuts=(10, 30), capacity=64, grows=2, asks=2)
# (the push kernel's compaction and emit with nothing to do in most of a workgroup: the eligible read goes to lane 0, three waves of every
#  round emit nothing, and the third workgroup holds one read below the MAPQ cut and emits no key)
_NL = 2 * INDEL_K_TILE + 1
_LAST = [i for i in range(_NL) if i % INDEL_BLOCK == INDEL_BLOCK - 1]
case("shape", "only the last lane of every round holds an eligible read", [R(_F, pos=10 * i, mapq=60 if i in _LAST else 3) for i in range(_NL)],
     [((K1(0, 10 * i + 5), DEL(1)), 1) for i in _LAST], {"records": _NL, "eligible": len(_LAST), "reads_with_events": len(_LAST), "deletions": len(_LAST)})

N_CASES = 53
FAMILIES = sorted({c["family"] for c in CASES})
