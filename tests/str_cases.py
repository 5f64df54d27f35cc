"""Aimed cases for the tandem-repeat genotypes (tiddit_amd/tiddit_str.py, csrc/tdt_str.hip): records built byte by byte, each case a
handful of reads against a small loci table, with the keys and counters it claims, and a second, independent reference: a restatement
that unpacks a record with one ``struct`` format, expands the CIGAR into a reference-to-query MAP (a dict with an entry per aligned
base), decodes the whole sequence to TEXT and finds the runs by string matching (``os.path.commonprefix`` against the motif written out
as text, the leftward run on the reversed texts).  The definition (``tiddit_str.keys_of_read``) walks operation by operation and compares
nibbles one at a time; the two share no code.

A case is a dict: ``loci`` (the rows of the table: (chrom, start, end, motif), all acceptable, in table order — a key's ``K1`` is an index
into them), ``reads`` (see :func:`R`), ``F`` / ``Q`` (the handle's flank and minimum MAPQ), ``cuts`` (where the reads are cut into batches),
``repeat``, ``capacity`` (of the store at its creation) and its claim, written down from the case's own numbers, never computed by
either reference:
  ``keys``  [((K1, K2), how many)]: spelled with :func:`SPAN`, :func:`LEFT`, :func:`RIGHT`;
  ``sn``    {name: n}: EVERY non-zero counter of the push.
:func:`expected` turns a claim into the sorted key rows, the counter array and the four row columns of the finish (a ``Counter`` over
the claim, not over any reference's output).

``GENOTYPES`` are the cases of the genotype rule: the sets of ONE locus of 12 reference bases as {L: n} SPAN rows and (kind, L, n) flank
rows, the cut ``S``, and the literal line :func:`tiddit_str.summarise` must give.

``STR_BLOCK`` is read from the `#define` line of csrc/tdt_str.hip, so the shape cases stay on their edges when it is retuned; 64 is
the wave.

``reader_ok``: the case's records can also travel through a BAM file and the device reader.  Malformed records, contig ids outside the
header, columns that contradict the record and sequences shorter than their CIGAR cannot, or need not: those go through ``tdt_str_push``
only.

Mutants of the restatement (``reference(case, mutant=...)``), each caught inside the family named beside it:
  ``span_plus``    L = qb - qa for a SPAN                                   -> cigar
  ``ins_lost``     an insertion directly behind ``a`` is not counted          -> cigar
  ``no_clip``      a run stops at the end of the aligned bases              -> run
  ``phase0``       the leftward run starts at the motif's last letter       -> run
  ``open_early``   open one base before the read's end                      -> run
  ``flank_lt``     ``pos < s - F`` and ``end > e + F``                          -> flank
  ``reach_lt``     in reach when ``s < end`` and ``e > pos``                    -> flank
  ``cap5``         five loci handled                                        -> table
  ``nostrand``     the strand bit left out of the keys                      -> merge
  ``q_off``        ``mapq > Q`` for ``mapq >= Q``                               -> gate
  ``dup_ok``       0x400 not filtered                                       -> gate
"""
import collections
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


STR_BLOCK = _define("tdt_str.hip", "STR_BLOCK")
WAVE = 64
SN = ("records", "eligible", "in_reach", "malformed", "no_alignment", "no_sequence", "span_keys", "left_keys", "right_keys", "unanchored",
      "over_cap")
SIZE = 11
MUTANTS = {"span_plus": "cigar", "ins_lost": "cigar", "no_clip": "run", "phase0": "run", "open_early": "run", "flank_lt": "flank",
           "reach_lt": "flank", "cap5": "table", "nostrand": "merge", "q_off": "gate", "dup_ok": "gate"}
NAMES = ("c0", "c1", "c2")
LENGTHS = (100000, 50000, 1000)
L_NAME = 9                                   # "r%07d" and its NUL
REV = 0x10
BASES = "=ACMGRSVTWYHKDBN"
COLUMNS = ("flag", "tid", "pos", "end", "mapq", "rec_off")
STD = ("c0", 1000, 1012, "CAG")              # the locus most cases use: a = 999, b = 1012, REF_LEN 12


# ------------------------------------------------------------------------------------------- the claim's spelling of a key
def SPAN(L, rev=0):
    return L * 2 + rev


def LEFT(L, open=False, rev=0):
    return (2 if open else 1) * 2 ** 33 + L * 2 + rev


def RIGHT(L, open=False, rev=0):
    return (4 if open else 3) * 2 ** 33 + L * 2 + rev


def R(cigar="40M", pos=990, seq=None, flag=0, tid=0, mapq=60, end=None, patch=(), bs_delta=0):
    """one read.  cigar: string, [(op, len)] or None (no operations); seq: the bases (None: ``T`` over the CIGAR's query length); end: the
    batch's ``end`` column (None: what the readers give, pos + the CIGAR's reference length, 1 when that is 0); patch: ((byte offset in
    the record, struct format, value), ...) applied to the encoded record; bs_delta: added to block_size"""
    cig = [] if cigar is None else bamio.parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    if seq is None:
        seq = "T" * sum(l for op, l in cig if op in (0, 1, 4, 7, 8))
    if end is None:
        end = pos + (sum(l for op, l in cig if op in (0, 2, 3, 7, 8)) or 1)
    return {"cigar": cig, "flag": flag, "tid": tid, "pos": pos, "end": end, "mapq": mapq, "seq": seq, "patch": tuple(patch), "bs_delta": bs_delta}


def T(n):
    return "T" * n


def _record(i, r):
    rec = bytearray(bamio.encode_record("r%07d" % i, r["flag"], r["tid"], r["pos"], r["mapq"], r["cigar"], -1, -1, 0, seq=r["seq"]))
    if r["bs_delta"]:
        struct.pack_into("<I", rec, 0, len(rec) - 4 + r["bs_delta"])
    for off, fmt, val in r["patch"]:
        struct.pack_into(fmt, rec, off, val)
    return bytes(rec)


class Batch:
    """the columns of a run of reads over one raw buffer — what tdt_str_push and the definition take"""

    def __init__(self, raw, **cols):
        self.raw = raw
        for k in COLUMNS:
            setattr(self, k, cols[k])

    def __len__(self):
        return len(self.tid)

    def cut(self, lo, hi):
        return Batch(self.raw, **{k: getattr(self, k)[lo:hi] for k in COLUMNS})


def build_reads(reads, truncate_last=False):
    """-> the reads as one Batch, the records back to back, as a BAM file holds them"""
    parts, offs, o = [], [], 0
    for i, r in enumerate(reads):
        rec = _record(i, r)
        offs.append(o)
        parts.append(rec)
        o += len(rec)
    col = lambda k, dt: np.array([r[k] for r in reads], dtype=dt)
    b = Batch(np.frombuffer(b"".join(parts), dtype=np.uint8), flag=col("flag", np.uint16), tid=col("tid", np.int32), pos=col("pos", np.int32),
              end=col("end", np.int32), mapq=col("mapq", np.uint8), rec_off=np.array(offs, dtype=np.uint64))
    if truncate_last:
        b.raw = b.raw[:offs[-1] + 35]
    return b


def build(case):
    if "built" not in case:
        case["built"] = build_reads(case["reads"], case.get("truncate_last", False))
    return case["built"]


def batches(case):
    """the pushes of the case, in order (``repeat`` times the cut batches)"""
    b = build(case)
    cuts = [0] + list(case["cuts"]) + [len(b)]
    return [b.cut(lo, hi) for lo, hi in zip(cuts, cuts[1:]) if hi > lo] * case["repeat"]


def loci_of(case):
    """the case's table as the handle and the definition take it (every row of a case is acceptable: nothing is skipped)"""
    from tiddit_amd import tiddit_str
    if "table" not in case:
        case["table"] = tiddit_str.loci_of_rows([list(map(str, r)) for r in case["loci"]], NAMES, LENGTHS)
        assert [r[:4] for r in case["table"].rows] == [(c, s, e, m.upper()) for c, s, e, m in case["loci"]], case["name"]
    return case["table"]


def key_rows(keys):
    """[(K1, K2)] -> the sorted rows, uint64[n][2]"""
    return np.array(sorted(keys), dtype=np.uint64).reshape(-1, 2)


def row_columns(rows):
    """[(K1, K2e, SUPPORT, REV)] -> the four columns as tdt_str_rows gives them"""
    return (np.array([r[0] for r in rows], dtype=np.uint64), np.array([r[1] for r in rows], dtype=np.uint64),
            np.array([r[2] for r in rows], dtype=np.uint32), np.array([r[3] for r in rows], dtype=np.uint32))


def _sets_of(keys):
    size = collections.Counter((k1, k2 - k2 % 2) for k1, k2 in keys)
    rev = collections.Counter((k1, k2 - k2 % 2) for k1, k2 in keys if k2 % 2)
    return [(k1, k2, n, rev[(k1, k2)]) for (k1, k2), n in sorted(size.items())]


def counters_of(sn):
    c = np.zeros(SIZE, dtype=np.uint64)
    for k, v in sn.items():
        assert v > 0, k
        c[SN.index(k)] = v
    return c


def expected(case):
    """the claim -> (sorted key rows, counters, row columns)"""
    keys = [k for k, n in case["keys"] for _ in range(n)] * case["repeat"]
    sn = {k: v * case["repeat"] for k, v in case["sn"].items()}
    rows = _sets_of(keys)
    if case.get("rows") is not None:
        assert [tuple(r) for r in case["rows"]] == rows, case["name"]                  # (the literal rows are the claim; the count agrees)
    return key_rows(keys), counters_of(sn), row_columns(rows)


def definition(case, cuts=None):
    from tiddit_amd import tiddit_str
    keys, sn = [], {}
    bs = batches(case) if cuts is None else [build(case).cut(lo, hi) for lo, hi in zip([0] + list(cuts), list(cuts) + [len(build(case))])] * case["repeat"]
    for b in bs:
        tiddit_str.keys_of_batch(b, loci_of(case), keys, sn, case["F"], case["Q"])
    return key_rows(keys), tiddit_str.counts_of(sn), row_columns(tiddit_str.rows_of_keys(keys))


# ------------------------------------------------------------------------------------------- the restatement
def reference_batch(b, loci, keys, sn, F, Q, mutant=None):
    raw = bytes(np.asarray(b.raw, dtype=np.uint8))
    by_contig = collections.defaultdict(list)
    for k, (chrom, s, e, motif) in enumerate(loci):
        by_contig[NAMES.index(chrom)].append((k, s, e, motif.upper()))
    cap = 5 if mutant == "cap5" else 4
    for i in range(len(b)):
        f, tid, pos, end, mapq, ro = (int(getattr(b, k)[i]) for k in COLUMNS)
        sn["records"] += 1
        dup = f & 0x400 and mutant != "dup_ok"
        if f & 0x4 or f & 0x100 or f & 0x200 or f & 0x800 or dup or tid < 0 or (mapq <= Q if mutant == "q_off" else mapq < Q):
            continue
        sn["eligible"] += 1
        if mutant == "reach_lt":
            near = [l for l in by_contig.get(tid, []) if l[1] < end and l[2] > pos]
        else:
            near = [l for l in by_contig.get(tid, []) if l[1] <= end and l[2] >= pos]
        if not near:
            continue
        sn["in_reach"] += 1
        if pos < 0 or len(raw) - ro < 36:
            sn["malformed"] += 1
            continue
        bs, _, _, l_name, _, _, n_cig, _, l_seq, _, _, _ = struct.unpack_from("<IiiBBHHHiiii", raw, ro)
        if l_seq < 0 or 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs or ro + 4 + bs > len(raw):
            sn["malformed"] += 1
            continue
        if n_cig == 0:
            sn["no_alignment"] += 1
            continue
        if l_seq == 0:
            sn["no_sequence"] += 1
            continue
        words = struct.unpack_from("<%dI" % n_cig, raw, ro + 36 + l_name)
        if any(w % 16 > 8 for w in words):
            sn["malformed"] += 1
            continue
        # the map: reference base -> query index, an entry per aligned base near a locus of the read
        want = {x for _, s, e, _ in near[:cap] for x in (s - 1, e)}
        at, r, q, aligned_end = {}, pos, 0, 0
        for w in words:
            c, n = "MIDNSHP=X"[w % 16], w // 16
            if c in "M=X":
                at.update({x: q + x - r for x in want if r <= x < r + n})
                aligned_end = q + n
            if c == "I" and mutant == "ins_lost" and r - 1 in want and r - 1 in at:
                q -= n                                                     # (the mutant forgets an insertion directly behind an anchor)
            r += n if c in "MDN=X" else 0
            q += n if c in "MIS=X" else 0
        handled = near[:cap]
        if any(v >= l_seq for v in at.values()):
            sn["malformed"] += 1
            continue
        packed = raw[ro + 36 + l_name + 4 * n_cig:ro + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2]
        text = "".join(BASES[x // 16] + BASES[x % 16] for x in packed)[:l_seq]
        rev = 0 if mutant == "nostrand" else (f // 16) % 2
        sn["over_cap"] += len(near) - len(handled)
        for k, s, e, motif in handled:
            m = len(motif)
            if mutant == "flank_lt":
                left, right = pos < s - F and s - 1 in at, end > e + F and e in at
            else:
                left, right = pos <= s - F and s - 1 in at, end >= e + F and e in at
            if left and right:
                sn["span_keys"] += 1
                keys.append((k, SPAN(at[e] - at[s - 1] - (0 if mutant == "span_plus" else 1), rev)))
            elif left:
                tail = text[at[s - 1] + 1:aligned_end] if mutant == "no_clip" else text[at[s - 1] + 1:]
                n = len(os.path.commonprefix([tail, motif * (len(tail) // m + 1)]))
                is_open = n >= len(tail) - (1 if mutant == "open_early" else 0)
                sn["left_keys"] += 1
                keys.append((k, LEFT(n, is_open, rev)))
            elif right:
                head = text[:at[e]][::-1]
                phase = 0 if mutant == "phase0" else (e - s) % m          # the letters of the locus, written out, end here
                written = (motif * ((e - s) // m + len(head) // m + 3))[:(len(head) // m + 2) * m + phase][::-1]
                n = len(os.path.commonprefix([head, written]))
                sn["right_keys"] += 1
                keys.append((k, RIGHT(n, n == len(head), rev)))
            else:
                sn["unanchored"] += 1


def reference(case, mutant=None):
    """-> (sorted key rows, counters, row columns) of the whole case"""
    keys, sn = [], collections.Counter()
    for b in batches(case):
        reference_batch(b, case["loci"], keys, sn, case["F"], case["Q"], mutant)
    return key_rows(keys), counters_of({k: v for k, v in sn.items() if v}), row_columns(_sets_of(keys))


def same(a, b):
    """two (key rows, counters, row columns) results are equal"""
    return (a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a[2], b[2])))


# ------------------------------------------------------------------------------------------- the cases
CASES = []


def case(family, name, loci, reads, keys, sn, F=5, Q=20, cuts=(), repeat=1, capacity=None, reader_ok=True, **more):
    kinds = collections.Counter(("span_keys", "left_keys", "left_keys", "right_keys", "right_keys")[k2 >> 33] for (_, k2), n in keys for _ in range(n))
    assert all(kinds.get(k, 0) == sn.get(k, 0) for k in ("span_keys", "left_keys", "right_keys")), name
    CASES.append(dict(more, family=family, name=family + " " + name, loci=loci, reads=reads, keys=keys, sn=sn, F=F, Q=Q, cuts=tuple(cuts), repeat=repeat,
                      capacity=capacity, reader_ok=reader_ok))


def plain(n, **more):
    """the push counters of n eligible reads that all have a locus in reach"""
    return dict({"records": n, "eligible": n, "in_reach": n}, **more)


CAG = "CAG" * 30

# ---- motif: every motif length, and a lower-case one; per locus a spanning read, a read that ends one base before the repeat does
# (LEFT, open) and a read that starts 2 bases in front of it (no left flank of 5: RIGHT, closed by the T in front of the repeat)
_M = [("c0", 1000, 1003, "A"), ("c0", 2000, 2004, "ac"), ("c0", 3000, 3012, "CAG"), ("c0", 4000, 4008, "AACG"), ("c0", 5000, 5010, "AAACG"),
      ("c0", 6000, 6012, "AACAGC")]
_reads, _keys = [], []
for _k, (_c, _s, _e, _m) in enumerate(_M):
    _rep = (_m.upper() * 12)[:_e - _s]
    _reads += [R("%dM" % (20 + _e - _s), _s - 10, T(10) + _rep + T(10)), R("%dM" % (10 + _e - _s - 1), _s - 10, T(10) + _rep[:-1]),
               R("%dM" % (12 + _e - _s), _s - 2, T(2) + _rep + T(10))]
    _keys += [((_k, SPAN(_e - _s)), 1), ((_k, LEFT(_e - _s - 1, True)), 1), ((_k, RIGHT(_e - _s)), 1)]
case("motif", "lengths 1 to 6 and a lower-case one: SPAN, LEFT open, RIGHT closed", _M, _reads, _keys, plain(18, span_keys=6, left_keys=6, right_keys=6))

# ---- run: the two run counts.  LEFT reads: pre T, then n bases of the repeat, a T, and T to the end: 12 aligned bases of the locus and a
# trailing soft clip of 30; pre = 10 puts qa + 1 on an even query index, pre = 11 on an odd one
_RUNS = (0, 1, 15, 16, 17, 31, 32, 33)
case("run", "LEFT runs of 0 1 15 16 17 31 32 33 from an even and an odd query index, through a trailing soft clip", [STD],
     [R("%dM30S" % (pre + 12), 1000 - pre, T(pre) + CAG[:n] + T(42 - n)) for pre in (10, 11) for n in _RUNS],
     [((0, LEFT(n)), 2) for n in _RUNS], plain(16, left_keys=16))
case("run", "LEFT runs broken at every nibble of the first two 16-base steps", [STD],
     [R("22M30S", 990, T(10) + CAG[:n] + T(42 - n)) for n in range(34)], [((0, LEFT(n)), 1) for n in range(34)], plain(34, left_keys=34))
# RIGHT reads: a leading soft clip of x, 12 aligned bases of the locus and 10 behind it; the last n bases in front of b repeat the motif
case("run", "RIGHT runs of 0 1 15 16 17 31 32 33 down from an odd and an even query index, through a leading soft clip", [STD],
     [R("%dS22M" % x, 1000, T(x + 12 - n) + CAG[90 - n:] + T(10)) for x in (30, 31) for n in _RUNS],
     [((0, RIGHT(n)), 2) for n in _RUNS], plain(16, right_keys=16))
case("run", "RIGHT runs broken at every nibble of the first two 16-base steps", [STD],
     [R("30S22M", 1000, T(42 - n) + CAG[90 - n:] + T(10)) for n in range(34)], [((0, RIGHT(n)), 1) for n in range(34)], plain(34, right_keys=34))
# (a locus of 10 bases: its last letter is C, so the leftward run reads C G A C G A ...)
case("run", "RIGHT where the locus ends inside a unit: the phase of the last base", [("c0", 2000, 2010, "CAG")],
     [R("30S20M", 2000, T(40 - n) + (CAG + "C")[91 - n:] + T(10)) for n in (1, 2, 3, 10, 16, 17, 33)],
     [((0, RIGHT(n)), 1) for n in (1, 2, 3, 10, 16, 17, 33)], plain(7, right_keys=7))
# (motifs of 5 and 6: 16 mod m is not 0, the motif word changes from step to step; 47 48 49 bases are three steps)
case("run", "runs of three steps with motifs of 5 and 6 letters, both directions",
     [("c0", 3000, 3010, "AAACG"), ("c0", 4000, 4012, "AACAGC")],
     [R("20M60S", 2990, T(10) + ("AAACG" * 20)[:n] + T(70 - n)) for n in (47, 48, 49)]
     + [R("22M60S", 3990, T(10) + ("AACAGC" * 20)[:n] + T(72 - n)) for n in (47, 48, 49)]
     + [R("60S20M", 3000, T(70 - n) + ("AAACG" * 20)[100 - n:] + T(10)) for n in (47, 48, 49)]
     + [R("60S22M", 4000, T(72 - n) + ("AACAGC" * 20)[120 - n:] + T(10)) for n in (47, 48, 49)],
     [((k, key(n)), 1) for k, key in ((0, LEFT), (1, LEFT), (0, RIGHT), (1, RIGHT)) for n in (47, 48, 49)], plain(12, left_keys=6, right_keys=6))
case("run", "a run that ends exactly at l_seq is open, one base before it closed; the same at query index 0", [STD],
     [R("22M8S", 990, T(10) + CAG[:20]), R("22M8S", 990, T(10) + CAG[:19] + "T"), R("8S22M", 1000, CAG[70:] + T(10)), R("8S22M", 1000, "T" + CAG[71:] + T(10)),
      R("22M", 990, T(10) + CAG[:12]), R("22M", 1000, CAG[78:] + T(10))],
     [((0, LEFT(20, True)), 1), ((0, LEFT(19)), 1), ((0, RIGHT(20, True)), 1), ((0, RIGHT(19)), 1), ((0, LEFT(12, True)), 1), ((0, RIGHT(12, True)), 1)],
     plain(6, left_keys=3, right_keys=3))
case("run", "a base that is not A C G T ends a run", [STD],
     [R("22M8S", 990, T(10) + "CAGCANCAG" + T(11)), R("8S22M", 1000, T(11) + "CAGNAGCAG" + T(10)), R("22M8S", 990, T(10) + "CAGCAMCAG" + T(11))],
     [((0, LEFT(5)), 2), ((0, RIGHT(5)), 1)], plain(3, left_keys=2, right_keys=1))

# ---- cigar: where the anchors fall in the CIGAR.  pos 990: a = 999 is query index 9 of a leading 10M
case("cigar", "an insertion directly behind a, inside the locus and directly in front of b; a deletion inside", [STD],
     [R("10M3I32M"), R("16M3I26M"), R("22M3I20M"), R("16M3D23M"), R("10M3I3D29M")],
     [((0, SPAN(15)), 3), ((0, SPAN(9)), 1), ((0, SPAN(12)), 1)], plain(5, span_keys=5))
# (8M4D: the deletion covers a, the read still counts from b leftwards; 20M5N: the skip covers b; 8M20D: both)
case("cigar", "a deletion or an N that covers an anchor: no anchor there", [STD],
     [R("8M4D30M", seq=T(8) + CAG[2:12] + T(20)), R("20M5N20M", seq=T(10) + CAG[:10] + T(20)), R("8M20D20M"), R("8M4N30M", seq=T(8) + CAG[2:12] + T(20))],
     [((0, RIGHT(10)), 2), ((0, LEFT(10)), 1)], plain(4, left_keys=1, right_keys=2, unanchored=1))
case("cigar", "= and X operations, hard clips and pads", [STD], [R("10=12X20="), R("5H10M12=18X5H"), R("10M2P30M")], [((0, SPAN(12)), 3)], plain(3, span_keys=3))
case("cigar", "anchors on the read's first and last aligned base, with and without clips", [STD],
     [R("14M", 999), R("5S14M5S", 999), R("13M", 999), R("13M", 1000)],
     [((0, SPAN(12)), 2), ((0, LEFT(0)), 1), ((0, RIGHT(0)), 1)], plain(4, span_keys=2, left_keys=1, right_keys=1), F=1)

# ---- flank: the two flank tests and the reach, F = 5
case("flank", "pos == s - F and one past it; end == e + F and one short of it; neither", [STD],
     [R("40M", 995), R("40M", 996, T(4) + CAG[:12] + T(24)), R("27M", 990), R("26M", 990, T(10) + CAG[:12] + T(4)), R("20M", 996)],
     [((0, SPAN(12)), 2), ((0, RIGHT(12)), 1), ((0, LEFT(12)), 1)], plain(5, span_keys=2, left_keys=1, right_keys=1, unanchored=1))
case("flank", "a locus in reach by one base on either side, and out of reach by one", [STD],
     [R("20M", 980), R("19M", 980), R("20M", 1012), R("20M", 1013)],
     [((0, LEFT(0, True)), 1), ((0, RIGHT(0, True)), 1)], dict(records=4, eligible=4, in_reach=2, left_keys=1, right_keys=1))

# ---- table: several loci in one read, the cap, neighbours one base apart, contig ends
_FIVE = [("c0", 1000 + 7 * k, 1006 + 7 * k, "CAG") for k in range(5)] + [("c2", 1, 7, "CAG"), ("c2", 993, 999, "CAG")]
case("table", "two to five loci in one read: the cap of four and over_cap; neighbours one base apart; loci at contig ends", _FIVE,
     [R("22M", 990, T(10) + "CAGCAG" + "T" + "CAGCA"), R("30M", 990), R("37M", 990), R("60M", 990), R("20M", 0, tid=2), R("20M", 980, tid=2)],
     [((0, SPAN(6)), 4), ((1, SPAN(6)), 3), ((2, SPAN(6)), 2), ((3, SPAN(6)), 1), ((1, LEFT(5, True)), 1), ((2, LEFT(0)), 1), ((3, LEFT(0)), 1),
      ((5, SPAN(6)), 1), ((6, SPAN(6)), 1)],
     plain(6, span_keys=12, left_keys=3, over_cap=1), F=1)

# ---- bad: records that are malformed, without alignment or without sequence emit nothing
_OP9 = ((36 + L_NAME, "<I", 40 * 16 + 9),)
case("bad", "malformed: l_seq < 0, an op code above 8, an anchor's query index >= l_seq, pos < 0; no_alignment; no_sequence", [STD],
     [R(), R(patch=((20, "<i", -1),)), R(patch=_OP9), R(seq=T(15)), R(seq=T(10)), R(pos=-1, end=1030), R(None, end=1030, seq=T(40)), R(seq=""),
      R("10M30S", seq=T(40), patch=((36 + L_NAME + 4, "<I", 30 * 16 + 11),))],
     [((0, SPAN(12)), 1)], plain(9, malformed=6, no_alignment=1, no_sequence=1, span_keys=1), reader_ok=False)
case("bad", "malformed: the header of the last record lies outside raw", [STD], [R(), R()], [((0, SPAN(12)), 1)], plain(2, malformed=1, span_keys=1),
     reader_ok=False, truncate_last=True)
case("bad", "malformed: the block reaches beyond raw; the body is larger than the block", [STD], [R(bs_delta=-8), R(), R(bs_delta=8)],
     [((0, SPAN(12)), 1)], plain(3, malformed=2, span_keys=1), reader_ok=False)

# ---- gate: every filter bit, the MAPQ cut at its edge, contigs
case("gate", "every flag bit of 0xF04, the others pass; MAPQ at Q - 1 and Q", [STD],
     [R(flag=f) for f in (0x4, 0x100, 0x200, 0x400, 0x800)] + [R(flag=0x1 | 0x2 | 0x20 | 0x40), R(flag=0x80 | REV), R(mapq=29), R(mapq=30)],
     [((0, SPAN(12)), 2), ((0, SPAN(12, 1)), 1)], dict(records=9, eligible=3, in_reach=3, span_keys=3), Q=30)
case("gate", "tid -1, a contig without loci, a contig beyond the table", [STD], [R(tid=-1), R(tid=1), R(tid=3), R(tid=2 ** 24), R()],
     [((0, SPAN(12)), 1)], dict(records=5, eligible=4, in_reach=1, span_keys=1), reader_ok=False)

# ---- merge: equal keys, the compaction's edges, the store
case("merge", "equal keys on both strands are one set", [STD], [R(), R(), R(flag=REV), R(), R(flag=REV), R("40M", 995, flag=REV), R("10M3I32M")],
     [((0, SPAN(12)), 3), ((0, SPAN(12, 1)), 3), ((0, SPAN(15)), 1)], plain(7, span_keys=7),
     rows=[(0, SPAN(12), 6, 3), (0, SPAN(15), 1, 0)])
for _n in (WAVE - 1, WAVE, WAVE + 1, STR_BLOCK, STR_BLOCK + 1):
    case("merge", "shape a batch of %d reads" % _n, [STD], [R()] * _n, [((0, SPAN(12)), _n)], plain(_n, span_keys=_n))
# (every third read spans, every third lies far away, every third is a duplicate: the two compactions pick different reads)
_N3 = STR_BLOCK + 1
case("merge", "shape a batch where a third of the reads has a locus in reach", [STD],
     [R() if i % 3 == 0 else R(pos=5000) if i % 3 == 1 else R(flag=0x400) for i in range(_N3)],
     [((0, SPAN(12)), (_N3 + 2) // 3)], dict(records=_N3, eligible=(_N3 + 2) // 3 + (_N3 + 1) // 3, in_reach=(_N3 + 2) // 3, span_keys=(_N3 + 2) // 3))
case("merge", "a store that grows from room for 64", [STD], [R()] * 65, [((0, SPAN(12)), 65)], plain(65, span_keys=65), capacity=64, grows=1, asks=1)
case("merge", "state two pushes and a repeat", [STD], [R(), R(flag=REV), R("26M", 990, T(10) + CAG[:12] + T(4)), R("10M3I32M")],
     [((0, SPAN(12)), 1), ((0, SPAN(12, 1)), 1), ((0, LEFT(12)), 1), ((0, SPAN(15)), 1)], plain(4, span_keys=3, left_keys=1), cuts=(1,), repeat=2,
     reader_ok=False)

N_CASES = len(CASES)
FAMILIES = sorted({c["family"] for c in CASES})


# ------------------------------------------------------------------------------------------- the genotype rule
# one locus of REF_LEN 12 (STD): spans {L: n}, flank rows [(kind, L, n)], S -> (SPAN_N, genotype or None, FLANK_N, FLANK_MAX, LONGER, HIST)
GENOTYPES = [
    ("a tie in n: the allele nearer REF_LEN is first", {12: 3, 15: 3}, [], 5, (6, (12, 3, 15, 3, "0/1"), 0, 0, 0, "12:3,15:3")),
    ("a tie in n and in the distance: the shorter one is first", {9: 3, 15: 3, 12: 1}, [], 5, (7, (9, 3, 15, 3, "1/2"), 0, 0, 0, "9:3,12:1,15:3")),
    ("a tie in n and in the distance for the second place", {12: 5, 9: 2, 15: 2}, [], 5, (9, (9, 2, 12, 5, "0/1"), 0, 0, 0, "9:2,12:5,15:2")),
    ("a second row of n = 1 is no allele", {12: 4, 15: 1}, [], 5, (5, (12, 4, 12, 4, "0/0"), 0, 0, 0, "12:4,15:1")),
    ("a second row of n = 2 is one", {12: 4, 15: 2}, [], 5, (6, (12, 4, 15, 2, "0/1"), 0, 0, 0, "12:4,15:2")),
    ("5 n one below SPAN_N", {12: 9, 15: 2}, [], 5, (11, (12, 9, 12, 9, "0/0"), 0, 0, 0, "12:9,15:2")),
    ("5 n at SPAN_N", {12: 8, 15: 2}, [], 5, (10, (12, 8, 15, 2, "0/1"), 0, 0, 0, "12:8,15:2")),
    ("S - 1 spanning reads: no genotype", {12: 4}, [], 5, (4, None, 0, 0, 0, "12:4")),
    ("S spanning reads", {12: 5}, [], 5, (5, (12, 5, 12, 5, "0/0"), 0, 0, 0, "12:5")),
    ("homozygous for another length", {15: 6}, [], 5, (6, (15, 6, 15, 6, "1/1"), 0, 0, 0, "15:6")),
    ("LONGER: an open run above the longer allele", {12: 3, 15: 3}, [(2, 16, 1), (4, 9, 2)], 5, (6, (12, 3, 15, 3, "0/1"), 3, 16, 1, "12:3,15:3")),
    ("LONGER off: an open run as long as the longer allele, a longer closed one", {12: 3, 15: 3}, [(2, 15, 1), (1, 40, 1), (3, 41, 2)], 5,
     (6, (12, 3, 15, 3, "0/1"), 4, 15, 0, "12:3,15:3")),
    ("LONGER without a genotype is against REF_LEN", {}, [(4, 13, 2)], 5, (0, None, 2, 13, 1, ".")),
    ("LONGER off without a genotype", {12: 1}, [(2, 12, 1)], 5, (1, None, 1, 12, 0, "12:1")),
]


def genotype_rows(spans, flanks, k1=0):
    """the sets of one locus as the finish gives them (REV 0)"""
    return sorted([(k1, SPAN(L), n, 0) for L, n in spans.items()] + [(k1, kind * 2 ** 33 + L * 2, n, 0) for kind, L, n in flanks])
