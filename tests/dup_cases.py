"""Aimed cases for the duplicate metrics (tiddit_amd/tiddit_dup.py, csrc/tdt_dup.hip): records built byte by byte, WITH aux fields, each
case with the keys and counters it claims, and a second, independent reference: a restatement that unpacks a record with one ``struct``
format, finds the aux fields with ``bytes.find`` and a table of formats, reads the ``MC`` text with a regular expression and counts the
sets with ``collections.Counter`` over tuples.  The definition (``tiddit_dup.key_of_read`` / ``summarise``) walks byte by byte and shifts;
the two share no code.

A case is a dict: ``reads`` (see :func:`R`), ``cuts`` (where the reads are cut into batches), ``repeat`` (the batches are pushed that many
times), ``capacity`` (of the store at its creation), and its claim, written down from the case's own numbers, never computed by either
reference:
  ``keys``  [((K1, K2, marked), how many)]: the keyed reads, spelled with :func:`K1` / :func:`K2` from contig, 5' end and strand;
  ``sn``    {name: n}: EVERY non-zero counter of the push;
  ``sets``  {("pair" | "frag", size): how many}: every set.
:func:`expected` turns a claim into the sorted key rows and the counter array.

``RS_TILE`` is read from the `#define` lines of csrc/tdt_sort.hip and ``DUP_TILE`` / ``DUP_BLOCK`` / ``DUP_K_TILE`` from those of csrc/tdt_dup.hip, so the
shape cases stay on their edges when a constant is retuned.

``reader_ok``: the case's records can also travel through a BAM file and the device reader.  Malformed records, records with broken aux
fields and contig ids outside the header cannot: the reader's own checks may refuse them before any consumer sees the batch, so
those go through ``tdt_dup_push`` only.

Mutants of the restatement (``reference(case, mutant=...)``), each caught inside the family named beside it:
  ``firstclip``  only the first / last clip operation counts      -> clips
  ``notrail``    no trailing clips on a reverse read              -> clips
  ``nomc``       ``MC`` ignored                                     -> mc
  ``notie``      the 0x40 tie-break of the carrier rule ignored   -> carrier
  ``nostrand``   the strand bits left out of the keys             -> sets
  ``histcap``    the histogram cap off by one                     -> sizes
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


RS_TILE = _define("tdt_sort.hip", "RS_THREADS") * _define("tdt_sort.hip", "RS_ROUNDS")      # (RS_TILE itself is their product)
DUP_TILE, DUP_BLOCK, DUP_K_TILE = (_define("tdt_dup.hip", k) for k in ("DUP_TILE", "DUP_BLOCK", "DUP_K_TILE"))
BIAS, HIST_MAX, TOP = 2 ** 28, 1024, 2 ** 33
SN = ("records", "eligible", "malformed", "fragments", "pairs", "pair_mates", "pairs_no_mc", "flagged", "fragment_sets", "pair_sets",
      "fragment_duplicates", "pair_duplicates")
OFF_HIST = 12
SIZE = OFF_HIST + 2 * HIST_MAX
MUTANTS = {"firstclip": "clips", "notrail": "clips", "nomc": "mc", "notie": "carrier", "nostrand": "sets", "histcap": "sizes"}
LENGTHS = (100000, 50000, 1000)
PAD_BYTE = 0x4d                              # "M": padding behind a record reads as aux text
L_NAME = 9                                   # "r%07d" and its NUL
PAIRED, MUNMAP, REV, MREV, R1, R2, DUPF = 0x1, 0x8, 0x10, 0x20, 0x40, 0x80, 0x400
MAXLEN = 2 ** 28 - 1                         # the longest CIGAR operation


def K1(tid, end5, rev):
    """the claim's spelling of a key: contig, unclipped 5' end (0-based), strand"""
    return tid * 2 ** 34 + (end5 + BIAS) * 2 + rev


def K2(mate_tid, mend5, mrev):
    return 2 ** 58 + mate_tid * 2 ** 34 + (mend5 + BIAS) * 2 + mrev


def R(cigar="10M", flag=0, tid=0, pos=100, mate_tid=-1, mate_pos=-1, tags=(), aux=b"", name=None, patch=(), pad=0):
    """one read.  cigar: string, [(op, len)] or None (no operations); tags: (tag, type, value) as bamio.encode_record takes them; aux: raw
    bytes appended behind the tags (inside block_size); name: the read name (default r%07d); patch: ((byte offset in the record, struct
    format, value), ...) applied to the encoded record; pad: bytes of PAD_BYTE behind the record in the push entry's buffer"""
    cig = [] if cigar is None else bamio.parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    return {"cigar": cig, "flag": flag, "tid": tid, "pos": pos, "mate_tid": mate_tid, "mate_pos": mate_pos, "tags": tuple(tags), "aux": aux,
            "name": name, "patch": tuple(patch), "pad": pad}


def P(cigar="10M", flag=PAIRED | R1, tid=0, pos=100, mate_tid=0, mate_pos=300, **kw):
    """a read of a pair; the defaults make it the carrier (pos < mate_pos)"""
    return R(cigar, flag, tid, pos, mate_tid, mate_pos, **kw)


def _record(i, r):
    rec = bamio.encode_record(r["name"] or "r%07d" % i, r["flag"], r["tid"], r["pos"], 60, r["cigar"], r["mate_tid"], r["mate_pos"], 0,
                              seq="A" * sum(l for op, l in r["cigar"] if op in (0, 1, 4, 7, 8) and l < 1000), tags=r["tags"])
    rec = bytearray(struct.pack("<i", len(rec) - 4 + len(r["aux"])) + rec[4:] + r["aux"])
    for off, fmt, val in r["patch"]:
        struct.pack_into(fmt, rec, off, val)
    return bytes(rec)


class Batch:
    """the columns of a run of reads over one raw buffer — what tdt_dup_push and the definition take"""
    COLUMNS = ("flag", "tid", "pos", "end", "mate_tid", "mate_pos", "rec_off")

    def __init__(self, raw, **cols):
        self.raw = raw
        for k in self.COLUMNS:
            setattr(self, k, cols[k])

    def __len__(self):
        return len(self.tid)

    def cut(self, lo, hi):
        return Batch(self.raw, **{k: getattr(self, k)[lo:hi] for k in self.COLUMNS})


def build_reads(reads, padding=True, truncate_last=False):
    """-> the reads as one Batch (padding=False: the records back to back, as a BAM file holds them).  The ``end`` column is htslib's
    bam_endpos, as the readers compute it: pos + the M D N = X lengths, pos + 1 when those are 0 or the read is unmapped."""
    parts, offs, o = [], [], 0
    for i, r in enumerate(reads):
        rec = _record(i, r)
        offs.append(o)
        parts.append(rec)
        o += len(rec)
        if padding and r["pad"]:
            parts.append(bytes([PAD_BYTE]) * r["pad"])
            o += r["pad"]
    col = lambda k, dt: np.array([r[k] for r in reads], dtype=dt)
    ends = [r["pos"] + (1 if r["flag"] & 0x4 else sum(l for op, l in r["cigar"] if op in (0, 2, 3, 7, 8)) or 1) for r in reads]
    b = Batch(np.frombuffer(b"".join(parts), dtype=np.uint8), flag=col("flag", np.uint16), tid=col("tid", np.int32), pos=col("pos", np.int32),
              end=np.array(ends, dtype=np.int32), mate_tid=col("mate_tid", np.int32), mate_pos=col("mate_pos", np.int32),
              rec_off=np.array(offs, dtype=np.uint64))
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


def rows_of(keys):
    """[(K1, K2, marked)] -> the sorted rows, uint64[n][3]"""
    return np.array(sorted(keys), dtype=np.uint64).reshape(-1, 3)


def counters_of(sn, sets):
    """a claim's counters as uint64[SIZE]: the push counters by name, every set by kind and size"""
    c = np.zeros(SIZE, dtype=np.uint64)
    for k, v in sn.items():
        assert v > 0, k
        c[SN.index(k)] = v
    for (kind, size), n in sets.items():
        assert kind in ("pair", "frag") and size >= 1 and n > 0
        frag = 1 if kind == "frag" else 0
        c[SN.index("fragment_sets" if frag else "pair_sets")] += n
        c[SN.index("fragment_duplicates" if frag else "pair_duplicates")] += n * (size - 1)
        c[OFF_HIST + 2 * (min(size, HIST_MAX) - 1) + frag] += n
    return c


def expected(case):
    """the claim -> (sorted key rows, counters)"""
    keys = [k for k, n in case["keys"] for _ in range(n)]
    return rows_of(keys), counters_of(case["sn"], case["sets"])


def definition(case):
    from tiddit_amd import tiddit_dup
    keys, sn = [], {}
    for b in batches(case):
        tiddit_dup.keys_of_batch_by_read(b, keys, sn)
    return rows_of(keys), tiddit_dup.summarise(keys, sn)


# ------------------------------------------------------------------------------------------- the restatement
_FIXED = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
_MC_RE = re.compile(rb"(?:[0-9]+[MIDNSHP=X])+")
_OP_RE = re.compile(rb"([0-9]+)([MIDNSHP=X])")


def _mc_of(aux):
    """the text of the first MC:Z of a block of aux bytes, or None"""
    while len(aux) >= 3:
        tag, ty, rest = aux[:2], aux[2:3], aux[3:]
        if ty in _FIXED:
            if len(rest) < _FIXED[ty]:
                return None
            aux = rest[_FIXED[ty]:]
        elif ty in (b"Z", b"H"):
            nul = rest.find(b"\x00")
            if nul < 0:
                return None
            if tag == b"MC" and ty == b"Z":
                return rest[:nul]
            aux = rest[nul + 1:]
        elif ty == b"B":
            if len(rest) < 5 or rest[:1] not in _FIXED or rest[:1] == b"A":
                return None
            size = 5 + _FIXED[rest[:1]] * struct.unpack("<I", rest[1:5])[0]
            if len(rest) < size:
                return None
            aux = rest[size:]
        else:
            return None
    return None


def _clips(ops, mutant):
    """[(letter, len)] -> (lead, trail)"""
    is_clip = [op in "SH" for op, _ in ops]
    if all(is_clip):
        return (ops[0][1] if mutant == "firstclip" and ops else sum(l for _, l in ops)), 0
    first, last = is_clip.index(False), len(ops) - 1 - is_clip[::-1].index(False)
    if mutant == "firstclip":
        return (ops[0][1] if is_clip[0] else 0), (ops[-1][1] if is_clip[-1] else 0)
    return sum(l for _, l in ops[:first]), sum(l for _, l in ops[last + 1:])


def reference_batch(b, keys, sn, mutant=None):
    raw = bytes(np.asarray(b.raw, dtype=np.uint8))
    for i in range(len(b)):
        f, tid, pos, end, mtid, mpos, ro = (int(getattr(b, k)[i]) for k in Batch.COLUMNS)
        sn["records"] += 1
        if f & 0x4 or f & 0x100 or f & 0x200 or f & 0x800 or tid < 0:
            continue
        sn["eligible"] += 1
        pair = f & 0x1 == 0x1 and f & 0x8 == 0 and mtid >= 0
        if pair:
            # (the two mates in coordinate order; a tie goes to the one with 0x40)
            tie = 0 if f & 0x40 and mutant != "notie" else 2
            if sorted([(tid, pos, tie, "me"), (mtid, mpos, 1, "mate")])[0][3] != "me":
                sn["pair_mates"] += 1
                continue
        if tid >= 2 ** 24 or (pair and mtid >= 2 ** 24) or len(raw) - ro < 36:
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
        lead, trail = _clips([("MIDNSHP=X"[w % 16], w // 16) for w in words], mutant)
        rev = (f // 16) % 2
        end5 = end - 1 + (0 if mutant == "notrail" else trail) if rev else pos - lead
        key = [(tid, end5, 0 if mutant == "nostrand" else rev), None]
        no_mc = False
        if pair:
            mrev = (f // 32) % 2
            text = _mc_of(raw[ro + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq:ro + 4 + bs])
            ops = None
            if mutant != "nomc" and text is not None and _MC_RE.fullmatch(text):
                ops = [(o.decode(), int(d)) for d, o in _OP_RE.findall(text)]
                if any(l >= 2 ** 28 for _, l in ops):
                    ops = None
            if ops is None:
                no_mc, mend5 = True, mpos
            else:
                mlead, mtrail = _clips(ops, None)
                mend5 = mpos + max(sum(l for o, l in ops if o in "MDN=X"), 1) - 1 + mtrail if mrev else mpos - mlead
            key[1] = (mtid, mend5, 0 if mutant == "nostrand" else mrev)
        if any(not -BIAS <= k[1] < TOP - BIAS for k in key if k):
            sn["malformed"] += 1
            continue
        sn["pairs" if pair else "fragments"] += 1
        sn["pairs_no_mc"] += no_mc
        sn["flagged"] += f & 0x400 == 0x400
        keys.append((K1(*key[0]), K2(*key[1]) if pair else 0, 1 if f & 0x400 else 0))


def reference(case, mutant=None, padding=True):
    """-> (sorted key rows, counters) of the whole case"""
    keys, sn = [], collections.Counter()
    for b in batches(case, padding):
        reference_batch(b, keys, sn, mutant)
    cap = HIST_MAX - 1 if mutant == "histcap" else HIST_MAX
    c = np.zeros(SIZE, dtype=np.uint64)
    for k, v in sn.items():
        c[SN.index(k)] = v
    for (k1, k2), size in collections.Counter((k1, k2) for k1, k2, _ in keys).items():
        frag = 1 if k2 < 2 ** 58 else 0
        c[SN.index("fragment_sets" if frag else "pair_sets")] += 1
        c[SN.index("fragment_duplicates" if frag else "pair_duplicates")] += size - 1
        c[OFF_HIST + 2 * (min(size, cap) - 1) + frag] += 1
    return rows_of(keys), c


# ------------------------------------------------------------------------------------------- the cases
CASES = []


def case(family, name, reads, keys, sn, sets, cuts=(), repeat=1, capacity=None, reader_ok=True, **more):
    assert sum(n for _, n in keys) * 1 == sn.get("fragments", 0) + sn.get("pairs", 0), name
    assert sum(size * n for (_, size), n in sets.items()) == sum(n for _, n in keys), name
    CASES.append(dict(more, family=family, name=family + " " + name, reads=reads, keys=keys, sn=sn, sets=sets, cuts=tuple(cuts), repeat=repeat,
                      capacity=capacity, reader_ok=reader_ok, lengths=LENGTHS))


def frags(*end5_rev, tid=0):
    """the keys of single fragments: (end5, rev), ..."""
    return [((K1(tid, e, r), 0, 0), 1) for e, r in end5_rev]


def plain(n, **more):
    """the push counters of n eligible fragments"""
    return dict({"records": n, "eligible": n, "fragments": n}, **more)


# ---- clips: the own 5' end
case("clips", "H", [R("5H10M"), R("10M5H", REV)], frags((95, 0), (114, 1)), plain(2), {("frag", 1): 2})
case("clips", "S", [R("5S10M"), R("10M5S", REV)], frags((95, 0), (114, 1)), plain(2), {("frag", 1): 2})
case("clips", "H then S, leading and trailing", [R("3H4S10M"), R("10M4S3H", REV), R("3H4S10M", REV), R("10M4S3H")],
     frags((93, 0), (116, 1), (109, 1), (100, 0)), plain(4), {("frag", 1): 4}, cuts=(1, 3))
case("clips", "on both ends", [R("2S10M3S"), R("2S10M3S", REV), R("1H2S10M3S4H"), R("1H2S10M3S4H", REV)],
     frags((98, 0), (112, 1), (97, 0), (116, 1)), plain(4), {("frag", 1): 4})
# (a CIGAR of clips only: all of it leads, nothing trails; its reference length is 0, so end = pos + 1)
case("clips", "only", [R("5S3H"), R("5S3H", REV), R("7H"), R("7H", REV)], frags((92, 0), (100, 1), (93, 0), (100, 1)), plain(4),
     {("frag", 1): 2, ("frag", 2): 1})
case("clips", "no operations", [R(None), R(None, REV), R(None, pos=0), R(None, REV, pos=0)], frags((100, 0), (100, 1), (0, 0), (0, 1)), plain(4),
     {("frag", 1): 4})
# (a reference length of 0 behaves as 1: end - 1 = pos)
case("clips", "a reference length of 0", [R("5I"), R("5I", REV), R("2S5I3S", REV), R("2S5I3S")], frags((100, 0), (100, 1), (103, 1), (98, 0)), plain(4),
     {("frag", 1): 4})
# (clips between aligned operations are no clips of an end: only what leads and trails counts)
case("clips", "inside the alignment", [R("2S4M3S4M1S"), R("2S4M3S4M1S", REV)], frags((98, 0), (108, 1)), plain(2), {("frag", 1): 2})
# ---- range: E = end5 + 2^28 in [0, 2^33)
_LOW = [(5, MAXLEN), (5, 1), (0, 1)]                                                  # pos 0, 2^28 of hard clip in front: end5 = -2^28
case("range", "end5 on -DUP_BIAS and one below", [R(_LOW, pos=0), R([(5, MAXLEN), (5, 2), (0, 1)], pos=0), R("1M", pos=0)],
     frags((-BIAS, 0), (0, 0)), plain(3, fragments=2, malformed=1), {("frag", 1): 2})
_HIGH = [(0, 1)] + [(5, MAXLEN)] * 31                                                 # reverse at pos 0: end5 = 0 + 31 * (2^28 - 1) + the last clip
assert 31 * MAXLEN + 30 + BIAS == TOP - 1
case("range", "end5 on the top of the range and one above", [R(_HIGH + [(5, 30)], REV, pos=0), R(_HIGH + [(5, 31)], REV, pos=0), R("1M", REV, pos=0)],
     frags((TOP - 1 - BIAS, 1), (0, 1)), plain(3, fragments=2, malformed=1), {("frag", 1): 2})
case("range", "contig ids of 2^24", [R(tid=2 ** 24), R(tid=2 ** 24 - 1), P(tid=5, mate_tid=2 ** 24), P(tid=5, mate_tid=2 ** 24 - 1)],
     frags((100, 0), tid=2 ** 24 - 1) + [((K1(5, 100, 0), K2(2 ** 24 - 1, 300, 0), 0), 1)],
     {"records": 4, "eligible": 4, "malformed": 2, "fragments": 1, "pairs": 1, "pairs_no_mc": 1}, {("frag", 1): 1, ("pair", 1): 1}, reader_ok=False)
# ---- malformed: each bound, an op code of 9.  The padding behind a record reads as 'M': a missing bound would find text there.
_GOOD = [R("10M", pos=50), R("10M", pos=60)]
_BAD_SN = plain(3, fragments=2, malformed=1)
_BAD_KEYS = frags((50, 0), (60, 0))
case("malformed", "the fixed fields end behind the buffer", _GOOD + [R("10M")], _BAD_KEYS, _BAD_SN, {("frag", 1): 2}, reader_ok=False, truncate_last=True)
case("malformed", "the fields are longer than block_size", [_GOOD[0], R("10M", patch=((0, "<I", 32 + L_NAME + 4 + 5 + 10 - 1),), pad=64), _GOOD[1]], _BAD_KEYS,
     _BAD_SN, {("frag", 1): 2}, reader_ok=False)
case("malformed", "block_size ends behind the buffer", _GOOD + [R("10M", patch=((0, "<I", 32 + L_NAME + 4 + 5 + 10 + 1),))], _BAD_KEYS, _BAD_SN,
     {("frag", 1): 2}, reader_ok=False)
case("malformed", "a negative l_seq", [_GOOD[0], R("10M", patch=((4 + 16, "<i", -1),), pad=64), _GOOD[1]], _BAD_KEYS, _BAD_SN, {("frag", 1): 2},
     reader_ok=False)
case("malformed", "an op code of 9", [_GOOD[0], R("2S10M", patch=((4 + 32 + L_NAME, "<I", 2 << 4 | 9),), pad=64), _GOOD[1]], _BAD_KEYS, _BAD_SN,
     {("frag", 1): 2}, reader_ok=False)
# ---- mc: the walk over the aux fields and the text.  A carrier at tid 0 pos 100, its mate at mate_pos; "3S10M2D5M4S": mlead 3, mref 17, mtrail 4
_MC = ("MC", "Z", "3S10M2D5M4S")
_CAR = K1(0, 100, 0)


def pairs_sn(n, no_mc=0, **more):
    sn = {"records": n, "eligible": n, "pairs": n}
    if no_mc:
        sn["pairs_no_mc"] = no_mc
    sn.update(more)
    return sn


def carriers(*mend5_mrev):
    return [((_CAR, K2(0, e, r), 0), 1) for e, r in mend5_mrev]


case("mc", "first and last, a mate that is forward and one that is reverse",
     [P(tags=(_MC, ("NM", "i", 1))), P(tags=(("NM", "i", 1), _MC)), P(flag=PAIRED | R1 | MREV, tags=(_MC, ("NM", "i", 1))),
      P(flag=PAIRED | R1 | MREV, tags=(("NM", "i", 1), ("XS", "A", "x"), _MC))],
     [((_CAR, K2(0, 297, 0), 0), 2), ((_CAR, K2(0, 320, 1), 0), 2)], pairs_sn(4), {("pair", 2): 2}, cuts=(2,))
_TYPES = [("A", "M"), ("c", -3), ("C", 77), ("s", -300), ("S", 60000), ("i", -70000), ("I", 4000000000), ("f", 1.5), ("Z", "text"), ("H", "4D43"),
          ("Bc", [-1, 2]), ("BC", [77, 67, 90]), ("Bs", [-300]), ("BS", [1, 2, 3]), ("Bi", [-70000, 1]), ("BI", [4000000000]), ("Bf", [0.5, 1.5]), ("BC", [])]
case("mc", "behind each aux type", [P(mate_pos=300 + 10 * k, tags=(("X%d" % (k % 10), ty, v), _MC)) for k, (ty, v) in enumerate(_TYPES)],
     carriers(*[(297 + 10 * k, 0) for k in range(len(_TYPES))]), pairs_sn(len(_TYPES)), {("pair", 1): len(_TYPES)}, cuts=(7,))
case("mc", "decoy bytes in Z, H and B:C values and in the read name",
     [P(tags=(("XZ", "Z", "MCZ9S1M"), _MC)), P(mate_pos=310, tags=(("XH", "H", "MCZ9S1M"), _MC)),
      P(mate_pos=320, tags=(("XB", "BC", [77, 67, 90, 57, 83, 49, 77, 0]), _MC)), P(mate_pos=330, name="MCZ9S1M", tags=(_MC,)),
      P(mate_pos=340, tags=(("XZ", "Z", "MCZ9S1M"),)), P(mate_pos=350, name="MCZ9S1M")],
     carriers((297, 0), (307, 0), (317, 0), (327, 0), (340, 0), (350, 0)), pairs_sn(6, 2), {("pair", 1): 6})
case("mc", "MC:A and MC:i are not the tag", [P(tags=(("MC", "A", "S"), ("MC", "i", 5), ("MC", "Z", "5S10M"))), P(mate_pos=310, tags=(("MC", "A", "S"),)),
                                             P(mate_pos=320, tags=(("MC", "i", 7),)), P(mate_pos=330, tags=(("MC", "H", "5S"), ("MC", "Z", "6S1M")))],
     carriers((295, 0), (310, 0), (320, 0), (324, 0)), pairs_sn(4, 2), {("pair", 1): 4})
_REVP = PAIRED | R1 | MREV
case("mc", "texts that are no CIGAR", [P(mate_pos=300 + 10 * k, tags=(("MC", "Z", t),)) for k, t in enumerate(("*", "", "268435456M", "10M5", "M", "10Q", "5S 10M", "-5M", "10m"))],
     carriers(*[(300 + 10 * k, 0) for k in range(9)]), pairs_sn(9, 9), {("pair", 1): 9})
# (2^28 - 1 is a number: mend5 = 300 - (2^28 - 1); a long run of digits is a small number; I and P hold no reference: mref = max(0, 1))
case("mc", "texts on their edges", [P(tags=(("MC", "Z", "268435455S10M"),)), P(tags=(("MC", "Z", "0000000000000000000005S10M"),)),
                                    P(flag=_REVP, tags=(("MC", "Z", "5S3I2P4S"),)), P(flag=_REVP, tags=(("MC", "Z", "5S3H"),)), P(tags=(("MC", "Z", "5S3H"),)),
                                    P(flag=_REVP, tags=(("MC", "Z", "2S1M1D1N1=1X3H"),)), P(flag=_REVP, tags=(("MC", "Z", "0M"),))],
     carriers((301 - BIAS, 0), (295, 0), (304, 1), (300, 1), (292, 0), (307, 1), (300, 1)), pairs_sn(7), {("pair", 1): 5, ("pair", 2): 1})
# (the first MC:Z wins also when it is unusable; a mate end below the range makes the record malformed)
case("mc", "the first MC:Z wins, a mate end outside the range", [P(tags=(("MC", "Z", "*"), ("MC", "Z", "5S10M"))), P(mate_pos=310, tags=(("MC", "Z", "4S1M"), ("MC", "Z", "5S10M"))),
                                                                  P(tags=(("MC", "Z", "268435455S268435455S10M"),)), P(mate_pos=-1, flag=PAIRED | R1, tid=0, pos=-1)],
     carriers((300, 0), (306, 0)) + [((K1(0, -1, 0), K2(0, -1, 0), 0), 1)], pairs_sn(4, 2, pairs=3, malformed=1), {("pair", 1): 3}, reader_ok=False)
# (broken fields end the walk: the record keeps mend5 = mate_pos; the padding behind the record is 'M' bytes, never read)
case("mc", "fields that run past the block",
     [P(aux=b"MCZ5S10M", pad=32), P(mate_pos=310, aux=b"XYi\x01\x02", pad=32), P(mate_pos=320, aux=b"XBBi\x03\x00\x00\x00" + b"\x00" * 11, pad=32),
      P(mate_pos=330, aux=b"XQq\x00MCZ5S10M\x00", pad=32), P(mate_pos=340, aux=b"XBBA\x01\x00\x00\x00AMCZ5S10M\x00", pad=32), P(mate_pos=350, aux=b"MC", pad=32),
      P(mate_pos=360, aux=b"XBBC\xff\xff\xff\xff", pad=32), P(mate_pos=370, aux=b"XZZabc", pad=32), P(mate_pos=380, aux=b"XBB", pad=32),
      P(mate_pos=390, tags=(("XZ", "Z", "ok"),), aux=b"MCZ5S10M\x00")],
     carriers(*[(300 + 10 * k, 0) for k in range(9)] + [(385, 0)]), pairs_sn(10, 9), {("pair", 1): 10}, reader_ok=False)
# ---- carrier: who of a pair holds the key
case("carrier", "pairs across contigs", [P(tid=0, pos=500, mate_tid=1, mate_pos=10), P(flag=PAIRED | R2, tid=1, pos=10, mate_tid=0, mate_pos=500),
                                         P(tid=1, pos=5, mate_tid=2, mate_pos=5), P(flag=PAIRED | R2, tid=2, pos=5, mate_tid=1, mate_pos=5)],
     [((K1(0, 500, 0), K2(1, 10, 0), 0), 1), ((K1(1, 5, 0), K2(2, 5, 0), 0), 1)],
     {"records": 4, "eligible": 4, "pairs": 2, "pair_mates": 2, "pairs_no_mc": 2}, {("pair", 1): 2})
case("carrier", "the smaller position, whichever mate is read 1", [P(flag=PAIRED | R2, pos=100, mate_pos=300), P(flag=PAIRED | R1, pos=300, mate_pos=100),
                                                                   P(flag=PAIRED | R1 | REV, pos=291, mate_pos=100)],
     [((K1(0, 100, 0), K2(0, 300, 0), 0), 1)], {"records": 3, "eligible": 3, "pairs": 1, "pair_mates": 2, "pairs_no_mc": 1}, {("pair", 1): 1})
# (equal (tid, pos): read 1 carries; 0x40 on both: both carry; on neither: nobody does)
case("carrier", "equal coordinates", [P(flag=PAIRED | R1, pos=100, mate_pos=100), P(flag=PAIRED | R2, pos=100, mate_pos=100),
                                      P(flag=PAIRED | R1 | R2, tid=1, pos=7, mate_tid=1, mate_pos=7), P(flag=PAIRED | R1 | R2, tid=1, pos=7, mate_tid=1, mate_pos=7),
                                      P(flag=PAIRED, tid=2, pos=9, mate_tid=2, mate_pos=9), P(flag=PAIRED, tid=2, pos=9, mate_tid=2, mate_pos=9)],
     [((K1(0, 100, 0), K2(0, 100, 0), 0), 1), ((K1(1, 7, 0), K2(1, 7, 0), 0), 2)],
     {"records": 6, "eligible": 6, "pairs": 3, "pair_mates": 3, "pairs_no_mc": 3}, {("pair", 1): 1, ("pair", 2): 1}, cuts=(3,))
case("carrier", "mates that make a fragment, records that are not eligible",
     [P(flag=PAIRED | R1 | MUNMAP, pos=300, mate_pos=100), P(flag=PAIRED | R1, pos=310, mate_tid=-1, mate_pos=100), R(flag=R1, pos=320, mate_tid=0, mate_pos=100),
      R(flag=0x4, pos=330), R(flag=0x100, pos=340), R(flag=0x800, pos=350), R(flag=0x200, pos=360), R(tid=-1, pos=370), R(flag=DUPF, pos=380),
      P(flag=PAIRED | R1 | DUPF, tags=(_MC,)), P(flag=PAIRED | R2 | DUPF, pos=300, mate_pos=100)],
     frags((300, 0), (310, 0), (320, 0)) + [((K1(0, 380, 0), 0, 1), 1), ((_CAR, K2(0, 297, 0), 1), 1)],
     {"records": 11, "eligible": 6, "fragments": 4, "pairs": 1, "pair_mates": 1, "flagged": 2}, {("frag", 1): 4, ("pair", 1): 1}, cuts=(4, 9))
# ---- sets: keys that differ in exactly one field are different sets
_BASE = dict(tid=1, pos=100, mate_tid=1, mate_pos=300)
case("sets", "pairs that differ in one field",
     [P(**_BASE), P(**_BASE), P(**dict(_BASE, tid=0)), P(**dict(_BASE, pos=101)), P(flag=PAIRED | R1 | REV, **dict(_BASE, pos=91)),
      R(flag=0, tid=1, pos=100), P(**dict(_BASE, mate_tid=2)), P(**dict(_BASE, mate_pos=301)), P(flag=PAIRED | R1 | MREV, **_BASE)],
     [((K1(1, 100, 0), K2(1, 300, 0), 0), 2), ((K1(0, 100, 0), K2(1, 300, 0), 0), 1), ((K1(1, 101, 0), K2(1, 300, 0), 0), 1),
      ((K1(1, 100, 1), K2(1, 300, 0), 0), 1), ((K1(1, 100, 0), 0, 0), 1), ((K1(1, 100, 0), K2(2, 300, 0), 0), 1), ((K1(1, 100, 0), K2(1, 301, 0), 0), 1),
      ((K1(1, 100, 0), K2(1, 300, 1), 0), 1)],
     {"records": 9, "eligible": 9, "fragments": 1, "pairs": 8, "pairs_no_mc": 8}, {("pair", 2): 1, ("pair", 1): 6, ("frag", 1): 1}, cuts=(5,))
case("sets", "fragments that differ in one field, marks that do not matter",
     [R(tid=1), R(tid=1, flag=DUPF), R(tid=0), R(tid=1, pos=101), R(tid=1, pos=91, flag=REV), R("3S7M", tid=1, pos=103), R("7M3S", REV, tid=1, pos=93)],
     [((K1(1, 100, 0), 0, 0), 2), ((K1(1, 100, 0), 0, 1), 1), ((K1(0, 100, 0), 0, 0), 1), ((K1(1, 101, 0), 0, 0), 1), ((K1(1, 100, 1), 0, 0), 1),
      ((K1(1, 102, 1), 0, 0), 1)], plain(7, flagged=1), {("frag", 3): 1, ("frag", 1): 4})
# ---- sizes: the histogram and its last row
_SIZES = (1, 2, 63, 64, 65, HIST_MAX - 1, HIST_MAX, HIST_MAX + 1)
_PSIZES = (1, 2, 63, 64, 65, HIST_MAX + 1)
case("sizes", "sets of 1 2 63 64 65 and round DUP_HIST_MAX",
     [R(pos=1000 * k) for k, s in enumerate(_SIZES) for _ in range(s)] + [P(pos=10 * k, mate_pos=20000) for k, s in enumerate(_PSIZES) for _ in range(s)],
     [((K1(0, 1000 * k, 0), 0, 0), s) for k, s in enumerate(_SIZES)] + [((K1(0, 10 * k, 0), K2(0, 20000, 0), 0), s) for k, s in enumerate(_PSIZES)],
     {"records": sum(_SIZES) + sum(_PSIZES), "eligible": sum(_SIZES) + sum(_PSIZES), "fragments": sum(_SIZES), "pairs": sum(_PSIZES), "pairs_no_mc": sum(_PSIZES)},
     dict([(("frag", s), 1) for s in _SIZES] + [(("pair", s), 1) for s in _PSIZES]), cuts=(1000, 3000))
assert (2 * RS_TILE + 1) % 3 == 0
case("sizes", "one set of 2 RS_TILE + 1 copies through repeated pushes", [R("2S8M", pos=102)] * ((2 * RS_TILE + 1) // 3), [((K1(0, 100, 0), 0, 0), 2 * RS_TILE + 1)],
     plain(2 * RS_TILE + 1), {("frag", 2 * RS_TILE + 1): 1}, repeat=3, reader_ok=False)
# ---- shape: batches round the wave and the workgroup; stores round the tile


def _mix(n):
    """read i by i % 4: a fragment at 10 i; a carrier at 10 i with its mate at 10 i + 200; a mate (behind its carrier); an unmapped read"""
    reads = [(R(pos=10 * i), P(pos=10 * i, mate_pos=10 * i + 200), P(flag=PAIRED | R2, pos=10 * i + 190, mate_pos=10 * i - 10), R(flag=0x4, pos=10 * i))[i % 4]
             for i in range(n)]
    keys = [((K1(0, 10 * i, 0), 0, 0), 1) for i in range(0, n, 4)] + [((K1(0, 10 * i, 0), K2(0, 10 * i + 200, 0), 0), 1) for i in range(1, n, 4)]
    nf, npair, nm, nu = (len(range(k, n, 4)) for k in range(4))
    sn = {k: v for k, v in (("records", n), ("eligible", n - nu), ("fragments", nf), ("pairs", npair), ("pairs_no_mc", npair), ("pair_mates", nm)) if v}
    return reads, keys, sn, {k: v for k, v in ((("frag", 1), nf), (("pair", 1), npair)) if v}


# (a wave, a round of a workgroup, the tile of a workgroup: one more read starts the next)
for _n in (1, DUP_BLOCK // 4 - 1, DUP_BLOCK // 4, DUP_BLOCK // 4 + 1, DUP_BLOCK + 1, DUP_K_TILE, DUP_K_TILE + 1):
    case("shape", "a batch of %d reads" % _n, *_mix(_n))
case("shape", "a store that grows from a capacity of 64", *_mix(4 * DUP_BLOCK + 1), cuts=(64, 128, 192, 256, 320, 600), capacity=64)


def _runs(sizes, seed):
    """fragments whose sorted store holds runs of these sizes in this order (run r at position 10 + r), pushed shuffled"""
    reads = [R(pos=10 + r) for r, s in enumerate(sizes) for _ in range(s)]
    order = np.random.default_rng(seed).permutation(len(reads))
    sets = collections.Counter(("frag", s) for s in sizes)
    return [reads[k] for k in order], [((K1(0, 10 + r, 0), 0, 0), s) for r, s in enumerate(sizes)], plain(len(reads)), dict(sets)


for _t in sorted({RS_TILE, DUP_TILE}):
    case("shape", "a store of %d - 1 keys, a run that ends the store" % _t, *_runs([1] * (_t - 3) + [2], 1), cuts=(1000,), reader_ok=False)
    case("shape", "a store of %d keys, a run that ends on the tile boundary" % _t, *_runs([1] * (_t - 2) + [2], 2), reader_ok=False)
    case("shape", "a store of %d + 1 keys, a run that crosses the boundary" % _t, *_runs([1] * (_t - 1) + [2], 3), reader_ok=False)
    case("shape", "a store of %d + 1 keys, a run that starts on the boundary" % _t, *_runs([2] + [1] * (_t - 2) + [1], 4), reader_ok=False)
    # (the second tile holds no run head at all: the carry of the first one reaches the third)
    case("shape", "a store of 2 x %d + 1 keys, a run over a whole tile" % _t, *_runs([1] * (_t - 2) + [_t + 2] + [1], 5), cuts=(_t, _t + 7), reader_ok=False)

N_CASES = 45
FAMILIES = sorted({c["family"] for c in CASES})
