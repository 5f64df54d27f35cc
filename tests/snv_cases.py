"""Aimed cases for the SNV candidates (tiddit_amd/tiddit_snvs.py, csrc/tdt_snv.hip): records built byte by byte with
``bamio.encode_record`` over a designed reference, each case with the keys and counters it claims, written down from what the case
PLANTED (where a base was changed, with which quality, on which strand) and from the kind each read is stated to have — never computed
by the definition or by the restatement of tests/test_snv_refs_cpu.py.

The reference (``TEXT``; ``host_reference()`` gives it as a ``refseq.HostReference``): contig 0 holds plain bases, an ``N`` run, a
lower-case stretch and a stretch of IUPAC codes; contigs 1 ... 5 have 1, 15, 16, 17 and 33 bases; contig 6 ends where contig 7 begins
with the bases that would continue it (a read that overhangs contig 6 by one base would match there: it is off the reference all the
same); contig 8 holds every reference code 16 times; contig 9 is in the header and NOT loaded.

A case is a dict: ``batches`` (the pushes, in order: lists of reads, each list over its own raw buffer), ``capacity`` (of the store at
its creation), ``Q`` / ``B`` (of the handle), ``S`` (the minimum supports the finish is asked for), ``family`` and what it claims in
``claims`` (a sentence).  A read (:func:`rd`) carries what was planted in it: ``events`` [(P, ref, alt)], ``low`` (mismatches planted
below the quality cut), ``aligned`` (its ``M = X`` bases) and its stated ``kind``.  :func:`expected` turns that into the sorted key rows
and, per S, the counter array and the four row columns (``collections.Counter`` over the planted events)."""
import collections
import struct

import numpy as np

from tiddit_amd import bamio, refseq

SN = ("records", "eligible", "malformed", "no_sequence", "off_reference", "aligned_bases", "low_quality", "noisy_reads", "reads_with_events",
      "mismatches", "distinct_events", "reported_events")
SIZE = 12
COLUMNS = ("flag", "tid", "pos", "mapq", "rec_off")
REV = 0x10
NOT_ELIGIBLE, MALFORMED, NO_SEQUENCE, OFF_REFERENCE, NOISY, OK = "not_eligible", "malformed", "no_sequence", "off_reference", "noisy", "ok"
SNV_BLOCK = 256                               # the reads of a snv_keys workgroup
KS_TILE = 4096                                # the keys of a run-length workgroup
CODES = "=ACMGRSVTWYHKDBN"

_rng = np.random.default_rng(77031)


def _acgt(n):
    """n bases of ACGT, no two neighbours equal (a changed base never equals its neighbour's reference by accident of the test)"""
    out, last = [], -1
    for v in _rng.integers(0, 3, n).tolist():
        last = (last + 1 + v) % 4 if last >= 0 else v
        out.append("ACGT"[last])
    return "".join(out)


N_RUN, LOWER, IUPAC = (400, 420), (420, 520), (520, 540)
_MAIN = _acgt(400) + "N" * 20 + _acgt(100).lower() + "RYKMSWBDHVNRYKMSWBDH" + _acgt(660)
_LEFT = _acgt(64)
TEXT = [_MAIN, _acgt(1), _acgt(15), _acgt(16), _acgt(17), _acgt(33), _LEFT, _acgt(64), "".join(c * 16 for c in CODES[1:]), _acgt(500)]
LENGTHS = tuple(len(t) for t in TEXT)
LOADED = tuple(range(9))                      # contig 9 is not loaded
NAMES = tuple("c%d" % t for t in range(len(TEXT)))
CODE_CONTIG, UNLOADED = 8, 9


def host_reference():
    return refseq.HostReference({t: refseq.codes_of_bases(TEXT[t]) for t in LOADED})


def other(base):
    """the base a planted mismatch carries instead of ``base``"""
    return "ACGT"[("ACGT".index(base.upper()) + 1) % 4]


# ------------------------------------------------------------------------------------------- a read and what is planted in it
def rd(tid=0, pos=0, cigar="20M", mm=(), low=(), alt=None, flag=0, mapq=60, kind=OK, qual=40, low_qual=0, seq=None, quals=None, ops=None, patch=(),
       bs_delta=0, over=None):
    """one read of the reference at ``pos`` with this CIGAR.  ``mm``: the query indices (inside M / = / X operations) where the base is
    changed to ``alt`` (default: :func:`other` of the reference base) with quality ``qual`` — the read's EVENTS; ``low``: the same with
    quality ``low_qual`` — counted as low quality, no events; ``over``: {query index: base} written as it is and claimed as nothing (the
    case says why); ``seq`` / ``quals``: the bases / quality bytes instead of the built ones; ``ops``: [(op, len)] instead of a CIGAR
    string; ``patch``: ((byte offset in the record, struct format, value), ...); ``bs_delta``: added to block_size; ``kind``: what the
    case STATES the definition makes of the read."""
    cig = list(ops) if ops is not None else bamio.parse_cigar(cigar) if cigar else []
    text = TEXT[tid] if 0 <= tid < len(TEXT) else ""
    bases, where, r = [], [], pos                                 # where[q] = the reference position under query base q, or None
    for op, ln in cig:
        if op in (0, 7, 8):
            for k in range(ln):
                inside = 0 <= r + k < len(text)
                bases.append(text[r + k].upper() if inside else "A")
                where.append(r + k if inside else None)
        elif op in (1, 4):
            bases += ["T" if (len(bases) + k) % 2 else "G" for k in range(ln)]
            where += [None] * ln
        if op in (0, 2, 3, 7, 8):
            r += ln
    q = [qual] * len(bases)
    events = []
    for qi in list(mm) + list(low):
        ref = bases[qi]
        assert where[qi] is not None and ref in "ACGT", (tid, pos, cigar, qi)
        bases[qi] = alt or other(ref)
        if qi in mm:
            events.append((where[qi] + 1, ref, bases[qi]))
        else:
            q[qi] = low_qual
    for qi, b in (over or {}).items():
        bases[qi] = b
    aligned = sum(ln for op, ln in cig if op in (0, 7, 8))
    walks = kind in (OK, NOISY)
    return {"cigar": cig, "flag": flag, "tid": tid, "pos": pos, "mapq": mapq, "seq": "".join(bases) if seq is None else seq,
            "qual": bytes(q) if quals is None else quals, "patch": tuple(patch), "bs_delta": bs_delta, "kind": kind,
            "events": events, "low": len(low) if walks else 0, "aligned": aligned if walks else 0}


def _record(i, r):
    near = 0 <= r["pos"] < 2 ** 29                               # (the bin field of a far or negative pos does not fit: pos is written afterwards)
    rec = bytearray(bamio.encode_record("r%d" % i, r["flag"], r["tid"], r["pos"] if near else 0, r["mapq"], r["cigar"], -1, -1, 0, seq=r["seq"],
                                        qual=r["qual"] if len(r["qual"]) == len(r["seq"]) else None))
    struct.pack_into("<i", rec, 8, r["pos"])
    if r["bs_delta"]:
        struct.pack_into("<I", rec, 0, len(rec) - 4 + r["bs_delta"])
    for off, fmt, val in r["patch"]:
        struct.pack_into(fmt, rec, off, val)
    return bytes(rec)


class Batch:
    """the columns of a run of reads over one raw buffer — what tdt_snv_push and the definition take"""

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
    # (not a column of tdt_snv_push: the end of the read on the reference as the decoder gives it, for tiddit_alleles.count_batch)
    b.end = np.array([r["pos"] + (sum(ln for op, ln in r["cigar"] if op in (0, 2, 3, 7, 8)) or 1) for r in reads], dtype=np.int64)
    return b


def batches(case):
    if "built" not in case:
        case["built"] = [build_batch(reads, cut) for reads, cut in case["batches"]]
    return case["built"]


def cigar_word_offset(r_name_len, j):
    """the byte offset of CIGAR word j in a record whose read name has that many characters"""
    return 36 + r_name_len + 1 + 4 * j


# ------------------------------------------------------------------------------------------- the claim
def K1(tid, P):
    return tid * 2 ** 32 + P


def K2(ref, alt, rev=0):
    return "ACGT".index(ref) * 8 + "ACGT".index(alt) * 2 + rev


def key_rows(keys):
    """[(K1, K2)] -> the sorted rows, uint64[n][2]"""
    return np.array(sorted(keys), dtype=np.uint64).reshape(-1, 2)


def row_columns(rows):
    return (np.array([r[0] for r in rows], dtype=np.uint64), np.array([r[1] for r in rows], dtype=np.uint64),
            np.array([r[2] for r in rows], dtype=np.uint32), np.array([r[3] for r in rows], dtype=np.uint32))


def claimed(case):
    """-> (keys [(K1, K2)], sn {name: n}) from what the case planted and states"""
    keys, sn = [], collections.Counter()
    for reads, _ in case["batches"]:
        for r in reads:
            sn["records"] += 1
            if r["kind"] == NOT_ELIGIBLE:
                continue
            sn["eligible"] += 1
            sn["aligned_bases"] += r["aligned"]
            sn["low_quality"] += r["low"]
            if r["kind"] != OK:
                sn[{MALFORMED: "malformed", NO_SEQUENCE: "no_sequence", OFF_REFERENCE: "off_reference", NOISY: "noisy_reads"}[r["kind"]]] += 1
                continue
            if r["events"]:
                sn["reads_with_events"] += 1
                sn["mismatches"] += len(r["events"])
            rev = 1 if r["flag"] & REV else 0
            keys += [(K1(r["tid"], P), K2(ref, alt, rev)) for P, ref, alt in r["events"]]
    return keys, sn


def counters_of(sn, distinct, reported):
    c = np.zeros(SIZE, dtype=np.uint64)
    for k, v in sn.items():
        c[SN.index(k)] = v
    c[10], c[11] = distinct, reported
    return c


def sets_of(keys, S, strict=False):
    size = collections.Counter((k1, k2 - k2 % 2) for k1, k2 in keys)
    rev = collections.Counter((k1, k2 - k2 % 2) for k1, k2 in keys if k2 % 2)
    return len(size), [(k1, k2, n, rev[(k1, k2)]) for (k1, k2), n in sorted(size.items()) if (n > S if strict else n >= S)]


def expected(case):
    """the claim -> (sorted key rows, {S: (counters, row columns)})"""
    keys, sn = claimed(case)
    out = {}
    for S in case["S"]:
        distinct, rows = sets_of(keys, S)
        if case.get("rows") is not None:
            assert [tuple(r) for r in case["rows"][S]] == rows, (case["name"], S)       # (the literal rows are the claim; the count agrees)
        out[S] = (counters_of(sn, distinct, len(rows)), row_columns(rows))
    return key_rows(keys), out


def definition(case, ref=None):
    from tiddit_amd import tiddit_snvs
    ref = ref or host_reference()
    keys, sn = [], {}
    for b in batches(case):
        tiddit_snvs.keys_of_batch_by_read(b, keys, sn, ref, case["Q"], case["B"])
    out = {}
    for S in case["S"]:
        c, rows = tiddit_snvs.summarise(keys, sn, S)
        out[S] = (c, row_columns(rows))
    return key_rows(keys), out


def same(a, b):
    return (a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and set(a[1]) == set(b[1]) and
            all(np.array_equal(a[1][S][0], b[1][S][0]) and all(np.array_equal(x, y) for x, y in zip(a[1][S][1], b[1][S][1])) for S in a[1]))


# ------------------------------------------------------------------------------------------- the cases
CASES = []


def case(family, name, claims, batches_, Q=20, B=20, S=(1, 2, 3), capacity=1 << 12, rows=None, clean=False):
    """``clean``: no read of the case is noisy, malformed or off the reference (the anchor of tests/test_snv_refs_cpu.py runs on these)"""
    bs = [(b, 0) if isinstance(b, list) else b for b in batches_]
    CASES.append({"family": family, "name": family + ": " + name, "claims": claims, "batches": bs, "Q": Q, "B": B, "S": S, "capacity": capacity,
                  "rows": rows, "clean": clean})


def _clip(s, cigar):
    return ("%dS" % s if s else "") + cigar


# ---- nibble, word and phase edges
case("phase", "one mismatch at every query offset 0 ... 33, pos even and odd, a leading S of 0 ... 3",
     "the event's P is pos + offset + 1 whatever the parity of the read's and the reference's nibble, and in every word of the compare",
     [[rd(0, 40 + odd, _clip(s, "34M"), mm=(s + k,), flag=REV * ((k + s) & 1)) for odd in (0, 1) for s in range(4) for k in range(34)]], clean=True)
case("phase", "read lengths 1 2 15 16 17 31 32 33 100 151, a mismatch on the first and on the last base",
     "the last, partial word of a read is compared up to its last base and no further",
     [[rd(0, 100 + n % 2, "%dM" % n, mm=sorted({0, n - 1})) for n in (1, 2, 15, 16, 17, 31, 32, 33, 100, 151)] +
      [rd(0, 101, "%dM" % n) for n in (1, 16, 17, 151)]], clean=True)
case("phase", "mismatches on the last base of an operation and on the first base of the next",
     "an operation's last partial step is masked at the operation's end: the next operation's bases are its own",
     [[rd(0, 60 + a, "%dM%d%s%dM" % (a, n, op, b), mm=(a - 1, a + (n if op in "I" else 0)))
       for a in (1, 15, 16, 17) for b in (1, 16, 17) for op, n in (("I", 1), ("D", 1), ("I", 2), ("D", 3))]], clean=True)

# ---- every operation between two M runs
_between = []
for _op in "IDNSHP=X":
    for _n in (1, 2, 15, 16, 17):
        _q_adv = _n if _op in "IS=X" else 0
        for _rev in (0, 1):
            _mm = [9, 10 + _q_adv]                                 # the last base of the first run, the first base of the second
            if _op in "=X":
                _mm.append(10)                                     # ... and the operation's own first base: `=` over a differing base counts
            _between.append(rd(0, 200 + _rev, "10M%d%s11M" % (_n, _op), mm=sorted(_mm), flag=REV * _rev))
_between.append(rd(0, 230, "10M5X11M"))                            # X over matching bases: nothing
case("ops", "I D N S H P = X of 1 2 15 16 17 bases between two M runs",
     "I and S advance the query, D and N the reference, = and X both, H and P neither; = and X are compared like M whatever they claim",
     [_between], clean=True)

# ---- tails
_tails, _short = [], []
for _n in range(1, 18):
    _r = rd(0, 300, "%dM" % _n, mm=(_n - 1,))
    _tails.append([rd(0, 10, "20M"), _r])
    _short.append(([rd(0, 10, "20M"), dict(_r, kind=MALFORMED, events=[], aligned=0, bs_delta=-1)], 0))
    _short.append(([rd(0, 10, "20M"), dict(_r, kind=MALFORMED, events=[], aligned=0)], 1))
case("tails", "a record of l_seq 1 ... 17 without aux bytes ends the batch exactly at raw_len",
     "the last bases and qualities of the batch are read, and nothing behind them", _tails, clean=True)
case("tails", "the same record with block_size one too small, and with raw_len one too small",
     "both are malformed: the bound fails before a base is read", _short)

# ---- contig ends
_ends = []
for _t in (1, 2, 3, 4, 5):
    _L = LENGTHS[_t]
    _ends.append(rd(_t, 0, "%dM" % _L, mm=sorted({0, _L - 1})))
    _ends.append(rd(_t, 0, "%dM" % _L, flag=REV))
    _ends.append(rd(_t, _L - 1, "1M", mm=(0,)))
    _ends.append(rd(_t, 0, "%dM" % (_L + 1), kind=OFF_REFERENCE))
    _ends.append(rd(_t, 1, "%dM" % _L, kind=OFF_REFERENCE))
_ends.append(rd(6, 55, "9M", mm=(8,)))
_ends.append(rd(6, 55, "10M", seq=_LEFT[55:] + TEXT[7][:1], kind=OFF_REFERENCE))         # (the neighbour contig would match)
_ends.append(rd(6, 54, "5M5D1M", kind=OFF_REFERENCE))
_ends.append(rd(7, 0, "16M", mm=(0,)))
_ends.append(rd(UNLOADED, 10, "20M", kind=OFF_REFERENCE))
_ends.append(rd(len(TEXT), 10, "20M", kind=OFF_REFERENCE))                                 # (a contig beyond the reference's table)
case("ends", "reads from base 0, to the last base, one base over the end, on a contig that is not loaded",
     "a read is compared inside its contig or not at all", [_ends])

# ---- codes and qualities
_codes = []
for _g in range(1, 16):
    _events = [(16 * (_g - 1) + _c + 1, CODES[_g], CODES[_c]) for _c in (1, 2, 4, 8) if _g in (1, 2, 4, 8) and _c != _g]
    _codes.append(dict(rd(CODE_CONTIG, 16 * (_g - 1), "16M", seq=CODES), events=_events))
    _codes.append(dict(rd(CODE_CONTIG, 16 * (_g - 1) + 1, "15M", seq=CODES[1:], flag=REV), events=_events))
_codes.append(rd(0, N_RUN[0] - 5, "30M", over={k: "A" for k in range(5, 25)}))    # over the N run: the read's A against N is nothing
_codes.append(rd(0, LOWER[0] + 3, "40M", mm=(0, 7, 39)))           # lower case is the base
_codes.append(rd(0, IUPAC[0] - 4, "28M", over={k: "A" for k in range(4, 24)}))     # A against R Y K M ...: never a mismatch
case("codes", "every pair of the 16 codes on both sides; N, lower case and IUPAC stretches",
     "only A C G T against a different A C G T counts", [_codes], clean=True)
for _B in (20, 0, 93, 1):
    _q = [rd(0, 600 + 2 * k, "20M", mm=(3, 12), qual=q) for k, q in enumerate((_B, _B + 1, 93, 0xff) if _B < 93 else (93, 0xff))]
    if _B:
        _q += [rd(0, 640, "20M", mm=(5,), low=(6, 19), low_qual=_B - 1, qual=max(40, _B)), rd(0, 641, "20M", low=(0,), low_qual=0, flag=REV)]
    else:
        _q += [rd(0, 640, "20M", mm=(5, 6), qual=0)]
    case("quality", "qualities of B - 1, B and 0xff at B = %d" % _B, "a mismatch below B is counted and is no event; 0xff (no quality) is never below",
         [_q], B=_B, clean=True)

# ---- the cap, malformed and skipped records
_eight = tuple(range(2, 34, 4))
_bad_op = ((cigar_word_offset(2, 1), "<I", 9),)                 # (the second operation, of length 0, becomes op code 9)
case("cap", "exactly 8 and 9 events; 8 events plus low-quality mismatches; 9 events in front of a bad op code",
     "more than 8 keyed events make a read noisy; low-quality mismatches are not keyed events; a bad op code makes the record malformed, not noisy",
     [[rd(0, 700, "40M", mm=_eight), rd(0, 700, "40M", mm=_eight + (35,), kind=NOISY), rd(0, 701, "40M", mm=_eight, low=(0, 1, 39), low_qual=5, flag=REV),
       rd(0, 702, "40M", mm=_eight[:7], low=(0, 39), low_qual=19), rd(0, 703, "40M", mm=tuple(range(0, 40, 2)), low=(1,), kind=NOISY),
       dict(rd(0, 700, "40M0M", mm=_eight + (35,), patch=_bad_op), kind=MALFORMED, events=[], aligned=0)]])
case("skipped", "l_seq against the CIGAR, no sequence, no CIGAR, bad positions",
     "malformed records and records without sequence give one counter each and nothing else",
     [[dict(rd(0, 800, "10M", seq="ACGTACGTACGT"), kind=MALFORMED, aligned=0), dict(rd(0, 800, "10M", seq="ACGTACGTA"), kind=MALFORMED, aligned=0),
       dict(rd(0, 800, "10M", seq=""), kind=NO_SEQUENCE, aligned=0), dict(rd(0, 800, "", seq="ACGTACGTAC"), kind=NO_SEQUENCE, aligned=0),
       dict(rd(0, 800, "", seq=""), kind=NO_SEQUENCE, aligned=0),
       dict(rd(0, 2 ** 31 - 10, "20M", seq="A" * 20), kind=MALFORMED, aligned=0), dict(rd(0, 2 ** 31 - 21, "20M", seq="A" * 20), kind=OFF_REFERENCE, aligned=0),
       dict(rd(0, 10, "5M" + "1N" * 8 + "5M", seq="A" * 10, patch=[(cigar_word_offset(2, j), "<I", (268435455 << 4) | 3) for j in range(1, 9)]), kind=MALFORMED, aligned=0),
       dict(rd(1 << 24, 10, "20M"), kind=MALFORMED, aligned=0), dict(rd(0, -1, "20M", seq="A" * 20), kind=MALFORMED, aligned=0),
       dict(rd(0, 800, "10M", seq="", patch=((cigar_word_offset(3, 0), "<I", (10 << 4) | 15),)), kind=MALFORMED, aligned=0),
       dict(rd(0, 800, "20M", patch=((20, "<i", -20),)), kind=MALFORMED, aligned=0),
       rd(0, 800, "20M", mm=(4,))]])
case("filters", "every bit of the flag, tid -1, mapq Q - 1 and Q", "0x4 0x100 0x200 0x400 0x800, no contig and a low MAPQ drop a record before its bytes are read",
     [[rd(0, 820, "20M", mm=(2,), flag=f, kind=NOT_ELIGIBLE if f & 0xF04 else OK) for f in [1 << k for k in range(12)] + [0xF04, 0x0FB]] +
      [rd(-1, 820, "20M", kind=NOT_ELIGIBLE), rd(0, 820, "20M", mm=(2,), mapq=29, kind=NOT_ELIGIBLE), rd(0, 820, "20M", mm=(2,), mapq=30),
       dict(rd(0, 820, "20M", mapq=0, bs_delta=-30), kind=NOT_ELIGIBLE)]], Q=30, clean=True)

# ---- workgroups and the store
for _n in (SNV_BLOCK - 1, SNV_BLOCK, SNV_BLOCK + 1, 2 * SNV_BLOCK - 1, 2 * SNV_BLOCK, 2 * SNV_BLOCK + 1):
    case("workgroups", "%d reads, one mismatch each" % _n, "the last workgroup takes what is left",
         [[rd(0, 850 + k % 50, "20M", mm=(k % 20,), flag=REV * (k % 3 == 0), mapq=60 if k % 7 else 0, kind=OK if k % 7 else NOT_ELIGIBLE) for k in range(_n)]], Q=1,
         clean=True)
case("workgroups", "every read of two tiles carries 8 events", "the staging is full: 8 keys per read of the tile",
     [[rd(0, 900 + k % 30, "40M", mm=_eight, flag=REV * (k & 1)) for k in range(2 * SNV_BLOCK)]], S=(1, 3), capacity=8 * 2 * SNV_BLOCK, clean=True)
case("workgroups", "eligible reads only in the last lane of each tile", "the compaction hands the one read to lane 0",
     [[rd(0, 950, "20M", mm=(1, 18), mapq=60 if k % SNV_BLOCK == SNV_BLOCK - 1 else 3, kind=OK if k % SNV_BLOCK == SNV_BLOCK - 1 else NOT_ELIGIBLE)
       for k in range(2 * SNV_BLOCK + 1)]], clean=True)
case("store", "a store made for 64 keys, five pushes", "the store grows more than once and keeps what it held",
     [[rd(0, 960 + k % 20, "30M", mm=(k % 30, (k + 7) % 30), flag=REV * (k & 1)) for k in range(40)] for _ in range(5)], capacity=64, clean=True)

# ---- sets
_p = 1001
_ref = _MAIN[_p - 1]
_a1, _a2 = sorted((other(_ref), other(other(_ref))), key="ACGT".index)
_site = ([rd(0, _p - 1 - k, "20M", mm=(k,), alt=_a1, flag=REV * (k & 1)) for k in range(5)] + [rd(0, _p - 1 - k, "20M", mm=(k,), alt=_a2, flag=REV * (k < 2)) for k in range(3)] +
         [rd(0, _p + 9 - k, "20M", mm=(k,), flag=0) for k in range(2)] + [rd(0, _p + 19, "20M", mm=(0,), flag=REV)])
case("sets", "one site with two alternative bases on both strands; supports of 1, 2, 3 and 5",
     "equal (K1, K2 >> 1) are one event whatever the strand; SUPPORT >= S is reported, S - 1 is not",
     [_site[:4], _site[4:9], _site[9:]], S=(1, 2, 3, 4),
     rows={1: [(K1(0, _p), K2(_ref, _a1), 5, 2), (K1(0, _p), K2(_ref, _a2), 3, 2), (K1(0, _p + 10), K2(_MAIN[_p + 9], other(_MAIN[_p + 9])), 2, 0),
               (K1(0, _p + 20), K2(_MAIN[_p + 19], other(_MAIN[_p + 19])), 1, 1)],
           2: [(K1(0, _p), K2(_ref, _a1), 5, 2), (K1(0, _p), K2(_ref, _a2), 3, 2), (K1(0, _p + 10), K2(_MAIN[_p + 9], other(_MAIN[_p + 9])), 2, 0)],
           3: [(K1(0, _p), K2(_ref, _a1), 5, 2), (K1(0, _p), K2(_ref, _a2), 3, 2)], 4: [(K1(0, _p), K2(_ref, _a1), 5, 2)]}, clean=True)
_runs = []
for _j, _n in enumerate((KS_TILE - 1, KS_TILE, KS_TILE + 1)):
    _runs += [rd(0, 1100 + 7 * _j - k % 5, "12M", mm=(k % 5,), flag=REV * (k % 3 == 1)) for k in range(_n)]
case("sets", "runs of 4095, 4096 and 4097 equal keys", "a run that crosses the run-length tile is one run, its REV counted across the seam",
     [_runs[:5000], _runs[5000:]], S=(1, KS_TILE, KS_TILE + 1), capacity=1 << 14, clean=True)

N_CASES = len(CASES)
FAMILIES = ("phase", "ops", "tails", "ends", "codes", "quality", "cap", "skipped", "filters", "workgroups", "store", "sets")
