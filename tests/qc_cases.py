"""Aimed cases for the read-level QC tables (tiddit_amd/tiddit_qc.py, csrc/tdt_qc.hip), each with the counters it claims, and a second,
independent reference: a numpy restatement that works on whole columns for the field sections and on expanded per-base arrays (one
entry per base: nibble, column, cycle, quality) for the byte sections.  The definition (``tiddit_qc.count_read``) walks base by base;
the two share no code.

A case is a dict: ``reads`` (see :func:`R`), ``cuts`` (where the reads are cut into batches), and its claim — ``expect`` = {key: count}
naming EVERY non-zero counter, keys ``("SN", name)``, ``("MAPQ", q)``, ``("RL", l)``, ``("IS", tlen, column)``, ``("CYC", cycle, column)``,
``("QUAL", q)``, ``("GCR", percent)``, ``("ID", length, "ins" | "del")`` — written down from the case's own strings and arithmetic, never
computed by either reference.  The helpers :func:`plain`, :func:`spell`, :func:`mono` and :func:`marked` spell a claim out from letters.

``QC_CYCLES``, ``QC_IS_MAX``, ``QC_ID_MAX`` and the two tile sizes are read from the `#define` lines of csrc/tdt_qc.hip, so the cases stay
on their edges when a constant is retuned.

``reader_ok``: the case's records can also travel through a BAM file and the device reader.  The malformed records cannot: the reader's
own record check may refuse them before any consumer sees the batch, so those go through ``tdt_qc_push`` only.  Every malformed case
states which counters the record still adds to: the field sections (SN up to mapq0, MAPQ, RL, IS), and ``malformed``.

Mutants of the restatement (``reference(case, mutant=...)``), each caught inside the family named beside it:
  ``nib``     the two nibbles of a byte swapped            -> nibbles
  ``norev``   the cycle of a reverse read not reversed     -> length
  ``nocomp``  no complement on a reverse read              -> nibbles
  ``tlen0``   tlen >= 0 counts as an insert size           -> insert
  ``ff``      a first quality byte 0xff counted as a value -> qualities
  ``d``       D counted as aligned query bases             -> cigar
"""
import os
import re
import struct

import numpy as np

from tiddit_amd import bamio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(REPO, "tiddit_amd", "csrc", "tdt_qc.hip")).read()


def _define(name):
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+([0-9]+)[ \t]*(?://[^\n]*)?$" % name, _SRC, re.M)
    if not m:
        raise KeyError("cannot parse #define %s" % name)
    return int(m.group(1))


CY, IM, IDM, BT, FT = (_define(k) for k in ("QC_CYCLES", "QC_IS_MAX", "QC_ID_MAX", "QC_B_TILE", "QC_F_TILE"))
SN = ("records", "secondary", "supplementary", "primary", "qc_fail", "duplicate", "unmapped", "mapped", "paired", "read1", "read2", "proper_pair",
      "mate_unmapped", "both_mapped", "mate_other_contig", "mate_other_contig_mapq5", "reverse", "mapq0", "malformed", "bases", "reads_no_seq",
      "reads_no_qual", "bases_q20", "bases_q30", "aligned_bases", "soft_clipped_bases", "hard_clipped_bases", "inserted_bases", "deleted_bases",
      "skipped_bases", "insertions", "deletions", "reads_clipped")
# the sections in the order of the counter array: name -> (offset, rows, columns)
SECTIONS, _o = {}, 0
for _name, _rows, _cols in (("SN", len(SN), 1), ("MAPQ", 256, 1), ("RL", CY + 1, 1), ("IS", IM + 1, 3), ("CYC", CY + 1, 7), ("QUAL", 256, 1), ("GCR", 101, 1),
                            ("ID", IDM, 2)):
    SECTIONS[_name] = (_o, _rows, _cols)
    _o += _rows * _cols
SIZE = _o
IS_COL = {"inward": 0, "outward": 1, "same": 2}
CYC_COL = {"A": 0, "C": 1, "G": 2, "T": 3, "o": 4, "qual_sum": 5, "qual_n": 6}
CODES = "=ACMGRSVTWYHKDBN"                  # the 16 sequence codes of the BAM format, by nibble value
MUTANTS = {"nib": "nibbles", "norev": "length", "nocomp": "nibbles", "tlen0": "insert", "ff": "qualities", "d": "cigar"}
PAD = 64 << 10
PAD_BYTE = 0x44                              # as a sequence byte: G G; as a quality: 68
L_NAME = 9                                   # "r%07d" and its NUL
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def index(key):
    """the counter a claim's key names"""
    o, rows, cols = SECTIONS[key[0]]
    if key[0] == "SN":
        return o + SN.index(key[1])
    if key[0] == "IS":
        return o + 3 * key[1] + IS_COL[key[2]]
    if key[0] == "CYC":
        return o + 7 * key[1] + CYC_COL[key[2]]
    if key[0] == "ID":
        return o + 2 * (key[1] - 1) + {"ins": 0, "del": 1}[key[2]]
    assert 0 <= key[1] < rows, key
    return o + key[1]


def R(seq=None, qual=None, cigar=None, flag=0, mapq=60, tid=0, pos=100, mate_tid=-1, mate_pos=-1, tlen=0, patch=(), pad=0):
    """one read.  seq: string over CODES (default: A for every query base of the CIGAR); qual: one value for every base, a list, or None
    (absent: 0xff); cigar: string, [(op, len)] or None (no operations); patch: ((byte offset in the record, struct format, value), ...)
    applied to the encoded record; pad: bytes of PAD_BYTE behind the record in the push entry's buffer"""
    cig = [] if cigar is None else bamio.parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    if seq is None:
        seq = "A" * sum(l for op, l in cig if op in (0, 1, 4, 7, 8))
    if isinstance(qual, int):
        qual = [qual] * len(seq)
    return {"seq": seq, "qual": qual, "cigar": cig, "flag": flag, "mapq": mapq, "tid": tid, "pos": pos, "mate_tid": mate_tid, "mate_pos": mate_pos,
            "tlen": tlen, "patch": tuple(patch), "pad": pad}


def seq_offset(n_cigar):
    """the byte offset of the first sequence byte in an encoded record"""
    return 4 + 32 + L_NAME + 4 * n_cigar


def _record(i, r):
    rec = bytearray(bamio.encode_record("r%07d" % i, r["flag"], r["tid"], r["pos"], r["mapq"], r["cigar"], r["mate_tid"], r["mate_pos"], r["tlen"],
                                        seq=r["seq"], qual=None if r["qual"] is None else bytes(r["qual"])))
    for off, fmt, val in r["patch"]:
        struct.pack_into(fmt, rec, off, val)
    return bytes(rec)


class Batch:
    """the columns of a run of reads over one raw buffer — what tdt_qc_push and the definition take"""
    COLUMNS = ("flag", "mapq", "tid", "mate_tid", "tlen", "l_seq", "rec_off")

    def __init__(self, raw, **cols):
        self.raw = raw
        for k in self.COLUMNS:
            setattr(self, k, cols[k])

    def __len__(self):
        return len(self.tid)

    def cut(self, lo, hi):
        return Batch(self.raw, **{k: getattr(self, k)[lo:hi] for k in self.COLUMNS})


def build(case, padding=True):
    """-> the whole case as one Batch (padding=False: the records back to back, as a BAM file holds them)"""
    if ("built", padding) in case:
        return case[("built", padding)]
    reads = case["reads"]
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
    b = Batch(np.frombuffer(b"".join(parts), dtype=np.uint8), flag=col("flag", np.uint16), mapq=col("mapq", np.uint8), tid=col("tid", np.int32),
              mate_tid=col("mate_tid", np.int32), tlen=col("tlen", np.int32), l_seq=np.array([len(r["seq"]) for r in reads], dtype=np.int32),
              rec_off=np.array(offs, dtype=np.uint64))
    if case.get("truncate_last"):
        b.raw = b.raw[:offs[-1] + 40]
    case[("built", padding)] = b
    return b


def batches(case, padding=True):
    b = build(case, padding)
    cuts = [0] + list(case["cuts"]) + [len(b)]
    return [b.cut(lo, hi) for lo, hi in zip(cuts, cuts[1:]) if hi > lo]


def expected(case):
    """the claim as uint64[SIZE]"""
    c = np.zeros(SIZE, dtype=np.uint64)
    for key, v in case["expect"].items():
        assert v > 0, (case["name"], key)
        c[index(key)] = v
    return c


# ------------------------------------------------------------------------------------------- the numpy restatement
_COL_OF_NIBBLE = np.full(16, 4, dtype=np.int64)
_COL_OF_NIBBLE[[1, 2, 4, 8]] = [0, 1, 2, 3]
_COMPLEMENT = np.array([3, 2, 1, 0, 4], dtype=np.int64)


def _u(raw, o, dt):
    return int(np.frombuffer(raw[o:o + np.dtype(dt).itemsize].tobytes(), dtype=dt)[0])


def reference_batch(c, b, mutant=None):
    """adds one batch to ``c`` (int64[SIZE])"""
    O = {k: v[0] for k, v in SECTIONS.items()}
    f, q = b.flag.astype(np.int64), b.mapq.astype(np.int64)
    tid, mtid, tlen, lseq = (getattr(b, k).astype(np.int64) for k in ("tid", "mate_tid", "tlen", "l_seq"))
    bit = lambda m: (f & m) != 0
    prim = ~bit(0x900)
    mapped, paired = prim & ~bit(0x4), prim & bit(0x1)
    both = paired & ~bit(0x4) & ~bit(0x8)
    other = both & (mtid != tid)
    for name, m in (("records", np.ones(len(f), dtype=bool)), ("secondary", bit(0x100)), ("supplementary", bit(0x800)), ("primary", prim),
                    ("qc_fail", prim & bit(0x200)), ("duplicate", prim & bit(0x400)), ("unmapped", prim & bit(0x4)), ("mapped", mapped), ("paired", paired),
                    ("read1", prim & bit(0x40)), ("read2", prim & bit(0x80)), ("proper_pair", paired & bit(0x2)), ("mate_unmapped", paired & bit(0x8)),
                    ("both_mapped", both), ("mate_other_contig", other), ("mate_other_contig_mapq5", other & (q >= 5)), ("reverse", mapped & bit(0x10)),
                    ("mapq0", mapped & (q == 0))):
        c[SN.index(name)] += int(m.sum())
    c[O["MAPQ"]:O["MAPQ"] + 256] += np.bincount(q[mapped], minlength=256)
    S = ~bit(0xB00)
    c[O["RL"]:O["RL"] + CY + 1] += np.bincount(np.clip(lseq[S], 0, CY), minlength=CY + 1)
    pair = S & bit(0x1) & ~bit(0x4) & ~bit(0x8) & (mtid == tid) & ((tlen >= 0) if mutant == "tlen0" else (tlen > 0))
    orient = np.where(~bit(0x10) & bit(0x20), 0, np.where(bit(0x10) & ~bit(0x20), 1, 2))
    np.add.at(c, O["IS"] + 3 * np.minimum(tlen[pair], IM) + orient[pair], 1)
    raw = np.asarray(b.raw, dtype=np.uint8)
    sn = lambda name, v: c.__setitem__(SN.index(name), c[SN.index(name)] + int(v))
    for i in np.flatnonzero(S):
        ro = int(b.rec_off[i])
        if ro + 36 > len(raw):
            sn("malformed", 1)
            continue
        bs, l_name, n_cig, L = _u(raw, ro, "<u4"), int(raw[ro + 12]), _u(raw, ro + 16, "<u2"), _u(raw, ro + 20, "<i4")
        if L < 0 or 32 + l_name + 4 * n_cig + (L + 1) // 2 + L > bs or ro + 4 + bs > len(raw):
            sn("malformed", 1)
            continue
        c0 = ro + 36 + l_name
        words = np.frombuffer(raw[c0:c0 + 4 * n_cig].tobytes(), dtype="<u4").astype(np.int64)
        code, ln = words & 0xf, words >> 4
        if (code > 8).any():
            sn("malformed", 1)
            continue
        s0 = c0 + 4 * n_cig
        seq = raw[s0:s0 + (L + 1) // 2].astype(np.int64)
        qual = raw[s0 + (L + 1) // 2:s0 + (L + 1) // 2 + L].astype(np.int64)
        hi_nib, lo_nib = seq >> 4, seq & 0xf
        if mutant == "nib":
            hi_nib, lo_nib = lo_nib, hi_nib
        nib = np.stack([hi_nib, lo_nib], axis=1).reshape(-1)[:L]         # one entry per base
        rev = bool(f[i] & 0x10)
        col = _COL_OF_NIBBLE[nib]
        cyc = np.arange(L, dtype=np.int64)
        if rev:
            if mutant != "nocomp":
                col = _COMPLEMENT[col]
            if mutant != "norev":
                cyc = cyc[::-1]
        row = O["CYC"] + 7 * np.minimum(cyc, CY)
        np.add.at(c, row + col, 1)
        sn("bases", L)
        sn("reads_no_seq", L == 0)
        has_q = L > 0 and (mutant == "ff" or qual[0] != 0xff)
        sn("reads_no_qual", L > 0 and not has_q)
        if has_q:
            np.add.at(c, row + 5, qual)
            np.add.at(c, row + 6, 1)
            c[O["QUAL"]:O["QUAL"] + 256] += np.bincount(qual, minlength=256)
            sn("bases_q20", (qual >= 20).sum())
            sn("bases_q30", (qual >= 30).sum())
        if L > 0:
            c[O["GCR"] + (100 * int(np.isin(nib, [2, 4]).sum())) // L] += 1
        if not f[i] & 0x4 and n_cig:
            for name, ops in (("aligned_bases", [0, 7, 8, 2] if mutant == "d" else [0, 7, 8]), ("soft_clipped_bases", [4]), ("hard_clipped_bases", [5]),
                              ("inserted_bases", [1]), ("deleted_bases", [2]), ("skipped_bases", [3])):
                sn(name, ln[np.isin(code, ops)].sum())
            for k, (name, op) in enumerate((("insertions", 1), ("deletions", 2))):
                ev = ln[(code == op) & (ln >= 1)]
                sn(name, len(ev))
                np.add.at(c, O["ID"] + 2 * (np.minimum(ev, IDM) - 1) + k, 1)
            sn("reads_clipped", np.isin(code, [4, 5]).any())


def reference(case, mutant=None, padding=True):
    """-> uint64[SIZE] of the whole case"""
    c = np.zeros(SIZE, dtype=np.int64)
    for b in batches(case, padding):
        reference_batch(c, b, mutant)
    return c.astype(np.uint64)


def definition(case, padding=True):
    from tiddit_amd import tiddit_qc
    c = [0] * SIZE
    for b in batches(case, padding):
        tiddit_qc.count_batch(c, b)
    return np.array(c, dtype=np.uint64)


# ------------------------------------------------------------------------------------------- how a claim is spelled
def merge(*parts):
    out = {}
    for p in parts:
        for k, v in p.items():
            if v:
                out[k] = out.get(k, 0) + v
    return out


def sn(**counts):
    return {("SN", k): v for k, v in counts.items()}


def plain(n=1, mapq=60):
    """the field counters of n mapped, unpaired, forward primary reads"""
    return merge(sn(records=n, primary=n, mapped=n), {("MAPQ", mapq): n})


def spell(text, quals=None, n=1):
    """the CYC counters of n reads whose cycles 0, 1, ... hold the columns ``text`` (A C G T, o = other) with the qualities ``quals``
    (in cycle order; None: the read has none): what the read looks like in READ orientation, written by hand for a reverse read"""
    out = {}
    for c, ch in enumerate(text):
        out = merge(out, {("CYC", min(c, CY), ch): n})
        if quals is not None:
            out = merge(out, {("CYC", min(c, CY), "qual_sum"): n * quals[c], ("CYC", min(c, CY), "qual_n"): n})
    return out


def mono(L, letter, q=None, n=1, rev=False):
    """the byte counters (and RL) of n reads of L times the stored base ``letter`` with the one quality q (None: absent)"""
    col = {"A": "T", "C": "G", "G": "C", "T": "A"}[letter] if rev else letter
    e = merge(sn(bases=n * L), {("RL", min(L, CY)): n})
    if L == 0:
        return merge(e, sn(reads_no_seq=n))
    e = merge(e, {("GCR", 100 if letter in "CG" else 0): n}, {("CYC", c, col): n for c in range(min(L, CY))}, {("CYC", CY, col): n * (L - CY) if L > CY else 0})
    if q is None:
        return merge(e, sn(reads_no_qual=n))
    e = merge(e, {("QUAL", q): n * L}, sn(bases_q20=n * L if q >= 20 else 0, bases_q30=n * L if q >= 30 else 0),
              {("CYC", c, "qual_sum"): n * q for c in range(min(L, CY))}, {("CYC", c, "qual_n"): n for c in range(min(L, CY))})
    if L > CY:
        e = merge(e, {("CYC", CY, "qual_sum"): n * q * (L - CY), ("CYC", CY, "qual_n"): n * (L - CY)})
    return e


MARK_Q, REST_Q = 10, 30


def marked_read(L, rev, **kw):
    """a read that looks different from its two ends: stored C then A ..., stored qualities 10 then 30 ..."""
    return R("C" + "A" * (L - 1), qual=[MARK_Q] + [REST_Q] * (L - 1), flag=0x10 if rev else 0, **kw)


def marked(L, rev):
    """the byte counters (and RL) of marked_read(L, rev), L >= 1: forward, cycle 0 is the C with quality 10 and every other cycle an A with
    30; reverse, cycle L - 1 is a G with 10 and every other cycle a T with 30"""
    mark_cycle, mark, rest = (L - 1, "G", "T") if rev else (0, "C", "A")
    e = merge(sn(bases=L, bases_q20=L - 1, bases_q30=L - 1), {("RL", min(L, CY)): 1, ("GCR", 100 // L): 1, ("QUAL", MARK_Q): 1, ("QUAL", REST_Q): L - 1})
    head = min(L, CY)
    in_head = mark_cycle < CY
    e = merge(e, {("CYC", c, rest): 1 for c in range(head) if c != mark_cycle}, {("CYC", c, "qual_sum"): REST_Q for c in range(head) if c != mark_cycle},
              {("CYC", c, "qual_n"): 1 for c in range(head)})
    if in_head:
        e = merge(e, {("CYC", mark_cycle, mark): 1, ("CYC", mark_cycle, "qual_sum"): MARK_Q})
    if L > CY:
        tail = L - CY                                                 # the cycles CY ... L - 1 share the last row
        tail_rest = tail - (0 if in_head else 1)
        e = merge(e, {("CYC", CY, rest): tail_rest, ("CYC", CY, "qual_n"): tail, ("CYC", CY, "qual_sum"): REST_Q * tail_rest + (0 if in_head else MARK_Q)},
                  {} if in_head else {("CYC", CY, mark): 1})
    return e


# ------------------------------------------------------------------------------------------- the cases
CASES = []


def case(name, family, reads, expect, cuts=(), reader_ok=True):
    CASES.append({"name": name, "family": family, "reads": reads, "expect": expect, "cuts": tuple(cuts), "reader_ok": reader_ok,
                  "lengths": [100000, 100000, 100000]})


# ---- read length: every length as a forward and as a reverse read that looks different from its two ends
case("length 0 forward and reverse", "length", [R(""), R("", flag=0x10)],
     merge(plain(2), sn(reverse=1, reads_no_seq=2), {("RL", 0): 2}), cuts=(1,))
case("length 1 forward and reverse", "length", [R("C", qual=[10]), R("C", qual=[10], flag=0x10)],
     merge(plain(2), sn(reverse=1, bases=2), {("RL", 1): 2, ("GCR", 100): 2, ("QUAL", 10): 2, ("CYC", 0, "C"): 1, ("CYC", 0, "G"): 1,
                                              ("CYC", 0, "qual_sum"): 20, ("CYC", 0, "qual_n"): 2}))
case("length 2 forward and reverse", "length", [R("CA", qual=[10, 30]), R("CA", qual=[10, 30], flag=0x10)],
     merge(plain(2), sn(reverse=1, bases=4, bases_q20=2, bases_q30=2), {("RL", 2): 2, ("GCR", 50): 2, ("QUAL", 10): 2, ("QUAL", 30): 2},
           spell("CA", [10, 30]), spell("TG", [30, 10])))
case("length 3 forward and reverse", "length", [R("CAA", qual=[10, 30, 30]), R("CAA", qual=[10, 30, 30], flag=0x10)],
     merge(plain(2), sn(reverse=1, bases=6, bases_q20=4, bases_q30=4), {("RL", 3): 2, ("GCR", 33): 2, ("QUAL", 10): 2, ("QUAL", 30): 4},
           spell("CAA", [10, 30, 30]), spell("TTG", [30, 30, 10])))
for _L in (63, 64, 65, 127, 128, 129, CY - 1, CY, CY + 1, 2 * CY + 1, 20001):
    case("length %d forward and reverse" % _L, "length", [marked_read(_L, False), marked_read(_L, True)],
         merge(plain(2), sn(reverse=1), marked(_L, False), marked(_L, True)), cuts=(1,) if _L in (64, CY) else ())

# ---- nibbles: each of the 16 codes in the high and in the low nibble of a byte, forward and reverse; a pad nibble that is not zero
case("nibbles every code in both nibbles", "nibbles", [R(CODES), R(CODES, flag=0x10), R("A" + CODES), R("A" + CODES, flag=0x10)],
     merge(plain(4), sn(reverse=2, bases=66, reads_no_qual=4), {("RL", 16): 2, ("RL", 17): 2, ("GCR", 12): 2, ("GCR", 11): 2},
           spell("oACoGoooTooooooo"),          # = A C M G R S V T W Y H K D B N
           spell("oooooooAoooCoGTo"),          # ... read from its other end, complemented
           spell("AoACoGoooTooooooo"), spell("oooooooAoooCoGToT")), cuts=(2,))
case("nibbles a pad nibble that is not zero", "nibbles",
     [R("ACG", patch=((seq_offset(0) + 1, "<B", 0x48),)), R("ACG", flag=0x10, patch=((seq_offset(0) + 1, "<B", 0x48),))],      # G and a T nobody asked for
     merge(plain(2), sn(reverse=1, bases=6, reads_no_qual=2), {("RL", 3): 2, ("GCR", 66): 2}, spell("ACG"), spell("CGT")))

# ---- qualities
case("qualities around 20 and 30 and the largest", "qualities", [R("ACGTACGT", qual=[0, 19, 20, 29, 30, 93, 94, 254])],
     merge(plain(1), sn(bases=8, bases_q20=6, bases_q30=4), {("RL", 8): 1, ("GCR", 50): 1}, {("QUAL", q): 1 for q in (0, 19, 20, 29, 30, 93, 94, 254)},
           spell("ACGTACGT", [0, 19, 20, 29, 30, 93, 94, 254])))
case("qualities 0xff first means absent", "qualities", [R("ACGT", qual=[0xff, 30, 30, 30]), R("ACGT", qual=None)],
     merge(plain(2), sn(bases=8, reads_no_qual=2), {("RL", 4): 2, ("GCR", 50): 2}, spell("ACGT", n=2)), cuts=(1,))
case("qualities 0xff only later is the value 255", "qualities", [R("ACGT", qual=[30, 0xff, 0xff, 7])],
     merge(plain(1), sn(bases=4, bases_q20=3, bases_q30=3), {("RL", 4): 1, ("GCR", 50): 1, ("QUAL", 30): 1, ("QUAL", 255): 2, ("QUAL", 7): 1},
           spell("ACGT", [30, 255, 255, 7])))
case("qualities of a reverse read follow its cycles", "qualities", [R("ACGT", qual=[1, 2, 3, 40], flag=0x10)],
     merge(plain(1), sn(reverse=1, bases=4, bases_q20=1, bases_q30=1), {("RL", 4): 1, ("GCR", 50): 1, ("QUAL", 1): 1, ("QUAL", 2): 1, ("QUAL", 3): 1, ("QUAL", 40): 1},
           spell("ACGT", [40, 3, 2, 1])))

# ---- GC per read: for every length, reads with g of their bases C or G; the bins written down per length
_GCR = {1: [0, 100], 2: [0, 50, 100], 3: [0, 33, 66, 100], 4: [0, 25, 50, 75, 100], 5: [0, 20, 40, 60, 80, 100], 6: [0, 16, 33, 50, 66, 83, 100],
        7: [0, 14, 28, 42, 57, 71, 85, 100], 8: [0, 12, 25, 37, 50, 62, 75, 87, 100]}
_GC_PICK = {100: {0: 0, 1: 1, 49: 49, 50: 50, 99: 99, 100: 100}, 150: {0: 0, 1: 0, 2: 1, 3: 2, 74: 49, 75: 50, 76: 50, 149: 99, 150: 100}}
for _L in list(range(1, 9)) + [100, 150]:
    _bins = dict(enumerate(_GCR[_L])) if _L in _GCR else _GC_PICK[_L]
    _seqs = [("CG" * _g)[:_g] + "A" * (_L - _g) for _g in _bins]
    case("gcr length %d" % _L, "gcr", [R(s) for s in _seqs],
         merge(plain(len(_seqs)), sn(bases=_L * len(_seqs), reads_no_qual=len(_seqs)), {("RL", _L): len(_seqs)}, *[{("GCR", b): 1} for b in _bins.values()],
               *[spell(s) for s in _seqs]), cuts=(1,) if _L == 3 else ())

# ---- flags: reads without bases (they add RL 0 and reads_no_seq when they are in S), tid 0
_BITS = (0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800)
case("flags each bit alone", "flags", [R("", flag=b, mate_tid=0) for b in _BITS],
     merge(sn(records=12, secondary=1, supplementary=1, primary=10, qc_fail=1, duplicate=1, unmapped=1, mapped=9, paired=1, read1=1, read2=1, both_mapped=1,
              reverse=1, reads_no_seq=9), {("MAPQ", 60): 9, ("RL", 0): 9}), cuts=(5,))
case("flags the combinations the rules branch on", "flags",
     [R("", flag=0x3, mate_tid=0),                         # a  proper pair
      R("", flag=0x9, mate_tid=0),                         # b  mate unmapped
      R("", flag=0x5, mate_tid=0),                         # c  unmapped itself
      R("", flag=0x1, mate_tid=1, mapq=5),                 # d  mate on another contig, mapq 5
      R("", flag=0x1, mate_tid=1, mapq=4),                 # e  ... mapq 4
      R("", flag=0x1, mate_tid=-1, mapq=255),              # f  ... mate_tid -1 is another contig too
      R("", flag=0x1, mate_tid=0, mapq=0),                 # g  mapq 0
      R("", flag=0x103, mate_tid=0),                       # h  secondary: nothing of the primary rows
      R("", flag=0x900, mate_tid=0),                       # i  secondary and supplementary
      R("", flag=0x14, mate_tid=0),                        # j  unmapped and reverse: not `reverse`
      R("", flag=0x4, mate_tid=0, mapq=0),                 # k  unmapped with mapq 0: not `mapq0`
      R("", flag=0x203, mate_tid=0)],                      # l  QC fail: primary rows, not S
     merge(sn(records=12, secondary=2, supplementary=1, primary=10, qc_fail=1, unmapped=3, mapped=7, paired=8, proper_pair=2, mate_unmapped=1, both_mapped=6,
              mate_other_contig=3, mate_other_contig_mapq5=2, mapq0=1, reads_no_seq=9),
           {("MAPQ", 60): 3, ("MAPQ", 5): 1, ("MAPQ", 4): 1, ("MAPQ", 255): 1, ("MAPQ", 0): 1, ("RL", 0): 9}), cuts=(3, 7))

# ---- insert sizes: every tlen in the four flag patterns of the three orientations (0x21 inward, 0x11 outward, 0x01 and 0x31 same)
_TLENS = (0, 1, IM - 1, IM, IM + 1, -1, INT32_MAX, INT32_MIN)
case("insert every tlen in every orientation", "insert", [R("", flag=f, mate_tid=0, tlen=t) for t in _TLENS for f in (0x21, 0x11, 0x01, 0x31)],
     merge(sn(records=32, primary=32, mapped=32, paired=32, both_mapped=32, reverse=16, reads_no_seq=32), {("MAPQ", 60): 32, ("RL", 0): 32},
           {("IS", 1, "inward"): 1, ("IS", 1, "outward"): 1, ("IS", 1, "same"): 2},
           {("IS", IM - 1, "inward"): 1, ("IS", IM - 1, "outward"): 1, ("IS", IM - 1, "same"): 2},
           {("IS", IM, "inward"): 3, ("IS", IM, "outward"): 3, ("IS", IM, "same"): 6}), cuts=(13,))      # (IM, IM + 1 and INT32_MAX share the last row)
case("insert who is counted", "insert",
     [R("", flag=0x0, mate_tid=0, tlen=100),               # unpaired
      R("", flag=0x9, mate_tid=0, tlen=100),               # mate unmapped
      R("", flag=0x5, mate_tid=0, tlen=100),               # unmapped itself
      R("", flag=0x1, mate_tid=1, tlen=100),               # mate on another contig
      R("", flag=0x101, mate_tid=0, tlen=100),             # secondary
      R("", flag=0x201, mate_tid=0, tlen=100),             # QC fail
      R("", flag=0x401, mate_tid=0, tlen=100),             # duplicate: in S, counted
      R("", flag=0x801, mate_tid=0, tlen=100)],            # supplementary
     merge(sn(records=8, secondary=1, supplementary=1, primary=6, qc_fail=1, duplicate=1, unmapped=1, mapped=5, paired=5, mate_unmapped=1, both_mapped=3,
              mate_other_contig=1, mate_other_contig_mapq5=1, reads_no_seq=5), {("MAPQ", 60): 5, ("RL", 0): 5, ("IS", 100, "same"): 1}))

# ---- CIGAR
case("cigar every op alone", "cigar", [R(cigar="5" + op) for op in "MIDNSHP=X"],
     merge(plain(9), sn(bases=25, reads_no_seq=4, reads_no_qual=5, aligned_bases=15, inserted_bases=5, deleted_bases=5, skipped_bases=5, soft_clipped_bases=5,
                        hard_clipped_bases=5, insertions=1, deletions=1, reads_clipped=2),
           {("RL", 5): 5, ("RL", 0): 4, ("GCR", 0): 5, ("ID", 5, "ins"): 1, ("ID", 5, "del"): 1}, spell("AAAAA", n=5)), cuts=(4,))
case("cigar ops in pairs", "cigar", [R(cigar=c) for c in ("2H3S", "3M2D", "2I3M", "3M4N", "3=2X", "2M3P")],
     merge(plain(6), sn(bases=21, reads_no_qual=6, aligned_bases=16, hard_clipped_bases=2, soft_clipped_bases=3, deleted_bases=2, inserted_bases=2,
                        skipped_bases=4, insertions=1, deletions=1, reads_clipped=1),
           {("RL", 3): 3, ("RL", 5): 2, ("RL", 2): 1, ("GCR", 0): 6, ("ID", 2, "ins"): 1, ("ID", 2, "del"): 1},
           spell("AAA", n=3), spell("AAAAA", n=2), spell("AA")))
case("cigar indel lengths around the last row", "cigar", [R(cigar="%d%s" % (l, op)) for l in (1, IDM - 1, IDM, IDM + 1) for op in "ID"],
     merge(plain(8), sn(bases=3 * IDM + 1, reads_no_seq=4, reads_no_qual=4, inserted_bases=3 * IDM + 1, deleted_bases=3 * IDM + 1, insertions=4, deletions=4),
           {("RL", 0): 4, ("RL", 1): 1, ("RL", IDM - 1): 1, ("RL", IDM): 1, ("RL", IDM + 1): 1, ("GCR", 0): 4},
           {("ID", 1, k): 1 for k in ("ins", "del")}, {("ID", IDM - 1, k): 1 for k in ("ins", "del")}, {("ID", IDM, k): 2 for k in ("ins", "del")},
           {("CYC", c, "A"): 4 if c < 1 else 3 if c < IDM - 1 else 2 if c < IDM else 1 for c in range(IDM + 1)}), cuts=(3,))
case("cigar none, 65 operations, on an unmapped read, of length 0", "cigar",
     [R("AAAAA"),                                           # a mapped read without a CIGAR: no sums
      R(cigar="1M1I" * 32 + "1M"),                          # 65 operations: more than the lanes of a wave
      R(cigar="5M2I", flag=0x4),                            # unmapped: its CIGAR is checked and not summed
      R(cigar="0I5M")],                                     # a length of 0 is no event
     merge(sn(records=4, primary=4, mapped=3, unmapped=1, bases=82, reads_no_qual=4, aligned_bases=38, inserted_bases=32, insertions=32),
           {("MAPQ", 60): 3, ("RL", 5): 2, ("RL", 65): 1, ("RL", 7): 1, ("GCR", 0): 4, ("ID", 1, "ins"): 32},
           {("CYC", c, "A"): 4 if c < 5 else 2 if c < 7 else 1 for c in range(65)}))

# ---- malformed: the record (four T with quality 40) sits between two good reads (one A each), 64 KB of bytes behind it that would count
# as G with quality 68.  It still adds to the field sections — records, primary, mapped, MAPQ 60, RL 4 — and to `malformed`; a missing
# bound shows as a T, a G or a quality
_GOOD = merge(plain(3), sn(malformed=1, bases=2, reads_no_qual=2), {("RL", 1): 2, ("RL", 4): 1, ("GCR", 0): 2, ("CYC", 0, "A"): 2})
for _name, _bad in (("an op code of 9", R("TTTT", qual=40, cigar=[(0, 2), (9, 1), (0, 2)], pad=PAD)),
                    ("a block_size too small for its fields", R("TTTT", qual=40, cigar="4M", patch=((0, "<I", 40),), pad=PAD)),
                    ("n_cigar_op runs past block_size", R("TTTT", qual=40, cigar="4M", patch=((4 + 12, "<H", 2000),), pad=PAD)),
                    ("an l_seq below 0", R("TTTT", qual=40, cigar="4M", patch=((4 + 16, "<i", -4),), pad=PAD))):
    case("malformed " + _name, "malformed", [R("A"), _bad, R("A")], _GOOD, reader_ok=False, cuts=(1,) if "op code" in _name else ())
case("malformed a record that runs past raw_len", "malformed", [R("A"), R("A"), R("TTTT", qual=40, cigar="4M")], _GOOD, reader_ok=False)
CASES[-1]["truncate_last"] = True            # (build: the buffer ends 40 bytes into the last record)

# ---- contention and batch shape
_N = 4096
case("shape 4096 identical reads", "shape", [R("ACGTTGCAAC", qual=37, cigar="10M", flag=0x63, mate_tid=0, tlen=300) for _ in range(_N)],
     merge(sn(records=_N, primary=_N, mapped=_N, paired=_N, read1=_N, proper_pair=_N, both_mapped=_N, bases=10 * _N, bases_q20=10 * _N, bases_q30=10 * _N,
              aligned_bases=10 * _N),
           {("MAPQ", 60): _N, ("RL", 10): _N, ("IS", 300, "inward"): _N, ("GCR", 50): _N, ("QUAL", 37): 10 * _N},
           spell("ACGTTGCAAC", [37] * 10, n=_N)), cuts=(1500,))
for _n in sorted({1, 63, 64, 65, 255, 256, 257, BT - 1, BT, BT + 1, FT - 1, FT, FT + 1}):
    _reads = [R("ACGT"[i % 4] * (1 + i % 3), qual=i % 50, mapq=(5 * i) % 61, flag=0x10 * (i % 2)) for i in range(_n)]
    case("shape a batch of %d reads" % _n, "shape", _reads,
         merge(sn(records=_n, primary=_n, mapped=_n, reverse=_n // 2, mapq0=len(range(0, _n, 61))),      # (5 i mod 61 is 0 for every 61st read)
               *[{("MAPQ", (5 * i) % 61): 1} for i in range(_n)],
               *[mono(1 + i % 3, "ACGT"[i % 4], i % 50, rev=bool(i % 2)) for i in range(_n)]), cuts=(_n // 3,) if _n in (257, BT + 1) else ())
_n = 2 * BT + 5
case("shape the largest quality across the flush bound", "shape", [R("A", qual=254) for _ in range(_n)],
     merge(plain(_n), mono(1, "A", 254, n=_n)))

FAMILIES = sorted({c["family"] for c in CASES})
N_CASES = 59
