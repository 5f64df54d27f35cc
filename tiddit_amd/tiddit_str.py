"""Tandem-repeat genotypes at known loci from the ``--sv`` scan (``TIDDIT_STR=loci.bed``, cuts in ``TIDDIT_STR_CUTS=F`` / ``F:S`` /
``F:S:Q``): for every locus of a catalogue the repeat lengths the reads show between its two neighbour bases, and how far reads that end
inside the repeat keep repeating its motif, from the batches the scan already holds in HBM (csrc/tdt_str.hip: one launch per batch
builds the keys, one sort and the run-length launches per job), written to ``{o}.str.tab``.  No second pass over the BAM, no reference
in HBM.  Nothing in the reference does this.  The definition below is the specification, :func:`keys_of_read` implements it read by
read and :func:`summarise` over the whole job.

THE LOCI FILE (:func:`read_loci`): tab-separated ``chrom start end motif [id]``, 0-based half-open, plain or gzip; lines that start with
``#``, ``track`` or ``browser`` and empty lines are skipped.  A row is accepted when all of these hold, tested in this order, each failure
counted by its reason (``SKIP_REASONS``): it has four columns; the contig is a BAM contig; ``start`` and ``end`` are integers with
``1 <= start < end <= LN - 1`` (both neighbour bases exist); ``end - start <= 10^6``; the motif is 1 to 6 letters of ``ACGT``, either
case; and, after a stable sort of the rows so far by ``(tid, start)``, ``start >= (end of the accepted row in front on that contig) + 1``
— so starts and ends both ascend per contig and two loci never share an anchor with a repeat base.  At most ``MAX_LOCI`` = 2^24 loci are
accepted (``over 2^24 loci``).  The file's motif is TRUSTED to be in phase with the reference at ``start``: ``motif[0]`` is the base at
``start``.  The table is contig-major, a locus's index in it is its ``K1``.

THE CUTS: ``F`` the flank, 1 ... 100, default 5; ``S`` the minimum number of spanning reads for a genotype, 1 ... 10^6, default 5;
``Q`` the minimum MAPQ, 0 ... 255, default 20.

Per record, from the batch's columns ``flag tid pos end mapq rec_off`` and the record's bytes (``raw`` at ``rec_off``):

  1. ``SN records`` += 1.  The record is ELIGIBLE by the keyed consumers' gate: ``flag & 0xF04 == 0``, ``tid >= 0``, ``mapq >= Q``:
        ``SN eligible`` += 1.
  2. A locus ``[s, e)`` of contig ``tid`` (``tid`` below the number of contigs, itself at most 2^24) with anchors ``a = s - 1`` and
        ``b = e`` is IN REACH of the read when ``s <= end`` and ``e >= pos`` (``end`` is the batch's column: ``pos`` + the CIGAR's
        reference length).  Starts and ends ascend, so the loci in reach are ``[lo, hi)``: ``lo`` the first locus with ``e >= pos``,
        ``hi`` the first with ``s > end`` — two lower bounds.  A read with none adds nothing more and its bytes are never looked at;
        else ``SN in_reach`` += 1.
  3. The record is bounded as tdt_indel bounds one (``KS_OPEN``).  It is MALFORMED (``SN malformed`` += 1) when ``pos < 0``, the header
        or the body lies outside ``raw``, ``l_seq < 0``, a CIGAR op code is above 8 (anywhere), or the query index of a defined anchor
        (step 4) of a handled locus is ``>= l_seq``.  ``n_cigar_op == 0``: ``SN no_alignment`` += 1; else ``l_seq == 0``:
        ``SN no_sequence`` += 1.  A read counted in any of the three emits nothing and adds to no other counter.
  4. The first ``MAX_PER_READ`` = 4 loci in reach are HANDLED; every further one adds 1 to ``SN over_cap``.  One walk over the CIGAR,
        ``r = pos``, ``q = 0``: ``M = X`` add their length to both, ``D N`` to ``r``, ``I S`` to ``q``, ``H P`` to neither.  ``qa`` is the
        query index of reference base ``a``, defined only when ``a`` lies in an ``M``, ``=`` or ``X`` operation; ``qb`` the same for ``b``.
  5. Exactly one outcome per (read, handled locus), tested in this order, ``m`` the motif's length:
          SPAN   ``pos <= s - F``, ``end >= e + F``, ``qa`` and ``qb`` defined: ``L = qb - qa - 1`` — every inserted base between the
                 anchors counts, an insertion directly behind ``a`` included.  ``SN span_keys`` += 1.
          LEFT   ``pos <= s - F`` and ``qa`` defined: ``L`` is the largest ``n`` such that every ``0 <= i < n`` has ``qa + 1 + i < l_seq``
                 and the 4-bit base code there is the code of ``motif[i mod m]`` (A C G T = 1 2 4 8).  OPEN when ``qa + 1 + L == l_seq``
                 (the read ended before the repeat did; the run goes through a trailing soft clip).  ``SN left_keys`` += 1.
          RIGHT  ``end >= e + F`` and ``qb`` defined: ``L`` is the largest ``n`` such that every ``0 <= j < n`` has ``qb - 1 - j >= 0`` and
                 the code there is the code of ``motif[(e - 1 - s - j) mod m]`` (the modulo non-negative).  OPEN when ``qb - 1 - L < 0``.
                 ``SN right_keys`` += 1.
          otherwise ``SN unanchored`` += 1.
  6. Keys: ``K1`` = the locus index, ``K2 = kind << 33 | L << 1 | rev``; ``kind`` 0 SPAN, 1 LEFT closed, 2 LEFT open, 3 RIGHT closed,
        4 RIGHT open; ``rev = flag >> 4 & 1``.  Keys with equal ``(K1, K2 >> 1)`` are one set: ``SUPPORT`` their number, ``REV`` those with
        bit 0 set.  Nothing depends on the order of the reads or on where batches are cut.

:func:`summarise`, from the sets (the rows of the finish; it keeps every set): per locus ``REF_LEN = e - s``; ``SPAN_N`` the sum of the
supports of its SPAN rows; ``HIST`` those rows as ``L:n,...`` ascending, ``.`` when there are none.  With ``SPAN_N >= S`` a genotype is
called: order the SPAN rows by ``(-n, |L - REF_LEN|, L)``; ``A1`` is the first row; ``A2`` the second when its ``n >= 2`` and
``5 n >= SPAN_N``, otherwise ``A2 = A1``; the two are printed with the shorter length first (``A1 A1_N A2 A2_N``); ``GT`` is ``0/0``
(both lengths are ``REF_LEN``), ``0/1`` (one is), ``1/1`` (neither, equal) or ``1/2`` (neither, different).  A stated integer rule, not a
calibrated model, as in tiddit_clip_vcf.py.  Below ``S`` the five genotype columns are ``.``.  ``FLANK_N`` is the number of reads of
kinds 1 to 4, ``FLANK_MAX`` the largest ``L`` among the OPEN rows (0 when there are none), ``LONGER`` 1 when ``FLANK_MAX`` is above the
longer called allele — above ``REF_LEN`` when there is no genotype: an allele longer than any spanning read can show.

``{o}.str.tab``: ``# tiddit_amd str v1 flank=F min_reads=S min_mapq=Q``, then ``SN name n`` for the eleven push counters in the order of
``SN``, ``SN loci n`` and one ``SN skipped_...`` row per reason of ``SKIP_REASONS``, then ``#CHROM START END MOTIF ID REF_LEN SPAN_N A1
A1_N A2 A2_N GT FLANK_N FLANK_MAX LONGER HIST`` and one line per accepted locus in table order, all tab-separated (``MOTIF`` in upper
case, ``ID`` ``.`` when the file has none).

NOT BUILT: in-repeat reads with no anchor; checking the motif against the reference; interrupted or compound motifs; indels the aligner
placed outside the anchors; mate-pair (insert-size) evidence; a VCF; N ranks (refused, ``__main__.run_sv``, like ``TIDDIT_INDELS``).
"""
import bisect
import gzip
import struct
import time

import numpy

from . import _native, bamio
from .bamio import _raw_of
from .keyed_counter import KeyedCounter

MAX_PER_READ = 4
MAX_LOCI = 1 << 24
MAX_LOCUS_LEN = 10 ** 6
MAX_MOTIF = 6
DEFAULT_FLANK, DEFAULT_READS, DEFAULT_MAPQ = 5, 5, 20
SN = ("records", "eligible", "in_reach", "malformed", "no_alignment", "no_sequence", "span_keys", "left_keys", "right_keys", "unanchored",
      "over_cap")
SN_INDEX = {k: i for i, k in enumerate(SN)}
SIZE = len(SN)
SKIP_REASONS = ("fewer than four columns", "unknown contig", "coordinates outside the contig", "longer than 10^6", "not a motif of 1 to 6 ACGT",
                "overlaps the locus in front", "over 2^24 loci")
SKIP_SN = ("skipped_columns", "skipped_contig", "skipped_range", "skipped_long", "skipped_motif", "skipped_overlap", "skipped_cap")
COLUMNS = "#CHROM\tSTART\tEND\tMOTIF\tID\tREF_LEN\tSPAN_N\tA1\tA1_N\tA2\tA2_N\tGT\tFLANK_N\tFLANK_MAX\tLONGER\tHIST\n"
SPAN, LEFT_CLOSED, LEFT_OPEN, RIGHT_CLOSED, RIGHT_OPEN = range(5)
# what keys_of_read says about a record
NOT_ELIGIBLE, NOT_IN_REACH, MALFORMED, NO_ALIGNMENT, NO_SEQUENCE, OK = "not_eligible", "not_in_reach", "malformed", "no_alignment", "no_sequence", "ok"
STAGE_SECONDS = {}
STAGE_NOTES = {}
_CODE = {"A": 1, "C": 2, "G": 4, "T": 8}


# ------------------------------------------------------------------------------------------- the switch
def parse_cuts(value):
    """``TIDDIT_STR_CUTS`` -> (F, S, Q); None or empty: the defaults; ValueError (its text is the error line) for anything else"""
    if value is None or value == "":
        return DEFAULT_FLANK, DEFAULT_READS, DEFAULT_MAPQ
    parts = value.split(":")
    if len(parts) > 3 or not all(p.isascii() and p.isdigit() and len(p) <= 9 for p in parts):
        raise ValueError("the cuts are F, F:S or F:S:Q (flank 1 ... 100, minimum spanning reads 1 ... 10^6, minimum MAPQ 0 ... 255)")
    f = int(parts[0])
    s = int(parts[1]) if len(parts) > 1 else DEFAULT_READS
    q = int(parts[2]) if len(parts) > 2 else DEFAULT_MAPQ
    if not 1 <= f <= 100:
        raise ValueError("the flank is 1 ... 100")
    if not 1 <= s <= 10 ** 6:
        raise ValueError("the minimum number of spanning reads is 1 ... 10^6")
    if not 0 <= q <= 255:
        raise ValueError("the minimum MAPQ is 0 ... 255")
    return f, s, q


def parse_switch(path, cuts):
    """(``TIDDIT_STR``, ``TIDDIT_STR_CUTS``) -> None (the switch unset or empty) or (path, F, S, Q); ValueError for cuts without the
    switch and for cuts of another form"""
    if path is None or path == "":
        if cuts is not None and cuts != "":
            raise ValueError("the cuts are those of TIDDIT_STR=loci.bed: TIDDIT_STR not set")
        return None
    return (path,) + parse_cuts(cuts)


# ------------------------------------------------------------------------------------------- the loci
def pack_motif(motif):
    """one uint32: the motif's length in bits 0 ... 3, the BAM 4-bit code of letter i in bits 4 + 4 i ..."""
    return len(motif) | sum(_CODE[c] << (4 + 4 * i) for i, c in enumerate(motif))


class Loci:
    """the accepted loci, contig-major: ``rows`` [(chrom, start, end, MOTIF, id)], the table's columns as the handle takes them
    (``lstart`` / ``lend`` int32, ``motif`` uint32 — :func:`pack_motif` —, ``loc_off`` int64[n_contigs + 1]) and ``skipped`` {reason: rows}"""

    def __init__(self, rows, tids, n_contigs, skipped):
        self.rows = rows
        self.skipped = skipped
        self.lstart = numpy.array([r[1] for r in rows], dtype=numpy.int32)
        self.lend = numpy.array([r[2] for r in rows], dtype=numpy.int32)
        self.motif = numpy.array([pack_motif(r[3]) for r in rows], dtype=numpy.uint32)
        self.loc_off = numpy.searchsorted(numpy.array(tids, dtype=numpy.int64), numpy.arange(n_contigs + 1)).astype(numpy.int64)
        self.starts, self.ends, self.offs = self.lstart.tolist(), self.lend.tolist(), self.loc_off.tolist()      # (for bisect)

    def __len__(self):
        return len(self.rows)


def loci_of_rows(rows, names, lengths):
    """the acceptance rules on already split rows [(chrom, start, end, motif[, id])] (start / end: int or text) -> :class:`Loci`"""
    tid_of = {n: i for i, n in enumerate(names)}
    skipped = {r: 0 for r in SKIP_REASONS}
    ok = []
    for c in rows:
        if len(c) < 4:
            skipped["fewer than four columns"] += 1
            continue
        t = tid_of.get(c[0])
        if t is None:
            skipped["unknown contig"] += 1
            continue
        try:
            s, e = int(c[1]), int(c[2])
        except ValueError:
            s, e = 0, 0
        if not 1 <= s < e <= lengths[t] - 1:
            skipped["coordinates outside the contig"] += 1
            continue
        if e - s > MAX_LOCUS_LEN:
            skipped["longer than 10^6"] += 1
            continue
        motif = str(c[3]).upper()
        if not 1 <= len(motif) <= MAX_MOTIF or any(ch not in _CODE for ch in motif):
            skipped["not a motif of 1 to 6 ACGT"] += 1
            continue
        ok.append((t, s, e, motif, c[4] if len(c) > 4 and c[4] != "" else ".", c[0]))
    ok.sort(key=lambda r: (r[0], r[1]))                            # (stable)
    out, tids = [], []
    last_t, last_e = -1, 0
    for t, s, e, motif, name, chrom in ok:
        if t == last_t and s < last_e + 1:
            skipped["overlaps the locus in front"] += 1
            continue
        if len(out) >= MAX_LOCI:
            skipped["over 2^24 loci"] += 1
            continue
        out.append((chrom, s, e, motif, name))
        tids.append(t)
        last_t, last_e = t, e
    return Loci(out, tids, len(names), skipped)


def read_loci(path, names, lengths):
    """the loci file -> :class:`Loci` for the header's contigs (see the module docstring for what is accepted)"""
    with open(path, "rb") as f:
        zipped = f.read(2) == b"\x1f\x8b"
    rows = []
    with (gzip.open(path, "rt") if zipped else open(path, "r")) as f:
        for line in f:
            if line.startswith(("#", "track", "browser")) or not line.strip():
                continue
            rows.append(line.rstrip("\r\n").split("\t"))
    return loci_of_rows(rows, names, lengths)


# ------------------------------------------------------------------------------------------- the definition
def keys_of_read(loci, flag, tid, pos, end, mapq, rec_off, raw, flank=DEFAULT_FLANK, min_mapq=DEFAULT_MAPQ):
    """THE DEFINITION, one read -> (kind, keys, unanchored, over_cap): ``keys`` the read's [(K1, K2)] when kind is OK, else []; the two
    counts are what the read adds to ``SN unanchored`` / ``SN over_cap``.  ``raw``: the batch's record bytes (bytes-like), the other
    arguments the read's entries of the batch's columns."""
    if flag & 0xF04 or tid < 0 or mapq < min_mapq:
        return NOT_ELIGIBLE, [], 0, 0
    if tid >= len(loci.offs) - 1:
        return NOT_IN_REACH, [], 0, 0
    o0, o1 = loci.offs[tid], loci.offs[tid + 1]
    lo = bisect.bisect_left(loci.ends, pos, o0, o1)                # the first locus with e >= pos
    hi = bisect.bisect_left(loci.starts, end + 1, o0, o1)          # the first locus with s > end
    if hi <= lo:
        return NOT_IN_REACH, [], 0, 0
    bad = (MALFORMED, [], 0, 0)
    raw_len = len(raw)
    if pos < 0 or rec_off + 36 > raw_len:
        return bad
    block_size, = struct.unpack_from("<I", raw, rec_off)
    r0 = rec_off + 4
    l_name = raw[r0 + 8]
    n_cig, = struct.unpack_from("<H", raw, r0 + 12)
    L, = struct.unpack_from("<i", raw, r0 + 16)
    if L < 0 or 32 + l_name + 4 * n_cig + (L + 1) // 2 + L > block_size or rec_off + 4 + block_size > raw_len:
        return bad
    if n_cig == 0:
        return NO_ALIGNMENT, [], 0, 0
    if L == 0:
        return NO_SEQUENCE, [], 0, 0
    cig = r0 + 32 + l_name
    words = struct.unpack_from("<%dI" % n_cig, raw, cig)
    if any((w & 0xf) > 8 for w in words):
        return bad
    mine = list(range(lo, min(hi, lo + MAX_PER_READ)))
    qa, qb = {}, {}
    r, q = pos, 0
    for w in words:
        op, ln = w & 0xf, w >> 4
        if op in (0, 7, 8):
            for k in mine:
                a, b = loci.starts[k] - 1, loci.ends[k]
                if r <= a < r + ln:
                    qa[k] = q + a - r
                if r <= b < r + ln:
                    qb[k] = q + b - r
        if op in (0, 2, 3, 7, 8):
            r += ln
        if op in (0, 1, 4, 7, 8):
            q += ln
    if any(v >= L for v in qa.values()) or any(v >= L for v in qb.values()):
        return bad
    seq = cig + 4 * n_cig
    code = lambda i: (raw[seq + (i >> 1)] >> (0 if i & 1 else 4)) & 0xf
    rev = (flag >> 4) & 1
    keys, un = [], 0
    for k in mine:
        s, e, motif = loci.starts[k], loci.ends[k], loci.rows[k][3]
        m = len(motif)
        left, right = pos <= s - flank and k in qa, end >= e + flank and k in qb
        if left and right:
            kind, n = SPAN, qb[k] - qa[k] - 1
        elif left:
            n = 0
            while qa[k] + 1 + n < L and code(qa[k] + 1 + n) == _CODE[motif[n % m]]:
                n += 1
            kind = LEFT_OPEN if qa[k] + 1 + n == L else LEFT_CLOSED
        elif right:
            n = 0
            while qb[k] - 1 - n >= 0 and code(qb[k] - 1 - n) == _CODE[motif[(e - 1 - s - n) % m]]:
                n += 1
            kind = RIGHT_OPEN if qb[k] - 1 - n < 0 else RIGHT_CLOSED
        else:
            un += 1
            continue
        keys.append((k, kind << 33 | n << 1 | rev))
    return OK, keys, un, hi - lo - len(mine)


def _count(sn, kind, keys, un, over):
    add = lambda k, n: sn.__setitem__(k, sn.get(k, 0) + n) if n else None
    add("records", 1)
    if kind == NOT_ELIGIBLE:
        return
    add("eligible", 1)
    if kind == NOT_IN_REACH:
        return
    add("in_reach", 1)
    add("malformed", int(kind == MALFORMED))
    add("no_alignment", int(kind == NO_ALIGNMENT))
    add("no_sequence", int(kind == NO_SEQUENCE))
    add("span_keys", sum(1 for _, k2 in keys if k2 >> 33 == SPAN))
    add("left_keys", sum(1 for _, k2 in keys if k2 >> 33 in (LEFT_CLOSED, LEFT_OPEN)))
    add("right_keys", sum(1 for _, k2 in keys if k2 >> 33 in (RIGHT_CLOSED, RIGHT_OPEN)))
    add("unanchored", un)
    add("over_cap", over)


def keys_of_batch(b, loci, keys, sn, flank=DEFAULT_FLANK, min_mapq=DEFAULT_MAPQ):
    """the definition over one batch, read by read: appends (K1, K2) to ``keys`` and adds to the push counters ``sn`` (a dict)"""
    raw = _raw_of(b)
    for i in range(len(b.tid)):
        kind, ks, un, over = keys_of_read(loci, int(b.flag[i]), int(b.tid[i]), int(b.pos[i]), int(b.end[i]), int(b.mapq[i]), int(b.rec_off[i]), raw, flank, min_mapq)
        _count(sn, kind, ks, un, over)
        keys.extend(ks)


def counts_of(sn):
    """the push counters (a dict) -> uint64[SIZE]"""
    c = numpy.zeros(SIZE, dtype=numpy.uint64)
    for k, v in (sn or {}).items():
        c[SN_INDEX[k]] = v
    return c


def rows_of_keys(keys):
    """every keyed outcome's (K1, K2) in any order -> the sets [(K1, K2 with bit 0 clear, SUPPORT, REV)], ascending: what the finish gives"""
    sets = {}
    for k1, k2 in keys:
        s = sets.setdefault((k1, k2 >> 1), [0, 0])
        s[0] += 1
        s[1] += k2 & 1
    return [(k1, e << 1, s[0], s[1]) for (k1, e), s in sorted(sets.items())]


def genotype(spans, ref_len, min_reads):
    """the SPAN rows of one locus {L: n} -> (A1, A1_N, A2, A2_N, GT), the shorter length first, or None below ``min_reads``"""
    total = sum(spans.values())
    if total < min_reads or not spans:
        return None
    order = sorted(spans.items(), key=lambda r: (-r[1], abs(r[0] - ref_len), r[0]))
    a1 = order[0]
    a2 = order[1] if len(order) > 1 and order[1][1] >= 2 and 5 * order[1][1] >= total else a1
    (x, xn), (y, yn) = sorted((a1, a2))
    nref = (x == ref_len) + (y == ref_len)
    gt = "0/0" if nref == 2 else "0/1" if nref == 1 else "1/1" if x == y else "1/2"
    return x, xn, y, yn, gt


def summarise(loci, rows, min_reads=DEFAULT_READS):
    """THE DEFINITION, the whole job: ``rows`` = the sets of the finish, [(K1, K2 with bit 0 clear, SUPPORT, REV)] or the four columns ->
    one tuple per accepted locus, in table order: (REF_LEN, SPAN_N, genotype or None, FLANK_N, FLANK_MAX, LONGER, HIST text)"""
    if isinstance(rows, tuple):
        rows = list(zip(*(numpy.asarray(r).tolist() for r in rows)))
    spans = [{} for _ in range(len(loci))]
    flank_n, flank_max = [0] * len(loci), [0] * len(loci)
    for k1, k2, sup, _rev in rows:
        kind, n = k2 >> 33, (k2 >> 1) & 0xffffffff
        if kind == SPAN:
            spans[k1][n] = spans[k1].get(n, 0) + sup
        else:
            flank_n[k1] += sup
            if kind in (LEFT_OPEN, RIGHT_OPEN):
                flank_max[k1] = max(flank_max[k1], n)
    out = []
    for k, (_chrom, s, e, _motif, _name) in enumerate(loci.rows):
        ref_len = e - s
        g = genotype(spans[k], ref_len, min_reads)
        longer = int(flank_max[k] > (max(g[0], g[2]) if g is not None else ref_len))
        hist = ",".join("%d:%d" % r for r in sorted(spans[k].items())) or "."
        out.append((ref_len, sum(spans[k].values()), g, flank_n[k], flank_max[k], longer, hist))
    return out


# ------------------------------------------------------------------------------------------- the device handle
class StrCounter(KeyedCounter):
    """``tdt_str_*``: the loci table, the key store and the counters in HBM; one push per batch of the scan, one finish per job."""
    PREFIX, SIZE = "tdt_str", SIZE

    def __init__(self, loci, flank=DEFAULT_FLANK, min_mapq=DEFAULT_MAPQ, capacity=1 << 16, ctx=None):
        self.loci = loci
        self._create(ctx, _native.ptr(loci.lstart), _native.ptr(loci.lend), _native.ptr(loci.motif), _native.ptr(loci.loc_off), len(loci.loc_off) - 1,
                     int(flank), int(min_mapq), int(capacity))
        self.flank, self.min_mapq = int(flank), int(min_mapq)

    def push_host_batch(self, b):
        """one host-decoded batch (or any object with its columns): uploaded, then the same kernel"""
        cols, raw = bamio.host_columns(b, ("flag", "tid", "pos", "end", "mapq", "rec_off"))      # (the arguments of tdt_str_push, in order)
        _native.check(self._c("push")(self.handle, *[_native.ptr(c) for c in cols], len(cols[0]), _native.ptr(raw), len(raw)))

    def finish(self):
        """-> uint64[SIZE]: the push counters; the sets are sorted out of the store (which is left as it was), every one a row"""
        import ctypes
        out = numpy.zeros(self.SIZE, dtype=numpy.uint64)
        n = ctypes.c_size_t(0)
        _native.check(self._c("finish")(self.handle, _native.ptr(out), ctypes.byref(n)))
        self._n_rows = n.value
        return out


class ScanTap:
    """what ``tiddit_signal.STR`` holds while a scan is to fill a counter: the loci and the cuts, and behind the scan the counter"""

    def __init__(self, loci, flank, min_reads, min_mapq):
        self.loci, self.flank, self.min_reads, self.min_mapq = loci, int(flank), int(min_reads), int(min_mapq)
        self.counter = None


def attach(loci, cuts):
    """the next scan of this process also fills a :class:`StrCounter` for ``loci`` at the cuts (F, S, Q) -> the tap it will leave it in"""
    from . import tiddit_signal
    tiddit_signal.STR = ScanTap(loci, *cuts)
    return tiddit_signal.STR


def detach():
    """the scans from here on do what they do without the switch (a counter a scan left in the tap stays the caller's)"""
    from . import tiddit_signal
    tiddit_signal.STR = None


# ------------------------------------------------------------------------------------------- the file
def write_file(path, loci, counts, table, flank, min_reads, min_mapq):
    """``{o}.str.tab`` (see the module docstring); ``table``: what :func:`summarise` gave"""
    c = [int(v) for v in numpy.asarray(counts).tolist()]
    out = ["# tiddit_amd str v1 flank=%d min_reads=%d min_mapq=%d\n" % (flank, min_reads, min_mapq)]
    out += ["SN\t%s\t%d\n" % (k, c[i]) for i, k in enumerate(SN)]
    out.append("SN\tloci\t%d\n" % len(loci))
    out += ["SN\t%s\t%d\n" % (name, loci.skipped[r]) for name, r in zip(SKIP_SN, SKIP_REASONS)]
    out.append(COLUMNS)
    for (chrom, s, e, motif, name), (ref_len, span_n, g, flank_n, flank_max, longer, hist) in zip(loci.rows, table):
        gt = "%d\t%d\t%d\t%d\t%s" % g if g is not None else ".\t.\t.\t.\t."
        out.append("%s\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s\n" % (chrom, s, e, motif, name, ref_len, span_n, gt, flank_n, flank_max, longer, hist))
    with open(path, "w") as f:
        f.write("".join(out))


def summary_line(counts, loci, table):
    c = numpy.asarray(counts)
    return "str: {} loci, {} records, {} eligible, {} in reach, {} spanning, {} flanking keys, {} genotyped, {} flagged longer, malformed records {}".format(
        len(loci), *(int(c[SN_INDEX[k]]) for k in ("records", "eligible", "in_reach", "span_keys")),
        int(c[SN_INDEX["left_keys"]]) + int(c[SN_INDEX["right_keys"]]), sum(1 for t in table if t[2] is not None), sum(t[5] for t in table),
        int(c[SN_INDEX["malformed"]]))


def main(counter, loci, prefix, cuts):
    """the stage behind the scan: the sort and the run lengths on the device, the genotype rule, the file and the summary line"""
    STAGE_SECONDS.clear()
    STAGE_NOTES.clear()
    t = time.time()
    counts = counter.finish()
    rows = counter.rows()
    ms = counter.timing()
    asks, grows, cap = counter.reserve_stats()
    counter.close()
    STAGE_SECONDS["str sets (device: two sorts, gather, run lengths, rows)"] = time.time() - t
    for k, v in zip(("sort by K2", "gather of K1", "sort by K1", "run lengths + rows"), ms.tolist()):
        STAGE_SECONDS["  " + k + " (device time)"] = v * 1e-3
    STAGE_NOTES.update({"str store: reserves that asked the device": asks, "str store: growths": grows, "str store: capacity (keys)": cap})
    t = time.time()
    table = summarise(loci, rows, cuts[1])
    write_file(prefix + ".str.tab", loci, counts, table, *cuts)
    STAGE_SECONDS["str genotype rule + table text (host)"] = time.time() - t
    print(summary_line(counts, loci, table))
    return counts
