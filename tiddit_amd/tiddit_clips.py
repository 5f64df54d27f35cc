"""Clipped-read breakpoint sites from the ``--sv`` scan (``TIDDIT_CLIPS=1`` / ``S`` / ``S:Q`` / ``S:Q:L``): every reference position where
at least ``S`` eligible reads are soft-clipped on the same side, with the support by strand and a consensus of the clipped bases beside
the breakpoint, from the batches the scan already holds in HBM (csrc/tdt_clip.hip: one launch per batch builds at most two keys per
read, one sort and the run-length launches of the shared key store per job, then a segmented vote over its rows), written to
``{o}.clips.tab``.  The reference selects clipped reads for a local assembly and has no such table.  The definition below is the
specification, :func:`events_of_read` implements it read by read and :func:`summarise` over the whole job.

The switch: ``S`` is the minimum support, 1 ... 10^6, default 3; ``Q`` the minimum MAPQ, 0 ... 255, default 20; ``L`` the minimum clip
length, 1 ... 65535, default 10.  A bare ``1`` means the defaults; a support of 1 is written ``1:20``.

Per record, from the batch's columns ``flag tid pos mapq rec_off`` and the record's bytes (``raw`` at ``rec_off``):

  1. ``SN records`` += 1.  The record is ELIGIBLE when ``flag & 0xF04 == 0`` (mapped, primary, not QC-failed, not marked duplicate),
        ``tid >= 0`` and ``mapq >= Q``: ``SN eligible`` += 1.  Nothing else is done for the others, and their bytes are never read.
  2. The record is bounded as ``tdt_snv`` bounds one (rule 2 of tiddit_snvs.py): ``rec_off + 36 <= raw_len``, its own ``l_seq >= 0``,
        ``32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size`` and ``rec_off + 4 + block_size <= raw_len``.  It is
        MALFORMED (``SN malformed`` += 1, nothing else) when the bound fails, a CIGAR op code is above 8, ``tid >= 2^24``, ``pos < 0``,
        ``pos`` plus the CIGAR's reference length (``M D N = X``) exceeds ``2^31 - 1``, or the CIGAR's query length (``M I S = X``) differs
        from ``l_seq`` when ``l_seq >= 1`` and ``n_cigar_op >= 1``.  Nothing outside ``[raw, raw + raw_len)`` is ever read.
  3. A well-bounded record with ``n_cigar_op == 0`` or ``l_seq == 0``: ``SN no_sequence`` += 1, nothing else.  Otherwise a CIGAR whose
        reference length is 0 (all ``S``, say): ``SN no_alignment`` += 1, nothing else.
  4. The LEADING clip is an ``S`` operation at CIGAR index 0, or at index 1 when index 0 is ``H``; the TRAILING clip the ``S`` at the last
        index, or at the last but one when the last is ``H``.  (Behind rule 3 the two are never one operation.)  ``H`` alone is no clip.
        A clip shorter than ``L`` adds 1 to ``SN short_clips`` and is no event.  Otherwise it is an EVENT: the leading clip with
        ``side = L = 0`` and ``P = pos + 1``, the first aligned base, 1-based; the trailing clip with ``side = R = 1`` and
        ``P = pos + reflen``, the last aligned base.  ``SN left_clips`` / ``SN right_clips`` += 1 per event, ``SN clipped_reads`` += 1 for
        a read with any.  A read gives at most two events.
  5. The stored bases are taken OUTWARD from the breakpoint: for ``L`` column ``j`` is the query base at index ``cliplen - 1 - j`` of
        the clip (the clip starts at query index 0), for ``R`` the clip's base ``j`` (the clip ends at ``l_seq``).  Bases are kept while
        their 4-bit codes are 1, 2, 4, 8 (A C G T), up to ``CLIP_COLS`` = 28 columns; ``n`` is the number kept.
        ``n < min(cliplen, 28)`` adds 1 to ``SN cut_at_other_base``.  An event with ``n == 0`` is still an event.
  6. Keys, ``rev = flag >> 4 & 1``: ``K1 = tid << 32 | P``, ``K2 = side << 63 | n << 58 | bases << 2 | rev``; bit 1 is always 0.  ``bases``
        holds column ``j`` in bits ``2j + 1 : 2j`` of its 56 bits, A C G T = 0 1 2 3, and the columns at and above ``n`` are zero.  Equal
        ``(K1, K2 >> 1)`` is one distinct sequence, as the shared finish counts them: ``SN distinct_sequences`` is their number.
  7. A SITE is all keys with equal ``(K1, side)``.  ``SUPPORT`` is its events, ``REV`` those with bit 0 set, ``FWD`` the rest, ``SEQS`` its
        distinct sequences.  Per column ``j``, ``depth_j`` is the number of events with ``n > j`` (it does not increase with ``j``), and
        the votes of the column are those events by base.  ``CLEN`` is the number of leading columns with ``depth_j >= S``.  The
        consensus base of a column is the one with the most votes, a tie going to the smaller code.  ``AGREE`` is the sum of the winning
        votes over the ``CLEN`` columns, ``TOTAL`` the sum of ``depth_j`` over them.  ``SN distinct_sites`` counts the sites,
        ``SN reported_sites`` those with ``SUPPORT >= S``.  Nothing depends on the order of the reads.

``{o}.clips.tab``: ``# tiddit_amd clips v1 min_support=S min_mapq=Q min_clip=L cols=28``, then ``SN name n`` for the thirteen counters in
the order of ``SN``, then ``#CHROM POS SIDE SUPPORT FWD REV SEQS CLEN CONSENSUS AGREE TOTAL COV`` and one row per reported site,
ascending by ``(K1, side)``, all tab-separated.  ``POS = P``; ``SIDE`` is ``L`` or ``R``; ``CONSENSUS`` is written in reference direction,
so the columns of an ``L`` site are reversed, and is ``.`` when ``CLEN`` is 0; ``COV`` is ``"%.2f"`` of the job's own 50-bp coverage bin
``coverage_data[chrom][(P - 1) // 50]``, ``.`` when the job holds no bins for that contig (or none that far), as
``tiddit_snvs.write_file`` writes it.

Where the clipped bases come from is tiddit_clip_align.py's (``TIDDIT_CLIPS_ALIGN``): the consensus placed on the same contig, and the
DEL / DUP / INV the junction implies; and tiddit_clip_far.py's (``TIDDIT_CLIPS_FAR``): the consensus placed on any contig by its seed.

Clipped bases beyond the 28 columns, up to 140, and the insertions that two facing sites close are tiddit_clip_ins.py's
(``TIDDIT_CLIPS_INS``), from a second key store beside this one (:meth:`ClipCounter.enable_ext`).

NOT built: more than 140 clipped bases of a clip; joining the sites to the VCF; hard clips (``H`` alone is no clip, and
the bases it removed are not in the record); supplementary records (0x800 is not eligible); N ranks (refused in ``__main__.run_sv``: a
site's keys can straddle shards).
"""
import ctypes
import struct
import time

import numpy

from . import _native
from .bamio import _raw_of
from .keyed_counter import KeyedCounter

CLIP_COLS = 28
CLIP_MAX_PER_READ = 2
CLIP_MAX_CONTIGS = 1 << 24
END_LIMIT = (1 << 31) - 1
MAX_SUPPORT = 10 ** 6
MAX_CLIP = 65535
DEFAULT_SUPPORT, DEFAULT_MAPQ, DEFAULT_CLIP = 3, 20, 10
SN = ("records", "eligible", "malformed", "no_sequence", "no_alignment", "short_clips", "left_clips", "right_clips", "clipped_reads",
      "cut_at_other_base", "distinct_sequences", "distinct_sites", "reported_sites")
SN_INDEX = {k: i for i, k in enumerate(SN)}
SIZE = len(SN)
COLUMNS = "#CHROM\tPOS\tSIDE\tSUPPORT\tFWD\tREV\tSEQS\tCLEN\tCONSENSUS\tAGREE\tTOTAL\tCOV\n"
ROW_DTYPES = (numpy.uint64, numpy.uint32, numpy.uint32, numpy.uint32, numpy.uint32, numpy.uint32, numpy.uint64, numpy.uint64, numpy.uint64)
STAGE_SECONDS = {}
STAGE_NOTES = {}            # counts of the last main() that are not seconds
# what events_of_read says about a record
NOT_ELIGIBLE, MALFORMED, NO_SEQUENCE, NO_ALIGNMENT, OK = "not_eligible", "malformed", "no_sequence", "no_alignment", "ok"
_CODE = {1: 0, 2: 1, 4: 2, 8: 3}


def parse_switch(value):
    """``TIDDIT_CLIPS`` -> None (unset or empty) or (S, Q, L); ValueError (its text is the error line) for anything else"""
    if value is None or value == "":
        return None
    if value == "1":
        return DEFAULT_SUPPORT, DEFAULT_MAPQ, DEFAULT_CLIP
    parts = value.split(":")
    if len(parts) > 3 or not all(p.isascii() and p.isdigit() and len(p) <= 9 for p in parts):
        raise ValueError("the switch is 1, S, S:Q or S:Q:L (minimum support 1 ... 10^6, minimum MAPQ 0 ... 255, minimum clip length 1 ... 65535)")
    s = int(parts[0])
    q = int(parts[1]) if len(parts) >= 2 else DEFAULT_MAPQ
    c = int(parts[2]) if len(parts) == 3 else DEFAULT_CLIP
    if not 1 <= s <= MAX_SUPPORT:
        raise ValueError("the minimum support is 1 ... 10^6")
    if not 0 <= q <= 255:
        raise ValueError("the minimum MAPQ is 0 ... 255")
    if not 1 <= c <= MAX_CLIP:
        raise ValueError("the minimum clip length is 1 ... 65535")
    return s, q, c


# ------------------------------------------------------------------------------------------- the definition
def clips_of_read(flag, tid, pos, mapq, rec_off, raw, min_mapq=DEFAULT_MAPQ, min_clip=DEFAULT_CLIP):
    """rules 1 to 4, one read -> (kind, clips, short_clips, base): ``clips`` the read's events before their bases are taken,
    [(side, P, cliplen, q0)] (the leading clip's first) when kind is OK, else []; column ``j`` of a clip is the query base at index
    ``q0 - j`` (L) or ``q0 + j`` (R), and ``base(qi)`` gives a query base's 4-bit code (None unless kind is OK)"""
    if flag & 0xF04 or tid < 0 or mapq < min_mapq:
        return NOT_ELIGIBLE, [], 0, None
    bad = (MALFORMED, [], 0, None)
    raw_len = len(raw)
    if tid >= CLIP_MAX_CONTIGS or pos < 0 or rec_off + 36 > raw_len:
        return bad
    block_size, = struct.unpack_from("<I", raw, rec_off)
    r0 = rec_off + 4
    l_name = raw[r0 + 8]
    n_cig, = struct.unpack_from("<H", raw, r0 + 12)
    L, = struct.unpack_from("<i", raw, r0 + 16)
    if L < 0 or 32 + l_name + 4 * n_cig + (L + 1) // 2 + L > block_size or rec_off + 4 + block_size > raw_len:
        return bad
    cig = r0 + 32 + l_name
    words = struct.unpack_from("<%dI" % n_cig, raw, cig)
    if any((w & 0xf) > 8 for w in words):
        return bad
    ref_len = sum(w >> 4 for w in words if (w & 0xf) in (0, 2, 3, 7, 8))
    query_len = sum(w >> 4 for w in words if (w & 0xf) in (0, 1, 4, 7, 8))
    if pos + ref_len > END_LIMIT or (L >= 1 and n_cig >= 1 and query_len != L):
        return bad
    if n_cig == 0 or L == 0:
        return NO_SEQUENCE, [], 0, None
    if ref_len == 0:
        return NO_ALIGNMENT, [], 0, None
    seq = cig + 4 * n_cig
    ops = [(w & 0xf, w >> 4) for w in words]
    lead = 0 if ops[0][0] == 4 else 1 if ops[0][0] == 5 and n_cig >= 2 and ops[1][0] == 4 else None
    trail = n_cig - 1 if ops[-1][0] == 4 else n_cig - 2 if ops[-1][0] == 5 and n_cig >= 2 and ops[-2][0] == 4 else None
    assert lead is None or lead != trail
    base = lambda qi: (raw[seq + (qi >> 1)] >> (0 if qi & 1 else 4)) & 0xf
    clips, short = [], 0
    for side, at in ((0, lead), (1, trail)):
        if at is None:
            continue
        cliplen = ops[at][1]
        if cliplen < min_clip:
            short += 1
            continue
        clips.append((side, pos + 1 if side == 0 else pos + ref_len, cliplen, cliplen - 1 if side == 0 else L - cliplen))
    return OK, clips, short, base


def kept_bases(side, cliplen, q0, base, cols):
    """rule 5 up to ``cols`` columns -> the kept codes (0 ... 3) outward from the breakpoint, cut at the first other base"""
    out = []
    while len(out) < min(cliplen, cols):
        c = base(q0 - len(out) if side == 0 else q0 + len(out))
        if c not in _CODE:
            break
        out.append(_CODE[c])
    return out


def events_of_read(flag, tid, pos, mapq, rec_off, raw, min_mapq=DEFAULT_MAPQ, min_clip=DEFAULT_CLIP):
    """THE DEFINITION, one read -> (kind, keys, short_clips, cut): ``keys`` the read's [(K1, K2)] (at most two, the leading clip's
    first) when kind is OK, else []; the two counts are what the read adds to ``SN short_clips`` / ``SN cut_at_other_base``.  ``raw``:
    the batch's record bytes (bytes-like), the other arguments the read's entries of the batch's columns."""
    kind, clips, short, base = clips_of_read(flag, tid, pos, mapq, rec_off, raw, min_mapq, min_clip)
    rev = (flag >> 4) & 1
    keys, cut = [], 0
    for side, P, cliplen, q0 in clips:
        kept = kept_bases(side, cliplen, q0, base, CLIP_COLS)
        n, bases = len(kept), sum(c << (2 * j) for j, c in enumerate(kept))
        cut += int(n < min(cliplen, CLIP_COLS))
        keys.append((tid << 32 | P, side << 63 | n << 58 | bases << 2 | rev))
    return kind, keys, short, cut


def _count(sn, kind, keys, short, cut):
    add = lambda k, n: sn.__setitem__(k, sn.get(k, 0) + n) if n else None
    add("records", 1)
    if kind == NOT_ELIGIBLE:
        return
    add("eligible", 1)
    add("malformed", int(kind == MALFORMED))
    add("no_sequence", int(kind == NO_SEQUENCE))
    add("no_alignment", int(kind == NO_ALIGNMENT))
    add("short_clips", short)
    add("left_clips", sum(1 for _, k2 in keys if not k2 >> 63))
    add("right_clips", sum(1 for _, k2 in keys if k2 >> 63))
    add("clipped_reads", int(bool(keys)))
    add("cut_at_other_base", cut)


def keys_of_batch_by_read(b, keys, sn, min_mapq=DEFAULT_MAPQ, min_clip=DEFAULT_CLIP, kinds=None):
    """the definition over one batch, read by read: appends (K1, K2) to ``keys`` and adds to the push counters ``sn`` (a dict);
    ``kinds``: a list that gets every record's kind"""
    raw = _raw_of(b)
    for i in range(len(b.tid)):
        kind, ks, short, cut = events_of_read(int(b.flag[i]), int(b.tid[i]), int(b.pos[i]), int(b.mapq[i]), int(b.rec_off[i]), raw, min_mapq, min_clip)
        _count(sn, kind, ks, short, cut)
        keys.extend(ks)
        if kinds is not None:
            kinds.append(kind)


def summarise(keys, sn=None, min_support=DEFAULT_SUPPORT):
    """THE DEFINITION, the whole job: ``keys`` = every event's (K1, K2) in any order, ``sn`` the push counters -> (uint64[SIZE], rows):
    rows = [(K1, side, SUPPORT, REV, SEQS, CLEN, consensus, AGREE, TOTAL)] of the sites with SUPPORT >= min_support, ascending by
    (K1, side); consensus holds column j's winner in bits 2j + 1 : 2j, zero at and above CLEN"""
    c = numpy.zeros(SIZE, dtype=numpy.uint64)
    for k, v in (sn or {}).items():
        c[SN_INDEX[k]] = v
    sites = {}
    for k1, k2 in keys:
        s = sites.setdefault((k1, k2 >> 63), {"support": 0, "rev": 0, "seqs": set(), "votes": [[0, 0, 0, 0] for _ in range(CLIP_COLS)]})
        s["support"] += 1
        s["rev"] += k2 & 1
        s["seqs"].add(k2 >> 1)
        for j in range((k2 >> 58) & 31):
            s["votes"][j][(k2 >> (2 + 2 * j)) & 3] += 1
    rows = []
    for (k1, side), s in sorted(sites.items()):
        if s["support"] < min_support:
            continue
        clen = 0
        while clen < CLIP_COLS and sum(s["votes"][clen]) >= min_support:
            clen += 1
        cons = agree = total = 0
        for j in range(clen):
            v = s["votes"][j]
            w = v.index(max(v))                                  # (the first of equal maxima: the smaller code)
            cons |= w << (2 * j)
            agree += v[w]
            total += sum(v)
        rows.append((k1, side, s["support"], s["rev"], len(s["seqs"]), clen, cons, agree, total))
    c[SN_INDEX["distinct_sequences"]] = sum(len(s["seqs"]) for s in sites.values())
    c[SN_INDEX["distinct_sites"]] = len(sites)
    c[SN_INDEX["reported_sites"]] = len(rows)
    return c, rows


def consensus_text(side, clen, cons):
    """the packed consensus of a row in reference direction; ``.`` for no column"""
    s = "".join("ACGT"[(cons >> (2 * j)) & 3] for j in range(clen))
    return (s[::-1] if side == 0 else s) or "."


# ------------------------------------------------------------------------------------------- the device handle
class ClipCounter(KeyedCounter):
    """``tdt_clip_*``: the key store and the counters in HBM; one push per batch of the scan, one finish per job (one sort of the store
    and the vote over its rows).  ``rows()``: (K1 uint64[], side, SUPPORT, REV, SEQS, CLEN uint32[], consensus, AGREE, TOTAL uint64[]) of
    the last finish, ascending by (K1, side); ``timing()``: the key store's four and [4] site heads + vote + site rows."""
    PREFIX, SIZE, DEFAULT_SUPPORT = "tdt_clip", SIZE, DEFAULT_SUPPORT
    ROW_DTYPES, N_TIMES = ROW_DTYPES, 5

    def __init__(self, n_contigs, min_mapq=DEFAULT_MAPQ, min_clip=DEFAULT_CLIP, capacity=1 << 20, ctx=None):
        self._create(ctx, int(n_contigs), int(min_mapq), int(min_clip), int(capacity))
        self.min_mapq, self.min_clip = int(min_mapq), int(min_clip)

    # ---- TIDDIT_CLIPS_INS (tiddit_clip_ins.py): a second store for the clipped bases beyond column 28, filled by every later push
    def enable_ext(self, capacity=1 << 20):
        """``tdt_clip_ext_enable``: before the first push"""
        _native.check(self._c("ext_enable")(self.handle, int(capacity)))

    def ext_keys(self):
        """-> (K1 uint64[], K2 uint64[]): the extension store as it lies in HBM"""
        n = ctypes.c_size_t(0)
        _native.check(self._c("ext_keys")(self.handle, None, None, ctypes.byref(n)))
        k1, k2 = numpy.zeros(n.value, dtype=numpy.uint64), numpy.zeros(n.value, dtype=numpy.uint64)
        if n.value:
            _native.check(self._c("ext_keys")(self.handle, _native.ptr(k1), _native.ptr(k2), ctypes.byref(n)))
        return k1, k2

    def ins(self, K, O, M):
        """``tdt_clip_ins`` on the rows of the last finish, where they lie -> uint64[tiddit_clip_ins.SIZE]"""
        from . import tiddit_clip_ins
        sn = numpy.zeros(tiddit_clip_ins.SIZE, dtype=numpy.uint64)
        _native.check(self._c("ins")(self.handle, int(K), int(O), int(M), _native.ptr(sn)))
        self._n_pairs = int(sn[tiddit_clip_ins.SN_INDEX["pairs"]])
        return sn

    def ext_rows(self):
        """-> (ECLEN uint32[], cons5 uint64[n][5]) of the last ``ins``, in the order of ``rows()``"""
        n = ctypes.c_size_t(self._n_rows)
        eclen, cons5 = numpy.zeros(n.value, dtype=numpy.uint32), numpy.zeros((n.value, 5), dtype=numpy.uint64)
        if n.value:
            _native.check(self._c("ext_rows")(self.handle, _native.ptr(eclen), _native.ptr(cons5), ctypes.byref(n)))
        return eclen, cons5

    def ins_rows(self):
        """-> ((R row, L row, TSD, status, LEN, MISMATCH, CLOSURES) uint32[], seq10 uint64[n][10]) of the last ``ins``"""
        n = ctypes.c_size_t(getattr(self, "_n_pairs", 0))
        cols, seq10 = [numpy.zeros(n.value, dtype=numpy.uint32) for _ in range(7)], numpy.zeros((n.value, 10), dtype=numpy.uint64)
        if n.value:
            _native.check(self._c("ins_rows")(self.handle, *[_native.ptr(c) for c in cols], _native.ptr(seq10), ctypes.byref(n)))
        return tuple(cols), seq10

    def ins_timing(self):
        """ms of the last ``ins``: [the extension store's finish, the gather, the pair launches]"""
        return self._out("ins_timing", 3, numpy.float64)

    # ---- TIDDIT_CLIPS_MEI (tiddit_clip_mei.py): the pair rows of the last ``ins`` named against a family library
    def mei(self, lib, A):
        """``tdt_clip_mei`` on the pair rows of the last ``ins``, where they lie; ``lib``: a refseq.RefSeq with every sequence loaded
        -> uint64[tiddit_clip_mei.SIZE]"""
        from . import tiddit_clip_mei
        sn = numpy.zeros(tiddit_clip_mei.SIZE, dtype=numpy.uint64)
        _native.check(self._c("mei")(self.handle, lib.handle, int(A), _native.ptr(sn)))
        self._n_mei = int(sn[tiddit_clip_mei.SN_INDEX["queries"]])
        return sn

    def mei_rows(self):
        """-> (pair row, part, QLEN uint32[], the nine result columns uint32[]) of the last ``mei``, one entry per query"""
        n = ctypes.c_size_t(getattr(self, "_n_mei", 0))
        cols = [numpy.zeros(n.value, dtype=numpy.uint32) for _ in range(12)]
        if n.value:
            _native.check(self._c("mei_rows")(self.handle, *[_native.ptr(c) for c in cols], ctypes.byref(n)))
        return cols[0], cols[1], cols[2], tuple(cols[3:])

    def mei_timing(self):
        """ms of the last ``mei``: [the query build, the alignment launch, the reduction]"""
        return self._out("mei_timing", 3, numpy.float64)


# ------------------------------------------------------------------------------------------- the file
def write_file(path, counts, rows, names, coverage_data, min_support, min_mapq, min_clip):
    """``{o}.clips.tab`` (see the module docstring); rows: the nine columns of :meth:`ClipCounter.rows` or a list of row tuples"""
    if isinstance(rows, tuple):
        rows = list(zip(*(numpy.asarray(r).tolist() for r in rows)))
    c = [int(v) for v in numpy.asarray(counts).tolist()]
    out = ["# tiddit_amd clips v1 min_support=%d min_mapq=%d min_clip=%d cols=%d\n" % (min_support, min_mapq, min_clip, CLIP_COLS)]
    out += ["SN\t%s\t%d\n" % (k, c[i]) for i, k in enumerate(SN)]
    out.append(COLUMNS)
    for k1, side, sup, rev, seqs, clen, cons, agree, total in rows:
        tid, P = k1 >> 32, k1 & 0xffffffff
        chrom = names[tid] if tid < len(names) else str(tid)
        bins = coverage_data.get(chrom) if coverage_data is not None else None
        cov = "%.2f" % float(bins[(P - 1) // 50]) if bins is not None and (P - 1) // 50 < len(bins) else "."
        out.append("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%s\n" % (chrom, P, "LR"[side], sup, sup - rev, rev, seqs, clen,
                                                                       consensus_text(side, clen, cons), agree, total, cov))
    with open(path, "w") as f:
        f.write("".join(out))


def summary_line(counts):
    c = numpy.asarray(counts)
    return "clips: {} records, {} eligible, {} clipped reads, {} left and {} right clips, {} distinct sites, {} reported, short clips {}, malformed records {}".format(
        *(int(c[SN_INDEX[k]]) for k in ("records", "eligible", "clipped_reads", "left_clips", "right_clips", "distinct_sites", "reported_sites", "short_clips",
                                        "malformed")))


def main(counter, prefix, coverage_data, names, S, align=None, far=None, ins=None, keep=None, mei=None):
    """the stage behind the scan: the sort, the run lengths and the vote on the device, the file and the summary line.  ``align``:
    None, or (reference, W, K, M) of ``TIDDIT_CLIPS_ALIGN`` — the rows are then realigned where they lie, behind the finish and before
    the counter is closed (tiddit_clip_align.main, which writes ``{o}.clips.align.tab``); ``far``: None, or (reference, K, M) of
    ``TIDDIT_CLIPS_FAR`` — the rows are placed genome-wide the same way (tiddit_clip_far.main, ``{o}.clips.far.tab``); the reference is not
    closed here; ``ins``: None, or (K, O, M) of ``TIDDIT_CLIPS_INS`` — the counter has its extension store (``enable_ext``), and the rows are
    extended, paired and closed where they lie (tiddit_clip_ins.main, ``{o}.clips.ins.tab``); ``keep``: None, or a dict that receives the rows of
    the stages that ran under ``"align"`` / ``"far"`` / ``"ins"`` / ``"mei"`` (``TIDDIT_CLIPS_VCF``, tiddit_clip_vcf.py, joins them behind this stage);
    ``mei``: None, or (library path, A) of ``TIDDIT_CLIPS_MEI`` — behind the INS stage its pair rows are named against the family library
    where they lie (tiddit_clip_mei.main, ``{o}.clips.mei.tab``)"""
    STAGE_SECONDS.clear()
    STAGE_NOTES.clear()
    t = time.time()
    counts = counter.finish(S)
    rows = counter.rows()
    ms = counter.timing()
    asks, grows, cap = counter.reserve_stats()
    min_mapq, min_clip = counter.min_mapq, counter.min_clip
    align_counts = None
    if align is not None:
        from . import tiddit_clip_align
        t_align = time.time()
        try:
            align_counts = tiddit_clip_align.main(counter, rows, align[0], prefix, names, *align[1:], rows_out=None if keep is None else keep.setdefault("align", []))
        except BaseException:
            counter.close()
            raise
        t += time.time() - t_align                              # (its seconds are its own: tiddit_clip_align.STAGE_SECONDS)
    far_counts = None
    if far is not None:
        from . import tiddit_clip_far
        t_far = time.time()
        try:
            far_counts = tiddit_clip_far.main(counter, rows, far[0], prefix, names, *far[1:], rows_out=None if keep is None else keep.setdefault("far", []))
        except BaseException:
            counter.close()
            raise
        t += time.time() - t_far                                # (the same: tiddit_clip_far.STAGE_SECONDS)
    ins_counts = mei_counts = None
    if ins is not None:
        from . import tiddit_clip_ins
        t_ins = time.time()
        try:
            ins_rows = [] if keep is None else keep.setdefault("ins", [])
            ins_counts = tiddit_clip_ins.main(counter, rows, prefix, names, *ins, rows_out=ins_rows)
            if mei is not None:
                from . import tiddit_clip_mei
                mei_counts = tiddit_clip_mei.main(counter, ins_rows, prefix, names, *mei, rows_out=None if keep is None else keep.setdefault("mei", []))
        except BaseException:
            counter.close()
            raise
        t += time.time() - t_ins                                # (the same: tiddit_clip_ins.STAGE_SECONDS, tiddit_clip_mei.STAGE_SECONDS)
    counter.close()
    STAGE_SECONDS["clip sites (device: two sorts, gather, run lengths, site heads, vote, rows)"] = time.time() - t
    for k, v in zip(("sort by K2", "gather of K1", "sort by K1", "run lengths + rows", "site heads + vote + site rows"), ms.tolist()):
        STAGE_SECONDS["  clip " + k + " (device time)"] = v * 1e-3
    STAGE_NOTES.update({"clip store: reserves that asked the device": asks, "clip store: growths": grows, "clip store: capacity (keys)": cap,
                        "clip store: keys": int(counts[SN_INDEX["left_clips"]] + counts[SN_INDEX["right_clips"]])})
    t = time.time()
    write_file(prefix + ".clips.tab", counts, rows, names, coverage_data, S, min_mapq, min_clip)
    STAGE_SECONDS["clip table text (host)"] = time.time() - t
    print(summary_line(counts))
    if align_counts is not None:
        print(tiddit_clip_align.summary_line(align_counts))
    if far_counts is not None:
        print(tiddit_clip_far.summary_line(far_counts))
    if ins_counts is not None:
        print(tiddit_clip_ins.summary_line(ins_counts))
    if mei_counts is not None:
        print(tiddit_clip_mei.summary_line(mei_counts))
    return counts
