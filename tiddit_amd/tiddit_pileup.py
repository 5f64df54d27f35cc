"""Exact per-base depth from the ``--sv`` scan: for every reference position the number of eligible reads with an ALIGNED base there,
CIGAR-exact — a deletion or a skip covers nothing — from the batches the scan already holds in HBM (csrc/tdt_pileup.hip: one launch per
batch adds +1 / -1 at the ends of every read's aligned spans, one prefix sum per job).  It is what ``TIDDIT_SMALL_VCF`` genotypes the
rows of ``TIDDIT_SNVS`` / ``TIDDIT_INDELS`` against (tiddit_small_vcf.py), because a candidate's position is known only at the finish,
when the reads are gone.  Nothing in the reference does this.  The definition below is the specification: :func:`spans_of_read` read by
read, :func:`depth_of` over the whole job.

Per record, from the batch's columns ``flag tid pos mapq rec_off`` and the record's bytes (``raw`` at ``rec_off``), with ``Q`` the
minimum MAPQ and ``lengths`` the contigs' lengths in the order of the BAM header:

  1. ``SN records`` += 1.  The record is ELIGIBLE by exactly step 1 of tiddit_snvs.py: ``flag & 0xF04 == 0``, ``tid >= 0`` and
        ``mapq >= Q``: ``SN eligible`` += 1.  Nothing else is done for the others, and their bytes are never read.
  2. The record is bounded, and found MALFORMED, exactly as in step 2 of tiddit_snvs.py (the bound, an op code above 8, ``tid >= 2^24``,
        ``pos < 0``, ``pos`` plus the reference length above ``2^31 - 1``, a query length that differs from ``l_seq`` where both are
        given); it is also malformed when ``tid >= len(lengths)``.  A malformed record adds 1 to ``SN malformed`` and nothing else.
        Nothing outside ``[raw, raw + raw_len)`` is ever read.
  3. ``n_cigar_op == 0``: ``SN no_cigar`` += 1 and nothing else.  (A record with ``l_seq == 0`` but a CIGAR does count: it has aligned
        positions.)
  4. One walk, ``r = pos``: ``M = X`` (0, 7, 8) cover ``[r, r + len)`` and advance ``r``; ``D N`` (2, 3) advance ``r`` and cover nothing;
        ``I S H P`` (1, 4, 5, 6) do nothing to ``r``.  Covered stretches that touch on the reference are ONE span (``10M2I10M`` gives
        ``[pos, pos + 20)``); operations of length 0 change nothing.  Every span is clamped to ``[0, lengths[tid]]``; a span that is
        empty after that is dropped, and ``SN clamped_spans`` += 1 for each span cut or dropped.  ``SN spans`` += the spans kept,
        ``SN covered_bases`` += their total length.  There is no cap on the spans of a read.
  5. :func:`depth_of`: ``depth[t][i]`` is the number of kept spans of contig ``t`` that hold ``i``, a ``uint32``.

Base quality plays no part: a low-quality base is a read with a base there.

The device keeps one ``int32`` per reference base plus a guard slot per contig — 4 B per base, 12.4 GB for a 3.1-Gb genome.

NOT built: base-quality-aware counts, a depth track or a gVCF written from the array, N ranks, long-read libraries (unmeasured).
"""
import ctypes
import struct

import numpy

from . import _native, bamio
from .bamio import _raw_of

PILE_MAX_CONTIGS = 1 << 24
END_LIMIT = (1 << 31) - 1
DEFAULT_MAPQ = 20
SN = ("records", "eligible", "malformed", "no_cigar", "spans", "covered_bases", "clamped_spans")
SN_INDEX = {k: i for i, k in enumerate(SN)}
SIZE = len(SN)
GENOTYPE_COLUMNS = ("DP0", "OTHER", "PL0", "PL1", "PL2", "GT", "GQ", "ABOVE")
# what spans_of_read says about a record
NOT_ELIGIBLE, MALFORMED, NO_CIGAR, OK = "not_eligible", "malformed", "no_cigar", "ok"


# ------------------------------------------------------------------------------------------- the definition
def _spans_of_read(flag, tid, pos, mapq, rec_off, raw, lengths, min_mapq):
    """-> (kind, kept spans, spans cut or dropped)"""
    if flag & 0xF04 or tid < 0 or mapq < min_mapq:
        return NOT_ELIGIBLE, [], 0
    bad = (MALFORMED, [], 0)
    raw_len = len(raw)
    if tid >= PILE_MAX_CONTIGS or tid >= len(lengths) or pos < 0 or rec_off + 36 > raw_len:
        return bad
    block_size, = struct.unpack_from("<I", raw, rec_off)
    r0 = rec_off + 4
    l_name = raw[r0 + 8]
    n_cig, = struct.unpack_from("<H", raw, r0 + 12)
    L, = struct.unpack_from("<i", raw, r0 + 16)
    if L < 0 or 32 + l_name + 4 * n_cig + (L + 1) // 2 + L > block_size or rec_off + 4 + block_size > raw_len:
        return bad
    words = struct.unpack_from("<%dI" % n_cig, raw, r0 + 32 + l_name)
    if any((w & 0xf) > 8 for w in words):
        return bad
    ref_len = sum(w >> 4 for w in words if (w & 0xf) in (0, 2, 3, 7, 8))
    query_len = sum(w >> 4 for w in words if (w & 0xf) in (0, 1, 4, 7, 8))
    if pos + ref_len > END_LIMIT or (L >= 1 and n_cig >= 1 and query_len != L):
        return bad
    if n_cig == 0:
        return NO_CIGAR, [], 0
    r = pos
    merged = []
    for w in words:
        op, ln = w & 0xf, w >> 4
        if ln == 0:
            continue
        if op in (0, 7, 8):
            if merged and merged[-1][1] == r:
                merged[-1][1] = r + ln
            else:
                merged.append([r, r + ln])
            r += ln
        elif op in (2, 3):
            r += ln
    length = int(lengths[tid])
    spans, clamped = [], 0
    for s, e in merged:
        cs, ce = min(max(s, 0), length), min(max(e, 0), length)
        clamped += (cs, ce) != (s, e)
        if cs < ce:
            spans.append((cs, ce))
    return OK, spans, clamped


def spans_of_read(flag, tid, pos, mapq, rec_off, raw, lengths, min_mapq=DEFAULT_MAPQ):
    """THE DEFINITION, one read -> (kind, spans): ``spans`` the read's kept ``[(start, end)]`` on contig ``tid``, half open and 0-based,
    when kind is OK, else [].  ``raw``: the batch's record bytes (bytes-like), ``lengths``: every contig's length, the other arguments the
    read's entries of the batch's columns."""
    return _spans_of_read(flag, tid, pos, mapq, rec_off, raw, lengths, min_mapq)[:2]


def spans_of_batch(b, spans, sn, lengths, min_mapq=DEFAULT_MAPQ):
    """the definition over one batch, read by read: appends (tid, start, end) to ``spans`` and adds to the counters ``sn`` (a dict)"""
    raw = _raw_of(b)
    add = lambda k, n: sn.__setitem__(k, sn.get(k, 0) + n) if n else None
    for i in range(len(b.tid)):
        tid = int(b.tid[i])
        kind, sp, clamped = _spans_of_read(int(b.flag[i]), tid, int(b.pos[i]), int(b.mapq[i]), int(b.rec_off[i]), raw, lengths, min_mapq)
        add("records", 1)
        if kind == NOT_ELIGIBLE:
            continue
        add("eligible", 1)
        add("malformed", int(kind == MALFORMED))
        add("no_cigar", int(kind == NO_CIGAR))
        add("spans", len(sp))
        add("covered_bases", sum(e - s for s, e in sp))
        add("clamped_spans", clamped)
        spans.extend((tid, s, e) for s, e in sp)


def depth_of(spans, lengths):
    """THE DEFINITION, the whole job: ``spans`` = every kept (tid, start, end) in any order -> [uint32[length] per contig]"""
    depth = [numpy.zeros(int(n), dtype=numpy.uint32) for n in lengths]
    for tid, s, e in spans:
        depth[tid][s:e] += 1
    return depth


def counters_of(sn):
    """the counters' dict as uint64[SIZE]"""
    c = numpy.zeros(SIZE, dtype=numpy.uint64)
    for k, v in (sn or {}).items():
        c[SN_INDEX[k]] = v
    return c


# ------------------------------------------------------------------------------------------- the device handle
class PileupDepth:
    """``tdt_pile_*``: the difference array and the counters in HBM; one push per batch of the scan, one finish per job, then the depth
    read-out and the genotype gather."""

    def __init__(self, lengths, min_mapq=DEFAULT_MAPQ, ctx=None):
        self.ctx = ctx or _native.default_context()
        assert self.ctx.lib.tdt_pile_sn_size() == SIZE
        self.lengths = [int(v) for v in lengths]
        self.min_mapq = int(min_mapq)
        arr = numpy.array(self.lengths, dtype=numpy.int64)
        h = ctypes.c_void_p()
        _native.check(self.ctx.lib.tdt_pile_create(self.ctx.handle, len(self.lengths), _native.ptr(arr), self.min_mapq, ctypes.byref(h)))
        self.handle = h

    @property
    def array_bytes(self):
        return 4 * (sum(self.lengths) + len(self.lengths))

    def push_device_batch(self, b):
        """one DeviceBatch: enqueued on the reader's stream, nothing is waited for (call before the batch's buffers are handed on)"""
        _native.check(self.ctx.lib.tdt_pile_push_device(self.handle, b.pointer_table(), len(b), b._raw_len))

    def push_host_batch(self, b):
        """one host-decoded batch (or any object with its columns): uploaded, then the same kernel"""
        cols, raw = bamio.host_columns(b, ("flag", "tid", "pos", "mapq", "rec_off"))
        _native.check(self.ctx.lib.tdt_pile_push(self.handle, *[_native.ptr(c) for c in cols], len(cols[0]), _native.ptr(raw), len(raw)))

    def counters(self):
        """-> uint64[SIZE]: ``SN`` of everything pushed so far"""
        out = numpy.zeros(SIZE, dtype=numpy.uint64)
        _native.check(self.ctx.lib.tdt_pile_counters(self.handle, _native.ptr(out)))
        return out

    def finish(self):
        """the differences become depths (three launches); -> the counters"""
        _native.check(self.ctx.lib.tdt_pile_finish(self.handle))
        return self.counters()

    def depth(self, tid, start=0, n=None):
        """-> uint32[n]: the depths of contig ``tid`` from base ``start`` on (behind :meth:`finish`)"""
        if n is None:
            n = self.lengths[tid] - start
        out = numpy.zeros(max(int(n), 0), dtype=numpy.uint32)
        _native.check(self.ctx.lib.tdt_pile_depth(self.handle, int(tid), int(start), int(n), _native.ptr(out)))
        return out

    def genotype(self, rows):
        """rows: (K1 uint64[], ..., SUPPORT uint32[], ...) as a counter's ``rows()`` gives them, or (K1[], SUPPORT[]) -> uint32[n][8]:
        ``GENOTYPE_COLUMNS`` of tiddit_small_vcf.genotype, one launch"""
        k1 = numpy.ascontiguousarray(rows[0], dtype=numpy.uint64)
        sup = numpy.ascontiguousarray(rows[2] if len(rows) == 4 else rows[1], dtype=numpy.uint32)
        out = numpy.zeros((len(k1), 8), dtype=numpy.uint32)
        _native.check(self.ctx.lib.tdt_pile_genotype(self.handle, _native.ptr(k1), _native.ptr(sup), len(k1), _native.ptr(out)))
        return out

    def timing(self):
        """device ms: [tile sums, carry, scan + write] of the last finish, [the last genotype launch]"""
        out = numpy.zeros(4, dtype=numpy.float64)
        _native.check(self.ctx.lib.tdt_pile_timing(self.handle, _native.ptr(out)))
        return out

    def reset(self):
        _native.check(self.ctx.lib.tdt_pile_reset(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.tdt_pile_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
