"""Read-level QC tables from the ``--sv`` scan (``TIDDIT_QC=1``): flag counts, MAPQ, read lengths, insert sizes, per-cycle base
composition and quality, the quality histogram, GC per read, CIGAR sums and indel lengths — what ``samtools flagstat`` / ``samtools
stats`` take one more pass over the file for — counted on the device from the batches the scan already holds in HBM
(csrc/tdt_qc.hip, two launches per batch), written to ``{o}.qc.tab``.  Nothing in the reference does this; the definition below is
the specification, and :func:`count_read` implements it read by read.

Every counter is a uint64 of ONE array of ``SIZE`` counters; ``LAYOUT`` names its sections (offset, rows, columns) and is the layout of
include/tiddit_hip.h.  The constants ``QC_CYCLES`` 512, ``QC_IS_MAX`` 2000, ``QC_ID_MAX`` 64 are csrc/tdt_qc.hip's.

From the field columns ``flag mapq tid mate_tid tlen l_seq`` of a read (a malformed record changes none of these):

  ``SN``, every record:  ``records``, ``secondary`` (0x100), ``supplementary`` (0x800).
  ``SN``, primary records (``flag & 0x900 == 0``):  ``primary``, ``qc_fail`` (0x200), ``duplicate`` (0x400), ``unmapped`` (0x4), ``mapped``
        (not 0x4), ``paired`` (0x1), ``read1`` (0x40), ``read2`` (0x80), ``proper_pair`` (0x1 and 0x2), ``mate_unmapped`` (0x1 and 0x8),
        ``both_mapped`` (0x1, neither 0x4 nor 0x8), ``mate_other_contig`` (both mapped, ``mate_tid != tid``),
        ``mate_other_contig_mapq5`` (the same with ``mapq >= 5``), ``reverse`` (mapped and 0x10), ``mapq0`` (mapped and ``mapq == 0``).
  ``MAPQ[256]``  mapped primary records by ``mapq``.
  ``S`` is the set of records with ``flag & 0xB00 == 0`` (primary, not QC-failed); every section below is counted over ``S``.
  ``RL[QC_CYCLES + 1]``  by ``min(max(l_seq, 0), QC_CYCLES)`` of the column.
  ``IS[QC_IS_MAX + 1][3]``  paired, both mapped, ``mate_tid == tid``, ``tlen > 0`` (one count per pair: the mate that carries the positive
        length) by ``min(tlen, QC_IS_MAX)``; column ``inward``: 0x10 clear and 0x20 set, ``outward``: 0x10 set and 0x20 clear, ``same``: else.

From the record bytes (the batch's ``raw`` at ``rec_off``: block_size, fixed fields, name, CIGAR, 4-bit sequence, qualities).  The record
is bounded first: ``rec_off + 36 <= raw_len`` (the fixed fields can be read), its own ``l_seq >= 0``,
``32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size`` and ``rec_off + 4 + block_size <= raw_len``.  A record that
fails, or holds a CIGAR op code above 8, is MALFORMED: ``SN malformed`` += 1 and nothing below.  ``l_seq`` below is the record's own.

  ``SN``  ``bases`` += l_seq; ``reads_no_seq`` (l_seq == 0); ``reads_no_qual`` (l_seq > 0 and the first quality byte is 0xff: the read has no
        qualities); for a read with qualities every quality byte q: ``bases_q20`` (q >= 20), ``bases_q30`` (q >= 30).
  ``CYC[QC_CYCLES + 1][7]``  columns ``A C G T other qual_sum qual_n``.  Query index i (even: the high nibble of sequence byte i / 2, odd:
        the low one; the pad nibble of an odd l_seq is no base) has cycle i, or l_seq - 1 - i when 0x10 is set; row ``min(cycle,
        QC_CYCLES)``.  Nibble 1 2 4 8 is A C G T, every other code ``other``; with 0x10 set A <-> T and C <-> G.  A read with qualities
        adds q to ``qual_sum`` and 1 to ``qual_n`` of the row (a 0xff behind the first byte is the value 255).
  ``QUAL[256]``  every quality byte of the reads with qualities.
  ``GCR[101]``  reads with l_seq > 0 by ``(100 * gc) // l_seq``, gc = the bases with nibble 2 or 4.
  mapped reads (not 0x4) with n_cigar_op > 0, per operation of length len:  ``SN aligned_bases`` (M = X), ``soft_clipped_bases`` (S),
        ``hard_clipped_bases`` (H), ``inserted_bases`` (I), ``deleted_bases`` (D), ``skipped_bases`` (N) += len; an I / D with len >= 1 is
        an event: ``insertions`` / ``deletions`` += 1 and ``ID[min(len, QC_ID_MAX) - 1][0 / 1]`` += 1; ``reads_clipped`` += 1 for a read
        with any S or H operation.

``{o}.qc.tab``: ``# tiddit_amd qc v1``, then tab-separated integer rows — ``SN name count`` (every row, always, in the order above),
``MAPQ q n``, ``RL l n``, ``IS tlen inward outward same``, ``CYC cycle A C G T other qual_sum qual_n`` (cycle from 0), ``QUAL q n``,
``GCR percent n``, ``ID len insertions deletions`` (len from 1) — a row of these only when one of its counts is non-zero.

N ranks.  Every record is decoded by exactly one rank, so the counters add: they are SUM-reduced to rank 0 over the job's process group
(tiddit_alleles.reduce_to_rank0), and rank 0 writes the file the one-process job writes.
"""
import ctypes
import struct
import time

import numpy

from . import _native, bamio

QC_CYCLES, QC_IS_MAX, QC_ID_MAX = 512, 2000, 64
SN = ("records", "secondary", "supplementary", "primary", "qc_fail", "duplicate", "unmapped", "mapped", "paired", "read1", "read2", "proper_pair",
      "mate_unmapped", "both_mapped", "mate_other_contig", "mate_other_contig_mapq5", "reverse", "mapq0", "malformed", "bases", "reads_no_seq",
      "reads_no_qual", "bases_q20", "bases_q30", "aligned_bases", "soft_clipped_bases", "hard_clipped_bases", "inserted_bases", "deleted_bases",
      "skipped_bases", "insertions", "deletions", "reads_clipped")
SN_INDEX = {k: i for i, k in enumerate(SN)}
IS_COLUMNS = ("inward", "outward", "same")
CYC_COLUMNS = ("A", "C", "G", "T", "other", "qual_sum", "qual_n")
# section -> (offset, rows, columns)
LAYOUT = {"SN": (0, 33, 1), "MAPQ": (33, 256, 1), "RL": (289, QC_CYCLES + 1, 1), "IS": (802, QC_IS_MAX + 1, 3), "CYC": (6805, QC_CYCLES + 1, 7),
          "QUAL": (10396, 256, 1), "GCR": (10652, 101, 1), "ID": (10753, QC_ID_MAX, 2)}
SIZE = 10881
HEADER = "# tiddit_amd qc v1\n"
STAGE_SECONDS = {}
_O = {k: v[0] for k, v in LAYOUT.items()}
_BASE_COL = {1: 0, 2: 1, 4: 2, 8: 3}
_OP_SN = {0: "aligned_bases", 7: "aligned_bases", 8: "aligned_bases", 1: "inserted_bases", 2: "deleted_bases", 3: "skipped_bases",
          4: "soft_clipped_bases", 5: "hard_clipped_bases"}


def parse_switch(value):
    """``TIDDIT_QC`` -> False (unset or empty) or True (``1``); ValueError (its text is the error line) for anything else"""
    if value is None or value == "":
        return False
    if value == "1":
        return True
    raise ValueError("the switch is 1 or unset")


def section(counts, name):
    """the section's view of the counter array, [rows][columns]"""
    o, r, c = LAYOUT[name]
    return counts[o:o + r * c].reshape(r, c)


# ------------------------------------------------------------------------------------------- the definition
def count_read(c, flag, mapq, tid, mate_tid, tlen, l_seq, rec_off, raw):
    """THE DEFINITION, one read: adds to ``c`` (SIZE uint64-like counters).  ``raw`` is the batch's record bytes (bytes-like), the other
    arguments the read's entries of the batch's columns."""
    def sn(k, v=1):
        c[SN_INDEX[k]] += v
    sn("records")
    if flag & 0x100:
        sn("secondary")
    if flag & 0x800:
        sn("supplementary")
    if flag & 0x900 == 0:
        sn("primary")
        mapped = not flag & 0x4
        both = bool(flag & 0x1) and not flag & 0xC
        for k, on in (("qc_fail", flag & 0x200), ("duplicate", flag & 0x400), ("unmapped", flag & 0x4), ("mapped", mapped), ("paired", flag & 0x1),
                      ("read1", flag & 0x40), ("read2", flag & 0x80), ("proper_pair", flag & 0x3 == 0x3), ("mate_unmapped", flag & 0x9 == 0x9),
                      ("both_mapped", both), ("mate_other_contig", both and mate_tid != tid),
                      ("mate_other_contig_mapq5", both and mate_tid != tid and mapq >= 5), ("reverse", mapped and flag & 0x10),
                      ("mapq0", mapped and mapq == 0)):
            if on:
                sn(k)
        if mapped:
            c[_O["MAPQ"] + mapq] += 1
    if flag & 0xB00:
        return
    c[_O["RL"] + min(max(l_seq, 0), QC_CYCLES)] += 1
    if flag & 0x1 and not flag & 0xC and mate_tid == tid and tlen > 0:
        col = 0 if (not flag & 0x10 and flag & 0x20) else 1 if (flag & 0x10 and not flag & 0x20) else 2
        c[_O["IS"] + 3 * min(tlen, QC_IS_MAX) + col] += 1
    # ---- the record's bytes
    raw_len = len(raw)
    if rec_off + 36 > raw_len:
        sn("malformed")
        return
    block_size, = struct.unpack_from("<I", raw, rec_off)
    r0 = rec_off + 4
    l_name = raw[r0 + 8]
    n_cig, = struct.unpack_from("<H", raw, r0 + 12)
    L, = struct.unpack_from("<i", raw, r0 + 16)
    if L < 0 or 32 + l_name + 4 * n_cig + (L + 1) // 2 + L > block_size or rec_off + 4 + block_size > raw_len:
        sn("malformed")
        return
    cig = r0 + 32 + l_name
    seq = cig + 4 * n_cig
    qual = seq + (L + 1) // 2
    ops = [struct.unpack_from("<I", raw, cig + 4 * j)[0] for j in range(n_cig)]
    if any((w & 0xf) > 8 for w in ops):
        sn("malformed")
        return
    sn("bases", L)
    if L == 0:
        sn("reads_no_seq")
    has_q = L > 0 and raw[qual] != 0xff
    if L > 0 and not has_q:
        sn("reads_no_qual")
    rev = bool(flag & 0x10)
    gc = 0
    for i in range(L):
        byte = raw[seq + (i >> 1)]
        nib = (byte & 0xf) if i & 1 else (byte >> 4)
        if nib == 2 or nib == 4:
            gc += 1
        col = _BASE_COL.get(nib, 4)
        if rev and col < 4:
            col = 3 - col
        row = _O["CYC"] + 7 * min(L - 1 - i if rev else i, QC_CYCLES)
        c[row + col] += 1
        if has_q:
            q = raw[qual + i]
            c[row + 5] += q
            c[row + 6] += 1
            c[_O["QUAL"] + q] += 1
            if q >= 20:
                sn("bases_q20")
            if q >= 30:
                sn("bases_q30")
    if L > 0:
        c[_O["GCR"] + (100 * gc) // L] += 1
    if not flag & 0x4 and n_cig:
        for w in ops:
            op, ln = w & 0xf, w >> 4
            if op in _OP_SN:
                sn(_OP_SN[op], ln)
            if op in (1, 2) and ln >= 1:
                sn("insertions" if op == 1 else "deletions")
                c[_O["ID"] + 2 * (min(ln, QC_ID_MAX) - 1) + (op == 2)] += 1
        if any((w & 0xf) in (4, 5) for w in ops):
            sn("reads_clipped")


def count_batch(c, b):
    """the definition over one batch (an object with the columns ``flag mapq tid mate_tid tlen l_seq rec_off`` and ``raw``)"""
    raw = b.raw if isinstance(b.raw, (bytes, bytearray)) else memoryview(numpy.ascontiguousarray(b.raw))
    for i in range(len(b.tid)):
        count_read(c, int(b.flag[i]), int(b.mapq[i]), int(b.tid[i]), int(b.mate_tid[i]), int(b.tlen[i]), int(b.l_seq[i]), int(b.rec_off[i]), raw)


def _within(counts):
    """[0 .. counts[0]), [0 .. counts[1]), ... in one array, and the owner of every entry"""
    owner = numpy.repeat(numpy.arange(len(counts)), counts)
    start = numpy.cumsum(counts) - counts
    return numpy.arange(int(counts.sum()), dtype=numpy.int64) - start[owner], owner


def count_batch_columns(c, b, chunk_bases=1 << 22):
    """The same rules over one batch on whole columns (numpy) — for files too large for the per-base loop of :func:`count_read`, to
    which tests/test_qc_refs_cpu.py pins it on every aimed case.  ``c``: int64[SIZE]."""
    f, q = numpy.asarray(b.flag).astype(numpy.int64), numpy.asarray(b.mapq).astype(numpy.int64)
    tid, mtid, tlen, lcol = (numpy.asarray(getattr(b, k)).astype(numpy.int64) for k in ("tid", "mate_tid", "tlen", "l_seq"))
    raw = numpy.frombuffer(b.raw, dtype=numpy.uint8) if isinstance(b.raw, (bytes, bytearray)) else numpy.ascontiguousarray(b.raw, dtype=numpy.uint8)

    def sn(k, mask):
        c[SN_INDEX[k]] += int(numpy.sum(mask))
    prim = (f & 0x900) == 0
    mapped, paired = prim & ((f & 0x4) == 0), prim & ((f & 0x1) != 0)
    both = paired & ((f & 0xC) == 0)
    other = both & (mtid != tid)
    for k, m in (("records", numpy.ones(len(f), dtype=bool)), ("secondary", (f & 0x100) != 0), ("supplementary", (f & 0x800) != 0), ("primary", prim),
                 ("qc_fail", prim & ((f & 0x200) != 0)), ("duplicate", prim & ((f & 0x400) != 0)), ("unmapped", prim & ((f & 0x4) != 0)), ("mapped", mapped),
                 ("paired", paired), ("read1", prim & ((f & 0x40) != 0)), ("read2", prim & ((f & 0x80) != 0)), ("proper_pair", paired & ((f & 0x2) != 0)),
                 ("mate_unmapped", paired & ((f & 0x8) != 0)), ("both_mapped", both), ("mate_other_contig", other),
                 ("mate_other_contig_mapq5", other & (q >= 5)), ("reverse", mapped & ((f & 0x10) != 0)), ("mapq0", mapped & (q == 0))):
        sn(k, m)
    c[_O["MAPQ"]:_O["MAPQ"] + 256] += numpy.bincount(q[mapped], minlength=256)
    S = (f & 0xB00) == 0
    c[_O["RL"]:_O["RL"] + QC_CYCLES + 1] += numpy.bincount(numpy.clip(lcol[S], 0, QC_CYCLES), minlength=QC_CYCLES + 1)
    pair = S & ((f & 0x1) != 0) & ((f & 0xC) == 0) & (mtid == tid) & (tlen > 0)
    col = numpy.where(((f & 0x10) == 0) & ((f & 0x20) != 0), 0, numpy.where(((f & 0x10) != 0) & ((f & 0x20) == 0), 1, 2))
    c[_O["IS"]:_O["CYC"]] += numpy.bincount(3 * numpy.minimum(tlen[pair], QC_IS_MAX) + col[pair], minlength=3 * (QC_IS_MAX + 1))
    # ---- the records of S: headers, bounds, op codes
    ro = numpy.asarray(b.rec_off).astype(numpy.int64)[S]
    fS = f[S]
    raw_len = len(raw)
    head = ro + 36 <= raw_len
    sn("malformed", ~head)
    ro, fS = ro[head], fS[head]
    u = lambda o, n: sum(raw[ro + o + k].astype(numpy.int64) << (8 * k) for k in range(n))
    bs, l_name, n_cig, L = u(0, 4), u(12, 1), u(16, 2), u(20, 4)
    L = numpy.where(L >= 1 << 31, L - (1 << 32), L)
    ok = (L >= 0) & (32 + l_name + 4 * n_cig + (L + 1) // 2 + L <= bs) & (ro + 4 + bs <= raw_len)
    sn("malformed", ~ok)
    ro, fS, l_name, n_cig, L = ro[ok], fS[ok], l_name[ok], n_cig[ok], L[ok]
    cig = ro + 36 + l_name
    j, owner = _within(n_cig)
    at = cig[owner] + 4 * j
    words = sum(raw[at + k].astype(numpy.int64) << (8 * k) for k in range(4))
    code, ln = words & 0xf, words >> 4
    badop = numpy.bincount(owner[code > 8], minlength=len(ro)) > 0
    sn("malformed", badop)
    good = ~badop
    use = good[owner] & ((fS[owner] & 0x4) == 0)                  # the operations of the mapped, well-formed reads
    code, ln, owner = code[use], ln[use], owner[use]
    for k, ops in (("aligned_bases", (0, 7, 8)), ("soft_clipped_bases", (4,)), ("hard_clipped_bases", (5,)), ("inserted_bases", (1,)),
                   ("deleted_bases", (2,)), ("skipped_bases", (3,))):
        c[SN_INDEX[k]] += int(ln[numpy.isin(code, ops)].sum())
    for k, (name, op) in enumerate((("insertions", 1), ("deletions", 2))):
        ev = ln[(code == op) & (ln >= 1)]
        c[SN_INDEX[name]] += len(ev)
        c[_O["ID"]:_O["ID"] + 2 * QC_ID_MAX] += numpy.bincount(2 * (numpy.minimum(ev, QC_ID_MAX) - 1) + k, minlength=2 * QC_ID_MAX)
    c[SN_INDEX["reads_clipped"]] += len(numpy.unique(owner[numpy.isin(code, (4, 5))]))
    # ---- their bases, chunk_bases at a time
    seq = (cig + 4 * n_cig)[good]
    L, rev = L[good], (fS[good] & 0x10) != 0
    qual = seq + (L + 1) // 2
    c[SN_INDEX["bases"]] += int(L.sum())
    sn("reads_no_seq", L == 0)
    has_q = numpy.zeros(len(L), dtype=bool)
    has_q[L > 0] = raw[qual[L > 0]] != 0xff
    sn("reads_no_qual", (L > 0) & ~has_q)
    base_col = numpy.full(16, 4, dtype=numpy.uint8)
    base_col[[1, 2, 4, 8]] = [0, 1, 2, 3]
    complement = numpy.array([3, 2, 1, 0, 4], dtype=numpy.uint8)
    cyc = c[_O["CYC"]:_O["CYC"] + 7 * (QC_CYCLES + 1)].reshape(QC_CYCLES + 1, 7)          # (a view: adds land in c)
    for Lv in numpy.unique(L[L > 0]).tolist():                     # reads of one length are one 2-D block, a column of it one cycle
        same = numpy.flatnonzero(L == Lv)
        step = max(1, chunk_bases // Lv)
        half, head = (Lv + 1) // 2, min(Lv, QC_CYCLES)
        for lo in range(0, len(same), step):
            rows = same[lo:lo + step]
            sb = raw[seq[rows][:, None] + numpy.arange(half)]
            nib = numpy.empty((len(rows), 2 * half), dtype=numpy.uint8)
            nib[:, 0::2], nib[:, 1::2] = sb >> 4, sb & 0xf
            nib = nib[:, :Lv]                                      # (the pad nibble of an odd length is no base)
            gc = ((nib == 2) | (nib == 4)).sum(axis=1, dtype=numpy.int64)
            c[_O["GCR"]:_O["GCR"] + 101] += numpy.bincount((100 * gc) // Lv, minlength=101)
            col, rv = base_col[nib], rev[rows]
            col[rv] = complement[col[rv]][:, ::-1]
            for k in range(5):
                hit = col == k
                cyc[:head, k] += hit[:, :head].sum(axis=0, dtype=numpy.int64)
                cyc[QC_CYCLES, k] += int(hit[:, head:].sum())
            hq = has_q[rows]
            qa = raw[qual[rows][hq][:, None] + numpy.arange(Lv)]
            qa[rv[hq]] = qa[rv[hq]][:, ::-1]
            cyc[:head, 5] += qa[:, :head].sum(axis=0, dtype=numpy.int64)
            cyc[:head, 6] += len(qa)
            cyc[QC_CYCLES, 5] += int(qa[:, head:].sum(dtype=numpy.int64))
            cyc[QC_CYCLES, 6] += len(qa) * (Lv - head)
            c[_O["QUAL"]:_O["QUAL"] + 256] += numpy.bincount(qa.reshape(-1), minlength=256)
            c[SN_INDEX["bases_q20"]] += int((qa >= 20).sum())
            c[SN_INDEX["bases_q30"]] += int((qa >= 30).sum())


# ------------------------------------------------------------------------------------------- the device handle
class QcCounter:
    """``tdt_qc_*``: the counter array in HBM; one push per batch of the scan."""

    def __init__(self, ctx=None):
        self.ctx = ctx or _native.default_context()
        assert self.ctx.lib.tdt_qc_size() == SIZE
        h = ctypes.c_void_p()
        _native.check(self.ctx.lib.tdt_qc_create(self.ctx.handle, ctypes.byref(h)))
        self.handle = h

    def push_device_batch(self, b):
        """one DeviceBatch: enqueued on the reader's stream, nothing waited for (call before the batch's buffers are handed on)"""
        _native.check(self.ctx.lib.tdt_qc_push_device(self.handle, b.pointer_table(), len(b), b._raw_len))

    def push_host_batch(self, b):
        """one host-decoded batch (or any object with its columns): uploaded, then the same kernels"""
        cols, raw = bamio.host_columns(b, ("flag", "mapq", "tid", "mate_tid", "tlen", "l_seq", "rec_off"))      # (the arguments of tdt_qc_push, in order)
        _native.check(self.ctx.lib.tdt_qc_push(self.handle, *[_native.ptr(c) for c in cols], len(cols[0]), _native.ptr(raw), len(raw)))

    def counts(self):
        """-> uint64[SIZE], behind everything pushed so far"""
        out = numpy.zeros(SIZE, dtype=numpy.uint64)
        _native.check(self.ctx.lib.tdt_qc_counts(self.handle, _native.ptr(out)))
        return out

    def reset(self):
        _native.check(self.ctx.lib.tdt_qc_reset(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.tdt_qc_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------- the file
def write_file(path, counts):
    """``{o}.qc.tab`` (see the module docstring)"""
    c = [int(v) for v in numpy.asarray(counts).tolist()]
    out = [HEADER]
    out += ["SN\t%s\t%d\n" % (k, c[i]) for i, k in enumerate(SN)]
    for name, first in (("MAPQ", 0), ("RL", 0), ("IS", 0), ("CYC", 0), ("QUAL", 0), ("GCR", 0), ("ID", 1)):
        o, rows, cols = LAYOUT[name]
        for r in range(rows):
            v = c[o + r * cols:o + (r + 1) * cols]
            if any(v):
                out.append("%s\t%d\t%s\n" % (name, r + first, "\t".join(map(str, v))))
    with open(path, "w") as f:
        f.write("".join(out))


def summary_line(counts):
    c = numpy.asarray(counts)
    return "qc tables: {} records, {} primary, {} mapped, {} bases, malformed records {}".format(
        *(int(c[SN_INDEX[k]]) for k in ("records", "primary", "mapped", "bases", "malformed")))


def reduce_to_rank0(counts, group=None):
    """the N-rank job: SUM of every rank's counters on rank 0 through the allele counters' helper (int64 on the wire: exact below
    2^63).  -> uint64[SIZE] on rank 0, None elsewhere."""
    from . import tiddit_alleles
    wire = numpy.zeros((SIZE + 7) // 8 * 8, dtype=numpy.int64)
    wire[:SIZE] = counts.astype(numpy.int64)
    got = tiddit_alleles.reduce_to_rank0(wire.reshape(-1, 8), 0, 0, group)
    return None if got is None else got[0].reshape(-1)[:SIZE].astype(numpy.uint64)


def main(counter, prefix, multi=False, rank=0):
    """the stage behind the scan: the counters off the device, on N ranks summed on rank 0, the file and the summary line"""
    STAGE_SECONDS.clear()
    t = time.time()
    counts = counter.counts()
    counter.close()
    STAGE_SECONDS["qc counters to the host"] = time.time() - t
    if multi:
        t = time.time()
        counts = reduce_to_rank0(counts)
        STAGE_SECONDS["qc counters summed on rank 0"] = time.time() - t
        if counts is None:
            return None
    if rank == 0:
        t = time.time()
        write_file(prefix + ".qc.tab", counts)
        STAGE_SECONDS["qc table text (host)"] = time.time() - t
        print(summary_line(counts))
    return counts
