"""The reference sequence, resident in HBM (``tdt_refseq_*``, csrc/tdt_refseq.hip): 4-bit base codes, BAM's own, two bases per byte,
every contig on an 8-byte boundary between zero guard bytes.  Packed on the device from the FASTA file's bytes as they are
(``FastaFile.fetch_raw``); what reference-aware kernels of the ``--sv`` scan read — the first is the left-normalisation of
``TIDDIT_INDELS_NORM`` (tiddit_indels.py).  :class:`HostReference` is the same thing as plain Python, for the definitions."""
import ctypes

import numpy

from . import _native

CODES = "=ACMGRSVTWYHKDBN"
_TABLE = numpy.full(256, 15, dtype=numpy.uint8)
for _c in range(1, 16):
    _TABLE[ord(CODES[_c])] = _TABLE[ord(CODES[_c].lower())] = _c


def codes_of_bases(bases):
    """bytes / str / uint8[] of bases -> uint8[] of codes: letters in either case to BAM's code, anything else to 15 (N)"""
    if isinstance(bases, str):
        bases = bases.encode("latin-1")
    return _TABLE[numpy.frombuffer(bytes(bases), dtype=numpy.uint8) if isinstance(bases, (bytes, bytearray)) else numpy.asarray(bases, dtype=numpy.uint8)]


class HostReference:
    """``length(tid)`` (-1: not loaded) and ``code(tid, i)`` over host arrays of codes: {tid: uint8[]}"""

    def __init__(self, contigs):
        self.contigs = {int(t): numpy.asarray(c, dtype=numpy.uint8) for t, c in contigs.items()}

    def length(self, tid):
        c = self.contigs.get(tid)
        return -1 if c is None else len(c)

    def code(self, tid, i):
        return int(self.contigs[tid][i])


class RefSeq:
    """the device handle; ``lengths``: every contig's bases, in the order of the BAM header"""

    def __init__(self, lengths, ctx=None):
        self.ctx = ctx or _native.default_context()
        self.lengths = [int(v) for v in lengths]
        arr = numpy.array(self.lengths, dtype=numpy.int64)
        h = ctypes.c_void_p()
        _native.check(self.ctx.lib.tdt_refseq_create(self.ctx.handle, len(self.lengths), _native.ptr(arr), ctypes.byref(h)))
        self.handle = h
        self.loaded = set()

    def load_fasta(self, tid, raw, length, linebases, linewidth):
        """one contig from the file's bytes (host uint8[]: ``FastaFile.fetch_raw``)"""
        raw = numpy.ascontiguousarray(raw, dtype=numpy.uint8)
        _native.check(self.ctx.lib.tdt_refseq_load_fasta(self.handle, int(tid), _native.ptr(raw), len(raw), int(length), int(linebases), int(linewidth)))
        self.loaded.add(int(tid))

    def load_fasta_device(self, tid, d_raw, nbytes, length, linebases, linewidth):
        """the same on device bytes the caller owns (``d_raw``: a device address)"""
        _native.check(self.ctx.lib.tdt_refseq_load_fasta_device(self.handle, int(tid), ctypes.c_void_p(int(d_raw)), int(nbytes), int(length), int(linebases),
                                                                int(linewidth)))
        self.loaded.add(int(tid))

    def fetch(self, tid, start=0, n=None):
        """-> uint8[n] codes of contig ``tid`` from base ``start`` on"""
        if n is None:
            n = self.lengths[tid] - start
        out = numpy.zeros(max(int(n), 0), dtype=numpy.uint8)
        _native.check(self.ctx.lib.tdt_refseq_fetch(self.handle, int(tid), int(start), int(n), _native.ptr(out)))
        return out

    def layout(self, store=False):
        """-> (bytes of the store, guard bytes, bases per pack workgroup, uint64[] byte offsets of the contigs[, the store as uint8[]])"""
        out3 = numpy.zeros(3, dtype=numpy.uint64)
        offs = numpy.zeros(max(len(self.lengths), 1), dtype=numpy.uint64)
        _native.check(self.ctx.lib.tdt_refseq_layout(self.handle, _native.ptr(out3), _native.ptr(offs), None))
        res = (int(out3[0]), int(out3[1]), int(out3[2]), offs[:len(self.lengths)])
        if store:
            buf = numpy.zeros(res[0], dtype=numpy.uint8)
            _native.check(self.ctx.lib.tdt_refseq_layout(self.handle, _native.ptr(out3), None, _native.ptr(buf)))
            res += (buf,)
        return res

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.tdt_refseq_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check_against_bam(fasta, names, lengths):
    """every contig of the BAM header (``names``, ``lengths``) is in ``fasta`` (a FastaFile) under its name, with that length; else
    ValueError (its text is the error line)"""
    for name, ln in zip(names, lengths):
        if name not in fasta.index:
            raise ValueError("contig %s has %d bases in the BAM header and is missing in the reference FASTA" % (name, ln))
        if fasta.index[name][0] != ln:
            raise ValueError("contig %s has %d bases in the BAM header and %d in the reference FASTA" % (name, ln, fasta.index[name][0]))


def load_all(fasta, ctx=None):
    """Every sequence of ``fasta`` (a FastaFile) in the order of its index, the lengths from the index -> RefSeq (a family library of
    ``TIDDIT_CLIPS_MEI``, say: a handle of its own beside the job's reference)"""
    names = list(fasta.references)
    ref = RefSeq([fasta.index[n][0] for n in names], ctx=ctx)
    try:
        for tid, name in enumerate(names):
            ref.load_fasta(tid, *fasta.fetch_raw(name))
    except Exception:
        ref.close()
        raise
    return ref


def load_for_bam(fasta, names, lengths, ctx=None):
    """The reference of a job: every contig of the BAM header (``names``, ``lengths``) from ``fasta`` (a FastaFile), matched by name ->
    (RefSeq, seconds reading the file, seconds in the loads: upload + pack).  ValueError (:func:`check_against_bam`) before anything is
    allocated."""
    import time
    check_against_bam(fasta, names, lengths)
    ref = RefSeq(lengths, ctx=ctx)
    t_read = t_load = 0.0
    try:
        for tid, name in enumerate(names):
            t = time.time()
            raw, length, linebases, linewidth = fasta.fetch_raw(name)
            t2 = time.time()
            ref.load_fasta(tid, raw, length, linebases, linewidth)
            t_read += t2 - t
            t_load += time.time() - t2
    except Exception:
        ref.close()
        raise
    return ref, t_read, t_load
