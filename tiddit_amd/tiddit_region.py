"""Regional evidence counts for SV candidates on the MI355X — the hot loop of ``tiddit_variant.get_region``
(tiddit_variant.pyx:54-151).  The reference re-opens the BAM region of every candidate through pysam; here a
contig's decoded records are kept as packed arrays (:class:`ReadTable`) and all candidates of the contig are
answered by one kernel launch, one wavefront per candidate (csrc/tdt_region.hip).

``get_region(table, chr, start, end, bp, min_q, max_ins)`` returns the reference's 6-tuple
``(coverage, frac_low_q, n_discs, n_splits, crossing_f, crossing_r)``; ``region_counts`` is the batch form.
"""
import numpy

from . import _native
from .bamio import open_bam

_FIELDS = (("start", "pos", numpy.int32), ("end", "end", numpy.int32), ("mapq", "mapq", numpy.uint8), ("flag", "flag", numpy.uint16),
           ("mate_tid", "mate_tid", numpy.int32), ("mate_pos", "mate_pos", numpy.int32), ("tlen", "tlen", numpy.int32))


class ReadTable:
    """Per-contig packed alignment records of a coordinate-sorted BAM (what a region fetch iterates over)."""

    def __init__(self, bam_file_name):
        reader = open_bam(bam_file_name)
        self.references, self.lengths = reader.references, reader.lengths
        self.tid = {n: i for i, n in enumerate(self.references)}
        parts = {i: {k: [] for k, _, _ in _FIELDS} for i in range(len(self.references))}
        for i in parts:
            parts[i]["has_sa"] = []
        for b in reader.batches():
            edges = numpy.flatnonzero(numpy.diff(b.tid)) + 1
            for lo, hi in zip(numpy.concatenate([[0], edges]), numpy.concatenate([edges, [len(b)]])):
                t = int(b.tid[lo])
                if t < 0:
                    continue
                for k, src, _ in _FIELDS:
                    parts[t][k].append(getattr(b, src)[lo:hi])
                parts[t]["has_sa"].append((b.sa_off[lo:hi] >= 0).astype(numpy.uint8))
        reader.close()
        self.contigs = {}
        for t, d in parts.items():
            self.contigs[t] = {k: (numpy.concatenate(v) if v else numpy.zeros(0, dtype=dt))
                               for (k, _, dt), v in zip(_FIELDS, (d[k] for k, _, _ in _FIELDS))}
            self.contigs[t]["has_sa"] = numpy.concatenate(d["has_sa"]) if d["has_sa"] else numpy.zeros(0, dtype=numpy.uint8)


def _resident(table, t, ctx):
    """the contig's arrays in HBM (uploaded on first use, kept for the life of the table) -> (dict of tensors, max read span)"""
    import torch
    cache = table.__dict__.setdefault("_device", {})
    if t not in cache:
        a = table.contigs[t]
        dev = torch.device("cuda", ctx.device)
        ten = {k: torch.from_numpy(v.view(numpy.int16) if v.dtype == numpy.uint16 else v).to(dev) for k, v in a.items()}
        if len(a["start"]) and numpy.any(numpy.diff(a["start"]) < 0):
            raise ValueError("tiddit_region: reads of %s are not coordinate sorted" % table.references[t])
        span = int((a["end"].astype(numpy.int64) - a["start"]).max()) if len(a["start"]) else 1
        torch.cuda.synchronize(dev)
        cache[t] = (ten, max(1, span))
    return cache[t]


def region_counts(table, chrom, starts, ends, bps, min_q, max_ins, ctx=None):
    """-> int64[nq, 7]: bases, n_reads, low_q, n_discs, n_splits, crossing_f, crossing_r for every (start, end, bp).
    The contig's reads stay resident on the device between calls; only the candidates travel."""
    import torch
    ctx = ctx or _native.default_context()
    t = table.tid[chrom]
    ten, span = _resident(table, t, ctx)
    dev = ten["start"].device
    nq = len(starts)
    q = torch.from_numpy(numpy.ascontiguousarray(numpy.stack([numpy.asarray(starts), numpy.asarray(ends), numpy.asarray(bps)]), dtype=numpy.int32)).to(dev)
    out = torch.empty((nq, 7), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)                       # torch's copies run on its stream, the library on its own
    n = int(ten["start"].numel())
    _native.check(ctx.lib.tdt_region_counts_device(ctx.handle, ten["start"].data_ptr(), ten["end"].data_ptr(), ten["mapq"].data_ptr(),
                                                   ten["flag"].data_ptr(), ten["mate_tid"].data_ptr(), ten["mate_pos"].data_ptr(),
                                                   ten["tlen"].data_ptr(), ten["has_sa"].data_ptr(), n, t, span, table.lengths[t],
                                                   q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), nq, int(min_q), int(max_ins),
                                                   out.data_ptr()))
    ctx.sync()
    return out.cpu().numpy()


def get_region(table, chrom, start, end, bp, min_q, max_ins, contig_number=None):
    """One candidate, the reference's return value (tiddit_variant.pyx:141-151)."""
    bases, n_reads, low_q, n_discs, n_splits, crossing_f, crossing_r = (int(v) for v in region_counts(table, chrom, [start], [end], [bp],
                                                                                                     min_q, max_ins)[0])
    coverage = bases / (end - start + 1)
    frac_low_q = low_q / float(n_reads) if n_reads > 0 else 0
    return (coverage, frac_low_q, n_discs, n_splits, crossing_f, crossing_r)


# ------------------------------------------------------------------------------------------------------------------
# Region means of the coverage bins (tiddit_variant.pyx:265-283, 307-315)
class BinTable:
    """The 50-bp coverage bins (and GC bins) of every contig, concatenated once — the arrays the segment-mean kernel indexes."""

    def __init__(self, coverage_data, gc=None):
        self.offset, self.length = {}, {}
        o = 0
        for name, bins in coverage_data.items():
            self.offset[name], self.length[name] = o, len(bins)
            o += len(bins)
        self.cov = numpy.ascontiguousarray(numpy.concatenate([numpy.asarray(b, dtype=numpy.float64) for b in coverage_data.values()])
                                           if coverage_data else numpy.zeros(0))
        self.gc = None
        if gc is not None:
            self.gc = numpy.ascontiguousarray(numpy.concatenate([numpy.asarray(gc[n][:len(coverage_data[n])], dtype=numpy.int8) for n in coverage_data]))
            if len(self.gc) != len(self.cov):
                raise IndexError("gc array shorter than its coverage array")

    def segment(self, chrom, s, e):
        """the index range Python's ``coverage_data[chrom][s:e]`` selects (non-negative s, e), as offsets into the concatenation"""
        n, o = self.length[chrom], self.offset[chrom]
        s, e = min(max(int(s), 0), n), min(max(int(e), 0), n)
        return o + s, o + max(s, e)


def region_means(table, segments, masked=None, ctx=None):
    """segments: list of (chrom, s, e) bin slices; masked[i] truthy: only bins with gc > -1 count (needs table.gc).
    -> (float64 means — numpy.average of the slice, bit for bit; nan for an empty one —, int64 counts of the bins averaged)"""
    ctx = ctx or _native.default_context()
    nq = len(segments)
    lo = numpy.empty(nq, dtype=numpy.int64)
    hi = numpy.empty(nq, dtype=numpy.int64)
    for i, (chrom, s, e) in enumerate(segments):
        lo[i], hi[i] = table.segment(chrom, s, e)
    m = numpy.zeros(nq, dtype=numpy.uint8) if masked is None else numpy.ascontiguousarray(masked, dtype=numpy.uint8)
    mean = numpy.empty(nq, dtype=numpy.float64)
    count = numpy.empty(nq, dtype=numpy.int64)
    _native.check(ctx.lib.tdt_segment_means(ctx.handle, _native.ptr(table.cov), _native.ptr(table.gc) if table.gc is not None else None,
                                            len(table.cov), _native.ptr(lo), _native.ptr(hi), _native.ptr(m), nq, _native.ptr(mean), _native.ptr(count)))
    return mean, count


def candidate_means(sv_clusters, coverage_data, gc, library, bin_size=50):
    """The three coverage means tiddit_variant.define_variant forms for every candidate (:265-283, :307-315), all candidates of all
    chromosome pairs in ONE device call: -> {(chrA, chrB, cluster): {"avg_a", "avg_b", "covM" (None where the reference takes it
    from get_region instead: breakpoints closer than 1000 bp; 0 for inter-chromosomal candidates)}}"""
    import math
    table = BinTable(coverage_data, gc)
    keys, segs, masked = [], [], []
    for chrA in sv_clusters:
        for chrB in sv_clusters[chrA]:
            for cid, c in sv_clusters[chrA][chrB].items():
                posA, posB = c["posA"], c["posB"]
                if chrA == chrB and posA > posB:
                    posA, posB = posB, posA
                keys.append((chrA, chrB, cid, posA, posB))
                segs.append((chrA, int(math.floor(c["startA"] / float(bin_size))), int(math.floor(c["endA"] / float(bin_size))) + 1))
                segs.append((chrB, int(math.floor(c["startB"] / float(bin_size))), int(math.floor(c["endB"] / float(bin_size))) + 1))
                between = chrA == chrB and abs(posB - posA) >= 1000
                segs.append((chrA, int(math.floor(posA / float(bin_size))), int(math.floor(posB / float(bin_size))) + 1) if between else (chrA, 0, 0))
                masked += [0, 0, 1 if between else 0]
    mean, count = region_means(table, segs, masked) if segs else (numpy.zeros(0), numpy.zeros(0, dtype=numpy.int64))
    out = {}
    for i, (chrA, chrB, cid, posA, posB) in enumerate(keys):
        if chrA != chrB:
            covM = 0
        elif abs(posB - posA) < 1000:
            covM = None
        else:
            covM = mean[3 * i + 2] if count[3 * i + 2] > 4 else library["avg_coverage_{}".format(chrA)]
        out[(chrA, chrB, cid)] = {"avg_a": mean[3 * i], "avg_b": mean[3 * i + 1], "covM": covM}
    return out


# ------------------------------------------------------------------------------------------------------------------
# The evidence store: every placed record of the scan, packed into 16 bytes on the device as the batches go by
# (csrc/tdt_region.hip, tdt_evstore_*), so that the variant stage answers get_region from HBM without reading the file again.
EV_RECORD = numpy.dtype([("start", "<i4"), ("end", "<i4"), ("mate_pos", "<i4"), ("bits", "u1"), ("pad", "u1", (3,))])
EV_UNMAPPED, EV_MATE_UNMAPPED, EV_DUPLICATE, EV_HAS_SA, EV_LOW_Q, EV_DISCORDANT = 0x04, 0x08, 0x01, 0x02, 0x10, 0x20
_EV_COLUMNS = ("tid", "pos", "end", "mapq", "flag", "mate_tid", "mate_pos", "tlen", "sa_off")
_EV_TYPES = (numpy.int32, numpy.int32, numpy.int32, numpy.uint8, numpy.uint16, numpy.int32, numpy.int32, numpy.int32, numpy.int64)


class EvidenceStore:
    """Packed records of one coordinate-sorted file in file order: contig t is records [offset[t], offset[t] + count[t]).
    min_q / max_ins are fixed when the store is made (the scan's own; max_ins truncated to int as get_region's ``int max_ins``)."""

    def __init__(self, path, references, lengths, min_q, max_ins, capacity=0, ctx=None):
        import ctypes
        self.ctx = ctx or _native.default_context()
        self.path = path
        self.references, self.lengths = list(references), [int(x) for x in lengths]
        self.tid = {n: i for i, n in enumerate(self.references)}
        self.min_q, self.max_ins = int(min_q), int(max_ins)
        self.offset = numpy.zeros(len(self.references), dtype=numpy.int64)
        self.count = numpy.zeros(len(self.references), dtype=numpy.int64)
        self.n = 0
        self._last = -1                    # the contig the store ends with
        h = ctypes.c_void_p()
        _native.check(self.ctx.lib.tdt_evstore_create(self.ctx.handle, len(self.references), self.min_q, self.max_ins, int(capacity), ctypes.byref(h)))
        self.handle = h

    def _placed(self, runs):
        """the runs [(tid, lo, hi)] of one batch -> n: records [0, n) of the batch are placed and go into the store; the contigs'
        ranges are booked.  Placed records after unplaced ones, or a contig that comes back, mean an unsorted file: an error."""
        n, tail = 0, False
        for t, lo, hi in runs:
            t, lo, hi = int(t), int(lo), int(hi)
            if hi <= lo:
                continue
            if t < 0:
                tail = True
                continue
            if tail or lo != n or (t != self._last and self.count[t]):
                raise ValueError("evidence store: %s is not coordinate sorted (%s)" % (self.path, self.references[t]))
            if t != self._last:
                self.offset[t] = self.n + lo
                self._last = t
            self.count[t] += hi - lo
            n = hi
        return n

    def add_device_batch(self, b):
        """one DeviceBatch: the pack kernel is enqueued on the reader's stream (call before the batch's buffers are handed back)"""
        n = self._placed(b.runs)
        if n:
            d = b.dev
            _native.check(self.ctx.lib.tdt_evstore_append_device(self.handle, *[d[k] for k in _EV_COLUMNS], n))
            self.n += n

    def add_host_batch(self, b):
        """one host-decoded batch: its columns are uploaded, then the same kernel"""
        tid = b.tid
        if not len(tid):
            return
        edges = numpy.flatnonzero(numpy.diff(tid)) + 1
        runs = [(int(tid[lo]), lo, hi) for lo, hi in zip(numpy.concatenate([[0], edges]), numpy.concatenate([edges, [len(tid)]]))]
        n = self._placed(runs)
        if n:
            cols = [numpy.ascontiguousarray(getattr(b, k)[:n], dtype=dt) for k, dt in zip(_EV_COLUMNS, _EV_TYPES)]
            _native.check(self.ctx.lib.tdt_evstore_append(self.handle, *[_native.ptr(c) for c in cols], n))
            self.n += n

    def spans(self):
        out = numpy.zeros(len(self.references), dtype=numpy.int32)
        _native.check(self.ctx.lib.tdt_evstore_spans(self.handle, _native.ptr(out)))
        return out

    def contig_table(self):
        """int64[n_contigs, 5]: offset, n, max span, tid, length — the table tdt_region_counts_packed reads"""
        t = numpy.zeros((len(self.references), 5), dtype=numpy.int64)
        t[:, 0], t[:, 1], t[:, 2] = self.offset, self.count, self.spans()
        t[:, 3] = numpy.arange(len(self.references))
        t[:, 4] = self.lengths
        return t

    def records(self, t):
        """contig t's packed records, copied to the host (tests)"""
        import ctypes
        out = numpy.zeros(int(self.count[t]), dtype=EV_RECORD)
        if len(out):
            base = ctypes.c_void_p()
            _native.check(self.ctx.lib.tdt_evstore_info(self.handle, None, None, ctypes.byref(base)))
            self.ctx.sync()
            _native.check(self.ctx.lib.tdt_copy_to_host(self.ctx.handle, _native.ptr(out), base.value + 16 * int(self.offset[t]), out.nbytes))
        return out

    def region_counts(self, queries, min_q, max_ins, table=None, ctx=None):
        """queries: (contig index, start, end, bp) rows -> int64[nq, 7] (bases, n_reads, low_q, n_discs, n_splits, crossing_f,
        crossing_r) in ONE launch.  min_q / max_ins must be the store's (the library refuses anything else)."""
        ctx = ctx or self.ctx
        q = numpy.ascontiguousarray(numpy.asarray(queries, dtype=numpy.int32).reshape(-1, 4))
        tab = numpy.ascontiguousarray(self.contig_table() if table is None else table, dtype=numpy.int64)
        out = numpy.zeros((len(q), 7), dtype=numpy.int64)
        _native.check(ctx.lib.tdt_region_counts_packed(ctx.handle, self.handle, _native.ptr(tab), len(tab), _native.ptr(q), len(q),
                                                       int(min_q), int(max_ins), _native.ptr(out)))
        return out

    def region_counts_device(self, d_queries, nq, min_q, max_ins, d_out, table=None, ctx=None):
        """the same counts with the queries and the output in HBM (device pointers: int32[nq][4], 16-byte aligned; int64[nq][7]) —
        the N-rank stage's broadcast queries and reduced counts.  The kernel checks every query's contig row (TDT_E_RANGE); the
        library's stream is finished when this returns."""
        ctx = ctx or self.ctx
        tab = numpy.ascontiguousarray(self.contig_table() if table is None else table, dtype=numpy.int64)
        _native.check(ctx.lib.tdt_region_counts_packed_device(ctx.handle, self.handle, _native.ptr(tab), len(tab), d_queries, int(nq),
                                                              int(min_q), int(max_ins), d_out))

    def depth_dist(self, table=None, ctx=None):
        """-> int64[n_contigs, DD_CAP + 4] in header order (rows of ``table`` when one is given): the bases at depth exactly d for
        d < DD_CAP, the bases at DD_CAP or more, the uncapped sum of depths, the maximum and the minimum depth — per base, from the
        records' exact start / end, all contigs in ONE launch (tiddit_depth_dist.py has the definition)."""
        from .tiddit_depth_dist import DD_CAP
        ctx = ctx or self.ctx
        tab = numpy.ascontiguousarray(self.contig_table() if table is None else table, dtype=numpy.int64).reshape(-1, 5)
        out = numpy.zeros((len(tab), DD_CAP + 4), dtype=numpy.int64)
        _native.check(ctx.lib.tdt_depth_dist(ctx.handle, self.handle, _native.ptr(tab), len(tab), DD_CAP, _native.ptr(out)))
        return out

    def junction_support(self, boundaries, F, table=None, ctx=None):
        """boundaries: (contig row, b) rows, b 0-based = the bases left of the cut -> int64[nb, 4] (left, right, span, span_lowq): the
        kept records that hold base b - F, base b + F - 1, both, and the low-MAPQ ones with both — the reads that cross a breakpoint
        intact with ``F`` (1 ... 1000) aligned bases on either side, all boundaries in ONE launch (tiddit_clip_vcf.py rule 4 has the
        definition)."""
        ctx = ctx or self.ctx
        q = numpy.ascontiguousarray(numpy.asarray(boundaries, dtype=numpy.int32).reshape(-1, 2))
        tab = numpy.ascontiguousarray(self.contig_table() if table is None else table, dtype=numpy.int64).reshape(-1, 5)
        out = numpy.zeros((len(q), 4), dtype=numpy.int64)
        _native.check(ctx.lib.tdt_junction_support(ctx.handle, self.handle, _native.ptr(tab), len(tab), _native.ptr(q), len(q), int(F), _native.ptr(out)))
        return out

    def junction_ms(self):
        """the device milliseconds of the last junction_support launch over this store"""
        import ctypes
        ms = ctypes.c_double(0)
        _native.check(self.ctx.lib.tdt_junction_timing(self.handle, ctypes.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.tdt_evstore_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_store(bam_file_name, min_q, max_ins, ctx=None, shard=None):
    """an evidence store from one ingest pass over the file (the device ingest unless TIDDIT_HOST_INGEST=1) — what the variant stage
    uses when no scan of this process left one.  shard = (rank, world): the records that start in this rank's byte range of the file
    only (bamio.DeviceBamReader); the seam offsets are left in ``store.seam`` = (first_off, next_off, empty) for dist.check_seams."""
    import os
    from .bamio import DeviceBamReader, DeviceBatch
    if shard is None:
        reader = open_bam(bam_file_name)
    else:
        reader = DeviceBamReader(bam_file_name, shard=shard, chunk=int(os.environ.get("TIDDIT_INGEST_CHUNK", str(448 << 20))))
    store = None
    try:
        store = EvidenceStore(bam_file_name, reader.references, reader.lengths, min_q, max_ins,
                              capacity=os.path.getsize(bam_file_name) // 64 // (1 if shard is None else shard[1]),
                              ctx=getattr(reader, "ctx", None) or ctx)
        for b in reader.batches():
            if isinstance(b, DeviceBatch):
                store.add_device_batch(b)
            else:
                store.add_host_batch(b)
        if shard is not None:
            store.seam = (reader.first_off, reader.next_off, reader.first_off is None)
    except BaseException:
        if store is not None:
            store.close()
        raise
    finally:
        reader.close()
    return store
