"""Copy-number segments from the depth bins of the ``--sv`` scan (``TIDDIT_CNV=1`` or ``TIDDIT_CNV=W``): ``{o}.cnv.bed`` — the deletions
and duplications that read depth alone shows, which pairs and split reads miss when the breakpoints lie in repeats.  The 50-bp coverage
bins, the GC bins and the ploidy table the job holds after the ploidy stage are all it needs; nothing reads the BAM again.  The CNV
bins and an exact Viterbi segmentation over them run on the device (csrc/tdt_cnv.hip), every processed contig in one call each.

Definition.  ``UNIT = 256``, ``S = 8`` states (copy numbers 0 ... 7), ``CAP = 4*UNIT*UNIT``, ``LAMBDA = 2*UNIT*UNIT``, ``MIN_CLASS = 100``
— parameters of the definition, not measurements: with them a segment needs roughly four or more clean bins to pay for its two
jumps.  ``W`` is the CNV bin size, a multiple of 50 with ``50 <= W <= 3200``; ``K = W // 50``.

  * CONTIGS.  Contig ``c`` is processed if it is in ``coverage_data`` with ``nb >= 1`` bins, its length is ``>= --min_contig``, its
    median ``C`` (``determine_ploidy``'s rule: ``cov > 0 and gc != -1``) is finite and ``> 0``, and ``P = library["contig_ploidy_c"]``
    lies in 1 ... 6.  Other contigs are skipped and named once in a note.
  * EXPECTED DEPTH of a 50-bp bin: ``E[b] = M[gc[b]]`` if class ``gc[b]`` has at least ``MIN_CLASS`` bins in ``tdt_gc_class_medians``'
    count (the contig's bins with that ``gc`` and ``cov > 0``), else ``C``.  ``M`` is numpy's median, formed from the two order
    statistics the device returns (``tiddit_depth.medians_of``).
  * CNV BIN ``t`` covers the 50-bp bins ``tK ... min((t+1)K, nb) - 1``: ``T = ceil(nb / K)`` CNV bins.  A 50-bp bin is usable if
    ``gc[b] != -1``; ``n_t`` is the usable count.  If ``2*n_t < K`` the bin is MASKED, ``x_t = -1``.  Otherwise ``obs_t`` is the float64
    sum of ``cov[b]`` over the usable bins, added left to right, ``exp_t`` the same sum of ``E[b]``, and
    ``x_t = min(8*UNIT, int(rint((obs_t / exp_t) * float(P*UNIT))))``: one IEEE division, one multiplication, round-half-even.
  * SCORES (int64).  ``e_t(k) = 0`` for a masked bin, else ``min(CAP, (x_t - UNIT*k)**2)``.
    ``V_0(k) = e_0(k) + (0 if k == P else LAMBDA)``.  For ``t >= 1``, with ``m = min_i V_{t-1}(i)`` and ``a`` the lowest ``i`` attaining
    it: ``V_t(k) = e_t(k) + min(V_{t-1}(k), m + LAMBDA)`` and the back-pointer ``B_t(k) = k`` if ``V_{t-1}(k) <= m + LAMBDA``, else ``a``.
    The end cost is ``V_{T-1}(k) + (0 if k == P else LAMBDA)``; ``s_{T-1}`` is the lowest ``k`` attaining its minimum, and
    ``s_{t-1} = B_t(s_t)``.
  * SEGMENTS.  The maximal runs of equal ``s_t`` with ``s_t != P``; masked bins are trimmed off both ends of a run and a run with no
    unmasked bin is dropped.  One line per segment, contigs in header order: ``chrom``, ``start = first*W``,
    ``end = min((last+1)*W, contig length)``, ``type`` (``DEL`` if ``CN < P`` else ``DUP``), ``CN``, ``bins`` (the unmasked bins of the
    run) and ``meanCN = "{:.3f}".format(sum_x / (bins*UNIT))`` from Python integers.  The first line is
    ``#chrom\\tstart\\tend\\ttype\\tCN\\tbins\\tmeanCN``; the file is written even when it has no segment.

All scores are integers, so the device's chunked (min,+) evaluation is the sequential definition bit for bit.  On N ranks rank 0 holds
the reduced coverage bins and the gathered GC bins when the ploidy stage ends, and runs this stage alone."""
import numpy

from . import _native

BIN = 50
UNIT = 256
STATES = 8
CAP = 4 * UNIT * UNIT
LAMBDA = 2 * UNIT * UNIT
MIN_CLASS = 100
CLASSES = 101
DEFAULT_W = 500
HEADER = "#chrom\tstart\tend\ttype\tCN\tbins\tmeanCN\n"
STAGE_SECONDS = {}


def parse_switch(value):
    """``TIDDIT_CNV``: unset or empty -> None, ``1`` -> 500, a multiple of 50 in 50 ... 3200 -> itself; ValueError (its text is the
    error line) for anything else."""
    if value is None or value == "":
        return None
    if value == "1":
        return DEFAULT_W
    import re
    if not re.fullmatch(r"[0-9]+", value):
        raise ValueError("the switch is 1 (bins of 500 bp) or the bin size W in bp")
    w = int(value)
    if w % BIN or not BIN <= w <= 64 * BIN:
        raise ValueError("the bin size W is a multiple of 50 with 50 <= W <= 3200")
    return w


def bins_of(nb, K):
    """T: the CNV bins of a contig of nb 50-bp bins"""
    return -(-int(nb) // int(K))


def bin_table(rows):
    """rows: (off, nb, K, P) per contig -> int64[len(rows)][5], tdt_cnv_bins' table with toff filled in"""
    t = numpy.zeros((len(rows), 5), dtype=numpy.int64)
    at = 0
    for i, (off, nb, K, P) in enumerate(rows):
        t[i] = (off, nb, K, P, at)
        at += bins_of(nb, K)
    return t


def chain_table(rows):
    """rows: (T, P) per contig -> int64[len(rows)][3], tdt_cnv_viterbi's table {toff, T, P}"""
    t = numpy.zeros((len(rows), 3), dtype=numpy.int64)
    at = 0
    for i, (T, P) in enumerate(rows):
        t[i] = (at, T, P)
        at += int(T)
    return t


def cnv_bins(cov, gc, table, E, unit=UNIT, ctx=None):
    """tdt_cnv_bins over host arrays; table: int64[nseg][5] {off, nb, K, P, toff}, E: float64[nseg][101] -> int32 x"""
    ctx = ctx or _native.default_context()
    cov = numpy.ascontiguousarray(cov, dtype=numpy.float64)
    gc = numpy.ascontiguousarray(gc, dtype=numpy.int8)
    table = numpy.ascontiguousarray(table, dtype=numpy.int64).reshape(-1, 5)
    E = numpy.ascontiguousarray(E, dtype=numpy.float64).reshape(-1, CLASSES)
    total = sum(bins_of(r[1], r[2]) for r in table)
    x = numpy.zeros(total, dtype=numpy.int32)
    _native.check(ctx.lib.tdt_cnv_bins(ctx.handle, _native.ptr(cov), _native.ptr(gc), len(cov), _native.ptr(table), len(table), _native.ptr(E),
                                       unit, _native.ptr(x)))
    return x


def viterbi(x, table, unit=UNIT, cap=CAP, lam=LAMBDA, ctx=None):
    """tdt_cnv_viterbi over host arrays; table: int64[nseg][3] {toff, T, P} -> int8 state"""
    ctx = ctx or _native.default_context()
    x = numpy.ascontiguousarray(x, dtype=numpy.int32)
    table = numpy.ascontiguousarray(table, dtype=numpy.int64).reshape(-1, 3)
    state = numpy.zeros(len(x), dtype=numpy.int8)
    _native.check(ctx.lib.tdt_cnv_viterbi(ctx.handle, _native.ptr(x), len(x), _native.ptr(table), len(table), unit, cap, lam, _native.ptr(state)))
    return state


def segments_of(state, x, P, W, length, chrom):
    """the segments of ONE contig from its states and CNV bins -> [(chrom, start, end, type, CN, bins, meanCN)]"""
    state = numpy.asarray(state)
    x = numpy.asarray(x)
    T = len(state)
    if T == 0:
        return []
    edges = numpy.flatnonzero(state[1:] != state[:-1]) + 1
    out = []
    for lo, hi in zip(numpy.concatenate([[0], edges]), numpy.concatenate([edges, [T]])):
        cn = int(state[lo])
        if cn == P:
            continue
        seen = numpy.flatnonzero(x[lo:hi] >= 0)
        if not len(seen):
            continue
        first, last = int(lo + seen[0]), int(lo + seen[-1])
        bins = len(seen)
        total = sum(int(v) for v in x[lo:hi][seen])
        out.append((chrom, first * W, min((last + 1) * W, int(length)), "DEL" if cn < P else "DUP", cn, bins,
                    "{:.3f}".format(total / (bins * UNIT))))
    return out


def write_bed(path, segments):
    with open(path, "w") as f:
        f.write(HEADER)
        for s in segments:
            f.write("\t".join(map(str, s)) + "\n")


def expected_depth(lower, upper, count, C):
    """E[nseg][101] from tdt_gc_class_medians' three outputs and the contigs' medians: a class of fewer than MIN_CLASS bins takes C"""
    from . import tiddit_depth
    M = tiddit_depth.medians_of(lower, upper, count)
    return numpy.ascontiguousarray(numpy.where(numpy.asarray(count) >= MIN_CLASS, M, numpy.asarray(C, dtype=numpy.float64)[:, None]))


class Bins:
    """what the first half of the stage leaves: ``contigs`` as given, the processed ones (``used``), the ``skipped`` ones, the
    ``ploidy`` of the used, their chain table ``chains`` (int64[nseg][3] {toff, T, P}), ``W``, and the CNV bins ``d_x`` — an int32
    tensor that stays on the device (None when no contig is processed)"""

    def __init__(self, contigs, used, skipped, ploidy, chains, W, d_x):
        self.contigs, self.used, self.skipped, self.ploidy, self.chains, self.W, self.d_x = contigs, used, skipped, ploidy, chains, W, d_x


def bins_stage(coverage_data, gc_dictionary, library, contigs, contig_length, min_contig, W, ctx=None):
    """the first half of :func:`main`: which contigs are processed, their ploidies and chain table, and x on the device -> Bins.
    One upload of the processed contigs' bins serves the class medians and the CNV bins."""
    import time
    import torch
    from . import tiddit_coverage_analysis
    STAGE_SECONDS.clear()
    ctx = ctx or _native.default_context()
    K = W // BIN
    t0 = time.time()
    cand, skipped = [], []
    for c in contigs:
        P = library.get("contig_ploidy_{}".format(c))
        if c in coverage_data and len(coverage_data[c]) >= 1 and contig_length[c] >= min_contig and P is not None and 1 <= P <= 6:
            cand.append(c)
        else:
            skipped.append(c)
    covs = [numpy.ascontiguousarray(coverage_data[c], dtype=numpy.float64) for c in cand]
    gcs = [numpy.ascontiguousarray(gc_dictionary[c][:len(v)], dtype=numpy.int8) for c, v in zip(cand, covs)]
    if any(len(g) != len(v) for g, v in zip(gcs, covs)):
        raise IndexError("gc array shorter than its coverage array")
    med = tiddit_coverage_analysis.masked_medians(list(zip(covs, gcs)), ctx=ctx)[0] if cand else []
    keep = [i for i, m in enumerate(med) if numpy.isfinite(m) and m > 0]
    skipped += [cand[i] for i in range(len(cand)) if i not in keep]
    used = [cand[i] for i in keep]
    covs, gcs, C = [covs[i] for i in keep], [gcs[i] for i in keep], [med[i] for i in keep]
    STAGE_SECONDS["CNV contig medians (device, masked_medians)"] = time.time() - t0
    if not used:
        return Bins(contigs, used, skipped, [], numpy.zeros((0, 3), dtype=numpy.int64), W, None)
    t0 = time.time()
    ploidy = [int(library["contig_ploidy_{}".format(c)]) for c in used]
    rows, o = [], 0
    for v, P in zip(covs, ploidy):
        rows.append((o, len(v), K, P))
        o += len(v)
    table = bin_table(rows)
    chains = chain_table([(bins_of(r[1], K), r[3]) for r in rows])
    total = int(chains[:, 1].sum())
    seg = numpy.ascontiguousarray(table[:, :2])
    dev = torch.device("cuda", ctx.device)
    d_cov = torch.from_numpy(numpy.concatenate(covs)).to(dev)
    d_gc = torch.from_numpy(numpy.concatenate(gcs)).to(dev)
    d_cls = torch.empty((2, len(used), CLASSES), dtype=torch.float64, device=dev)        # lower, upper
    d_cls_n = torch.empty((len(used), CLASSES), dtype=torch.int64, device=dev)
    d_x = torch.empty(total, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)                   # torch's copies run on its stream, the library on its own
    STAGE_SECONDS["CNV upload of the bins"] = time.time() - t0
    t0 = time.time()
    _native.check(ctx.lib.tdt_gc_class_medians_device(ctx.handle, d_cov.data_ptr(), d_gc.data_ptr(), o, _native.ptr(seg), len(used),
                                                      d_cls[0].data_ptr(), d_cls[1].data_ptr(), d_cls_n.data_ptr()))
    cls = d_cls.cpu().numpy()
    E = expected_depth(cls[0], cls[1], d_cls_n.cpu().numpy(), C)
    d_E = torch.from_numpy(E).to(dev)
    torch.cuda.synchronize(dev)
    STAGE_SECONDS["CNV expected depth (device, tdt_gc_class_medians)"] = time.time() - t0
    t0 = time.time()
    _native.check(ctx.lib.tdt_cnv_bins_device(ctx.handle, d_cov.data_ptr(), d_gc.data_ptr(), o, _native.ptr(table), len(used), d_E.data_ptr(),
                                              UNIT, d_x.data_ptr()))
    STAGE_SECONDS["CNV bins (device, tdt_cnv_bins)"] = time.time() - t0
    return Bins(contigs, used, skipped, ploidy, chains, W, d_x)


def segments_stage(bins, contig_length, prefix, ctx=None):
    """the second half of :func:`main`: the note on the skipped contigs, x through the Viterbi segmentation, ``{prefix}.cnv.bed`` ->
    the segments.  x stays where it is, for a stage behind this one (tiddit_ascn.py)."""
    import time
    import torch
    ctx = ctx or _native.default_context()
    if bins.skipped:
        order = {c: i for i, c in enumerate(bins.contigs)}
        print("note: TIDDIT_CNV skips {}".format(", ".join(sorted(bins.skipped, key=order.get))))
    segments = []
    if bins.used:
        chains, W = bins.chains, bins.W
        total = int(chains[:, 1].sum())
        t0 = time.time()
        d_state = torch.empty(total, dtype=torch.int8, device=bins.d_x.device)
        torch.cuda.synchronize(bins.d_x.device)
        _native.check(ctx.lib.tdt_cnv_viterbi_device(ctx.handle, bins.d_x.data_ptr(), total, _native.ptr(chains), len(bins.used), UNIT, CAP, LAMBDA,
                                                     d_state.data_ptr()))
        STAGE_SECONDS["CNV segmentation (device, tdt_cnv_viterbi: five kernels)"] = time.time() - t0
        t0 = time.time()
        x, state = bins.d_x.cpu().numpy(), d_state.cpu().numpy()
        for c, P, (toff, T, _) in zip(bins.used, bins.ploidy, chains):
            segments += segments_of(state[toff:toff + T], x[toff:toff + T], P, W, contig_length[c], c)
        STAGE_SECONDS["CNV segments (host)"] = time.time() - t0
    t0 = time.time()
    write_bed(prefix + ".cnv.bed", segments)
    STAGE_SECONDS["CNV text (host)"] = time.time() - t0
    return segments


def main(coverage_data, gc_dictionary, library, contigs, contig_length, min_contig, W, prefix, ctx=None):
    """the stage behind the ploidy table: ``{prefix}.cnv.bed`` from the job's bins (the module docstring has the definition) -> the
    segments.  x stays on the device between the two halves, :func:`bins_stage` and :func:`segments_stage`."""
    return segments_stage(bins_stage(coverage_data, gc_dictionary, library, contigs, contig_length, min_contig, W, ctx=ctx), contig_length,
                          prefix, ctx=ctx)
