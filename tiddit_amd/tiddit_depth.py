"""Depth fold-changes of genotyped SV sites (``TIDDIT_GENOTYPE_DEPTH=1`` beside ``TIDDIT_GENOTYPE=sites.vcf``): the sample column of
``{o}.genotyped.vcf`` gains ``DHFC:DHBFC:DHFFC`` — the site's median depth against the contig, against bins of equal GC content and
against its flanks — from the 50-bp coverage bins and GC bins the ``--sv`` job already holds.  The order statistics are selected on
the device (csrc/tdt_depth.hip); nothing reads the BAM again.

Definitions.  ``cov`` (float64) and ``gc`` (int8, -1 = N-masked) are the 50-bp bins of ONE contig, ``nb`` of them.

  * A site gets values only if ``chrA == chrB`` (and the contig has bins).  Otherwise all three are ``.``.
  * ``lo = min(posA, posB)``, ``hi = max(posA, posB)``.
  * The INSIDE bins are ``lo // 50 ... (hi - 1) // 50``, clipped to ``0 ... nb - 1``; ``lo == hi`` gives the one bin ``lo // 50``, clipped.
  * A bin is USABLE if ``gc != -1``.  Zero coverage is usable: a homozygous deletion has none and must not be masked away.
  * ``I`` = ``numpy.median`` of ``cov`` over the usable inside bins.
  * The FLANK bins are the 20 bins below the first inside bin and the 20 bins above the last, clipped to the contig, taken as one
    set.  ``F`` = ``numpy.median`` of ``cov`` over its usable bins.
  * ``C`` = the contig's median by ``determine_ploidy``'s rule, ``cov > 0 and gc != -1``, over the whole contig.
  * ``M[g]``, g = 0 ... 100, are the contig's class medians: ``numpy.median`` of ``cov`` over the contig's bins with ``gc == g and
    cov > 0``; undefined for an empty class.
  * ``G`` = ``numpy.median`` of ``M[gc[b]]`` over the usable inside bins ``b`` whose class median is defined.
  * ``DHFC = I / C``, ``DHBFC = I / G``, ``DHFFC = I / F``, each written as ``"{:.3f}".format(x)`` — and as ``.`` when ``I`` has no
    usable bin, or when the denominator has no bin or is 0.
  * The median of an even count is the mean of the two middle values, formed on the host by numpy from the two order statistics
    the device returns (as ``tiddit_coverage_analysis`` does): every median is bit-identical to numpy's.

Three device calls for all sites: the class medians of the contigs that hold sites (``tdt_gc_class_medians``), their ``C``
(``tdt_masked_medians_parts``) and ONE table of three windows per site (``tdt_window_medians``: inside, flanks, and inside again with
the class medians looked up for ``G``)."""
import numpy

from . import _native

BIN = 50
FLANK = 20
CLASSES = 101
FORMAT_IDS = ("DHFC", "DHBFC", "DHFFC")
FORMAT_COL = ":".join(FORMAT_IDS)
FORMAT_LINES = (
    '##FORMAT=<ID=DHFC,Number=1,Type=Float,Description="Median depth of the 50-bp bins between the breakpoints over the median depth of the contig">',
    '##FORMAT=<ID=DHBFC,Number=1,Type=Float,Description="Median depth of the 50-bp bins between the breakpoints over the median depth of the contig\'s bins of the same GC content">',
    '##FORMAT=<ID=DHFFC,Number=1,Type=Float,Description="Median depth of the 50-bp bins between the breakpoints over the median depth of the 20 bins on either side">',
)
NONE = (".", ".", ".")
_EMPTY = (-1, -1)


def inside_bins(posA, posB, nb):
    """-> (first, last) inside bin of a site on a contig of nb > 0 bins"""
    lo, hi = min(posA, posB), max(posA, posB)
    first = lo // BIN
    last = max(first, (hi - 1) // BIN)
    return min(max(first, 0), nb - 1), min(max(last, 0), nb - 1)


def flank_bins(first, last, nb):
    """-> ((first, last) below, (first, last) above), each (-1, -1) when the contig leaves it no bin"""
    below = (max(first - FLANK, 0), first - 1) if first > 0 else _EMPTY
    above = (last + 1, min(last + FLANK, nb - 1)) if last < nb - 1 else _EMPTY
    return below, above


def windows_of(sites, contig_bins):
    """sites: tiddit_genotype's tuples (chrA, posA, chrB, posB, ...); contig_bins: {contig: (offset of its bins in the concatenation,
    nb)}, a contig's class-median row being its position in the dict -> int64[3 * len(sites)][6], tdt_window_medians' rows
    {off, first1, last1, first2, last2, cls}: rows 3i, 3i + 1, 3i + 2 are site i's inside bins, flank bins, and inside bins with the
    class medians looked up.  A site on two contigs, or on a contig without bins, gets three empty windows."""
    row_of = {c: i for i, c in enumerate(contig_bins)}
    t = numpy.full((3 * len(sites), 6), -1, dtype=numpy.int64)
    t[:, 0] = 0
    for i, s in enumerate(sites):
        chrA, posA, chrB, posB = s[0], s[1], s[2], s[3]
        if chrA != chrB or chrA not in contig_bins or contig_bins[chrA][1] < 1:
            continue
        off, nb = contig_bins[chrA]
        first, last = inside_bins(posA, posB, nb)
        below, above = flank_bins(first, last, nb)
        t[3 * i] = (off, first, last, -1, -1, -1)
        t[3 * i + 1] = (off,) + below + above + (-1,)
        t[3 * i + 2] = (off, first, last, -1, -1, row_of[chrA])
    return t


def medians_of(lower, upper, count):
    """numpy.median from the two middle order statistics: their mean as numpy forms it, nan for an empty selection"""
    m = numpy.mean(numpy.stack([numpy.asarray(lower, dtype=numpy.float64), numpy.asarray(upper, dtype=numpy.float64)]), axis=0)
    return numpy.where(numpy.asarray(count) > 0, m, numpy.nan)


def window_medians(cov, gc, table, class_med=None, ctx=None):
    """tdt_window_medians over host arrays -> (lower, upper, count)"""
    ctx = ctx or _native.default_context()
    cov = numpy.ascontiguousarray(cov, dtype=numpy.float64)
    gc = numpy.ascontiguousarray(gc, dtype=numpy.int8)
    table = numpy.ascontiguousarray(table, dtype=numpy.int64).reshape(-1, 6)
    cm = None if class_med is None else numpy.ascontiguousarray(class_med, dtype=numpy.float64).reshape(-1, CLASSES)
    nq = len(table)
    lower, upper, count = numpy.zeros(nq), numpy.zeros(nq), numpy.zeros(nq, dtype=numpy.int64)
    _native.check(ctx.lib.tdt_window_medians(ctx.handle, _native.ptr(cov), _native.ptr(gc), len(cov), _native.ptr(table), nq, _native.ptr(cm),
                                             0 if cm is None else len(cm), _native.ptr(lower), _native.ptr(upper), _native.ptr(count)))
    return lower, upper, count


def gc_class_medians(cov, gc, segments, ctx=None):
    """tdt_gc_class_medians over host arrays; segments: (offset, bins) rows -> (lower, upper, count), each [len(segments)][101]"""
    ctx = ctx or _native.default_context()
    cov = numpy.ascontiguousarray(cov, dtype=numpy.float64)
    gc = numpy.ascontiguousarray(gc, dtype=numpy.int8)
    seg = numpy.ascontiguousarray(segments, dtype=numpy.int64).reshape(-1, 2)
    ns = len(seg)
    lower, upper, count = numpy.zeros((ns, CLASSES)), numpy.zeros((ns, CLASSES)), numpy.zeros((ns, CLASSES), dtype=numpy.int64)
    _native.check(ctx.lib.tdt_gc_class_medians(ctx.handle, _native.ptr(cov), _native.ptr(gc), len(cov), _native.ptr(seg), ns,
                                               _native.ptr(lower), _native.ptr(upper), _native.ptr(count)))
    return lower, upper, count


def _ratio(num, den):
    if numpy.isnan(num) or numpy.isnan(den) or den == 0:
        return "."
    return "{:.3f}".format(num / den)


def fields_of(I, C, G, F):
    """the three strings of a site from its four medians (nan = no bin)"""
    return (_ratio(I, C), _ratio(I, G), _ratio(I, F))


def depth_fields(sites, coverage_data, gc, ctx=None):
    """-> [(DHFC, DHBFC, DHFFC)] strings of every site (the module docstring has the definitions).  coverage_data / gc: the job's
    {contig: float64 coverage bins} / {contig: int8 GC bins}.  The class and window kernels share one upload of the bins of the contigs that hold sites."""
    import torch
    from . import tiddit_coverage_analysis
    ctx = ctx or _native.default_context()
    used = []
    for s in sites:
        if s[0] == s[2] and s[0] in coverage_data and s[0] not in used and len(coverage_data[s[0]]):
            used.append(s[0])
    if not used:
        return [NONE for _ in sites]
    covs = [numpy.ascontiguousarray(coverage_data[c], dtype=numpy.float64) for c in used]
    gcs = [numpy.ascontiguousarray(gc[c][:len(v)], dtype=numpy.int8) for c, v in zip(used, covs)]
    if any(len(g) != len(v) for g, v in zip(gcs, covs)):
        raise IndexError("gc array shorter than its coverage array")
    contig_bins, o = {}, 0
    for c, v in zip(used, covs):
        contig_bins[c] = (o, len(v))
        o += len(v)
    table = windows_of(sites, contig_bins)
    seg = numpy.array([contig_bins[c] for c in used], dtype=numpy.int64)
    dev = torch.device("cuda", ctx.device)
    d_cov = torch.from_numpy(numpy.concatenate(covs)).to(dev)
    d_gc = torch.from_numpy(numpy.concatenate(gcs)).to(dev)
    d_table = torch.from_numpy(table).to(dev)
    d_cls = torch.empty((2, len(used), CLASSES), dtype=torch.float64, device=dev)        # lower, upper
    d_cls_n = torch.empty((len(used), CLASSES), dtype=torch.int64, device=dev)
    d_out = torch.empty((2, len(table)), dtype=torch.float64, device=dev)
    d_out_n = torch.empty(len(table), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)                       # torch's copies run on its stream, the library on its own
    _native.check(ctx.lib.tdt_gc_class_medians_device(ctx.handle, d_cov.data_ptr(), d_gc.data_ptr(), o, _native.ptr(seg), len(used),
                                                      d_cls[0].data_ptr(), d_cls[1].data_ptr(), d_cls_n.data_ptr()))
    cls = d_cls.cpu().numpy()
    M = numpy.ascontiguousarray(medians_of(cls[0], cls[1], d_cls_n.cpu().numpy()))
    d_M = torch.from_numpy(M).to(dev)
    torch.cuda.synchronize(dev)
    _native.check(ctx.lib.tdt_window_medians_device(ctx.handle, d_cov.data_ptr(), d_gc.data_ptr(), o, d_table.data_ptr(), len(table),
                                                    d_M.data_ptr(), len(used), d_out[0].data_ptr(), d_out[1].data_ptr(), d_out_n.data_ptr()))
    out = d_out.cpu().numpy()
    med = medians_of(out[0], out[1], d_out_n.cpu().numpy())
    per_contig, _ = tiddit_coverage_analysis.masked_medians(list(zip(covs, gcs)), ctx=ctx)
    C = dict(zip(used, per_contig))
    fields = []
    for i, s in enumerate(sites):
        if s[0] != s[2] or s[0] not in C:
            fields.append(NONE)
        else:
            fields.append(fields_of(med[3 * i], C[s[0]], med[3 * i + 2], med[3 * i + 1]))
    return fields
