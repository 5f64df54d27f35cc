"""Genotyping of known SV sites from the ``--sv`` scan: ``TIDDIT_GENOTYPE=sites.vcf`` writes ``{o}.genotyped.vcf``, one record per
record of ``sites.vcf`` in its order, columns 1-8 as they came in, FORMAT ``GT:CN:COV:DV:RV:LQ:RR:DR`` and the sample column computed
from THIS sample's evidence at the site — what a cohort merge (SVDB) leaves as ``./.`` for every site called in another sample only.

Nothing reads the BAM again: the evidence store the scan left in HBM answers the ``get_region`` calls of all sites in one launch
(``tiddit_variant.evidence``), the coverage bins give ``covM`` (``tiddit_region.candidate_means``), and the cluster table of the job's
own signal tables, kept on the device sorted by posA (:class:`Links`, csrc/tdt_links.hip), gives DV / RV of all sites in one more.

The site of a record (:func:`read_sites`)
  * its own breakpoint is CHROM:POS; the other one is CHROM:END for a symbolic ALT with ``INFO/END``, or the ``chr:pos`` of a
    break-end ALT (``N[c:p[``, ``]c:p]N``, ``N]c:p]``, ``[c:p[N``).  Every record gets its own output record: mates are not paired by ID.
  * regions: ``INFO/REGIONA=s,e`` and ``REGIONB=s,e`` when both are present (TIDDIT's own VCFs and merges of them carry them).  The
    breakpoint inside REGIONA is then A and the one inside REGIONB is B, whichever of them is the record's POS — both records of a
    break-end pair carry the same INFO and get the same column, as in the reference.  REGIONA names no contig: when either
    assignment fits, A is the record's own breakpoint on one contig, and on two contigs the breakpoint whose contig NAME sorts first
    (the order tiddit_signal gives chrA / chrB).
  * the WINDOW RULE otherwise — no regions, or the two breakpoints fit them in neither assignment (counted, and noted at the end of
    the job): A is the record's own breakpoint and around each breakpoint ``start = max(1, pos - max_ins_len)``,
    ``end = min(contig length, pos + max_ins_len)``, ``max_ins_len`` being the job's (``-i``, or the library's 99.9th percentile): a
    pair that supports a junction lies within one maximum insert of it.

DV / RV count the rows of the cluster table — the signals ``tiddit_cluster`` clusters, chrA / chrB and posA / posB oriented as it
orients them — with ``startA <= posA <= endA`` and ``startB <= posB <= endB``.  Signals on contigs the table drops (shorter than
``--min_contig``) count as zero, as they do for the clustering.  A site whose contigs are in the table's other order is flipped
before it is sent; a window-rule site on one contig is sent with its lower breakpoint as A, the order of a pair's two reads.

CN, GT and the number formats are ``tiddit_variant``'s (``copy_number``, ``genotype_of`` with n_contigs = 0, ``depth_genotype`` by the
input's SVTYPE, ``_sample_column``); the SV type is the input's, sites are not retyped.

``TIDDIT_GENOTYPE_DEPTH=1`` appends ``DHFC:DHBFC:DHFFC`` to FORMAT and to every column: the site's depth fold-changes against the
contig, the bins of equal GC content and the flanks (``tiddit_depth``); the eight sub-fields in front of them do not change."""
import ctypes
import re

import numpy

from . import _native, tiddit_depth, tiddit_variant

STAGE_SECONDS = {}
_BND = re.compile(r"^(?:[A-Za-z.]+([\[\]])(?P<c1>[^\[\]]+):(?P<p1>[0-9]+)\1|([\[\]])(?P<c2>[^\[\]]+):(?P<p2>[0-9]+)\4[A-Za-z.]+)$")


class SitesError(ValueError):
    """a sites file the job refuses; str() is the one-line reason"""


def parse_vcf(path):
    """-> (the ``##`` lines, [(line number, columns)] of the records).  Plain text only."""
    if str(path).endswith(".gz"):
        raise SitesError("{}: compressed VCFs are not read; decompress it first".format(path))
    meta, records = [], []
    try:
        f = open(path)
    except OSError as e:
        raise SitesError("{}: {}".format(path, e.strerror or e))
    with f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line:
                continue
            if line.startswith("##"):
                meta.append(line)
            elif not line.startswith("#"):
                records.append((no, line.split("\t")))
    return meta, records


def _info(field):
    out = {}
    for item in field.split(";"):
        k, eq, v = item.partition("=")
        out[k] = v if eq else True
    return out


def _pair(value, what, no):
    try:
        s, e = (int(x) for x in value.split(","))
    except (ValueError, AttributeError):
        raise SitesError("line {}: {}={} is not two integers".format(no, what, value))
    if s > e:
        raise SitesError("line {}: {}={} starts behind its end".format(no, what, value))
    return s, e


def site_of(no, cols, contig_number, contig_length, max_ins_len):
    """one record -> ((chrA, posA, chrB, posB, startA, endA, startB, endB, svtype), rule): rule "regions", "window" (the record has
    no regions) or "missed" (the window rule because its breakpoints fit its regions in neither order)"""
    if len(cols) < 8:
        raise SitesError("line {}: {} columns, a record has at least 8".format(no, len(cols)))
    chrom, alt = cols[0], cols[4]
    if chrom not in contig_number:
        raise SitesError("line {}: contig {} is not in the BAM header".format(no, chrom))
    try:
        pos = int(cols[1])
    except ValueError:
        raise SitesError("line {}: POS {} is not an integer".format(no, cols[1]))
    info = _info(cols[7])
    svtype = info.get("SVTYPE")
    if not isinstance(svtype, str) or not svtype:
        raise SitesError("line {}: no INFO/SVTYPE".format(no))
    m = _BND.match(alt)
    if m:
        mate_chr, mate_pos = (m.group("c1"), int(m.group("p1"))) if m.group("c1") is not None else (m.group("c2"), int(m.group("p2")))
        if mate_chr not in contig_number:
            raise SitesError("line {}: contig {} of ALT {} is not in the BAM header".format(no, mate_chr, alt))
    elif alt.startswith("<") and alt.endswith(">"):
        if "END" not in info:
            raise SitesError("line {}: ALT {} without INFO/END".format(no, alt))
        try:
            mate_chr, mate_pos = chrom, int(info["END"])
        except (ValueError, TypeError):
            raise SitesError("line {}: END={} is not an integer".format(no, info["END"]))
    else:
        raise SitesError("line {}: ALT {} is neither symbolic nor a break end".format(no, alt))
    for c, p in ((chrom, pos), (mate_chr, mate_pos)):
        if p < 0 or p > contig_length[c]:
            raise SitesError("line {}: position {} outside {} (length {})".format(no, p, c, contig_length[c]))
    own, mate = (chrom, pos), (mate_chr, mate_pos)
    rule = "window"
    if "REGIONA" in info and "REGIONB" in info:
        ra, rb = _pair(info["REGIONA"], "REGIONA", no), _pair(info["REGIONB"], "REGIONB", no)
        own_a = ra[0] <= pos <= ra[1] and rb[0] <= mate_pos <= rb[1]
        mate_a = ra[0] <= mate_pos <= ra[1] and rb[0] <= pos <= rb[1]
        if own_a and mate_a and chrom != mate_chr:
            own_a = chrom < mate_chr
            mate_a = not own_a
        if own_a:
            return (chrom, pos, mate_chr, mate_pos, ra[0], ra[1], rb[0], rb[1], svtype), "regions"
        if mate_a:
            return (mate_chr, mate_pos, chrom, pos, ra[0], ra[1], rb[0], rb[1], svtype), "regions"
        rule = "missed"
    w = int(max_ins_len)
    (ca, pa), (cb, pb) = own, mate
    return (ca, pa, cb, pb, max(1, pa - w), min(contig_length[ca], pa + w), max(1, pb - w), min(contig_length[cb], pb + w), svtype), rule


def sites_of(records, contig_number, contig_length, max_ins_len):
    """-> (the sites of parse_vcf's records, the rule each one took: see :func:`site_of`)"""
    out = [site_of(no, cols, contig_number, contig_length, max_ins_len) for no, cols in records]
    return [s for s, _ in out], [r for _, r in out]


def read_sites(path, contig_number, contig_length, max_ins_len):
    """the sites of a plain-text VCF: [(chrA, posA, chrB, posB, startA, endA, startB, endB, svtype)], one per record in file order
    (the module docstring has the rules).  SitesError for a .gz, a contig outside the BAM header, or a malformed record (with its
    line number) — never a silent skip."""
    return sites_of(parse_vcf(path)[1], contig_number, contig_length, max_ins_len)[0]


# ---- evidence -> the sample column: a pure function ---------------------------------------------------------------------------
def site_queries(site):
    """the get_region calls of a site: tiddit_variant.region_queries' three keys"""
    chrA, posA, chrB, posB, startA, endA, startB, endB, _ = site
    return tiddit_variant.region_queries(chrA, chrB, {"startA": startA, "endA": endA, "startB": startB, "endB": endB}, posA, posB)


def sample_column(site, regions, cov_between, dv, rv, args, library):
    """the sample column of one site: regions[(chrom, start, end, bp)] = get_region's 6-tuple for :func:`site_queries`' keys,
    cov_between = covM of an intrachromosomal site with breakpoints 1000 bp or more apart (else unused), dv / rv = its link counts"""
    chrA, posA, chrB, posB, startA, endA, startB, endB, svtype = site
    sd = tiddit_variant.site_evidence(chrA, chrB, posA, posB, startA, endA, startB, endB, regions, cov_between)
    GT = tiddit_variant.genotype_of(rv, dv, sd, args, 0)
    cn = "."
    if chrA == chrB:
        cn = tiddit_variant.copy_number(chrA, sd["covM"], args, library)
        GT = tiddit_variant.depth_genotype(GT, svtype, cn, library["contig_ploidy_{}".format(chrA)])
    return tiddit_variant._sample_column(GT, cn, sd, dv, rv)


def sample_columns(sites, regions, means, counts, args, library, depth=None):
    """every site's column; means[i] = cov_between of site i, counts[i] = (DV, RV), depth[i] = its (DHFC, DHBFC, DHFFC) strings
    (tiddit_depth.depth_fields; None: the eight sub-fields alone)"""
    cols = [sample_column(s, regions, means[i], int(counts[i][0]), int(counts[i][1]), args, library) for i, s in enumerate(sites)]
    if depth is not None:
        cols = [c + ":" + ":".join(d) for c, d in zip(cols, depth)]
    return cols


# ---- link counts on the device ------------------------------------------------------------------------------------------------
class Links:
    """the cluster table's signals in HBM, every (chrA, chrB) bucket sorted by posA (``tdt_links_*``).  posA / posB int32, kind uint8
    (0 pair, 1 split, 2 contig) per signal, bucket_off int64[nb + 1], bucket_a / bucket_b the contig ids of every bucket."""

    def __init__(self, posA, posB, kind, bucket_off, bucket_a=None, bucket_b=None, ctx=None):
        self.ctx = ctx or _native.default_context()
        off = numpy.ascontiguousarray(bucket_off, dtype=numpy.int64)
        self.nb = len(off) - 1
        cols = [numpy.ascontiguousarray(posA, dtype=numpy.int32), numpy.ascontiguousarray(posB, dtype=numpy.int32),
                numpy.ascontiguousarray(kind, dtype=numpy.uint8)]
        if self.nb < 0 or any(len(c) < off[-1] for c in cols):
            raise ValueError("Links: the columns are shorter than the bucket offsets say")
        self.bucket = {}
        if bucket_a is not None:
            self.bucket = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(bucket_a, bucket_b))}
        h = ctypes.c_void_p()
        _native.check(self.ctx.lib.tdt_links_create(self.ctx.handle, *[_native.ptr(c) for c in cols], _native.ptr(off), self.nb, ctypes.byref(h)))
        self.handle = h

    def count(self, rows):
        """rows: (bucket, startA, endA, startB, endB) -> int64[ns, 2] (pairs, splits), ONE launch"""
        r = numpy.zeros((len(rows), 6), dtype=numpy.int32)
        if len(rows):
            r[:, :5] = numpy.asarray(rows, dtype=numpy.int64).reshape(-1, 5).astype(numpy.int32)
        out = numpy.zeros((len(r), 2), dtype=numpy.int64)
        _native.check(self.ctx.lib.tdt_links_count(self.handle, _native.ptr(r), len(r), _native.ptr(out)))
        return out

    def count_device(self, d_sites, ns, d_out):
        """the same with int32[ns][6] sites and int64[ns][2] counts in HBM (device pointers, 8-byte aligned)"""
        _native.check(self.ctx.lib.tdt_links_count_device(self.handle, d_sites, int(ns), d_out))

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.tdt_links_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def links_of_tables(tables, is_mp, min_contig, ctx=None):
    """the :class:`Links` of a job's signal tables (sigtab.SignalTables): its cluster table, as the clustering built it"""
    n, nb = tables.cluster_table(is_mp, min_contig)
    posA, posB = numpy.zeros(n, dtype=numpy.int32), numpy.zeros(n, dtype=numpy.int32)
    off, ba, bb = tables.cluster_columns(posA, posB, nb)
    return Links(posA, posB, tables.cluster_kinds(n), off, ba, bb, ctx=ctx)


def link_rows(sites, bucket, contig_number):
    """the rows :meth:`Links.count` takes for the sites: bucket = {(chrA id, chrB id): index}; a site whose contigs the table holds in
    the other order is flipped, one that it holds in neither gets bucket -1"""
    rows = []
    for chrA, posA, chrB, posB, startA, endA, startB, endB, _ in sites:
        a, b = contig_number[chrA], contig_number[chrB]
        if (a, b) in bucket:
            rows.append((bucket[(a, b)], startA, endA, startB, endB))
        elif (b, a) in bucket:
            rows.append((bucket[(b, a)], startB, endB, startA, endA))
        else:
            rows.append((-1, startA, endA, startB, endB))
    return rows


def _lower_first(sites, rules):
    """window-rule sites on one contig with posA > posB, turned round (a pair's first read is its A side)"""
    out = []
    for s, w in zip(sites, rules):
        if w != "regions" and s[0] == s[2] and s[1] > s[3]:
            s = (s[2], s[3], s[0], s[1], s[6], s[7], s[4], s[5], s[8])
        out.append(s)
    return out


def genotype_sites(store, links, sites, args, library, coverage_data, gc, min_mapq, max_ins_len, contig_number=None, rules=None, depth=False):
    """-> the sample column of every site.  store: the evidence store (tiddit_region.EvidenceStore); links: :class:`Links` with its
    bucket map; rules[i]: the rule site i took (:func:`sites_of`; default: all "regions").  Two launches: the region counts, the link counts.
    depth: the columns end with the depth fold-changes (tiddit_depth.depth_fields)."""
    import time
    from . import tiddit_region
    T = STAGE_SECONDS
    if not sites:
        return []
    contig_number = contig_number or store.tid
    t = time.time()
    regions = tiddit_variant.evidence(store, [q for s in sites for q in site_queries(s)], min_mapq, int(max_ins_len))
    T["region counts (device, one launch)"] = time.time() - t
    t = time.time()
    fake = {}
    for i, (chrA, posA, chrB, posB, startA, endA, startB, endB, _) in enumerate(sites):
        fake.setdefault(chrA, {}).setdefault(chrB, {})[i] = {"posA": posA, "posB": posB, "startA": startA, "endA": endA, "startB": startB, "endB": endB}
    m = tiddit_region.candidate_means(fake, coverage_data, gc, library)
    means = [m[(s[0], s[2], i)]["covM"] for i, s in enumerate(sites)]
    T["coverage means (device)"] = time.time() - t
    t = time.time()
    sent = sites if rules is None else _lower_first(sites, rules)
    counts = links.count(link_rows(sent, links.bucket, contig_number))
    T["link counts (device, one launch)"] = time.time() - t
    fields = None
    if depth:
        t = time.time()
        fields = tiddit_depth.depth_fields(sites, coverage_data, gc)
        T["depth fold-changes (device)"] = time.time() - t
    t = time.time()
    cols = sample_columns(sites, regions, means, counts, args, library, depth=fields)
    T["column text (host)"] = time.time() - t
    return cols


def format_col(depth=False):
    return tiddit_variant.FORMAT_COL + (":" + tiddit_depth.FORMAT_COL if depth else "")


def header(vcf_header, meta, path, max_ins_len, depth=False):
    """this sample's header (tiddit_vcf_header.main) with the input's ##INFO / ##ALT / ##FILTER lines whose ID it lacks and the
    ##TIDDITgenotype line in front of the #CHROM line; depth: the three ##FORMAT lines of the fold-changes in front of that line"""
    lines = vcf_header.split("\n")
    chrom = next(i for i, l in enumerate(lines) if l.startswith("#CHROM"))
    ident = re.compile(r"^##(INFO|ALT|FILTER)=<ID=([^,>]+)")
    have = {m.groups() for m in (ident.match(l) for l in lines[:chrom]) if m}
    extra = []
    for l in meta:
        m = ident.match(l)
        if m and m.groups() not in have:
            have.add(m.groups())
            extra.append(l)
    note = "##TIDDITgenotype=<sites={},window=\"REGIONA/REGIONB of the record, else pos-{w}..pos+{w} clipped to 1..contig length\">".format(path, w=int(max_ins_len))
    if depth:
        extra = extra + list(tiddit_depth.FORMAT_LINES)
    return "\n".join(lines[:chrom] + extra + [note] + lines[chrom:])


def write_vcf(path, head, records, columns, depth=False):
    fmt = format_col(depth)
    with open(path, "w") as f:
        f.write(head + "\n")
        for (_, cols), col in zip(records, columns):
            f.write("\t".join(cols[:8] + [fmt, col]) + "\n")
