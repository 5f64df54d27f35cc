"""Per-contig depth distributions from the ``--sv`` scan's evidence store (``TIDDIT_DEPTH_DIST=1``): how many bases of every contig
are covered at exactly d x and at d x or more, and the mean / min / max depth — statistics of the depth PER BASE, which the 50-bp
coverage bins cannot give (a bin mean of 15 can be 30 x over half the bin and nothing over the rest).  The store's 16-byte records
carry every placed read's exact ``start`` / ``end``, so the answer is in HBM when the scan ends: one kernel launch
(csrc/tdt_depth_dist.hip, ``tdt_depth_dist``) and two small files, no second pass over the BAM.

Definition.  For contig ``t`` of ``LN`` bases, the depth of base ``b`` (0 <= b < LN) is the number of the store's records on ``t`` with

  * ``bits & (TDT_EV_UNMAPPED | TDT_EV_DUPLICATE | TDT_EV_LOW_Q) == 0`` and
  * ``start <= b < min(end, LN)``.

That is the read filter of ``--sv``'s own coverage (``-q`` is the store's ``min_q``; secondary and supplementary records count as they
do there) and the half-open interval ``update_coverage`` adds.  The store's ``end`` is the EXCLUSIVE reference end:
``tdt_evstore_append*`` pack the decoded batch's ``end`` column unchanged, and that column is htslib's ``bam_endpos()`` — pos + the
M/D/N/=/X lengths, pos + 1 when there are none (csrc/tdt_bam.hip) — pysam's ``reference_end``, one past the last aligned base.  A record
with ``end <= start`` covers nothing.

Per contig the result is ``int64[DD_CAP + 4]``: ``hist[d]`` for d < DD_CAP the bases at depth exactly d, ``hist[DD_CAP]`` the bases at
depth DD_CAP or more, then the uncapped sum of depths over all bases, the maximum depth, the minimum depth.  The ``hist`` entries sum to
``LN``; a contig without kept records has ``hist[0] = LN`` and sum, max, min 0.

One process only.  On N ranks every rank holds the records that START in its byte range of the file, and the depth of a base near a
shard seam is the sum over two shards' reads: the histogram of a sum is not the sum of the histograms, so per-shard tables do not add
up.  The N-rank job refuses the switch on every rank before its first collective.
"""
import numpy

DD_CAP = 1000          # csrc/tdt_depth_dist.hip's #define: depths of DD_CAP and more share the last bin
SUM, MAX, MIN = DD_CAP + 1, DD_CAP + 2, DD_CAP + 3
STAGE_SECONDS = {}


def parse_switch(value):
    """``TIDDIT_DEPTH_DIST``: unset or empty -> False, ``1`` -> True; ValueError (its text is the error line) for anything else."""
    if value is None or value == "":
        return False
    if value == "1":
        return True
    raise ValueError("the switch is 1 or unset")


def _block(f, name, hist, length):
    at_or_above = numpy.cumsum(hist[::-1])[::-1]
    for d in numpy.flatnonzero(hist > 0):
        f.write("{}\t{}\t{}\t{}\n".format(name, "{}+".format(DD_CAP) if d == DD_CAP else d, int(hist[d]),
                                         "{:.6f}".format(int(at_or_above[d]) / length)))


def write_files(prefix, names, lengths, table):
    """``{prefix}.depth_dist.tab`` (#contig, depth, bases, fraction_at_or_above: one row per depth 0 .. DD_CAP with bases > 0, the last
    bin written ``1000+``; every contig in header order, then ``total``, the element-wise sum) and ``{prefix}.depth_summary.tab``
    (#contig, length, bases = the uncapped sum of depths, mean, min, max; every contig, then ``total``)."""
    table = numpy.asarray(table, dtype=numpy.int64).reshape(len(names), DD_CAP + 4)
    lengths = [int(x) for x in lengths]
    rows = list(zip(names, lengths, table))
    total = numpy.zeros(DD_CAP + 4, dtype=numpy.int64)
    if len(names):
        total[:SUM + 1] = table[:, :SUM + 1].sum(axis=0)
        total[MAX] = table[:, MAX].max()
        total[MIN] = table[:, MIN].min()
    rows.append(("total", sum(lengths), total))
    with open(prefix + ".depth_dist.tab", "w") as f:
        f.write("#contig\tdepth\tbases\tfraction_at_or_above\n")
        for name, length, row in rows:
            _block(f, name, row[:DD_CAP + 1], length)
    with open(prefix + ".depth_summary.tab", "w") as f:
        f.write("#contig\tlength\tbases\tmean\tmin\tmax\n")
        for name, length, row in rows:
            mean = "{:.2f}".format(int(row[SUM]) / length) if length else "nan"
            f.write("{}\t{}\t{}\t{}\t{}\t{}\n".format(name, length, int(row[SUM]), mean, int(row[MIN]), int(row[MAX])))


def main(store, prefix, names=None, lengths=None):
    """the stage behind the scan: the table from the live store in one launch, then the two files.  The store stays as it is."""
    import time
    STAGE_SECONDS.clear()
    t = time.time()
    table = store.depth_dist()
    STAGE_SECONDS["depth distribution launch (device, one launch over all contigs)"] = time.time() - t
    t = time.time()
    write_files(prefix, store.references if names is None else names, store.lengths if lengths is None else lengths, table)
    STAGE_SECONDS["depth distribution text (host)"] = time.time() - t
    return table
