"""SNV candidates from the ``--sv`` scan (``TIDDIT_SNVS=1`` / ``S`` / ``S:Q`` / ``S:Q:B``): every position where at least ``S`` eligible
reads carry the same base that differs from the reference, with its support by strand and the local depth, from the batches the scan
already holds in HBM and the resident reference (refseq.py; csrc/tdt_snv.hip: one launch per batch compares every aligned base of every
eligible read with the reference and builds the keys, one sort and the run-length launches per job), written to ``{o}.snvs.tab``.
Nothing in the reference does this.  The definition below is the specification, :func:`events_of_read` implements it read by read and
:func:`summarise` over the whole job.

The switch: ``S`` is the minimum support, 1 ... 10^6, default 3; ``Q`` the minimum MAPQ, 0 ... 255, default 20; ``B`` the minimum base
quality, 0 ... 93, default 20.  A bare ``1`` means the defaults; a support of 1 is written ``1:20``.

Per record, from the batch's columns ``flag tid pos mapq rec_off`` and the record's bytes (``raw`` at ``rec_off``):

  1. ``SN records`` += 1.  The record is ELIGIBLE when ``flag & 0xF04 == 0`` (mapped, primary, not QC-failed, not marked duplicate),
        ``tid >= 0`` and ``mapq >= Q``: ``SN eligible`` += 1.  Nothing else is done for the others, and their bytes are never read.
  2. The record is bounded as ``tdt_indel`` bounds one: ``rec_off + 36 <= raw_len``, its own ``l_seq >= 0``,
        ``32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size`` and ``rec_off + 4 + block_size <= raw_len``.  It is
        MALFORMED (``SN malformed`` += 1, no event, no other counter) when the bound fails, a CIGAR op code is above 8, ``tid >= 2^24``,
        ``pos < 0``, ``pos`` plus the CIGAR's reference length (``M D N = X``) exceeds ``2^31 - 1``, or the CIGAR's query length
        (``M I S = X``) differs from ``l_seq`` when ``l_seq >= 1`` and ``n_cigar_op >= 1``.  Nothing outside ``[raw, raw + raw_len)`` is ever
        read.
  3. A well-bounded record with ``n_cigar_op == 0`` or ``l_seq == 0``: ``SN no_sequence`` += 1, nothing else.
  4. The contig is not loaded in the reference, or ``pos`` plus the reference length is greater than the contig's length:
        ``SN off_reference`` += 1, nothing else (also when a neighbouring contig would match: a contig ends where it ends).
  5. One walk, ``r = pos``, ``q = 0``: ``M = X`` (0, 7, 8) add their length to ``r`` and ``q``; ``D N`` (2, 3) to ``r``; ``I S`` (1, 4) to
        ``q``; ``H P`` (5, 6) to neither.  ``SN aligned_bases`` += the sum of the ``M = X`` lengths.  For every base of an ``M``, ``=`` or
        ``X`` operation — whatever the operation claims — ``c`` is the read's 4-bit code (the even index in the high nibble), ``g`` the
        reference's, ``b`` the quality byte.  The base is a MISMATCH when ``c`` and ``g`` are both one of 1, 2, 4, 8 (A C G T) and
        ``c != g``: an ``N`` in the reference, another IUPAC code on either side and the read's ``=`` code 0 never are.  A mismatch with
        ``b != 0xff`` and ``b < B`` adds 1 to ``SN low_quality`` and is no event; every other mismatch is a KEYED EVENT with ``P = r + 1``,
        the 1-based position of the base.  (``aligned_bases`` and ``low_quality`` count for every record that reaches the walk, noisy
        ones included.)
  6. A read with more than ``SNV_MAX_PER_READ`` = 8 keyed events is NOISY: ``SN noisy_reads`` += 1 and none of its events count (a
        150-bp read with nine high-quality mismatches is a misalignment; the cap is also what bounds the store).  Otherwise
        ``SN reads_with_events`` += 1 when it has any, and ``SN mismatches`` += 1 per event.
  7. Keys, ``rev = flag >> 4 & 1``: ``K1 = tid << 32 | P``, ``K2 = ref2 << 3 | alt2 << 1 | rev`` with A C G T = 0 1 2 3.  Keyed events with
        equal ``(K1, K2 >> 1)`` are one distinct event: ``SUPPORT`` their number, ``REV`` those with bit 0 set, ``FWD`` the rest.
        ``SN distinct_events`` is the number of sets, ``SN reported_events`` those with ``SUPPORT >= S``.  Nothing depends on the order of
        the reads.

``{o}.snvs.tab``: ``# tiddit_amd snvs v1 min_support=S min_mapq=Q min_bq=B``, then ``SN name n`` for the twelve counters in the order of
``SN``, then ``#CHROM POS ID REF ALT SUPPORT FWD REV COV`` and one row per reported event, ascending by ``(K1, K2 >> 1)``, all
tab-separated.  ``POS = P``; ``ID`` is ``.``; ``COV`` is ``"%.2f"`` of the job's own 50-bp coverage bin
``coverage_data[chrom][(P - 1) // 50]``, ``.`` when the job holds no bins for that contig (or none that far).  The column order is
deliberate: the file is a valid ``TIDDIT_ALLELES`` sites file as it stands — ``tiddit_alleles.read_sites`` accepts exactly its data rows
and skips its twelve three-column ``SN`` rows as "not a biallelic SNV" — so a second job, or another sample's, gets exact ``REF_N`` /
``ALT_N`` / ``BAF`` at the discovered sites.

NOT built: an exact per-site depth or reference count in this file (``COV`` is a 50-bp bin; ``TIDDIT_ALLELES`` on the written file gives
the exact counts), filters near indels or read ends, MNVs (two neighbouring mismatches are two rows), genotypes, a VCF, N ranks
(refused in ``__main__.run_sv``: a set of equal keys can straddle shards), long-read libraries (the cap of 8).
"""
import struct
import time

import numpy

from .bamio import _raw_of
from .keyed_counter import KeyedCounter

SNV_MAX_PER_READ = 8
SNV_MAX_CONTIGS = 1 << 24
END_LIMIT = (1 << 31) - 1
MAX_SUPPORT = 10 ** 6
MAX_BQ = 93
DEFAULT_SUPPORT, DEFAULT_MAPQ, DEFAULT_BQ = 3, 20, 20
SN = ("records", "eligible", "malformed", "no_sequence", "off_reference", "aligned_bases", "low_quality", "noisy_reads", "reads_with_events",
      "mismatches", "distinct_events", "reported_events")
SN_INDEX = {k: i for i, k in enumerate(SN)}
SIZE = len(SN)
COLUMNS = "#CHROM\tPOS\tID\tREF\tALT\tSUPPORT\tFWD\tREV\tCOV\n"
STAGE_SECONDS = {}
STAGE_NOTES = {}            # counts of the last main() that are not seconds
# what events_of_read says about a record
NOT_ELIGIBLE, MALFORMED, NO_SEQUENCE, OFF_REFERENCE, NOISY, OK = "not_eligible", "malformed", "no_sequence", "off_reference", "noisy", "ok"
_CODE = {1: 0, 2: 1, 4: 2, 8: 3}


def parse_switch(value):
    """``TIDDIT_SNVS`` -> None (unset or empty) or (S, Q, B); ValueError (its text is the error line) for anything else"""
    if value is None or value == "":
        return None
    if value == "1":
        return DEFAULT_SUPPORT, DEFAULT_MAPQ, DEFAULT_BQ
    parts = value.split(":")
    if len(parts) > 3 or not all(p.isascii() and p.isdigit() and len(p) <= 9 for p in parts):
        raise ValueError("the switch is 1, S, S:Q or S:Q:B (minimum support 1 ... 10^6, minimum MAPQ 0 ... 255, minimum base quality 0 ... 93)")
    s = int(parts[0])
    q = int(parts[1]) if len(parts) >= 2 else DEFAULT_MAPQ
    b = int(parts[2]) if len(parts) == 3 else DEFAULT_BQ
    if not 1 <= s <= MAX_SUPPORT:
        raise ValueError("the minimum support is 1 ... 10^6")
    if not 0 <= q <= 255:
        raise ValueError("the minimum MAPQ is 0 ... 255")
    if not 0 <= b <= MAX_BQ:
        raise ValueError("the minimum base quality is 0 ... 93")
    return s, q, b


# ------------------------------------------------------------------------------------------- the definition
def events_of_read(flag, tid, pos, mapq, rec_off, raw, ref, min_mapq=DEFAULT_MAPQ, min_bq=DEFAULT_BQ):
    """THE DEFINITION, one read -> (kind, keys, aligned_bases, low_quality): ``keys`` the read's [(K1, K2)] when kind is OK, else [];
    the two counts are what the read adds to ``SN aligned_bases`` / ``SN low_quality`` (0 unless the record reaches the walk).  ``raw``:
    the batch's record bytes (bytes-like), the other arguments the read's entries of the batch's columns; ``ref``: an object with
    ``length(tid)`` (negative: the contig is not loaded) and ``code(tid, i)`` (refseq.HostReference)."""
    if flag & 0xF04 or tid < 0 or mapq < min_mapq:
        return NOT_ELIGIBLE, [], 0, 0
    bad = (MALFORMED, [], 0, 0)
    raw_len = len(raw)
    if tid >= SNV_MAX_CONTIGS or pos < 0 or rec_off + 36 > raw_len:
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
        return NO_SEQUENCE, [], 0, 0
    contig = ref.length(tid)
    if contig < 0 or pos + ref_len > contig:
        return OFF_REFERENCE, [], 0, 0
    seq = cig + 4 * n_cig
    qual = seq + (L + 1) // 2
    rev = (flag >> 4) & 1
    r, q = pos, 0
    keys, aligned, low = [], 0, 0
    for w in words:
        op, ln = w & 0xf, w >> 4
        if op in (0, 7, 8):
            aligned += ln
            for k in range(ln):
                c = (raw[seq + ((q + k) >> 1)] >> (0 if (q + k) & 1 else 4)) & 0xf
                g = ref.code(tid, r + k)
                if c in _CODE and g in _CODE and c != g:
                    b = raw[qual + q + k]
                    if b != 0xff and b < min_bq:
                        low += 1
                    else:
                        keys.append((tid << 32 | (r + k + 1), _CODE[g] << 3 | _CODE[c] << 1 | rev))
        if op in (0, 2, 3, 7, 8):
            r += ln
        if op in (0, 1, 4, 7, 8):
            q += ln
    if len(keys) > SNV_MAX_PER_READ:
        return NOISY, [], aligned, low
    return OK, keys, aligned, low


def _count(sn, kind, keys, aligned, low):
    add = lambda k, n: sn.__setitem__(k, sn.get(k, 0) + n) if n else None
    add("records", 1)
    if kind == NOT_ELIGIBLE:
        return
    add("eligible", 1)
    add("malformed", int(kind == MALFORMED))
    add("no_sequence", int(kind == NO_SEQUENCE))
    add("off_reference", int(kind == OFF_REFERENCE))
    add("noisy_reads", int(kind == NOISY))
    add("aligned_bases", aligned)
    add("low_quality", low)
    add("reads_with_events", int(bool(keys)))
    add("mismatches", len(keys))


def keys_of_batch_by_read(b, keys, sn, ref, min_mapq=DEFAULT_MAPQ, min_bq=DEFAULT_BQ, kinds=None):
    """the definition over one batch, read by read: appends (K1, K2) to ``keys`` and adds to the push counters ``sn`` (a dict);
    ``kinds``: a list that gets every record's kind"""
    raw = _raw_of(b)
    for i in range(len(b.tid)):
        kind, ks, aligned, low = events_of_read(int(b.flag[i]), int(b.tid[i]), int(b.pos[i]), int(b.mapq[i]), int(b.rec_off[i]), raw, ref, min_mapq, min_bq)
        _count(sn, kind, ks, aligned, low)
        keys.extend(ks)
        if kinds is not None:
            kinds.append(kind)


def summarise(keys, sn=None, min_support=DEFAULT_SUPPORT):
    """THE DEFINITION, the whole job: ``keys`` = every keyed event's (K1, K2) in any order, ``sn`` the push counters ->
    (uint64[SIZE], rows): rows = [(K1, K2 with bit 0 clear, SUPPORT, REV)] of the sets with SUPPORT >= min_support, ascending"""
    c = numpy.zeros(SIZE, dtype=numpy.uint64)
    for k, v in (sn or {}).items():
        c[SN_INDEX[k]] = v
    sets = {}
    for k1, k2 in keys:
        s = sets.setdefault((k1, k2 >> 1), [0, 0])
        s[0] += 1
        s[1] += k2 & 1
    rows = [(k1, e << 1, s[0], s[1]) for (k1, e), s in sorted(sets.items()) if s[0] >= min_support]
    c[SN_INDEX["distinct_events"]] = len(sets)
    c[SN_INDEX["reported_events"]] = len(rows)
    return c, rows


# ------------------------------------------------------------------------------------------- the device handle
class SnvCounter(KeyedCounter):
    """``tdt_snv_*``: the key store and the counters in HBM; one push per batch of the scan, one finish per job.  ``reference``: a
    refseq.RefSeq on the same context (kept alive by this object until ``close``)."""
    PREFIX, SIZE, DEFAULT_SUPPORT = "tdt_snv", SIZE, DEFAULT_SUPPORT

    def __init__(self, n_contigs, reference, min_mapq=DEFAULT_MAPQ, min_bq=DEFAULT_BQ, capacity=1 << 20, ctx=None):
        self._create(ctx, int(n_contigs), int(min_mapq), int(min_bq), int(capacity), reference.handle)
        self.min_mapq, self.min_bq = int(min_mapq), int(min_bq)
        self.reference = reference


# ------------------------------------------------------------------------------------------- the file
def write_file(path, counts, rows, names, coverage_data, min_support, min_mapq, min_bq):
    """``{o}.snvs.tab`` (see the module docstring); rows: (K1[], K2[], SUPPORT[], REV[]) or a list of such tuples"""
    if isinstance(rows, tuple):
        rows = list(zip(*(numpy.asarray(r).tolist() for r in rows)))
    c = [int(v) for v in numpy.asarray(counts).tolist()]
    out = ["# tiddit_amd snvs v1 min_support=%d min_mapq=%d min_bq=%d\n" % (min_support, min_mapq, min_bq)]
    out += ["SN\t%s\t%d\n" % (k, c[i]) for i, k in enumerate(SN)]
    out.append(COLUMNS)
    for k1, k2, sup, rev in rows:
        tid, P = k1 >> 32, k1 & 0xffffffff
        chrom = names[tid] if tid < len(names) else str(tid)
        bins = coverage_data.get(chrom) if coverage_data is not None else None
        cov = "%.2f" % float(bins[(P - 1) // 50]) if bins is not None and (P - 1) // 50 < len(bins) else "."
        out.append("%s\t%d\t.\t%s\t%s\t%d\t%d\t%d\t%s\n" % (chrom, P, "ACGT"[(k2 >> 3) & 3], "ACGT"[(k2 >> 1) & 3], sup, sup - rev, rev, cov))
    with open(path, "w") as f:
        f.write("".join(out))


def summary_line(counts):
    c = numpy.asarray(counts)
    return "snvs: {} records, {} eligible, {} aligned bases, {} mismatches, {} distinct events, {} reported, noisy reads {}, malformed records {}".format(
        *(int(c[SN_INDEX[k]]) for k in ("records", "eligible", "aligned_bases", "mismatches", "distinct_events", "reported_events", "noisy_reads", "malformed")))


def main(counter, prefix, coverage_data, names, S, keep=None):
    """the stage behind the scan: the sort and the run lengths on the device, the file and the summary line; ``keep``: a dict that gets
    the finished rows under ``"rows"`` (TIDDIT_SMALL_VCF genotypes them)"""
    STAGE_SECONDS.clear()
    STAGE_NOTES.clear()
    t = time.time()
    counts = counter.finish(S)
    rows = counter.rows()
    if keep is not None:
        keep["rows"] = rows
    ms = counter.timing()
    asks, grows, cap = counter.reserve_stats()
    min_mapq, min_bq = counter.min_mapq, counter.min_bq
    counter.close()
    STAGE_SECONDS["snv sets (device: two sorts, gather, run lengths, rows)"] = time.time() - t
    for k, v in zip(("sort by K2", "gather of K1", "sort by K1", "run lengths + rows"), ms.tolist()):
        STAGE_SECONDS["  snv " + k + " (device time)"] = v * 1e-3
    STAGE_NOTES.update({"snv store: reserves that asked the device": asks, "snv store: growths": grows, "snv store: capacity (keys)": cap,
                        "snv store: keys": int(counts[SN_INDEX["mismatches"]])})
    t = time.time()
    write_file(prefix + ".snvs.tab", counts, rows, names, coverage_data, S, min_mapq, min_bq)
    STAGE_SECONDS["snv table text (host)"] = time.time() - t
    print(summary_line(counts))
    return counts
