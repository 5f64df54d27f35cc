"""Allele counts at known SNV sites from the ``--sv`` scan (``TIDDIT_ALLELES=sites.vcf[.gz]``): per site of the sites file the
reads' bases — ``A C G T N``, deletions, reference skips and low-quality bases — counted on the device from the batches the scan
already holds in HBM (csrc/tdt_alleles.hip, one launch per batch), written to ``{o}.alleles.tab`` with the B-allele frequency.
Nothing in the reference does this; the definition below is the specification, and :func:`count_read` implements it read by read.

Sites.  Data rows of a VCF (plain or gzip; anything with ``CHROM POS . REF ALT`` in its first five columns).  A row is accepted when
CHROM is a contig of the BAM header, ``1 <= POS <= LN``, and REF and ALT are each one of ``ACGT`` (either case) and differ.  Every
other row is skipped and counted by reason: unknown contig, position outside the contig, not a biallelic SNV — tested in this order.
Several rows at one position share one device site.

Reads that count.  A read of a batch — its decoded columns ``tid pos end mapq flag rec_off`` and the batch's raw record bytes — counts
when

  * ``0 <= tid < n_contigs`` (every contig of the header, as the coverage track),
  * ``flag & (0x4 | 0x100 | 0x200 | 0x400 | 0x800) == 0`` and ``mapq >= min_q`` (the job's ``-q``),
  * at least one site ``s`` (0-based) of its contig lies in ``[pos, end)`` — ``end`` is the batch's column, htslib's ``bam_endpos``:
    pos + the M/D/N/=/X lengths, pos + 1 when there are none.  The bytes of a read without such a site are never looked at,
  * its record has at least one CIGAR operation and ``l_seq >= 1``,
  * and the record is well formed: ``rec_off + 36 <= raw_len`` (the fixed fields can be read),
    ``32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size``, ``rec_off + 4 + block_size <= raw_len``, and every
    CIGAR op code is ``<= 8``.

A read that fails the well-formedness test — or one that the walk below asks for a query base at an index ``>= l_seq`` — is
MALFORMED: it contributes nothing to any site and adds one to the ``malformed`` counter.  (A record with no CIGAR or ``l_seq < 1``
whose fixed fields can be read is simply not a read that counts.)  Every other read that reaches this point adds one to
``reads_used``.  Mates that overlap a site are both counted.

Walk.  Start at ``r = pos``, ``q = 0``.  A site ``s`` is touched by an operation when ``r <= s < r + len``:

  ``M = X``  the base at query index ``q + s - r`` is taken (below); r and q advance
  ``D``      ``DEL`` += 1; r advances
  ``N``      ``SKIP`` += 1; r advances
  ``I S``    only q advances
  ``H P``    nothing

Base and quality: query indices count from 0, an even index is the high nibble of its sequence byte, an odd index the low nibble.
If the quality byte is not ``0xff`` and is below ``min_bq`` (``TIDDIT_ALLELES_MIN_BQ``, default 13, an integer 0 ... 93), ``LOWBQ``
+= 1.  Otherwise nibble 1, 2, 4, 8 adds to ``A C G T`` and every other nibble to ``N``.

Each site has eight uint32 counters ``A C G T N DEL SKIP LOWBQ``, 32 bytes in this order.  More than 2^32 - 1 reads on one site are
outside the contract (the counter wraps).

N ranks.  Every record belongs to exactly one shard of the file, so the counters add: the ``[sites][8]`` table and the two read
counters are SUM-reduced to rank 0 over the job's process group, and rank 0 writes the file the one-process job writes.
"""
import bisect
import ctypes
import gzip
import os
import struct
import time

import numpy

from . import _native, bamio

COLUMNS = ("A", "C", "G", "T", "N", "DEL", "SKIP", "LOWBQ")
A, C, G, T, N, DEL, SKIP, LOWBQ = range(8)
FLAG_MASK = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
DEFAULT_MIN_BQ = 13
SKIP_REASONS = ("unknown contig", "position outside the contig", "not a biallelic SNV")
HEADER = "#CHROM\tPOS\tREF\tALT\tA\tC\tG\tT\tN\tDEL\tSKIP\tLOWBQ\tREF_N\tALT_N\tBAF\n"
_NIBBLE = {1: A, 2: C, 4: G, 8: T}
STAGE_SECONDS = {}


# ------------------------------------------------------------------------------------------- the switch and the sites
def parse_switch(path, min_bq):
    """``TIDDIT_ALLELES`` / ``TIDDIT_ALLELES_MIN_BQ`` -> None (unset or empty) or ``(path, min_bq)``; ValueError (its text is the
    error line) for a file that is not there and for a min_bq that is not an integer 0 ... 93."""
    if path is None or path == "":
        return None
    if not os.path.isfile(path):
        raise ValueError("could not find the sites file")
    if min_bq is None or min_bq == "":
        return path, DEFAULT_MIN_BQ
    try:
        v = int(min_bq)
    except ValueError:
        v = -1
    if not (0 <= v <= 93) or str(v) != min_bq.strip():
        raise ValueError("TIDDIT_ALLELES_MIN_BQ={} is not an integer 0 ... 93".format(min_bq))
    return path, v


class Sites:
    """The accepted rows of a sites file and the device table they share: ``rows`` = [(chrom, pos1, ref, alt, site index)] in file
    order, ``site_pos`` int32 (0-based, contig-major, per contig sorted and unique), ``site_off`` int64[n_contigs + 1], ``skipped`` =
    {reason: rows}."""

    def __init__(self, rows, site_pos, site_off, skipped):
        self.rows, self.site_pos, self.site_off, self.skipped = rows, site_pos, site_off, skipped

    def __len__(self):
        return len(self.site_pos)


def read_sites(path, names, lengths):
    """the sites file -> :class:`Sites` for the header's contigs (see the module docstring for what is accepted)"""
    tid_of = {n: i for i, n in enumerate(names)}
    skipped = {r: 0 for r in SKIP_REASONS}
    accepted = []                                          # (tid, pos0, chrom, ref, alt)
    with open(path, "rb") as f:
        zipped = f.read(2) == b"\x1f\x8b"
    with (gzip.open(path, "rt") if zipped else open(path, "r")) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            c = line.rstrip("\r\n").split("\t")
            if len(c) < 5:
                skipped["not a biallelic SNV"] += 1
                continue
            t = tid_of.get(c[0])
            if t is None:
                skipped["unknown contig"] += 1
                continue
            try:
                pos = int(c[1])
            except ValueError:
                pos = 0
            if not (1 <= pos <= lengths[t]):
                skipped["position outside the contig"] += 1
                continue
            ref, alt = c[3].upper(), c[4].upper()
            if len(ref) != 1 or len(alt) != 1 or ref not in "ACGT" or alt not in "ACGT" or ref == alt:
                skipped["not a biallelic SNV"] += 1
                continue
            accepted.append((t, pos - 1, c[0], ref, alt))
    n = len(names)
    key = numpy.array([(a[0] << 32) | a[1] for a in accepted], dtype=numpy.int64)
    uniq, inverse = numpy.unique(key, return_inverse=True) if len(key) else (key, key)
    site_pos = (uniq & 0xffffffff).astype(numpy.int32)
    site_off = numpy.searchsorted(uniq >> 32, numpy.arange(n + 1)).astype(numpy.int64)
    rows = [(a[2], a[1] + 1, a[3], a[4], int(k)) for a, k in zip(accepted, inverse)]
    return Sites(rows, site_pos, site_off, skipped)


# ------------------------------------------------------------------------------------------- the definition
MALFORMED = "malformed"


def walk_read(site_pos, site_off, tid, pos, end, mapq, flag, rec_off, raw, min_q):
    """the gate, the well-formedness test and the CIGAR walk of THE DEFINITION, one read (tiddit_phase imports them from here):
    -> None (not a read that counts), :data:`MALFORMED`, or ``(name offset in raw, l_read_name, touches)`` with one
    ``(site index, op, nibble, quality byte)`` per site of the read an operation touches, in walk order — op 0 for ``M = X`` (nibble
    and quality are the base's), 2 for ``D``, 3 for ``N`` (both None)."""
    n_contigs = len(site_off) - 1
    if not (0 <= tid < n_contigs) or (flag & FLAG_MASK) or mapq < min_q:
        return None
    o0, o1 = int(site_off[tid]), int(site_off[tid + 1])
    mine = range(bisect.bisect_left(site_pos, pos, o0, o1), bisect.bisect_left(site_pos, end, o0, o1))     # the sites in [pos, end)
    if not mine:
        return None
    raw_len = len(raw)
    if rec_off + 36 > raw_len:
        return MALFORMED
    block_size, = struct.unpack_from("<I", raw, rec_off)
    r0 = rec_off + 4
    l_name = raw[r0 + 8]
    n_cig, = struct.unpack_from("<H", raw, r0 + 12)
    l_seq, = struct.unpack_from("<i", raw, r0 + 16)
    if n_cig == 0 or l_seq < 1:
        return None
    if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > block_size or rec_off + 4 + block_size > raw_len:
        return MALFORMED
    cig = r0 + 32 + l_name
    seq = cig + 4 * n_cig
    qual = seq + (l_seq + 1) // 2
    ops = [struct.unpack_from("<I", raw, cig + 4 * j)[0] for j in range(n_cig)]
    if any((w & 0xf) > 8 for w in ops):
        return MALFORMED
    touches = []
    for k in mine:
        s = int(site_pos[k])
        r, q = pos, 0
        for w in ops:
            op, ln = w & 0xf, w >> 4
            if op in (0, 7, 8):
                if r <= s < r + ln:
                    qi = q + s - r
                    if qi >= l_seq:
                        return MALFORMED
                    byte = raw[seq + (qi >> 1)]
                    touches.append((k, 0, (byte & 0xf) if qi & 1 else (byte >> 4), raw[qual + qi]))
                r += ln
                q += ln
            elif op == 2 or op == 3:
                if r <= s < r + ln:
                    touches.append((k, op, None, None))
                r += ln
            elif op == 1 or op == 4:
                q += ln
    return r0 + 32, l_name, touches


def count_read(table, stats, site_pos, site_off, tid, pos, end, mapq, flag, rec_off, raw, min_q, min_bq):
    """THE DEFINITION, one read: adds to ``table`` (uint32-like [sites][8]) and to ``stats`` = [reads_used, malformed].  ``raw`` is the
    batch's record bytes (bytes-like), the other arguments the read's entries of the batch's columns."""
    got = walk_read(site_pos, site_off, tid, pos, end, mapq, flag, rec_off, raw, min_q)
    if got is None:
        return
    if got is MALFORMED:
        stats[1] += 1
        return
    stats[0] += 1
    for k, op, nib, ql in got[2]:
        table[k][DEL if op == 2 else SKIP if op == 3 else LOWBQ if ql != 0xff and ql < min_bq else _NIBBLE.get(nib, N)] += 1


def count_batch(table, stats, site_pos, site_off, b, min_q, min_bq, only=None):
    """the definition over one batch (an object with the columns ``tid pos end mapq flag rec_off`` and ``raw``); ``only``: the record
    indices to look at (a caller that has already dropped the reads no site can lie in)"""
    raw = b.raw if isinstance(b.raw, (bytes, bytearray)) else memoryview(numpy.ascontiguousarray(b.raw))
    site_pos = [int(x) for x in site_pos]
    for i in (range(len(b.tid)) if only is None else only):
        count_read(table, stats, site_pos, site_off, int(b.tid[i]), int(b.pos[i]), int(b.end[i]), int(b.mapq[i]), int(b.flag[i]),
                   int(b.rec_off[i]), raw, min_q, min_bq)


# ------------------------------------------------------------------------------------------- the device handle
class AlleleCounter:
    """``tdt_alleles_*``: the sites and their counters in HBM; one push per batch of the scan."""

    def __init__(self, site_pos, site_off, min_q, min_bq, ctx=None, phase=None):
        self.ctx = ctx or _native.default_context()
        self.site_pos = numpy.ascontiguousarray(site_pos, dtype=numpy.int32)
        self.site_off = numpy.ascontiguousarray(site_off, dtype=numpy.int64)
        self.n_sites = len(self.site_pos)
        self.min_bq = int(min_bq)
        h = ctypes.c_void_p()
        _native.check(self.ctx.lib.tdt_alleles_create(self.ctx.handle, _native.ptr(self.site_pos), _native.ptr(self.site_off),
                                                      len(self.site_off) - 1, int(min_q), int(min_bq), ctypes.byref(h)))
        self.handle = h
        self.phase = phase                     # TIDDIT_PHASE: (site_codes uint8[sites], capacity, hash_bits[, S, H]) — the observation store beside the counters (tiddit_phase)
        if phase is not None:
            codes = numpy.ascontiguousarray(phase[0], dtype=numpy.uint8)
            try:
                _native.check(self.ctx.lib.tdt_alleles_phase_enable(h, _native.ptr(codes), len(codes), int(phase[1]), int(phase[2])))
            except Exception:
                self.close()
                raise

    def push_device_batch(self, b):
        """one DeviceBatch: enqueued on the reader's stream, nothing waited for (call before the batch's buffers are handed on)"""
        _native.check(self.ctx.lib.tdt_alleles_push_device(self.handle, b.pointer_table(), len(b), b._raw_len))

    def push_host_batch(self, b):
        """one host-decoded batch (or any object with its columns): uploaded, then the same kernel"""
        cols, raw = bamio.host_columns(b, ("tid", "pos", "end", "mapq", "flag", "rec_off"))      # (the arguments of tdt_alleles_push, in order)
        _native.check(self.ctx.lib.tdt_alleles_push(self.handle, *[_native.ptr(c) for c in cols], len(cols[0]), _native.ptr(raw), len(raw)))

    def counts(self):
        """-> (uint32[sites][8], reads_used, malformed), behind everything pushed so far"""
        out = numpy.zeros((self.n_sites, 8), dtype=numpy.uint32)
        used, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _native.check(self.ctx.lib.tdt_alleles_counts(self.handle, _native.ptr(out), ctypes.byref(used), ctypes.byref(bad)))
        return out, used.value, bad.value

    def reset(self):
        _native.check(self.ctx.lib.tdt_alleles_reset(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.tdt_alleles_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------- the file
def write_file(path, rows, table):
    """``{o}.alleles.tab``: the header line, then one line per accepted row in the order of the sites file.  REF_N / ALT_N are the
    row's REF / ALT columns of its site; BAF = ALT_N / (REF_N + ALT_N) as %.6f, ``.`` when the denominator is 0."""
    col = {"A": A, "C": C, "G": G, "T": T}
    counts = numpy.asarray(table).tolist()                 # (Python ints once, not one numpy scalar per field)
    line = "%s\t%d\t%s\t%s" + "\t%d" * 10 + "\t%s\n"
    with open(path, "w") as f:
        f.write(HEADER)
        out = []
        for chrom, pos, ref, alt, k in rows:
            c = counts[k]
            ref_n, alt_n = c[col[ref]], c[col[alt]]
            out.append(line % (chrom, pos, ref, alt, *c, ref_n, alt_n, "%.6f" % (alt_n / (ref_n + alt_n)) if ref_n + alt_n else "."))
            if len(out) >= 65536:
                f.write("".join(out))
                out = []
        f.write("".join(out))


def summary_line(sites, reads_used, malformed):
    return "allele counts: {} sites accepted ({} device sites), rows skipped: {}; reads used {}, malformed records {}".format(
        len(sites.rows), len(sites), ", ".join("{} {}".format(sites.skipped[r], r) for r in SKIP_REASONS), reads_used, malformed)


def reduce_to_rank0(table, reads_used, malformed, group=None):
    """the N-rank job: SUM of every rank's table and read counters on rank 0 (the counters add: a record belongs to one shard).
    -> (table, reads_used, malformed) on rank 0, None elsewhere.  int64 on the wire: exact for any counters inside the contract."""
    import torch
    import torch.distributed as dist
    from . import dist as tdist
    wire = numpy.concatenate([table.reshape(-1).astype(numpy.int64), numpy.array([reads_used, malformed], dtype=numpy.int64)])
    t = torch.from_numpy(wire).to(tdist._wire_device())
    dist.reduce(t, 0, op=dist.ReduceOp.SUM, group=group)
    if dist.get_rank(group) != 0:
        return None
    total = t.cpu().numpy()
    return total[:-2].reshape(-1, 8), int(total[-2]), int(total[-1])


def main(counter, sites, prefix, multi=False, rank=0):
    """the stage behind the scan: the counters off the device, on N ranks summed on rank 0, the file and the summary line"""
    STAGE_SECONDS.clear()
    t = time.time()
    table, used, bad = counter.counts()
    if counter.phase is None:                              # (TIDDIT_PHASE: tiddit_phase.main runs the store's finish behind this stage and closes it)
        counter.close()
    STAGE_SECONDS["allele counters to the host"] = time.time() - t
    if multi:
        t = time.time()
        got = reduce_to_rank0(table, used, bad)
        STAGE_SECONDS["allele counters summed on rank 0"] = time.time() - t
        if got is None:
            return None
        table, used, bad = got
    if rank == 0:
        t = time.time()
        write_file(prefix + ".alleles.tab", sites.rows, table)
        STAGE_SECONDS["allele table text (host)"] = time.time() - t
        print(summary_line(sites, used, bad))
    return table
