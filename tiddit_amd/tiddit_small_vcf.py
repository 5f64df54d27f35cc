"""A genotyped small-variant VCF from the ``--sv`` scan (``TIDDIT_SMALL_VCF=1``, valid only together with ``TIDDIT_SNVS`` and/or
``TIDDIT_INDELS``): every finished row of ``{o}.snvs.tab`` and ``{o}.indels.tab`` with the EXACT depth at its position (tiddit_pileup.py:
one more launch per batch of the scan, one prefix sum per job), a reference-read count, a genotype by a stated integer rule and a VCF 4.1
record, written to ``{o}.small.vcf`` in the same pass over the BAM.  Nothing in the reference does this.  The rule (:func:`genotype`)
and the writer (:func:`records_of`, :func:`write_file`) below are the specification; the device computes the rule in one launch per
table (csrc/tdt_pileup.hip, pile_genotype), in integers, so it equals :func:`genotype` bit for bit.

The switch: ``1``.  Any other value, neither partner set, or both partners set with different minimum MAPQ end the job with an error
line before the scan.  The depth uses the partners' ``Q``.  The reference goes into HBM (deletion records need its bases).

The rule.  Every finished row is ``(K1, K2, SUPPORT, REV)`` with ``K1 = tid << 32 | P``, ``P`` 1-based: an SNV's own position, an indel's
anchor base.  With ``depth`` of tiddit_pileup.depth_of:
  * ``ALT = SUPPORT``; ``DP0 = depth[tid][P - 1]``, 0 when ``P - 1 >= length`` (or the contig is unknown);
  * ``OTHER = max(DP0 - ALT, 0)``, ``DP = ALT + OTHER``; ``SN support_above_depth`` += 1 when ``ALT > DP0``.  That can happen: the indel
    gate has no query-length test (nor the ``2^31 - 1`` and ``tid < n_contigs`` tests), so a record tiddit_pileup calls malformed can
    support an indel; an indel's anchor can lie beyond the contig's end, where the read's span is clamped away; and a left-normalised
    indel (``TIDDIT_INDELS_NORM``) is keyed at a shifted anchor that some of its reads do not reach.  For an SNV row it cannot: the SNV
    consumer drops ``off_reference`` reads whole (the depth clamps and counts them), so every read behind an SNV row is counted there;
  * ``L = (20 ALT, 3 (ALT + OTHER), 20 OTHER)`` for ``0/0``, ``0/1``, ``1/1``, in 64 bits; ``m = min(L)``; ``PL_i = min(L_i - m, 9999)``;
    ``GT`` is the smallest ``i`` with ``L_i == m``; ``GQ = min(the second smallest PL, 99)``; ``QUAL = PL_0``.
It is a stated integer rule, not a calibrated model: 20 is the cost of a read that contradicts a homozygous call, 3 the cost of any read
under the heterozygous one (10 log10 2, rounded).

``FILTER`` joins with ``;`` in this order ``RefCall`` (``GT`` is ``0/0``), ``LowGQ`` (``GQ < 20``), ``OneStrand`` (``SUPPORT >= 6`` and
``FWD == 0`` or ``REV == 0``); ``PASS`` when none applies.  ``FORMAT`` is ``GT:DP:AD:GQ:PL`` with ``AD = OTHER,ALT``; ``INFO`` is
``TYPE=...;AS=SUPPORT;FWD=...;REV=...`` and, for the symbolic forms, what the table says:

  SNV                                      REF the table's REF                      ALT the table's ALT
  DEL of n < 50 at anchor P                REF the n + 1 reference bases from P     ALT the first of them
  DEL of n >= 50                           REF the anchor base                      ALT <DEL>          END=P+n;SVLEN=-n
  INS of kind 0 (bases known, n <= 22)     REF the anchor base                      ALT anchor + SEQ
  INS of kind 1 or 2                       REF the anchor base                      ALT <INS>          SVLEN=n

A reference code that is not A, C, G or T is written ``N``.  An indel row is skipped (``SN no_reference`` += 1) when its contig is not
loaded or the bases its record writes — the anchor; a short deletion's ``n + 1`` — run past the contig's end.  Rows of both tables are
merged ascending by ``(tid, P, SNV < DEL < INS, K2)``; two alternative alleles at one position are two biallelic records.

The header: ``##fileformat=VCFv4.1``, the ``##contig`` lines, the command line and the sample column of tiddit_vcf_header (as
tiddit_clip_vcf.header_parts gives them), ``##small_vcf_min_mapq=Q``, ``##small_vcf_left_normalised=0|1`` and one
``##small_vcf_<counter>=n`` per counter of ``SN``: tiddit_pileup's seven, then ``support_above_depth``, ``no_reference``, ``written_records``.

HBM: 4 B per reference base for the depth array, beside the resident reference.

NOT built: calibrated likelihoods, base-quality-aware reference counts, multi-allelic records and MNVs, filters near indels or read
ends, a gVCF or a depth track from the array, N ranks (refused as the partners are), long reads, merging with ``{o}.vcf`` or
``{o}.clips.vcf``.
"""
import time

import numpy

from . import tiddit_pileup

PL_CAP, GQ_CAP, LOW_GQ, ONE_STRAND_MIN, SYMBOLIC_DEL = 9999, 99, 20, 6, 50
SN = tiddit_pileup.SN + ("support_above_depth", "no_reference", "written_records")
GT_TEXT = ("0/0", "0/1", "1/1")
STAGE_SECONDS = {}
STAGE_NOTES = {}
_BASE = ["N"] * 16
_BASE[1], _BASE[2], _BASE[4], _BASE[8] = "A", "C", "G", "T"
_ALT = (("DEL", "Deletion of 50 bases or more"), ("INS", "Insertion whose bases are not written (a hashed or an unknown sequence)"))
_INFO = (("TYPE", 1, "String", "SNV, DEL or INS"), ("AS", 1, "Integer", "Eligible reads that carry the allele"),
         ("FWD", 1, "Integer", "Those on the forward strand"), ("REV", 1, "Integer", "Those on the reverse strand"),
         ("END", 1, "Integer", "End of a symbolic deletion"), ("SVLEN", 1, "Integer", "Length of a symbolic allele (negative: deleted)"))
_FILTER = (("RefCall", "The genotype is 0/0"), ("LowGQ", "GQ below 20"), ("OneStrand", "Six or more supporting reads, all on one strand"))
_FORMAT = (("GT", 1, "String", "Genotype by the integer rule of tiddit_small_vcf"), ("DP", 1, "Integer", "AD summed"),
           ("AD", "R", "Integer", "Eligible reads with an aligned base at POS that do not carry the allele, reads that carry it"),
           ("GQ", 1, "Integer", "The second smallest PL, at most 99"), ("PL", "G", "Integer", "20 ALT, 3 DP, 20 OTHER less their minimum, at most 9999"))


def parse_switch(value, snvs=None, indels=None):
    """``TIDDIT_SMALL_VCF`` -> None (unset or empty) or the minimum MAPQ of the depth; ``snvs`` / ``indels``: what the partners'
    ``parse_switch`` made of ``TIDDIT_SNVS`` / ``TIDDIT_INDELS``.  ValueError (its text is the error line) for anything else"""
    if value is None or value == "":
        return None
    if value != "1":
        raise ValueError("the switch is 1")
    if snvs is None and indels is None:
        raise ValueError("the switch genotypes the rows of TIDDIT_SNVS and TIDDIT_INDELS, neither of which is set")
    if snvs is not None and indels is not None and snvs[1] != indels[1]:
        raise ValueError("TIDDIT_SNVS and TIDDIT_INDELS have different minimum MAPQ (%d and %d): the depth is counted at one" % (snvs[1], indels[1]))
    return snvs[1] if snvs is not None else indels[1]


# ------------------------------------------------------------------------------------------- the rule
def genotype(alt, dp0):
    """THE RULE, one row: ``alt`` = SUPPORT, ``dp0`` the exact depth at its position -> (DP0, OTHER, PL0, PL1, PL2, GT index, GQ, 1 when
    SUPPORT > DP0): the eight columns of ``tiddit_pileup.GENOTYPE_COLUMNS``"""
    alt, dp0 = int(alt), int(dp0)
    other = max(dp0 - alt, 0)
    L = (20 * alt, 3 * (alt + other), 20 * other)
    m = min(L)
    pl = tuple(min(v - m, PL_CAP) for v in L)
    gt = next(i for i in range(3) if L[i] == m)
    return dp0, other, pl[0], pl[1], pl[2], gt, min(sorted(pl)[1], GQ_CAP), int(alt > dp0)


def genotype_rows(rows, depth, lengths):
    """the rule over a table: rows = [(K1, K2, SUPPORT, REV)] (or the four columns), ``depth`` of tiddit_pileup.depth_of -> uint32[n][8]"""
    rows = _row_list(rows)
    out = numpy.zeros((len(rows), 8), dtype=numpy.uint32)
    for i, (k1, _, sup, _) in enumerate(rows):
        tid, P = k1 >> 32, k1 & 0xffffffff
        dp0 = int(depth[tid][P - 1]) if tid < len(lengths) and 1 <= P <= lengths[tid] else 0
        out[i] = genotype(sup, dp0)
    return out


def _row_list(rows):
    if isinstance(rows, tuple):
        return list(zip(*(numpy.asarray(r).tolist() for r in rows)))
    return list(rows or [])


# ------------------------------------------------------------------------------------------- the file
def filter_of(gt, gq, support, rev):
    flags = [name for name, on in (("RefCall", gt == 0), ("LowGQ", gq < LOW_GQ), ("OneStrand", support >= ONE_STRAND_MIN and (rev == 0 or rev == support))) if on]
    return ";".join(flags) or "PASS"


class _Codes:
    """the reference codes of one contig at a time, fetched whole when its first indel row comes (the rows ascend by contig): ``ref`` is
    a refseq.RefSeq or a refseq.HostReference, or None"""

    def __init__(self, ref):
        self.ref, self.tid, self.codes = ref, None, None

    def of(self, tid):
        if tid != self.tid:
            self.tid, self.codes = tid, None
            if self.ref is None:
                pass
            elif hasattr(self.ref, "contigs"):
                self.codes = self.ref.contigs.get(tid)
            elif tid in self.ref.loaded:
                self.codes = self.ref.fetch(tid)
        return self.codes


def records_of(snv_rows, snv_gt, indel_rows, indel_gt, names, ref):
    """``snv_rows`` / ``indel_rows``: the finished rows of the two tables (None: that partner is off), ``snv_gt`` / ``indel_gt``:
    their uint32[n][8] of :func:`genotype_rows` (or of the device) -> (the records' lines in file order, support_above_depth, no_reference)"""
    from . import tiddit_indels
    name = lambda t: names[t] if t < len(names) else str(t)
    merged = [((k1 >> 32, k1 & 0xffffffff, 0, k2), (k1, k2, sup, rev), g) for (k1, k2, sup, rev), g in zip(_row_list(snv_rows), numpy.asarray(snv_gt).tolist())]
    merged += [((k1 >> 32, k1 & 0xffffffff, 2 if k2 >> 63 else 1, k2), (k1, k2, sup, rev), g)
               for (k1, k2, sup, rev), g in zip(_row_list(indel_rows), numpy.asarray(indel_gt).tolist())]
    merged.sort(key=lambda m: m[0])
    codes_of = _Codes(ref)
    lines, above, no_ref = [], 0, 0
    for (tid, P, rank, _), (k1, k2, sup, rev), (dp0, other, pl0, pl1, pl2, gt, gq, ab) in merged:
        info = "AS=%d;FWD=%d;REV=%d" % (sup, sup - rev, rev)
        if rank == 0:
            ref_text, alt_text, info = "ACGT"[(k2 >> 3) & 3], "ACGT"[(k2 >> 1) & 3], "TYPE=SNV;" + info
        else:
            n = (k2 >> 47) & 0xffff
            codes = codes_of.of(tid)
            need = n + 1 if rank == 1 and n < SYMBOLIC_DEL else 1
            if codes is None or P < 1 or P - 1 + need > len(codes):
                no_ref += 1
                continue
            anchor = _BASE[int(codes[P - 1])]
            if rank == 1 and n < SYMBOLIC_DEL:
                ref_text, alt_text, info = "".join(_BASE[c] for c in codes[P - 1:P + n].tolist()), anchor, "TYPE=DEL;" + info
            elif rank == 1:
                ref_text, alt_text, info = anchor, "<DEL>", "TYPE=DEL;%s;END=%d;SVLEN=-%d" % (info, P + n, n)
            elif (k2 >> 45) & 3 == 0:
                ref_text, alt_text, info = anchor, anchor + tiddit_indels.seq_text(k2), "TYPE=INS;" + info
            else:
                ref_text, alt_text, info = anchor, "<INS>", "TYPE=INS;%s;SVLEN=%d" % (info, n)
        above += ab
        lines.append("%s\t%d\t.\t%s\t%s\t%d\t%s\t%s\tGT:DP:AD:GQ:PL\t%s:%d:%d,%d:%d:%d,%d,%d" % (
            name(tid), P, ref_text, alt_text, pl0, filter_of(gt, gq, sup, rev), info, GT_TEXT[gt], sup + other, other, sup, gq, pl0, pl1, pl2))
    return lines, above, no_ref


def counts_of(pile_counts, above, no_reference, records):
    """-> {counter: n} over ``SN``"""
    c = {k: int(v) for k, v in zip(tiddit_pileup.SN, numpy.asarray(pile_counts).tolist())}
    c.update(support_above_depth=int(above), no_reference=int(no_reference), written_records=int(records))
    return c


def write_file(path, parts, min_mapq, normalised, counts, lines):
    """``{o}.small.vcf``: ``parts`` of tiddit_clip_vcf.header_parts, ``counts`` a dict over ``SN``, ``lines`` of :func:`records_of`"""
    contig_lines, cmd, columns, version = parts
    out = ["##fileformat=VCFv4.1", "##source=TIDDIT-%s small_vcf v1" % version]
    out += ['##ALT=<ID={},Description="{}">'.format(*row) for row in _ALT]
    out += contig_lines
    out += ['##INFO=<ID={},Number={},Type={},Description="{}">'.format(*row) for row in _INFO]
    out += ['##FILTER=<ID={},Description="{}">'.format(*row) for row in _FILTER]
    out += ['##FORMAT=<ID={},Number={},Type={},Description="{}">'.format(*row) for row in _FORMAT]
    out += ["##small_vcf_min_mapq=%d" % min_mapq, "##small_vcf_left_normalised=%d" % int(bool(normalised))]
    out += ["##small_vcf_%s=%d" % (k, counts[k]) for k in SN]
    out += [cmd, columns]
    out += lines
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def summary_line(counts):
    return "small vcf: {} records written, {} spans, {} covered bases, {} clamped spans, support above depth {}, no reference {}, malformed records {}".format(
        *(counts[k] for k in ("written_records", "spans", "covered_bases", "clamped_spans", "support_above_depth", "no_reference", "malformed")))


def main(pile, prefix, names, parts, snv_rows, indel_rows, reference, normalised):
    """the stage behind the SNV and indel stages, whose finished rows it reuses (None: that partner is off): the prefix sum, one
    genotype launch per table, the file and the summary line -> the counters"""
    STAGE_SECONDS.clear()
    STAGE_NOTES.clear()
    t = time.time()
    pile_counts = pile.finish()
    STAGE_SECONDS["small vcf depth (device: prefix sum over the difference array)"] = time.time() - t
    empty = numpy.zeros((0, 8), dtype=numpy.uint32)
    t = time.time()
    snv_gt = pile.genotype(snv_rows) if snv_rows is not None else empty
    ms_snv = pile.timing()[3] if snv_rows is not None and len(snv_rows[0]) else 0.0
    indel_gt = pile.genotype(indel_rows) if indel_rows is not None else empty
    ms = pile.timing()
    STAGE_SECONDS["small vcf genotypes (device: one gather launch per table, rows up and down)"] = time.time() - t
    for k, v in zip(("tile sums", "carry", "scan + write"), ms.tolist()):
        STAGE_SECONDS["  pile " + k + " (device time)"] = v * 1e-3
    STAGE_SECONDS["  pile_genotype, snv rows (device time)"] = ms_snv * 1e-3
    STAGE_SECONDS["  pile_genotype, indel rows (device time)"] = (ms[3] if indel_rows is not None and len(indel_rows[0]) else 0.0) * 1e-3
    STAGE_NOTES["small vcf: depth array (bytes)"] = pile.array_bytes
    min_mapq = pile.min_mapq
    pile.close()
    t = time.time()
    lines, above, no_ref = records_of(snv_rows, snv_gt, indel_rows, indel_gt, names, reference)
    counts = counts_of(pile_counts, above, no_ref, len(lines))
    write_file(prefix + ".small.vcf", parts, min_mapq, normalised, counts, lines)
    STAGE_SECONDS["small vcf text (host)"] = time.time() - t
    print(summary_line(counts))
    return counts
