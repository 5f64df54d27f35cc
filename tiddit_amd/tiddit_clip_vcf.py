"""Genotyped VCF of the clip-site junctions (``TIDDIT_CLIPS_VCF=1`` / ``F``, valid only together with ``TIDDIT_CLIPS`` and at least one of
``TIDDIT_CLIPS_ALIGN`` / ``TIDDIT_CLIPS_FAR`` / ``TIDDIT_CLIPS_INS``): the rows of ``{o}.clips.align.tab``, ``{o}.clips.far.tab`` and
``{o}.clips.ins.tab`` tell one event once per junction side and once per stage, in three layouts, and none counts the reads that support
the REFERENCE at a breakpoint.  Here the rows become junctions, each junction one record (a BND two), every record's two breakpoints are
looked up in the evidence store the scan left in HBM — one launch counts, base-pair exactly, the reads that cross each breakpoint intact
(csrc/tdt_junction.hip) — and ``{o}.clips.vcf`` holds the records with a genotype.  The reference project answers this size class with an
assembly and ``bwa`` and writes it into its VCF; this is the last step of the path that replaced it.  The definition below is the
specification; :func:`junctions_of`, :func:`events_of`, :func:`boundary_support` and :func:`genotype` implement it in plain Python.

The switch: ``F`` is the flank a read must cover on BOTH sides of a breakpoint to count as reference support, 1 ... 1000, default 10.
A bare ``1`` means the default, so a flank of 1 cannot be asked for from the command line (the device entry takes it); other values are
decimal numbers 2 ... 1000 without leading zeros.

Clip rows are 1-based: an ``R`` site at ``P`` is a read whose last aligned base is ``P``, an ``L`` site at ``P`` one whose first aligned
base is ``P``.  The store is 0-based ``start``, exclusive ``end`` (tiddit_depth_dist.py).

  1. JUNCTIONS from the ALIGN and the FAR rows (``tiddit_clip_align.summarise`` / ``tiddit_clip_far.summarise``).  An ``R`` row ``r`` and
        an ``L`` row ``o`` are a junction when each is the other's mate (``r.MATE == o.POS`` and ``o.MATE == r.POS``; the ALIGN rows of
        one contig, for FAR ``r``'s mate contig is ``o``'s contig and ``o``'s is ``r``'s), both have the same ``TYPE`` in DEL, DUP, BND,
        the same ``LEN`` and the same ``HOM``.  The junction's identity is ``(tid_R, P_R, tid_L, P_L)``.  Rows that make no record are
        counted: ``inv_rows`` (``TYPE`` INV), ``one_sided`` (DEL / DUP / BND without a mate; the reverse-strand rows of FAR are among
        them), ``not_mutual`` (a mate whose own choice, type, length or homology is another).  ``REF`` rows and rows without a placement
        are not events and not counted.  A junction found by both stages is ONE junction with ALIGN's rows (``both_sources``;
        ``sources_disagree`` when type, length or ``HOM`` differ).  ``AMBIGUOUS`` is set when either row has ``HITS > 1``.
  2. COORDINATES, left-aligned through the microhomology ``h = HOM``.  Either aligner extends its reads through the homology, the
        left-anchored ones to the right and the right-anchored ones to the left, so the ``R`` site lies ``h`` bases right of the
        left-most placement of the event and the ``L`` site on it:
          DEL   the deleted bases are ``P_R - h + 1 ... P_L - 1``:  ``POS = P_R - h`` (the base in front), ``END = P_L - 1``,
                ``SVLEN = -LEN``;
          DUP   the duplicated bases are ``P_L ... P_R - h``:  ``POS = P_L - 1``, ``END = P_R - h``, ``SVLEN = LEN``;
          BND   two records with ``MATEID``: on the ``R`` row's contig at ``P_R - h`` with ``ALT = N[chrL:P_L[`` and on the ``L`` row's
                contig at ``P_L`` with ``ALT = ]chrR:(P_R - h)]N``.
        ``END - POS = LEN`` follows from rule 1 for DEL and DUP.  Every record carries ``CIPOS=0,h`` and ``HOMLEN=h``.
  3. INSERTIONS from the INS rows (``tiddit_clip_ins.file_rows``: the pairs of ``summarise`` with their sites resolved).  Every pair row,
        CLOSED or OPEN, whose two sites are not the two sites of a junction of rule 1 is a record (``ins_rows``); one whose sites are
        is that junction — a short tandem duplication that ALIGN typed — and is dropped (``ins_explained``).  ``POS = P_R - TSD``,
        ``END = POS``, ``ALT = <INS>``, ``CIPOS=0,TSD``, ``TSD=d``; CLOSED: ``SVLEN=LEN`` and ``SVINSSEQ=SEQ``; OPEN:
        ``LEFT_SVINSSEQ`` / ``RIGHT_SVINSSEQ`` and no ``SVLEN``.  A site that appears in several pair rows makes every one of them a
        record, all ``AMBIGUOUS``; so is a row with ``CLOSURES > 1``.
  4. BOUNDARIES AND SUPPORT.  Every record has two clip sites, hence two boundaries, 0-based, ``b`` = the number of bases left of the
        cut: an ``R`` site at ``P`` cuts at ``b = P``, an ``L`` site at ``P`` at ``b = P - 1``.  For a boundary ``b`` on a contig of
        ``LN`` bases and the flank ``F``, over the store's records of that contig with ``end > start`` and ``e = min(end, LN)``:
          left      the kept records with ``start <= b - F < e``, 0 when ``b - F < 0``;
          right     the kept records with ``start <= b + F - 1 < e``, 0 when ``b + F > LN``;
          span      the kept records with both;
          span_lowq the records with both whose only excluding bit is ``TDT_EV_LOW_Q``.
        Kept is the read filter of tiddit_depth_dist.py: none of ``TDT_EV_UNMAPPED | TDT_EV_DUPLICATE | TDT_EV_LOW_Q``.  A read
        soft-clipped at the boundary has its aligned edge there and cannot span: that is the point.  ``b`` outside ``0 ... LN`` is legal.
        All arithmetic is 64-bit (``b + F`` passes 2^31 on a contig of 2^31 - 1 bases).
  5. GENOTYPE, integers only.  ``ALT = R_SUPPORT + L_SUPPORT`` (the two sites' ``SUPPORT``), ``REF = span_R + span_L``.  DEL / BND / INS:
        ``1/1`` when ``4 ALT >= 3 (ALT + REF)``, else ``0/1`` — the cut is the midpoint of the allele fractions 1/2 and 1 that one and
        two carrying alleles give.  DUP: ``1/1`` when ``12 ALT >= 5 (ALT + REF)``, else ``0/1`` — a tandem duplication keeps both
        reference boundaries intact on the carrying allele, so the fractions are 1/3 and 1/2 and their midpoint 5/12.  This is a STATED
        rule, not a calibrated model: a read over the junction is clipped on one side and counted once in ``ALT``, a reference read long
        enough to cross both boundaries is counted twice in ``REF``, and nothing is fitted to coverage, so a call near its cut is weak
        evidence (``RV`` / ``RR`` are written so that a reader can apply another rule).
  6. THE FILE ``{o}.clips.vcf``.  VCF 4.1; the ``##contig`` lines, the ``##TIDDITcmd`` line and the sample column are what
        tiddit_vcf_header.py gives; ``##ALT`` / ``##INFO`` / ``##FORMAT`` / ``##FILTER`` lines for every key used; ``##clips_vcf_flank=F``
        and one ``##clips_vcf_<counter>=n`` line per counter of ``SN``.  Events ascend by ``(tid of CHROM, POS, END, type, tid_L, P_L)``
        of their (first) record and are numbered ``CLIP_n`` from 1 in that order, a BND pair ``CLIP_n_1`` / ``CLIP_n_2``; the records
        ascend by ``(tid of CHROM, POS, END, type, n)``.  ``REF`` is ``N``, ``QUAL`` ``.``, ``FILTER`` ``PASS`` or ``Ambiguous``.  ``INFO``
        also carries ``SVTYPE``, ``SRC=align|far|align,far|ins`` and ``MISMATCH`` (the two rows' mismatches; a closed insertion's).
        ``FORMAT`` is ``GT:RV:RR:LQ:DPF``: the genotype, ``R_SUPPORT,L_SUPPORT``, ``span_R,span_L``, ``span_lowq_R,span_lowq_L`` and
        ``left_R,right_R,left_L,right_L``, the base-exact depth step across each breakpoint.

With ``TIDDIT_CLIPS_MEI`` (tiddit_clip_mei.py) the ``<INS>`` record of a pair that rule 6 there names gains, behind ``SRC`` and
``MISMATCH``, ``MEI=family;MEISTRAND=+|-;MEISCORE=n;MEISPAN=fstart,fend``; the header gains the four ``##INFO`` lines and
``##clips_vcf_mei_min_score=A`` behind the flank line.  Records of unnamed pairs and all other records are unchanged, and without
the switch the file is byte for byte what it is without this paragraph.

NOT built: mates of INV rows and one-sided records; discordant-pair support (``DV``) for the clip records; cross-referencing or merging
with the records of ``{o}.vcf``; ``HOMSEQ`` and a real ``REF`` base; genotype likelihoods / ``GQ``; N ranks (refused with
``TIDDIT_CLIPS``).
"""
import time

import numpy

DEFAULT_FLANK, MAX_FLANK = 10, 1000
EV_UNMAPPED, EV_DUPLICATE, EV_LOW_Q = 0x04, 0x01, 0x10            # tiddit_region.EV_*: the three bits that exclude a record
EXCLUDING = EV_UNMAPPED | EV_DUPLICATE | EV_LOW_Q
SN = ("junctions", "both_sources", "sources_disagree", "one_sided", "not_mutual", "inv_rows", "ins_rows", "ins_explained", "records", "ambiguous")
L_SIDE, R_SIDE = 0, 1
TYPES = ("DEL", "DUP", "BND")
STAGE_SECONDS = {}

_ALT = (("DEL", "Deletion"), ("DUP", "Tandem duplication"), ("INS", "Insertion"), ("BND", "Break end"))
_INFO = (("SVTYPE", "1", "String", "Type of structural variant"),
         ("END", "1", "Integer", "End of an intra-chromosomal variant"),
         ("SVLEN", "1", "Integer", "Difference in length between REF and ALT alleles"),
         ("MATEID", "1", "String", "ID of the mate break end"),
         ("CIPOS", "2", "Integer", "The event can be placed this far right of POS: the microhomology or target-site duplication"),
         ("HOMLEN", "1", "Integer", "Length of the microhomology at the junction"),
         ("TSD", "1", "Integer", "Length of the target-site duplication of an insertion"),
         ("SVINSSEQ", "1", "String", "Sequence of a closed insertion"),
         ("LEFT_SVINSSEQ", "1", "String", "Known sequence at the left end of an open insertion"),
         ("RIGHT_SVINSSEQ", "1", "String", "Known sequence at the right end of an open insertion"),
         ("SRC", ".", "String", "The clip stages that found the junction: align, far, ins"),
         ("MISMATCH", ".", "Integer", "Mismatches of the two sites' placements (R, L), or inside a closed insertion's overlap"))
_INFO_MEI = (("MEI", "1", "String", "Family of the library that the inserted sequence aligns to best"),
             ("MEISTRAND", "1", "String", "Strand of the family the inserted sequence lies on"),
             ("MEISCORE", "1", "Integer", "Local alignment score against the family (match 1, mismatch 4, gap 6 + length)"),
             ("MEISPAN", "2", "Integer", "First and last base of the family that the alignment covers"))
_FILTER = (("Ambiguous", "A site's consensus places more than once, a site is in several insertion pairs, or an insertion closes at several lengths"),)
_FORMAT = (("GT", "1", "String", "Genotype"),
           ("RV", "2", "Integer", "Clipped reads that support the event at the R and the L site"),
           ("RR", "2", "Integer", "Reads that cross the R and the L breakpoint intact, the flank aligned on both sides"),
           ("LQ", "2", "Integer", "Low mapping quality reads that cross the R and the L breakpoint the same way"),
           ("DPF", "4", "Integer", "Reads over the base one flank left and right of the R breakpoint, then of the L breakpoint"))


def parse_switch(value, clips=True, stages=True):
    """``TIDDIT_CLIPS_VCF`` -> None (unset or empty) or the flank F; ValueError (its text is the error line) for anything else; ``clips``:
    whether ``TIDDIT_CLIPS`` is on; ``stages``: whether one of ``TIDDIT_CLIPS_ALIGN`` / ``TIDDIT_CLIPS_FAR`` / ``TIDDIT_CLIPS_INS`` is"""
    if value is None or value == "":
        return None
    if not clips:
        raise ValueError("the switch joins the rows of TIDDIT_CLIPS, which is not set")
    if not stages:
        raise ValueError("the switch joins the rows of TIDDIT_CLIPS_ALIGN, TIDDIT_CLIPS_FAR and TIDDIT_CLIPS_INS, none of which is set")
    if value == "1":
        return DEFAULT_FLANK
    if not (value.isascii() and value.isdigit() and len(value) <= 9 and value[0] != "0"):
        raise ValueError("the switch is 1 or F (the flank a read covers on both sides of a breakpoint, 2 ... 1000; 1 means 10)")
    if not 2 <= int(value) <= MAX_FLANK:
        raise ValueError("the flank is 2 ... 1000 (1 means 10)")
    return int(value)


# ------------------------------------------------------------------------------------------- the definition
def _site(row, far):
    """an ALIGN or a FAR row of ``summarise`` -> (tid, P, side, SUPPORT, strand, mm, HITS, TYPE, LEN, mate tid, MATE, HOM)"""
    if far:
        tid, P, side, sup, _, _, _, strand, mm, hits, typ, ln, mt, mate, hom = row
    else:
        tid, P, side, sup, _, _, strand, mm, hits, typ, ln, mate, hom = row
        mt = None if mate is None else tid
    return tid, P, side, sup, strand, mm, hits, typ, ln, mt, mate, hom


def junctions_of(rows, far, counts):
    """rule 1 over one stage's rows -> {(tid_R, P_R, tid_L, P_L): (TYPE, LEN, HOM, R site, L site)}; adds to ``inv_rows``, ``one_sided``
    and ``not_mutual`` of ``counts`` (a dict)"""
    sites = [_site(r, far) for r in rows]
    at = {(s[0], s[1], s[2]): s for s in sites}
    out = {}
    for s in sites:
        tid, P, side, _, _, _, _, typ, ln, mt, mate, hom = s
        if typ == "INV":
            counts["inv_rows"] += 1
        if typ not in TYPES:
            continue
        if mate is None:
            counts["one_sided"] += 1
            continue
        o = at.get((mt, mate, 1 - side))
        if o is None or o[9] != tid or o[10] != P or o[7] != typ or o[8] != ln or o[11] != hom:
            counts["not_mutual"] += 1
            continue
        if side == R_SIDE:
            out[(tid, P, o[0], o[1])] = (typ, ln, hom, s, o)
    return out


def events_of(align_rows=None, far_rows=None, ins_rows=None, mei_calls=None):
    """rules 1 to 3: the rows of the three stages (None: the stage did not run) -> (counts: a dict over ``SN`` without ``records`` and
    ``ambiguous`` filled, events): an event is a dict with ``type`` (DEL / DUP / BND / INS), the two sites ``tid_r P_r tid_l P_l``,
    ``sup`` = (R_SUPPORT, L_SUPPORT), ``src``, ``ambiguous``, ``mm`` (a tuple, or None) and, by type, ``len hom`` or ``tsd len seq left
    right``; and ``tid pos end``, the (first) record's place.  The events ascend as rule 6 orders them.  ``mei_calls``: None, or {index
    into ``ins_rows``: (family, strand, score, fstart, fend)} of ``tiddit_clip_mei.calls_for_vcf``: an INS event of such a row has it as ``mei``."""
    counts = {k: 0 for k in SN}
    found = junctions_of(align_rows, False, counts) if align_rows is not None else {}
    src = {k: "align" for k in found}
    for k, v in (junctions_of(far_rows, True, counts) if far_rows is not None else {}).items():
        if k in found:
            counts["both_sources"] += 1
            src[k] = "align,far"
            if found[k][:3] != v[:3]:
                counts["sources_disagree"] += 1
        else:
            found[k], src[k] = v, "far"
    counts["junctions"] = len(found)
    events = []
    for (tr, pr, tl, pl), (typ, ln, hom, r, o) in found.items():
        e = {"type": typ, "tid_r": tr, "P_r": pr, "tid_l": tl, "P_l": pl, "sup": (r[3], o[3]), "src": src[(tr, pr, tl, pl)], "ambiguous": r[6] > 1 or o[6] > 1,
             "mm": (r[5], o[5]), "len": ln, "hom": hom}
        if typ == "DEL":
            e["tid"], e["pos"], e["end"] = tr, pr - hom, pl - 1
        elif typ == "DUP":
            e["tid"], e["pos"], e["end"] = tr, pl - 1, pr - hom
        else:
            e["tid"], e["pos"], e["end"] = tr, pr - hom, pr - hom
        events.append(e)
    in_r, in_l = {}, {}
    for row in ins_rows or ():
        in_r[(row[0], row[1])] = in_r.get((row[0], row[1]), 0) + 1
        in_l[(row[0], row[2])] = in_l.get((row[0], row[2]), 0) + 1
    for p, (tid, pr, pl, tsd, rs, ls, _, _, status, ln, mm, closures, seq, left, right) in enumerate(ins_rows or ()):
        if (tid, pr, tid, pl) in found:
            counts["ins_explained"] += 1
            continue
        counts["ins_rows"] += 1
        events.append({"type": "INS", "tid_r": tid, "P_r": pr, "tid_l": tid, "P_l": pl, "sup": (rs, ls), "src": "ins",
                       "ambiguous": in_r[(tid, pr)] > 1 or in_l[(tid, pl)] > 1 or closures > 1, "mm": None if ln is None else (mm,), "tsd": tsd,
                       "len": ln, "seq": seq, "left": left, "right": right, "tid": tid, "pos": pr - tsd, "end": pr - tsd,
                       "mei": None if mei_calls is None else mei_calls.get(p)})
    events.sort(key=lambda e: (e["tid"], e["pos"], e["end"], e["type"], e["tid_l"], e["P_l"]))
    return counts, events


def boundaries_of(events):
    """rule 4: two boundaries per event, the R site's then the L site's -> [(tid, b)]"""
    out = []
    for e in events:
        out += [(e["tid_r"], e["P_r"]), (e["tid_l"], e["P_l"] - 1)]
    return out


def boundary_support(records, LN, b, F):
    """THE DEFINITION, rule 4, one boundary: ``records`` = the contig's (start, end, bits) in any order -> (left, right, span, span_lowq)"""
    left = right = span = lowq = 0
    pl, pr = b - F, b + F - 1
    for start, end, bits in records:
        start, end, x = int(start), int(end), int(bits) & EXCLUDING
        if end <= start:
            continue
        e = min(end, LN)
        l = pl >= 0 and start <= pl < e
        r = b + F <= LN and start <= pr < e
        if x == 0:
            left += l
            right += r
            span += l and r
        elif x == EV_LOW_Q:
            lowq += l and r
    return left, right, span, lowq


def genotype(typ, alt, ref):
    """rule 5"""
    if typ == "DUP":
        return "1/1" if 12 * alt >= 5 * (alt + ref) else "0/1"
    return "1/1" if 4 * alt >= 3 * (alt + ref) else "0/1"


# ------------------------------------------------------------------------------------------- the file
def header_parts(bam_header, sample_id, version):
    """the ``##contig`` lines, the ``##TIDDITcmd`` line and the column line as tiddit_vcf_header.py gives them for this job (the library
    statistics of its full header are not complete when this stage runs, and are not written here)"""
    from . import tiddit_vcf_header
    return tiddit_vcf_header.contig_lines(bam_header), tiddit_vcf_header.cmd_line(), tiddit_vcf_header.column_line(sample_id), version


def records_of(events, support, names):
    """rules 2, 3, 5 and 6: the events in order and ``support`` = (left, right, span, span_lowq) of every boundary of
    :func:`boundaries_of` -> [(sort key, the record's line without its newline)], ascending"""
    name = lambda t: names[t] if t < len(names) else str(t)
    out = []
    for n, e in enumerate(events, 1):
        (lr, rr, sr, qr), (ll, rl, sl, ql) = (tuple(int(v) for v in support[2 * n - 2]), tuple(int(v) for v in support[2 * n - 1]))
        typ = e["type"]
        sample = "%s:%d,%d:%d,%d:%d,%d:%d,%d,%d,%d" % (genotype(typ, e["sup"][0] + e["sup"][1], sr + sl), e["sup"][0], e["sup"][1], sr, sl, qr, ql, lr, rr, ll, rl)
        flt = "Ambiguous" if e["ambiguous"] else "PASS"
        tail = "SRC=%s" % e["src"] + ("" if e["mm"] is None else ";MISMATCH=" + ",".join(str(m) for m in e["mm"]))
        line = lambda tid, pos, rid, alt, info: "%s\t%d\t%s\tN\t%s\t.\t%s\t%s\tGT:RV:RR:LQ:DPF\t%s" % (name(tid), pos, rid, alt, flt, info, sample)
        if typ == "BND":
            hom, a, b = e["hom"], e["P_r"] - e["hom"], e["P_l"]
            ids = ("CLIP_%d_1" % n, "CLIP_%d_2" % n)
            out.append(((e["tid_r"], a, a, typ, n, 1), line(e["tid_r"], a, ids[0], "N[%s:%d[" % (name(e["tid_l"]), b),
                                                              "SVTYPE=BND;MATEID=%s;CIPOS=0,%d;HOMLEN=%d;%s" % (ids[1], hom, hom, tail))))
            out.append(((e["tid_l"], b, b, typ, n, 2), line(e["tid_l"], b, ids[1], "]%s:%d]N" % (name(e["tid_r"]), a),
                                                              "SVTYPE=BND;MATEID=%s;CIPOS=0,%d;HOMLEN=%d;%s" % (ids[0], hom, hom, tail))))
            continue
        if typ == "INS":
            info = "SVTYPE=INS;END=%d;" % e["end"] + ("" if e["len"] is None else "SVLEN=%d;" % e["len"]) + "CIPOS=0,%d;TSD=%d;" % (e["tsd"], e["tsd"])
            info += ("SVINSSEQ=%s;" % e["seq"]) if e["len"] is not None else "LEFT_SVINSSEQ=%s;RIGHT_SVINSSEQ=%s;" % (e["left"], e["right"])
        else:
            info = "SVTYPE=%s;END=%d;SVLEN=%d;CIPOS=0,%d;HOMLEN=%d;" % (typ, e["end"], -e["len"] if typ == "DEL" else e["len"], e["hom"], e["hom"])
        if typ == "INS" and e.get("mei") is not None:
            tail += ";MEI=%s;MEISTRAND=%s;MEISCORE=%d;MEISPAN=%d,%d" % e["mei"]
        out.append(((e["tid"], e["pos"], e["end"], typ, n, 0), line(e["tid"], e["pos"], "CLIP_%d" % n, "<%s>" % typ, info + tail)))
    out.sort(key=lambda r: r[0])
    return out


def write_file(path, parts, F, counts, records, mei_min=None):
    """``{o}.clips.vcf`` (rule 6): ``parts`` of :func:`header_parts`, ``counts`` a dict over ``SN``, ``records`` of :func:`records_of``;
    ``mei_min``: None, or the minimum score of ``TIDDIT_CLIPS_MEI``"""
    contig_lines, cmd, columns, version = parts
    out = ["##fileformat=VCFv4.1", "##source=TIDDIT-%s clips_vcf v1" % version]
    out += ['##ALT=<ID={},Description="{}">'.format(*row) for row in _ALT]
    out += contig_lines
    out += ['##INFO=<ID={},Number={},Type={},Description="{}">'.format(*row) for row in _INFO + (_INFO_MEI if mei_min is not None else ())]
    out += ['##FILTER=<ID={},Description="{}">'.format(*row) for row in _FILTER]
    out += ['##FORMAT=<ID={},Number={},Type={},Description="{}">'.format(*row) for row in _FORMAT]
    out.append("##clips_vcf_flank=%d" % F)
    if mei_min is not None:
        out.append("##clips_vcf_mei_min_score=%d" % mei_min)
    out += ["##clips_vcf_%s=%d" % (k, counts[k]) for k in SN]
    out += [cmd, columns]
    out += [r[1] for r in records]
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def finish_counts(counts, events, records):
    counts["records"] = len(records)
    counts["ambiguous"] = sum(1 for e in events if e["ambiguous"])
    return counts


def _mei_calls(mei):
    """``mei`` = None or (A, the rows of ``tiddit_clip_mei.file_rows``, the families' names) -> (A or None, the calls or None)"""
    if mei is None:
        return None, None
    from . import tiddit_clip_mei
    return mei[0], tiddit_clip_mei.calls_for_vcf(mei[1], mei[0], mei[2])


def definition_file(path, parts, names, lengths, F, records_of_contig, align_rows=None, far_rows=None, ins_rows=None, mei=None):
    """the file from the definition alone (what the tests compare a job's file with): ``records_of_contig(tid)`` -> the contig's
    (start, end, bits) -> the counters"""
    mei_min, calls = _mei_calls(mei)
    counts, events = events_of(align_rows, far_rows, ins_rows, calls)
    support = [boundary_support(records_of_contig(t), lengths[t], b, F) for t, b in boundaries_of(events)]
    records = records_of(events, support, names)
    write_file(path, parts, F, finish_counts(counts, events, records), records, mei_min)
    return counts


def summary_line(counts):
    return ("clips vcf: {junctions} junctions ({both_sources} from both stages, {sources_disagree} disagree), {ins_rows} insertions ({ins_explained} explained by a "
            "junction), {records} records ({ambiguous} events ambiguous), rows without a record: {one_sided} one-sided, {not_mutual} not mutual, "
            "{inv_rows} inv").format(**counts)


def main(store, prefix, names, F, parts, align_rows=None, far_rows=None, ins_rows=None, mei=None):
    """the stage behind the clip stages: the junctions on the host, ONE launch over the live store for all boundaries (the store stays
    as it is), the file -> the counters (:func:`summary_line`).  Without a boundary nothing is launched.  ``mei``: None, or (A, the
    rows of ``tiddit_clip_mei.file_rows``, the families' names) of ``TIDDIT_CLIPS_MEI``."""
    STAGE_SECONDS.clear()
    t = time.time()
    mei_min, calls = _mei_calls(mei)
    counts, events = events_of(align_rows, far_rows, ins_rows, calls)
    bounds = boundaries_of(events)
    STAGE_SECONDS["clip vcf junctions (host)"] = time.time() - t
    t = time.time()
    support = store.junction_support(bounds, F) if bounds else numpy.zeros((0, 4), dtype=numpy.int64)
    STAGE_SECONDS["clip vcf support (device: one wavefront per boundary over the evidence store)"] = time.time() - t
    if bounds:
        STAGE_SECONDS["  clip vcf junction_support kernel (device time)"] = store.junction_ms() * 1e-3
    t = time.time()
    records = records_of(events, support, names)
    write_file(prefix + ".clips.vcf", parts, F, finish_counts(counts, events, records), records, mei_min)
    STAGE_SECONDS["clip vcf text (host)"] = time.time() - t
    return counts
