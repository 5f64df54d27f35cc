"""Clip-site consensus realigned to the reference (``TIDDIT_CLIPS_ALIGN=1`` / ``W`` / ``W:K`` / ``W:K:M``, valid only together with
``TIDDIT_CLIPS``): for every reported clip site of ``{o}.clips.tab`` whose consensus has at least ``K`` columns, the best placement of
that consensus on the same contig within ``W`` bases of the breakpoint, on either strand, and the event the junction implies (DEL /
DUP / INV with its length, base-pair exact), written to ``{o}.clips.align.tab``.  The clipped bases of a read over a 50-bp ... few-kb
deletion, tandem duplication or inversion are the reference itself a few hundred bases away: too long for a CIGAR indel, too short to
move an insert size.  The search is exact and windowed, on the device (csrc/tdt_clip_align.hip: one workgroup per site over the packed
reference of refseq.py, the site rows of the clip counter's last finish where they lie in HBM).  The definition below is the
specification, :func:`place_site` implements it site by site and :func:`summarise` over the job.

The switch: ``W`` is the search window on either side of the breakpoint, 1 ... 2^20, default 10000; ``K`` the minimum consensus columns
(``CLEN``) for a site to be searched, 1 ... 28, default 20; ``M`` the most mismatches an accepted placement has, 0 ... 27, default 2.
A bare ``1`` means the defaults; a window of 1 is written ``1:20``.

A site is a row of ``ClipCounter.rows()``: ``tid``, ``P`` (1-based), ``side`` (0 = L, 1 = R), ``CLEN`` and the consensus columns
``c_0 ... c_{CLEN-1}`` OUTWARD from the breakpoint, A C G T = 0 1 2 3.  ``len`` is the contig's length, ``ref[q]`` the reference's 4-bit
code at 1-based ``q`` (refseq.CODES); a code that is not A, C, G or T equals no consensus base.

  1. STATUS.  ``CLEN < K``: ``short_consensus``.  Otherwise the contig is not loaded, or ``P`` is outside ``1 ... len``:
        ``off_reference``.  Otherwise the site is ``searched``.
  2. CANDIDATES.  A candidate is a pair ``(Q, strand)`` with ``max(1, P - W) <= Q <= min(len, P + W)``, ``strand`` 0 (forward) or 1
        (reverse complement).  Column ``j`` is compared with ``ref[Q + j]`` (ASCENDING) for (R, forward) and (L, reverse), with
        ``ref[Q - j]`` (DESCENDING) for (R, reverse) and (L, forward); with that base itself on the forward strand and with its
        complement on the reverse strand.  A candidate whose ``CLEN`` reference bases do not all lie inside ``1 ... len`` is no
        candidate.  ``mm`` is the number of columns that differ.
  3. BEST.  The best candidate is the minimum of ``(mm, |Q - P|, strand, Q)``; ``HITS`` is the number of candidates with ``mm <= M``.
        No candidate at all, or a best ``mm > M``: ``unaligned``, ``TYPE`` ``.``.  Otherwise the site is ``aligned``; ``HITS > 1`` also
        counts as ``ambiguous``, and the row is still typed from its best candidate.
  4. TYPE / LEN of an aligned site.  (R, forward): ``Q == P + 1`` REF 0, ``Q > P + 1`` DEL ``Q - P - 1``, ``Q <= P`` DUP ``P - Q + 1``.
        (L, forward): ``Q == P - 1`` REF 0, ``Q < P - 1`` DEL ``P - Q - 1``, ``Q >= P`` DUP ``Q - P + 1``.  Reverse, either side: INV
        ``|Q - P|``.
  5. MATES (host side, over the few rows).  An R row and an L row of one contig are mates when both are DEL or both are DUP, their
        ``LEN`` are equal and ``HOM = R.PARTNER - L.POS`` satisfies ``0 <= HOM <= 28``: an aligner extends each read through the
        junction's microhomology, so both junction sites shift by the homology and ``HOM`` is its length.  A row takes the mate with the
        smallest ``HOM``, then the smaller ``POS``; mating is reported from both rows, each by its own choice.  INV rows are NOT mated:
        the sign of their offset under homology is not worked out here.

``{o}.clips.align.tab``: ``# tiddit_amd clips_align v1 window=W min_cols=K max_mismatch=M``, then ``SN name n`` for the twelve counters
in the order of ``SN``, then ``#CHROM POS SIDE SUPPORT CLEN PARTNER STRAND MISMATCH HITS TYPE LEN MATE HOM`` and one row per SEARCHED
site, in the order of ``{o}.clips.tab``, all tab-separated.  ``PARTNER`` / ``STRAND`` (``+`` / ``-``) / ``MISMATCH`` are those of the best
candidate (also of an unaligned site), ``.`` when there is none; ``TYPE`` / ``LEN`` are ``.`` for an unaligned site; ``MATE`` is the
mate's ``POS`` and ``HOM`` the homology, or ``.``.

Other contigs (translocations) and placements beyond the window are tiddit_clip_far.py's (``TIDDIT_CLIPS_FAR``), by an exact seed.

Sites that place nowhere and face each other are tiddit_clip_ins.py's (``TIDDIT_CLIPS_INS``): insertions, closed from up to 140 columns.

NOT built: gapped placements, searching with more than the 28 consensus columns (the 140 of ``TIDDIT_CLIPS_INS`` are not searched), mates
of INV rows, joining the rows to the SV candidates of ``{o}.vcf`` (tiddit_clip_vcf.py, ``TIDDIT_CLIPS_VCF``, writes the mated DEL / DUP rows as
genotyped records of their own file, ``{o}.clips.vcf``).
"""
import ctypes
import time

import numpy

from . import _native

COLS = 28
MAX_WINDOW = 1 << 20
DEFAULT_WINDOW, DEFAULT_COLS, DEFAULT_MISMATCH = 10000, 20, 2
MAX_HOM = 28
SN = ("sites", "short_consensus", "off_reference", "searched", "aligned", "ambiguous", "unaligned", "ref", "del", "dup", "inv", "mated")
SN_INDEX = {k: i for i, k in enumerate(SN)}
SIZE = len(SN)
COLUMNS = "#CHROM\tPOS\tSIDE\tSUPPORT\tCLEN\tPARTNER\tSTRAND\tMISMATCH\tHITS\tTYPE\tLEN\tMATE\tHOM\n"
SHORT_CONSENSUS, OFF_REFERENCE, SEARCHED = 0, 1, 2               # the status column
NO_MM = 0xffffffff                                               # the mismatch column of a site without a candidate (PARTNER is 0 then)
ALIGN_DTYPES = (numpy.uint32,) * 5                               # status, PARTNER, strand, mismatches, HITS
STAGE_SECONDS = {}
_ACGT = {1: 0, 2: 1, 4: 2, 8: 3}


def parse_switch(value, clips=True):
    """``TIDDIT_CLIPS_ALIGN`` -> None (unset or empty) or (W, K, M); ValueError (its text is the error line) for anything else;
    ``clips``: whether ``TIDDIT_CLIPS`` is on"""
    if value is None or value == "":
        return None
    if not clips:
        raise ValueError("the switch realigns the sites of TIDDIT_CLIPS, which is not set")
    if value == "1":
        return DEFAULT_WINDOW, DEFAULT_COLS, DEFAULT_MISMATCH
    parts = value.split(":")
    if len(parts) > 3 or not all(p.isascii() and p.isdigit() and len(p) <= 9 for p in parts):
        raise ValueError("the switch is 1, W, W:K or W:K:M (window 1 ... 2^20, minimum consensus columns 1 ... 28, maximum mismatches 0 ... 27)")
    w = int(parts[0])
    k = int(parts[1]) if len(parts) >= 2 else DEFAULT_COLS
    m = int(parts[2]) if len(parts) == 3 else DEFAULT_MISMATCH
    if not 1 <= w <= MAX_WINDOW:
        raise ValueError("the window is 1 ... 2^20")
    if not 1 <= k <= COLS:
        raise ValueError("the minimum consensus columns are 1 ... 28")
    if not 0 <= m <= COLS - 1:
        raise ValueError("the maximum mismatches are 0 ... 27")
    return w, k, m


# ------------------------------------------------------------------------------------------- the definition
def place_site(ref, tid, P, side, clen, cons, W=DEFAULT_WINDOW, K=DEFAULT_COLS, M=DEFAULT_MISMATCH):
    """THE DEFINITION, one site -> (status, PARTNER, strand, mm, HITS): rules 1 to 3.  ``ref``: ``length(tid)`` (-1: not loaded) and
    ``code(tid, i)`` with 0-based ``i`` (refseq.HostReference); ``cons`` holds column j in bits 2j + 1 : 2j.  Without a candidate (and
    for a site that is not searched) PARTNER and strand are 0, mm is ``NO_MM`` and HITS 0."""
    none = (0, 0, NO_MM, 0)
    if clen < K:
        return (SHORT_CONSENSUS,) + none
    ln = ref.length(tid)
    if ln < 0 or not 1 <= P <= ln:
        return (OFF_REFERENCE,) + none
    cols = [(cons >> (2 * j)) & 3 for j in range(clen)]
    best, hits = None, 0
    for Q in range(max(1, P - W), min(ln, P + W) + 1):
        for strand in (0, 1):
            step = 1 if (side == 1) == (strand == 0) else -1
            last = Q + step * (clen - 1)
            if not 1 <= last <= ln:
                continue
            mm = 0
            for j in range(clen):
                c = _ACGT.get(ref.code(tid, Q + step * j - 1))
                if c is None or (3 - c if strand else c) != cols[j]:
                    mm += 1
            hits += mm <= M
            key = (mm, abs(Q - P), strand, Q)
            if best is None or key < best:
                best = key
    if best is None:
        return (SEARCHED,) + none
    return SEARCHED, best[3], best[2], best[0], hits


def type_of(P, side, Q, strand):
    """rule 4 -> (TYPE, LEN) of an aligned site"""
    if strand:
        return "INV", abs(Q - P)
    if side == 1:
        return ("REF", 0) if Q == P + 1 else ("DEL", Q - P - 1) if Q > P + 1 else ("DUP", P - Q + 1)
    return ("REF", 0) if Q == P - 1 else ("DEL", P - Q - 1) if Q < P - 1 else ("DUP", Q - P + 1)


def summarise(sites, placed, M=DEFAULT_MISMATCH):
    """THE DEFINITION, the whole job: ``sites`` = [(K1, side, SUPPORT, CLEN)] in the order of ``{o}.clips.tab``, ``placed`` = every
    site's (status, PARTNER, strand, mm, HITS) -> (uint64[SIZE], rows): rows = [(tid, P, side, SUPPORT, CLEN, PARTNER, strand, mm, HITS,
    TYPE, LEN, MATE, HOM)] of the searched sites, in that order; PARTNER / TYPE / MATE are None where the file writes ``.``"""
    c = numpy.zeros(SIZE, dtype=numpy.uint64)
    add = lambda k: c.__setitem__(SN_INDEX[k], c[SN_INDEX[k]] + numpy.uint64(1))
    rows = []
    for (k1, side, sup, clen), (status, Q, strand, mm, hits) in zip(sites, placed):
        k1, side, Q, strand, mm, hits = int(k1), int(side), int(Q), int(strand), int(mm), int(hits)
        add("sites")
        add(("short_consensus", "off_reference", "searched")[status])
        if status != SEARCHED:
            continue
        tid, P = k1 >> 32, k1 & 0xffffffff
        typ = ln = None
        have = mm != NO_MM
        if have and mm <= M:
            add("aligned")
            if hits > 1:
                add("ambiguous")
            typ, ln = type_of(P, side, Q, strand)
            add(typ.lower())
        else:
            add("unaligned")
        rows.append([tid, P, side, int(sup), int(clen), Q if have else None, strand if have else None, mm if have else None, hits, typ, ln, None, None])
    # rule 5
    for r in rows:
        if r[9] not in ("DEL", "DUP"):
            continue
        best = None
        for o in rows:
            if o[0] != r[0] or o[2] == r[2] or o[9] != r[9] or o[10] != r[10]:
                continue
            R, L = (r, o) if r[2] == 1 else (o, r)
            hom = R[5] - L[1]
            if 0 <= hom <= MAX_HOM and (best is None or (hom, o[1]) < best):
                best = (hom, o[1])
        if best is not None:
            r[11], r[12] = best[1], best[0]
            add("mated")
    return c, [tuple(r) for r in rows]


# ------------------------------------------------------------------------------------------- the device entries
def _check_columns(k1, side, clen, cons):
    k1, cons = numpy.ascontiguousarray(k1, dtype=numpy.uint64), numpy.ascontiguousarray(cons, dtype=numpy.uint64)
    side, clen = numpy.ascontiguousarray(side, dtype=numpy.uint32), numpy.ascontiguousarray(clen, dtype=numpy.uint32)
    assert len(k1) == len(side) == len(clen) == len(cons)
    return k1, side, clen, cons


def align_sites(reference, k1, side, clen, cons, W=DEFAULT_WINDOW, K=DEFAULT_COLS, M=DEFAULT_MISMATCH, ctx=None):
    """``tdt_clip_align_sites``: host columns of sites against ``reference`` (a refseq.RefSeq) -> the five columns of ``ALIGN_DTYPES``"""
    ctx = ctx or reference.ctx
    k1, side, clen, cons = _check_columns(k1, side, clen, cons)
    out = [numpy.zeros(len(k1), dtype=dt) for dt in ALIGN_DTYPES]
    _native.check(ctx.lib.tdt_clip_align_sites(ctx.handle, reference.handle, len(k1), _native.ptr(k1), _native.ptr(side), _native.ptr(clen), _native.ptr(cons),
                                               int(W), int(K), int(M), *[_native.ptr(o) for o in out]))
    return tuple(out)


def align_counter(counter, reference, W=DEFAULT_WINDOW, K=DEFAULT_COLS, M=DEFAULT_MISMATCH):
    """``tdt_clip_align`` + ``tdt_clip_align_rows``: the rows of the counter's last finish, where they lie in HBM -> (uint64[SIZE] with
    ``mated`` still 0: rule 5 is the host's, the five columns of ``ALIGN_DTYPES``, the kernel's device milliseconds)"""
    lib = counter.ctx.lib
    sn = numpy.zeros(SIZE, dtype=numpy.uint64)
    _native.check(lib.tdt_clip_align(counter.handle, reference.handle, int(W), int(K), int(M), _native.ptr(sn)))
    n = ctypes.c_size_t(int(sn[0]))
    out = [numpy.zeros(n.value, dtype=dt) for dt in ALIGN_DTYPES]
    if n.value:
        _native.check(lib.tdt_clip_align_rows(counter.handle, *[_native.ptr(o) for o in out], ctypes.byref(n)))
    ms = ctypes.c_double(0)
    _native.check(lib.tdt_clip_align_timing(counter.handle, ctypes.byref(ms)))
    return sn, tuple(out), ms.value


# ------------------------------------------------------------------------------------------- the file
def write_file(path, counts, rows, names, W, K, M):
    """``{o}.clips.align.tab`` (see the module docstring); rows: those of :func:`summarise`"""
    c = [int(v) for v in numpy.asarray(counts).tolist()]
    dot = lambda v: "." if v is None else str(v)
    out = ["# tiddit_amd clips_align v1 window=%d min_cols=%d max_mismatch=%d\n" % (W, K, M)]
    out += ["SN\t%s\t%d\n" % (k, c[i]) for i, k in enumerate(SN)]
    out.append(COLUMNS)
    for tid, P, side, sup, clen, Q, strand, mm, hits, typ, ln, mate, hom in rows:
        chrom = names[tid] if tid < len(names) else str(tid)
        out.append("%s\t%d\t%s\t%d\t%d\t%s\t%s\t%s\t%d\t%s\t%s\t%s\t%s\n" % (chrom, P, "LR"[side], sup, clen, dot(Q), "." if strand is None else "+-"[strand],
                                                                           dot(mm), hits, dot(typ), dot(ln), dot(mate), dot(hom)))
    with open(path, "w") as f:
        f.write("".join(out))


def summary_line(counts):
    c = numpy.asarray(counts)
    return "clips align: {} sites, {} searched, {} aligned ({} ambiguous), {} unaligned, ref {}, del {}, dup {}, inv {}, mated {}".format(
        *(int(c[SN_INDEX[k]]) for k in ("sites", "searched", "aligned", "ambiguous", "unaligned", "ref", "del", "dup", "inv", "mated")))


def main(counter, clip_rows, reference, prefix, names, W, K, M, rows_out=None):
    """the stage behind the clip counter's finish and in front of its close: the search on the device over the rows where they lie,
    rule 5 on the host and the file -> the counters (:func:`summary_line`); ``clip_rows``: the columns ``counter.rows()`` gave;
    ``rows_out``: None, or a list that receives the rows of :func:`summarise` (tiddit_clip_vcf.py joins them)"""
    STAGE_SECONDS.clear()
    t = time.time()
    sn, placed, ms = align_counter(counter, reference, W, K, M)
    STAGE_SECONDS["clip align (device: one workgroup per site over the packed reference)"] = time.time() - t
    STAGE_SECONDS["  clip align kernel (device time)"] = ms * 1e-3
    t = time.time()
    k1, side, sup, _, _, clen = (numpy.asarray(v).tolist() for v in clip_rows[:6])
    counts, rows = summarise(list(zip(k1, side, sup, clen)), list(zip(*(p.tolist() for p in placed))), M)
    if not numpy.array_equal(counts[:SN_INDEX["mated"]], sn[:SN_INDEX["mated"]]):
        raise RuntimeError("tdt_clip_align: the device's counters {} differ from the rows' {}".format(sn.tolist(), counts.tolist()))
    write_file(prefix + ".clips.align.tab", counts, rows, names, W, K, M)
    if rows_out is not None:
        rows_out.extend(rows)
    STAGE_SECONDS["clip align mates + table text (host)"] = time.time() - t
    return counts
