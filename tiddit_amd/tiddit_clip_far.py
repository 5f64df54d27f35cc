"""Clip-site consensus placed genome-wide by a seeded search (``TIDDIT_CLIPS_FAR=1`` / ``K`` / ``K:M``, valid only together with
``TIDDIT_CLIPS``, independent of ``TIDDIT_CLIPS_ALIGN``): for every reported clip site of ``{o}.clips.tab`` whose consensus has at least
``K`` columns, the best placement of that consensus on ANY loaded contig, on either strand, whose first 16 columns match the reference
exactly, and the event the junction implies (BND on another contig; REF / DEL / DUP / INV with its length on the site's own), written
to ``{o}.clips.far.tab``.  These are the placements tiddit_clip_align.py's window cannot reach: translocations, dispersed duplications
and large rearrangements, and clips that place many times (mobile elements).  The search is exact in the seed and turned around
against the windowed one, on the device (csrc/tdt_clip_far.hip: the packed reference of refseq.py streams once against a sorted seed
table of the sites; the site rows of the clip counter's last finish where they lie in HBM).  The definition below is the specification,
:func:`place_site` implements it site by site and :func:`summarise` over the job.

The switch: ``K`` is the minimum consensus columns (``CLEN``) for a site to be searched, 16 ... 28, default 20; ``M`` the most mismatches
an accepted placement has outside its seed, 0 ... 12, default 2.  A bare ``1`` means the defaults (a ``K`` of 1 does not exist).

The notation is tiddit_clip_align.py's: a site is ``tid``, ``P`` (1-based), ``side`` (0 = L, 1 = R), ``CLEN`` and the consensus columns
``c_0 ... c_{CLEN-1}`` OUTWARD from the breakpoint, A C G T = 0 1 2 3.  ``len_t`` is the length of contig ``t``, ``ref[t][q]`` its 4-bit code
at 1-based ``q`` (refseq.CODES); a code that is not A, C, G or T equals no consensus base.

  1. STATUS.  ``CLEN < K``: ``short_consensus``.  Otherwise the site's own contig is not loaded, or ``P`` is outside ``1 ... len``:
        ``off_reference``.  Otherwise the site is ``searched``.
  2. CANDIDATES.  A candidate is ``(t, Q, strand)`` for every loaded contig ``t`` (the site's own included), every ``1 <= Q <= len_t`` and
        ``strand`` 0 (forward) or 1 (reverse complement).  Column ``j`` is compared with ``ref[t][Q + j]`` (ASCENDING) for (R, forward) and
        (L, reverse), with ``ref[t][Q - j]`` (DESCENDING) for (R, reverse) and (L, forward); with that base itself on the forward strand
        and with its complement on the reverse strand: rule 2 of tiddit_clip_align.py.  All ``CLEN`` bases must lie inside
        ``1 ... len_t``.  The SEED, columns ``0 ... 15``, must match exactly.  ``mm`` is the number of differing columns among
        ``16 ... CLEN - 1``.  The exact seed is a stated limit of this stage: a placement with a mismatch in its first 16 columns does not
        exist here.
  3. BEST and HITS.  ``HITS`` is the number of candidates with ``mm <= M``.  The best candidate is the minimum over those of
        ``(mm, t != tid, |Q - P| if t == tid else 0, strand, t, Q)``: fewest mismatches, then the site's own contig, then the nearest
        placement.  No such candidate: ``unplaced``.  Otherwise ``placed``; ``HITS > 1`` also counts as ``ambiguous``.
  4. TYPE / LEN of a placed site.  Another contig: ``BND``, ``LEN`` ``.``.  The site's own: ``tiddit_clip_align.type_of`` (REF / DEL /
        DUP / INV and its length).  A placed site also counts as ``same_contig`` or ``other_contig``, and as ``reverse`` on strand 1.
  5. MATES (host side, over the few rows).  A forward-strand row ``r`` of side R and a forward-strand row ``o`` of side L are mates when
        ``r``'s partner contig is ``o``'s contig and ``o``'s partner contig is ``r``'s, ``h = r.PARTNER - o.POS`` equals
        ``r.POS - o.PARTNER`` and ``0 <= h <= 28``; ``h`` is ``HOM``, the junction's microhomology: each aligner extends its reads through
        it, so both junction sites shift by it.  The one rule covers BND, DEL and DUP.  A row takes the mate with the smallest ``HOM``,
        then the smaller ``(contig, POS)``; mating is reported from both rows, each by its own choice.  Reverse-strand rows are NOT mated.

``{o}.clips.far.tab``: ``# tiddit_amd clips_far v1 seed=16 min_cols=K max_mismatch=M``, then ``SN name n`` for the eleven counters in the
order of ``SN``, then ``#CHROM POS SIDE SUPPORT CLEN PCHROM PARTNER STRAND MISMATCH HITS TYPE LEN MATE_CHROM MATE HOM`` and one row per
SEARCHED site, in the order of ``{o}.clips.tab``, all tab-separated, ``.`` where there is nothing (an unplaced site has no partner).

A site whose consensus places nowhere is sequence the reference does not hold: two such sites that face each other are an insertion,
which tiddit_clip_ins.py (``TIDDIT_CLIPS_INS``) pairs and closes from up to 140 clipped columns per side.

NOT built: mismatches inside the seed (spaced or multiple seeds), gapped placements, searching with more than the 28 consensus columns
(the 140 of ``TIDDIT_CLIPS_INS`` are not searched), mates of reverse-strand rows, joining the rows to the SV candidates of ``{o}.vcf`` (tiddit_clip_vcf.py,
``TIDDIT_CLIPS_VCF``, writes the mated BND / DEL / DUP rows as genotyped records of their own file, ``{o}.clips.vcf``), N ranks.
"""
import ctypes
import time

import numpy

from . import _native
from .tiddit_clip_align import type_of

COLS = 28
SEED = 16
MAX_MISMATCH = COLS - SEED
DEFAULT_COLS, DEFAULT_MISMATCH = 20, 2
MAX_HOM = 28
SN = ("sites", "short_consensus", "off_reference", "searched", "placed", "ambiguous", "unplaced", "same_contig", "other_contig", "reverse", "mated")
SN_INDEX = {k: i for i, k in enumerate(SN)}
SIZE = len(SN)
COLUMNS = "#CHROM\tPOS\tSIDE\tSUPPORT\tCLEN\tPCHROM\tPARTNER\tSTRAND\tMISMATCH\tHITS\tTYPE\tLEN\tMATE_CHROM\tMATE\tHOM\n"
SHORT_CONSENSUS, OFF_REFERENCE, SEARCHED = 0, 1, 2               # the status column
NO_MM = 0xffffffff                                               # the mismatch column of a site that is not placed (contig and PARTNER are 0 then)
FAR_DTYPES = (numpy.uint32,) * 6                                 # status, the partner's contig, PARTNER, strand, mismatches, HITS
STAGE_SECONDS = {}
_TO_BASE = bytes(({1: 0, 2: 1, 4: 2, 8: 3}).get(c, 4) for c in range(256))     # a reference code -> 0 ... 3, or 4 for what is no base


def parse_switch(value, clips=True):
    """``TIDDIT_CLIPS_FAR`` -> None (unset or empty) or (K, M); ValueError (its text is the error line) for anything else; ``clips``:
    whether ``TIDDIT_CLIPS`` is on"""
    if value is None or value == "":
        return None
    if not clips:
        raise ValueError("the switch places the sites of TIDDIT_CLIPS, which is not set")
    if value == "1":
        return DEFAULT_COLS, DEFAULT_MISMATCH
    parts = value.split(":")
    if len(parts) > 2 or not all(p.isascii() and p.isdigit() and len(p) <= 9 for p in parts):
        raise ValueError("the switch is 1, K or K:M (minimum consensus columns 16 ... 28, maximum mismatches 0 ... 12)")
    k = int(parts[0])
    m = int(parts[1]) if len(parts) == 2 else DEFAULT_MISMATCH
    if not SEED <= k <= COLS:
        raise ValueError("the minimum consensus columns are 16 ... 28")
    if not 0 <= m <= MAX_MISMATCH:
        raise ValueError("the maximum mismatches are 0 ... 12")
    return k, m


# ------------------------------------------------------------------------------------------- the definition
def _bases(ref):
    """every loaded contig of a refseq.HostReference as bytes of 0 ... 3 and 4 (no base), made once per reference"""
    cache = getattr(ref, "_far_bases", None)
    if cache is None:
        cache = ref._far_bases = {t: c.tobytes().translate(_TO_BASE) for t, c in sorted(ref.contigs.items())}
    return cache


def place_site(ref, tid, P, side, clen, cons, K=DEFAULT_COLS, M=DEFAULT_MISMATCH):
    """THE DEFINITION, one site -> (status, the partner's contig, PARTNER, strand, mm, HITS): rules 1 to 3.  ``ref``: a
    refseq.HostReference (``length(tid)``, -1: not loaded; ``contigs``); ``cons`` holds column j in bits 2j + 1 : 2j.  A site that is not
    placed has contig, PARTNER and strand 0, mm ``NO_MM`` and HITS 0.  The candidates of rule 2 are enumerated by their seeds: every
    occurrence of the 16 seed bases, as the reading direction and the strand lay them over ascending reference bases, is looked up
    with ``bytes.find`` — which IS the exact seed — and only there the other columns are compared one by one."""
    none = (0, 0, 0, NO_MM, 0)
    if clen < K:
        return (SHORT_CONSENSUS,) + none
    ln = ref.length(tid)
    if ln < 0 or not 1 <= P <= ln:
        return (OFF_REFERENCE,) + none
    cols = [(cons >> (2 * j)) & 3 for j in range(clen)]
    best, hits = None, 0
    for t, text in _bases(ref).items():
        for strand in (0, 1):
            step = 1 if (side == 1) == (strand == 0) else -1
            want = [3 - c if strand else c for c in cols]                      # what ref[t][Q + step * j] must be
            seed = bytes(want[:SEED]) if step == 1 else bytes(want[:SEED][::-1])
            at = text.find(seed)
            while at >= 0:
                Q = at + 1 if step == 1 else at + SEED                         # 1-based; descending, the seed's bases are Q - 15 ... Q
                last = Q + step * (clen - 1)
                if 1 <= last <= len(text):
                    mm = sum(text[Q + step * j - 1] != want[j] for j in range(SEED, clen))
                    if mm <= M:
                        hits += 1
                        key = (mm, int(t != tid), abs(Q - P) if t == tid else 0, strand, t, Q)
                        if best is None or key < best:
                            best = key
                at = text.find(seed, at + 1)
    if best is None:
        return (SEARCHED,) + none
    return SEARCHED, best[4], best[5], best[3], best[0], hits


def summarise(sites, placed, M=DEFAULT_MISMATCH):
    """THE DEFINITION, the whole job: ``sites`` = [(K1, side, SUPPORT, CLEN)] in the order of ``{o}.clips.tab``, ``placed`` = every
    site's (status, contig, PARTNER, strand, mm, HITS) -> (uint64[SIZE], rows): rows = [(tid, P, side, SUPPORT, CLEN, partner contig,
    PARTNER, strand, mm, HITS, TYPE, LEN, mate contig, MATE, HOM)] of the searched sites, in that order; None where the file writes ``.``"""
    c = numpy.zeros(SIZE, dtype=numpy.uint64)
    add = lambda k: c.__setitem__(SN_INDEX[k], c[SN_INDEX[k]] + numpy.uint64(1))
    rows = []
    for (k1, side, sup, clen), (status, pt, Q, strand, mm, hits) in zip(sites, placed):
        k1, side, pt, Q, strand, mm, hits = int(k1), int(side), int(pt), int(Q), int(strand), int(mm), int(hits)
        add("sites")
        add(("short_consensus", "off_reference", "searched")[status])
        if status != SEARCHED:
            continue
        tid, P = k1 >> 32, k1 & 0xffffffff
        have = mm != NO_MM and mm <= M
        typ = ln = None
        if have:
            add("placed")
            if hits > 1:
                add("ambiguous")
            add("same_contig" if pt == tid else "other_contig")
            if strand:
                add("reverse")
            typ, ln = type_of(P, side, Q, strand) if pt == tid else ("BND", None)
        else:
            add("unplaced")
        rows.append([tid, P, side, int(sup), int(clen)] + ([pt, Q, strand, mm] if have else [None] * 4) + [hits if have else 0, typ, ln, None, None, None])
    # rule 5: a site is one (contig, POS, side), so the mate with homology h, if any, is ONE row, found by its key: for an R row the L row
    # of its partner contig at PARTNER - h, for an L row the R row at PARTNER + h (sites come by the ten thousand: no loop over pairs)
    forward = {(r[0], r[1], r[2]): r for r in rows if r[10] is not None and not r[7]}
    for r in forward.values():
        sign = -1 if r[2] == 1 else 1
        for hom in range(MAX_HOM + 1):
            o = forward.get((r[5], r[6] + sign * hom, 1 - r[2]))
            if o is not None and o[5] == r[0] and o[6] == r[1] + sign * hom:
                r[12], r[13], r[14] = o[0], o[1], hom
                add("mated")
                break
    return c, [tuple(r) for r in rows]


# ------------------------------------------------------------------------------------------- the device entries
def _check_columns(k1, side, clen, cons):
    k1, cons = numpy.ascontiguousarray(k1, dtype=numpy.uint64), numpy.ascontiguousarray(cons, dtype=numpy.uint64)
    side, clen = numpy.ascontiguousarray(side, dtype=numpy.uint32), numpy.ascontiguousarray(clen, dtype=numpy.uint32)
    assert len(k1) == len(side) == len(clen) == len(cons)
    return k1, side, clen, cons


def far_sites(reference, k1, side, clen, cons, K=DEFAULT_COLS, M=DEFAULT_MISMATCH, ctx=None):
    """``tdt_clip_far_sites``: host columns of sites against ``reference`` (a refseq.RefSeq) -> the six columns of ``FAR_DTYPES``"""
    ctx = ctx or reference.ctx
    k1, side, clen, cons = _check_columns(k1, side, clen, cons)
    out = [numpy.zeros(len(k1), dtype=dt) for dt in FAR_DTYPES]
    _native.check(ctx.lib.tdt_clip_far_sites(ctx.handle, reference.handle, len(k1), _native.ptr(k1), _native.ptr(side), _native.ptr(clen), _native.ptr(cons),
                                             int(K), int(M), *[_native.ptr(o) for o in out]))
    return tuple(out)


def far_counter(counter, reference, K=DEFAULT_COLS, M=DEFAULT_MISMATCH):
    """``tdt_clip_far`` + ``tdt_clip_far_rows``: the rows of the counter's last finish, where they lie in HBM -> (uint64[SIZE] with
    ``mated`` still 0: rule 5 is the host's, the six columns of ``FAR_DTYPES``, float64[4] device milliseconds: seeds and filter, sort,
    scan, rows)"""
    lib = counter.ctx.lib
    sn = numpy.zeros(SIZE, dtype=numpy.uint64)
    _native.check(lib.tdt_clip_far(counter.handle, reference.handle, int(K), int(M), _native.ptr(sn)))
    n = ctypes.c_size_t(int(sn[0]))
    out = [numpy.zeros(n.value, dtype=dt) for dt in FAR_DTYPES]
    if n.value:
        _native.check(lib.tdt_clip_far_rows(counter.handle, *[_native.ptr(o) for o in out], ctypes.byref(n)))
    ms = numpy.zeros(4, dtype=numpy.float64)
    _native.check(lib.tdt_clip_far_timing(counter.handle, _native.ptr(ms)))
    return sn, tuple(out), ms


# ------------------------------------------------------------------------------------------- the file
def write_file(path, counts, rows, names, K, M):
    """``{o}.clips.far.tab`` (see the module docstring); rows: those of :func:`summarise`"""
    c = [int(v) for v in numpy.asarray(counts).tolist()]
    dot = lambda v: "." if v is None else str(v)
    name = lambda t: "." if t is None else names[t] if t < len(names) else str(t)
    out = ["# tiddit_amd clips_far v1 seed=%d min_cols=%d max_mismatch=%d\n" % (SEED, K, M)]
    out += ["SN\t%s\t%d\n" % (k, c[i]) for i, k in enumerate(SN)]
    out.append(COLUMNS)
    for tid, P, side, sup, clen, pt, Q, strand, mm, hits, typ, ln, mt, mate, hom in rows:
        out.append("%s\t%d\t%s\t%d\t%d\t%s\t%s\t%s\t%s\t%d\t%s\t%s\t%s\t%s\t%s\n" % (name(tid), P, "LR"[side], sup, clen, name(pt), dot(Q), "." if strand is None else "+-"[strand],
                                                                                 dot(mm), hits, dot(typ), dot(ln), name(mt), dot(mate), dot(hom)))
    with open(path, "w") as f:
        f.write("".join(out))


def summary_line(counts):
    c = numpy.asarray(counts)
    return "clips far: {} sites, {} searched, {} placed ({} ambiguous), {} unplaced, same contig {}, other contig {}, reverse {}, mated {}".format(
        *(int(c[SN_INDEX[k]]) for k in ("sites", "searched", "placed", "ambiguous", "unplaced", "same_contig", "other_contig", "reverse", "mated")))


def main(counter, clip_rows, reference, prefix, names, K, M, rows_out=None):
    """the stage behind the clip counter's finish and in front of its close: the search on the device over the rows where they lie,
    rule 5 on the host and the file -> the counters (:func:`summary_line`); ``clip_rows``: the columns ``counter.rows()`` gave;
    ``rows_out``: None, or a list that receives the rows of :func:`summarise` (tiddit_clip_vcf.py joins them)"""
    STAGE_SECONDS.clear()
    t = time.time()
    sn, placed, ms = far_counter(counter, reference, K, M)
    STAGE_SECONDS["clip far (device: seed table, sort, one scan of the packed reference, rows)"] = time.time() - t
    for k, v in zip(("seeds + filter", "sort", "scan", "rows"), ms.tolist()):
        STAGE_SECONDS["  clip far " + k + " (device time)"] = v * 1e-3
    t = time.time()
    k1, side, sup, _, _, clen = (numpy.asarray(v).tolist() for v in clip_rows[:6])
    counts, rows = summarise(list(zip(k1, side, sup, clen)), list(zip(*(p.tolist() for p in placed))), M)
    if not numpy.array_equal(counts[:SN_INDEX["mated"]], sn[:SN_INDEX["mated"]]):
        raise RuntimeError("tdt_clip_far: the device's counters {} differ from the rows' {}".format(sn.tolist(), counts.tolist()))
    write_file(prefix + ".clips.far.tab", counts, rows, names, K, M)
    if rows_out is not None:
        rows_out.extend(rows)
    STAGE_SECONDS["clip far mates + table text (host)"] = time.time() - t
    return counts
