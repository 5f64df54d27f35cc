"""Naming inserted sequences (``TIDDIT_CLIPS_MEI=library.fa``, valid only together with ``TIDDIT_CLIPS`` and ``TIDDIT_CLIPS_INS``;
``TIDDIT_CLIPS_MEI_MIN=A``, valid only with it): the sequences of ``{o}.clips.ins.tab`` — a CLOSED pair's ``SEQ``, an OPEN pair's two
flanks — are aligned WITH GAPS to every sequence of a family library (Alu, L1, SVA, HERV-K consensus, say) on both strands, and the
best family, its strand, score and spans are written to ``{o}.clips.mei.tab``.  A consensus assembled from reads against a family
consensus tens of millions of years diverged does not align without gaps; every other placement of the clip stages is an ungapped
window.  The reference answers this class with ``bwa`` and a local assembly; this is an integer definition with a unique result and no
second pass over the BAM.  The definition below is the specification, :func:`align` implements rule 3 cell by cell,
:func:`align_batch` the same by anti-diagonals over many queries at once, :func:`best_of_query` rule 4 and :func:`summarise` the
counters; the device path is csrc/tdt_swalign.hip.

The switch: a FASTA read through fasta.py (the ``.fai`` is written when missing) of 1 ... 4096 sequences of 1 ... 2^20 bases, 2^20
in all — the work is ``queries x 2 strands x library bases x query length`` cell updates, and a 20-kb library of family consensus is the
intended use.  Letters in either case map to BAM's 4-bit code, every other byte to 15.  ``A`` is the minimum score of a NAMED query,
12 ... 280, default 30.

  1. QUERIES.  Every row of ``{o}.clips.ins.tab`` gives queries, in reference direction, in the order of the rows: a ``CLOSED`` row
        one, ``SEQ`` (``PART=SEQ``, 8 ... 272 bases); an ``OPEN`` row two, ``LEFT_SEQ`` (``PART=LEFT``) then ``RIGHT_SEQ``
        (``PART=RIGHT``, 10 ... 140 bases each).  Queries are A C G T = 0 1 2 3 by construction.
  2. SCORES, bwa-mem's integers: a match +1, a mismatch -4, a gap of ``k`` bases on either side ``-(6 + k)``; a library base that is
        not A C G T scores -1 against anything.
  3. ONE LOCAL ALIGNMENT PROBLEM per (query, strand, family).  Strand ``-`` aligns the reverse complement of the query to the family
        as written.  With ``i`` the 0-based family base and ``j`` the 0-based base of the (reverse-complemented) query, the three Gotoh
        matrices ``H``, ``E``, ``F`` hold one integer KEY each: ``score << 32 | (2^32 - 1 - (fstart << 9 | qstart))``, ``(fstart,
        qstart)`` the cell where the alignment began.  Adding a score ``s`` adds ``s << 32``.  A value whose score is ``<= 0`` is EMPTY
        (0) in all three matrices, and so is everything outside the matrices.
          E[i][j] = max(H[i-1][j] - 7, E[i-1][j] - 1)        a gap that skips family bases
          F[i][j] = max(H[i][j-1] - 7, F[i][j-1] - 1)        a gap that skips query bases
          D[i][j] = (H[i-1][j-1], or when that is EMPTY the key of score 0 that starts at (i, j)) + s(i, j)
          H[i][j] = max(D[i][j], E[i][j], F[i][j])
        The maximum of keys is the larger score, then the smaller family start, then the smaller query start: every tie inside the
        recurrence is decided by integer comparison, not by evaluation order.  The problem's result is the maximum over all cells
        of ``(H key, -fend, -qend)``: among equal keys the smaller end in the family, then in the query.  No positive cell: nothing.
  4. A QUERY'S RESULT is the best problem result by (score descending, family index ascending, strand ``+`` before ``-``).
        ``SECOND`` / ``SECOND_FAMILY`` is the best score among the OTHER families on either strand and the smallest family index
        that has it, or ``0`` / ``.``.  The query is NAMED when ``SCORE >= A``; otherwise ``FAMILY`` and the columns behind it are
        ``.``.  ``QSTART`` / ``QEND`` are 1-based in the query as the file writes it (converted back for strand ``-``), ``FSTART`` /
        ``FEND`` 1-based in the family.
  5. THE FILE ``{o}.clips.mei.tab``: ``# tiddit_amd clips_mei v1 match=1 mismatch=4 gap_open=6 gap_extend=1 other=1 min_score=A
        families=n bases=N``, then ``SN name n`` for the ten counters in the order of ``SN`` (``ambiguous``: named with ``SECOND ==
        SCORE``), then ``#CHROM POS END STATUS PART QLEN FAMILY STRAND SCORE QSTART QEND FSTART FEND SECOND SECOND_FAMILY`` and one
        row per query, all tab-separated.
  6. A PAIR'S CALL, used by ``{o}.clips.vcf`` and counted in ``pairs_named`` / ``pairs_conflict``.  A ``CLOSED`` pair's call is its
        query's result.  An ``OPEN`` pair is named when at least one part is named and the named parts agree in family and strand: its
        score is the larger one and its span ``min FSTART, max FEND``.  Two named parts that disagree are a conflict, not a name.

The kernel does not cut a family into chunks: one wavefront walks a whole family, so the only block size in it is the 64 family
codes a wave takes at a time, and rule 3 is computed as written.

NOT built: seeds or filters that would make large libraries affordable; a traceback (CIGAR, identity); one-sided sites; gapped
placement of the site consensus against the genome; poly-A handling; subfamily resolution beyond ``SECOND``; N ranks (refused with
``TIDDIT_CLIPS``).
"""
import ctypes
import os
import time

import numpy

from . import _native
from .tiddit_clip_ins import CLOSED, SEQ_WORDS, pack_words

MATCH, MISMATCH, GAP_OPEN, GAP_EXTEND, OTHER = 1, 4, 6, 1, 1
QMAX = 280
MIN_SCORE_LO, DEFAULT_MIN_SCORE = 12, 30
LIB_MAX_SEQS, LIB_MAX_BASES = 4096, 1 << 20
POS_BITS = 9
NONE = 0xffffffff                                                # a family column without a family
PART_SEQ, PART_LEFT, PART_RIGHT = 0, 1, 2
PARTS = ("SEQ", "LEFT", "RIGHT")
SN = ("queries", "closed_queries", "left_queries", "right_queries", "named", "unnamed", "reverse", "ambiguous", "pairs_named", "pairs_conflict")
SN_INDEX = {k: i for i, k in enumerate(SN)}
SIZE = len(SN)
COLUMNS = "#CHROM\tPOS\tEND\tSTATUS\tPART\tQLEN\tFAMILY\tSTRAND\tSCORE\tQSTART\tQEND\tFSTART\tFEND\tSECOND\tSECOND_FAMILY\n"
RESULT_COLUMNS = 9                                               # family, strand, score, qstart, qend, fstart, fend, second, second_family
STAGE_SECONDS = {}
_ONE = 1 << 32
_ACGT = (1, 2, 4, 8)


def library_index(path):
    """the library's (FastaFile, names, lengths); ValueError (its text is the error line) for a file that cannot be read or a library
    outside the limits"""
    from .fasta import FastaFile
    if not os.path.isfile(path) or not os.access(path, os.R_OK):
        raise ValueError("the library FASTA cannot be read")
    try:
        fasta = FastaFile(path)
    except Exception as e:
        raise ValueError("the library FASTA cannot be indexed: %s" % e)
    names = list(fasta.references)
    lengths = [fasta.index[n][0] for n in names]
    if not 1 <= len(names) <= LIB_MAX_SEQS:
        raise ValueError("the library has %d sequences (1 ... 4096)" % len(names))
    if len(set(names)) != len(names):
        raise ValueError("the library has two sequences of one name")
    for n, ln in zip(names, lengths):
        if not 1 <= ln <= LIB_MAX_BASES:
            raise ValueError("library sequence %s has %d bases (1 ... 2^20)" % (n, ln))
    if sum(lengths) > LIB_MAX_BASES:
        raise ValueError("the library has %d bases (at most 2^20)" % sum(lengths))
    return fasta, names, lengths


def parse_switch(value, min_value=None, clips=True, ins=True):
    """``TIDDIT_CLIPS_MEI`` and ``TIDDIT_CLIPS_MEI_MIN`` -> None (both unset or empty) or (path, A); ValueError (its text is the error
    line) for anything else; ``clips`` / ``ins``: whether ``TIDDIT_CLIPS`` / ``TIDDIT_CLIPS_INS`` are on"""
    if value is None or value == "":
        if min_value is not None and min_value != "":
            raise ValueError("the minimum score belongs to TIDDIT_CLIPS_MEI, which is not set")
        return None
    if not clips:
        raise ValueError("the switch names the insertions of TIDDIT_CLIPS and TIDDIT_CLIPS_INS, and TIDDIT_CLIPS is not set")
    if not ins:
        raise ValueError("the switch names the insertions of TIDDIT_CLIPS_INS, which is not set")
    A = DEFAULT_MIN_SCORE
    if min_value is not None and min_value != "":
        if not (min_value.isascii() and min_value.isdigit() and len(min_value) <= 9):
            raise ValueError("TIDDIT_CLIPS_MEI_MIN=%s: the minimum score is a number 12 ... 280" % min_value)
        A = int(min_value)
        if not MIN_SCORE_LO <= A <= QMAX:
            raise ValueError("TIDDIT_CLIPS_MEI_MIN=%s: the minimum score is 12 ... 280" % min_value)
    library_index(value)
    return value, A


# ------------------------------------------------------------------------------------------- the definition
def codes_of_text(text):
    """a query's text -> codes 0 ... 3"""
    return ["ACGT".index(c) for c in text]


def reverse_complement(codes):
    return [3 - c for c in reversed(codes)]


def _less(k, pen):
    return k - pen * _ONE if k >= (pen + 1) * _ONE else 0


def align(query, family):
    """THE DEFINITION, rule 3, one problem: ``query`` = codes 0 ... 3 of the strand's query, ``family`` = 4-bit codes -> (key, fend,
    qend), 0-based, or (0, None, None) without a positive cell"""
    n, m = len(query), len(family)
    best = (0, None, None)
    Hp, Ep = [0] * n, [0] * n                                    # the row above
    for i in range(m):
        fc = int(family[i])
        pen = MISMATCH if fc in _ACGT else OTHER
        H, E = [0] * n, [0] * n
        f = h_left = 0
        for j in range(n):
            e = max(_less(Hp[j], GAP_OPEN + GAP_EXTEND), _less(Ep[j], GAP_EXTEND))
            f = max(_less(h_left, GAP_OPEN + GAP_EXTEND), _less(f, GAP_EXTEND))
            d0 = (Hp[j - 1] if j else 0) or NONE - (i << POS_BITS | j)
            d = d0 + MATCH * _ONE if fc == 1 << query[j] else _less(d0, pen)
            h = max(d, e, f)
            H[j], E[j], h_left = h, e, h
            if h > best[0]:                                      # (the cells ascend by (i, j): a strict > keeps the smaller end)
                best = (h, i, j)
        Hp, Ep = H, E
    return best


def align_batch(queries, family):
    """rule 3 for many queries against one family, by anti-diagonals in numpy: the same integers as :func:`align` ->
    [(key, fend, qend)]"""
    B, m = len(queries), len(family)
    if not B:
        return []
    lens = numpy.array([len(q) for q in queries], dtype=numpy.int64)
    N = max(int(lens.max()), 1)
    hot = numpy.zeros((B, N), dtype=numpy.int64)                 # one-hot 4-bit code per column, 0 behind a query's end
    for b, q in enumerate(queries):
        hot[b, :len(q)] = 1 << numpy.asarray(q, dtype=numpy.int64) if len(q) else 0
    fam = numpy.asarray(family, dtype=numpy.int64)
    fam_pen = numpy.where((fam == 1) | (fam == 2) | (fam == 4) | (fam == 8), MISMATCH, OTHER).astype(numpy.int64)
    cols = numpy.arange(N, dtype=numpy.int64)
    Z = numpy.zeros((B, N), dtype=numpy.int64)
    H1, H2, E1, F1 = Z.copy(), Z.copy(), Z.copy(), Z.copy()
    bestk, besti = Z.copy(), Z.copy()
    less = lambda k, pen: numpy.where(k >= (pen + 1) * _ONE, k - pen * _ONE, 0)
    shift = lambda a: numpy.concatenate([numpy.zeros((B, 1), dtype=numpy.int64), a[:, :-1]], axis=1)
    for d in range(m + N - 1):
        i = d - cols
        valid = (i >= 0) & (i < m)
        ic = numpy.clip(i, 0, m - 1)
        e = numpy.maximum(less(H1, GAP_OPEN + GAP_EXTEND), less(E1, GAP_EXTEND))
        f = numpy.maximum(less(shift(H1), GAP_OPEN + GAP_EXTEND), less(shift(F1), GAP_EXTEND))
        dg = shift(H2)
        d0 = numpy.where(dg != 0, dg, NONE - (ic << POS_BITS | cols))
        dv = numpy.where(hot == fam[ic], d0 + MATCH * _ONE, less(d0, fam_pen[ic]))
        h = numpy.maximum(dv, numpy.maximum(e, f))
        h, e, f = (numpy.where(valid, a, 0) for a in (h, e, f))
        better = h > bestk
        bestk = numpy.where(better, h, bestk)
        besti = numpy.where(better, ic, besti)
        H2, H1, E1, F1 = H1, h, e, f
    out = []
    for b in range(B):
        n = int(lens[b])
        k = bestk[b, :n]
        if n == 0 or int(k.max()) == 0:
            out.append((0, None, None))
            continue
        top = int(k.max())
        at = [(int(besti[b, j]), j) for j in range(n) if int(k[j]) == top]
        out.append((top,) + min(at))
    return out


def best_of_query(problems, n):
    """rule 4: ``problems`` = {(family, strand): (key, fend, qend)} of one query of ``n`` bases -> the nine result columns (family,
    strand, score, qstart, qend, fstart, fend, second, second_family); ``NONE`` for a family that is not there, zeros behind it"""
    best = None
    for (f, s), (key, fend, qend) in problems.items():
        if key >> 32 and (best is None or (-(key >> 32), f, s) < best[0]):
            best = ((-(key >> 32), f, s), key, fend, qend)
    if best is None:
        return (NONE, 0, 0, 0, 0, 0, 0, 0, NONE)
    (_, f, s), key, fend, qend = best
    start = NONE - (key & NONE)
    fs, qs = start >> POS_BITS, start & ((1 << POS_BITS) - 1)
    second, second_family = 0, NONE
    for (f2, _), (k2, _, _) in sorted(problems.items()):
        if f2 != f and k2 >> 32 > second:
            second, second_family = k2 >> 32, f2
    qstart, qend1 = (n - qend, n - qs) if s else (qs + 1, qend + 1)
    return (f, s, key >> 32, qstart, qend1, fs + 1, fend + 1, second, second_family)


def results(queries, library):
    """rules 3 and 4 over a table: ``queries`` = [codes 0 ... 3], ``library`` = [4-bit codes per family] -> [the nine columns]"""
    per = [{} for _ in queries]
    both = [q for q in queries] + [reverse_complement(q) for q in queries]
    for f, fam in enumerate(library):
        r = align_batch(both, fam)
        for qi in range(len(queries)):
            per[qi][(f, 0)], per[qi][(f, 1)] = r[qi], r[len(queries) + qi]
    return [best_of_query(p, len(q)) for p, q in zip(per, queries)]


def pair_call(named_parts):
    """rule 6: the NAMED results of a pair's parts (one or two of the nine columns) -> ("named", (family, strand, score, fstart, fend)),
    ("conflict", None) or (None, None)"""
    if not named_parts:
        return None, None
    if len({(r[0], r[1]) for r in named_parts}) > 1:
        return "conflict", None
    return "named", (named_parts[0][0], named_parts[0][1], max(r[2] for r in named_parts), min(r[5] for r in named_parts), max(r[6] for r in named_parts))


def summarise(res, parts, A, pairs=None):
    """the counters: ``res`` = the nine columns per query, ``parts`` = every query's part, ``pairs`` = every query's pair row (None:
    every query is a pair of its own) -> (uint64[SIZE], {pair row: the call of rule 6 for the named pairs})"""
    c = numpy.zeros(SIZE, dtype=numpy.uint64)
    add = lambda k, n=1: c.__setitem__(SN_INDEX[k], c[SN_INDEX[k]] + numpy.uint64(n))
    by_pair = {}
    for qi, (r, part) in enumerate(zip(res, parts)):
        named = r[2] >= A
        add("queries")
        add(("closed_queries", "left_queries", "right_queries")[part])
        add("named" if named else "unnamed")
        if named and r[1]:
            add("reverse")
        if named and r[7] == r[2]:
            add("ambiguous")
        by_pair.setdefault(qi if pairs is None else int(pairs[qi]), []).extend([r] if named else [])
    calls = {}
    for p, named_parts in by_pair.items():
        kind, call = pair_call(named_parts)
        if kind == "named":
            add("pairs_named")
            calls[p] = call
        elif kind == "conflict":
            add("pairs_conflict")
    return c, calls


def queries_of_rows(ins_rows):
    """rule 1: the rows of ``tiddit_clip_ins.file_rows`` -> [(row index, part, text)]"""
    out = []
    for p, row in enumerate(ins_rows):
        if row[8] == CLOSED:
            out.append((p, PART_SEQ, row[12]))
        else:
            out += [(p, PART_LEFT, row[13]), (p, PART_RIGHT, row[14])]
    return out


# ------------------------------------------------------------------------------------------- the device entries
def query_columns(queries):
    """[codes] -> (seq10 uint64[n][10], qlen uint32[n]) as the device entries take them"""
    n = len(queries)
    seq10 = numpy.array([pack_words(q, SEQ_WORDS) for q in queries], dtype=numpy.uint64).reshape(n, SEQ_WORDS)
    return seq10, numpy.array([len(q) for q in queries], dtype=numpy.uint32).reshape(n)


def sw_align(seq10, qlen, lib, A=DEFAULT_MIN_SCORE, ctx=None, device=False):
    """``tdt_sw_align`` (``device``: ``tdt_sw_align_device`` on torch copies of the arrays): host columns of queries and ``lib``, a
    refseq.RefSeq with every sequence loaded -> (uint64[SIZE], the nine uint32 columns)"""
    ctx = ctx or _native.default_context()
    lib_, P = ctx.lib, _native.ptr
    seq10, qlen = numpy.ascontiguousarray(seq10, dtype=numpy.uint64), numpy.ascontiguousarray(qlen, dtype=numpy.uint32)
    n = len(qlen)
    assert seq10.size == n * SEQ_WORDS
    if not device:
        sn = numpy.zeros(SIZE, dtype=numpy.uint64)
        cols = [numpy.zeros(n, dtype=numpy.uint32) for _ in range(RESULT_COLUMNS)]
        _native.check(lib_.tdt_sw_align(ctx.handle, lib.handle, n, P(seq10), P(qlen), int(A), P(sn), *[P(c) for c in cols]))
        return sn, tuple(cols)
    import torch
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a).view(numpy.uint8).reshape(-1).copy()).cuda() if a.size else torch.zeros(8, dtype=torch.uint8).cuda()
    d_in = [dev(seq10), dev(qlen)]
    d_sn = torch.zeros(SIZE * 8, dtype=torch.uint8).cuda()
    d_out = [torch.zeros(max(n, 1) * 4, dtype=torch.uint8).cuda() for _ in range(RESULT_COLUMNS)]
    torch.cuda.synchronize()
    _native.check(lib_.tdt_sw_align_device(ctx.handle, lib.handle, n, *[ctypes.c_void_p(t.data_ptr()) for t in d_in], int(A), ctypes.c_void_p(d_sn.data_ptr()),
                                           *[ctypes.c_void_p(t.data_ptr()) for t in d_out]))
    torch.cuda.synchronize()
    return d_sn.cpu().numpy().view(numpy.uint64).copy(), tuple(t.cpu().numpy().view(numpy.uint32)[:n].copy() for t in d_out)


def sw_align_timing(ctx=None):
    """ms of this thread's last :func:`sw_align`: [the alignment launch, the reduction]"""
    ctx = ctx or _native.default_context()
    ms = numpy.zeros(2, dtype=numpy.float64)
    _native.check(ctx.lib.tdt_sw_align_timing(_native.ptr(ms)))
    return ms


# ------------------------------------------------------------------------------------------- the file
def file_rows(ins_rows, pair, part, qlen, cols):
    """the rows of ``tiddit_clip_ins.file_rows`` and the queries' columns (pair row, part, length, the nine result columns) -> the file's
    rows [(tid, P_R, P_L, status, part, QLEN, family, strand, score, qstart, qend, fstart, fend, second, second_family)]"""
    cols = [numpy.asarray(c).tolist() for c in cols]
    out = []
    for qi, (p, pt, n) in enumerate(zip(numpy.asarray(pair).tolist(), numpy.asarray(part).tolist(), numpy.asarray(qlen).tolist())):
        row = ins_rows[p]
        out.append((row[0], row[1], row[2], row[8], pt, n) + tuple(c[qi] for c in cols))
    return out


def write_file(path, counts, rows, names, lib_names, lib_bases, A):
    """``{o}.clips.mei.tab`` (rule 5); rows: those of :func:`file_rows`; ``names``: the contigs', ``lib_names``: the families'"""
    c = [int(v) for v in numpy.asarray(counts).tolist()]
    out = ["# tiddit_amd clips_mei v1 match=%d mismatch=%d gap_open=%d gap_extend=%d other=%d min_score=%d families=%d bases=%d\n"
           % (MATCH, MISMATCH, GAP_OPEN, GAP_EXTEND, OTHER, A, len(lib_names), lib_bases)]
    out += ["SN\t%s\t%d\n" % (k, c[i]) for i, k in enumerate(SN)]
    out.append(COLUMNS)
    fam = lambda f: "." if f == NONE else lib_names[f] if f < len(lib_names) else str(f)
    for tid, PR, PL, status, part, n, f, s, score, qs, qe, fs, fe, second, sf in rows:
        chrom = names[tid] if tid < len(names) else str(tid)
        head = "%s\t%d\t%d\t%s\t%s\t%d\t" % (chrom, PR, PL, ("OPEN", "CLOSED")[status], PARTS[part], n)
        if score >= A:
            out.append(head + "%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (fam(f), "+-"[s], score, qs, qe, fs, fe, second, fam(sf)))
        else:
            out.append(head + "\t".join("." * RESULT_COLUMNS) + "\n")
    with open(path, "w") as f_:
        f_.write("".join(out))


def calls_for_vcf(rows, A, lib_names):
    """rule 6 over the file's rows -> {ins row index: (family name, "+" / "-", score, fstart, fend)} of the named pairs; the pairs are
    numbered as the distinct (tid, P_R, P_L) of the rows appear, which is the order of ``{o}.clips.ins.tab``"""
    res, parts, pairs, index = [], [], [], {}
    for r in rows:
        res.append(r[6:])
        parts.append(r[4])
        pairs.append(index.setdefault(r[:3], len(index)))
    _, calls = summarise(res, parts, A, pairs)
    return {p: (lib_names[f] if f < len(lib_names) else str(f), "+-"[s], score, fs, fe) for p, (f, s, score, fs, fe) in calls.items()}


def library_codes(fasta, lib_names):
    """the library as the definition reads it: [uint8[] of 4-bit codes per family]"""
    from .refseq import codes_of_bases
    return [codes_of_bases(fasta.fetch_array(n)) for n in lib_names]


def definition_file(path, ins_rows, names, library_path, A):
    """the file from the definition alone (what the tests compare a job's file with) -> (the counters, the rows of :func:`file_rows`)"""
    fasta, lib_names, lengths = library_index(library_path)
    qs = queries_of_rows(ins_rows)
    queries = [codes_of_text(t) for _, _, t in qs]
    res = results(queries, library_codes(fasta, lib_names))
    counts, _ = summarise(res, [pt for _, pt, _ in qs], A, [p for p, _, _ in qs])
    rows = file_rows(ins_rows, [p for p, _, _ in qs], [pt for _, pt, _ in qs], [len(q) for q in queries], list(zip(*res)) if res else [[]] * RESULT_COLUMNS)
    write_file(path, counts, rows, names, lib_names, sum(lengths), A)
    return counts, rows


def summary_line(counts):
    c = numpy.asarray(counts)
    return "clips mei: {} queries ({} closed, {} left, {} right), {} named ({} reverse, {} ambiguous), {} unnamed, {} pairs named, {} in conflict".format(
        *(int(c[SN_INDEX[k]]) for k in ("queries", "closed_queries", "left_queries", "right_queries", "named", "reverse", "ambiguous", "unnamed", "pairs_named",
                                        "pairs_conflict")))


def main(counter, ins_rows, prefix, names, library_path, A, rows_out=None):
    """the stage behind the INS stage and in front of the counter's close: the library into a handle of its own, the query build, the
    alignment and the reduction on the device over the pair rows where they lie, and the file -> the counters (:func:`summary_line`);
    ``ins_rows``: the rows of ``tiddit_clip_ins.file_rows``; ``rows_out``: None, or a list that receives the rows of :func:`file_rows`
    (tiddit_clip_vcf.py joins them).  The library is closed before the return."""
    from . import refseq
    STAGE_SECONDS.clear()
    t = time.time()
    fasta, lib_names, lengths = library_index(library_path)
    lib = refseq.load_all(fasta, ctx=counter.ctx)
    STAGE_SECONDS["clip mei library (read, upload, pack)"] = time.time() - t
    try:
        t = time.time()
        sn = counter.mei(lib, A)
        pair, part, qlen, cols = counter.mei_rows()
        ms = counter.mei_timing()
    finally:
        lib.close()
    STAGE_SECONDS["clip mei (device: query build, alignment, reduction)"] = time.time() - t
    for k, v in zip(("query build", "gapped alignment (one wavefront per query, strand and family)", "reduction"), ms.tolist()):
        STAGE_SECONDS["  clip mei " + k + " (device time)"] = v * 1e-3
    t = time.time()
    rows = file_rows(ins_rows, pair, part, qlen, cols)
    write_file(prefix + ".clips.mei.tab", sn, rows, names, lib_names, sum(lengths), A)
    if rows_out is not None:
        rows_out.extend(rows)
    STAGE_SECONDS["clip mei table text (host)"] = time.time() - t
    return sn
