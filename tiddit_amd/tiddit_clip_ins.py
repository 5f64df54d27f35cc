"""Insertion candidates from facing clip sites (``TIDDIT_CLIPS_INS=1`` / ``K`` / ``K:O`` / ``K:O:M``, valid only together with
``TIDDIT_CLIPS``; independent of ``TIDDIT_CLIPS_ALIGN`` and ``TIDDIT_CLIPS_FAR``, and no FASTA goes into HBM for it): sequence that is
not in the reference leaves an ``R`` site whose clipped bases are the START of the inserted sequence and, one base to its right (or a
little to its left, behind a target-site duplication), an ``L`` site whose clipped bases are its END.  Neither consensus places
anywhere, so ``{o}.clips.align.tab`` and ``{o}.clips.far.tab`` call both ``unplaced``.  Here the vote over the clipped bases is carried
from 28 to 140 columns, facing sites are paired, and the insertion is CLOSED where the two extended consensus overlap, written to
``{o}.clips.ins.tab``.  The reference answers this class with ``bwa`` and a local assembly; this is narrower, exact and
order-independent.  The definition below is the specification, :func:`extended_events_of_read` implements it read by read and
:func:`summarise` over the job; the device path is csrc/tdt_clip_ins.hip.

The switch: ``K`` is the minimum extended-consensus columns per side, 10 ... 140, default 20; ``O`` the minimum overlap of the two
consensus, 8 ... 140, default 12; ``M`` the maximum mismatches inside the overlap, 0 ... 8, default 1.  A bare ``1`` means the
defaults; a ``K`` of 1 cannot be written, because ``K`` starts at 10.

  1. EXTENDED EVENTS.  The reads, their eligibility, the malformed rules, the clip choice, ``P``, the side and ``rev`` are rules 1 to 4
        of tiddit_clips.py (``tiddit_clips.clips_of_read``).  Rule 5 continues to ``CLIP_EXT_COLS`` = 140 columns: bases are taken
        outward from the breakpoint while their 4-bit code is A C G T, up to ``min(cliplen, 140)``; ``n`` is the number kept.  The
        first 28 columns are exactly the event ``tiddit_clips`` keys.  ``28 <= n < min(cliplen, 140)`` adds 1 to
        ``SN cut_beyond_28`` (a cut in front of column 28 is ``tiddit_clips``' ``cut_at_other_base``).
  2. EXTENSION KEYS.  An event with ``n > 28`` gives one key per further CHUNK ``c = 1 ... 4`` of 28 columns that holds a base,
        ``n_c = min(n - 28 c, 28) >= 1``: ``K1 = c << 56 | tid << 32 | P`` (the tid has 24 bits: the top byte is free) and
        ``K2 = side << 63 | n_c << 58 | bases_c << 2 | rev`` in the layout of rule 6 of tiddit_clips.py, ``bases_c`` holding column
        ``28 c + j`` in bits ``2j + 1 : 2j``.  At most ``CLIP_EXT_MAX_PER_READ`` = 8 keys per read.  ``SN ext_left_events`` /
        ``ext_right_events`` count the events with a key, ``SN ext_keys`` the keys.
  3. EXTENDED CONSENSUS of a site ``(K1, side)`` with ``SUPPORT >= S`` (``S``: the minimum support of ``TIDDIT_CLIPS``): ``depth_j``
        is the number of events with ``n > j``, ``j`` in 0 ... 139; ``ECLEN`` the number of leading columns with ``depth_j >= S``; the
        base of a column is the vote's winner, ties going to the smaller code.  By construction columns 0 ... 27 equal ``CLEN`` /
        ``CONSENSUS`` of ``{o}.clips.tab``.  ``SN sites_extended`` counts the sites with ``ECLEN > 28``, ``SN left_sites`` /
        ``right_sites`` those with ``ECLEN >= K``.
  4. FACING PAIRS.  An ``R`` site at ``(t, P_R)`` and an ``L`` site at ``(t, P_L)`` with ``0 <= d = P_R + 1 - P_L <=
        CLIP_INS_MAX_TSD`` = 32, both with ``ECLEN >= K``.  Every such pair is a row; one site may appear in several rows.  Rows
        ascend by ``(t, P_R, P_L)``.  ``d`` is written as ``TSD``: a target-site duplication or a microhomology.  ``P_L > P_R + 1`` is
        not a pair here.
  5. CLOSURE.  ``x_0 ... x_{a-1}`` is the ``R`` consensus (``x_0`` the first base right of ``P_R``), ``y_0 ... y_{b-1}`` the ``L``
        consensus outward (``y_0`` the base just left of ``P_L``).  For an insertion of ``l`` bases ``y_j`` lies at coordinate
        ``l - 1 - j`` of ``x``'s axis; ``o(l) = min(a, l) - max(0, l - b)`` columns overlap and ``mm(l)`` is the number of ``i`` in
        the overlap with ``x_i != y_{l-1-i}``.  The candidates are ``l`` in ``O ... a + b - O``; one is ACCEPTED when ``o(l) >= O`` and
        ``mm(l) <= M``.  ``CLOSURES`` is the number of accepted ``l``, the best one the minimum of ``(mm, l)``.  A pair with an
        accepted ``l`` is ``CLOSED``: ``LEN = l``, ``SEQ[i] = x_i`` for ``i < min(a, l)``, else ``y_{l-1-i}``, ``MISMATCH = mm``.  A
        pair with none is ``OPEN``: ``LEN``, ``MISMATCH`` and ``SEQ`` are ``.``, and the two flanks are what is known of a longer
        insertion.  ``LEFT_SEQ`` is ``x`` and ``RIGHT_SEQ`` is ``y``, both in reference direction, on every row.
        A short tandem duplication is reported as the insertion it is: the duplicated copy's bases are clipped at both junctions
        exactly as novel bases would be, and nothing here looks into the reference to tell the two apart.

``{o}.clips.ins.tab``: ``# tiddit_amd clips_ins v1 cols=140 max_tsd=32 min_cols=K min_overlap=O max_mismatch=M``, then ``SN name n``
for the eleven counters in the order of ``SN``, then ``#CHROM POS END TSD R_SUPPORT L_SUPPORT R_COLS L_COLS STATUS LEN MISMATCH
CLOSURES SEQ LEFT_SEQ RIGHT_SEQ`` and one row per pair, all tab-separated.  ``POS = P_R``, ``END = P_L``.

NOT built: insertions with a deleted stretch (``P_L > P_R + 1``); one-sided sites; checking the consensus tails against the
reference; more than 140 columns; joining the rows to ``{o}.vcf`` (tiddit_clip_vcf.py, ``TIDDIT_CLIPS_VCF``, writes them as genotyped
records of their own file, ``{o}.clips.vcf``); N ranks (refused with ``TIDDIT_CLIPS``).  Naming the inserted sequences against a library of
mobile-element families is tiddit_clip_mei.py's (``TIDDIT_CLIPS_MEI``).
"""
import ctypes
import time

import numpy

from . import _native
from .tiddit_clips import CLIP_COLS, OK, clips_of_read, kept_bases

CLIP_EXT_COLS = 140
CLIP_EXT_WORDS = CLIP_EXT_COLS // CLIP_COLS                      # 5 words of 56 bits
CLIP_EXT_MAX_PER_READ = 8
CLIP_INS_MAX_TSD = 32
SEQ_WORDS = 10                                                   # a closed insertion has at most 2 * 140 - 8 bases: ten words of 28
MIN_COLS, MIN_OVERLAP, MAX_MISMATCH = 10, 8, 8
DEFAULT_COLS, DEFAULT_OVERLAP, DEFAULT_MISMATCH = 20, 12, 1
SN = ("ext_left_events", "ext_right_events", "ext_keys", "cut_beyond_28", "sites_extended", "left_sites", "right_sites", "pairs", "closed", "open",
      "closed_multi")
SN_INDEX = {k: i for i, k in enumerate(SN)}
SIZE = len(SN)
PUSH_SN = SN[:4]
COLUMNS = "#CHROM\tPOS\tEND\tTSD\tR_SUPPORT\tL_SUPPORT\tR_COLS\tL_COLS\tSTATUS\tLEN\tMISMATCH\tCLOSURES\tSEQ\tLEFT_SEQ\tRIGHT_SEQ\n"
PAIR_DTYPES = (numpy.uint32,) * 7                                # R row, L row, TSD, status, LEN, MISMATCH, CLOSURES (and uint64[10] SEQ words)
OPEN, CLOSED = 0, 1
STAGE_SECONDS = {}


def parse_switch(value, clips=True):
    """``TIDDIT_CLIPS_INS`` -> None (unset or empty) or (K, O, M); ValueError (its text is the error line) for anything else;
    ``clips``: whether ``TIDDIT_CLIPS`` is on"""
    if value is None or value == "":
        return None
    if not clips:
        raise ValueError("the switch pairs the sites of TIDDIT_CLIPS, which is not set")
    if value == "1":
        return DEFAULT_COLS, DEFAULT_OVERLAP, DEFAULT_MISMATCH
    parts = value.split(":")
    if len(parts) > 3 or not all(p.isascii() and p.isdigit() and len(p) <= 9 for p in parts):
        raise ValueError("the switch is 1, K, K:O or K:O:M (minimum extended-consensus columns 10 ... 140, minimum overlap 8 ... 140, maximum mismatches 0 ... 8)")
    k = int(parts[0])
    o = int(parts[1]) if len(parts) >= 2 else DEFAULT_OVERLAP
    m = int(parts[2]) if len(parts) == 3 else DEFAULT_MISMATCH
    if not MIN_COLS <= k <= CLIP_EXT_COLS:
        raise ValueError("the minimum extended-consensus columns are 10 ... 140")
    if not MIN_OVERLAP <= o <= CLIP_EXT_COLS:
        raise ValueError("the minimum overlap is 8 ... 140")
    if not 0 <= m <= MAX_MISMATCH:
        raise ValueError("the maximum mismatches are 0 ... 8")
    return k, o, m


# ------------------------------------------------------------------------------------------- the definition
def extended_events_of_read(flag, tid, pos, mapq, rec_off, raw, min_mapq=20, min_clip=10):
    """THE DEFINITION, rules 1 and 2, one read -> (events, ext_keys, cut): ``events`` = [(K1, side, rev, [codes outward, at most
    140])] of the read's clips (none unless the read is OK for ``tiddit_clips``), ``ext_keys`` = [(K1, K2)] of rule 2 in the order
    (leading clip first, chunks ascending), ``cut`` what the read adds to ``SN cut_beyond_28``"""
    kind, clips, _, base = clips_of_read(flag, tid, pos, mapq, rec_off, raw, min_mapq, min_clip)
    if kind != OK:
        return [], [], 0
    rev = (flag >> 4) & 1
    events, keys, cut = [], [], 0
    for side, P, cliplen, q0 in clips:
        kept = kept_bases(side, cliplen, q0, base, CLIP_EXT_COLS)
        n = len(kept)
        cut += int(CLIP_COLS <= n < min(cliplen, CLIP_EXT_COLS))
        events.append((tid << 32 | P, side, rev, kept))
        for c in range(1, CLIP_EXT_WORDS):
            chunk = kept[CLIP_COLS * c:CLIP_COLS * (c + 1)]
            if not chunk:
                break
            keys.append((c << 56 | tid << 32 | P, side << 63 | len(chunk) << 58 | sum(b << (2 * j) for j, b in enumerate(chunk)) << 2 | rev))
    return events, keys, cut


def events_of_batch_by_read(b, events, keys, sn, min_mapq=20, min_clip=10):
    """rules 1 and 2 over one batch, read by read: appends to ``events`` and ``keys`` and adds to the four push counters ``sn`` (a dict)"""
    from .bamio import _raw_of
    raw = _raw_of(b)
    for i in range(len(b.tid)):
        ev, ks, cut = extended_events_of_read(int(b.flag[i]), int(b.tid[i]), int(b.pos[i]), int(b.mapq[i]), int(b.rec_off[i]), raw, min_mapq, min_clip)
        events.extend(ev)
        keys.extend(ks)
        for k, v in (("ext_left_events", sum(1 for e in ev if e[1] == 0 and len(e[3]) > CLIP_COLS)),
                     ("ext_right_events", sum(1 for e in ev if e[1] == 1 and len(e[3]) > CLIP_COLS)), ("ext_keys", len(ks)), ("cut_beyond_28", cut)):
            if v:
                sn[k] = sn.get(k, 0) + v


def extended_sites(events, min_support):
    """rule 3: ``events`` of :func:`extended_events_of_read` in any order -> [(K1, side, SUPPORT, ECLEN, [winning codes])] of the sites
    with SUPPORT >= min_support, ascending by (K1, side)"""
    sites = {}
    for k1, side, _, kept in events:
        s = sites.setdefault((k1, side), [0, [[0, 0, 0, 0] for _ in range(CLIP_EXT_COLS)]])
        s[0] += 1
        for j, c in enumerate(kept):
            s[1][j][c] += 1
    out = []
    for (k1, side), (support, votes) in sorted(sites.items()):
        if support < min_support:
            continue
        eclen = 0
        while eclen < CLIP_EXT_COLS and sum(votes[eclen]) >= min_support:
            eclen += 1
        out.append((k1, side, support, eclen, [v.index(max(v)) for v in votes[:eclen]]))          # (the first of equal maxima: the smaller code)
    return out


def close_pair(x, y, O=DEFAULT_OVERLAP, M=DEFAULT_MISMATCH):
    """rule 5: the R consensus ``x`` and the L consensus ``y`` (codes, outward) -> (status, LEN, MISMATCH, CLOSURES, SEQ codes);
    LEN, MISMATCH 0 and SEQ [] for an OPEN pair"""
    a, b = len(x), len(y)
    best, closures = None, 0
    for l in range(O, a + b - O + 1):
        lo, hi = max(0, l - b), min(a, l)
        if hi - lo < O:
            continue
        mm = sum(1 for i in range(lo, hi) if x[i] != y[l - 1 - i])
        if mm <= M:
            closures += 1
            if best is None or (mm, l) < best:
                best = (mm, l)
    if best is None:
        return OPEN, 0, 0, 0, []
    mm, l = best
    return CLOSED, l, mm, closures, [x[i] if i < min(a, l) else y[l - 1 - i] for i in range(l)]


def pairs_of_sites(sites, K=DEFAULT_COLS, O=DEFAULT_OVERLAP, M=DEFAULT_MISMATCH):
    """rules 4 and 5: ``sites`` = [(K1, side, SUPPORT, ECLEN, codes)] ascending by (K1, side) -> (uint64[SIZE] with the four push
    counters 0, rows): rows = [(R index, L index, TSD, status, LEN, MISMATCH, CLOSURES, SEQ codes)] ascending by (t, P_R, P_L)"""
    c = numpy.zeros(SIZE, dtype=numpy.uint64)
    add = lambda k, n=1: c.__setitem__(SN_INDEX[k], c[SN_INDEX[k]] + numpy.uint64(n))
    lefts = {}
    for i, (k1, side, _, eclen, _) in enumerate(sites):
        if eclen > CLIP_COLS:
            add("sites_extended")
        if eclen >= K:
            add("right_sites" if side else "left_sites")
            if side == 0:
                lefts[k1] = i
    rows = []
    for i, (k1, side, _, eclen, x) in enumerate(sites):
        if side != 1 or eclen < K:
            continue
        tid, P = k1 >> 32, k1 & 0xffffffff
        for PL in range(max(P + 1 - CLIP_INS_MAX_TSD, 0), P + 2):
            j = lefts.get(tid << 32 | PL) if PL < 1 << 32 else None
            if j is None:
                continue
            status, l, mm, closures, seq = close_pair(x, sites[j][4], O, M)
            add("pairs")
            add("closed" if status == CLOSED else "open")
            if closures > 1:
                add("closed_multi")
            rows.append((i, j, P + 1 - PL, status, l, mm, closures, seq))
    return c, rows


def summarise(events, sn=None, min_support=3, K=DEFAULT_COLS, O=DEFAULT_OVERLAP, M=DEFAULT_MISMATCH):
    """THE DEFINITION, the whole job: ``events`` of every read in any order, ``sn`` the push counters -> (uint64[SIZE], sites, rows) of
    :func:`extended_sites` and :func:`pairs_of_sites`"""
    sites = extended_sites(events, min_support)
    c, rows = pairs_of_sites(sites, K, O, M)
    for k, v in (sn or {}).items():
        c[SN_INDEX[k]] = v
    return c, sites, rows


# ------------------------------------------------------------------------------------------- packing
def pack_words(codes, n_words):
    """codes -> ``n_words`` words of 56 bits: column 28 w + j in bits 2j + 1 : 2j of word w"""
    out = [0] * n_words
    for i, c in enumerate(codes):
        out[i // CLIP_COLS] |= c << (2 * (i % CLIP_COLS))
    return out


def unpack_words(words, n):
    return [(int(words[i // CLIP_COLS]) >> (2 * (i % CLIP_COLS))) & 3 for i in range(n)]


def site_columns(sites):
    """[(K1, side, SUPPORT, ECLEN, codes)] -> (k1 uint64[], side, eclen uint32[], cons5 uint64[n][5]) as the device entries take them"""
    n = len(sites)
    k1 = numpy.array([s[0] for s in sites], dtype=numpy.uint64).reshape(n)
    side = numpy.array([s[1] for s in sites], dtype=numpy.uint32).reshape(n)
    eclen = numpy.array([s[3] for s in sites], dtype=numpy.uint32).reshape(n)
    cons5 = numpy.array([pack_words(s[4], CLIP_EXT_WORDS) for s in sites], dtype=numpy.uint64).reshape(n, CLIP_EXT_WORDS)
    return k1, side, eclen, cons5


def pair_columns(rows):
    """rows of :func:`pairs_of_sites` -> (seven uint32 columns, seq10 uint64[n][10]) as the device entries give them"""
    n = len(rows)
    cols = tuple(numpy.array([r[k] for r in rows], dtype=numpy.uint32).reshape(n) for k in range(7))
    return cols, numpy.array([pack_words(r[7], SEQ_WORDS) for r in rows], dtype=numpy.uint64).reshape(n, SEQ_WORDS)


# ------------------------------------------------------------------------------------------- the device entries
def ins_sites(k1, side, eclen, cons5, K=DEFAULT_COLS, O=DEFAULT_OVERLAP, M=DEFAULT_MISMATCH, ctx=None, device=False):
    """``tdt_clip_ins_sites`` (``device``: ``tdt_clip_ins_sites_device`` on torch copies of the arrays): host columns of sites ascending
    by (K1, side) -> (uint64[SIZE], the seven columns of ``PAIR_DTYPES``, seq10 uint64[n][10])"""
    ctx = ctx or _native.default_context()
    lib, P = ctx.lib, _native.ptr
    k1, side = numpy.ascontiguousarray(k1, dtype=numpy.uint64), numpy.ascontiguousarray(side, dtype=numpy.uint32)
    eclen, cons5 = numpy.ascontiguousarray(eclen, dtype=numpy.uint32), numpy.ascontiguousarray(cons5, dtype=numpy.uint64)
    n = len(k1)
    assert len(side) == len(eclen) == n and cons5.size == n * CLIP_EXT_WORDS
    sn = numpy.zeros(SIZE, dtype=numpy.uint64)
    np_ = ctypes.c_size_t(0)
    if not device:
        args = (ctx.handle, n, P(k1), P(side), P(eclen), P(cons5), int(K), int(O), int(M))
        _native.check(lib.tdt_clip_ins_sites(*args, P(sn), *[None] * 8, ctypes.byref(np_)))
        cols = [numpy.zeros(np_.value, dtype=dt) for dt in PAIR_DTYPES]
        seq = numpy.zeros((np_.value, SEQ_WORDS), dtype=numpy.uint64)
        if np_.value:
            _native.check(lib.tdt_clip_ins_sites(*args, P(sn), *[P(c) for c in cols], P(seq), ctypes.byref(np_)))
        return sn, tuple(cols), seq
    import torch
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a).view(numpy.uint8).reshape(-1).copy()).cuda() if a.size else torch.zeros(8, dtype=torch.uint8).cuda()
    d_in = [dev(a) for a in (k1, side, eclen, cons5)]
    d_sn = torch.zeros(SIZE * 8, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    args = (ctx.handle, n, *[ctypes.c_void_p(t.data_ptr()) for t in d_in], int(K), int(O), int(M), ctypes.c_void_p(d_sn.data_ptr()))
    _native.check(lib.tdt_clip_ins_sites_device(*args, *[None] * 8, ctypes.byref(np_)))
    m = np_.value
    d_out = [torch.zeros(max(m, 1) * 4, dtype=torch.uint8).cuda() for _ in PAIR_DTYPES] + [torch.zeros(max(m, 1) * 8 * SEQ_WORDS, dtype=torch.uint8).cuda()]
    torch.cuda.synchronize()
    if m:
        _native.check(lib.tdt_clip_ins_sites_device(*args, *[ctypes.c_void_p(t.data_ptr()) for t in d_out], ctypes.byref(np_)))
        assert np_.value == m
    torch.cuda.synchronize()
    cols = tuple(t.cpu().numpy().view(numpy.uint32)[:m].copy() for t in d_out[:7])
    seq = d_out[7].cpu().numpy().view(numpy.uint64)[:m * SEQ_WORDS].reshape(m, SEQ_WORDS).copy()
    return d_sn.cpu().numpy().view(numpy.uint64).copy(), cols, seq


# ------------------------------------------------------------------------------------------- the file
def text_of(codes, reverse=False):
    s = "".join("ACGT"[c] for c in codes)
    return (s[::-1] if reverse else s) or "."


def file_rows(k1, support, eclen, cons5, pair_cols, seq10):
    """the columns of the clip rows (K1, SUPPORT), of ``ext_rows`` (ECLEN, cons5) and of the pairs -> the file's rows
    [(tid, P_R, P_L, TSD, R_SUPPORT, L_SUPPORT, R_COLS, L_COLS, status, LEN, MISMATCH, CLOSURES, SEQ, LEFT_SEQ, RIGHT_SEQ)], texts"""
    out = []
    ri, li, tsd, status, ln, mm, closures = (numpy.asarray(c).tolist() for c in pair_cols)
    cons5, seq10 = numpy.asarray(cons5).reshape(-1, CLIP_EXT_WORDS), numpy.asarray(seq10).reshape(-1, SEQ_WORDS)
    for p in range(len(ri)):
        r, l = ri[p], li[p]
        kr, kl = int(k1[r]), int(k1[l])
        x, y = unpack_words(cons5[r], int(eclen[r])), unpack_words(cons5[l], int(eclen[l]))
        closed = status[p] == CLOSED
        out.append((kr >> 32, kr & 0xffffffff, kl & 0xffffffff, tsd[p], int(support[r]), int(support[l]), int(eclen[r]), int(eclen[l]), status[p],
                    ln[p] if closed else None, mm[p] if closed else None, closures[p], text_of(unpack_words(seq10[p], ln[p])) if closed else ".",
                    text_of(x), text_of(y, reverse=True)))
    return out


def write_file(path, counts, rows, names, K, O, M):
    """``{o}.clips.ins.tab`` (see the module docstring); rows: those of :func:`file_rows`"""
    c = [int(v) for v in numpy.asarray(counts).tolist()]
    dot = lambda v: "." if v is None else str(v)
    out = ["# tiddit_amd clips_ins v1 cols=%d max_tsd=%d min_cols=%d min_overlap=%d max_mismatch=%d\n" % (CLIP_EXT_COLS, CLIP_INS_MAX_TSD, K, O, M)]
    out += ["SN\t%s\t%d\n" % (k, c[i]) for i, k in enumerate(SN)]
    out.append(COLUMNS)
    for tid, PR, PL, tsd, rs, ls, rc, lc, status, ln, mm, closures, seq, left, right in rows:
        chrom = names[tid] if tid < len(names) else str(tid)
        out.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\t%s\t%d\t%s\t%s\t%s\n" % (chrom, PR, PL, tsd, rs, ls, rc, lc, ("OPEN", "CLOSED")[status], dot(ln), dot(mm),
                                                                                   closures, seq, left, right))
    with open(path, "w") as f:
        f.write("".join(out))


def definition_file(path, events, sn, names, S, K, O, M):
    """the file from the definition alone (what the tests compare a job's file with) -> the counters"""
    counts, sites, rows = summarise(events, sn, S, K, O, M)
    k1, _, eclen, cons5 = site_columns(sites)
    cols, seq10 = pair_columns(rows)
    write_file(path, counts, file_rows(k1, [s[2] for s in sites], eclen, cons5, cols, seq10), names, K, O, M)
    return counts


def summary_line(counts):
    c = numpy.asarray(counts)
    return "clips ins: {} extension keys, {} sites extended, {} left and {} right sites, {} pairs, {} closed ({} with several closures), {} open".format(
        *(int(c[SN_INDEX[k]]) for k in ("ext_keys", "sites_extended", "left_sites", "right_sites", "pairs", "closed", "closed_multi", "open")))


def main(counter, clip_rows, prefix, names, K, O, M, rows_out=None):
    """the stage behind the clip counter's finish and in front of its close: the extension store's finish, the gather and the pair
    launches on the device over the rows where they lie, and the file -> the counters (:func:`summary_line`); ``clip_rows``: the
    columns ``counter.rows()`` gave; ``rows_out``: None, or a list that receives the rows of :func:`file_rows` (tiddit_clip_vcf.py joins them)"""
    STAGE_SECONDS.clear()
    t = time.time()
    sn = counter.ins(K, O, M)
    eclen, cons5 = counter.ext_rows()
    cols, seq10 = counter.ins_rows()
    ms = counter.ins_timing()
    STAGE_SECONDS["clip ins (device: extension finish, gather, pairs)"] = time.time() - t
    for k, v in zip(("extension finish (sort, run lengths, vote)", "gather of the extended consensus", "pair count + closure"), ms.tolist()):
        STAGE_SECONDS["  clip ins " + k + " (device time)"] = v * 1e-3
    t = time.time()
    rows = file_rows(clip_rows[0], clip_rows[2], eclen, cons5, cols, seq10)
    write_file(prefix + ".clips.ins.tab", sn, rows, names, K, O, M)
    if rows_out is not None:
        rows_out.extend(rows)
    STAGE_SECONDS["clip ins table text (host)"] = time.time() - t
    return sn
