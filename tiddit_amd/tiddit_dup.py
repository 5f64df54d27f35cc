"""Duplicate metrics and library size from the ``--sv`` scan (``TIDDIT_DUPS=1``): how many duplicates the library HAS — recomputed from
the reads' unclipped 5' ends, whatever the file's 0x400 marks say — and how complex it is, from the batches the scan already holds in HBM
(csrc/tdt_dup.hip: one launch per batch builds the keys, one sort and three run-length launches per job), written to ``{o}.dup.tab``.
What Picard ``MarkDuplicates`` / ``samtools markdup`` take one more pass over the file for.  Nothing in the reference does this; the
definition below is the specification, :func:`key_of_read` implements it read by read and :func:`summarise` over the whole job.

ONE library is assumed: read groups (``RG`` tags, ``@RG`` lines) are ignored, every read of the file belongs to the same library.

Per record, from the batch's columns ``flag tid pos end mate_tid mate_pos`` and the record's bytes (``raw`` at ``rec_off``):

  ``SN records`` += 1.  The record is ELIGIBLE when ``flag & 0xB04 == 0`` (mapped, primary, not QC-failed) and ``tid >= 0``: ``SN eligible``
        += 1.  The 0x400 bit is ignored on purpose: the stage recomputes duplicates.
  It belongs to a PAIR when it is paired (0x1), its mate is mapped (0x8 clear) and ``mate_tid >= 0``; otherwise it is a FRAGMENT.
  Of a pair exactly one mate CARRIES the pair's key, decided on the aligned coordinates alone (symmetric between the mates, no tag
        needed): the read is the carrier when ``(tid, pos) < (mate_tid, mate_pos)``, on equality when it has 0x40.  The other mate adds
        1 to ``SN pair_mates``, gets no key, and its bytes are never looked at.
  A fragment or a carrier is bounded as ``tdt_qc`` and ``tdt_alleles`` bound a record: ``rec_off + 36 <= raw_len``, its own ``l_seq >= 0``,
        ``32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size`` and ``rec_off + 4 + block_size <= raw_len``.  A
        record that fails, holds a CIGAR op code above 8, has a ``tid`` (a carrier: or a ``mate_tid``) of ``DUP_MAX_CONTIGS`` = 2^24 or
        more, or an ``E`` / ``ME`` (below) outside ``[0, 2^33)`` is MALFORMED: ``SN malformed`` += 1, no key, nothing else.  Nothing outside
        ``[raw, raw + raw_len)`` is ever read.  So ``eligible = malformed + fragments + pairs + pair_mates``.
  Own 5' end: ``lead`` = the summed lengths of ALL leading ``S`` / ``H`` operations, ``trail`` the same for the trailing ones (a CIGAR of
        clips only: all of it is ``lead``, ``trail = 0``; no operations: both 0).  Forward (0x10 clear): ``end5 = pos - lead``; reverse:
        ``end5 = end - 1 + trail``.  ``pos`` and ``end`` are the batch's columns (``end`` is htslib's ``bam_endpos``: a reference length of 0
        behaves as 1); the sums are int64.  ``E = end5 + DUP_BIAS``, ``DUP_BIAS`` = 2^28.  ``K1 = tid << 34 | E << 1 | rev``.
  A fragment: ``K2 = 0``, ``SN fragments`` += 1.
  A carrier: the aux fields are walked from the end of the qualities to the end of the block (tag, tag, type; types ``A c C`` take 1
        byte, ``s S`` 2, ``i I f`` 4, ``Z H`` run to their NUL, ``B`` is a subtype byte of ``c C s S i I f``, an int32 count and count x size
        bytes; any other type, a missing NUL or a field running past the block ends the walk).  The first ``MC`` of type ``Z`` wins; its
        text is ``(digits op)+`` with op in ``MIDNSHP=X`` and every number below 2^28 — ``*``, an empty text or anything else counts as no
        ``MC``.  ``mlead`` / ``mtrail`` are its clip sums as above, ``mref = max(sum of M D N = X, 1)``.  Mate forward (0x20 clear):
        ``mend5 = mate_pos - mlead``; mate reverse: ``mend5 = mate_pos + mref - 1 + mtrail``.  Without a usable ``MC``:
        ``mend5 = mate_pos`` and ``SN pairs_no_mc`` += 1.  ``ME = mend5 + DUP_BIAS``.
        ``K2 = 1 << 58 | mate_tid << 34 | ME << 1 | mrev``, ``SN pairs`` += 1.
  ``SN flagged`` counts the keyed reads that carry 0x400 (what the file's own marks say about the same reads).

Sets.  Keyed reads with equal ``(K1, K2)`` form a set; a set of size k holds k - 1 duplicates.  Bit 58 of K2 keeps fragments and pairs
apart: fragments are compared with fragments only.  THIS DIFFERS FROM PICARD, which also marks a fragment that shares its end with a
read of a pair.  :func:`summarise` gives ``fragment_sets``, ``pair_sets``, ``fragment_duplicates``, ``pair_duplicates`` and
``HIST[DUP_HIST_MAX][2]``: sets by ``min(k, DUP_HIST_MAX)`` (row k - 1), columns ``pair_sets`` and ``fragment_sets``; ``DUP_HIST_MAX`` = 1024.
Nothing depends on the order of the reads.

Two derived rows, integers computed on the host (:func:`derived`):
  ``duplication_ppm = floor(10^6 * (fragment_duplicates + 2 * pair_duplicates) / (fragments + 2 * pairs))``; absent when the denominator is 0.
  ``estimated_library_size = floor(L)``, L the solution of ``pair_sets = L * (1 - exp(-pairs / L))`` (the Lander-Waterman estimate Picard
        prints) by :func:`library_size`; absent when ``pair_duplicates == 0`` or ``pairs == 0``.

``{o}.dup.tab``: ``# tiddit_amd dup v1``, then tab-separated integer rows: ``SN name n`` (the twelve counters always, in the order of
``SN``, then the derived rows that exist) and ``HIST size pair_sets fragment_sets`` (size from 1) only where one of the two is non-zero.

The counters are ONE uint64 array of ``SIZE`` entries: ``SN`` at 0, ``HIST`` at 12 (the layout of include/tiddit_hip.h).

N ranks: refused (``__main__.run_sv``).  A set can straddle a shard seam and per-rank set counts do not add; an exchange of keys to owner
ranks is out of scope.
"""
import ctypes
import math
import struct
import time

import numpy

from . import _native, bamio
from .bamio import _raw_of

DUP_BIAS = 1 << 28
DUP_HIST_MAX = 1024
DUP_MAX_CONTIGS = 1 << 24
E_LIMIT = 1 << 33
PAIR_BIT = 1 << 58
SN = ("records", "eligible", "malformed", "fragments", "pairs", "pair_mates", "pairs_no_mc", "flagged", "fragment_sets", "pair_sets",
      "fragment_duplicates", "pair_duplicates")
SN_INDEX = {k: i for i, k in enumerate(SN)}
OFF_HIST = len(SN)
SIZE = OFF_HIST + 2 * DUP_HIST_MAX
HEADER = "# tiddit_amd dup v1\n"
STAGE_SECONDS = {}
# what key_of_read says about a record
NOT_ELIGIBLE, MATE, MALFORMED, FRAGMENT, PAIR = "not_eligible", "mate", "malformed", "fragment", "pair"
BISECTIONS = 64
_AUX_SIZE = {ord(k): v for k, v in (("A", 1), ("c", 1), ("C", 1), ("s", 2), ("S", 2), ("i", 4), ("I", 4), ("f", 4))}
_B_SIZE = {ord(k): v for k, v in (("c", 1), ("C", 1), ("s", 2), ("S", 2), ("i", 4), ("I", 4), ("f", 4))}
_MC_OPS = {ord(c): c for c in "MIDNSHP=X"}


def parse_switch(value):
    """``TIDDIT_DUPS`` -> False (unset or empty) or True (``1``); ValueError (its text is the error line) for anything else"""
    if value is None or value == "":
        return False
    if value == "1":
        return True
    raise ValueError("the switch is 1 or unset")


# ------------------------------------------------------------------------------------------- the definition
def clip_sums(ops):
    """[(op letter or code, len)] -> (lead, trail): the summed leading / trailing clips; clips only: (all of it, 0)"""
    lead = trail = 0
    seen = False
    for op, ln in ops:
        if op in (4, 5, "S", "H"):
            if seen:
                trail += ln
            else:
                lead += ln
        else:
            seen = True
            trail = 0
    return lead, trail


def mate_cigar(raw, p, e):
    """the walk over the aux fields raw[p:e]: -> the operations [(letter, len)] of the first ``MC:Z`` when its text is usable, else None"""
    while p + 3 <= e:
        tag, ty = bytes(raw[p:p + 2]), raw[p + 2]
        p += 3
        if ty in _AUX_SIZE:
            if p + _AUX_SIZE[ty] > e:
                return None
            p += _AUX_SIZE[ty]
        elif ty in (0x5a, 0x48):                                   # Z H
            q = p
            while q < e and raw[q] != 0:
                q += 1
            if q >= e:
                return None                                        # (no NUL inside the block)
            if tag == b"MC" and ty == 0x5a:
                return _mc_text(bytes(raw[p:q]))
            p = q + 1
        elif ty == 0x42:                                           # B
            if p + 5 > e or raw[p] not in _B_SIZE:
                return None
            count, = struct.unpack_from("<I", raw, p + 1)
            if p + 5 + count * _B_SIZE[raw[p]] > e:
                return None
            p += 5 + count * _B_SIZE[raw[p]]
        else:
            return None
    return None


def _mc_text(text):
    ops, num, digits = [], 0, 0
    for ch in text:
        if 0x30 <= ch <= 0x39:
            num = min(num * 10 + ch - 0x30, 1 << 28)               # (saturates: a long run of digits stays a small integer)
            digits += 1
        elif ch in _MC_OPS and digits and num < (1 << 28):
            ops.append((_MC_OPS[ch], num))
            num = digits = 0
        else:
            return None
    return ops if ops and not digits else None


def key_of_read(flag, tid, pos, end, mate_tid, mate_pos, rec_off, raw):
    """THE DEFINITION, one read -> (kind, K1, K2, marked, no_mc); K1 .. no_mc are None unless kind is FRAGMENT or PAIR.  ``raw``: the
    batch's record bytes (bytes-like), the other arguments the read's entries of the batch's columns."""
    none = (None, None, None, None)
    if flag & 0xB04 or tid < 0:
        return (NOT_ELIGIBLE,) + none
    pair = bool(flag & 0x1) and not flag & 0x8 and mate_tid >= 0
    if pair and not ((tid, pos) < (mate_tid, mate_pos) or ((tid, pos) == (mate_tid, mate_pos) and flag & 0x40)):
        return (MATE,) + none
    bad = (MALFORMED,) + none
    raw_len = len(raw)
    if tid >= DUP_MAX_CONTIGS or (pair and mate_tid >= DUP_MAX_CONTIGS) or rec_off + 36 > raw_len:
        return bad
    block_size, = struct.unpack_from("<I", raw, rec_off)
    r0 = rec_off + 4
    l_name = raw[r0 + 8]
    n_cig, = struct.unpack_from("<H", raw, r0 + 12)
    L, = struct.unpack_from("<i", raw, r0 + 16)
    if L < 0 or 32 + l_name + 4 * n_cig + (L + 1) // 2 + L > block_size or rec_off + 4 + block_size > raw_len:
        return bad
    cig = r0 + 32 + l_name
    words = [struct.unpack_from("<I", raw, cig + 4 * j)[0] for j in range(n_cig)]
    if any((w & 0xf) > 8 for w in words):
        return bad
    lead, trail = clip_sums([(w & 0xf, w >> 4) for w in words])
    rev = 1 if flag & 0x10 else 0
    E = (end - 1 + trail if rev else pos - lead) + DUP_BIAS
    if not 0 <= E < E_LIMIT:
        return bad
    k1 = tid << 34 | E << 1 | rev
    marked = 1 if flag & 0x400 else 0
    if not pair:
        return FRAGMENT, k1, 0, marked, 0
    mc = mate_cigar(raw, cig + 4 * n_cig + (L + 1) // 2 + L, r0 + block_size)
    mrev = 1 if flag & 0x20 else 0
    if mc is None:
        mend5 = mate_pos
    else:
        mlead, mtrail = clip_sums(mc)
        mref = max(sum(ln for op, ln in mc if op in "MDN=X"), 1)
        mend5 = mate_pos + mref - 1 + mtrail if mrev else mate_pos - mlead
    ME = mend5 + DUP_BIAS
    if not 0 <= ME < E_LIMIT:
        return bad
    return PAIR, k1, PAIR_BIT | mate_tid << 34 | ME << 1 | mrev, marked, 1 if mc is None else 0


def keys_of_batch_by_read(b, keys, sn):
    """the definition over one batch, read by read: appends (K1, K2, marked) to ``keys`` and adds to the push counters ``sn`` (a dict)"""
    raw = _raw_of(b)
    for i in range(len(b.tid)):
        kind, k1, k2, marked, no_mc = key_of_read(int(b.flag[i]), int(b.tid[i]), int(b.pos[i]), int(b.end[i]), int(b.mate_tid[i]),
                                                  int(b.mate_pos[i]), int(b.rec_off[i]), raw)
        _count(sn, kind, marked, no_mc)
        if k1 is not None:
            keys.append((k1, k2, marked))


def _count(sn, kind, marked, no_mc, n=1):
    sn["records"] = sn.get("records", 0) + n
    if kind == NOT_ELIGIBLE:
        return
    sn["eligible"] = sn.get("eligible", 0) + n
    name = {MATE: "pair_mates", MALFORMED: "malformed", FRAGMENT: "fragments", PAIR: "pairs"}[kind]
    sn[name] = sn.get(name, 0) + n
    if marked:
        sn["flagged"] = sn.get("flagged", 0) + n
    if no_mc:
        sn["pairs_no_mc"] = sn.get("pairs_no_mc", 0) + n


def summarise(keys, sn=None):
    """THE DEFINITION, the whole job: ``keys`` = every keyed read's (K1, K2, marked) in any order, ``sn`` the push counters ->
    uint64[SIZE]"""
    c = numpy.zeros(SIZE, dtype=numpy.uint64)
    for k, v in (sn or {}).items():
        c[SN_INDEX[k]] = v
    sizes = {}
    for k1, k2, _ in keys:
        sizes[(k1, k2)] = sizes.get((k1, k2), 0) + 1
    for (k1, k2), k in sizes.items():
        frag = 0 if k2 & PAIR_BIT else 1
        c[SN_INDEX["fragment_sets" if frag else "pair_sets"]] += 1
        c[SN_INDEX["fragment_duplicates" if frag else "pair_duplicates"]] += k - 1
        c[OFF_HIST + 2 * (min(k, DUP_HIST_MAX) - 1) + frag] += 1
    return c


def library_size(pairs, pair_sets):
    """floor(L), L solving ``pair_sets = L * (1 - exp(-pairs / L))``, or None when ``pairs <= pair_sets`` or either is < 1 (no duplicate
    seen: the library's size cannot be told).  In float64: ``f(L) = L * -expm1(-pairs / L)`` grows with L towards ``pairs``.  ``lo = hi =
    pair_sets`` (f(lo) < pair_sets); ``hi`` doubles, at most 64 times, until ``f(hi) >= pair_sets``; then exactly BISECTIONS = 64 times
    ``mid = (lo + hi) / 2`` replaces ``lo`` when ``f(mid) < pair_sets`` and ``hi`` otherwise; the answer is ``floor(hi)``."""
    if pair_sets < 1 or pairs <= pair_sets:
        return None
    n, c = float(pairs), float(pair_sets)
    f = lambda L: L * -math.expm1(-n / L)
    lo = hi = c
    for _ in range(64):
        if f(hi) >= c:
            break
        hi *= 2.0
    for _ in range(BISECTIONS):
        mid = (lo + hi) / 2.0
        if f(mid) < c:
            lo = mid
        else:
            hi = mid
    return int(math.floor(hi))


def derived(counts):
    """-> [(name, n)]: the derived rows that exist"""
    v = lambda k: int(counts[SN_INDEX[k]])
    out = []
    den = v("fragments") + 2 * v("pairs")
    if den:
        out.append(("duplication_ppm", 10 ** 6 * (v("fragment_duplicates") + 2 * v("pair_duplicates")) // den))
    if v("pair_duplicates") and v("pairs"):
        L = library_size(v("pairs"), v("pair_sets"))
        if L is not None:
            out.append(("estimated_library_size", L))
    return out


# ------------------------------------------------------------------------------------------- the same rules on whole columns
def _within(counts):
    owner = numpy.repeat(numpy.arange(len(counts)), counts)
    start = numpy.cumsum(counts) - counts
    return numpy.arange(int(counts.sum()), dtype=numpy.int64) - start[owner], owner


def keys_of_batch(b, sn):
    """The definition over one batch on whole columns (numpy) — for files too large for :func:`key_of_read`'s loop, to which
    tests/test_dup_refs_cpu.py pins it on every aimed case.  Only the ``MC`` walk of the carriers that HAVE aux bytes is per read.
    Adds to the push counters ``sn`` (a dict) -> (K1 uint64[], K2 uint64[], marked uint8[]) of the batch's keyed reads."""
    f, tid, pos, end, mtid, mpos = (numpy.asarray(getattr(b, k)).astype(numpy.int64) for k in ("flag", "tid", "pos", "end", "mate_tid", "mate_pos"))
    ro = numpy.asarray(b.rec_off).astype(numpy.int64)
    raw = numpy.frombuffer(b.raw, dtype=numpy.uint8) if isinstance(b.raw, (bytes, bytearray)) else numpy.ascontiguousarray(b.raw, dtype=numpy.uint8)
    raw_len = len(raw)
    add = lambda k, n: sn.__setitem__(k, sn.get(k, 0) + int(n))
    add("records", len(f))
    elig = ((f & 0xB04) == 0) & (tid >= 0)
    add("eligible", elig.sum())
    pair = elig & ((f & 0x1) != 0) & ((f & 0x8) == 0) & (mtid >= 0)
    first = (tid < mtid) | ((tid == mtid) & (pos < mpos)) | ((tid == mtid) & (pos == mpos) & ((f & 0x40) != 0))
    add("pair_mates", (pair & ~first).sum())
    need = numpy.flatnonzero(elig & (~pair | first))
    f, tid, pos, end, mtid, mpos, ro, pair = f[need], tid[need], pos[need], end[need], mtid[need], mpos[need], ro[need], pair[need]
    ok = (tid < DUP_MAX_CONTIGS) & (~pair | (mtid < DUP_MAX_CONTIGS)) & (ro + 36 <= raw_len)
    at = numpy.where(ok, ro, 0)
    if raw_len < 36:
        ok[:] = False
        raw = numpy.zeros(36, dtype=numpy.uint8)
    u = lambda o, n: sum(raw[at + o + k].astype(numpy.int64) << (8 * k) for k in range(n))
    bs, l_name, n_cig, L = u(0, 4), u(12, 1), u(16, 2), u(20, 4)
    L = numpy.where(L >= 1 << 31, L - (1 << 32), L)
    ok &= (L >= 0) & (32 + l_name + 4 * n_cig + (L + 1) // 2 + L <= bs) & (ro + 4 + bs <= raw_len)
    n_cig = numpy.where(ok, n_cig, 0)
    cig = at + 36 + l_name
    j, owner = _within(n_cig)
    w_at = cig[owner] + 4 * j
    words = sum(raw[w_at + k].astype(numpy.int64) << (8 * k) for k in range(4))
    code, ln = words & 0xf, words >> 4
    n = len(need)
    ok &= numpy.bincount(owner[code > 8], minlength=n) == 0
    clip = (code == 4) | (code == 5)
    first_nc = numpy.full(n, 1 << 20, dtype=numpy.int64)
    numpy.minimum.at(first_nc, owner[~clip], j[~clip])
    last_nc = numpy.full(n, -1, dtype=numpy.int64)
    numpy.maximum.at(last_nc, owner[~clip], j[~clip])
    lead = numpy.bincount(owner, weights=numpy.where(clip & (j < first_nc[owner]), ln, 0), minlength=n).astype(numpy.int64)
    trail = numpy.bincount(owner, weights=numpy.where(clip & (j > last_nc[owner]) & (last_nc[owner] >= 0), ln, 0), minlength=n).astype(numpy.int64)
    rev = (f & 0x10) != 0
    E = numpy.where(rev, end - 1 + trail, pos - lead) + DUP_BIAS
    ok &= (E >= 0) & (E < E_LIMIT)
    # ---- the mates' ends: the aux walk only where there are aux bytes
    mrev = (f & 0x20) != 0
    mend5 = mpos.copy()
    no_mc = pair.copy()
    aux = cig + 4 * n_cig + (L + 1) // 2 + L
    stop = at + 4 + bs
    mem = memoryview(raw)
    for k in numpy.flatnonzero(ok & pair & (stop > aux)).tolist():
        mc = mate_cigar(mem, int(aux[k]), int(stop[k]))
        if mc is not None:
            no_mc[k] = False
            mlead, mtrail = clip_sums(mc)
            mref = max(sum(x for op, x in mc if op in "MDN=X"), 1)
            mend5[k] = min(int(mpos[k]) + mref - 1 + mtrail, 1 << 62) if mrev[k] else int(mpos[k]) - mlead
    ME = mend5 + DUP_BIAS
    ok &= ~pair | ((ME >= 0) & (ME < E_LIMIT))
    add("malformed", (~ok).sum())
    add("fragments", (ok & ~pair).sum())
    add("pairs", (ok & pair).sum())
    add("pairs_no_mc", (ok & pair & no_mc).sum())
    add("flagged", (ok & ((f & 0x400) != 0)).sum())
    g = numpy.flatnonzero(ok)
    k1 = (tid[g].astype(numpy.uint64) << numpy.uint64(34)) | (E[g].astype(numpy.uint64) << numpy.uint64(1)) | rev[g].astype(numpy.uint64)
    k2 = (numpy.uint64(PAIR_BIT) | (mtid[g].astype(numpy.uint64) << numpy.uint64(34)) | (numpy.where(pair[g], ME[g], 0).astype(numpy.uint64) << numpy.uint64(1))
          | mrev[g].astype(numpy.uint64))
    k2 = numpy.where(pair[g], k2, numpy.uint64(0)).astype(numpy.uint64)
    return k1, k2, ((f[g] & 0x400) != 0).astype(numpy.uint8)


def summarise_columns(k1, k2, sn):
    """:func:`summarise` over key columns (numpy) -> uint64[SIZE]"""
    c = numpy.zeros(SIZE, dtype=numpy.uint64)
    for k, v in sn.items():
        c[SN_INDEX[k]] = v
    if len(k1):
        order = numpy.lexsort((k2, k1))
        a, b2 = k1[order], k2[order]
        head = numpy.concatenate([[True], (a[1:] != a[:-1]) | (b2[1:] != b2[:-1])])
        starts = numpy.flatnonzero(head)
        size = numpy.diff(numpy.concatenate([starts, [len(a)]]))
        frag = (b2[starts] & numpy.uint64(PAIR_BIT)) == 0
        for is_frag, sets, dups in ((True, "fragment_sets", "fragment_duplicates"), (False, "pair_sets", "pair_duplicates")):
            s = size[frag == is_frag]
            c[SN_INDEX[sets]] = len(s)
            c[SN_INDEX[dups]] = int((s - 1).sum())
            h = numpy.bincount(numpy.minimum(s, DUP_HIST_MAX) - 1, minlength=DUP_HIST_MAX).astype(numpy.uint64)
            c[OFF_HIST + int(is_frag):OFF_HIST + 2 * DUP_HIST_MAX:2] = h
    return c


# ------------------------------------------------------------------------------------------- the device handle
class DupCounter:
    """``tdt_dup_*``: the key store and the counters in HBM; one push per batch of the scan, one finish per job."""

    def __init__(self, n_contigs, max_contig_len, capacity=1 << 20, ctx=None):
        self.ctx = ctx or _native.default_context()
        assert self.ctx.lib.tdt_dup_size() == SIZE
        h = ctypes.c_void_p()
        _native.check(self.ctx.lib.tdt_dup_create(self.ctx.handle, int(n_contigs), int(max_contig_len), int(capacity), ctypes.byref(h)))
        self.handle = h

    def push_device_batch(self, b):
        """one DeviceBatch: enqueued on the reader's stream, nothing waited for (call before the batch's buffers are handed on)"""
        _native.check(self.ctx.lib.tdt_dup_push_device(self.handle, b.pointer_table(), len(b), b._raw_len))

    def push_host_batch(self, b):
        """one host-decoded batch (or any object with its columns): uploaded, then the same kernel"""
        cols, raw = bamio.host_columns(b, ("flag", "tid", "pos", "end", "mate_tid", "mate_pos", "rec_off"))      # (the arguments of tdt_dup_push, in order)
        _native.check(self.ctx.lib.tdt_dup_push(self.handle, *[_native.ptr(c) for c in cols], len(cols[0]), _native.ptr(raw), len(raw)))

    def keys(self):
        """-> (K1 uint64[], K2 uint64[], marked uint8[]): the store as it lies in HBM (its order is not the file's)"""
        n = ctypes.c_size_t(0)
        _native.check(self.ctx.lib.tdt_dup_keys(self.handle, None, None, None, ctypes.byref(n)))
        k1, k2, m = numpy.zeros(n.value, dtype=numpy.uint64), numpy.zeros(n.value, dtype=numpy.uint64), numpy.zeros(n.value, dtype=numpy.uint8)
        if n.value:
            _native.check(self.ctx.lib.tdt_dup_keys(self.handle, _native.ptr(k1), _native.ptr(k2), _native.ptr(m), ctypes.byref(n)))
        return k1, k2, m

    def finish(self):
        """-> uint64[SIZE]: the push counters and, from one sort of the store, the sets (the store is left as it was)"""
        out = numpy.zeros(SIZE, dtype=numpy.uint64)
        _native.check(self.ctx.lib.tdt_dup_finish(self.handle, _native.ptr(out)))
        return out

    def timing(self):
        """ms of the last finish: [sort by K2, gather, sort by K1, run lengths]"""
        out = numpy.zeros(4, dtype=numpy.float64)
        _native.check(self.ctx.lib.tdt_dup_timing(self.handle, _native.ptr(out)))
        return out

    def reset(self):
        _native.check(self.ctx.lib.tdt_dup_reset(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.tdt_dup_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------- the file
def write_file(path, counts):
    """``{o}.dup.tab`` (see the module docstring)"""
    c = [int(v) for v in numpy.asarray(counts).tolist()]
    out = [HEADER]
    out += ["SN\t%s\t%d\n" % (k, c[i]) for i, k in enumerate(SN)]
    out += ["SN\t%s\t%d\n" % kv for kv in derived(c)]
    for r in range(DUP_HIST_MAX):
        p, f = c[OFF_HIST + 2 * r], c[OFF_HIST + 2 * r + 1]
        if p or f:
            out.append("HIST\t%d\t%d\t%d\n" % (r + 1, p, f))
    with open(path, "w") as f:
        f.write("".join(out))


def summary_line(counts):
    c = numpy.asarray(counts)
    d = dict(derived([int(v) for v in c.tolist()]))
    return "duplicates: {} records, {} fragments, {} pairs, {} fragment duplicates, {} pair duplicates, {} ppm, library size {}, malformed records {}".format(
        *(int(c[SN_INDEX[k]]) for k in ("records", "fragments", "pairs", "fragment_duplicates", "pair_duplicates")),
        d.get("duplication_ppm", "-"), d.get("estimated_library_size", "-"), int(c[SN_INDEX["malformed"]]))


def main(counter, prefix):
    """the stage behind the scan: the sort and the run lengths on the device, the file and the summary line"""
    STAGE_SECONDS.clear()
    t = time.time()
    counts = counter.finish()
    ms = counter.timing()
    counter.close()
    STAGE_SECONDS["duplicate sets (device: two sorts, gather, run lengths)"] = time.time() - t
    for k, v in zip(("sort by K2", "gather of K1", "sort by K1", "run lengths + histogram"), ms.tolist()):
        STAGE_SECONDS["  " + k + " (device time)"] = v * 1e-3
    t = time.time()
    write_file(prefix + ".dup.tab", counts)
    STAGE_SECONDS["duplicate table text (host)"] = time.time() - t
    print(summary_line(counts))
    return counts
