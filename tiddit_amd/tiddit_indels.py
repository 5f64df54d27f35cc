"""Small-indel candidates from the ``--sv`` scan (``TIDDIT_INDELS=1`` / ``S`` / ``S:Q``): every distinct insertion or deletion that at
least ``S`` eligible reads carry in their CIGAR, with its support by strand and the local depth, from the batches the scan already holds
in HBM (csrc/tdt_indel.hip: one launch per batch builds the keys, one sort and the run-length launches per job), written to
``{o}.indels.tab``.  Nothing in the reference does this: its signals start at discordant pairs and split reads.  The definition below
is the specification, :func:`events_of_read` implements it read by read and :func:`summarise` over the whole job.

The switch: ``S`` is the minimum support, 1 ... 10^6, default 2; ``Q`` the minimum MAPQ, 0 ... 255, default 20.  A bare ``1`` means the
defaults; a support of 1 is written ``1:20``.

Per record, from the batch's columns ``flag tid pos mapq rec_off`` and the record's bytes (``raw`` at ``rec_off``):

  1. ``SN records`` += 1.  The record is ELIGIBLE when ``flag & 0xF04 == 0`` (mapped, primary, not QC-failed, not marked duplicate),
        ``tid >= 0`` and ``mapq >= Q``: ``SN eligible`` += 1.  Nothing else is done for the others, and their bytes are never read.
  2. The record is bounded as ``tdt_dup`` / ``tdt_qc`` / ``tdt_alleles`` bound one: ``rec_off + 36 <= raw_len``, its own ``l_seq >= 0``,
        ``32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size`` and ``rec_off + 4 + block_size <= raw_len``.  It is
        MALFORMED (``SN malformed`` += 1, no event, no other counter) when the bound fails, a CIGAR op code is above 8, ``tid >= 2^24``,
        ``pos < 0``, or ANY keyed event's ``P`` (below; also one beyond the cap of step 4) lies outside ``[1, 2^31)``.  Nothing outside
        ``[raw, raw + raw_len)`` is ever read.
  3. One walk over the CIGAR, ``r = pos``, ``q = 0`` (both int64): ``M = X`` (0, 7, 8) add their length to ``r`` and ``q``; ``D N`` (2, 3)
        to ``r``; ``I S`` (1, 4) to ``q``; ``H P`` (5, 6) to neither.  An ``I`` or ``D`` at index j is FLANKED when the operations j - 1 and
        j + 1 both exist and both have a code in {0, 7, 8}.  One that is not flanked, or has length 0, adds 1 to ``SN unanchored`` and is
        no event (leading or trailing indels, indels beside a clip, ``I`` beside ``D``).  A flanked one of length >= 65536 adds 1 to
        ``SN too_long`` and is no event.  Every other flanked one is a KEYED EVENT with ``P = r`` BEFORE the operation's own advance: the
        0-based position of the first deleted base, or of the base to the right of an insertion — either way the 1-based position of
        the anchor base, as a VCF writes it.  It carries its length, its type and, an insertion, the query offset ``q`` before its own
        advance.  (``unanchored`` and ``too_long`` count for every record that is not malformed, noisy ones included.)
  4. A read with more than ``INDEL_MAX_PER_READ`` = 4 keyed events is NOISY: ``SN noisy_reads`` += 1 and none of its events count (a
        150-bp read with five indels is a misalignment; the cap is also what bounds the store).  Otherwise ``SN reads_with_events`` += 1
        when it has any, and ``SN insertions`` / ``SN deletions`` += 1 per event.
  5. Keys, ``rev = flag >> 4 & 1``: ``K1 = tid << 32 | P``, ``K2 = type << 63 | len << 47 | kind << 45 | payload << 1 | rev``; ``type`` 0 is a
        deletion (kind 0, payload 0), 1 an insertion:
          its query span ``[q, q + len)`` is not inside ``[0, l_seq)`` (``SEQ *``): kind 2, payload 0;
          ``len <= 22`` and every 4-bit base code one of A C G T (1, 2, 4, 8): kind 0, ``payload = sum(code_i << 2 i)``, A C G T = 0 1 2 3;
          otherwise kind 1: ``h = 0xcbf29ce484222325``; for each base code b in order ``h = ((h ^ b) * 0x100000001b3) mod 2^64``; then
          ``payload = (h ^ (h >> 44)) & (2^44 - 1)``.
  6. Sets.  Keyed events with equal ``(K1, K2 >> 1)`` are one distinct event: ``SUPPORT`` their number, ``REV`` those with bit 0 set,
        ``FWD`` the rest.  ``SN distinct_events`` is the number of sets, ``SN reported_events`` those with ``SUPPORT >= S``.  Nothing
        depends on the order of the reads.

``{o}.indels.tab``: ``# tiddit_amd indels v1 min_support=S min_mapq=Q``, then ``SN name n`` for the eleven counters in the order of
``SN``, then ``#CHROM POS TYPE LEN SEQ SUPPORT FWD REV COV`` and one row per reported event, ascending by ``(K1, K2 >> 1)``, all
tab-separated.  ``POS = P``; ``TYPE`` is ``INS`` or ``DEL``; ``SEQ`` the bases (kind 0 insertion), ``#`` and 11 lower-case hex digits of
the payload (kind 1), ``*`` (kind 2), ``.`` (deletion); ``COV`` is ``"%.2f"`` of the job's own 50-bp coverage bin
``coverage_data[chrom][(P - 1) // 50]``, ``.`` when the job holds no bins for that contig (or none that far).

Events are NOT left-normalised against the reference, unless ``TIDDIT_INDELS_NORM=1``: two reads that place the same indel of a repeat
differently give two rows.

``TIDDIT_INDELS_NORM=1`` (valid only with ``TIDDIT_INDELS``): the reference is loaded into HBM before the scan (refseq.py) and, behind
step 4 and in front of step 5, every keyed event of an OK read is moved as far LEFT as the reference allows (:func:`left_normalise`).
With ``p = P``, ``n`` the length and ``CAP = INDEL_NORM_MAX_SHIFT = 1024``:
  * the contig is not loaded, ``p + n >`` its length (deletion) or ``p >`` its length (insertion): the event keeps its key,
        ``SN off_reference`` += 1.  An insertion of kind 2 is never shifted and counts nowhere.
  * ``k = 0``; while ``k < CAP`` and ``p - k >= 2``: ``a = ref[p - k - 1]``; a deletion's ``b = ref[p - k - 1 + n]``; an insertion's ``b`` is the
        last code of its allele after k shifts, ``S[n - 1 - k]`` for ``k < n`` (``S`` the read's inserted codes) and ``ref[p - k + n - 1]``
        behind that; ``a == b`` and ``a`` one of A C G T: ``k += 1``, otherwise stop.
  * ``P' = P - k >= 1``; the insertion's allele becomes ``S_k`` = the first ``n`` codes of ``ref[p - k .. p) ++ S`` and step 5's payload (packed
        or hashed) is computed from ``S_k``.  ``SN shifted_events`` += 1 when ``k > 0``; ``SN shift_capped`` += 1 when the loop stopped
        because ``k == CAP`` — the event is keyed at the capped position, so two placements more than ``CAP`` apart can still differ.
Everything else — eligibility, the bound, malformed / noisy, the cap of four, the eleven counters — is unchanged.  The file's first
line gains `` left_normalised=1024`` and three ``SN`` rows follow the eleven: ``shifted_events``, ``shift_capped``, ``off_reference``.
Long-read libraries are out of scope (the cap of 4).  N ranks: refused (``__main__.run_sv``) — merging per-rank rows needs an exchange
of keys.
"""
import struct
import time

import numpy

from . import _native
from .bamio import _raw_of
from .keyed_counter import KeyedCounter

INDEL_MAX_PER_READ = 4
INDEL_MAX_LEN = 1 << 16
INDEL_MAX_CONTIGS = 1 << 24
P_LIMIT = 1 << 31
PACK_MAX = 22
MAX_SUPPORT = 10 ** 6
DEFAULT_SUPPORT, DEFAULT_MAPQ = 2, 20
SN = ("records", "eligible", "malformed", "unanchored", "too_long", "noisy_reads", "reads_with_events", "insertions", "deletions",
      "distinct_events", "reported_events")
SN_INDEX = {k: i for i, k in enumerate(SN)}
INDEL_NORM_MAX_SHIFT = 1024          # CAP of left_normalise
NORM_SN = ("shifted_events", "shift_capped", "off_reference")          # the three counters of TIDDIT_INDELS_NORM, behind the eleven
NORM_OK, NORM_CAPPED, NORM_OFF = "ok", "capped", "off_reference"
SIZE = len(SN)
COLUMNS = "#CHROM\tPOS\tTYPE\tLEN\tSEQ\tSUPPORT\tFWD\tREV\tCOV\n"
STAGE_SECONDS = {}
STAGE_NOTES = {}            # counts of the last main() that are not seconds
# what events_of_read says about a record
NOT_ELIGIBLE, MALFORMED, NOISY, OK = "not_eligible", "malformed", "noisy", "ok"
_FNV, _PRIME, _M64, _M44 = 0xcbf29ce484222325, 0x100000001b3, (1 << 64) - 1, (1 << 44) - 1
_CODE = {1: 0, 2: 1, 4: 2, 8: 3}


def parse_switch(value):
    """``TIDDIT_INDELS`` -> None (unset or empty) or (S, Q); ValueError (its text is the error line) for anything else"""
    if value is None or value == "":
        return None
    if value == "1":
        return DEFAULT_SUPPORT, DEFAULT_MAPQ
    parts = value.split(":")
    if len(parts) > 2 or not all(p.isascii() and p.isdigit() and len(p) <= 9 for p in parts):
        raise ValueError("the switch is 1, S or S:Q (minimum support 1 ... 10^6, minimum MAPQ 0 ... 255)")
    s, q = int(parts[0]), int(parts[1]) if len(parts) == 2 else DEFAULT_MAPQ
    if not 1 <= s <= MAX_SUPPORT:
        raise ValueError("the minimum support is 1 ... 10^6")
    if not 0 <= q <= 255:
        raise ValueError("the minimum MAPQ is 0 ... 255")
    return s, q


def parse_norm_switch(value, indels):
    """``TIDDIT_INDELS_NORM`` -> False (unset or empty) or True; ``indels``: what :func:`parse_switch` made of ``TIDDIT_INDELS``.
    ValueError (its text is the error line) for any other value, and for the switch without its partner"""
    if value is None or value == "":
        return False
    if value != "1":
        raise ValueError("the switch is 1")
    if indels is None:
        raise ValueError("the switch left-normalises the events of TIDDIT_INDELS: TIDDIT_INDELS not set")
    return True


# ------------------------------------------------------------------------------------------- the definition
def insertion_payload(raw, seq, q, length, l_seq):
    """(kind, payload) of an insertion of ``length`` bases at query offset ``q``; ``seq``: where the record's 4-bit sequence starts in raw"""
    if q + length > l_seq:
        return 2, 0
    codes = [(raw[seq + (k >> 1)] >> (0 if k & 1 else 4)) & 0xf for k in range(q, q + length)]
    if length <= PACK_MAX and all(b in _CODE for b in codes):
        return 0, sum(_CODE[b] << (2 * i) for i, b in enumerate(codes))
    h = _FNV
    for b in codes:
        h = ((h ^ b) * _PRIME) & _M64
    return 1, (h ^ (h >> 44)) & _M44


def payload_of_codes(codes):
    """(kind, payload) of an insertion whose bases are the 4-bit ``codes`` (step 5's kinds 0 and 1)"""
    if len(codes) <= PACK_MAX and all(b in _CODE for b in codes):
        return 0, sum(_CODE[b] << (2 * i) for i, b in enumerate(codes))
    h = _FNV
    for b in codes:
        h = ((h ^ b) * _PRIME) & _M64
    return 1, (h ^ (h >> 44)) & _M44


def left_normalise(ref, tid, P, length, is_ins, ins_codes):
    """THE DEFINITION of ``TIDDIT_INDELS_NORM``, one keyed event -> (P', ins_codes', k, status).  ``ref``: an object with ``length(tid)``
    (negative: the contig is not loaded) and ``code(tid, i)`` (the 4-bit code of base i); ``P``, ``length``: the event's; ``ins_codes``:
    an insertion's bases as 4-bit codes, None for a deletion and for an insertion of kind 2 (which is never shifted).  ``k`` is the
    shift distance, ``P' = P - k``, ``ins_codes'`` the rotated allele; ``status`` is NORM_OFF (the event keeps its key), NORM_CAPPED
    (the loop stopped because ``k == INDEL_NORM_MAX_SHIFT``) or NORM_OK."""
    p, n = P, length
    if is_ins and ins_codes is None:
        return P, None, 0, NORM_OK
    L = ref.length(tid)
    if L < 0 or (p > L if is_ins else p + n > L):
        return P, ins_codes, 0, NORM_OFF
    k = 0
    while k < INDEL_NORM_MAX_SHIFT and p - k >= 2:
        a = ref.code(tid, p - k - 1)
        if is_ins:
            b = ins_codes[n - 1 - k] if k < n else ref.code(tid, p - k + n - 1)
        else:
            b = ref.code(tid, p - k - 1 + n)
        if a == b and a in _CODE:
            k += 1
        else:
            break
    if is_ins and k:
        ins_codes = ([ref.code(tid, i) for i in range(p - k, p)] + list(ins_codes))[:n]
    return P - k, ins_codes, k, NORM_CAPPED if k == INDEL_NORM_MAX_SHIFT else NORM_OK


def events_of_read(flag, tid, pos, mapq, rec_off, raw, min_mapq=DEFAULT_MAPQ, ref=None):
    """THE DEFINITION, one read -> (kind, keys, unanchored, too_long): ``keys`` the read's [(K1, K2)] when kind is OK, else [];
    the two counts are what the read adds to ``SN unanchored`` / ``SN too_long`` (0 for a malformed record).  ``raw``: the batch's record
    bytes (bytes-like), the other arguments the read's entries of the batch's columns.  With ``ref`` (see :func:`left_normalise`) every
    event of an OK read is left-normalised before its keys are made, and a fifth value follows: what the read adds to
    (``shifted_events``, ``shift_capped``, ``off_reference``)."""
    r = _events_of_read(flag, tid, pos, mapq, rec_off, raw, min_mapq, ref)
    return r if ref is not None else r[:4]


def _events_of_read(flag, tid, pos, mapq, rec_off, raw, min_mapq, ref):
    if flag & 0xF04 or tid < 0 or mapq < min_mapq:
        return NOT_ELIGIBLE, [], 0, 0, (0, 0, 0)
    bad = (MALFORMED, [], 0, 0, (0, 0, 0))
    raw_len = len(raw)
    if tid >= INDEL_MAX_CONTIGS or pos < 0 or rec_off + 36 > raw_len:
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
    r, q = pos, 0
    events, un, tl = [], 0, 0
    for j, w in enumerate(words):
        op, ln = w & 0xf, w >> 4
        if op in (1, 2):
            flanked = 0 < j < n_cig - 1 and (words[j - 1] & 0xf) in (0, 7, 8) and (words[j + 1] & 0xf) in (0, 7, 8)
            if not flanked or ln == 0:
                un += 1
            elif ln >= INDEL_MAX_LEN:
                tl += 1
            else:
                if not 1 <= r < P_LIMIT:
                    return bad
                events.append((r, ln, op == 1, q))
        if op in (0, 2, 3, 7, 8):
            r += ln
        if op in (0, 1, 4, 7, 8):
            q += ln
    if len(events) > INDEL_MAX_PER_READ:
        return NOISY, [], un, tl, (0, 0, 0)
    rev = (flag >> 4) & 1
    keys = []
    norm = [0, 0, 0]
    seq = cig + 4 * n_cig
    for P, ln, ins, q in events:
        if ref is None:
            kind, payload = insertion_payload(raw, seq, q, ln, L) if ins else (0, 0)
        else:
            codes = [(raw[seq + (k >> 1)] >> (0 if k & 1 else 4)) & 0xf for k in range(q, q + ln)] if ins and q + ln <= L else None
            P, codes, k, status = left_normalise(ref, tid, P, ln, ins, codes)
            norm[0] += k > 0
            norm[1] += status == NORM_CAPPED
            norm[2] += status == NORM_OFF
            kind, payload = (0, 0) if not ins else (2, 0) if codes is None else payload_of_codes(codes)
        keys.append((tid << 32 | P, int(ins) << 63 | ln << 47 | kind << 45 | payload << 1 | rev))
    return OK, keys, un, tl, tuple(norm)


def _count(sn, kind, keys, un, tl, norm=None):
    add = lambda k, n: sn.__setitem__(k, sn.get(k, 0) + n) if n else None
    add("records", 1)
    if kind == NOT_ELIGIBLE:
        return
    add("eligible", 1)
    add("malformed", int(kind == MALFORMED))
    add("noisy_reads", int(kind == NOISY))
    add("unanchored", un)
    add("too_long", tl)
    add("reads_with_events", int(bool(keys)))
    add("insertions", sum(1 for _, k2 in keys if k2 >> 63))
    add("deletions", sum(1 for _, k2 in keys if not k2 >> 63))
    for name, v in zip(NORM_SN, norm or ()):
        add(name, v)


def keys_of_batch_by_read(b, keys, sn, min_mapq=DEFAULT_MAPQ, ref=None):
    """the definition over one batch, read by read: appends (K1, K2) to ``keys`` and adds to the push counters ``sn`` (a dict; with
    ``ref`` also to the three of ``NORM_SN``)"""
    raw = _raw_of(b)
    for i in range(len(b.tid)):
        kind, ks, un, tl, *norm = events_of_read(int(b.flag[i]), int(b.tid[i]), int(b.pos[i]), int(b.mapq[i]), int(b.rec_off[i]), raw, min_mapq, ref)
        _count(sn, kind, ks, un, tl, *norm)
        keys.extend(ks)


def summarise(keys, sn=None, min_support=DEFAULT_SUPPORT):
    """THE DEFINITION, the whole job: ``keys`` = every keyed event's (K1, K2) in any order, ``sn`` the push counters ->
    (uint64[SIZE], rows): rows = [(K1, K2 with bit 0 clear, SUPPORT, REV)] of the sets with SUPPORT >= min_support, ascending"""
    c = numpy.zeros(SIZE, dtype=numpy.uint64)
    for k, v in (sn or {}).items():
        if k not in NORM_SN:                                    # (those three are not among the eleven: norm_counts)
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


# ------------------------------------------------------------------------------------------- the same rules on whole columns
def keys_of_batch(b, sn, min_mapq=DEFAULT_MAPQ, ref=None):
    """The definition over one batch for files too large for :func:`events_of_read`'s loop, to which tests/test_indel_refs_cpu.py pins it
    on every aimed case: the filters, the record bound and a search for ``I`` / ``D`` / bad op codes run on whole columns (numpy); only
    the reads that HAVE such an operation go through :func:`events_of_read` (with ``ref``: left-normalised, and ``sn`` also gets the three
    counters of ``NORM_SN``).  Adds to the push counters ``sn`` -> [(K1, K2)]."""
    f, tid, pos, mq = (numpy.asarray(getattr(b, k)).astype(numpy.int64) for k in ("flag", "tid", "pos", "mapq"))
    ro = numpy.asarray(b.rec_off).astype(numpy.int64)
    raw = numpy.frombuffer(b.raw, dtype=numpy.uint8) if isinstance(b.raw, (bytes, bytearray)) else numpy.ascontiguousarray(b.raw, dtype=numpy.uint8)
    raw_len = len(raw)
    add = lambda k, n: sn.__setitem__(k, sn.get(k, 0) + int(n)) if int(n) else None
    add("records", len(f))
    need = numpy.flatnonzero(((f & 0xF04) == 0) & (tid >= 0) & (mq >= min_mapq))
    add("eligible", len(need))
    tid_, pos_, ro_ = tid[need], pos[need], ro[need]
    ok = (tid_ < INDEL_MAX_CONTIGS) & (pos_ >= 0) & (ro_ + 36 <= raw_len)
    at = numpy.where(ok, ro_, 0)
    table = raw if raw_len >= 36 else numpy.zeros(36, dtype=numpy.uint8)
    u = lambda o, n: sum(table[at + o + k].astype(numpy.int64) << (8 * k) for k in range(n))
    bs, l_name, n_cig, L = u(0, 4), u(12, 1), u(16, 2), u(20, 4)
    L = numpy.where(L >= 1 << 31, L - (1 << 32), L)
    ok &= (L >= 0) & (32 + l_name + 4 * n_cig + (L + 1) // 2 + L <= bs) & (ro_ + 4 + bs <= raw_len)
    n_cig = numpy.where(ok, n_cig, 0)
    owner = numpy.repeat(numpy.arange(len(need)), n_cig)
    j = numpy.arange(int(n_cig.sum()), dtype=numpy.int64) - (numpy.cumsum(n_cig) - n_cig)[owner]
    code = table[(at + 36 + l_name)[owner] + 4 * j] & 0xf if len(owner) else numpy.zeros(0, dtype=numpy.uint8)
    look = numpy.bincount(owner[(code == 1) | (code == 2) | (code > 8)], minlength=len(need)) > 0
    add("malformed", (~ok).sum())
    keys = []
    mem = _raw_of(b)
    for k in need[ok & look].tolist():
        kind, ks, un, tl, *norm = events_of_read(int(f[k]), int(tid[k]), int(pos[k]), int(mq[k]), int(ro[k]), mem, min_mapq, ref)
        c = {}
        _count(c, kind, ks, un, tl, *norm)
        for name in SN[2:9] + NORM_SN:
            add(name, c.get(name, 0))
        keys.extend(ks)
    return keys


# ------------------------------------------------------------------------------------------- the device handle
class IndelCounter(KeyedCounter):
    """``tdt_indel_*``: the key store and the counters in HBM; one push per batch of the scan, one finish per job."""
    PREFIX, SIZE, DEFAULT_SUPPORT = "tdt_indel", SIZE, DEFAULT_SUPPORT

    def __init__(self, n_contigs, min_mapq=DEFAULT_MAPQ, capacity=1 << 20, ctx=None):
        self._create(ctx, int(n_contigs), int(min_mapq), int(capacity))
        self.min_mapq = int(min_mapq)

    def set_reference(self, ref):
        """attach a resident reference (refseq.RefSeq; kept alive by this object) — the pushes from here on left-normalise every event
        against it (``TIDDIT_INDELS_NORM``) — or detach it with None"""
        _native.check(self.ctx.lib.tdt_indel_set_reference(self.handle, ref.handle if ref is not None else None))
        self.reference = ref

    def norm_stats(self):
        """-> uint64[3]: ``NORM_SN`` — events shifted, shifts that stopped at the cap, events off the reference — since the last reset"""
        return self._out("norm_stats", 3, numpy.uint64)


# ------------------------------------------------------------------------------------------- the file
def seq_text(k2):
    """the SEQ field of a row's K2"""
    if not k2 >> 63:
        return "."
    ln, kind, payload = (k2 >> 47) & 0xffff, (k2 >> 45) & 3, (k2 >> 1) & _M44
    if kind == 0:
        return "".join("ACGT"[(payload >> (2 * i)) & 3] for i in range(ln))
    return "#%011x" % payload if kind == 1 else "*"


def write_file(path, counts, rows, names, coverage_data, min_support, min_mapq, norm=None):
    """``{o}.indels.tab`` (see the module docstring); rows: (K1[], K2[], SUPPORT[], REV[]) or a list of such tuples; ``norm``: the three
    counters of ``NORM_SN`` when the events were left-normalised, else None"""
    if isinstance(rows, tuple):
        rows = list(zip(*(numpy.asarray(r).tolist() for r in rows)))
    c = [int(v) for v in numpy.asarray(counts).tolist()]
    out = ["# tiddit_amd indels v1 min_support=%d min_mapq=%d%s\n" % (min_support, min_mapq, " left_normalised=%d" % INDEL_NORM_MAX_SHIFT if norm is not None else "")]
    out += ["SN\t%s\t%d\n" % (k, c[i]) for i, k in enumerate(SN)]
    if norm is not None:
        out += ["SN\t%s\t%d\n" % (k, int(v)) for k, v in zip(NORM_SN, norm)]
    out.append(COLUMNS)
    for k1, k2, sup, rev in rows:
        tid, P = k1 >> 32, k1 & 0xffffffff
        chrom = names[tid] if tid < len(names) else str(tid)
        bins = coverage_data.get(chrom) if coverage_data is not None else None
        cov = "%.2f" % float(bins[(P - 1) // 50]) if bins is not None and (P - 1) // 50 < len(bins) else "."
        out.append("%s\t%d\t%s\t%d\t%s\t%d\t%d\t%d\t%s\n" % (chrom, P, "INS" if k2 >> 63 else "DEL", (k2 >> 47) & 0xffff, seq_text(k2), sup, sup - rev,
                                                           rev, cov))
    with open(path, "w") as f:
        f.write("".join(out))


def summary_line(counts):
    c = numpy.asarray(counts)
    return "indels: {} records, {} eligible, {} insertions, {} deletions, {} distinct events, {} reported, noisy reads {}, malformed records {}".format(
        *(int(c[SN_INDEX[k]]) for k in ("records", "eligible", "insertions", "deletions", "distinct_events", "reported_events", "noisy_reads", "malformed")))


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
    norm = counter.norm_stats() if counter.reference is not None else None
    ms = counter.timing()
    asks, grows, cap = counter.reserve_stats()
    min_mapq = counter.min_mapq
    counter.close()
    STAGE_SECONDS["indel sets (device: two sorts, gather, run lengths, rows)"] = time.time() - t
    for k, v in zip(("sort by K2", "gather of K1", "sort by K1", "run lengths + rows"), ms.tolist()):
        STAGE_SECONDS["  " + k + " (device time)"] = v * 1e-3
    STAGE_NOTES.update({"indel store: reserves that asked the device": asks, "indel store: growths": grows, "indel store: capacity (keys)": cap})
    t = time.time()
    write_file(prefix + ".indels.tab", counts, rows, names, coverage_data, S, min_mapq, norm)
    STAGE_SECONDS["indel table text (host)"] = time.time() - t
    print(summary_line(counts))
    if norm is not None:
        print("indels, left-normalised: {} events shifted, {} stopped at the cap of {} bases, {} off the reference".format(
            int(norm[0]), int(norm[1]), INDEL_NORM_MAX_SHIFT, int(norm[2])))
    return counts
