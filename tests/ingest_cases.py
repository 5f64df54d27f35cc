"""Record streams AIMED at the structure of the BAM ingest kernels (csrc/tdt_ingest.hip: bam_find_first, bam_find_records, the four
bam_decode_fields flavours, bam_tid_edges), and an independent reference for what they must give.  Pure Python / numpy.

The reference (`reference`) is a plain `struct` walk of an inflated BAM record stream written from the SAM/BAM specification; it calls
nothing native and not `bamio.BamReader`.  Per record it gives the thirteen columns of `tdt_ingest_arrays` (rec_off / sa_off absolute in
the stream: `batches` rebases them) and the generic 8-byte coverage record of csrc/tdt_cov_record.h.  Its rules:
  end     = pos + (sum of the M D N = X lengths), pos + 1 when that sum is 0 or flag 0x4 is set (htslib's bam_endpos);
  sa_off  = the value offset of the first well-formed SA tag of type Z, found by walking the aux fields by their types; -1 when there
            is none or the walk meets a malformed field first; type `d` is skipped as 8 bytes;
  packed  = span:24 (0xffffff: escape) | min(mapq, 63):6 | unmapped:1 | duplicate:1 in the high word, pos in the low word.
`guess_and_confirm` restates the contract of the record finder from the header comment of tdt_ingest.hip: per 16 KiB segment of a batch
the first offset that passes the record sanity check and whose block_size chain runs cleanly to the end of the segment, and a batch
whose segment guesses disagree with the chain from the known first record goes to the host chase.  It tells which batches a case
expects in `host_chases`; the cases of families F and G also STATE those batches, and tests/test_ingest_refs_cpu.py holds the two
against each other.

The streams are built byte by byte (header bytes + `bamio.encode_record` output, hand-packed aux bytes where that cannot express the
case) and cut into BGZF blocks of chosen inflated sizes with `bamio._bgzf_block`; every case fixes which bytes go into which push.
ING_SEG, ING_MAXREC and ING_EDGES are read from the `#define` lines of tdt_ingest.hip, so the cases move with them.

Families (cases of each: asserted in tests/test_ingest_refs_cpu.py):
  A  34  boundary placement: a record starting 36, 35, 33, 5, 4, 3, 2, 1 bytes in front of, on and 1 behind a segment boundary, ending
         1 in front of, on and 1 behind one, a record of exactly ING_SEG bytes (aligned and not), records covering 2 and 3 whole
         segments — in the first batch (placed by padding the header text) and again in a second batch behind a carried partial record
  B  10  dense segments: the shortest records of the format (38 bytes: up to 432 starts per segment, seven rounds of the lane loop),
         segments of exactly 63, 64, 65, 128 and 129 record starts, 255- and 257-byte records, two of them again behind a carry
  C  16  batch tails: pushes that leave 0, 1, 2, 3, 4, 20, 35, 36 bytes and a cut name of the next record, an incomplete first record,
         a push that is the rest of a carried record, a push inside a carried record, pushes of 4999 bytes, an empty file, only a header
  D   8  field edges: every CIGAR operation alone and in pairs, reference length 0, flag 0x4 with a CIGAR, n_cigar 0 and 65535, l_seq
         0 / 1 / odd, l_read_name 2 and 255, extreme field values, spans around the packed record's escape
  E   7  aux / SA: SA:Z first, in the middle, last, behind every other type and B subtype (count 0 too), empty, look-alikes inside Z, H
         and B:C values, SA of another type, stray bytes, malformed fields before and behind a real SA:Z
  F   7  decoys: bytes that form a plausible record inside a B:C array (and qualities) behind a segment boundary, in front of the true
         chain's entry point — complete (chased), behind a carry, in the last segment in front of the partial record, weak, chain-broken
  G   4  records the device check refuses but the chain and the host decoder accept: tid >= n_ref (in a guessed segment and in the
         batch's first), CIGAR query length != l_seq and a name byte outside 33..126 on the first record behind a segment boundary
  H   4  sharded seams (tdt_ingest_push_bounded twice): clean cut, own_bytes on a record start, one byte behind one, a decoy at the seam
  I   4  contig runs: 1, ING_EDGES (reported) and ING_EDGES + 1 (overflow) runs, a tid change on the first and last record of a batch
"""
import os
import re
import struct

import numpy as np

from tiddit_amd import bamio

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiddit_amd", "csrc", "tdt_ingest.hip")


def parse_constants(text=None):
    """ING_SEG, ING_EDGES and ING_MAXREC evaluated from the `#define` lines (the first definition: the one under #ifndef); KeyError
    when one can no longer be read.  `text`: the source, for the test of this parser."""
    text = open(_SRC).read() if text is None else text
    defs = {}
    for name, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+([A-Za-z_]\w*)[ \t]+([^\n]*?)[ \t]*(?://[^\n]*)?$", text, re.M):
        defs.setdefault(name, body)

    def value(name, depth=0):
        if name not in defs or depth > 8:
            raise KeyError("cannot parse #define %s" % name)
        expr = re.sub(r"\b(0[xX][0-9a-fA-F]+|[0-9]+)[uUlL]*\b", lambda h: str(int(h.group(1), 0)), defs[name])
        expr = re.sub(r"[A-Za-z_]\w*", lambda h: str(value(h.group(0), depth + 1)), expr)
        if not re.fullmatch(r"[0-9()+\-*/ \t]+", expr):
            raise KeyError("#define %s is not an integer expression: %r" % (name, defs[name]))
        return int(eval(expr.replace("/", "//")))

    return {k: value(k) for k in ("ING_SEG", "ING_EDGES", "ING_MAXREC")}


K = parse_constants()
SEG, EDGES, MAXREC = K["ING_SEG"], K["ING_EDGES"], K["ING_MAXREC"]
NONE = 0xffffffff
SIZE_MAX = (1 << 64) - 1
COLUMNS = ("tid", "pos", "end", "mapq", "flag", "mate_tid", "mate_pos", "tlen", "l_seq", "cigar_first", "cigar_last", "rec_off", "sa_off")
TYPES = (np.int32, np.int32, np.int32, np.uint8, np.uint16, np.int32, np.int32, np.int32, np.int32, np.uint32, np.uint32, np.uint64, np.int64)
REFS = [("c0", 250_000_000), ("c1", 50_000), ("c2", 1000), ("c3", 20_000_000)]
FAMILIES = ("A", "B", "C", "D", "E", "F", "G", "H", "I")
FAMILY_COUNTS = {"A": 34, "B": 10, "C": 16, "D": 8, "E": 7, "F": 7, "G": 4, "H": 4, "I": 4}
# a departure of the reference -> the family in which it must change the expected output of at least one case
MUTANTS = {"end_ignores_N": "D", "end_no_fallback": "D", "unmapped_keeps_span": "D", "span_saturates_early": "D",
           "sa_byte_scan": "E", "sa_any_type": "E", "first_plausible_offset": "F"}
START_D = (-36, -35, -33, -5, -4, -3, -2, -1, 0, 1)
END_D = (-1, 0, 1)
TAILS = (0, 1, 2, 3, 4, 20, 35, 36)


# ------------------------------------------------------------------------------------------------------------------- the reference
_AUX_FIXED = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4, b"d": 8}
_B_ELEM = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


def aux_fields(raw, a, end):
    """(tag, type, value offset, value size) of the well-formed aux fields in [a, end), in order, up to the first malformed one"""
    while a + 3 <= end:
        tag, typ, v = raw[a:a + 2], raw[a + 2:a + 3], a + 3
        if typ in _AUX_FIXED:
            size = _AUX_FIXED[typ]
        elif typ in (b"Z", b"H"):
            nul = raw.find(b"\x00", v, end)
            if nul < 0:
                return
            size = nul - v + 1
        elif typ == b"B":
            if v + 5 > end or raw[v:v + 1] not in _B_ELEM:
                return
            size = 5 + _B_ELEM[raw[v:v + 1]] * struct.unpack_from("<I", raw, v + 1)[0]
        else:
            return
        if v + size > end:
            return
        yield tag, typ, v, size
        a = v + size


def sa_offset(raw, a, end, mutant=None):
    if mutant == "sa_byte_scan":
        i = raw.find(b"SAZ", a, end)
        return i + 3 if i >= 0 else -1
    for tag, typ, v, _ in aux_fields(raw, a, end):
        if tag == b"SA" and (typ == b"Z" or mutant == "sa_any_type"):
            return v
    return -1


def reference_end(pos, flag, cigar, mutant=None):
    ops = (0, 2, 7, 8) if mutant == "end_ignores_N" else (0, 2, 3, 7, 8)
    rlen = sum(l for op, l in cigar if op in ops)
    if flag & 0x4 and mutant != "unmapped_keeps_span":
        rlen = 1
    if rlen == 0 and mutant != "end_no_fallback":
        rlen = 1
    return pos + rlen


def pack_record(pos, end, mapq, flag, mutant=None):
    """the generic coverage record, from the layout comment of csrc/tdt_cov_record.h"""
    span = end - pos
    escape = 0xffffff
    sp = escape if (span < 0 or span >= (escape - 1 if mutant == "span_saturates_early" else escape)) else span
    info = sp | (min(mapq, 63) << 24) | ((1 << 30) if flag & 0x4 else 0) | ((1 << 31) if flag & 0x400 else 0)
    return (info << 32) | (pos & 0xffffffff)


def reference(stream, skip, mutant=None):
    """every record of the inflated stream from byte `skip` on -> dict of the thirteen columns, `packed` and `rec_end` (numpy arrays)"""
    raw = bytes(stream)
    rows, o = [], skip
    while o < len(raw):
        assert o + 36 <= len(raw), "the stream ends inside a record"
        bs, tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<IiiBBHHHiiii", raw, o)
        nxt = o + 4 + bs
        assert nxt <= len(raw), "the stream ends inside a record"
        c0 = o + 36 + l_name
        words = struct.unpack_from("<%dI" % n_cig, raw, c0)
        cigar = [(w & 0xf, w >> 4) for w in words]
        end = reference_end(pos, flag, cigar, mutant)
        assert -(1 << 31) <= end < (1 << 31)
        aux = c0 + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        assert aux <= nxt
        rows.append((tid, pos, end, mapq, flag, mtid, mpos, tlen, l_seq, words[0] if n_cig else NONE, words[-1] if n_cig else NONE, o,
                     sa_offset(raw, aux, nxt, mutant), pack_record(pos, end, mapq, flag, mutant), nxt))
        o = nxt
    cols = list(zip(*rows)) if rows else [[] for _ in range(15)]
    out = {k: np.array(cols[i], dtype=t) for i, (k, t) in enumerate(zip(COLUMNS, TYPES))}
    out["packed"] = np.array(cols[13], dtype=np.uint64)
    out["rec_end"] = np.array(cols[14], dtype=np.uint64)
    return out


def runs_of(tid):
    """(edges, tids of the runs) of one batch's tid column, as tdt_ingest_edges / tdt_ingest_edge_tids report them; None when there
    are more than ING_EDGES runs (the device reports (size_t)-1)"""
    tid = np.asarray(tid)
    if not len(tid):
        return np.zeros(0, np.uint32), np.zeros(0, np.int32)
    e = np.concatenate([[0], np.flatnonzero(np.diff(tid)) + 1])
    if len(e) > EDGES:
        return None
    return e.astype(np.uint32), tid[e].astype(np.int32)


# ------------------------------------------------------------------------------------------ the finder's contract, restated
def plausible(buf, p, T, n_ref, deep):
    """the record sanity check at offset p of a batch of T bytes -> (0 complete and plausible | 1 runs past the batch | 2 not a record,
    block_size).  deep: also the name's characters (33..126) and the CIGAR / l_seq identity"""
    if p + 4 > T:
        return 1, 0
    bs = struct.unpack_from("<I", buf, p)[0]
    if bs < 32 or bs > 1 << 28:
        return 2, 0
    if p + 36 > T:
        return 1, 0
    tid, pos, l_name, _mapq, _bin, n_cig, _flag, l_seq, mtid, mpos, _tlen = struct.unpack_from("<iiBBHHHiiii", buf, p + 4)
    if not (-1 <= tid < n_ref and -1 <= mtid < n_ref) or pos < -1 or mpos < -1 or l_seq < 0 or l_name == 0:
        return 2, 0
    if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        return 2, 0
    if p + 36 + l_name <= T:
        if buf[p + 36 + l_name - 1] != 0:
            return 2, 0
        if deep and any(not 33 <= ch <= 126 for ch in buf[p + 36:p + 36 + l_name - 1]):
            return 2, 0
    if p + 4 + bs > T:
        return 1, 0
    if deep and n_cig and l_seq:
        qlen = 0
        for w in struct.unpack_from("<%dI" % n_cig, buf, p + 36 + l_name):
            if w & 0xf > 8:
                return 2, 0
            if w & 0xf in (0, 1, 4, 7, 8):
                qlen += w >> 4
        if qlen != l_seq:
            return 2, 0
    return 0, bs


def _candidates(buf, T, n_ref):
    """offsets that can pass the fixed-field part of the check (a superset of the deep check's passes), ascending"""
    a = np.frombuffer(buf, dtype=np.uint8, count=T).astype(np.uint32)
    ok = np.ones(T, dtype=bool)
    if T >= 4:
        u = a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24)
        ok[:T - 3] = (u >= 32) & (u <= 1 << 28)
        n = T - 35
        if n > 0:
            s = u.view(np.int32)
            f = lambda o: s[o:o + n]
            ok[:n] &= (f(4) >= -1) & (f(4) < n_ref) & (f(24) >= -1) & (f(24) < n_ref) & (f(8) >= -1) & (f(28) >= -1) & (f(20) >= 0) & (a[12:12 + n] != 0)
    return np.flatnonzero(ok)


class _Finder:
    def __init__(self, buf, T, s0, limit, n_ref, mutant=None):
        self.buf, self.T, self.s0, self.limit, self.n_ref, self.mutant = bytes(buf), T, s0, limit, n_ref, mutant
        self.cand = _candidates(self.buf, T, n_ref)
        self.seg = {}

    def segment(self, g):
        """(first, exit, count) of segment g: the per-segment guess of bam_find_records, from the file's header comment"""
        if g in self.seg:
            return self.seg[g]
        buf, T, s0, limit = self.buf, self.T, self.s0, self.limit
        lo = g * SEG
        hi = min(lo + SEG, T)
        p = hi if (s0 >= hi or lo >= limit) else max(lo, s0)
        forced = lo <= s0 < hi
        stop = min(hi, limit)
        f, e, c, weak = NONE, 0, 0, False
        while p < stop:
            if forced:
                rc, bs = plausible(buf, p, T, self.n_ref, True)
            else:
                rc = 2
                i = np.searchsorted(self.cand, p)
                while i < len(self.cand) and self.cand[i] < stop:
                    rc, bs = plausible(buf, int(self.cand[i]), T, self.n_ref, True)
                    if rc != 2:
                        break
                    i += 1
                if rc == 2:
                    break
                p = int(self.cand[i])
            q, n = p, 0
            while rc == 0 and q < stop:
                q += 4 + bs
                n += 1
                if q >= T:
                    break
                rc, bs = plausible(buf, q, T, self.n_ref, q >= stop)
                if self.mutant == "first_plausible_offset" and rc == 2:
                    rc = 1                                   # the mutant does not care where the chain of its first candidate leads
            if rc != 2 or forced:
                if n == 0 and not forced:
                    if not weak:
                        weak, f, e = True, p, p
                    p += 1
                else:
                    f, e, c = p, q, n
                    if forced and rc == 2:
                        f = NONE - 1
                    break
            else:
                p += 1
        self.seg[g] = (f, e, c)
        return self.seg[g]


def guess_and_confirm(buf, s0, n_ref, limit=None, mutant=None):
    """One batch: buf = its bytes, s0 = offset of its first record (None: unknown, a sharded start), limit = records starting at or
    behind it are the next shard's.  -> dict(confirmed, start, n, cur): the host's walk over the segment guesses; confirmed False =
    the batch goes to the host chase (an unknown start cannot: there the call fails)"""
    T = len(buf)
    limit = T if limit is None else limit
    F = _Finder(buf, T, -1 if s0 is None else s0, limit, n_ref, mutant)
    nseg = (T + SEG - 1) // SEG
    cur = s0
    if s0 is None:
        cur = T
        for s in range(nseg):
            if s * SEG >= limit:
                break
            if F.segment(s)[0] < NONE - 1:
                cur = F.segment(s)[0]
                break
    start, n, confirmed = cur, 0, True
    while cur < limit:
        s = cur // SEG
        f, e, c = F.segment(s)
        if f != cur:
            confirmed = False
            break
        n += c
        if e == cur:
            break
        cur = e
        if cur < (s + 1) * SEG and cur < limit:
            break
    return {"confirmed": confirmed, "start": start, "n": n, "cur": cur}


# ------------------------------------------------------------------------------------------------------------------- building streams
def header(refs=REFS, total=None):
    """BAM header bytes; total: pad the text with a @CO line so that the first record starts at exactly that offset"""
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    tail = struct.pack("<i", len(refs)) + b"".join(struct.pack("<i", len(n) + 1) + n.encode() + b"\x00" + struct.pack("<i", l) for n, l in refs)
    if total is not None:
        extra = total - (8 + len(text) + len(tail))
        assert extra >= 5, "header cannot be that short"
        text += "@CO\t" + "x" * (extra - 5) + "\n"
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + tail
    assert total is None or len(out) == total
    return out


_FLAGS = (99, 147, 83, 163, 0, 16, 1024 + 99, 2048 + 16, 256, 1024 + 147)


def rec(i, size=None, bare=None, **kw):
    """record number i of a stream, every field a function of i so that no two neighbours agree; size: exactly that many bytes
    (name and an XP:Z tag are stretched); bare: no CIGAR, no sequence, no tags"""
    bare = (size is not None and size < 200) if bare is None else bare
    l = 20 + i % 30
    d = dict(qname="r%d" % i, flag=_FLAGS[i % 10], tid=0, pos=1000 + 17 * i, mapq=(7 * i + 3) % 256, cigar="" if bare else "%dM" % l,
             mate_tid=i % len(REFS), mate_pos=5000 + 31 * i, tlen=400 - 3 * i, seq="" if bare else ("ACGTN" * 10)[:l],
             tags=[] if bare else [("NM", "i", i)] + ([("SA", "Z", "c1,%d,+,10S40M,60,0;" % (i + 1))] if i % 5 == 0 else []))
    d.update(kw)
    d["tags"] = list(d["tags"])
    r = bamio.encode_record(**d)
    if size is not None:
        extra = size - len(r)
        assert extra >= 0, (size, len(r))
        if 0 < extra < 4:
            d["qname"] += "n" * extra
        elif extra:
            d["tags"].append(("XP", "Z", "p" * (extra - 4)))
        r = bamio.encode_record(**d)
        assert len(r) == size
    return r


def with_aux(r, aux):
    """append raw aux bytes to an encoded record"""
    body = r[4:] + aux
    return struct.pack("<i", len(body)) + body


class Stream:
    def __init__(self, refs=REFS, header_len=None):
        self.refs = refs
        self.buf = bytearray(header(refs, header_len))
        self.skip = len(self.buf)
        self.starts = []

    @property
    def i(self):
        return len(self.starts)

    def __len__(self):
        return len(self.buf)

    def add(self, r):
        self.starts.append(len(self.buf))
        self.buf += r
        return self.starts[-1]

    def fill_to(self, target, **kw):
        """ordinary records until the next one starts at exactly `target`"""
        while target - len(self.buf) > 700:
            self.add(rec(self.i, size=200 + (self.i * 13) % 150, **kw))
        gap = target - len(self.buf)
        assert gap == 0 or gap >= 60, gap
        if gap:
            self.add(rec(self.i, size=gap, **kw))
        assert len(self.buf) == target
        return self


class Case:
    """One stream and how it is fed.  stream / skip: the inflated bytes and the offset of the first record; pushes: inflated bytes of
    every push (their sum is the stream); block: inflated bytes per BGZF block inside a push; aims: the placements the case claims
    (checked in test_ingest_refs_cpu.py); chased: the batches the case states to be host-chased; decoys: planted look-alikes;
    shard: for family H, (inflated block sizes, index of shard 1's first block)"""

    def __init__(self, name, family, aim, S, pushes=None, block=0xff00, aims=(), chased=(), decoys=(), shard=None, host=True, loose_aux=False,
                 sa_by_oracle=True):
        self.name, self.family, self.aim = name, family, aim
        self.stream, self.skip, self.refs = bytes(S.buf), S.skip, S.refs
        self.n_ref = len(S.refs)
        self.pushes = list(pushes) if pushes is not None else [len(self.stream)]
        assert sum(self.pushes) == len(self.stream) and (self.pushes[0] >= self.skip)
        self.block, self.aims, self.chased, self.decoys, self.shard = block, list(aims), list(chased), list(decoys), shard
        self.host, self.loose_aux, self.sa_by_oracle = host, loose_aux, sa_by_oracle
        self.routes = ("sharded",) if family == "H" else ("wave", "serial") if family in "ABCDE" else ("wave",)
        self._cache = {}

    def _blocks(self, data):
        return b"".join(bamio._bgzf_block(data[o:o + self.block], 1) for o in range(0, len(data), self.block))

    def comp_pushes(self):
        """the compressed bytes of every push; the last one ends with the BGZF end-of-file block"""
        if "comp" not in self._cache:
            out, o = [], 0
            for n in self.pushes:
                out.append(self._blocks(self.stream[o:o + n]))
                o += n
            out[-1] += bamio._BGZF_EOF
            self._cache["comp"] = out
        return self._cache["comp"]

    def shard_blocks(self):
        sizes, j = self.shard
        assert sum(sizes) == len(self.stream)
        out, o = [], 0
        for n in sizes:
            out.append(bamio._bgzf_block(self.stream[o:o + n], 1))
            o += n
        return out, j, sum(sizes[:j])

    def file_bytes(self):
        if self.shard:
            return b"".join(self.shard_blocks()[0]) + bamio._BGZF_EOF
        return b"".join(self.comp_pushes())

    def reference(self, mutant=None):
        key = ("ref", mutant if mutant in ("end_ignores_N", "end_no_fallback", "unmapped_keeps_span", "span_saturates_early", "sa_byte_scan",
                                             "sa_any_type") else None)
        if key not in self._cache:
            self._cache[key] = reference(self.stream, self.skip, key[1])
        return self._cache[key]

    def batches(self, mutant=None, model=True):
        """what every push must give: n, the columns (rec_off / sa_off rebased to the batch), packed, raw (the batch's bytes: carried
        partial record + the push), edges / edge_tids (None: overflow), carry (bytes left behind the last complete record), s0, and
        — model — chased: whether the finder's contract sends the batch to the host chase"""
        key = ("batches", mutant, model)
        if key in self._cache:
            return self._cache[key]
        R = self.reference(mutant)
        out, cursor, end_abs, lo = [], self.skip, 0, 0
        for b, plen in enumerate(self.pushes):
            base = 0 if b == 0 else cursor
            end_abs += plen
            hi = lo
            while hi < len(R["rec_off"]) and int(R["rec_end"][hi]) <= end_abs:
                hi += 1
            s0 = cursor - base
            if hi > lo:
                cursor = int(R["rec_end"][hi - 1])
            B = {"n": hi - lo, "base": base, "s0": s0, "raw": self.stream[base:end_abs], "carry": end_abs - cursor, "lo": lo, "hi": hi,
                 "packed": R["packed"][lo:hi]}
            if end_abs - base == s0:                                   # nothing behind the header / nothing at all: no batch is formed
                B["carry"] = 0
            for k in COLUMNS:
                B[k] = R[k][lo:hi].copy()
            B["rec_off"] -= np.uint64(base)
            B["sa_off"][B["sa_off"] >= 0] -= base
            r = runs_of(B["tid"])
            B["edges"], B["edge_tids"] = r if r is not None else (None, None)
            B["searched"] = end_abs - base != s0
            if model:
                B["chased"] = B["searched"] and not guess_and_confirm(B["raw"], s0, self.n_ref, mutant=mutant)["confirmed"]
            out.append(B)
            lo = hi
        self._cache[key] = out
        return out


# ------------------------------------------------------------------------------------------------------------------- the families
def _family_a():
    out = []

    def first_batch(name, aim, recs, j, at, kind, extra_aims=()):
        """records `recs` behind a header padded so that record j starts (kind "start") or ends ("end") at offset `at`"""
        rel = sum(len(r) for r in recs[:j + (kind == "end")])
        S = Stream(header_len=at - rel)
        for r in recs:
            S.add(r)
        out.append(Case(name, "A", aim, S, aims=[{"kind": kind, "batch": 0, "rec": j, "at": at}] + list(extra_aims)))

    def body(n0, special, n1):
        return [rec(i) for i in range(n0)] + [special] + [rec(n0 + 1 + i) for i in range(n1)]

    def second_batch(name, aim, build):
        """the same placement in a second batch: the first push ends 17 bytes into a record, so the second batch's grid starts there"""
        S = Stream()
        S.fill_to(S.skip + 3000)
        c0 = len(S)
        S.add(rec(S.i, size=260))
        aims = build(S, c0)
        S.fill_to(max(len(S) + 2000, c0 + 2 * SEG + 777))
        for a in aims:
            a["batch"] = 1
            if "at" in a:
                a["at"] -= c0
        out.append(Case(name, "A", aim + " (second batch, grid shifted by the carry)", S, pushes=[c0 + 17, len(S) - c0 - 17],
                        aims=aims + [{"kind": "tail", "batch": 0, "left": 17}]))

    for d in START_D:
        tag = ("m%d" % -d) if d < 0 else "p%d" % d
        first_batch("A_start_%s" % tag, "a record starts at SEG%+d" % d, body(20, rec(20, size=300), 120), 20, SEG + d, "start")

        def build(S, c0, d=d):
            S.fill_to(c0 + SEG + d)
            j = S.i
            S.add(rec(j, size=300))
            return [{"kind": "start", "rec": j, "at": c0 + SEG + d}]
        second_batch("A2_start_%s" % tag, "a record starts at SEG%+d" % d, build)
    for d in END_D:
        tag = ("m%d" % -d) if d < 0 else "p%d" % d
        first_batch("A_end_%s" % tag, "a record ends at SEG%+d" % d, body(20, rec(20, size=300), 120), 20, SEG + d, "end")

        def build(S, c0, d=d):
            S.fill_to(c0 + SEG + d - 300)
            j = S.i
            S.add(rec(j, size=300))
            return [{"kind": "end", "rec": j, "at": c0 + SEG + d}]
        second_batch("A2_end_%s" % tag, "a record ends at SEG%+d" % d, build)
    # records of a whole segment and more, between short ones
    first_batch("A_size_seg_aligned", "a record of exactly ING_SEG bytes on the grid", body(20, rec(20, size=SEG), 60), 20, SEG, "start",
                [{"kind": "size", "rec": 20, "size": SEG}, {"kind": "start", "batch": 0, "rec": 21, "at": 2 * SEG}])
    first_batch("A_size_seg_off", "a record of exactly ING_SEG bytes off the grid", body(20, rec(20, size=SEG), 60), 20, SEG - 1000, "start",
                [{"kind": "size", "rec": 20, "size": SEG}])
    first_batch("A_covers_2", "a record covering two whole segments", body(20, rec(20, size=2 * SEG + 20), 60), 20, SEG - 10, "start",
                [{"kind": "covers", "batch": 0, "rec": 20, "segments": [1, 2]}])
    first_batch("A_covers_3", "a record covering three whole segments", body(20, rec(20, size=3 * SEG + 20), 60), 20, SEG - 10, "start",
                [{"kind": "covers", "batch": 0, "rec": 20, "segments": [1, 2, 3]}])

    def big(size, off, segments):
        def build(S, c0):
            S.fill_to(c0 + SEG + off)
            j = S.i
            S.add(rec(j, size=size))
            a = [{"kind": "start", "rec": j, "at": c0 + SEG + off}, {"kind": "size", "rec": j, "size": size}]
            if segments:
                a.append({"kind": "covers", "rec": j, "segments": segments})
            return a
        return build
    second_batch("A2_size_seg_aligned", "a record of exactly ING_SEG bytes on the grid", big(SEG, 0, []))
    second_batch("A2_size_seg_off", "a record of exactly ING_SEG bytes off the grid", big(SEG, -1000, []))
    second_batch("A2_covers_2", "a record covering two whole segments", big(2 * SEG + 20, -10, [1, 2]))
    second_batch("A2_covers_3", "a record covering three whole segments", big(3 * SEG + 20, -10, [1, 2, 3]))
    return out


def _tiny(i, size=38, **kw):
    """the shortest record of the format (38 bytes: a one-character name, no CIGAR, no sequence) or a bare one of `size` bytes"""
    return rec(i, size=size, bare=True, qname=chr(33 + i % 94), **kw)


def _family_b():
    out = []

    def aligned(name, aim, sizes, nseg=2, carry=False):
        """segments 1 .. nseg of the (first or second) batch hold records of exactly `sizes` (summing to ING_SEG)"""
        assert sum(sizes) == SEG
        if carry:
            S = Stream()
            S.fill_to(S.skip + 3000)
            c0 = len(S)
            S.add(rec(S.i, size=260))
            S.fill_to(c0 + SEG)
        else:
            S, c0 = Stream(header_len=SEG), 0
        for _ in range(nseg):
            for z in sizes:
                S.add(_tiny(S.i, z))
        for _ in range(5):
            S.add(_tiny(S.i, 90))
        b = 1 if carry else 0
        out.append(Case(name, "B", aim, S, pushes=[c0 + 17, len(S) - c0 - 17] if carry else None,
                        aims=[{"kind": "per_segment", "batch": b, "segment": 1 + g, "starts": len(sizes)} for g in range(nseg)]))

    aligned("B_63", "63 record starts per segment", [256] * 62 + [512])
    aligned("B_64", "64 starts per segment: 256-byte records on the grid", [256] * 64)
    aligned("B_65", "65 starts per segment", [256] * 63 + [128] * 2)
    aligned("B_128", "128 starts per segment", [128] * 128)
    aligned("B_129", "129 starts per segment", [128] * 127 + [64] * 2)
    aligned("B2_64", "64 starts per segment behind a carry", [256] * 64, carry=True)
    for z, want in ((255, [65, 64]), (257, [64, 64])):
        S = Stream(header_len=SEG)
        for _ in range(150):
            S.add(_tiny(S.i, z))
        out.append(Case("B_%d" % z, "B", "%d-byte records drifting over the grid" % z, S,
                        aims=[{"kind": "per_segment", "batch": 0, "segment": 1 + g, "starts": w} for g, w in enumerate(want)]))
    most = -(-SEG // 38)
    for carry in (False, True):
        if carry:
            S = Stream()
            S.fill_to(S.skip + 3000)
            c0 = len(S)
            S.add(rec(S.i, size=260))
            S.fill_to(c0 + SEG)
        else:
            S, c0 = Stream(header_len=SEG), 0
        for _ in range(int(2.6 * most)):
            S.add(_tiny(S.i))
        out.append(Case("B2_min38" if carry else "B_min38", "B", "the shortest records: as many starts per segment as the format allows", S,
                        pushes=[c0 + 17, len(S) - c0 - 17] if carry else None,
                        aims=[{"kind": "per_segment", "batch": int(carry), "segment": 1, "starts": most}]))
    return out


def _family_c():
    out = []

    def base():
        S = Stream()
        S.fill_to(S.skip + SEG + 5000)
        x = len(S)
        S.add(rec(S.i, qname="n" * 40))
        S.fill_to(x + SEG + 3000)
        return S, x
    for t in TAILS + (36 + 10,):
        S, x = base()
        name = "C_tail_name" if t > 36 else "C_tail_%d" % t
        out.append(Case(name, "C", "the first push ends %d bytes into a record%s" % (t, " (inside its name)" if t > 36 else ""), S,
                        pushes=[x + t, len(S) - x - t], aims=[{"kind": "tail", "batch": 0, "left": t}]))
    S = Stream()
    S.fill_to(S.skip + SEG + 100)
    out.append(Case("C_first_incomplete", "C", "the first push ends 20 bytes into the first record: a batch of zero records", S,
                    pushes=[S.skip + 20, len(S) - S.skip - 20], aims=[{"kind": "tail", "batch": 0, "left": 20}, {"kind": "zero", "batch": 0}]))
    S = Stream()
    S.fill_to(S.skip + 4000)
    x = len(S)
    S.add(rec(S.i, size=3000))
    S.fill_to(x + 3000 + 5000)
    out.append(Case("C_remainder_only", "C", "a push that is exactly the rest of the carried record", S, pushes=[x + 50, 2950, len(S) - x - 3000],
                    aims=[{"kind": "tail", "batch": 0, "left": 50}, {"kind": "tail", "batch": 1, "left": 0}, {"kind": "count", "batch": 1, "n": 1}]))
    S = Stream()
    S.fill_to(S.skip + 4000)
    x = len(S)
    S.add(rec(S.i, size=40000))
    S.fill_to(x + 40000 + 5000)
    out.append(Case("C_inside_record", "C", "a push that lies inside the carried record: zero records, a longer carry", S,
                    pushes=[x + 50, 10000, len(S) - x - 10050],
                    aims=[{"kind": "tail", "batch": 0, "left": 50}, {"kind": "tail", "batch": 1, "left": 10050}, {"kind": "zero", "batch": 1}]))
    S = Stream()
    S.fill_to(S.skip + 3 * SEG)
    n = len(S)
    pushes = [4999] * (n // 4999) + ([n % 4999] if n % 4999 else [])
    out.append(Case("C_stride_4999", "C", "pushes of 4999 bytes: a tail and a shifted grid on every one", S, pushes=pushes, block=2048))
    S = Stream()
    out.append(Case("C_header_only", "C", "a file holding only a header", S, aims=[{"kind": "zero", "batch": 0}]))
    S = Stream()
    S.buf, S.skip = bytearray(), 0
    out.append(Case("C_empty_file", "C", "an empty file: the BGZF end-of-file block alone", S, aims=[{"kind": "zero", "batch": 0}], host=False))
    S, x = base()
    out.append(Case("C_three_tails", "C", "three pushes, each ending inside the fixed fields", S,
                    pushes=[S.starts[5] + 9, x + 33 - S.starts[5] - 9, len(S) - x - 33],
                    aims=[{"kind": "tail", "batch": 0, "left": 9}, {"kind": "tail", "batch": 1, "left": 33}]))
    return out


def _ops_record(i, ops, seq=None, **kw):
    qlen = sum(l for op, l in ops if op in (0, 1, 4, 7, 8))
    return rec(i, cigar=ops, seq=("ACGT" * (qlen // 4 + 1))[:qlen] if seq is None else seq, **kw)


def _family_d():
    out = []
    S = Stream()
    for a in range(9):
        S.add(_ops_record(S.i, [(a, 3 + a)], flag=0))
    for a in range(9):
        for b in range(9):
            S.add(_ops_record(S.i, [(a, 2 + a), (b, 11 + b)], flag=16))
    out.append(Case("D_cigar_ops", "D", "every CIGAR operation alone and every ordered pair", S))
    S = Stream()
    for ops in ([(1, 5)], [(4, 5)], [(5, 5)], [(6, 5)], [(4, 3), (1, 4), (5, 2), (6, 1)]):
        S.add(_ops_record(S.i, ops, flag=0))
        S.add(rec(S.i))
    out.append(Case("D_reference_length_0", "D", "only I / S / H / P operations on a mapped read: end = pos + 1", S))
    S = Stream()
    for ops, flag in (([(0, 30)], 4), ([(0, 10), (3, 500), (0, 10)], 4 | 1 | 64), ([(0, 30)], 0x404), ([(2, 9)], 4)):
        S.add(_ops_record(S.i, ops, flag=flag))
        S.add(rec(S.i))
    out.append(Case("D_unmapped_with_cigar", "D", "flag 0x4 together with a CIGAR: end = pos + 1", S))
    S = Stream()
    S.add(rec(0))
    S.add(rec(1, cigar="", seq="ACGTACGTAC", flag=0))
    S.add(rec(2))
    for l in (0, 1, 7):
        S.add(rec(S.i, cigar="", seq="ACGTACG"[:l], flag=0))
        S.add(rec(S.i, cigar=[(0, l)] if l else [(2, 4)], seq="ACGTACG"[:l], flag=0))
    S.add(rec(S.i, qname="q"))
    S.add(rec(S.i, qname="".join(chr(33 + k % 94) for k in range(254))))
    S.add(rec(S.i))
    out.append(Case("D_lengths", "D", "n_cigar 0 on a mapped read; l_seq 0, 1 and odd; l_read_name 2 and 255", S))
    S = Stream()
    S.add(rec(0))
    S.add(_ops_record(1, [(0, 1)] * 65535, seq=""))
    S.add(rec(2))
    S.add(rec(3))
    out.append(Case("D_ncigar_65535", "D", "n_cigar 65535", S))
    S = Stream()
    S.add(rec(0))
    S.add(rec(S.i, pos=-1, tid=0))
    S.add(rec(S.i, tid=-1, pos=500))
    S.add(rec(S.i, tid=-1, pos=-1, mate_tid=-1, mate_pos=-1, flag=77, cigar="", mapq=0))
    S.add(rec(S.i, mapq=255))
    S.add(rec(S.i, mapq=63))
    S.add(rec(S.i, mapq=64))
    S.add(rec(S.i, flag=0xffff))
    S.add(rec(S.i, flag=0xffff & ~0x4))
    S.add(rec(S.i, tlen=-(1 << 31)))
    S.add(rec(S.i, tlen=(1 << 31) - 1))
    S.add(rec(S.i, mate_pos=-1))
    S.add(rec(S.i, pos=(1 << 29) - 100, mate_pos=(1 << 31) - 1))
    S.add(rec(S.i, tid=len(REFS) - 1, mate_tid=len(REFS) - 1))
    S.add(rec(S.i))
    out.append(Case("D_extremes", "D", "pos -1, tid -1 with a position, mapq 255, flag 0xffff, tlen INT32_MIN / MAX, mate_pos -1", S))
    S = Stream()
    for span in (0xfffffd, 0xfffffe, 0xffffff, 0x1000000):
        S.add(_ops_record(S.i, [(0, 1), (3, span - 2), (0, 1)], flag=0))
        S.add(_ops_record(S.i, [(0, 1), (3, span - 2), (0, 1)], flag=0x400, mapq=70))
        S.add(rec(S.i))
    out.append(Case("D_spans", "D", "spans either side of the packed record's escape", S))
    S = Stream()
    S.fill_to(S.skip + SEG - 200)
    for a in range(9):
        S.add(_ops_record(S.i, [(4, 5), (a, 40), (3, 1000 + a), (0, 7), (5, 3)], flag=0))
    out.append(Case("D_cigar_first_last", "D", "five-operation CIGARs astride a segment boundary: first and last word, N in the span", S))
    return out


def _aux(tag, typ, payload):
    return tag.encode() + typ.encode() + payload


def _sa(i):
    return _aux("SA", "Z", b"c3,%d,-,30M20S,60,1;\x00" % (100 + i))


def _barr(sub, values):
    fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]
    return sub.encode() + struct.pack("<I", len(values)) + struct.pack("<%d%s" % (len(values), fmt), *values)


def _family_e():
    out = []

    def case(name, aim, auxes, **kw):
        S = Stream()
        S.add(rec(0))
        for a in auxes:
            S.add(with_aux(rec(S.i, tags=[]), a))
            if S.i % 4 == 0:
                S.add(rec(S.i))
        S.add(rec(S.i))
        out.append(Case(name, "E", aim, S, **kw))

    nm, xs = _aux("NM", "i", struct.pack("<i", 3)), _aux("XS", "Z", b"hello\x00")
    case("E_sa_position", "SA:Z as the first, a middle and the last field; an empty SA value; no aux at all",
         [_sa(1) + nm + xs, nm + _sa(2) + xs, nm + xs + _sa(3), _sa(4), _aux("SA", "Z", b"\x00"), nm + _aux("SA", "Z", b"\x00") + xs, b"", nm + xs,
          _sa(5) + _sa(6)], sa_by_oracle=False)
    others = [_aux("XA", "A", b"x"), _aux("Xc", "c", b"\xff"), _aux("XC", "C", b"S"), _aux("Xs", "s", b"SA"), _aux("XS", "S", b"AZ"),
              _aux("Xi", "i", b"SAZ\x00"), _aux("XI", "I", b"\x00SAZ"), _aux("Xf", "f", b"SAZS"), _aux("Xd", "d", b"SAZSAZSA"),
              _aux("XZ", "Z", b"text\x00"), _aux("XZ", "Z", b"\x00"), _aux("XH", "H", b"1AE301\x00")]
    for sub in "cCsSiIf":
        others.append(_aux("XB", "B", _barr(sub, [1, 2, 3])))
        others.append(_aux("XB", "B", _barr(sub, [])))
    case("E_sa_behind_types", "SA:Z behind every other aux type, B arrays of every subtype and of count 0",
         [o + _sa(k) for k, o in enumerate(others)] + [b"".join(others) + _sa(99)], loose_aux=True, sa_by_oracle=False)
    case("E_lookalikes", "the bytes SAZ inside a Z value, an H value and a B:C array: no match",
         [_aux("XZ", "Z", b"xxSAZyy\x00"), _aux("XH", "H", b"SAZ\x00"), _aux("XB", "B", _barr("C", [1, 0x53, 0x41, 0x5a, 0x31, 0, 9])),
          _aux("XZ", "Z", b"xxSAZyy\x00") + _sa(1), _aux("XB", "B", _barr("C", [0x53, 0x41, 0x5a, 0x31, 0])) + _sa(2), _aux("XS", "A", b"Z") + nm,
          _aux("XS", "Z", b"AZ\x00"), _aux("XS", "A", b"S") + _aux("AZ", "i", b"abc\x00")])
    case("E_sa_not_Z", "an SA tag whose type is not Z, and no other SA tag; and one in front of a real SA:Z",
         [_aux("SA", "i", struct.pack("<i", 5)), _aux("SA", "A", b"x") + nm, _aux("SA", "H", b"AB\x00"), _aux("SA", "B", _barr("C", [65, 66, 0])),
          _aux("SA", "i", struct.pack("<i", 5)) + _sa(7)], sa_by_oracle=False)
    case("E_stray_bytes", "aux areas that end in 1 or 2 stray bytes",
         [nm + b"S", nm + b"SA", _sa(1) + b"X", _sa(2) + b"XY", b"S", b"SA", nm + xs + b"\x00"], loose_aux=True, sa_by_oracle=False)
    u32 = lambda v: struct.pack("<I", v)
    unknown, open_z = _aux("Xq", "q", b"1234"), _aux("XZ", "Z", b"open")
    past, subtype, short = _aux("XB", "B", b"C" + u32(1 << 20) + b"abc"), _aux("XB", "B", b"q" + u32(2) + b"ab"), _aux("XB", "B", b"C\x01")
    case("E_malformed_first", "an unknown type, a Z without NUL up to the record end, a B whose count runs past the record, a B of unknown subtype: "
         "in front of a real SA:Z; an SA:Z that itself has no NUL",
         [unknown + _sa(1), open_z + _sa(2)[:-1], past + _sa(3), subtype + _sa(4), _aux("SA", "Z", b"unterminated"), nm + _aux("SA", "Z", b"c1,5")],
         loose_aux=True, sa_by_oracle=False)
    case("E_malformed_behind", "the same malformed fields, and a B cut short, behind a real SA:Z",
         [_sa(k) + b for k, b in enumerate((unknown, open_z, past, subtype, short))], loose_aux=True, sa_by_oracle=False)
    return out


def _decoy(i, size=None, bs=None):
    """bytes that read as a complete plausible record: in-range tids, a printable NUL-terminated name, n_cigar 0, l_seq 0"""
    r = rec(1000 + i, size=size, bare=True, tid=1, mate_tid=2, qname="dcy", flag=0, mapq=9, pos=77 + i, mate_pos=5, tlen=0)
    return r if bs is None else struct.pack("<I", bs) + r[4:]


def _straddler(S, start, decoy_at, end, kind, where="B", i=0):
    """the next record of S starts at `start` and ends at `end`; from `decoy_at` its B:C array (or its qualities) hold a decoy:
    complete = ends where the record ends, weak = a block_size past any batch, broken = a complete record followed by zeros"""
    S.fill_to(start)
    name = "r%d" % S.i
    if where == "B":
        n = end - start - len(rec(S.i, bare=True, tags=[("XB", "BC", [])]))
    else:
        while (end - start - len(rec(S.i, bare=True, qname=name))) % 3:     # l_seq = n (even): n / 2 sequence bytes + n qualities
            name += "n"
        n = (end - start - len(rec(S.i, bare=True, qname=name))) // 3 * 2
    data0 = end - n
    assert data0 < decoy_at
    if kind == "complete":
        d = _decoy(i, size=end - decoy_at)
    elif kind == "weak":
        d = _decoy(i, size=40, bs=1 << 27)
    else:
        d = _decoy(i, size=60)
    data = bytes(decoy_at - data0) + d
    data += bytes(n - len(data))
    r = rec(S.i, bare=True, tags=[("XB", "BC", list(data))]) if where == "B" else rec(S.i, bare=True, qname=name, seq="A" * n, qual=data)
    assert len(r) == end - start
    S.add(r)
    return {"off": decoy_at, "kind": kind, "len": len(d)}


def _family_f():
    out = []
    S = Stream()
    d = _straddler(S, SEG - 300, SEG + 40, SEG + 500, "complete")
    S.fill_to(2 * SEG + 3000)
    out.append(Case("F_complete", "F", "a complete decoy behind a boundary, ending where the straddling record ends", S, chased=[0], decoys=[d]))
    S = Stream()
    S.fill_to(S.skip + 3000)
    c0 = len(S)
    S.add(rec(S.i, size=260))
    d = _straddler(S, c0 + 2 * SEG - 300, c0 + 2 * SEG + 40, c0 + 2 * SEG + 500, "complete", i=1)
    S.fill_to(c0 + 3 * SEG + 1000)
    out.append(Case("F_complete_carry", "F", "the same in a second batch behind a carry", S, pushes=[c0 + 17, len(S) - c0 - 17], chased=[1], decoys=[d]))
    S = Stream()
    d = _straddler(S, SEG - 300, SEG + 41, SEG + 500, "complete", where="Q", i=2)
    S.fill_to(2 * SEG + 3000)
    out.append(Case("F_in_qualities", "F", "a complete decoy in the qualities of the straddling record", S, chased=[0], decoys=[d]))
    S = Stream()
    d = _straddler(S, 2 * SEG - 300, 2 * SEG + 40, 2 * SEG + 500, "weak", i=3)
    x = len(S)
    S.add(rec(S.i, size=400))
    S.fill_to(x + 400 + 3000)
    out.append(Case("F_last_segment", "F", "a weak decoy in the last segment, in front of the true partial record", S, pushes=[x + 100, len(S) - x - 100],
                    chased=[0], decoys=[d]))
    S = Stream()
    d = _straddler(S, SEG - 300, SEG + 40, SEG + 500, "weak", i=4)
    S.fill_to(2 * SEG + 3000)
    out.append(Case("F_weak_mid", "F", "a decoy whose block_size runs past the batch, a true chain behind it: not chased", S, chased=[], decoys=[d]))
    S = Stream()
    d = _straddler(S, SEG - 300, SEG + 40, SEG + 500, "broken", i=5)
    S.fill_to(2 * SEG + 3000)
    out.append(Case("F_broken_chain", "F", "a plausible record whose chain leads into zeros: the search goes on, not chased", S, chased=[], decoys=[d]))
    S = Stream()
    d0 = _straddler(S, SEG - 300, SEG + 40, SEG + 500, "broken", i=6)
    d1 = _straddler(S, 2 * SEG - 300, 2 * SEG + 40, 2 * SEG + 500, "complete", i=7)
    S.fill_to(3 * SEG + 3000)
    out.append(Case("F_two", "F", "a chain-broken decoy in one segment and a complete one in the next: one chase", S, chased=[0], decoys=[d0, d1]))
    return out


def _family_g():
    out = []
    S = Stream()
    S.fill_to(S.skip + SEG + 4000)
    S.add(rec(S.i, tid=len(REFS), pos=123456))
    S.fill_to(2 * SEG + 5000)
    x = len(S)
    S.fill_to(x + 6000)
    out.append(Case("G_tid_beyond_n_ref", "G", "a mid-stream record with tid = n_ref", S, pushes=[x, len(S) - x], chased=[0]))
    S = Stream()
    S.fill_to(S.skip + 5000)
    S.add(rec(S.i, tid=len(REFS) + 3, pos=654321))
    S.fill_to(2 * SEG + 5000)
    out.append(Case("G_tid_beyond_first_segment", "G", "the same in the batch's first segment, whose chain starts at the known first record", S, chased=[0]))
    S = Stream()
    S.fill_to(SEG + 57)
    S.add(rec(S.i, cigar="20M5S", seq="ACGT" * 10))
    S.fill_to(2 * SEG + 5000)
    out.append(Case("G_cigar_query_length", "G", "CIGAR query length 25, l_seq 40, on the first record behind a boundary", S, chased=[0],
                    aims=[{"kind": "first_behind", "batch": 0, "rec": S.starts.index(SEG + 57), "segment": 1}]))
    S = Stream()
    S.fill_to(SEG + 57)
    S.add(rec(S.i, qname="a name"))
    S.fill_to(2 * SEG + 5000)
    out.append(Case("G_name_byte", "G", "a blank in the name of the first record behind a boundary", S, chased=[0],
                    aims=[{"kind": "first_behind", "batch": 0, "rec": S.starts.index(SEG + 57), "segment": 1}]))
    return out


def _cut_blocks(n, cuts):
    """inflated block sizes (each <= 0xff00) whose boundaries include every offset of `cuts`"""
    sizes, o = [], 0
    for c in list(cuts) + [n]:
        while o < c:
            sizes.append(min(0xff00, c - o))
            o += sizes[-1]
    return sizes


def _family_h():
    out = []

    def case(name, aim, S, own, **kw):
        sizes = _cut_blocks(len(S), [own])
        j = next(k for k in range(len(sizes) + 1) if sum(sizes[:k]) == own)
        out.append(Case(name, "H", aim, S, shard=(sizes, j), **kw))

    S = Stream()
    S.fill_to(S.skip + 3 * SEG)
    case("H_clean", "a clean stream cut at a block boundary inside a record", S, S.starts[len(S.starts) // 2] + 100)
    S = Stream()
    S.fill_to(S.skip + 3 * SEG)
    case("H_on_record_start", "own_bytes falls exactly on a record start", S, S.starts[len(S.starts) // 2])
    S = Stream()
    S.fill_to(S.skip + 3 * SEG)
    case("H_one_behind_start", "own_bytes falls one byte behind a record start", S, S.starts[len(S.starts) // 2] + 1)
    S = Stream()
    d = _straddler(S, S.skip + SEG + 3000, S.skip + SEG + 3400, S.skip + SEG + 3900, "complete", i=8)
    S.fill_to(S.skip + 3 * SEG)
    case("H_decoy_at_seam", "shard 1 starts 20 bytes in front of a complete decoy: the seam disagrees", S, d["off"] - 20, decoys=[d])
    return out


def _family_i():
    out = []

    def case(name, aim, tids, pushes_at=(), **kw):
        S = Stream()
        cuts = []
        for k, t in enumerate(tids):
            if k in pushes_at:
                cuts.append(len(S))
            S.add(_tiny(S.i, 38 + k % 3, tid=t))
        p, o = [], 0
        for c in cuts + [len(S)]:
            p.append(c - o)
            o = c
        out.append(Case(name, "I", aim, S, pushes=p, **kw))

    case("I_one_run", "one run", [2] * 500)
    alt = lambda n: [(0, 1, 3, 2, 0, 2, 1, 3)[k % 8] for k in range(n)]
    case("I_runs_at_cap", "ING_EDGES runs: reported, in order, with their tids", alt(EDGES), aims=[{"kind": "runs", "batch": 0, "n": EDGES}])
    case("I_runs_over_cap", "ING_EDGES + 1 runs: the overflow marker", alt(EDGES + 1), aims=[{"kind": "runs", "batch": 0, "n": None}])
    case("I_first_and_last", "a tid change on the first and on the last record of both batches", [0] + [1] * 300 + [2] + [3] + [1] * 200 + [0],
         pushes_at=(302,), aims=[{"kind": "edges", "batch": 0, "edges": [0, 1, 301]}, {"kind": "edges", "batch": 1, "edges": [0, 1, 201]}])
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = []
        for f in (_family_a, _family_b, _family_c, _family_d, _family_e, _family_f, _family_g, _family_h, _family_i):
            _CASES += f()
        names = [c.name for c in _CASES]
        assert len(set(names)) == len(names)
        # further routes: one case of every family with a second histogram attached (a bin size with a binned form, one without);
        # one case of A and of C with the spans begun through tdt_ingest_push_ahead
        for name in ("A2_start_m3", "B_65", "C_tail_3", "D_spans", "E_sa_position", "F_complete_carry", "G_tid_beyond_n_ref", "I_first_and_last"):
            get(name).routes += ("second_binned", "second_generic")
        for name in ("A2_end_p0", "C_three_tails"):
            get(name).routes += ("ahead",)
    return _CASES


def get(name):
    for c in _CASES if _CASES is not None else cases():
        if c.name == name:
            return c
    raise KeyError(name)


def by_family(f):
    return [c for c in cases() if c.family == f]


def ledger():
    """every (case, route) the device file must run"""
    return sorted((c.name, r) for c in cases() for r in c.routes)


def shard_expectation(case, mutant=None):
    """family H: what the two bounded pushes give.  shard 0 decodes the records that start in front of own_bytes and reports where the
    next one starts (next_off, from own_bytes); shard 1, fed from the block boundary with an unknown start, reports its first guess
    (first_off) and decodes from there"""
    R = case.reference()
    _, _, own = case.shard_blocks()
    n0 = int(np.count_nonzero(R["rec_off"] < own))
    m0 = guess_and_confirm(case.stream, case.skip, case.n_ref, limit=own, mutant=mutant)
    m1 = guess_and_confirm(case.stream[own:], None, case.n_ref, mutant=mutant)
    return {"own": own, "n0": n0, "next_off": int(R["rec_end"][n0 - 1]) - own, "model0": m0, "model1": m1}
