"""Random LEGAL records for every consumer of the ``--sv`` scan: what tests/scan_all_cases.py is for designed records, for records nobody
designed.  :func:`generate` writes a coordinate-sorted BAM over ``scan_all_cases.contigs()`` whose sequences are cut from
``scan_all_cases.reference()``, with the same FASTA, sites VCF, STR catalogue and family library beside it, so that ``partial``,
``combine`` and ``write_definition_files`` of that module apply to it unchanged.  Everything derives from the seed.

A record is legal when ``bamio.BamReader`` and the device's record check accept it: ``tid`` and ``mate_tid`` in ``[-1, contigs)``, ``pos``
and ``mate_pos`` at least -1, a name of ``[!-~]``, and a CIGAR whose query length is ``l_seq`` wherever ``l_seq`` is not 0.

About 40 % of the records are BACKGROUND: a CIGAR of 1 ... 12 operations over all nine codes (``H`` outermost, ``S`` inside it, lengths
1 ... 300 biased small, ``N`` up to 50 000; a share with no reference-consuming operation, a share that is one ``M``); the reference's
bases under the aligned operations changed at a per-read rate of 0, 0.5, 3 or 20 %, about 1 % IUPAC codes, inserted and clipped bases
random, ``l_seq = 0`` on about 5 %; qualities 0 ... 60, all ``0xff`` on about 5 %; about 45 % of the flags drawn to pass the ``0xF04``
gate, the rest any of the twelve bits; MAPQ uniform over ``MAPQS``; unmapped reads with and without a placement and a tail of unplaced
ones; reads from base 0, reads that end on a contig's last base, one that hangs over it, reads on the small contigs; mates on the same
contig, another one, none, ``tlen`` on both sides of ``MAX_INS``; names of 1 ... 250 characters, every eighth record or so under the name
of an earlier one; aux fields of every type, ``MC:Z`` on about half of the paired reads and ``SA:Z`` on about 10 %, a few of both odd.
Every record of the file also carries an array of up to 240 random integers (``XR:B:i``) somewhere among its aux fields: the device
reader takes a file's last MiB along with the span in front of it, and these bytes, which do not compress, make 4 000 records a file of
more than two dozen 64-KiB spans.

About 60 % are drawn round ``HOT`` grid points of the reference — their indel position, allele sites and STR locus: the SAME event
carried by 2 ... 6 reads on both strands (an indel, an indel of one unit of the planted repeat, a substitution, reads that span, enter
and leave the STR locus, reads clipped beside one breakpoint — these with ``SA:Z`` on 10 % and an empty sequence on 5 %, as the
background), duplicate sets as scan_all_cases plants them, and clip-site events from its planter (a deletion, a junction to
another contig, facing sites round an insertion cut from the family library), five reads per junction side: the clip chain behind the
scan gets rows in every stage.  The MAPQ of these reads is uniform over the values of ``MAPQS`` that pass the cut of 20."""
import numpy as np

import scan_all_cases as C

RECORDS = 4000
SEEDS = (1, 2, 3, 4, 5, 6)
HOT = 150
HOT_SHARE = 0.6
MAPQS = (0, 4, 5, 6, 19, 20, 21, 29, 30, 59, 60, 254, 255)
RATES = (0.0, 0.005, 0.03, 0.2)
_M, _I, _D, _N, _S, _H, _P, _EQ, _X = range(9)
_PRINTABLE = [chr(c) for c in range(33, 127) if chr(c) != "@"]
_IUPAC = "NRYSWKMBDHVN"
_REFERENCE = []


def _reference():
    if not _REFERENCE:
        _REFERENCE.append(C.reference())
    return _REFERENCE[0]


class _Gen(C._Planter):
    """scan_all_cases' planter (its reads, pairs, duplicate sets and clip-site events) with a seed of its own, and the random records"""

    def __init__(self, table, seqs, sites, seed):
        super().__init__(table, seqs)
        self.rng = np.random.default_rng([C.SEED, 7, seed])
        self.sites = sites
        self.names = []
        self.done = set()
        self.count = {"hot": 0, "background": 0, "tail": 0, "drawn": 0}          # drawn: the reads with a CIGAR that get SA:Z and an empty sequence at random

    # ---- pieces
    def pick(self, values):
        return values[int(self.rng.integers(0, len(values)))]

    def text(self, n, alphabet="ACGT"):
        return "".join(alphabet[int(x)] for x in self.rng.integers(0, len(alphabet), n))

    def qual(self, n, at=None):
        if self.rng.random() < 0.05:
            return b"\xff" * n
        q = self.rng.integers(0, 61, n, dtype=np.uint8)
        if at is not None and 0 <= at < n:
            q[at] = 30 + int(self.rng.integers(0, 31))                         # (the event's own base passes every base-quality cut)
        return bytes(q.tolist())

    def ballast(self):
        """an array of up to 240 random 32-bit integers: bytes no compressor shortens, so that a file of a few thousand records is dozens
        of 64-KiB spans of compressed data, with records that straddle them, and every walk over the aux fields has something to hop over"""
        n = int(self.rng.integers(0, 241))
        return ("XR", "Bi", self.rng.integers(-2 ** 31, 2 ** 31, n).tolist())

    def add(self, qname, flag, tid, pos, mapq, cigar, seq, qual, mate_tid=-1, mate_pos=-1, tlen=0, tags=()):
        from tiddit_amd import bamio
        tags = list(tags)
        tags.insert(int(self.rng.integers(0, len(tags) + 1)), self.ballast())
        self.recs.append((tid, pos, bamio.encode_record(qname, flag, tid, pos, mapq, cigar, mate_tid, mate_pos, tlen, seq, tags, qual)))

    def put(self, qname, flag, tid, pos, cigar, seq, mate_tid=-1, mate_pos=-1, tlen=0, tags=(), mapq=60):
        """(the planter's records: its qualities of 2 ... 40, and the ballast)"""
        super().put(qname, flag, tid, pos, cigar, seq, mate_tid, mate_pos, tlen, tuple(tags) + (self.ballast(),), mapq)

    def sequence(self, tid, pos, cigar, rate=0.0, change=None, ins=None):
        """the query of a CIGAR at pos: the reference under M = X (changed at ``rate``; ``change`` = {reference position: base}), ``ins``
        or random bases under I, random ones under S -> (text, {reference position: query index})"""
        out, at, r = [], {}, pos
        L = self.table[tid][1]
        for op, ln in cigar:
            if op in (_M, _EQ, _X):
                b = list(self.bases(tid, r, ln).ljust(ln, "N"))                # (beyond the contig's end: N)
                for i in range(ln):
                    if change and r + i in change:
                        at[r + i] = sum(len(x) for x in out) + i
                        b[i] = change[r + i]
                    elif rate and self.rng.random() < rate and r + i < L:
                        b[i] = self.pick([c for c in "ACGT" if c != b[i]])
                out.append("".join(b))
                r += ln
            elif op in (_D, _N):
                r += ln
            elif op in (_I, _S):
                out.append(ins if op == _I and ins is not None else self.text(ln))
        return "".join(out), at

    def aux(self):
        tags = []
        for _ in range(int(self.rng.integers(0, 5))):
            ty = self.pick(["A", "c", "C", "s", "S", "i", "I", "f", "Z", "H", "BC", "Bs", "Bi", "Bf"])
            val = {"A": "q", "c": -5, "C": 200, "s": -3000, "S": 60000, "i": -70000, "I": 4000000000, "f": 1.5, "Z": "some text", "H": "1AE301",
                   "BC": [1, 2, 3], "Bs": [-1, 5], "Bi": list(range(int(self.rng.integers(0, 40)))), "Bf": [0.5]}[ty]
            tags.append(("X" + self.pick(list("ABCDEFGH")), ty, val))
        return tags

    def sa_text(self):
        """an SA:Z value naming a real contig; one in six is odd: two entries, no closing ``;``, a CIGAR with H / D / I, a mapQ of 0"""
        name, L = self.pick(self.table)
        p = 1 + int(self.rng.integers(0, L - 200))
        plain = "%s,%d,%s,%dS%dM,%d,%d;" % (name, p, self.pick("+-"), int(self.rng.integers(1, 80)), int(self.rng.integers(20, 100)), self.pick(MAPQS), int(self.rng.integers(0, 5)))
        if self.rng.random() >= 1 / 6:
            return plain
        return self.pick([plain + "%s,7,-,50M50S,60,0;" % self.table[0][0], plain[:-1], "%s,%d,-,10H30M2D10M3I20M25S,60,1;" % (name, p), "%s,%d,+,40M60S,0,0;" % (name, p)])

    def mc_text(self):
        if self.rng.random() < 0.06:
            return self.pick(["*", "100", "M100", "12Q", ""])                     # (not a CIGAR text)
        return self.pick(["100M", "%dS%dM" % (int(self.rng.integers(1, 40)), int(self.rng.integers(20, 100))), "50M%dN50M" % int(self.rng.integers(1, 5000)),
                          "%dM%dS" % (int(self.rng.integers(20, 100)), int(self.rng.integers(1, 40))), "30M2D70M", "5H95M"])

    def qname(self):
        if self.names and self.rng.random() < 0.13:
            return self.pick(self.names[-200:])                                  # (a name two or three records share)
        n = self.text(self.pick([1, 2, 5, 12, 20, 40, 100, 250]), _PRINTABLE)
        self.names.append(n)
        return n

    def mate(self, tid, pos):
        """-> (mate_tid, mate_pos, tlen): the same contig (tlen on both sides of MAX_INS), another one, or none"""
        u = self.rng.random()
        if u < 0.55:
            t = self.pick([C.MAX_INS - 1, C.MAX_INS, C.MAX_INS + 1, int(self.rng.integers(0, 2 * C.MAX_INS)), int(self.rng.integers(0, 400))])
            sign = 1 if self.rng.random() < 0.5 else -1
            return tid, min(self.table[tid][1] - 1, max(0, pos + sign * t)), sign * t
        if u < 0.8:
            t2 = int(self.rng.integers(0, len(self.table)))
            return t2, int(self.rng.integers(0, self.table[t2][1])), 0
        return -1, -1, 0

    # ---- the background
    def cigar(self):
        u = self.rng.random()
        ln = lambda: int(self.pick([1, 1, 2, 3, 5, 8, 13, 25, 40, 60, 100, 150, 300, int(self.rng.integers(1, 301))]))
        if u < 0.15:
            return [(_M, int(self.rng.integers(1, 301)))]
        if u < 0.22:                                                             # no reference-consuming operation
            core = [(self.pick([_I, _S, _P]), ln()) for _ in range(int(self.rng.integers(1, 4)))]
        else:
            core, long = [], True                                                # (one long skip per read at the most: it has to fit a contig)
            for _ in range(int(self.rng.integers(1, 9))):
                op = self.pick([_M, _M, _M, _M, _I, _D, _N, _P, _EQ, _X])
                if op == _N and long and self.rng.random() < 0.5:
                    core.append((op, int(self.pick([50000, int(self.rng.integers(301, 50001))]))))
                    long = False
                else:
                    core.append((op, ln()))
        core = [(op, n) for op, n in core if op != _S]
        lead = [(_H, ln())] * (self.rng.random() < 0.15) + [(_S, ln())] * (self.rng.random() < 0.35)
        trail = [(_S, ln())] * (self.rng.random() < 0.35) + [(_H, ln())] * (self.rng.random() < 0.15)
        if not core:
            core = [(_I, ln())]
        return lead + core + trail                                               # (12 operations at the most)

    def flag(self):
        if self.rng.random() < 0.45:                                             # passes the 0xF04 gate
            return sum(b for b in (0x1, 0x2, 0x8, 0x10, 0x20, 0x40, 0x80) if self.rng.random() < 0.4)
        return sum(1 << i for i in range(12) if self.rng.random() < 0.25)

    def place(self, ref_len, where=None):
        """a contig and a start such that the alignment lies on the contig"""
        for _ in range(100):
            tid = int(self.rng.integers(0, len(self.table))) if where is None else where
            L = self.table[tid][1]
            if ref_len <= L:
                return tid, int(self.rng.integers(0, L - ref_len + 1))
            where = None
        raise AssertionError("no contig holds %d bases" % ref_len)

    def background_read(self, how=None):
        rng = self.rng
        flag, mapq = self.flag(), self.pick(MAPQS)
        if how is None and rng.random() < 0.05:                                  # unmapped, no CIGAR; with and without a placement
            lseq = int(rng.integers(0, 200))
            tid, pos = self.place(1) if rng.random() < 0.5 else (-1, -1)
            mt, mp, tl = self.mate(tid, pos) if tid >= 0 else (-1, -1, 0)
            self.add(self.qname(), flag | 0x4, tid, pos, mapq, [], self.text(lseq, "ACGTN"), self.qual(lseq), mt, mp, tl, self.aux())
            return
        cigar = self.cigar()
        while how in ("first", "last") and cigar[-1][0] not in (_M, _EQ, _X):   # (a read that ends ON a base ends with an aligned one ...
            cigar = self.cigar()
        if how in ("first", "last"):
            flag &= ~0x4                                                         #  ... and is mapped: an unmapped read's end is pos + 1)
        ref_len = sum(n for op, n in cigar if op in (_M, _D, _N, _EQ, _X))
        tid, pos = self.place(max(ref_len, 1))
        L = self.table[tid][1]
        if how == "first":
            pos = 0
        elif how == "last":
            pos = L - max(ref_len, 1)
        elif how == "small":
            tid, pos = self.place(max(ref_len, 1), len(self.table) - 1 - int(rng.integers(0, 2)))
        seq, _ = self.sequence(tid, pos, cigar, self.pick(RATES))
        seq = "".join(self.pick(_IUPAC) if rng.random() < 0.01 else c for c in seq)
        if rng.random() < 0.05:
            seq = ""
        mt, mp, tl = self.mate(tid, pos)
        tags = self.aux()
        if flag & 0x1 and rng.random() < 0.5:
            tags.insert(int(rng.integers(0, len(tags) + 1)), ("MC", "Z", self.mc_text()))
        if rng.random() < 0.1:
            tags.insert(int(rng.integers(0, len(tags) + 1)), ("SA", "Z", self.sa_text()))
        self.count["drawn"] += 1
        self.add(self.qname(), flag, tid, pos, mapq, cigar, seq, self.qual(len(seq)), mt, mp, tl, tags)

    # ---- the hot spots: one event, 2 ... 6 reads, both strands
    def carriers(self, tid, make, near=False):
        """``make(j)`` -> (pos, cigar, change, the reference position whose base must pass the quality cuts, the inserted bases); 2 ... 6
        unpaired or paired reads (``near``: every one paired, its mate close by on the same contig)"""
        n = int(self.rng.integers(2, 7))
        for j in range(n):
            pos, cigar, change, mark, ins = make(j)
            seq, at = self.sequence(tid, pos, cigar, self.pick(RATES[:3]) if self.rng.random() < 0.3 else 0.0, change, ins)
            flag = 0x10 * (j % 2)
            mt, mp, tl = -1, -1, 0
            if near or self.rng.random() < 0.4:
                flag |= 0x1 | self.pick([0x40, 0x80]) | (0x20 if not flag & 0x10 else 0) | self.pick([0, 0x2])
                mt, mp, tl = (tid, pos + 300, 400) if near else self.mate(tid, pos)
            tags = self.aux() if self.rng.random() < 0.3 else []
            if self.rng.random() < 0.1:                                          # (SA:Z and the empty sequence at the background's shares)
                tags.append(("SA", "Z", self.sa_text()))
            if self.rng.random() < 0.05:
                seq = ""
            self.count["drawn"] += 1
            self.add(self.name("h"), flag, tid, pos, self.pick([q for q in MAPQS if q >= 20]), cigar, seq, self.qual(len(seq), at.get(mark)), mt, mp, tl, tags)

    def hot_indel(self, k, tid, g):
        p = g + 120
        if k % 2:
            n, ins = 1 + k % 30, None
        else:
            n = 1 + k % 40                                                       # (over 22 bases: the hashed payload)
            ins = "".join("ACGT"[(k + 3 * i * i) % 4] for i in range(n))

        def make(j):
            a, b = 20 + int(self.rng.integers(0, 60)), 20 + int(self.rng.integers(0, 60))
            clip = [(_S, int(self.rng.integers(1, 20)))] * (self.rng.random() < 0.3)
            return p - a, clip + [(_M, a), (_D if ins is None else _I, n), (_M, b)], None, None, ins
        self.carriers(tid, make)

    def hot_unit(self, k, tid, g):
        """one unit of the planted repeat deleted or inserted, every read at another unit (scan_all_cases' repeat events)"""
        unit, _ = C.repeat_of(k)
        u = len(unit)
        for j in range(int(self.rng.integers(2, 5))):
            at = g + 200 + 2 * u * j
            a = 30 + int(self.rng.integers(0, 40))
            if k % 2:
                self.read(tid, at - a, [(_M, a), (_D, u), (_M, 100 - a)], j % 2, what="hu")
            else:
                self.read(tid, at - a, [(_M, a), (_I, u), (_M, 100 - u - a)], j % 2, unit, what="hu")

    def hot_sub(self, k, tid, g):
        p = self.pick([x for x in C.site_positions(g) if x < self.table[tid][1] - 200] + [g + 250])
        ref = self.bases(tid, p, 1)
        alt = "ACGT"[("ACGT".index(ref) + 1 + k % 3) % 4]

        def make(j):
            a, b = 10 + int(self.rng.integers(0, 80)), 10 + int(self.rng.integers(0, 80))
            lead = [(_S, int(self.rng.integers(1, 40)))] * (self.rng.random() < 0.25)
            return p - a, lead + [(self.pick([_M, _M, _M, _X]), a + 1 + b)], {p: alt}, p, None
        self.carriers(tid, make)

    def hot_str(self, k, tid, g):
        """reads that span the locus at g + 200 ... g + 216, that enter it from the left and end inside it, and that start inside it"""
        s, e = g + 200, g + 216

        def make(j):
            kind = (j + k) % 3
            if kind == 0:
                a, b = 10 + int(self.rng.integers(0, 60)), 10 + int(self.rng.integers(0, 60))
                return s - a, [(_M, a + 16 + b)], None, None, None
            if kind == 1:
                a, inside = 10 + int(self.rng.integers(0, 60)), 1 + int(self.rng.integers(0, 15))
                return s - a, [(_M, a + inside)] + [(_S, int(self.rng.integers(1, 30)))] * (self.rng.random() < 0.5), None, None, None
            inside, b = 1 + int(self.rng.integers(0, 15)), 10 + int(self.rng.integers(0, 60))
            return e - inside, [(_S, int(self.rng.integers(1, 30)))] * (self.rng.random() < 0.5) + [(_M, inside + b)], None, None, None
        self.carriers(tid, make)

    def hot_soft(self, k, tid, g):
        """paired reads clipped by more than MIN_CLIP bases beside more than MIN_ANCHOR aligned ones, at one breakpoint: the signal
        predicates' clip rows, and one more clip site"""
        p, left = g + 420 + k % 7, k % 2

        def make(j):
            s, m = C.MIN_CLIP + 1 + int(self.rng.integers(0, 40)), C.MIN_ANCHOR + 1 + int(self.rng.integers(0, 60))
            return (p, [(_S, s), (_M, m)], None, None, None) if left else (p - m, [(_M, m), (_S, s)], None, None, None)
        self.carriers(tid, make, near=True)

    def hot_clip(self, k, tid, g, points):
        if (k, "clip") in self.done or not 1000 <= g or g + 700 > self.table[tid][1]:
            return
        self.done.add((k, "clip"))
        kind = len(self.done) % 4
        if kind == 0:                                                            # (the planter raises where the window holds no deletion of the kind asked for)
            self.deletion(k, tid, g, False)
        elif kind == 1:
            self.translocation(k, tid, g, points)
        else:
            self.insertion(len(self.done), tid, g + 100, kind == 3)

    def tandem_insertion(self, tid, b):
        """facing sites round 48 inserted bases of a dinucleotide repeat: the pair closes at more than one length (``closed_multi``)"""
        s = self.seqs[self.table[tid][0]]
        ins = ("CA" if chr(s[b]) != "C" and chr(s[b - 1]) != "A" else "GT") * 24
        self.r_site(tid, b, (ins + self.bases(tid, b, 60))[:60], C.INS_ANCHORS)
        self.l_site(tid, b, (self.bases(tid, b - 60, 60) + ins)[-60:], C.INS_ANCHORS)

    def hot(self, budget, points):
        spots = [points[int(i)] for i in self.rng.choice(len(points), min(HOT, len(points)), replace=False)]
        n0 = len(self.recs)
        _, tid, g = spots[0]
        self.tandem_insertion(tid, g + 260)
        while len(self.recs) - n0 < budget:
            k, tid, g = self.pick(spots)
            u = self.rng.random()
            if u < 0.2:
                self.hot_indel(k, tid, g)
            elif u < 0.3:
                self.hot_unit(k, tid, g)
            elif u < 0.5:
                self.hot_sub(k, tid, g)
            elif u < 0.7:
                self.hot_str(k, tid, g)
            elif u < 0.78:
                self.dups(k, tid, g)
            elif u < 0.9:
                self.hot_soft(k, tid, g)
            else:
                self.hot_clip(k, tid, g, points)
        self.count["hot"] = len(self.recs) - n0

    def background(self, budget):
        n0 = len(self.recs)
        for how in ("first", "first", "last", "last", "small", "small", "small"):
            self.background_read(how)
        # over the end of the first contig, inside its last coverage bins: 5 aligned bases, and a deletion that reaches 1 base over it
        L = self.table[0][1]
        assert L % 100 <= 90
        for cigar, pos in (([(_M, 60)], L - 55), ([(_M, 30), (_D, 3), (_M, 4)], L - 32)):
            seq, _ = self.sequence(0, pos, cigar)
            self.add(self.qname(), self.pick([0, 0x10]), 0, pos, 60, cigar, seq, self.qual(len(seq)))
        # one deletion too long for a key, flanked on both sides (the indel counter's ``too_long``)
        self.add(self.qname(), 0, 0, 100, 60, [(_M, 30), (_D, 65536), (_M, 30)], self.bases(0, 100, 30) + self.bases(0, 100 + 30 + 65536, 30), self.qual(60))
        # a tandem duplication as an insertion: 1 100 inserted bases equal to the 1 100 reference bases in front of them, so the
        # left-normalisation shifts it base by base until its cap of 1 024 stops it (the indel counter's ``shift_capped``)
        n, P = 1100, 1101
        dup = self.bases(0, P - n, n)
        assert n > 1024 and len(dup) == n and set(dup) <= set("ACGT")
        self.add(self.qname(), 0, 0, P - 30, 60, [(_M, 30), (_I, n), (_M, 30)], self.bases(0, P - 30, 30) + dup + self.bases(0, P, 30), self.qual(n + 60))
        # five flanked deletions in one read (the indel counter's ``noisy_reads``), and a read without a CIGAR whose flags say mapped, on a
        # catalogued repeat (the STR counter's ``no_alignment``)
        tid, pos = self.place(200)
        cigar = [(_M, 10), (_D, 1)] * 5 + [(_M, 50)]
        seq, _ = self.sequence(tid, pos, cigar)
        self.add(self.qname(), 0x10, tid, pos, 60, cigar, seq, self.qual(len(seq)))
        _, tid, g = C.grid_points(self.table)[int(self.rng.integers(0, 100))]
        self.add(self.qname(), 0, tid, g + 205, 60, [], self.text(20), self.qual(20))
        while len(self.recs) - n0 < budget:
            self.background_read()
        self.count["background"] = len(self.recs) - n0

    def tail(self, n):
        for _ in range(n):
            lseq = int(self.rng.integers(0, 200))
            self.add(self.qname(), 0x4 | (0x1 | 0x8 | self.pick([0x40, 0x80])) * (self.rng.random() < 0.7), -1, -1, self.pick(MAPQS), [], self.text(lseq, "ACGTN"),
                     self.qual(lseq), -1, -1, 0, self.aux())
        self.count["tail"] = n


def generate(directory, seed, records=RECORDS):
    """write the BAM of this seed and what lies beside it into ``directory`` -> {"n_records", "hot", "background", "tail", "drawn"}"""
    table = C.contigs()
    seqs, sites = _reference()
    C.write_beside(directory, table, seqs, sites)
    G = _Gen(table, seqs, sites, seed)
    tail = records // 50
    G.hot(int(HOT_SHARE * records), C.grid_points(table))
    G.background(records - len(G.recs) - tail)
    G.tail(tail)
    tk = np.array([t if t >= 0 else 1 << 30 for t, _, _ in G.recs], dtype=np.int64)
    pk = np.array([p for _, p, _ in G.recs], dtype=np.int64)
    order = np.lexsort((np.arange(len(tk)), pk, tk))                             # (stable)
    C.write_records(C.paths(directory)[0], table, [G.recs[i][2] for i in order.tolist()])
    return dict(G.count, n_records=len(G.recs), sites=sites)


# ------------------------------------------------------------------------------------------- what a file must hold
# The smallest value of every quantity of :func:`measure` over the six seeds, from the definitions on the CPU, and half of it:
#   batches 23, records 4000, indel rows at support 3: 66 (89 left-normalised, 208 events shifted), SNV rows at support 3: 69, clip rows at
#   support 4: 110, extension keys 900, duplicate sets 16 of pairs and 85 of fragments (23 of size 4 and more), STR keys 326 span, 157 left,
#   145 right, 50 sets of support 3 and more, 50 loci genotyped, alleles counted at 188 sites from 559 reads, 216 reads selected as clip, 212
#   as split and 372 as discordant, chain rows 110 align, 110 far (20 of them placed by far alone), 19 ins, 28 mei, 48 VCF records (18 named)
FLOORS = {"batches": 11, "records": 2000, "indel_rows_top": 33, "norm_rows_top": 44, "norm_shifted": 104, "snv_rows_top": 34, "clip_rows_top": 55,
          "clip_ext_keys": 450, "dup_pair_sets": 8, "dup_fragment_sets": 42, "dup_sets_of_4_and_more": 11, "str_span_keys": 163, "str_left_keys": 78,
          "str_right_keys": 72, "str_sets_top": 25, "str_genotyped": 25, "allele_sites": 94, "allele_reads": 279, "signal_clip": 108, "signal_split": 106,
          "signal_discordant": 186, "chain_align": 55, "chain_far": 55, "chain_ins": 9, "chain_mei": 14, "chain_vcf": 24, "chain_far_only": 10,
          "chain_named": 9}
SPANS = 24                              # 64-KiB spans of compressed data in front of the last MiB, which the device reader takes in one piece


def measure(batches, E):
    """what the definitions find in a file, by name: the quantities ``FLOORS`` puts a floor under (rows of every
    keyed consumer at its highest tested support among them), so that no comparison with a device result passes on an empty table"""
    from tiddit_amd import tiddit_dup, tiddit_str
    out = {"batches": len(batches), "records": E["records"]}
    out["indel_rows_top"] = len(E["indels"][1][C.INDEL_SUPPORTS[-1]][1][0])
    out["norm_rows_top"] = len(E["indels_norm"][1][C.INDEL_SUPPORTS[-1]][1][0])
    out["norm_shifted"] = E["indels_norm"][2][0]
    out["snv_rows_top"] = len(E["snvs"][1][C.SNV_SUPPORTS[-1]][1][0])
    out["clip_rows_top"] = len(E["clips"][1][C.CLIP_SUPPORTS[-1]][1][0])
    out["clip_ext_keys"] = len(E["clip_ext"])
    hist = E["dups"][1][tiddit_dup.OFF_HIST:].reshape(-1, 2)                     # [size - 1][pair sets, fragment sets]
    out["dup_pair_sets"], out["dup_fragment_sets"] = int(hist[1:, 0].sum()), int(hist[1:, 1].sum())
    out["dup_sets_of_4_and_more"] = int(hist[3:].sum())
    keys, counts, cols, table = E["str"]
    for k in ("span_keys", "left_keys", "right_keys"):
        out["str_" + k] = int(counts[tiddit_str.SN_INDEX[k]])
    out["str_sets_top"] = int((cols[2] >= C.STR_S).sum())
    out["str_genotyped"] = sum(1 for t in table if t[2] is not None)
    out["allele_sites"] = int((E["alleles"][0][:, :4].sum(axis=1) > 0).sum())
    out["allele_reads"] = E["alleles"][1]
    kinds = [C.signal_kinds(b) for b in batches]
    for i, name in enumerate(("signal_clip", "signal_split", "signal_discordant")):
        out[name] = sum(int(k[i].sum()) for k in kinds)
    for stage in ("align", "far", "ins", "mei", "vcf"):
        out["chain_" + stage] = len(E["clip_chain"][stage][1])
    out["chain_far_only"] = sum(1 for a, f in zip(E["clip_chain"]["align"][1], E["clip_chain"]["far"][1]) if a[9] is None and f[10] is not None)
    out["chain_named"] = sum(1 for r in E["clip_chain"]["vcf"][1] if ";MEI=" in r)
    return out
