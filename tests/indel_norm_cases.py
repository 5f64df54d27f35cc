"""Aimed cases for the left-normalisation of the small-indel candidates (``TIDDIT_INDELS_NORM``: tiddit_indels.left_normalise,
indel_keys<true> of csrc/tdt_indel.hip) and for the resident reference under it (csrc/tdt_refseq.hip).

The reference is DESIGNED here, nothing comes from a genome: three contigs of 100 000, 49 999 (odd: the next contig's alignment in the
store is exercised) and 1000 bases of seeded random A C G T, into which :func:`_design` plants the features the cases aim at —
homopolymers of every length 1 ... 40, ``CA`` and ``CAG`` repeats, runs whose shifts end on the word and nibble edges of the kernel's
16-base steps, runs of CAP - 1 ... 3000 bases, an ``N``, an IUPAC code and a lower-case stretch inside runs, runs that touch both ends of
every contig.  Every planted feature sets its own flanks, so its shift is known from the case's own numbers.

A case is a dict as tests/indel_cases.py's (``reads cuts repeat capacity Q S lengths reader_ok``; its ``build`` / ``batches`` are used as they
are) plus ``family``, ``loaded`` (the contigs of the reference that are loaded) and ``want`` — the CLAIM, written from the design:
the (tid, P') of every keyed event in read order, or None where only the two references speak.  A read made by :func:`DEL` / :func:`INS` /
:func:`EVENTS` carries ``events``: what it was built from, [(P, n, inserted text or None)] — the restatement starts from those, not from
the CIGAR (tests/indel_cases.py pins the walk).

Two references, sharing no code:
  * the definition, ``tiddit_indels.keys_of_batch_by_read(ref=HostReference)``: a loop that compares one base with one base;
  * :func:`restate`: the event is APPLIED to the reference text, and P' is the smallest position within CAP (and >= 1, and with only
    A C G T between it and P) at which an event of the same type and length — for an insertion: the allele the text itself shows
    there — yields the IDENTICAL haplotype, compared as strings.
``restate(mutant=...)`` departs from the rule in one line; each departure is caught inside the family named beside it:
  ``n_minus_1``  the periodic comparison n - 1 apart            -> repeats
  ``no_acgt``    the A C G T test dropped                       -> codes
  ``p_zero``     P' = 0 allowed                                 -> contig_start
  ``hash_s``     the payload from S, not from the rotated S_k   -> ins_repeat
  ``cap_plus``   one more shift than CAP                        -> cap
"""
import collections

import numpy as np

import indel_cases as D

CAP = 1024
LENGTHS = (100000, 49999, 1000)
NAMES = ("c0", "c1", "c2")
NORM_SN = ("shifted_events", "shift_capped", "off_reference")
MUTANTS = {"n_minus_1": "repeats", "no_acgt": "codes", "p_zero": "contig_start", "hash_s": "ins_repeat", "cap_plus": "cap"}
SHIFTS = (15, 16, 17, 31, 32, 33, 63, 64, 65)
CAP_RUNS = (CAP, CAP + 1, CAP + 2, 3000)                       # a deletion of the last base shifts by the run's length - 1


# ------------------------------------------------------------------------------------------- the designed reference
def _plant(c, s, text, left=None, right=None):
    c[s:s + len(text)] = text.encode()
    if left:
        c[s - 1:s] = left.encode()
    if right:
        c[s + len(text):s + len(text) + 1] = right.encode()


def homopolymer_at(r):
    return 1000 + 100 * r                                       # run of r x A, C to its left, G to its right


def edge_run_at(i, residue, n):
    """the T run whose last n bases, deleted, shift by SHIFTS[i], the deletion's P on ``residue`` mod 16"""
    base = 10000 + ((i * 16 + residue) * 2 + (n - 1)) * 96       # (a multiple of 16; runs are at most 67 long)
    p = base + 80 + residue                                     # P = 80 + residue mod 16 ... the run ends at P + n
    return p + n - (SHIFTS[i] + n), p                           # (start of the run, P)


def cap_run_at(j):
    return 50000 + 4000 * j


def _design():
    rng = np.random.RandomState(20240607)
    c0, c1, c2 = (bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()) for n in LENGTHS)
    for r in range(1, 41):
        _plant(c0, homopolymer_at(r), "A" * r, "C", "G")
    _plant(c0, 6000, "CA" * 20, "T", "G")                       # [6000, 6040)
    _plant(c0, 6200, "CAG" * 15, "T", "T")                      # [6200, 6245)
    _plant(c0, 6400, "CA" * 10 + "CG", "T", "T")                # a CA run that a deletion can straddle: partial shifts
    for i in range(len(SHIFTS)):
        for residue in range(16):
            for n in (1, 2):
                s, p = edge_run_at(i, residue, n)
                _plant(c0, s, "T" * (p + n - s), "G", "C")
    for j, run in enumerate(CAP_RUNS):
        _plant(c0, cap_run_at(j), "G" * run, "A", "T")
    _plant(c0, 7000, "A" * 10 + "N" + "A" * 19, "C", "G")        # an N inside a run: [7000, 7030), the N at 7010
    _plant(c0, 7100, "A" * 10 + "R" + "A" * 19, "C", "G")        # an IUPAC code (R = A or G) at 7110
    _plant(c0, 7200, "a" * 20, "c", "g")                        # lower case
    _plant(c0, 7300, "N" * 30, "C", "G")                        # a run of N: nothing shifts across it
    _plant(c0, 8000, "ACGTTGCA" * 8, "G", "C")                  # a unit of 8: [8000, 8064)
    _plant(c0, 8200, "ACGTTGCAAGCTTCGATCGGATC" * 4, "T", "T")    # a unit of 23: [8200, 8292)
    _plant(c0, 8400, "ACGTTGCAAGCTTCGATCGGAT" * 4, "G", "G")     # a unit of 22: [8400, 8488)
    _plant(c0, 0, "C" + "A" * 12, None, "G")                    # the contig's start: a run from base 1
    _plant(c0, LENGTHS[0] - 40, "A" * 40, "C")                  # ... and its end
    _plant(c1, 0, "AC" + "A" * 30, None, "G")                   # a run from base 2 — and A at base 0, as behind c0's last base
    _plant(c1, 300, "CA" * 12, "G", "T")
    _plant(c1, LENGTHS[1] - 25, "T" * 25, "G")
    _plant(c2, 0, "T" * 20, None, "C")                          # T from base 0, as c1's last bases
    _plant(c2, 500, "G" * 9, "A", "C")
    _plant(c2, LENGTHS[2] - 12, "ACACACACACAC", "G")
    return bytes(c0), bytes(c1), bytes(c2)


TEXT = _design()
assert tuple(len(t) for t in TEXT) == LENGTHS


_CODE_OF = {b: (D.BASES.index(chr(b).upper()) if chr(b).upper() in D.BASES[1:] else 15) for b in range(256)}


def codes(text):
    """bases -> 4-bit codes: letters in either case to BAM's, anything else 15 — a plain strip-and-map, no table shared with the package"""
    return np.array([_CODE_OF[b] for b in bytes(text)], dtype=np.uint8)


CODES = tuple(codes(t) for t in TEXT)
HELD = tuple("".join(D.BASES[c] for c in cs.tolist()) for cs in CODES)       # the reference as the device holds it: upper case, strays as N


def fasta_bytes(contigs, linebases, eol=b"\n", final=True):
    """[(name, bases)] -> the file's bytes; final False: no line end behind the last line"""
    out = []
    for name, text in contigs:
        out.append(b">" + name.encode() + eol)
        out += [text[i:i + linebases] + eol for i in range(0, len(text), linebases)]
    data = b"".join(out)
    return data if final or not data.endswith(eol) else data[:-len(eol)]


def contig_raw(text, linebases, eol=b"\n", final=True):
    """one contig's bytes as FastaFile.fetch_raw returns them (no line end behind the last base) + what follows them in a file"""
    lines = [text[i:i + linebases] for i in range(0, len(text), linebases)]
    return eol.join(lines), (eol if final and lines else b"")


# ------------------------------------------------------------------------------------------- reads
def EVENTS(tid, events, flag=0, mapq=60, lead=None, seq_cut=None):
    """one read carrying ``events`` = [(P, n, inserted text or None)], ascending and apart, with M operations around and between them;
    lead: the bases matched in front of the first event (default 7 + an odd / even mix from P); seq_cut: the sequence is cut to that
    many bases (an insertion's span then lies outside it)"""
    first = events[0][0]
    lead = (7 if first >= 7 else first) if lead is None else lead
    pos = first - lead
    cigar, seq, r = [], [], pos
    for P, n, text in events:
        assert P > r
        cigar.append((0, P - r))
        seq.append(D.pattern(P - r))
        if text is None:
            cigar.append((2, n))
            r = P + n
        else:
            assert len(text) == n
            cigar.append((1, n))
            seq.append(text)
            r = P
    cigar.append((0, 9))
    seq.append(D.pattern(9))
    seq = "".join(seq)
    read = D.R(cigar, flag=flag, tid=tid, pos=pos, mapq=mapq, seq=seq if seq_cut is None else seq[:seq_cut])
    read["events"] = list(events)
    return read


def DEL(tid, P, n, **kw):
    return EVENTS(tid, [(P, n, None)], **kw)


def INS(tid, P, text, **kw):
    return EVENTS(tid, [(P, len(text), text)], **kw)


CASES = []


def case(name, family, reads, want=None, norm=None, loaded=(0, 1, 2), reader_ok=True, cuts=(), S=(1,), Q=20, lengths=LENGTHS):
    CASES.append({"name": name, "family": family, "reads": reads, "want": want, "norm": norm, "loaded": tuple(loaded), "reader_ok": reader_ok,
                  "cuts": tuple(cuts), "repeat": 1, "capacity": None, "Q": Q, "S": tuple(S), "lengths": tuple(lengths)})


# ---- deletions
for r in (1, 2, 3, 15, 16, 17, 31, 32, 33, 40):
    s = homopolymer_at(r)
    case("homopolymer of %d: a deletion of 1 at each of its positions" % r, "homopolymer", [DEL(0, s + j, 1) for j in range(r)],
         want=[(0, s)] * r, norm=(r - 1, 0, 0))
case("homopolymers of 1 ... 40: deletions of 1, 2 and 3 bases at every placement", "homopolymer",
     [DEL(0, homopolymer_at(r) + j, n) for r in range(1, 41) for n in (1, 2, 3) if n <= r for j in range(r - n + 1)],
     want=[(0, homopolymer_at(r)) for r in range(1, 41) for n in (1, 2, 3) if n <= r for j in range(r - n + 1)])
case("CA repeat: deletions of the unit and of twice the unit at every placement", "repeats",
     [DEL(0, 6000 + j, n) for n in (2, 4) for j in range(0, 40 - n + 1)], want=[(0, 6000)] * (39 + 37))
case("CA repeat: a deletion of 3 does not shift inside the run", "repeats", [DEL(0, 6000 + j, 3) for j in range(1, 30)],
     want=[(0, 6000 + j) for j in range(1, 30)], norm=(0, 0, 0))
case("CAG repeat: deletions of 3 and 6 at every placement; 2 and 4 stay", "repeats",
     [DEL(0, 6200 + j, n) for n in (3, 6) for j in range(0, 45 - n + 1)] + [DEL(0, 6200 + j, n) for n in (2, 4) for j in range(1, 30)],
     want=[(0, 6200)] * (43 + 40) + [(0, 6200 + j) for n in (2, 4) for j in range(1, 30)])
case("a deletion that straddles the end of a CA run: partial shifts", "repeats", [DEL(0, 6400 + j, n) for n in (1, 2, 3, 4, 5) for j in range(12, 22)])
case("a shift of 0: deletions in random sequence whose neighbours differ", "repeats",
     [DEL(0, p, 1) for p in range(90000, 90400) if TEXT[0][p - 1] != TEXT[0][p]][:64], norm=(0, 0, 0))
for i, k in enumerate(SHIFTS):
    reads, want = [], []
    for residue in range(16):
        for n in (1, 2):
            s, p = edge_run_at(i, residue, n)
            reads.append(DEL(0, p, n))
            want.append((0, s))
    case("a shift of exactly %d: P on every residue mod 16, n odd and even" % k, "word_edges", reads, want=want, norm=(32, 0, 0))
case("shifts that run into the contig's start: P' = 1 (c0, c2) and P' = 2 (c1)", "contig_start",
     [DEL(0, p, 1, lead=1) for p in range(1, 13)] + [DEL(0, 9, 3)] + [DEL(1, p, n) for p in (2, 5, 17, 30) for n in (1, 2)] + [DEL(2, 5, 1)],
     want=[(0, 1)] * 13 + [(1, 2)] * 8 + [(2, 1)], norm=(11 + 1 + 6 + 1, 0, 0))       # (c2 has T at base 0 too: P' stays 1)
case("an N and an IUPAC code inside a run stop the shift behind them; a run of N does not shift", "codes",
     [DEL(0, 7000 + j, 1) for j in (3, 9, 11, 12, 29)] + [DEL(0, 7100 + j, 1) for j in (3, 9, 11, 12, 29)] + [DEL(0, 7300 + j, n) for j in (1, 15, 28) for n in (1, 2)],
     want=[(0, 7000)] * 2 + [(0, 7011)] * 3 + [(0, 7100)] * 2 + [(0, 7111)] * 3 + [(0, 7300 + j) for j in (1, 15, 28) for n in (1, 2)],
     norm=(8, 0, 0))
case("a lower-case reference is the same reference", "codes", [DEL(0, 7200 + j, n) for j in range(0, 19) for n in (1, 2)], want=[(0, 7200)] * 38)
reads, want, capped = [], [], 0
for j, run in enumerate(CAP_RUNS):
    s = cap_run_at(j)
    for n in (1, 2):
        reads.append(DEL(0, s + run - n, n))
        k = min(run - n, CAP)
        want.append((0, s + run - n - k))
        capped += k == CAP
case("runs of CAP, CAP + 1, CAP + 2 and 3000: shifts of CAP - 1, CAP, and the cap", "cap", reads, want=want, norm=(8, capped, 0))
case("p + n one below, on and above the contig's length (c2, 1000 bases; c1)", "contig_end",
     [DEL(2, 1000 - n - d, n) for n in (1, 2, 7) for d in (1, 0, -1)] + [DEL(1, LENGTHS[1] - 3, 1), DEL(1, LENGTHS[1] - 1, 1), DEL(1, LENGTHS[1] - 1, 2)],
     norm=None, reader_ok=False)
case("a contig that is not loaded, and one outside the table: the keys stay", "unloaded",
     [DEL(1, 310, 2), DEL(0, 6010, 2), DEL(2, 504, 1), DEL(3, 504, 1), INS(1, 310, "CA")],
     want=[(1, 310), (0, 6000), (2, 500), (3, 504), (1, 310)], norm=(2, 0, 3), loaded=(0, 2), reader_ok=False, lengths=LENGTHS + (1000,))
case("events at the start of c1 and c2 do not see the neighbour through the guard", "guard",
     [DEL(1, p, 1) for p in (2, 3, 31)] + [DEL(2, p, n) for p in (1, 2, 3, 18) for n in (1, 2)] + [DEL(0, LENGTHS[0] - 1, 1), DEL(1, LENGTHS[1] - 2, 2)],
     want=[(1, 2)] * 3 + [(2, 1)] * 8 + [(0, LENGTHS[0] - 40), (1, LENGTHS[1] - 25)])

# ---- insertions
case("CA repeat: the unit inserted at every placement gives one key and one rotation", "ins_repeat",
     [INS(0, 6000 + j, "CA" if j % 2 == 0 else "AC") for j in range(0, 41)] + [INS(1, 300 + j, "CACA" if j % 2 == 0 else "ACAC") for j in range(0, 25)],
     want=[(0, 6000)] * 41 + [(1, 300)] * 25, norm=(40 + 24, 0, 0))
case("an insertion shifts by less than, exactly and more than its length", "ins_k",
     [INS(0, 8000 + 8 * 3 + j, ("ACGTTGCA" * 2)[j:j + 8]) for j in (0, 3, 7)] +        # k = 24 + j > n = 8
     [INS(0, 8000 + j, ("ACGTTGCA" * 2)[j:j + 8]) for j in (1, 5, 8)] +               # k = j <= n
     [INS(0, 8003, "TAGC"), INS(0, 8003, "TACG")],                                     # k = 0 (C != G) and k = 3 of 4 (S[0] != ref[7999])
     want=[(0, 8000)] * 6 + [(0, 8003), (0, 8000)], norm=(7, 0, 0))
case("insertions of 22 and 23 bases: packed and hashed alleles rotate alike", "ins_hash",
     [INS(0, 8400 + j, ("ACGTTGCAAGCTTCGATCGGAT" * 2)[j % 22:j % 22 + 22]) for j in (0, 1, 21, 22, 30, 66)] +
     [INS(0, 8200 + j, ("ACGTTGCAAGCTTCGATCGGATC" * 2)[j % 23:j % 23 + 23]) for j in (0, 1, 22, 23, 30, 69)],
     want=[(0, 8400)] * 6 + [(0, 8200)] * 6, norm=(10, 0, 0))
case("an inserted N stops the shift, and so does an N of the reference", "ins_n",
     [INS(0, homopolymer_at(20) + 9, "ANA"), INS(0, homopolymer_at(20) + 9, "NAA"), INS(0, 7012, "AA"), INS(0, 7011, "AA"), INS(0, 7020, "AAAAAAAAAAAA")],
     want=[(0, homopolymer_at(20) + 8), (0, homopolymer_at(20) + 7), (0, 7011), (0, 7011), (0, 7011)], norm=(4, 0, 0))
case("an insertion whose span is outside the sequence is never shifted", "ins_kind2",
     [INS(0, 6010, "CA", seq_cut=8), INS(0, 6010, "CA"), EVENTS(0, [(6010, 2, "CA"), (6220, 3, None)], seq_cut=5)],
     want=[(0, 6010), (0, 6000), (0, 6010), (0, 6200)], norm=(2, 0, 0), reader_ok=False)
case("an insertion whose query offset is on an odd and on an even nibble", "ins_oddq",
     [INS(0, 6020, "CACA", lead=k) for k in (1, 2, 3, 4, 5, 6, 15, 16, 17)], want=[(0, 6000)] * 9, norm=(9, 0, 0))

# ---- reads and sets
case("a read with four events that all shift", "four",
     [EVENTS(0, [(homopolymer_at(9) + 5, 2, None), (homopolymer_at(10) + 9, 1, "A"), (homopolymer_at(11) + 4, 3, None), (homopolymer_at(12) + 12, 2, "AA")]),
      EVENTS(0, [(6010, 2, None), (6030, 2, "CA"), (6230, 3, None), (6240, 3, "AGC")], flag=D.REV)],
     want=[(0, homopolymer_at(r)) for r in (9, 10, 11, 12)] + [(0, 6000), (0, 6000), (0, 6200), (0, 6200)], norm=(8, 0, 0))
case("a noisy read: none of its events counts, shifted or not", "noisy",
     [EVENTS(0, [(homopolymer_at(r) + r - 1, 1, None) for r in (5, 6, 7, 8, 9)]), DEL(0, homopolymer_at(30) + 29, 1)],
     want=[(0, homopolymer_at(30))], norm=(1, 0, 0))
case("one deletion and one insertion placed at three positions on both strands: one row each, SUPPORT 3", "sets",
     [DEL(0, homopolymer_at(25) + 3, 2), DEL(0, homopolymer_at(25) + 11, 2, flag=D.REV), DEL(0, homopolymer_at(25) + 23, 2, flag=D.REV),
      INS(0, 6004, "CA", flag=D.REV), INS(0, 6011, "AC"), INS(0, 6040, "CA")],
     want=[(0, homopolymer_at(25))] * 3 + [(0, 6000)] * 3, norm=(6, 0, 0), cuts=(2, 4), S=(1, 2, 3))
N_CASES = len(CASES)
FAMILIES = sorted({c["family"] for c in CASES})


# ------------------------------------------------------------------------------------------- the definition
def host_reference(loaded=(0, 1, 2)):
    from tiddit_amd import refseq
    return refseq.HostReference({t: CODES[t] for t in loaded})


def definition(case, ref="case"):
    """-> (keys in read order, {S: (counters, row columns)}, the three NORM counters); ref None: the keys of TIDDIT_INDELS alone"""
    from tiddit_amd import tiddit_indels
    if ref == "case":
        ref = host_reference(case["loaded"])
    keys, sn = [], {}
    for b in D.batches(case):
        tiddit_indels.keys_of_batch_by_read(b, keys, sn, case["Q"], ref)
    out = {}
    for S in case["S"]:
        c, rows = tiddit_indels.summarise(keys, sn, S)
        out[S] = (c, D.row_columns(rows))
    return keys, out, tuple(sn.get(k, 0) for k in NORM_SN)


# ------------------------------------------------------------------------------------------- the restatement
def _acgt(text):
    return set(text) <= set("ACGT")


def _payload_key(text, rev):
    return D.INS(text, rev) if len(text) <= 22 and _acgt(text) else D.INSH(text, rev)


def restate_event(tid, P, n, text, loaded, mutant=None):
    """-> (P', allele text or None, shifted, capped, off)"""
    if tid not in loaded or tid >= len(TEXT):
        return P, text, 0, 0, 1
    ref = HELD[tid]
    if (P > len(ref)) if text is not None else (P + n > len(ref)):
        return P, text, 0, 0, 1
    cap = CAP + 1 if mutant == "cap_plus" else CAP
    lo = max(P - cap - 2, 0)
    hi = min(P + n + 2, len(ref))
    w = ref[lo:hi]
    p = P - lo
    hap = w[:p] + w[p + n:] if text is None else w[:p] + text + w[p:]
    best, best_allele = P, text
    floor = 0 if mutant == "p_zero" else 1
    for cand in range(P - 1, max(P - cap, floor) - 1, -1):
        c = cand - lo
        between = w[c:p]
        if mutant != "no_acgt" and not _acgt(between):
            break
        if text is None:
            allele = None
            same_hap = between == w[c + n - 1:p + n - 1] if mutant == "n_minus_1" else w[:c] + w[c + n:] == hap
        else:
            allele = (between + text)[:n]
            same_hap = w[:c] + allele + w[c:] == hap
        if not same_hap:
            break
        best, best_allele = cand, allele
    k = P - best
    return best, (text if mutant == "hash_s" else best_allele), int(k > 0), int(k == cap), 0


def restate(case, mutant=None):
    """-> (keys in read order, {S: (counters, row columns)}, the three NORM counters) from the reads' ``events``"""
    keys, sn, norm = [], collections.Counter(), [0, 0, 0]
    for r in case["reads"]:
        sn["records"] += 1
        sn["eligible"] += 1
        ev = r["events"]
        if len(ev) > 4:
            sn["noisy_reads"] += 1
            continue
        sn["reads_with_events"] += 1
        rev = (r["flag"] >> 4) & 1
        q = 0
        at = r["pos"]
        for P, n, text in ev:
            q += P - at
            at = P + (n if text is None else 0)
            if text is None:
                sn["deletions"] += 1
                P2, _, a, b, c = restate_event(r["tid"], P, n, None, case["loaded"], mutant)
                keys.append((D.K1(r["tid"], P2), D.DEL(n, rev)))
            else:
                sn["insertions"] += 1
                if q + n > len(r["seq"]):                           # (SEQ *: untouched)
                    keys.append((D.K1(r["tid"], P), D.INSX(n, rev)))
                    q += n
                    continue
                q += n
                P2, allele, a, b, c = restate_event(r["tid"], P, n, text, case["loaded"], mutant)
                keys.append((D.K1(r["tid"], P2), _payload_key(allele, rev)))
            norm[0] += a
            norm[1] += b
            norm[2] += c
    out = {}
    for S in case["S"]:
        distinct, rows = D._sets_of(keys, S)
        out[S] = (D.counters_of(dict(sn), distinct, len(rows)), D.row_columns(rows))
    return keys, out, tuple(norm)


def same(a, b):
    """two (keys, by_support, norm) triples agree: the keys in read order, every counter and every row"""
    if a[0] != b[0] or a[2] != b[2] or set(a[1]) != set(b[1]):
        return False
    for S in a[1]:
        (ca, ra), (cb, rb) = a[1][S], b[1][S]
        if not np.array_equal(ca, cb) or not all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(ra, rb)):
            return False
    return True
