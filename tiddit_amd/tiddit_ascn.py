"""Allele-specific copy number and LOH segments from the ``--sv`` scan (``TIDDIT_ASCN=1``, with ``TIDDIT_CNV`` and ``TIDDIT_ALLELES``):
``{o}.ascn.bed`` — the CNV bins of tiddit_cnv.py joined with the B-allele fractions of tiddit_alleles.py's counter table.  Depth alone
cannot see a copy-neutral loss of heterozygosity, cannot tell 2+2 from 3+1 at four copies, and cannot tell a one-copy region from a
run of homozygosity; the sites can.  Everything is in the job once the ploidy stage ends — the bins ``x_t``, the ``[sites][8]`` table,
the ploidy table — so this is one more stage, with no second pass over the BAM.  The per-bin emissions and an exact 16-state Viterbi run
on the device (csrc/tdt_ascn.hip), every processed contig in one call each.  :func:`define_contig` is this text as plain Python.

Definition.  All values are integers; there is no tolerance.

  * CONSTANTS.  ``UNIT``, ``CAP``, ``LAMBDA`` are tiddit_cnv's.  ``BU = 512`` (the unit of an allele fraction), ``ACAP = BU*BU//4``,
    ``HOM = 4096``, ``MIN_N = 8`` — parameters of the definition, not measurements.
  * STATES.  ``S = 16`` states ``(c, m)``: total copies ``c = 0 ... 6``, minor copies ``0 <= m <= c // 2``, indexed with ``c`` ascending,
    then ``m`` ascending.  ``MU[k] = (BU*m)//c``, and 0 for ``c = 0``.
  * CONTIGS, ``W``, ``x_t``, ``P`` are exactly what ``TIDDIT_CNV`` processes and computes (tiddit_cnv.bins_stage).  The home state of a
    contig is ``(P, P // 2)``.
  * SITES.  The device sites of ``tiddit_alleles.Sites``: unique positions, contig-major, sorted.  REF and ALT of a site are those of its
    first accepted row in file order; ``ref_n`` and ``alt_n`` are the counter columns of those two bases.  With ``n = ref_n + alt_n`` the
    site is INFORMATIVE when ``n >= MIN_N``, and ``beta = (min(ref_n, alt_n) * BU) // n`` (64 bits).  The site lies in CNV bin
    ``pos0 // W`` of its contig.  Sites of contigs the CNV stage skipped count nowhere.
  * SITE SCORE.  ``h = min(ACAP, beta*beta)``.  For ``m = 0``: ``g(k) = h``.  Otherwise
    ``g(k) = min(min(ACAP, (beta - MU[k])**2), h + HOM)``: the site is either het at the state's expected fraction, or homozygous at a
    price.
  * EMISSION.  ``E_t(k) = d_t(c_k)`` plus the sum of ``g_s(k)`` over the informative sites of the bin; ``d`` is tiddit_cnv's ``e_t``
    (``min(CAP, (x_t - UNIT*c)**2)``), and 0 for ``x_t < 0``.  With ``W <= 3200`` this is below 2^28.  A bin is EMPTY when ``x_t < 0``
    and it has no informative site.
  * VITERBI.  tiddit_cnv's recurrence word for word, over 16 states with ``E_t(k)`` as the emission:
    ``V_0(k) = E_0(k) + (0 if k == home else LAMBDA)``; for ``t >= 1``, with ``m = min_i V_{t-1}(i)`` and ``a`` the lowest ``i`` attaining
    it, ``V_t(k) = E_t(k) + min(V_{t-1}(k), m + LAMBDA)`` and ``B_t(k) = k`` if ``V_{t-1}(k) <= m + LAMBDA``, else ``a``.  The end cost is
    ``V_{T-1}(k) + (0 if k == home else LAMBDA)``; ``s_{T-1}`` is the lowest ``k`` attaining its minimum, ``s_{t-1} = B_t(s_t)``.
  * SEGMENTS.  The maximal runs of equal state other than home; EMPTY bins are trimmed off both ends of a run and a run of only EMPTY
    bins is dropped.  One line per segment, contigs in header order: ``chrom``, ``start = first*W``,
    ``end = min((last+1)*W, contig length)``, ``type`` (``DEL`` if ``c < P``, ``DUP`` if ``c > P``, ``LOH`` if ``c == P`` and ``m == 0``,
    else ``AI``), ``CN = c``, ``minorCN = m``, ``bins`` (the run's bins with ``x_t >= 0``),  ``sites`` (the informative sites of the
    trimmed run), ``meanCN = "{:.3f}".format(sum_x / (bins*UNIT))`` or ``.`` without bins, and
    ``meanBAF = "{:.3f}".format(sum_beta / (sites*BU))`` or ``.`` without sites, both from Python integers.  The first line is
    ``#chrom\\tstart\\tend\\ttype\\tCN\\tminorCN\\tbins\\tsites\\tmeanCN\\tmeanBAF``; the file is written even when it has no segment.
    Skipped contigs are named once in a note.

What it takes to be called.  A het site at the home fraction costs a state with ``m = 0`` about ``ACAP``; a homozygous site costs a
state with ``m > 0`` ``HOM`` — and tells nothing apart from a run of homozygosity in a normal region, which is why it is cheap.  A
copy-neutral LOH shows only as the ABSENCE of het sites, so about ``2*LAMBDA/HOM = 64`` homozygous sites pay for its two jumps: on a
prototype of this definition (3000 bins of 500 bp, one site per kb, 30 % het, 15x per copy) an LOH of 400 bins was called within ten
bins of its ends, (1,0), (3,1), (4,1), (4,2) and (3,0) plants of 20 to 400 bins exactly, and an LOH of 60 bins with 30 sites was NOT
reported — by construction.

On N ranks rank 0 holds the reduced bins and the summed counter table, and runs this stage alone."""
import numpy

from . import _native
from .tiddit_cnv import CAP, LAMBDA, UNIT

BU = 512
ACAP = BU * BU // 4
HOM = 4096
MIN_N = 8
STATES = tuple((c, m) for c in range(7) for m in range(c // 2 + 1))
S = len(STATES)
MU = tuple(0 if c == 0 else (BU * m) // c for c, m in STATES)
HEADER = "#chrom\tstart\tend\ttype\tCN\tminorCN\tbins\tsites\tmeanCN\tmeanBAF\n"
STAGE_SECONDS = {}
_COLUMN = {"A": 0, "C": 1, "G": 2, "T": 3}


def parse_switch(value, cnv, alleles):
    """``TIDDIT_ASCN``: unset or empty -> False, ``1`` -> True when both partner switches are set (``cnv`` / ``alleles``: what their
    parsers returned); ValueError (its text is the error line) for anything else."""
    if value is None or value == "":
        return False
    if value != "1":
        raise ValueError("the switch is 1")
    missing = [n for n, v in (("TIDDIT_CNV", cnv), ("TIDDIT_ALLELES", alleles)) if v is None]
    if missing:
        raise ValueError("the stage joins the bins of TIDDIT_CNV with the counters of TIDDIT_ALLELES: {} not set".format(
            " and ".join(missing) + (" is" if len(missing) == 1 else " are")))
    return True


def home_of(P):
    return STATES.index((int(P), int(P) // 2))


def kind_of(c, m, P):
    return "DEL" if c < P else "DUP" if c > P else "LOH" if m == 0 else "AI"


def site_columns(sites):
    """uint8[device sites][2]: the counter columns of REF and ALT of every device site — those of its first accepted row"""
    rows = sites.rows
    cols = numpy.zeros((len(sites), 2), dtype=numpy.uint8)
    if not rows:
        return cols
    lut = numpy.zeros(256, dtype=numpy.uint8)
    lut[[ord(b) for b in "ACGT"]] = [_COLUMN[b] for b in "ACGT"]
    letters = numpy.frombuffer("".join([r[2] + r[3] for r in rows]).encode(), dtype=numpy.uint8).reshape(-1, 2)
    site, first = numpy.unique(numpy.fromiter((r[4] for r in rows), dtype=numpy.int64, count=len(rows)), return_index=True)
    cols[site] = lut[letters[first]]
    return cols


# ------------------------------------------------------------------------------------------- the definition
def site_score(ref_n, alt_n):
    """-> None for a site that is not informative, else (beta, [g(k) for the 16 states])"""
    n = int(ref_n) + int(alt_n)
    if n < MIN_N:
        return None
    beta = (min(int(ref_n), int(alt_n)) * BU) // n
    h = min(ACAP, beta * beta)
    return beta, [h if m == 0 else min(min(ACAP, (beta - MU[k]) ** 2), h + HOM) for k, (c, m) in enumerate(STATES)]


def define_contig(x, P, W, length, chrom, pos, ref_n, alt_n):
    """THE DEFINITION, one contig: its CNV bins ``x``, ploidy ``P``, and its sites (0-based positions, sorted, with their two counters)
    -> (E [T][16], nsite [T], sum_beta [T], states [T], segments)"""
    T = len(x)
    E = [[0 if int(x[t]) < 0 else min(CAP, (int(x[t]) - UNIT * c) ** 2) for c, m in STATES] for t in range(T)]
    nsite, sum_beta = [0] * T, [0] * T
    for p, r, a in zip(pos, ref_n, alt_n):
        t = int(p) // W
        sc = site_score(r, a)
        if sc is None or t >= T:
            continue
        nsite[t] += 1
        sum_beta[t] += sc[0]
        for k in range(S):
            E[t][k] += sc[1][k]
    if T == 0:
        return E, nsite, sum_beta, [], []
    home = home_of(P)
    V = [E[0][k] + (0 if k == home else LAMBDA) for k in range(S)]
    B = [None]
    for t in range(1, T):
        m = min(V)
        a = V.index(m)
        B.append([k if V[k] <= m + LAMBDA else a for k in range(S)])
        V = [E[t][k] + min(V[k], m + LAMBDA) for k in range(S)]
    end = [V[k] + (0 if k == home else LAMBDA) for k in range(S)]
    s = [0] * T
    s[T - 1] = end.index(min(end))
    for t in range(T - 1, 0, -1):
        s[t - 1] = B[t][s[t]]
    segments = []
    t = 0
    while t < T:
        e = t
        while e + 1 < T and s[e + 1] == s[t]:
            e += 1
        if s[t] != home:
            first, last = t, e
            while first <= last and int(x[first]) < 0 and nsite[first] == 0:
                first += 1
            while last >= first and int(x[last]) < 0 and nsite[last] == 0:
                last -= 1
            if first <= last:
                c, m = STATES[s[t]]
                seen = [int(x[i]) for i in range(first, last + 1) if int(x[i]) >= 0]
                ns, sb = sum(nsite[first:last + 1]), sum(sum_beta[first:last + 1])
                segments.append((chrom, first * W, min((last + 1) * W, int(length)), kind_of(c, m, P), c, m, len(seen), ns,
                                 "{:.3f}".format(sum(seen) / (len(seen) * UNIT)) if seen else ".",
                                 "{:.3f}".format(sb / (ns * BU)) if ns else "."))
        t = e + 1
    return E, nsite, sum_beta, s, segments


def text_of(segments):
    return HEADER + "".join("\t".join(map(str, s)) + "\n" for s in segments)


# ------------------------------------------------------------------------------------------- the two entries over host arrays
def site_table(rows):
    """rows: (site_lo, site_hi, T, W) per contig -> int64[len(rows)][5], tdt_ascn_emissions' table with toff filled in"""
    t = numpy.zeros((len(rows), 5), dtype=numpy.int64)
    at = 0
    for i, (lo, hi, T, W) in enumerate(rows):
        t[i] = (lo, hi, at, T, W)
        at += int(T)
    return t


def emissions(counts, site_pos, cols, x, table, ctx=None):
    """tdt_ascn_emissions over host arrays -> (int32 E[total][16], int32 nsite, int32 sum_beta)"""
    ctx = ctx or _native.default_context()
    counts = numpy.ascontiguousarray(counts, dtype=numpy.uint32).reshape(-1, 8)
    site_pos = numpy.ascontiguousarray(site_pos, dtype=numpy.int32)
    cols = numpy.ascontiguousarray(cols, dtype=numpy.uint8).reshape(-1, 2)
    x = numpy.ascontiguousarray(x, dtype=numpy.int32)
    table = numpy.ascontiguousarray(table, dtype=numpy.int64).reshape(-1, 5)
    E = numpy.zeros((len(x), S), dtype=numpy.int32)
    nsite, sum_beta = numpy.zeros(len(x), dtype=numpy.int32), numpy.zeros(len(x), dtype=numpy.int32)
    _native.check(ctx.lib.tdt_ascn_emissions(ctx.handle, _native.ptr(counts), _native.ptr(site_pos), _native.ptr(cols), len(site_pos), _native.ptr(x),
                                             len(x), _native.ptr(table), len(table), UNIT, CAP, BU, ACAP, HOM, MIN_N, _native.ptr(E),
                                             _native.ptr(nsite), _native.ptr(sum_beta)))
    return E, nsite, sum_beta


def viterbi(E, table, lam=LAMBDA, ctx=None):
    """tdt_hmm16_viterbi over host arrays; table: int64[nseg][3] {toff, T, home} -> int8 state"""
    ctx = ctx or _native.default_context()
    E = numpy.ascontiguousarray(E, dtype=numpy.int32).reshape(-1, S)
    table = numpy.ascontiguousarray(table, dtype=numpy.int64).reshape(-1, 3)
    state = numpy.zeros(len(E), dtype=numpy.int8)
    _native.check(ctx.lib.tdt_hmm16_viterbi(ctx.handle, _native.ptr(E), len(E), _native.ptr(table), len(table), lam, _native.ptr(state)))
    return state


# ------------------------------------------------------------------------------------------- segments and the file
def segments_of(state, x, nsite, sum_beta, chains, ploidy, W, lengths, names):
    """the segments of every contig from the concatenated states, CNV bins and per-bin site sums; chains: int64[nseg][3]
    {toff, T, home}.  numpy over the run edges: the only Python loop is over the segments that are written."""
    state, x = numpy.asarray(state), numpy.asarray(x)
    n = len(state)
    if n == 0:
        return []
    chains = numpy.asarray(chains, dtype=numpy.int64).reshape(-1, 3)
    contig = numpy.repeat(numpy.arange(len(chains)), chains[:, 1])
    cut = numpy.flatnonzero((state[1:] != state[:-1]) | (contig[1:] != contig[:-1])) + 1
    lo, hi = numpy.concatenate([[0], cut]), numpy.concatenate([cut, [n]])
    full = numpy.flatnonzero((x >= 0) | (numpy.asarray(nsite) > 0))                  # the bins that are not EMPTY
    i0, i1 = numpy.searchsorted(full, lo), numpy.searchsorted(full, hi)
    keep = numpy.flatnonzero((state[lo] != chains[contig[lo], 2]) & (i1 > i0))
    if not len(keep):
        return []
    first, last = full[i0[keep]], full[i1[keep] - 1]

    def between(v):
        c = numpy.concatenate([[0], numpy.cumsum(numpy.asarray(v, dtype=numpy.int64))])
        return (c[last + 1] - c[first]).tolist()
    bins, sum_x = between(x >= 0), between(numpy.where(x >= 0, x, 0))
    sites, sum_b = between(nsite), between(sum_beta)
    out = []
    for i, (r, f, l) in enumerate(zip(keep.tolist(), first.tolist(), last.tolist())):
        s = int(contig[lo[r]])
        toff, P = int(chains[s, 0]), ploidy[s]
        c, m = STATES[int(state[lo[r]])]
        out.append((names[s], (f - toff) * W, min((l - toff + 1) * W, int(lengths[s])), kind_of(c, m, P), c, m, bins[i], sites[i],
                    "{:.3f}".format(sum_x[i] / (bins[i] * UNIT)) if bins[i] else ".",
                    "{:.3f}".format(sum_b[i] / (sites[i] * BU)) if sites[i] else "."))
    return out


def write_bed(path, segments):
    with open(path, "w") as f:
        f.write(text_of(segments))


def main(bins, table, sites, contig_number, contig_length, prefix, ctx=None):
    """the stage behind ``TIDDIT_CNV``: ``{prefix}.ascn.bed`` from the CNV bins that stage left on the device (``bins``:
    tiddit_cnv.bins_stage's result), the counter table tiddit_alleles.main returned and the sites it counted at -> the segments"""
    import time
    import torch
    STAGE_SECONDS.clear()
    ctx = ctx or _native.default_context()
    if bins.skipped:
        order = {c: i for i, c in enumerate(bins.contigs)}
        print("note: TIDDIT_ASCN skips {}".format(", ".join(sorted(bins.skipped, key=order.get))))
    segments = []
    if bins.used:
        t0 = time.time()
        W = bins.W
        rows = [(int(sites.site_off[contig_number[c]]), int(sites.site_off[contig_number[c] + 1]), int(T), W)
                for c, T in zip(bins.used, bins.chains[:, 1])]
        stab = site_table(rows)
        chains = bins.chains.copy()
        chains[:, 2] = [home_of(P) for P in bins.ploidy]
        total = int(chains[:, 1].sum())
        dev = torch.device("cuda", ctx.device)
        # (counters above 2^32 - 1 are outside tiddit_alleles' contract; the N-rank sum arrives as int64)
        d_counts = torch.from_numpy(numpy.ascontiguousarray(numpy.asarray(table).reshape(-1, 8).astype(numpy.uint32)).view(numpy.int32)).to(dev)
        d_pos = torch.from_numpy(numpy.ascontiguousarray(sites.site_pos, dtype=numpy.int32)).to(dev)
        d_cols = torch.from_numpy(site_columns(sites)).to(dev)
        d_E = torch.empty((total, S), dtype=torch.int32, device=dev)
        d_sums = torch.empty((2, total), dtype=torch.int32, device=dev)               # nsite, sum_beta
        d_state = torch.empty(total, dtype=torch.int8, device=dev)
        torch.cuda.synchronize(dev)                   # torch's copies run on its stream, the library on its own
        STAGE_SECONDS["ASCN upload of the counter table"] = time.time() - t0
        t0 = time.time()
        _native.check(ctx.lib.tdt_ascn_emissions_device(ctx.handle, d_counts.data_ptr(), d_pos.data_ptr(), d_cols.data_ptr(), len(sites),
                                                        bins.d_x.data_ptr(), total, _native.ptr(stab), len(stab), UNIT, CAP, BU, ACAP, HOM, MIN_N,
                                                        d_E.data_ptr(), d_sums[0].data_ptr(), d_sums[1].data_ptr()))
        STAGE_SECONDS["ASCN emissions (device, tdt_ascn_emissions)"] = time.time() - t0
        t0 = time.time()
        _native.check(ctx.lib.tdt_hmm16_viterbi_device(ctx.handle, d_E.data_ptr(), total, _native.ptr(chains), len(chains), LAMBDA,
                                                       d_state.data_ptr()))
        STAGE_SECONDS["ASCN segmentation (device, tdt_hmm16_viterbi: five kernels)"] = time.time() - t0
        t0 = time.time()
        sums = d_sums.cpu().numpy()
        segments = segments_of(d_state.cpu().numpy(), bins.d_x.cpu().numpy(), sums[0], sums[1], chains, bins.ploidy, W,
                               [contig_length[c] for c in bins.used], bins.used)
        STAGE_SECONDS["ASCN segments (host)"] = time.time() - t0
    t0 = time.time()
    write_bed(prefix + ".ascn.bed", segments)
    STAGE_SECONDS["ASCN text (host)"] = time.time() - t0
    return segments
