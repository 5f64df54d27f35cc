"""Adversarial inputs and plain references for the device pieces of the native variant stage (TIDDIT_VARIANTS=1): the evidence store
(csrc/tdt_region.hip: evidence_pack, ev_reserve), the region counts over columns and over the store (region_counts,
region_counts_packed with their 64-ary lower bound) and the segment means (csrc/tdt_means.hip: seg_means).

Everything here is deterministic (numpy.random.default_rng with fixed seeds) and written from the rules of tiddit_variant.pyx:54-151 in
plain Python and numpy; the references share no code with tiddit_amd.  They are pinned on the CPU by test_variant_stage_refs_cpu.py
(loop == numpy == the C oracle, and the predicate-edge cases tell every one-comparison mutant of the loop apart) and compared with the
kernels by test_gpu_variant_stages.py.  Test infrastructure only.

A column set is a dict of the nine decoded columns (COLS) over several contigs, coordinate sorted per contig, contigs in ascending
order, an unplaced tail (tid -1) last.  A counts case is one column set plus a list of (contig, start, end, bp) queries."""
import itertools

import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
MIN_Q, MAX_INS = 20, 600
COLS = ("tid", "pos", "end", "mapq", "flag", "mate_tid", "mate_pos", "tlen", "sa_off")
_DT = dict(tid=np.int32, pos=np.int32, end=np.int32, mapq=np.uint8, flag=np.uint16, mate_tid=np.int32, mate_pos=np.int32, tlen=np.int32,
           sa_off=np.int64)
TABLE_KEYS = ("start", "end", "mapq", "flag", "mate_tid", "mate_pos", "tlen", "has_sa")
# the packed record of the evidence store and its bits, restated from include/tiddit_hip.h (the CPU test holds them to tiddit_region's)
EV_RECORD = np.dtype([("start", "<i4"), ("end", "<i4"), ("mate_pos", "<i4"), ("bits", "u1"), ("pad", "u1", (3,))])
EV_DUPLICATE, EV_HAS_SA, EV_UNMAPPED, EV_MATE_UNMAPPED, EV_LOW_Q, EV_DISCORDANT = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20


def make_cols(**kw):
    return {k: np.ascontiguousarray(np.asarray(kw[k], dtype=np.int64).astype(_DT[k])) for k in COLS}


def concat_cols(parts):
    return {k: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, _DT[k]) for k in COLS}


def slice_cols(cols, lo, hi):
    return {k: cols[k][lo:hi] for k in COLS}


def contig_table(cols, tid):
    """one contig's records as the eight arrays the per-contig entries and the C oracle take"""
    m = cols["tid"] == tid
    t = {"start": cols["pos"][m], "end": cols["end"][m], "mapq": cols["mapq"][m], "flag": cols["flag"][m], "mate_tid": cols["mate_tid"][m],
         "mate_pos": cols["mate_pos"][m], "tlen": cols["tlen"][m], "has_sa": (cols["sa_off"][m] >= 0).astype(np.uint8)}
    return {k: np.ascontiguousarray(v) for k, v in t.items()}


def _table(cols, tid):
    return cols if "start" in cols else contig_table(cols, tid)


# ===================================================================================================== get_region: references
# The comparisons of the chain, in order; `trace` (a dict) collects for each the operand differences lhs - rhs (clamped to +-2) met
# while the read was still live there, so a test can demand that a case set touches -1, 0 and +1 on every one of them.
COMPARISONS = ("clamp", "fallback", "fetch_pos", "fetch_end", "mate_skip_mpos", "mate_skip_rs", "unmapped_mate_skip_rs", "counted_rs",
               "lowq", "cross_r_rs", "cross_r_re", "cross_f_mpos", "cross_f_re", "tlen", "re_lt_start", "final_rs", "r_start_clip",
               "r_end_clip")

# One mutant per comparison of the chain: the loop below with exactly that comparison changed.  They exist only so that the CPU test can
# prove that the predicate-edge queries tell each of them from the loop.  (tiddit_variant.pyx has four `rs > end` tests — :92, :95, :101,
# :127 — and each has its mutant.)
MUTANTS = ("fetch_pos_le",               # fetch: pos < q_end -> <=
           "fetch_end_ge",               # fetch: end > q_start -> >=
           "clamp_dropped",              # :71-72 q_end > contig_length clamp dropped
           "fallback_gt",                # :74 q_start >= q_end -> >
           "fallback_minus9",            # :75 q_end - 10 -> q_end - 9
           "mate_skip_mpos_ge",          # :92 mpos > end -> >=
           "mate_skip_rs_ge",            # :92 rs > end -> >=
           "unmapped_mate_skip_rs_ge",   # :95 rs > end -> >=
           "counted_rs_ge",              # :101 rs > end -> >=
           "lowq_count_le",              # :103 mapq < min_q -> <=
           "lowq_skip_le",               # :106 mapq < min_q -> <=
           "cross_r_rs_le",              # :116 rs < bp-20 -> <=
           "cross_r_re_ge",              # :116 re > bp+20 -> >=
           "cross_f_mpos_le",            # :119 mpos < bp-50 -> <=
           "cross_f_re_ge",              # :119 re > bp+50 -> >=
           "tlen_ge",                    # :120 abs(tlen) > max_ins -> >=
           "abs_wrapped_int32",          # :120 abs taken in wrapped int32 (abs(INT32_MIN) == INT32_MIN)
           "mate_tid_ignored",           # :120 mate_tid != tid ignored
           "re_lt_start_le",             # :125 re < start -> <=
           "final_rs_ge",                # :127 rs > end -> >=
           "r_start_clip_dropped",       # :130-131
           "r_end_clip_dropped",         # :133-134
           "bases_plus1_dropped",        # :136
           "ignore_0x4",                 # :86
           "ignore_0x8",                 # :91 (every read takes the mate-mapped branch)
           "ignore_0x400",               # :98
           "splits_before_skip",         # :138 counted before :125-128
           "discs_before_skip")          # :141 counted before :125-128


def get_region_loop(cols, tid, contig_length, start, end, bp, min_q, max_ins, mutant=None, trace=None):
    """tiddit_variant.pyx:54-151 read by read over ALL records of the contig, in Python integers (nothing can overflow): the region
    fetch is `pos < q_end and end > q_start`, no search, no max-span shortcut.
    -> int64[7]: bases, n_reads, low_q, n_discs, n_splits, crossing_f, crossing_r."""
    t = _table(cols, tid)
    S, E, MQ, FL, MT, MP, TL, SA = (t[k].tolist() for k in TABLE_KEYS)
    m = mutant
    if m is not None and m not in MUTANTS:
        raise KeyError(m)

    def T(name, d):
        if trace is not None:
            trace.setdefault(name, set()).add(max(-2, min(2, d)))
    start, end, bp, L, max_ins = int(start), int(end), int(bp), int(contig_length), int(max_ins)
    low_q = n_reads = bases = n_discs = n_splits = crossing_r = crossing_f = 0
    q_start, q_end = start, end + max_ins                                                   # :68-69
    T("clamp", q_end - L)
    if m != "clamp_dropped" and q_end > L:                                                  # :71
        q_end = L
    T("fallback", q_start - q_end)
    if (q_start > q_end) if m == "fallback_gt" else (q_start >= q_end):                     # :74
        q_start = q_end - (9 if m == "fallback_minus9" else 10)
    for i in range(len(S)):
        rs, re, mpos, f = S[i], E[i], MP[i], FL[i]
        T("fetch_pos", rs - q_end)
        if not (rs <= q_end if m == "fetch_pos_le" else rs < q_end):                        # :85 fetch
            continue
        T("fetch_end", re - q_start)
        if not (re >= q_start if m == "fetch_end_ge" else re > q_start):
            continue
        if f & 0x4 and m != "ignore_0x4":                                                   # :86
            continue
        if not (f & 0x8) or m == "ignore_0x8":                                              # :91
            T("mate_skip_mpos", mpos - end)
            if mpos >= end if m == "mate_skip_mpos_ge" else mpos > end:                     # :92
                T("mate_skip_rs", rs - end)
                if rs >= end if m == "mate_skip_rs_ge" else rs > end:
                    continue
        else:
            T("unmapped_mate_skip_rs", rs - end)
            if rs >= end if m == "unmapped_mate_skip_rs_ge" else rs > end:                  # :95
                continue
        if f & 0x400 and m != "ignore_0x400":                                               # :98
            continue
        T("counted_rs", rs - end)
        if not (rs >= end if m == "counted_rs_ge" else rs > end):                           # :101
            n_reads += 1
            if MQ[i] <= min_q if m == "lowq_count_le" else MQ[i] < min_q:                   # :103
                low_q += 1
        T("lowq", MQ[i] - min_q)
        if MQ[i] <= min_q if m == "lowq_skip_le" else MQ[i] < min_q:                        # :106
            continue
        r_start, r_end = rs, re                                                             # :113-114
        T("cross_r_rs", rs - (bp - 20))
        if rs <= bp - 20 if m == "cross_r_rs_le" else rs < bp - 20:                         # :116
            T("cross_r_re", re - (bp + 20))
            if re >= bp + 20 if m == "cross_r_re_ge" else re > bp + 20:
                crossing_r += 1
        mate_bp_read = False                                                                # :119
        T("cross_f_mpos", mpos - (bp - 50))
        if mpos <= bp - 50 if m == "cross_f_mpos_le" else mpos < bp - 50:
            T("cross_f_re", re - (bp + 50))
            mate_bp_read = re >= bp + 50 if m == "cross_f_re_ge" else re > bp + 50
        isz = abs(TL[i])
        if m == "abs_wrapped_int32":
            isz = (isz + (1 << 31)) % (1 << 32) - (1 << 31)
        T("tlen", isz - max_ins)
        discordant = (isz >= max_ins if m == "tlen_ge" else isz > max_ins) or (MT[i] != tid and m != "mate_tid_ignored")   # :120
        if mate_bp_read and not discordant:                                                 # :122
            crossing_f += 1
        if m == "splits_before_skip" and SA[i]:
            n_splits += 1
        if m == "discs_before_skip" and discordant:
            n_discs += 1
        T("re_lt_start", re - start)
        if re <= start if m == "re_lt_start_le" else re < start:                            # :125
            continue
        T("final_rs", rs - end)
        if rs >= end if m == "final_rs_ge" else rs > end:                                   # :127
            continue
        T("r_start_clip", rs - start)
        if rs < start and m != "r_start_clip_dropped":                                      # :130
            r_start = start
        T("r_end_clip", re - end)
        if re > end and m != "r_end_clip_dropped":                                          # :133
            r_end = end
        bases += r_end - r_start + (0 if m == "bases_plus1_dropped" else 1)                 # :136
        if SA[i] and m != "splits_before_skip":                                             # :138
            n_splits += 1
        if discordant and m != "discs_before_skip":                                         # :141
            n_discs += 1
    return np.array([bases, n_reads, low_q, n_discs, n_splits, crossing_f, crossing_r], dtype=np.int64)


def get_region_numpy(cols, tid, contig_length, start, end, bp, min_q, max_ins):
    """the same rules over the whole contig at once, in int64 (for the large cases)"""
    t = _table(cols, tid)
    start, end, bp, L, max_ins = int(start), int(end), int(bp), int(contig_length), int(max_ins)
    q_start, q_end = start, end + max_ins
    if q_end > L:
        q_end = L
    if q_start >= q_end:
        q_start = q_end - 10
    S, E = t["start"].astype(np.int64), t["end"].astype(np.int64)
    sel = np.flatnonzero((S < q_end) & (E > q_start))                                        # the fetch
    rs, re = S[sel], E[sel]
    f = t["flag"][sel].astype(np.int64)
    mpos = t["mate_pos"][sel].astype(np.int64)
    mapq = t["mapq"][sel].astype(np.int64)
    live = (f & 0x4) == 0
    live &= ~np.where((f & 0x8) != 0, rs > end, (mpos > end) & (rs > end))
    live &= (f & 0x400) == 0
    counted = live & ~(rs > end)
    lowq = mapq < min_q
    n_reads, low_q = int(counted.sum()), int((counted & lowq).sum())
    live &= ~lowq
    crossing_r = int((live & (rs < bp - 20) & (re > bp + 20)).sum())
    disc = (np.abs(t["tlen"][sel].astype(np.int64)) > max_ins) | (t["mate_tid"][sel].astype(np.int64) != tid)
    crossing_f = int((live & (mpos < bp - 50) & (re > bp + 50) & ~disc).sum())
    live &= ~(re < start) & ~(rs > end)
    bases = int((np.minimum(re, end) - np.maximum(rs, start) + 1)[live].sum())
    return np.array([bases, n_reads, low_q, int((live & disc).sum()), int((live & (t["has_sa"][sel] != 0)).sum()), crossing_f, crossing_r],
                    dtype=np.int64)


def pack_reference(cols, min_q, max_ins, n_contigs=None):
    """what the evidence store holds for these columns -> (records of the placed reads in order, as EV_RECORD; int64 max(end - start)
    per contig, 0 for a contig without reads)"""
    tid = cols["tid"].astype(np.int64)
    p = tid >= 0
    f = cols["flag"][p].astype(np.int64)
    bits = np.where(f & 0x4, EV_UNMAPPED, 0) | np.where(f & 0x8, EV_MATE_UNMAPPED, 0) | np.where(f & 0x400, EV_DUPLICATE, 0)
    bits |= np.where(cols["sa_off"][p] >= 0, EV_HAS_SA, 0)
    bits |= np.where(cols["mapq"][p].astype(np.int64) < min_q, EV_LOW_Q, 0)
    bits |= np.where((np.abs(cols["tlen"][p].astype(np.int64)) > max_ins) | (cols["mate_tid"][p].astype(np.int64) != tid[p]), EV_DISCORDANT, 0)
    rec = np.zeros(int(p.sum()), dtype=EV_RECORD)
    rec["start"], rec["end"], rec["mate_pos"], rec["bits"] = cols["pos"][p], cols["end"][p], cols["mate_pos"][p], bits
    nc = int(tid.max()) + 1 if n_contigs is None else n_contigs
    spans = np.zeros(max(nc, 0), dtype=np.int64)
    if len(rec):
        np.maximum.at(spans, tid[p], cols["end"][p].astype(np.int64) - cols["pos"][p].astype(np.int64))
    return rec, spans


# ===================================================================================================== column sets
class _Reads:
    """collects reads one by one; cols() sorts them by (contig, start), stably, the unplaced ones last"""

    def __init__(self):
        self.rows = []

    def add(self, tid, L, rs, re, mpos=None, flag=0x1, mapq=60, mtid=None, tlen=300, sa=False):
        """a read if it is a legal one (0 <= rs < L, rs <= re <= L, mate_pos >= -1): edge generators may ask for one off the contig"""
        if rs < 0 or rs >= L or re < rs or re > L:
            return False
        if mpos is None:
            mpos = min(rs + 150, L - 1)
        if mpos < -1 or mpos > I32_MAX:
            return False
        self.rows.append((tid, rs, re, mapq, flag, tid if mtid is None else mtid, mpos, tlen, 77 if sa else -1))
        return True

    def cols(self):
        r = np.array(self.rows, dtype=np.int64).reshape(-1, 9)
        key = np.where(r[:, 0] < 0, 1 << 40, r[:, 0])
        o = np.lexsort((r[:, 1], key))
        return make_cols(**{k: r[o, j] for j, k in enumerate(COLS)})


def _random_contig(rng, tid, starts, L, n_contigs=3, span=100):
    """a contig of random reads on the given sorted starts: lengths 30..span with the first read exactly span long"""
    n = len(starts)
    starts = np.asarray(starts, dtype=np.int64)
    ln = rng.integers(30, span + 1, n)
    if n:
        ln[0] = span
    end = np.minimum(starts + ln, L)
    flag = rng.choice([0x1, 0x3, 0x11, 0x401, 0x9, 0x5, 0x801], n, p=[.4, .3, .1, .05, .05, .05, .05])
    mtid = np.where(rng.random(n) < 0.05, (tid + 1) % n_contigs, tid)
    mpos = np.clip(starts + rng.integers(-2000, 2000, n), 0, L - 1)
    return make_cols(tid=np.full(n, tid), pos=starts, end=end, mapq=rng.integers(0, 61, n), flag=flag, mate_tid=mtid, mate_pos=mpos,
                     tlen=rng.integers(-3 * MAX_INS, 3 * MAX_INS, n), sa_off=np.where(rng.random(n) < 0.03, 100, -1))


def _case(name, family, lengths, cols, queries, large=False, **extra):
    q = np.array(queries, dtype=np.int64).reshape(-1, 4)
    assert q[:, 1:].min(initial=0) >= 0 and q[:, 1:].max(initial=0) <= I32_MAX and (q[:, 2] >= q[:, 1]).all()
    assert q[:, 0].min(initial=0) >= 0 and q[:, 0].max(initial=0) < len(lengths)
    return dict(name=name, family=family, names=["ctg%d" % i for i in range(len(lengths))], lengths=[int(x) for x in lengths], cols=cols,
                queries=q, min_q=MIN_Q, max_ins=MAX_INS, large=large, **extra)


# ----------------------------------------------------------------------------------------------------- predicate edges
MAPQ_VALUES = (MIN_Q - 1, MIN_Q, MIN_Q + 1, 0, 255)
TLEN_VALUES = (MAX_INS, -MAX_INS, MAX_INS + 1, -(MAX_INS + 1), MAX_INS - 1, -(MAX_INS - 1), 0, I32_MIN, I32_MAX)
FLAG_BITS = tuple(a | b | c for a in (0, 0x4) for b in (0, 0x8) for c in (0, 0x400))
BP_NEAR_ORIGIN = (0, 19, 20, 21, 49, 50, 51)
EDGE_LENGTHS = (100_000, 50_000, 30_000, 10_000, I32_MAX)         # ctg3 holds no read: it is the "other" contig of the mates
EDGE_OTHER = 3


def _edge_probes(R, tid, L, s, e, bp):
    """the reads aimed at ONE query: for every comparison of the chain three reads whose operand sits at -1, 0 and +1 of the other,
    everything else arranged so that the read is still live there; then the flag, mapq, tlen, mate_tid and mate_pos grids"""
    q_start, q_end = s, min(e + MAX_INS, L)
    if q_start >= q_end:
        q_start = q_end - 10

    def add(rs, re, **kw):
        R.add(tid, L, rs, min(re, L), **kw)
    below = max(0, e - 5)                                           # a mate position that keeps a read starting behind `end`
    for d in (-1, 0, 1):
        add(q_end + d, q_end + d + 1000, mpos=below)                                        # fetch: pos < q_end
        add(q_start + d - 100, q_start + d)                                                 # fetch: end > q_start
        add(max(0, q_start + d - 3), q_start + d)
        add(e + 5, e + 1005, mpos=e + d)                                                    # :92 mpos > end
        add(e + d, e + d + 100, mpos=e + 50)                                                # :92 rs > end
        add(e + d, e + d + 100, mpos=-1, flag=0x9)                                          # :95
        add(e + d, e + d + 1000, mpos=below, sa=True, tlen=MAX_INS + 1)                     # :101, :127; SA + discordant behind `end`
        add(bp - 20 + d, bp + 100)                                                          # :116 rs < bp-20
        add(max(0, bp - 100), bp + 20 + d)                                                  # :116 re > bp+20
        add(max(0, bp - 80), bp + 100, mpos=bp - 50 + d)                                    # :119 mpos < bp-50
        add(max(0, bp - 100), bp + 50 + d, mpos=max(-1, bp - 200))                          # :119 re > bp+50
        add(max(0, s + d - 100), s + d, sa=True, mtid=EDGE_OTHER)                           # :125 re < start
        add(s + d, s + 50)                                                                  # :130 the r_start clip
        add(max(0, e - 50), e + d)                                                          # :133 the r_end clip
    body = dict(rs=max(0, bp - 100), re=bp + 100, mpos=max(-1, bp - 300))                   # a read every later test still sees
    for k in range(13):                                                                     # the last bases of the contig (fallback)
        add(L - 100, L - k)
    for bits, sa in itertools.product(FLAG_BITS, (False, True)):
        add(body["rs"], body["re"], mpos=body["mpos"], flag=0x1 | bits, sa=sa)
        add(e + 5, e + 1005, mpos=below, flag=0x1 | bits, sa=sa)
        add(e + 5, e + 1005, mpos=e + 50, flag=0x1 | bits, sa=sa)
    for mq in MAPQ_VALUES:
        add(body["rs"], body["re"], mpos=body["mpos"], mapq=mq)
        add(s + 5, s + 105, mapq=mq)
    for tl in TLEN_VALUES:
        add(body["rs"], body["re"], mpos=body["mpos"], tlen=tl)
        add(s + 5, s + 105, tlen=tl)
    for mt in (tid, EDGE_OTHER, -1):
        for mp in (-1, 0, body["mpos"]):
            add(body["rs"], body["re"], mpos=mp, mtid=mt)
            add(s + 5, s + 105, mpos=mp, mtid=mt)


def edge_queries():
    """(contig, start, end, bp) of the predicate-edge family, by the property each group is there for"""
    g = {}

    def bps(L, s, e):
        q_end = min(e + MAX_INS, L)
        return [(s + e) // 2, max(0, s - 60), min(e + 40, I32_MAX), min(q_end + 30, I32_MAX)]   # inside; before; behind; behind q_end
    L = EDGE_LENGTHS[0]
    g["plain"] = [(0, s, e, bp) for s, e in ((5000, 5400), (20_000, 20_000), (40_000, 40_001)) for bp in bps(L, s, e)]
    L = EDGE_LENGTHS[1]
    g["bp_near_origin"] = [(1, s, e, bp) for s, e in ((0, 100), (0, 0), (3, 60)) for bp in BP_NEAR_ORIGIN]
    L = EDGE_LENGTHS[2]
    g["q_end_at_length"] = [(2, e - 300, e, bp) for e in (L - MAX_INS - 1, L - MAX_INS, L - MAX_INS + 1) for bp in bps(L, e - 300, e)[:3]]
    g["start_at_length"] = [(2, s, s + w, bp) for s in (L - 1, L, L + 1, L + 5) for w in (0, 50) for bp in (L - 5, L - 60, L)]
    L = EDGE_LENGTHS[4]                                             # coordinates just below 2^31: end + max_ins leaves int32
    g["int32_top"] = [(4, s, e, bp) for s, e in ((L - 1500, L - 300), (L - 5000, L - 4400), (L - 200, L - 200)) for bp in bps(L, s, e)]
    g["int32_top"] += [(4, s, s, bp) for s in (L - 1, L) for bp in (L - 5, L)]
    return g


def edge_case():
    R = _Reads()
    groups = edge_queries()
    queries = [q for grp in groups.values() for q in grp]
    for t, s, e, bp in queries:
        _edge_probes(R, t, EDGE_LENGTHS[t], s, e, bp)
    return _case("predicate_edges", "edges", EDGE_LENGTHS, R.cols(), queries, groups={k: len(v) for k, v in groups.items()})


# ----------------------------------------------------------------------------------------------------- search shapes
SEARCH_N = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4160, 262143, 262144, 262145, 262209)
SEARCH_SMALL = tuple(n for n in SEARCH_N if n <= 4160)
SEARCH_LARGE = tuple(n for n in SEARCH_N if n > 4160)
SEARCH_PATTERNS = ("increasing", "runs", "equal")
SEARCH_LENGTH = 4_000_000
SEARCH_SPAN = 100
NQ_TAILS = (1, 3, 4, 5)


def search_probes(a, v):
    """the element indices the wave-cooperative 64-ary lower bound (first i with a[i] >= v) loads, round by round: a bracket [lo, hi)
    wider than 64 is cut in 64 chunks of c = (hi - lo) >> 6 and lane j looks at lo + (j + 1) * c - 1.  -> (list of index arrays, result)
    A model of the search's geometry, used only to show that a generated run of equal starts lies across a probed index."""
    lo, hi, rounds = 0, len(a), []
    while hi - lo > 64:
        c = (hi - lo) >> 6
        idx = lo + (np.arange(64) + 1) * c - 1
        rounds.append(idx)
        k = int((a[idx] < v).sum())
        lo, hi = lo + k * c, (lo + (k + 1) * c - 1 if k < 64 else hi)
    return rounds, lo + int((a[lo:hi] < v).sum())


def search_runs(n):
    """[(first index, length)] of the runs of equal starts of pattern "runs": one across the first round's probe of lane 31, and where
    the search has a second round one across a probe of that round (inside the first round's chunk 45)"""
    c1 = n >> 6
    if n < 127:
        return []
    r1 = min(5000, max(65, c1 + c1 // 2 + 1), n)
    lo1 = max(0, min(32 * c1 - 1 - r1 // 2, n - r1))
    runs = [(lo1, r1)]
    if c1 - 1 > 64:
        c2 = (c1 - 1) >> 6
        r2 = max(65, 2 * c2 + 1)
        runs.append((45 * c1 + 20 * c2 - 1 - r2 // 2, r2))
    return runs


def search_starts(n, pattern):
    a = 3000 + 3 * np.arange(n, dtype=np.int64)
    if pattern == "equal":
        a[:] = 9000
    elif pattern == "runs":
        for lo, r in search_runs(n):
            a[lo:lo + r] = a[lo]
    return a


def search_query_values(a, few=False):
    """the key values aimed at: the stored starts at the ends, around the first round's chunk borders and inside the runs, each
    with its two neighbours, plus one below the first and one above the last start"""
    n = len(a)
    if n == 0:
        return [2990, 3000, 3010]
    c1 = max(1, n >> 6)
    ks = (1, 32, 64) if few else (1, 2, 31, 32, 33, 45, 46, 63, 64)
    idx = {0, 1, n - 2, n - 1} | {k * c1 + d for k in ks for d in (-2, -1, 0)}
    c2 = max(1, (c1 - 1) >> 6)
    idx |= {45 * c1 + k * c2 + d for k in ((20, 64) if few else (1, 19, 20, 21, 63, 64)) for d in (-1, 0)}
    vals = {int(a[0]) - 5, int(a[-1]) + 5}
    for i in idx:
        if 0 <= i < n:
            vals |= {int(a[i]) - 1, int(a[i]), int(a[i]) + 1}
    return sorted(vals)


def search_queries(tid, a, few=False):
    """for every aimed value v one query whose upper key q_end is v and one whose lower key q_start - max_span is v"""
    q = []
    for v in search_query_values(a, few):
        e = v - MAX_INS
        q.append((tid, e - 10, e, e - 5))                           # q_end = end + max_ins = v (far from the contig end: no clamp)
        s = v + SEARCH_SPAN
        q.append((tid, s, s + 7, s + 3))                            # q_start - max_span = v
    return q


def _search_case(name, ns, patterns, seed, large=False, nq=None, few=False):
    rng = np.random.default_rng(seed)
    parts, queries, shape = [], [], []
    for n in ns:
        for p in patterns:
            t = len(shape)
            a = search_starts(n, p)
            parts.append(_random_contig(rng, t, a, SEARCH_LENGTH, n_contigs=len(ns) * len(patterns), span=SEARCH_SPAN))
            queries += search_queries(t, a, few)
            shape.append((n, p))
    if nq is not None:
        queries = queries[::max(1, len(queries) // nq)][:nq]                   # spread over the contigs
    return _case(name, "search", [SEARCH_LENGTH] * len(shape), concat_cols(parts), queries, large=large, shape=shape)


def _search_specs(large=True):
    specs = [("search_small_" + p, dict(ns=SEARCH_SMALL, patterns=(p,), seed=100 + i)) for i, p in enumerate(SEARCH_PATTERNS)]
    specs += [("search_nq%d" % k, dict(ns=(129, 4097), patterns=("runs",), seed=200 + k, nq=k)) for k in NQ_TAILS]
    if large:
        specs += [("search_n%d" % n, dict(ns=(n,), patterns=SEARCH_PATTERNS, seed=300 + i, large=True, few=True)) for i, n in enumerate(SEARCH_LARGE)]
    return specs


def search_cases(large=True):
    return [_search_case(name, **kw) for name, kw in _search_specs(large)]


# ----------------------------------------------------------------------------------------------------- span
SPAN_N, SPAN_FAR, SPAN_AT = 400_000, 7, 350_000


def span_case():
    """reads 7 and 9 of 400 000 reach hundreds of thousands of records forward: read 7 ends exactly 1 past the start of read 350 000,
    read 9 exactly on it.  The lower bound must reach back by the contig's true maximum span to count read 7 for a query starting
    there, and `end > q_start` must drop read 9."""
    rng = np.random.default_rng(41)
    L = 2_000_000
    a = 1000 + 3 * np.arange(SPAN_N, dtype=np.int64)
    c = _random_contig(rng, 1, a, L, span=60)
    x = int(a[SPAN_AT])
    for i, e in ((SPAN_FAR, x + 1), (SPAN_FAR + 2, x)):
        c["end"][i], c["flag"][i], c["mapq"][i], c["mate_tid"][i], c["tlen"][i] = e, 0x1, 60, 1, 300
        c["mate_pos"][i] = a[i] + 200
    queries = [(1, x, x + 200, x + 100), (1, x + 1, x + 201, x + 100), (1, x - 1, x + 50, x), (1, x, x, x),
               (1, x - 5000, x - 4000, x - 4500), (1, 0, 100, 50), (1, int(a[-1]), int(a[-1]) + 10, int(a[-1])), (0, 5, 50, 20),
               (2, 5, 50, 20)]
    few = _random_contig(rng, 2, [10, 10, 40], 1000, span=60)
    return _case("far_read", "span", [1000, L, 1000], concat_cols([c, few]), queries, large=True, far_index=SPAN_FAR, at=x)


def counts_case_names(large=True):
    """the names of the counts cases, without building one (the large ones hold millions of reads)"""
    return ["predicate_edges"] + [name for name, _ in _search_specs(large)] + (["far_read"] if large else [])


def counts_case(name):
    if name == "predicate_edges":
        return edge_case()
    if name == "far_read":
        return span_case()
    return _search_case(name, **dict(_search_specs(True))[name])


def counts_cases(large=True):
    return [counts_case(name) for name in counts_case_names(large)]


# ===================================================================================================== pack
PACK_SIZES = (1, 63, 64, 65, 255, 256, 257, 70_000)
EV_FLOOR = 1 << 20


def _pack_contigs(rng, tids, n_contigs, L=3_000_000):
    """random sorted reads for the given (ascending, -1 last) contig of every record"""
    tids = np.asarray(tids, dtype=np.int64)
    parts = []
    for t in sorted(set(tids.tolist()) - {-1}):
        n = int((tids == t).sum())
        parts.append(_random_contig(rng, t, np.sort(rng.integers(0, L - 200, n)), L, n_contigs=n_contigs, span=100))
    k = int((tids == -1).sum())
    if k:
        parts.append(make_cols(tid=np.full(k, -1), pos=np.full(k, -1), end=np.zeros(k), mapq=np.zeros(k), flag=np.full(k, 4),
                               mate_tid=np.full(k, -1), mate_pos=np.full(k, -1), tlen=np.zeros(k), sa_off=np.full(k, -1)))
    return concat_cols(parts)


def _widen(cols, i, by):
    """record i becomes the widest read of its contig by far"""
    cols["end"][i] = cols["pos"][i] + by
    return i


def expected_capacities(capacity, appends):
    """the store's capacity after every append, by the rule of ev_reserve: when n + more does not fit, the new capacity is the largest
    of 1.5 x the old one, n + more and 2^20 records.  -> (capacities, the rule that produced each: None / "floor" / "x1.5" / "exact")"""
    caps, why, n = [], [], 0
    for more in appends:
        rule = None
        if n + more > capacity:
            grown = capacity + capacity // 2
            capacity, rule = max((EV_FLOOR, "floor"), (n + more, "exact"), (grown, "x1.5"))
        n += more
        caps.append(capacity)
        why.append(rule)
    return caps, why


PACK_SMALL = tuple("n%d" % n for n in PACK_SIZES) + ("wave_of_2_contigs", "wave_of_5_contigs", "three_appends")
PACK_LARGE = ("grow_from_0", "grow_from_1000")


def pack_cases(large=True):
    """each: names, lengths, batches (column sets appended one after the other), capacity, and what the batches were built to hold;
    the names are PACK_SMALL (+ PACK_LARGE)"""
    out = []

    def case(name, n_contigs, batches, capacity=0, **extra):
        out.append(dict(name=name, names=["ctg%d" % i for i in range(n_contigs)], lengths=[3_000_000] * n_contigs, batches=batches,
                        capacity=capacity, min_q=MIN_Q, max_ins=MAX_INS, **extra))
    for j, n in enumerate(PACK_SIZES):
        rng = np.random.default_rng(500 + j)
        tids = np.sort(rng.integers(0, 3, n)) if n > 256 else np.zeros(n, dtype=np.int64)
        c = _pack_contigs(rng, tids, 3)
        _widen(c, n // 2, 5000 + n)
        c["tlen"][0] = I32_MIN                                      # |tlen| in 64 bits: discordant
        c["tlen"][n - 1] = I32_MAX
        c["mate_tid"][0], c["mate_tid"][n - 1] = c["tid"][0], c["tid"][n - 1]      # (discordant by |tlen| alone)
        case("n%d" % n, 3, [c])
    # one 64-record wave (records 64..127) holds 2 contigs; the widest read of the second sits in lane 37 of that wave
    rng = np.random.default_rng(520)
    c = _pack_contigs(rng, [0] * 100 + [1] * 156, 2)
    case("wave_of_2_contigs", 2, [c], wave=1, wide=[_widen(c, 5, 7000), _widen(c, 101, 9000)])
    # the first wave holds 5 contigs (ctg2 is empty); the widest read of ctg4 in lane 47, of ctg1 in lane 12
    c = _pack_contigs(rng, [0] * 10 + [1] * 10 + [3] * 10 + [4] * 20 + [5] * 150, 6)
    case("wave_of_5_contigs", 6, [c], wave=0, wide=[_widen(c, 12, 6000), _widen(c, 47, 8000), _widen(c, 130, 4000)])
    # ctg1 runs over three appends with its widest read in the middle one; ctg2 empty; an unplaced tail
    c = _pack_contigs(rng, [0] * 40 + [1] * 240 + [3] * 35 + [-1] * 5, 4)
    case("three_appends", 4, [slice_cols(c, 0, 100), slice_cols(c, 100, 230), slice_cols(c, 230, 320)], wide=[_widen(c, 170, 12_000)])
    if large:
        for name, cap, sizes in (("grow_from_0", 0, (400_000, 400_000, 400_000)),
                                 ("grow_from_1000", 1000, (700, 600, 600_000, 600_000, 1_500_000))):
            rng = np.random.default_rng(530 + cap)
            n = sum(sizes)
            c = _pack_contigs(rng, np.arange(n) // 250_000, -(-n // 250_000))
            cuts = np.concatenate([[0], np.cumsum(sizes)])
            case(name, -(-n // 250_000), [slice_cols(c, int(a), int(b)) for a, b in zip(cuts, cuts[1:])], capacity=cap, sizes=sizes)
    return out


# ===================================================================================================== means
KEPT_COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 8191, 8192, 8193, 16385)
MASK_KINDS = ("all", "none", "alternating", "lane0", "lane63", "random")
VALUE_FAMILIES = ("gamma", "cancel", "special")
MEAN_OFFSETS = (0, 1, 3, 5)


def mean_mask(kind, kept, rng):
    """a gc column (-1: dropped, else kept) with exactly `kept` kept bins, positions relative to the segment's first bin (where the
    kernel's 64-lane ballot starts); None where the kind cannot give that count"""
    if kind == "all":
        g = np.full(kept, 41)
    elif kind == "none":
        if kept:
            return None
        g = np.full(200, -1)
    elif kind == "alternating":
        g = np.where(np.arange(2 * kept) % 2 == 1, 0, -1)           # (gc 0 is a kept bin: the test is gc > -1)
    elif kind in ("lane0", "lane63"):
        g = np.full(64 * kept, -1)
        g[(0 if kind == "lane0" else 63)::64] = 100
    else:
        g = np.full(2 * kept + 3, -1)
        g[rng.choice(len(g), kept, replace=False)] = rng.integers(0, 101, kept)
    return g.astype(np.int8)


def mean_values(family, n, rng):
    if family == "gamma":
        return rng.gamma(30, 1.0, n) * rng.choice([1e-3, 1.0, 1e3], n)
    if family == "cancel":                                          # +-1e16 swallow the O(1) terms unless the order is numpy's
        v = rng.integers(1, 9, n).astype(np.float64)
        v[0::4], v[2::4] = 1e16, -1e16
        return v
    palette = [(-0.0,), (-0.0, np.inf), (-0.0, -np.inf), (-0.0, np.inf, -np.inf, np.nan)][int(rng.integers(0, 4))]
    return rng.choice(np.array(palette), n)


def means_case(family):
    """-> (coverage dict, gc dict, segments [(contig, s, e)], masked flags, kept count of every segment): one contig per
    (mask kind, kept count, offset); the all-kept masks are also averaged unmasked.  The 64-bin-stride masks use two offsets only."""
    rng = np.random.default_rng(600 + VALUE_FAMILIES.index(family))
    cov, gc, segs, masked, kept = {}, {}, [], [], []
    for kind in MASK_KINDS:
        for k in KEPT_COUNTS:
            for off in (MEAN_OFFSETS if kind not in ("lane0", "lane63") else (0, 5)):
                g = mean_mask(kind, k, rng)
                if g is None:
                    continue
                name = "%s_%d_%d" % (kind, k, off)
                cov[name] = mean_values(family, off + len(g), rng)
                gc[name] = np.concatenate([np.full(off, 7, dtype=np.int8), g])
                segs.append((name, off, off + len(g)))
                masked.append(1)
                kept.append(k)
                if kind == "all":
                    segs.append((name, off, off + len(g)))
                    masked.append(0)
                    kept.append(k)
    return cov, gc, segs, masked, kept
