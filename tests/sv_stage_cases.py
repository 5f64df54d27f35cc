"""Adversarial inputs and plain references for the three device stages of `tiddit --sv` that the whole-file fixtures reach only
through one family of synthetic BAMs: the library statistics (csrc/tdt_stats.hip), the per-read action chain with its gather
(csrc/tdt_signal.hip) and the masked medians (csrc/tdt_median.hip).

Everything here is deterministic (numpy.random.default_rng with fixed seeds) and written from the rules, in numpy and plain Python; the
references share no code with tiddit_amd (the BAM files are written with its test writer, bamio.BamWriter).  The references are pinned
on the CPU by test_sv_stage_refs_cpu.py and compared with the kernels by test_gpu_sv_stages.py.  Test infrastructure only."""
import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
COLS = ("tid", "pos", "mate_tid", "mate_pos", "tlen", "l_seq", "flag", "mapq")
_DT = dict(tid=np.int32, pos=np.int32, mate_tid=np.int32, mate_pos=np.int32, tlen=np.int32, l_seq=np.int32, flag=np.uint16, mapq=np.uint8)


# =============================================================================================== library statistics: references
def _concat(cols_batches):
    return {k: np.concatenate([np.asarray(b[k]) for b in cols_batches]) if cols_batches else np.zeros(0, _DT[k]) for k in COLS}


def stats_reference(cols_batches, n_reads, min_mapq, max_ins_len):
    """The sampling rules of tiddit_stats.statistics (tiddit_stats.py:17-47) on decoded columns, vectorised.
    -> (counters, insert sizes in order as int32).  counters: sampled, sum_len, n_len, innie, outtie, n_ins, sum_ins.
    Only placed reads (tid >= 0) are visited; a read's n_sampled is the running count of placed reads including itself.  The read
    length is appended before the cut-off test, so reads up to n_sampled == n_reads + 1 leave their length behind; the pair tests see
    reads up to n_sampled == n_reads."""
    c = _concat(cols_batches)
    placed = c["tid"] >= 0
    ns = np.cumsum(placed, dtype=np.int64)
    in_len = placed & (ns <= n_reads + 1)
    f = c["flag"].astype(np.int64)
    rev, mrev = (f & 0x10) != 0, (f & 0x20) != 0
    ok = placed & (ns <= n_reads)
    ok &= (f & 0x8) == 0
    ok &= rev != mrev
    ok &= (c["mate_tid"] == c["tid"]) & (c["tlen"].astype(np.int64) <= max_ins_len)
    ok &= c["mate_pos"] >= c["pos"]
    ok &= ((f & 0x800) == 0) & ((f & 0x100) == 0) & ((f & 0x400) == 0) & (c["mapq"].astype(np.int64) >= min_mapq)
    ins = c["tlen"][ok].astype(np.int32)
    outtie = int((ok & rev & ~mrev).sum())
    counters = dict(sampled=int(min(int(placed.sum()), n_reads + 1)), sum_len=int(c["l_seq"][in_len].astype(np.int64).sum()),
                    n_len=int(in_len.sum()), innie=int(ok.sum()) - outtie, outtie=outtie, n_ins=int(len(ins)),
                    sum_ins=int(ins.astype(np.int64).sum()))
    return counters, ins


def stats_loop(cols_batches, n_reads, min_mapq, max_ins_len):
    """the same rules, read by read (the loop of tests/test_gpu_pipeline.py::test_stats_vs_per_read_loop on columns)"""
    c = {k: v.tolist() for k, v in _concat(cols_batches).items()}
    sum_len = n_len = innie = outtie = ns = 0
    ins = []
    for i in range(len(c["tid"])):
        if c["tid"][i] < 0:
            continue
        sum_len += c["l_seq"][i]
        n_len += 1
        ns += 1
        if ns > n_reads:
            break
        f = c["flag"][i]
        if f & 0x8 or bool(f & 0x10) == bool(f & 0x20):
            continue
        if c["mate_tid"][i] != c["tid"][i] or c["tlen"][i] > max_ins_len:
            continue
        if c["mate_pos"][i] < c["pos"][i]:
            continue
        if f & 0x800 or f & 0x100 or f & 0x400 or c["mapq"][i] < min_mapq:
            continue
        ins.append(c["tlen"][i])
        if f & 0x10 and not f & 0x20:
            outtie += 1
        else:
            innie += 1
    counters = dict(sampled=ns, sum_len=sum_len, n_len=n_len, innie=innie, outtie=outtie, n_ins=len(ins), sum_ins=sum(ins))
    return counters, np.array(ins, dtype=np.int32)


def done_flags(cols_batches, n_reads):
    """per batch: has the reference's loop met its break (`n_sampled > n_reads`) by the end of this batch"""
    placed = np.cumsum([int((np.asarray(b["tid"]) >= 0).sum()) for b in cols_batches])
    return [bool(p > n_reads) for p in placed]


def percentile_ranks(n):
    """the two order statistics numpy.percentile(x, 99.9) (method "linear") interpolates between, for n values"""
    vi = (n - 1) * np.true_divide(99.9, 100)
    k0 = int(np.floor(vi))
    return k0, min(k0 + 1, n - 1)


def stats_figures(ins):
    """(mean, std, 99.9th percentile) of the insert-size list, by the numpy calls of tiddit_stats.py:52-56"""
    return np.average(ins), np.std(ins), np.percentile(ins, 99.9)


# =============================================================================================== library statistics: inputs
MIN_MAPQ = 10
# what a read that must NOT join the insert-size list gets wrong — each exactly one step past its filter's edge
FAIL_KINDS = ("mapq", "tlen", "mate_pos", "f0x8", "both_rev", "both_fwd", "f0x100", "f0x400", "f0x800", "mate_tid", "unplaced")
# ... and where a read that joins it sits ON an edge
PASS_KINDS = ("plain", "mapq_edge", "mate_pos_edge")
TLEN_FAMILIES = ("equal", "two", "uniform", "top1", "top2", "top3", "fixture")
INSERT_LENGTHS = (1, 2, 3, 255, 256, 257, 8191, 8192, 8193, 16385)
LARGE_INSERTS = 1_150_000
D_BASE = {1: 0x12000000, 2: 0xF2340000 - (1 << 32), 3: 0x2B3C4D00}       # family top<k>: the k top bytes every value shares


def tlen_family(name, n, seed):
    """n insert sizes of one family, in list order (int32).  equal: one value.  two: two values split so that the percentile's ranks
    k0 and k1 (percentile_ranks) fall on different values, of different sign and top byte.  uniform: over [-2^30, 2^30).  top<k>: the
    k top bytes are shared, the bytes below are uniform, so byte k is the first that differs.  fixture: the synthetic BAMs' own shape,
    N(400, 40) with a few large pairs."""
    rng = np.random.default_rng(seed)
    if name == "equal":
        v = np.full(n, 417)
    elif name == "two":
        k0, k1 = percentile_ranks(n)
        v = np.where(np.arange(n) <= k0, -3, (1 << 24) + 5)
        if k1 == k0:
            v[:] = -3
        v = rng.permutation(v)
    elif name == "uniform":
        v = rng.integers(-(1 << 30), 1 << 30, n)
    elif name.startswith("top"):
        k = int(name[3:])
        v = D_BASE[k] + rng.integers(0, 1 << (8 * (4 - k)), n)
        if n >= 2:                                                     # byte k really takes more than one value
            v[0], v[1] = D_BASE[k], D_BASE[k] + (1 << (8 * (4 - k))) - 1
    elif name == "fixture":
        v = np.rint(rng.normal(400, 40, n)).astype(np.int64)
        big = rng.random(n) < 0.01
        v[big] = rng.integers(1000, 100000, int(big.sum()))
    else:
        raise KeyError(name)
    return v.astype(np.int32)


def stats_columns(tlen_pass, seed, max_ins_len, min_mapq=MIN_MAPQ, fail_frac=0.3):
    """Decoded columns in which exactly the reads carrying `tlen_pass` (in that order) pass every filter of the sampling loop; reads
    that fail are scattered between them, each failing ONE filter by one step (FAIL_KINDS, every kind at least once), and carry
    insert sizes drawn from the same family, so that letting one in would move the figures.  The passing reads rotate through
    PASS_KINDS: mapq == min_mapq and mate_pos == pos sit on their edges; tlen == max_ins_len does when the caller passes the family's
    maximum.  -> (columns, kind of every read)"""
    rng = np.random.default_rng(seed)
    tlen_pass = np.asarray(tlen_pass, dtype=np.int32)
    L = len(tlen_pass)
    assert L == 0 or int(tlen_pass.max()) <= max_ins_len
    kinds_f = [k for k in FAIL_KINDS if not (k == "tlen" and max_ins_len + 1 > I32_MAX)]
    n_fail = int(L * fail_frac) + len(kinds_f)
    N = L + n_fail
    is_pass = np.zeros(N, dtype=bool)
    is_pass[rng.permutation(N)[:L]] = True
    tid = rng.integers(0, 3, N).astype(np.int32)
    pos = rng.integers(0, 1_000_000, N).astype(np.int32)
    c = dict(tid=tid, pos=pos, mate_tid=tid.copy(), mate_pos=(pos + rng.integers(1, 500, N)).astype(np.int32),
             tlen=np.zeros(N, np.int32), l_seq=rng.integers(30, 251, N).astype(np.int32),
             flag=(0x1 | np.where(rng.random(N) < 0.5, 0x10, 0x20) | rng.choice([0, 0x2, 0x40, 0x80, 0x200], N)).astype(np.uint16),
             mapq=rng.integers(min_mapq + 1, 61, N).astype(np.uint8))
    c["tlen"][is_pass] = tlen_pass
    c["tlen"][~is_pass] = tlen_pass[rng.integers(0, L, n_fail)] if L else 400
    kind = np.empty(N, dtype=object)
    pk = np.array(PASS_KINDS, dtype=object)[np.arange(L) % len(PASS_KINDS)]
    kind[is_pass] = pk
    fk = np.array(kinds_f, dtype=object)[rng.permutation(np.arange(n_fail) % len(kinds_f))]
    kind[~is_pass] = fk
    m = kind == "mapq_edge"
    c["mapq"][m] = min_mapq
    m = kind == "mate_pos_edge"
    c["mate_pos"][m] = c["pos"][m]
    m = kind == "mapq"
    c["mapq"][m] = min_mapq - 1
    m = kind == "tlen"
    c["tlen"][m] = min(max_ins_len + 1, I32_MAX)
    m = kind == "mate_pos"
    c["pos"][m] += 1
    c["mate_pos"][m] = c["pos"][m] - 1
    for k, bits in (("f0x8", 0x8), ("f0x100", 0x100), ("f0x400", 0x400), ("f0x800", 0x800), ("both_rev", 0x30)):
        c["flag"][kind == k] |= bits
    c["flag"][kind == "both_fwd"] &= 0xffff ^ 0x30
    m = kind == "mate_tid"
    c["mate_tid"][m] = (c["tid"][m] + 1) % 3
    c["tid"][kind == "unplaced"] = -1
    return c, kind


def unplaced_batch(n, seed):
    """n reads without a contig (the unplaced tail of a BAM) whose other fields would pass every filter"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, 1000, n).astype(np.int32)
    return dict(tid=np.full(n, -1, np.int32), pos=pos, mate_tid=np.full(n, -1, np.int32), mate_pos=pos + 1, tlen=np.full(n, 333, np.int32),
                l_seq=np.full(n, 151, np.int32), flag=np.full(n, 0x21, np.uint16), mapq=np.full(n, 60, np.uint8))


def split_batches(cols, sizes):
    """the columns cut into consecutive batches whose sizes cycle through `sizes`"""
    out, o, k, n = [], 0, 0, len(cols["tid"])
    while o < n:
        s = sizes[k % len(sizes)]
        out.append({c: cols[c][o:o + s] for c in COLS})
        o += s
        k += 1
    return out


def _case(name, batches, n_reads, max_ins_len, **kw):
    d = dict(name=name, batches=batches, n_reads=int(n_reads), min_mapq=MIN_MAPQ, max_ins_len=int(max_ins_len), figures=True, large=False)
    d.update(kw)
    return d


def _n_placed(batches):
    return int(sum(int((b["tid"] >= 0).sum()) for b in batches))


def stats_value_cases():
    """every insert-size family at every list length of INSERT_LENGTHS: the whole data is sampled (n_reads beyond the data for odd
    lengths, exactly the number of placed reads for even ones), in ONE batch or in many small ones; max_ins_len is the family's maximum"""
    out = []
    for fi, fam in enumerate(TLEN_FAMILIES):
        for li, L in enumerate(INSERT_LENGTHS):
            t = tlen_family(fam, L, 1000 + 37 * fi + li)
            cols, _ = stats_columns(t, 5000 + 41 * fi + li, int(t.max()))
            batches = [cols] if (fi + li) % 2 == 0 else split_batches(cols, (257, 64, 1, 1024, 63))
            n_reads = _n_placed(batches) + (1000 if L % 2 else 0)
            out.append(_case("%s-%d" % (fam, L), batches, n_reads, int(t.max())))
    return out


BATCH_SIZES = (1, 63, 64, 65, 255, 256, 257, 1024 * 256 - 1, 1024 * 256 + 1, 300_007)


def stats_large_cases():
    """two lists of LARGE_INSERTS insert sizes (several 8192-chunks of the numpy-order sum, more than one grid-stride round of the
    select's histogram) cut into every batch size of BATCH_SIZES, an all-unplaced batch among them"""
    out = []
    for fam, seed in (("uniform", 71), ("fixture", 72)):
        t = tlen_family(fam, LARGE_INSERTS, seed)
        cols, _ = stats_columns(t, seed + 100, int(t.max()), fail_frac=0.05)
        batches = split_batches(cols, BATCH_SIZES)
        batches.insert(4, unplaced_batch(300, seed))
        out.append(_case("large-" + fam, batches, _n_placed(batches) + 5, int(t.max()), large=True))
    return out


def stats_extreme_case():
    """INT32_MIN and INT32_MAX in the list (uniform over the whole int32 range otherwise): numpy's own int32 interpolation wraps here,
    so only the counters and the order statistics are asserted.  1000 values: the percentile's upper rank is the maximum itself."""
    rng = np.random.default_rng(99)
    t = rng.integers(I32_MIN, I32_MAX + 1, 1000).astype(np.int32)
    t[123], t[877] = I32_MAX, I32_MIN
    cols, _ = stats_columns(t, 98, I32_MAX)
    return _case("int32-extremes", split_batches(cols, (500,)), 10 ** 6, I32_MAX, figures=False)


CUT_TARGETS = ("lane0", "lane63", "lane64", "tile_last", "tile_first", "batch_last", "next_batch_first", "before_unplaced_batch",
               "after_unplaced_batch", "zero", "one", "beyond", "exact_total")


def stats_cutoff_cases():
    """one data set (uniform insert sizes, batches of 1000 reads = four 256-read tiles, batch 4 all unplaced) with the cut-off n_reads
    chosen so that the n_reads-th placed read is a given read of batch 2: lane 0, 63 or 64 of a wave, the last / first read of a tile,
    the last read of the batch, the first of the next; the reads either side of the all-unplaced batch; and n_reads = 0, 1, beyond the
    data, exactly the number of placed reads.  -> cases, each with "cut" = (batch, offset) of the n_reads-th placed read or None"""
    t = tlen_family("uniform", 6000, 7)
    cols, _ = stats_columns(t, 8, int(t.max()))
    where = {"lane0": (2, 512), "lane63": (2, 63), "lane64": (2, 64), "tile_last": (2, 255), "tile_first": (2, 256), "batch_last": (2, 999),
             "next_batch_first": (3, 0), "before_unplaced_batch": (3, 999), "after_unplaced_batch": (5, 0)}
    batches = split_batches(cols, (1000,))
    batches.insert(4, unplaced_batch(1000, 9))
    for b, o in where.values():                                        # the targeted reads are placed ones
        for k in COLS:
            batches[b][k] = batches[b][k].copy()
        if batches[b]["tid"][o] < 0:
            batches[b]["tid"][o] = 0
    total = _n_placed(batches)
    out = []
    for name in CUT_TARGETS:
        if name in where:
            b, o = where[name]
            n_reads = sum(int((x["tid"] >= 0).sum()) for x in batches[:b]) + int((batches[b]["tid"][:o + 1] >= 0).sum())
            cut = (b, o)
        else:
            n_reads, cut = {"zero": 0, "one": 1, "beyond": total + 12345, "exact_total": total}[name], None
        out.append(_case("cut-" + name, batches, n_reads, int(t.max()), cut=cut))
    return out


def stats_filter_case():
    """a small case for the literal loop in which every FAIL_KIND and PASS_KIND occurs several times; -> (case, kinds)"""
    t = tlen_family("uniform", 400, 3)
    cols, kind = stats_columns(t, 4, int(t.max()), fail_frac=0.5)
    return _case("filters", split_batches(cols, (97,)), 550, int(t.max())), kind


def stats_cases(large=True):
    out = stats_value_cases() + stats_cutoff_cases() + [stats_filter_case()[0], stats_extreme_case()]
    return out + (stats_large_cases() if large else [])


# =============================================================================================== signal scan: records and rules
SCAN_CONTIGS = [("chr1", 5_000_000), ("chr2", 3_000_000), ("small", 5_000)]
# the parameter set whose three lengths are exactly the generated edge values, and two others
SCAN_EDGE = dict(min_q=5, max_ins=600, min_contig=10_000, min_anchor_len=60, min_clip_len=25)
SCAN_PARAMS = (SCAN_EDGE, dict(min_q=20, max_ins=450, min_contig=1_000, min_anchor_len=30, min_clip_len=20),
               dict(min_q=0, max_ins=100_000, min_contig=4_000_000, min_anchor_len=100, min_clip_len=39))
_SA = "chr2,7000,+,70S80M,60,0;"
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rec(label, qname="q", flag=0x21, tid=0, pos=1000, mapq=60, cigar="150M", mate_tid=None, mate_pos=None, tlen=400, seq="", tags=()):
    return dict(label=label, qname=qname, flag=flag, tid=tid, pos=pos, mapq=mapq, cigar=cigar, mate_tid=tid if mate_tid is None else mate_tid,
                mate_pos=pos + 200 if mate_pos is None else mate_pos, tlen=tlen, seq=seq, tags=tuple(tags))


def _seq(rng, n):
    return _BASES[rng.integers(0, 4, n)].tobytes().decode()


def scan_edge_records(E=SCAN_EDGE):
    """every comparison of the action chain on its edge and one step past it; label -> what the record is (unique)"""
    mi, mc, ma, mq = E["max_ins"], E["min_clip_len"], E["min_anchor_len"], E["min_q"]
    clip = "%dS%dM" % (mc + 15, ma + 50)                               # a CIGAR that qualifies as clipped
    R = []
    for sign in (1, -1):                                               # |tlen| against max_ins: < for clips, > for discordants
        for d in (-1, 0, 1):
            R.append(_rec("tlen%+d*(max_ins%+d)" % (sign, d), cigar=clip, tlen=sign * (mi + d)))
    R.append(_rec("tlen=int32_min", cigar=clip, tlen=I32_MIN))
    for c in (mc, mc + 1):                                             # clip and anchor lengths, either end
        for a in (ma, ma + 1):
            R.append(_rec("left_clip%d_anchor%d" % (c - mc, a - ma), cigar="%dS%dM" % (c, a)))
            R.append(_rec("right_clip%d_anchor%d" % (c - mc, a - ma), cigar="%dM%dS" % (a, c)))
    for cig in ("10H40S100M", "40S100M10H", "40S110=", "110=40S", "40S100M10I", "10I100M40S", "40I110M", "40H110M", "110M40H",
                "150M", "150S", "40S20M5D85M", "40S60M40S", ""):
        R.append(_rec("cigar:" + (cig or "none"), cigar=cig))
    R.append(_rec("cigar:none+discordant", cigar="", tlen=5000, flag=0x21))
    for q in (mq - 1, mq):                                             # mapq >= min_q
        if q >= 0:
            R.append(_rec("mapq%+d_discordant" % (q - mq), mapq=q, tlen=5000))
            R.append(_rec("mapq%+d_clip" % (q - mq), mapq=q, cigar=clip))
            R.append(_rec("mapq%+d_sa" % (q - mq), mapq=q, tags=[("SA", "Z", _SA)]))
    for bit in (0x1, 0x4, 0x8, 0x100, 0x400, 0x800):                   # every flag bit the chain reads, on each of the three actions
        for what, kw in (("discordant", dict(tlen=5000)), ("clip", dict(cigar=clip)), ("sa", dict(tags=[("SA", "Z", _SA)])),
                         ("mate_elsewhere", dict(mate_tid=1))):
            R.append(_rec("flag^0x%x_%s" % (bit, what), flag=0x21 ^ bit, **kw))
    R.append(_rec("flag_base_discordant", tlen=5000))
    R.append(_rec("flag_base_mate_elsewhere", mate_tid=1))
    R.append(_rec("mate_tid=-1,0x8_clear", mate_tid=-1, mate_pos=-1, tlen=0))
    R.append(_rec("mate_tid=-1,0x8_clear,sa", mate_tid=-1, mate_pos=-1, tlen=0, tags=[("SA", "Z", _SA)]))
    R.append(_rec("mate_tid=-1,0x8_set", flag=0x29, mate_tid=-1, mate_pos=-1, tlen=0))
    other = [("NM", "i", 3), ("MD", "Z", "150"), ("XA", "A", "x"), ("XB", "BS", [1, 2, 3]), ("XH", "H", "1AE3"), ("Xf", "f", 1.5), ("Xc", "c", -1),
             ("XS", "S", 7), ("XI", "BI", [])]
    R.append(_rec("sa_first", tags=[("SA", "Z", _SA)] + other))
    R.append(_rec("sa_last", tags=other + [("SA", "Z", _SA)]))
    R.append(_rec("sa_middle", tags=other[:5] + [("SA", "Z", _SA)] + other[5:] + [("RG", "Z", "g")]))
    R.append(_rec("sa_only_as_text", tags=[("XD", "Z", "SAZ" + _SA), ("XE", "H", "5A5A")] + other))       # no SA tag: "SAZ" inside a value
    R.append(_rec("sa_and_clip_and_discordant", cigar=clip, tlen=mi - 1, mate_tid=1, tags=other + [("SA", "Z", _SA)]))
    for what, kw in (("discordant", dict(tlen=5000)), ("clip", dict(cigar=clip)), ("sa", dict(tags=[("SA", "Z", _SA)]))):
        R.append(_rec("small_contig_" + what, tid=2, pos=100, **kw))                                        # below min_contig
    R.append(_rec("mate_on_small_contig", mate_tid=2))
    R.append(_rec("unplaced_with_sa", flag=0x4 | 0x1 | 0x8, tid=-1, pos=-1, mapq=0, cigar="", mate_tid=-1, mate_pos=-1, tlen=0,
                  tags=[("SA", "Z", _SA)]))
    assert len({r["label"] for r in R}) == len(R)
    return R


def _quiet(rng, i, tid=0):
    """a read with no action bit under any of SCAN_PARAMS; every other one carries 150 random bases (an incompressible file body)"""
    return _rec("quiet", qname="r%d" % i, pos=1000 + i, tid=tid, seq=_seq(rng, 150) if i & 1 else "", tlen=int(rng.integers(200, 440)))


def _selected(rng, i, tid=0):
    """a read with an action bit under SCAN_EDGE, of varying kind and record size"""
    k = i % 4
    name = "s%d" % i + "x" * int(rng.integers(0, 40))
    seq = _seq(rng, int(rng.integers(0, 300)))
    if k == 0:
        return _rec("sel_discordant", qname=name, pos=1000 + i, tid=tid, tlen=int(rng.integers(200_000, 900_000)) * (1 if i & 4 else -1), seq=seq)
    if k == 1:
        return _rec("sel_mate_elsewhere", qname=name, pos=1000 + i, tid=tid, mate_tid=1 - tid, seq=seq)
    if k == 2:
        return _rec("sel_sa", qname=name, pos=1000 + i, tid=tid, seq=seq, tags=[("NM", "i", i), ("SA", "Z", _SA)])
    return _rec("sel_clip", qname=name, pos=1000 + i, tid=tid, seq=seq, cigar="45S105M" if i & 4 else "105M45S", tlen=300)


def scan_records(seed=21):
    """The records of the main scan file, in file order (>= 40 000, ten or more 4096-read tiles in one batch):
      0 .. 4097      quiet reads, then selected reads at indices 4095, 4096 and 4097 (the last word of tile 0, the first of tile 1)
      edge block     scan_edge_records, twice (the second time in reverse order)
      size extremes  the smallest legal record (one-character name, no CIGAR, no sequence, no tags) and records with a 250-byte name
                     and 10 000 bases, selected and not
      empty stretch  9 000 reads, none selected
      full stretch   5 000 reads, all selected
      mix            quiet reads with ~3 % selected ones, on chr1 then chr2, up to 41 000 records
    -> (records, spans): spans[name] = (first index, end index)"""
    rng = np.random.default_rng(seed)
    R, spans = [], {}
    R += [_quiet(rng, i) for i in range(4095)] + [_selected(rng, i) for i in (4, 5, 6)]
    spans["head"] = (0, len(R))
    o = len(R)
    edge = scan_edge_records()
    R += edge + edge[::-1]
    spans["edges"] = (o, len(R))
    o = len(R)
    long_seq = _seq(rng, 10_000)
    R += [_rec("smallest_selected", qname="a", cigar="", tlen=5000), _rec("smallest_quiet", qname="b", cigar="", tlen=0),
          _rec("largest_selected", qname="L" * 250, cigar="40S9960M", seq=long_seq, tags=[("SA", "Z", _SA * 20)]),
          _rec("largest_quiet", qname="M" * 250, cigar="10000M", seq=long_seq),
          _rec("largest_selected_again", qname="N" * 250, cigar="10000M", seq=long_seq, tlen=-700_000),
          _rec("smallest_selected_again", qname="c", cigar="", tlen=-5000)]
    spans["sizes"] = (o, len(R))
    o = len(R)
    R += [_quiet(rng, i) for i in range(9000)]
    spans["empty"] = (o, len(R))
    o = len(R)
    R += [_selected(rng, i) for i in range(5000)]
    spans["full"] = (o, len(R))
    o = len(R)
    while len(R) < 41_000:
        i = len(R)
        tid = 0 if i < 32_000 else 1
        R.append(_selected(rng, i, tid) if rng.random() < 0.03 else _quiet(rng, i, tid))
    spans["mix"] = (o, len(R))
    return R, spans


def scan_count_records(n_selected, seed=22):
    """3 000 records of which exactly n_selected are selected (1023 / 1024 / 1025: either side of the gather's 1024-element scan tile)"""
    rng = np.random.default_rng(seed)
    pick = np.zeros(3000, dtype=bool)
    pick[rng.permutation(3000)[:n_selected]] = True
    return [_selected(rng, i) if pick[i] else _quiet(rng, i) for i in range(3000)]


def scan_batch(records, path):
    """the records as a small BAM (bamio.BamWriter / bamio.encode_record, file order as given, header of SCAN_CONTIGS); -> path"""
    from tiddit_amd import bamio
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in SCAN_CONTIGS)
    w = bamio.BamWriter(str(path), SCAN_CONTIGS, text=text)
    for r in records:
        w.write(r["qname"], r["flag"], r["tid"], r["pos"], r["mapq"], r["cigar"], r["mate_tid"], r["mate_pos"], r["tlen"], seq=r["seq"], tags=r["tags"])
    w.close()
    return str(path)


_CIGAR_OPS = "MIDNSHP=X"


def _cigar(s):
    out, num = [], ""
    for ch in s:
        if ch.isdigit():
            num += ch
        else:
            out.append((_CIGAR_OPS.index(ch), int(num)))
            num = ""
    return out


def record_action(r, P, contigs=SCAN_CONTIGS):
    """The action byte of one record by the per-read chain of tiddit_signal.worker (tiddit_signal.pyx:171-221), literally:
    2 = clipped read kept for assembly, 4 = has an SA tag, 8 = discordant pair."""
    if r["tid"] < 0 or contigs[r["tid"]][1] < P["min_contig"]:          # worker() runs per contig of at least min_contig
        return 0
    f = r["flag"]
    if f & 0x4 or f & 0x400:
        return 0
    if f & 0x800 or f & 0x100:
        return 0
    if r["mapq"] < P["min_q"]:
        return 0
    a = 0
    cig = _cigar(r["cigar"])
    same = r["mate_tid"] == r["tid"]
    if abs(r["tlen"]) < P["max_ins"] and same and cig:
        if (cig[0][0] == 4 and cig[0][1] > P["min_clip_len"]) and (cig[-1][0] == 0 and cig[-1][1] > P["min_anchor_len"]):
            a |= 2
        elif cig[-1][0] == 4 and cig[-1][1] > P["min_clip_len"] and (cig[0][0] == 0 and cig[0][1] > P["min_anchor_len"]):
            a |= 2
    if any(t[0] == "SA" and t[1] == "Z" for t in r["tags"]):
        a |= 4
    if not f & 0x8 and f & 0x1 and r["mate_tid"] >= 0:
        if abs(r["tlen"]) > P["max_ins"] or not same:
            a |= 8
    return a


# =============================================================================================== masked medians
MEDIAN_LENGTHS = (0, 1, 2, 3, 2047, 2048, 2049, 4096, 4097)
MEDIAN_FAMILIES = ("equal", "two", "wide", "low_byte", "dropped", "masked_segment", "many_segments")


def _segments(lengths, total, rng):
    """segments of the given lengths at odd start offsets, overlapping freely, and a last one that covers everything"""
    seg = []
    for ln in lengths:
        lo = int(rng.integers(0, (total - ln + 1) // 2)) * 2 + 1 if total - ln >= 1 else 0
        seg.append((lo, lo + ln))
    seg.append((0, total))
    return np.array(seg, dtype=np.int64)


def _wide(rng, n):
    """positive doubles whose bit patterns are spread over the whole exponent range 1e-300 .. 1e300, and subnormals"""
    v = 10.0 ** rng.uniform(-300, 300, n)
    sub = rng.random(n) < 0.05
    v[sub] = rng.integers(1, 1 << 52, int(sub.sum())).astype(np.uint64).view(np.float64)
    return v


def byte_ladder(k):
    """an odd number of positive doubles whose MEDIAN is decided in byte k of the 8-byte pattern (0 = top): every value shares the
    bytes above k with the median, several share byte k too, and the bytes below k are all zero"""
    base = 0x3FF0_0000_0000_0000 if k else 0                            # (byte 1 of the base is 0xF0: no carry into byte 0)
    step = 1 << (8 * (7 - k))
    pat = [base + j * step for j in (1, 2, 3, 3, 3, 4, 5, 6, 7)]
    return np.array(pat, dtype=np.uint64).view(np.float64)


def median_cases():
    """-> [(name, cov float64[], gc int8[], seg_off int64[nseg, 2])], one per MEDIAN_FAMILIES entry.  Every case has segments of every
    MEDIAN_LENGTHS length (2048 = one block of the histogram kernel) at odd offsets, overlapping, the last covering everything."""
    out = []
    total = 12_001
    for fi, fam in enumerate(MEDIAN_FAMILIES):
        rng = np.random.default_rng(300 + fi)
        gc = np.where(rng.random(total) < 0.07, -1, rng.integers(0, 101, total)).astype(np.int8)
        lengths = list(MEDIAN_LENGTHS)
        if fam == "equal":
            cov = np.full(total, 31.25) * (rng.random(total) > 0.1)
        elif fam == "two":
            cov = np.where(rng.random(total) < 0.5, 2.0, 3.0)                      # an even split puts the median between the two
            cov[:2], gc[:2] = (2.0, 3.0), 50                                       # segment (0, 2): exactly one of each
        elif fam == "wide":
            cov = _wide(rng, total)
            for k in range(8):                                                       # the deciding pass is each of the eight bytes
                cov[100 * k:100 * k + 9], gc[100 * k:100 * k + 9] = byte_ladder(k), 50
        elif fam == "low_byte":
            cov = (np.uint64(0x4037_0000_0000_0000) + rng.integers(0, 256, total).astype(np.uint64)).view(np.float64)
        elif fam == "dropped":                                                       # what `cov > 0` must drop
            cov = _wide(rng, total)
            r = rng.random(total)
            cov[r < 0.5] = -cov[r < 0.5]
            cov[r < 0.15] = -0.0
            cov[(r >= 0.5) & (r < 0.6)] = np.nan
            cov[(r >= 0.6) & (r < 0.65)] = 0.0
            cov[(r >= 0.65) & (r < 0.67)] = -np.nan
            cov[(r >= 0.67) & (r < 0.7)] = -np.finfo(np.float64).tiny / 4           # negative subnormals
        elif fam == "masked_segment":
            cov = np.round(rng.gamma(9.0, 3.3, total), 3)
        elif fam == "many_segments":                                                 # a GRCh38-shaped header: thousands of short contigs
            cov = np.round(rng.gamma(9.0, 3.3, total), 3) * (rng.random(total) > 0.1)
            lengths += [int(x) for x in rng.integers(0, 40, 3400)]
        seg = _segments(lengths, total, rng)
        if fam == "wide":
            seg = np.concatenate([np.array([(100 * k, 100 * k + 9) for k in range(8)], dtype=np.int64), seg])
        if fam == "two":
            seg = np.concatenate([np.array([(0, 2)], dtype=np.int64), seg])
        if fam == "masked_segment":
            lo, hi = seg[5]                                                          # gc == -1 on the whole 2048-segment
            gc[lo:hi] = -1
        out.append((fam, np.ascontiguousarray(cov, dtype=np.float64), gc, np.ascontiguousarray(seg)))
    return out


def median_reference(cov, gc, seg_off):
    """per segment (numpy.median of { cov[i] : cov[i] > 0 and gc[i] != -1 } or nan, how many were selected)
    (determine_ploidy, tiddit_coverage_analysis.pyx:14-27)"""
    med, cnt = [], []
    for lo, hi in seg_off:
        c, g = cov[lo:hi], gc[lo:hi]
        with np.errstate(invalid="ignore"):
            sel = c[(c > 0) & (g != -1)]
        cnt.append(len(sel))
        med.append(np.median(sel) if len(sel) else np.nan)
    return np.array(med), np.array(cnt, dtype=np.int64)


def median_parts(cov, gc, cuts):
    """the data cut at `cuts` into consecutive parts [(cov, gc)] (what tdt_masked_medians_parts takes), and the segments they are"""
    edges = [0] + list(cuts) + [len(cov)]
    parts = [(cov[a:b], gc[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    seg = np.array([(a, b) for a, b in zip(edges[:-1], edges[1:])] + [(0, len(cov))], dtype=np.int64)
    return parts, seg
