"""`TIDDIT_STR` on the GPU: the kernel (csrc/tdt_str.hip) on every aimed case of tests/str_cases.py through both entries —
``tdt_str_push`` on host columns, and ``tdt_str_push_device`` on the batches a ``DeviceBamReader`` decodes from a small BAM written from
the case's records — against the case's claim and the map / string-matching restatement: the store read out by ``tdt_str_keys`` equals
the definition's keys as a multiset (``np.array_equal`` on the sorted ``(K1, K2)`` rows), ``tdt_str_finish`` its counter array and
``tdt_str_rows`` its four row columns, exactly; the handle's state, its refusals on poisoned outputs, and the switch end to end on a
generated reference of 20 kb with planted loci, every job a fresh child process under its own time limit (the first job that fails
ends the fixture: nothing more is started behind a crash, a time-out or a GPU error).

Every test of this file fails on the parent commit: the module, the symbols and the switch do not exist there."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import str_cases as D
from clip_align_cases import fasta_raw, other, seeded

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = []                       # the (case, entry) pairs that ran and passed
READER_OK = [c for c in D.CASES if c["reader_ok"]]


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _counter(case, ctx=None, capacity=None):
    from tiddit_amd import tiddit_str
    return tiddit_str.StrCounter(D.loci_of(case), case["F"], case["Q"], capacity=capacity or case["capacity"] or 1 << 12, ctx=ctx)


def _same(h, want, what):
    rows, counts, columns = want
    k1, k2 = h.keys()
    assert k1.dtype == k2.dtype == np.uint64 and len(k1) == len(k2)
    got = D.key_rows(list(zip(k1.tolist(), k2.tolist())))
    assert got.shape == rows.shape and np.array_equal(got, rows), (what, got.shape, rows.shape, got[:8].tolist(), rows[:8].tolist())
    c = h.finish()
    assert c.dtype == np.uint64 and c.shape == (D.SIZE,)
    assert np.array_equal(c, counts), (what, c.tolist(), counts.tolist())
    r = h.rows()
    assert [x.dtype for x in r] == [np.uint64, np.uint64, np.uint32, np.uint32]
    for name, x, y in zip(("K1", "K2", "SUPPORT", "REV"), r, columns):
        assert x.shape == y.shape and np.array_equal(x, y), (what, name, x[:8].tolist(), y[:8].tolist())


@pytest.fixture(scope="module")
def wanted():
    out = {}
    for c in D.CASES:
        claim, ref = D.expected(c), D.reference(c)
        assert D.same(claim, ref), c["name"]
        out[c["name"]] = ref
    return out


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_push_equals_the_reference(case, wanted):
    h = _counter(case)
    try:
        for b in D.batches(case):
            h.push_host_batch(b)
        _same(h, wanted[case["name"]], case["name"])
        if "grows" in case:                                     # (the store grew where the case says it does)
            asks, grows, cap = h.reserve_stats()
            assert (asks, grows) == (case["asks"], case["grows"]) and cap > case["capacity"]
    finally:
        h.close()
    PAIRS.append((case["name"], "push"))


def _write_bam(path, case):
    from tiddit_amd import bamio
    b = D.build(case)
    w = bamio.BamWriter(path, list(zip(D.NAMES, D.LENGTHS)))
    w._buf += b.raw.tobytes()                     # the case's records as they are
    w.close()


@pytest.mark.parametrize("case", READER_OK, ids=[c["name"] for c in READER_OK])
def test_push_device_from_a_small_bam_equals_the_reference(case, wanted, tmp_path):
    from tiddit_amd import bamio
    assert case["repeat"] == 1
    path = str(tmp_path / "case.bam")
    _write_bam(path, case)
    rd = bamio.DeviceBamReader(path)
    h = None
    try:
        h = _counter(case, ctx=rd.ctx)
        n = 0
        for b in rd.batches():
            h.push_device_batch(b)
            n += len(b)
        assert n == len(case["reads"])
        _same(h, wanted[case["name"]], case["name"])
    finally:
        if h is not None:
            h.close()
        rd.close()
    PAIRS.append((case["name"], "push_device"))


def test_the_stated_count_of_case_entry_pairs_ran():
    assert len(D.CASES) == D.N_CASES == 30 and len(READER_OK) == 25
    assert len(set(PAIRS)) == 30 + 25, len(set(PAIRS))


def _case(name):
    return next(c for c in D.CASES if c["name"] == name)


def test_state_accumulates_between_pushes_resets_keeps_handles_apart_and_finishes_again(wanted):
    case = _case("merge state two pushes and a repeat")
    other_case = _case("merge shape a batch of 65 reads")
    first, second, third, fourth = D.batches(case)
    h, g = _counter(case), _counter(other_case, capacity=64)
    try:
        assert h.ctx is g.ctx
        assert not h.finish().any() and len(h.keys()[0]) == 0 and len(h.rows()[0]) == 0
        h.push_host_batch(first)
        g.push_host_batch(D.build(other_case))
        part = h.finish()
        assert part[D.SN.index("records")] == len(first) == 1 and part[D.SN.index("span_keys")] == 1 and len(h.rows()[0]) == 1
        for b in (second, third, fourth):
            h.push_host_batch(b)
        _same(h, wanted[case["name"]], "all pushes")
        _same(h, wanted[case["name"]], "the finish again")                       # (the store is left as it was)
        _same(g, wanted[other_case["name"]], "the other handle")
        h.reset()
        assert not h.finish().any() and len(h.keys()[0]) == 0 and len(h.rows()[0]) == 0
        _same(g, wanted[other_case["name"]], "the other handle after the reset")
        for b in (fourth, second, first, third):
            h.push_host_batch(b)
        _same(h, wanted[case["name"]], "after the reset, in another order")
    finally:
        h.close()
        g.close()


def test_refused_arguments_leave_the_outputs_untouched():
    from tiddit_amd import _native
    case = _case("merge equal keys on both strands are one set")
    ctx = _native.default_context()
    lib, P = ctx.lib, _native.ptr
    assert lib.tdt_str_sn_size() == D.SIZE
    t = D.loci_of(_case("table two to five loci in one read: the cap of four and over_cap; neighbours one base apart; loci at contig ends"))
    ls, le, mo, off = t.lstart.copy(), t.lend.copy(), t.motif.copy(), t.loc_off.copy()
    h = ctypes.c_void_p(0x5a5a)

    def create(ls_=ls, le_=le, mo_=mo, off_=off, nc=3, flank=5, q=20, cap=64, ctx_=ctx.handle, out=h):
        return lib.tdt_str_create(ctx_, P(ls_), P(le_), P(mo_), P(off_), nc, flank, q, cap, ctypes.byref(out) if out is not None else None)
    assert create(ctx_=None) == -1 and create(out=None) == -1 and create(nc=-1) == -1 and create(off_=None) == -1
    assert create(off_=off + 1) == -1                                                              # loc_off[0] != 0
    assert create(off_=np.array([0, 5, 4, 7], dtype=np.int64)) == -1                               # offsets that decrease
    assert create(ls_=None) == -1 and create(le_=None) == -1 and create(mo_=None) == -1
    for k, v in ((1, 1006), (0, 0)):                                                               # a start at the end in front; a start of 0
        bad = ls.copy()
        bad[k] = v
        assert create(ls_=bad) == -1
    bad = le.copy()
    bad[2] = ls[2]                                                                                 # an empty locus
    assert create(le_=bad) == -1
    for w in (0x120, 0x4127, 0x3123, 0x14123, 0x4023):                                             # m = 0, m = 7, a code that is no base, a code behind the last, no code
        bad = mo.copy()
        bad[3] = w
        assert create(mo_=bad) == -1
    assert create(flank=0) == -3 and create(flank=101) == -3 and create(q=-1) == -3 and create(q=256) == -3
    assert create(nc=(1 << 24) + 1) == -3 and create(cap=1 << 40) == -3
    big = np.array([0, (1 << 24) + 1], dtype=np.int64)
    assert create(off_=big, nc=1) == -3 and h.value == 0x5a5a                                       # more than 2^24 loci
    none = np.zeros(4, dtype=np.int64)
    g = ctypes.c_void_p()
    assert lib.tdt_str_create(ctx.handle, None, None, None, P(none), 3, 100, 255, 0, ctypes.byref(g)) == 0     # (no locus, no store yet)
    assert lib.tdt_str_destroy(g) == 0
    assert create() == 0 and h.value != 0x5a5a
    assert lib.tdt_str_destroy(h) == 0
    std = D.loci_of(case)
    h = ctypes.c_void_p()
    assert lib.tdt_str_create(ctx.handle, P(std.lstart), P(std.lend), P(std.motif), P(std.loc_off), 3, 5, 20, 64, ctypes.byref(h)) == 0
    try:
        b = D.build(case)
        cols = [getattr(b, k) for k in D.COLUMNS]
        n = len(b)

        def push(hh, c, nn, raw, raw_len):
            return lib.tdt_str_push(hh, *[P(x) if x is not None else None for x in c], nn, P(raw) if raw is not None else None, raw_len)
        assert push(None, cols, n, b.raw, len(b.raw)) == -1
        for k in range(6):
            assert push(h, cols[:k] + [None] + cols[k + 1:], n, b.raw, len(b.raw)) == -1
        assert push(h, cols, n, None, len(b.raw)) == -1
        assert push(h, cols, 1 << 31, b.raw, len(b.raw)) == -1
        assert push(h, cols[:5] + [np.ascontiguousarray(b.rec_off[::-1])], n, b.raw, len(b.raw)) == -1           # offsets that decrease
        assert lib.tdt_str_push_device(None, None, 0, 0) == -1
        assert lib.tdt_str_push_device(h, None, 5, 100) == -1
        nulls = (ctypes.c_void_p * 14)()
        assert lib.tdt_str_push_device(h, nulls, 5, 100) == -1                                     # a batch without its columns (the batch view)
        assert lib.tdt_str_push_device(h, nulls, 1 << 31, 100) == -1
        out = np.full(D.SIZE, 7, dtype=np.uint64)
        nr = ctypes.c_size_t(77)
        assert lib.tdt_str_finish(None, P(out), ctypes.byref(nr)) == -1 and lib.tdt_str_finish(h, None, ctypes.byref(nr)) == -1
        assert lib.tdt_str_finish(h, P(out), None) == -1
        assert (out == 7).all() and nr.value == 77
        ms = np.full(4, 7.0)
        assert lib.tdt_str_timing(None, P(ms)) == -1 and lib.tdt_str_timing(h, None) == -1 and (ms == 7).all()
        st = np.full(3, 7, dtype=np.uint64)
        assert lib.tdt_str_reserve_stats(None, P(st)) == -1 and lib.tdt_str_reserve_stats(h, None) == -1 and (st == 7).all()
        assert lib.tdt_str_reset(None) == -1
        cnt = ctypes.c_size_t(77)
        k1, k2 = np.full(16, 7, dtype=np.uint64), np.full(16, 7, dtype=np.uint64)
        sup, rev = np.full(16, 7, dtype=np.uint32), np.full(16, 7, dtype=np.uint32)
        assert lib.tdt_str_keys(None, P(k1), P(k2), ctypes.byref(cnt)) == -1 and lib.tdt_str_keys(h, P(k1), P(k2), None) == -1
        assert lib.tdt_str_keys(h, P(k1), None, ctypes.byref(cnt)) == -1 and cnt.value == 77
        assert lib.tdt_str_rows(None, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -1 and lib.tdt_str_rows(h, P(k1), P(k2), P(sup), P(rev), None) == -1
        assert lib.tdt_str_rows(h, P(k1), P(k2), None, P(rev), ctypes.byref(cnt)) == -1
        assert lib.tdt_str_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -1 and cnt.value == 77            # no finish yet
        # nothing refused above stored anything; n = 0 is a no-op; and the handle still works
        assert push(h, [None] * 6, 0, None, 0) == 0 and lib.tdt_str_push_device(h, None, 0, 0) == 0
        assert lib.tdt_str_finish(h, P(out), ctypes.byref(nr)) == 0 and not out.any() and nr.value == 0
        assert lib.tdt_str_keys(h, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 0
        assert push(h, cols, n, b.raw, len(b.raw)) == 0
        cnt = ctypes.c_size_t(16)
        assert lib.tdt_str_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -1 and cnt.value == 16            # a push since the finish
        want_keys, want_counts, want_cols = D.expected(case)
        assert lib.tdt_str_finish(h, P(out), ctypes.byref(nr)) == 0 and nr.value == 2
        assert np.array_equal(out, want_counts)
        cnt = ctypes.c_size_t(6)                                                                   # room for 6 of the 7 keys: refused, nothing written
        assert lib.tdt_str_keys(h, P(k1), P(k2), ctypes.byref(cnt)) == -3 and cnt.value == 6 and (k1 == 7).all() and (k2 == 7).all()
        cnt = ctypes.c_size_t(1)                                                                   # room for 1 of the 2 rows: the same
        assert lib.tdt_str_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -3 and cnt.value == 1
        assert (k1 == 7).all() and (k2 == 7).all() and (sup == 7).all() and (rev == 7).all()
        cnt = ctypes.c_size_t(0)
        assert lib.tdt_str_rows(h, None, None, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 2                      # the count alone
        cnt = ctypes.c_size_t(16)
        assert lib.tdt_str_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == 0 and cnt.value == 2 and (k1[2:] == 7).all() and (rev[2:] == 7).all()
        assert all(np.array_equal(x[:2], y) for x, y in zip((k1, k2, sup, rev), want_cols))
        assert sup[:2].tolist() == [6, 1] and rev[:2].tolist() == [3, 0]
        cnt = ctypes.c_size_t(16)
        assert lib.tdt_str_keys(h, P(k1), P(k2), ctypes.byref(cnt)) == 0 and cnt.value == 7 and (k1[7:] == 7).all()
        assert np.array_equal(D.key_rows(list(zip(k1[:7].tolist(), k2[:7].tolist()))), want_keys)
        # a raw_len of 0: every read with a locus in reach is malformed, nothing is read; the column counters still count
        assert lib.tdt_str_reset(h) == 0 and push(h, cols, n, None, 0) == 0
        assert lib.tdt_str_finish(h, P(out), ctypes.byref(nr)) == 0 and nr.value == 0
        assert np.array_equal(out, D.counters_of({"records": 7, "eligible": 7, "in_reach": 7, "malformed": 7}))
    finally:
        assert lib.tdt_str_destroy(h) == 0 and lib.tdt_str_destroy(None) == 0


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------
READ, LEN = 100, 20000
CUTS = "5:5:20"
# the planted loci: (start, motif, units in the reference, what the sample carries)
HOM, PLUS, MINUS, EXP, LOW = (2000, "CAG", 6), (5000, "AC", 8), (8000, "AAACG", 5), (11000, "CAG", 5), (14000, "AG", 6)
EXP_UNITS = 60                                   # 180 bases: longer than a read


def _genome():
    g = list(seeded(LEN, 4711))
    for s, motif, units in (HOM, PLUS, MINUS, EXP, LOW):
        g[s:s + len(motif) * units] = motif * units
        g[s - 1] = other(motif[-1]) if other(motif[-1]) != motif[0] else other(other(motif[-1]))      # (neither neighbour base continues the repeat)
        e = s + len(motif) * units
        g[e] = other(motif[0]) if other(motif[0]) != motif[-1] else other(other(motif[0]))
    return "".join(g)


def _sample_reads(g):
    """100-bp reads of the reference haplotype every 10 bases (two reads only over the low-coverage locus), and of the second haplotype
    at the three loci where it differs: spanning reads with the inserted or deleted units directly behind the left anchor, as an aligner
    that left-aligns places them, and for the expansion the reads that run into it from either side and are clipped at the locus's far end"""
    reads = []
    rd = lambda pos, cigar, seq: reads.append(D.R(cigar, pos, seq, flag=D.REV * ((pos // 10) % 2)))
    ls, le = LOW[0], LOW[0] + len(LOW[1]) * LOW[2]
    for p in range(0, LEN - READ, 10):
        if p + READ >= ls - 1 and p <= le + 1 and p not in (ls - 50, ls - 40):
            continue
        rd(p, "%dM" % READ, g[p:p + READ])
    s, motif, units = PLUS
    for x in range(10, 70, 10):                                                   # x reference bases, then the three extra units
        rd(s - x, "%dM6I%dM" % (x, READ - x - 6), g[s - x:s] + motif * 3 + g[s:s + READ - x - 6])
    s, motif, units = MINUS
    for x in range(10, 70, 10):                                                   # two units fewer
        rd(s - x, "%dM10D%dM" % (x, READ - x), g[s - x:s] + g[s + 10:s + 10 + READ - x])
    s, motif, units = EXP
    e = s + len(motif) * units
    for x in range(10, 80, 10):
        rd(s - x, "%dM%dS" % (x + e - s, READ - x - (e - s)), g[s - x:s] + (motif * EXP_UNITS)[:READ - x])
        rd(s, "%dS%dM" % (READ - x - (e - s), e - s + x), (motif * EXP_UNITS)[-(READ - x):] + g[e:e + x])
    return sorted(reads, key=lambda r: r["pos"])


def _loci_text():
    rows = ["# planted loci", "track name=planted"]
    for name, (s, motif, units) in zip(("hom", "plus3", "minus2", "expansion", "low"), (HOM, PLUS, MINUS, EXP, LOW)):
        rows.append("chrS\t%d\t%d\t%s\t%s" % (s, s + len(motif) * units, motif if name != "plus3" else motif.lower(), name))
    rows.append("chrX\t10\t20\tA\tnot in the header")
    return "\n".join(rows) + "\n"


def _job(bam, fa, out, timeout=300, **env):
    e = {k: v for k, v in os.environ.items() if not (k.startswith("TIDDIT_") and k != "TIDDIT_HIP_LIB") and k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env)
    argv = [sys.executable, "-m", "tiddit_amd", "--sv", "--bam", bam, "--ref", fa, "-o", out, "--skip_assembly"]
    return subprocess.run(argv, cwd=REPO, env=e, capture_output=True, text=True, timeout=timeout)


def _ok(r):
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r


def _files(prefix):
    d, base = os.path.split(prefix)
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            rel = os.path.relpath(p, d)
            if rel.startswith(base + ".") or rel.startswith(base + "_tiddit"):
                data = open(p, "rb").read()
                if p.endswith(".vcf"):                                        # (its ##TIDDITcmd= line names the job's own prefix)
                    data = b"\n".join(l for l in data.split(b"\n") if not l.startswith(b"##TIDDITcmd="))
                out[rel[len(base):]] = hashlib.sha256(data).hexdigest()
    return out


def write_sample(d):
    """the generated reference as a FASTA, the sample's reads as a sorted BAM, the loci file -> (bam, fa, loci path)"""
    from tiddit_amd import bamio
    g = _genome()
    fa, bam, bed = os.path.join(d, "ref.fa"), os.path.join(d, "sample.bam"), os.path.join(d, "loci.bed")
    open(fa, "wb").write(b">chrS\n" + fasta_raw(g) + b"\n")
    w = bamio.BamWriter(bam, [("chrS", LEN)])
    w._buf += D.build_reads(_sample_reads(g)).raw.tobytes()
    w.close()
    open(bed, "w").write(_loci_text())
    return bam, fa, bed


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """(each job is checked before the next one is started: a crash, a time-out or a GPU error ends the fixture there)"""
    d = str(tmp_path_factory.mktemp("str"))
    bam, fa, bed = write_sample(d)
    paths = {n: os.path.join(d, n) for n in ("off", "on", "host", "ranks", "bad", "cuts")}
    _ok(_job(bam, fa, paths["off"]))
    r = _ok(_job(bam, fa, paths["on"], TIDDIT_STR=bed, TIDDIT_STR_CUTS=CUTS))
    _ok(_job(bam, fa, paths["host"], TIDDIT_STR=bed, TIDDIT_STR_CUTS=CUTS, TIDDIT_HOST_INGEST="1"))
    return bam, fa, bed, paths, r


def definitions_file(bam, bed, path, cuts=(5, 5, 20)):
    """the definition over the host reader's batches, written through the module's own writer -> (counts, loci, table)"""
    from tiddit_amd import bamio, tiddit_str
    rd = bamio.BamReader(bam)
    loci = tiddit_str.read_loci(bed, list(rd.references), list(rd.lengths))
    sn, keys = {}, []
    for b in rd.batches():
        tiddit_str.keys_of_batch(b, loci, keys, sn, cuts[0], cuts[2])
    rd.close()
    counts = tiddit_str.counts_of(sn)
    table = tiddit_str.summarise(loci, tiddit_str.rows_of_keys(keys), cuts[1])
    tiddit_str.write_file(path, loci, counts, table, *cuts)
    return counts, loci, table


def test_the_file_equals_the_definitions_file_and_names_the_planted_genotypes(jobs, tmp_path):
    from tiddit_amd import tiddit_str
    bam, fa, bed, paths, r = jobs
    want = str(tmp_path / "want.str.tab")
    counts, loci, table = definitions_file(bam, bed, want)
    got = open(paths["on"] + ".str.tab", "rb").read()
    assert len(got) > 500 and got == open(want, "rb").read()
    assert got.startswith(b"# tiddit_amd str v1 flank=5 min_reads=5 min_mapq=20\nSN\trecords\t")
    assert b"SN\tloci\t5\n" in got and b"SN\tskipped_contig\t1\n" in got and b"SN\tmalformed\t0\n" in got
    lines = [l.split("\t") for l in got.decode().split("\n") if l and not l.startswith(("#", "SN"))]
    # CHROM START END MOTIF ID REF_LEN | A1 A2 GT | LONGER, as the loci were planted (the counts beside them are the definition's, above)
    assert [l[:6] + [l[7], l[9], l[11], l[14]] for l in lines] == [
        ["chrS", "2000", "2018", "CAG", "hom", "18", "18", "18", "0/0", "0"],
        ["chrS", "5000", "5016", "AC", "plus3", "16", "16", "22", "0/1", "0"],
        ["chrS", "8000", "8025", "AAACG", "minus2", "25", "15", "25", "0/1", "0"],
        ["chrS", "11000", "11015", "CAG", "expansion", "15", "15", "15", "0/0", "1"],
        ["chrS", "14000", "14012", "AG", "low", "12", ".", ".", ".", "0"]]
    by_id = {l[4]: l for l in lines}
    assert by_id["low"][6] == "2" and by_id["low"][15] == "12:2"                     # two spanning reads: below S
    assert int(by_id["expansion"][13]) == 90 and int(by_id["expansion"][12]) >= 14   # FLANK_MAX: the longest open run, 100 - 10 bases
    assert by_id["plus3"][15].startswith("16:") and ",22:6" in by_id["plus3"][15] and by_id["minus2"][15].startswith("15:6,25:")
    assert [l for l in r.stdout.split("\n") if l.startswith("str:")] == [tiddit_str.summary_line(counts, loci, table)]


def test_host_ingest_writes_the_same_bytes(jobs):
    bam, fa, bed, paths, r = jobs
    assert open(paths["host"] + ".str.tab", "rb").read() == open(paths["on"] + ".str.tab", "rb").read()


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    bam, fa, bed, paths, r = jobs
    off, on, host = (_files(paths[k]) for k in ("off", "on", "host"))
    assert set(on) - set(off) == {".str.tab"} and set(off) <= set(on) and len(off) >= 5
    assert all(on[k] == off[k] for k in off), [k for k in off if on[k] != off[k]]
    assert not os.path.exists(paths["off"] + ".str.tab") and ".str.tab" in host


def test_malformed_switch_values_are_errors(jobs):
    bam, fa, bed, paths, r = jobs
    bad = _job(bam, fa, paths["bad"], timeout=120, TIDDIT_STR=bed, TIDDIT_STR_CUTS="5:5:300")
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == ["error, TIDDIT_STR_CUTS=5:5:300: the minimum MAPQ is 0 ... 255"]
    alone = _job(bam, fa, paths["cuts"], timeout=120, TIDDIT_STR_CUTS="5")
    assert alone.returncode == 1
    assert [l for l in alone.stdout.split("\n") if l.startswith("error")] == [
        "error, TIDDIT_STR_CUTS=5: the cuts are those of TIDDIT_STR=loci.bed: TIDDIT_STR not set"]
    gone = _job(bam, fa, paths["bad"], timeout=120, TIDDIT_STR=bed + ".none")
    assert gone.returncode == 1 and [l for l in gone.stdout.split("\n") if l.startswith("error")][0].startswith("error, TIDDIT_STR=" + bed + ".none: ")
    for k in ("bad", "cuts"):
        assert not os.path.exists(paths[k] + "_tiddit") and not os.path.exists(paths[k] + ".str.tab")


def test_n_ranks_refuse_the_switch_and_write_nothing(jobs):
    """every rank ends with the refusal before the first collective (no process group is ever made) and no file is written"""
    bam, fa, bed, paths, r = jobs
    res = _job(bam, fa, paths["ranks"], timeout=120, TIDDIT_STR=bed, RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29547",
               TIDDIT_DIST_BACKEND="gloo", TIDDIT_FORCE_DIST="1")
    assert res.returncode == 1, (res.returncode, res.stdout[-1000:], res.stderr[-2000:])
    errors = [l for l in res.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_STR is a one-process switch")
    assert not os.path.exists(paths["ranks"] + "_tiddit") and not os.path.exists(paths["ranks"] + ".str.tab")
