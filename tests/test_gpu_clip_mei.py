"""`TIDDIT_CLIPS_MEI` on the GPU: the alignment kernel (csrc/tdt_swalign.hip) on every case of tests/clip_mei_cases.py through
``tdt_sw_align`` and ``tdt_sw_align_device`` — the nine result columns and the counters equal the definition's, exactly, and the
literal claims; the 500 generated queries; the handle path (``tdt_clip_mei`` / ``tdt_clip_mei_rows`` / ``tdt_clip_mei_timing``) from pushed
batches, where the query table is built on the device from the pair rows; the C-ABI refusals with poisoned outputs; and the switch end
to end on a generated reference of two contigs and 20 kb with insertions cut from a library of three families, every job a fresh child
process under its own time limit (the first job that fails ends the fixture: nothing more is started behind a crash, a time-out or a
GPU error).

Every test of this file fails on the parent commit: the module, the symbols and the switch do not exist there."""
import ctypes
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import clip_cases as D
import clip_ins_cases as C
import clip_mei_cases as X

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = []                       # the (case, entry) pairs that ran and passed
N_CONTIGS = 1 << 24


@pytest.fixture(scope="module")
def ctx():
    from tiddit_amd import _native
    return _native.default_context()


def _library(ctx, library):
    """a family library as the job loads it: a handle of its own, every sequence packed from its FASTA bytes"""
    from tiddit_amd import refseq
    lib = refseq.RefSeq([len(t) for _, t in library], ctx=ctx)
    for tid, (_, t) in enumerate(library):
        lib.load_fasta(tid, np.frombuffer(X.fasta_raw(t), dtype=np.uint8), len(t), min(len(t), 60), min(len(t), 60) + 1)
    return lib


@functools.lru_cache(maxsize=None)
def _definition(k):
    c = X.CASES[k] if k >= 0 else X.random_case()
    return (c,) + X.definition(c)


def _entry(ctx, k, device):
    from tiddit_amd import tiddit_clip_mei as M
    c, res, counts, calls = _definition(k)
    assert X.agrees_with_claim(c, res, counts, calls) is None, c["name"]
    lib = _library(ctx, c["library"])
    try:
        sn, cols = M.sw_align(*M.query_columns(X.query_codes(c)), lib, c["A"], ctx=ctx, device=device)
    finally:
        lib.close()
    want = list(zip(*res))
    for name, x, y in zip(("FAMILY", "STRAND", "SCORE", "QSTART", "QEND", "FSTART", "FEND", "SECOND", "SECOND_FAMILY"), cols, want):
        assert x.dtype == np.uint32 and x.tolist() == list(y), (c["name"], name, [(i, a, b) for i, (a, b) in enumerate(zip(x.tolist(), y)) if a != b][:6])
    assert X.agrees_with_claim(c, list(zip(*[x.tolist() for x in cols]))) is None
    if c["parts"] is None:                                       # (the plain entries take every query as a closed pair of its own)
        assert sn.dtype == np.uint64 and np.array_equal(sn, counts), (c["name"], sn.tolist(), counts.tolist())
    else:
        plain, _ = M.summarise(res, [X.SEQ] * len(res), c["A"])
        assert np.array_equal(sn, plain), (c["name"], sn.tolist(), plain.tolist())


@pytest.mark.parametrize("entry", ["sw_align", "sw_align_device"])
@pytest.mark.parametrize("k", range(X.N_AIMED), ids=[c["name"] for c in X.CASES])
def test_both_entries_equal_the_definition_and_the_claim(k, entry, ctx):
    _entry(ctx, k, entry == "sw_align_device")
    PAIRS.append((k, entry))


def test_the_stated_count_of_case_entry_pairs_ran():
    assert X.N_AIMED == 59 and len(set(PAIRS)) == 2 * 59, len(set(PAIRS))


@pytest.mark.parametrize("entry", ["sw_align", "sw_align_device"])
def test_the_500_generated_queries(entry, ctx):
    _entry(ctx, -1, entry == "sw_align_device")


def test_no_query_and_the_counters_alone(ctx):
    from tiddit_amd import _native, tiddit_clip_mei as M
    c = X.CASES[0]
    lib = _library(ctx, c["library"])
    try:
        sn, cols = M.sw_align(np.zeros((0, 10), dtype=np.uint64), np.zeros(0, dtype=np.uint32), lib, ctx=ctx)
        assert not sn.any() and all(len(x) == 0 for x in cols)
        seq10, qlen = M.query_columns(X.query_codes(c))
        sn = np.full(M.SIZE, 7, dtype=np.uint64)
        P = _native.ptr
        assert ctx.lib.tdt_sw_align(ctx.handle, lib.handle, 1, P(seq10), P(qlen), 30, P(sn), *[None] * 9) == 0
        assert sn.tolist() == [1, 1, 0, 0, 1, 0, 0, 0, 1, 0]
    finally:
        lib.close()


# ---- the handle path -------------------------------------------------------------------------------------------------------------------
def test_the_handle_path_from_pushed_batches(ctx):
    """the job's reads pushed as a host batch: the pair rows of tdt_clip_ins become queries on the device (four CLOSED pairs of 130 and
    250 bases on either strand, one that names nothing, an OPEN pair's two flanks), and every column is the definition's"""
    from tiddit_amd import tiddit_clip_ins as I, tiddit_clip_mei as M, tiddit_clips
    b = D.build_batch(X.job_reads(X.job_genome()))
    h = tiddit_clips.ClipCounter(N_CONTIGS, C.JOB_Q, C.JOB_L, capacity=1 << 12, ctx=ctx)
    lib = _library(ctx, X.JOB_LIBRARY)
    try:
        h.enable_ext(1 << 12)
        h.push_host_batch(b)
        h.finish(C.JOB_S)
        rows = h.rows()
        h.ins(C.JOB_K, C.JOB_O, C.JOB_M)
        eclen, cons5 = h.ext_rows()
        cols, seq10 = h.ins_rows()
        ins_rows = I.file_rows(rows[0], rows[2], eclen, cons5, cols, seq10)
        assert [(r[0], r[1], r[8]) for r in ins_rows] == [(t, P, int(len(s) <= 268)) for t, P, _, s, _ in X.JOB_PLANTED]
        qs = M.queries_of_rows(ins_rows)
        assert [(p, pt, len(t)) for p, pt, t in qs] == [(0, 0, 130), (1, 0, 130), (2, 0, 250), (3, 0, 250), (4, 0, 250), (5, 1, 140), (5, 2, 140)]
        res = M.results([M.codes_of_text(t) for _, _, t in qs], [np.asarray(x) for x in X.library_codes({"library": X.JOB_LIBRARY})])
        counts, calls = M.summarise(res, [pt for _, pt, _ in qs], X.JOB_A, [p for p, _, _ in qs])
        sn = h.mei(lib, X.JOB_A)
        assert sn.dtype == np.uint64 and np.array_equal(sn, counts), (sn.tolist(), counts.tolist())
        assert sn.tolist() == [7, 5, 1, 1, 6, 1, 2, 0, 5, 0]
        pair, part, qlen, got = h.mei_rows()
        assert pair.tolist() == [p for p, _, _ in qs] and part.tolist() == [pt for _, pt, _ in qs] and qlen.tolist() == [len(t) for _, _, t in qs]
        assert [tuple(int(v) for v in r) for r in zip(*got)] == [tuple(int(v) for v in r) for r in res]
        names = [n for n, _ in X.JOB_LIBRARY]
        assert [(names[r[0]], "+-"[r[1]], r[5], r[6]) if r[2] >= X.JOB_A else None for r in res[:6]] == [w for _, _, _, _, w in X.JOB_PLANTED[:5]] + [("L1X", "+", 101, 240)]
        assert calls[5] == (1, 0, 140, 101, 700)
        assert (h.mei_timing() >= 0).all() and h.mei_timing()[1] > 0
        # another minimum on the same rows: the columns stay, the counters move
        assert h.mei(lib, 251).tolist() == [7, 5, 1, 1, 0, 7, 0, 0, 0, 0]
        h.finish(C.JOB_S)
        with pytest.raises(Exception):
            h.mei(lib, X.JOB_A)                                  # a finish since the tdt_clip_ins
    finally:
        h.close()
        lib.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_outputs_untouched(ctx):
    from tiddit_amd import _native, refseq, tiddit_clip_mei as M
    lib_, P = ctx.lib, _native.ptr
    c = next(x for x in X.CASES if x["name"].startswith("named: a score of exactly"))
    lib = _library(ctx, c["library"])
    seq10, qlen = M.query_columns(X.query_codes(c))
    n = len(qlen)
    sn = np.full(M.SIZE, 7, dtype=np.uint64)
    outs = [np.full(4, 7, dtype=np.uint32) for _ in range(9)]
    untouched = lambda: (sn == 7).all() and all((o == 7).all() for o in outs)
    unloaded = refseq.RefSeq([10, 10], ctx=ctx)
    unloaded.load_fasta(0, np.frombuffer(b"ACGTACGTAC", dtype=np.uint8), 10, 10, 11)
    big = refseq.RefSeq([1 << 19, (1 << 19) + 1], ctx=ctx)
    long_ = refseq.RefSeq([(1 << 20) + 1], ctx=ctx)
    many = refseq.RefSeq([1] * 4097, ctx=ctx)
    none = refseq.RefSeq([], ctx=ctx)
    zero = refseq.RefSeq([0], ctx=ctx)

    def align(cx=ctx.handle, l=lib.handle, nn=n, s10=seq10, ql=qlen, A=30, s=sn, o=outs):
        return lib_.tdt_sw_align(cx, l, nn, P(s10) if s10 is not None else None, P(ql) if ql is not None else None, A, P(s) if s is not None else None,
                                 *[P(a) if a is not None else None for a in o])
    try:
        assert align(cx=None) == -1 and align(l=None) == -1 and align(s10=None) == -1 and align(ql=None) == -1 and align(s=None) == -1
        for k in range(9):
            assert align(o=[None if j == k else a for j, a in enumerate(outs)]) == -1                # some but not all output arrays
        assert align(l=unloaded.handle) == -1                                                        # a sequence that is not loaded
        for A in (11, 281, 0, -30):
            assert align(A=A) == -3, A
        for ql in ([0, 30], [29, 281]):
            assert align(ql=np.array(ql, dtype=np.uint32)) == -3, ql
        bad = seq10.copy()
        bad[1, 1] = 1 << 4                                                                           # base 30 of a query of 30: word 1, column 2
        assert align(s10=bad) == -3
        bad = seq10.copy()
        bad[0, 0] |= np.uint64(1) << np.uint64(58)                                                   # a bit above the 56 of a word
        assert align(s10=bad) == -3
        bad = seq10.copy()
        bad[0, 1] = 1 << 2                                                                           # base 29 of a query of 29
        assert align(s10=bad) == -3
        for l in (big, long_, many, none, zero):
            assert align(l=l.handle) == -3
        assert align(nn=1 << 31) == -3                                                              # 2^31 problems or more
        assert untouched()
        assert align() == 0 and sn.tolist() == [2, 2, 0, 0, 1, 1, 0, 0, 1, 0] and outs[2][:2].tolist() == [29, 30] and all((o[2:] == 7).all() for o in outs)
        # the device entry: null pointers and ranges (its arrays are never touched by a refused call: nothing is launched)
        dev = lambda *a: lib_.tdt_sw_align_device(*a)
        one = ctypes.c_void_p(256)
        assert dev(None, lib.handle, 1, one, one, 30, one, *[None] * 9) == -1 and dev(ctx.handle, None, 1, one, one, 30, one, *[None] * 9) == -1
        assert dev(ctx.handle, lib.handle, 1, None, one, 30, one, *[None] * 9) == -1 and dev(ctx.handle, lib.handle, 1, one, None, 30, one, *[None] * 9) == -1
        assert dev(ctx.handle, lib.handle, 1, one, one, 30, None, *[None] * 9) == -1 and dev(ctx.handle, lib.handle, 1, one, one, 30, one, one, *[None] * 8) == -1
        assert dev(ctx.handle, lib.handle, 1, one, one, 11, one, *[None] * 9) == -3 and dev(ctx.handle, many.handle, 1, one, one, 30, one, *[None] * 9) == -3
        # ---- the handle
        h = ctypes.c_void_p()
        assert lib_.tdt_clip_create(ctx.handle, 8, 20, 10, 64, ctypes.byref(h)) == 0
        try:
            res, ms3, cnt = np.full(M.SIZE, 7, dtype=np.uint64), np.full(3, 7.0), ctypes.c_size_t(4)
            cols = [np.full(4, 7, dtype=np.uint32) for _ in range(12)]
            clean = lambda: (res == 7).all() and (ms3 == 7).all() and all((x == 7).all() for x in cols)
            assert lib_.tdt_clip_ext_enable(h, 64) == 0
            assert lib_.tdt_clip_mei(h, lib.handle, 30, P(res)) == -1                               # no finish, no tdt_clip_ins
            b = D.build_batch([D.rd(pos=100, trail=X.seeded(60, 1))] * 3 + [D.rd(pos=300, lead=X.seeded(60, 2))] * 3)
            assert lib_.tdt_clip_push(h, *[P(getattr(b, k)) for k in D.COLUMNS], len(b), P(b.raw), len(b.raw)) == 0
            c13, nr = np.zeros(13, dtype=np.uint64), ctypes.c_size_t()
            assert lib_.tdt_clip_finish(h, 3, P(c13), ctypes.byref(nr)) == 0 and nr.value == 2
            assert lib_.tdt_clip_mei(h, lib.handle, 30, P(res)) == -1                               # a finish, but no tdt_clip_ins
            ins = np.zeros(11, dtype=np.uint64)
            assert lib_.tdt_clip_ins(h, 20, 12, 1, P(ins)) == 0
            assert lib_.tdt_clip_mei_rows(h, *[P(x) for x in cols], ctypes.byref(cnt)) == -1 and lib_.tdt_clip_mei_timing(h, P(ms3)) == -1   # no tdt_clip_mei yet
            assert lib_.tdt_clip_mei(None, lib.handle, 30, P(res)) == -1 and lib_.tdt_clip_mei(h, None, 30, P(res)) == -1 and lib_.tdt_clip_mei(h, lib.handle, 30, None) == -1
            assert lib_.tdt_clip_mei(h, unloaded.handle, 30, P(res)) == -1
            assert lib_.tdt_clip_mei(h, lib.handle, 11, P(res)) == -3 and lib_.tdt_clip_mei(h, lib.handle, 281, P(res)) == -3 and lib_.tdt_clip_mei(h, many.handle, 30, P(res)) == -3
            assert clean()
            assert lib_.tdt_clip_mei(h, lib.handle, 30, P(res)) == 0 and not res.any()              # an R site at 120 and an L site at 301: no pair, no query
            assert lib_.tdt_clip_mei_rows(h, *[P(x) for x in cols[:5]], None, *[P(x) for x in cols[6:]], ctypes.byref(cnt)) == -1
            assert lib_.tdt_clip_mei_rows(None, *[P(x) for x in cols], ctypes.byref(cnt)) == -1 and lib_.tdt_clip_mei_rows(h, *[P(x) for x in cols], None) == -1
            assert lib_.tdt_clip_mei_rows(h, *[None] * 12, ctypes.byref(cnt)) == 0 and cnt.value == 0
            assert lib_.tdt_clip_mei_timing(h, None) == -1 and lib_.tdt_clip_mei_timing(None, P(ms3)) == -1
            assert all((x == 7).all() for x in cols) and (ms3 == 7).all()
            assert lib_.tdt_clip_mei_timing(h, P(ms3)) == 0 and (ms3 >= 0).all()
            assert lib_.tdt_clip_ins(h, 20, 12, 1, P(ins)) == 0
            assert lib_.tdt_clip_mei_rows(h, *[None] * 12, ctypes.byref(cnt)) == -1                 # a tdt_clip_ins since the tdt_clip_mei
        finally:
            assert lib_.tdt_clip_destroy(h) == 0
    finally:
        for l in (lib, unloaded, big, long_, many, none, zero):
            l.close()


def test_too_little_room_for_the_rows(ctx):
    from tiddit_amd import _native, tiddit_clips
    P = _native.ptr
    b = D.build_batch(X.job_reads(X.job_genome()))
    h = tiddit_clips.ClipCounter(N_CONTIGS, C.JOB_Q, C.JOB_L, capacity=1 << 12, ctx=ctx)
    lib = _library(ctx, X.JOB_LIBRARY)
    try:
        h.enable_ext(1 << 12)
        h.push_host_batch(b)
        h.finish(C.JOB_S)
        h.ins(C.JOB_K, C.JOB_O, C.JOB_M)
        h.mei(lib, 30)
        cols, cnt = [np.full(8, 7, dtype=np.uint32) for _ in range(12)], ctypes.c_size_t(6)
        assert ctx.lib.tdt_clip_mei_rows(h.handle, *[P(x) for x in cols], ctypes.byref(cnt)) == -3 and cnt.value == 6 and all((x == 7).all() for x in cols)
        cnt = ctypes.c_size_t(8)
        assert ctx.lib.tdt_clip_mei_rows(h.handle, *[P(x) for x in cols], ctypes.byref(cnt)) == 0 and cnt.value == 7 and all(x[7] == 7 for x in cols)
    finally:
        h.close()
        lib.close()


# ---- the switch, end to end -------------------------------------------------------------------------------------------------------------
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


THREE = {"TIDDIT_CLIPS": C.CLIPS, "TIDDIT_CLIPS_INS": C.INS, "TIDDIT_CLIPS_VCF": "10"}


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """the generated reference and the library as FASTA files, the sample's reads as a sorted BAM; two jobs, each checked before the
    next is started"""
    from tiddit_amd import bamio
    d = str(tmp_path_factory.mktemp("clip_mei"))
    g = X.job_genome()
    contigs = [("chrA", g[0].text()), ("chrB", g[1].text())]
    fa, bam, lib = os.path.join(d, "ref.fa"), os.path.join(d, "sample.bam"), os.path.join(d, "families.fa")
    open(fa, "wb").write(b"".join(b">" + n.encode() + b"\n" + X.fasta_raw(t) + b"\n" for n, t in contigs))
    X.write_library(lib)
    w = bamio.BamWriter(bam, [(n, len(t)) for n, t in contigs])
    w._buf += D.build_batch(X.job_reads(g)).raw.tobytes()
    w.close()
    paths = {n: os.path.join(d, n) for n in ("three", "mei", "bad")}
    _ok(_job(bam, fa, paths["three"], **THREE))
    r = _ok(_job(bam, fa, paths["mei"], TIDDIT_CLIPS_MEI=lib, TIDDIT_CLIPS_MEI_MIN=str(X.JOB_A), **THREE))
    return bam, fa, lib, contigs, paths, r


def _ins_rows(bam):
    from tiddit_amd import bamio, tiddit_clip_ins as I
    events, keys, sn = [], [], {}
    rd = bamio.BamReader(bam)
    for b in rd.batches():
        I.events_of_batch_by_read(b, events, keys, sn, C.JOB_Q, C.JOB_L)
    rd.close()
    _, sites, pairs = I.summarise(events, sn, C.JOB_S, C.JOB_K, C.JOB_O, C.JOB_M)
    k1, _, eclen, cons5 = I.site_columns(sites)
    cols, seq10 = I.pair_columns(pairs)
    return I.file_rows(k1, [s[2] for s in sites], eclen, cons5, cols, seq10)


def test_the_file_equals_the_definitions_file_and_names_the_planted_families(jobs, tmp_path):
    from tiddit_amd import tiddit_clip_mei as M
    bam, fa, lib, contigs, paths, r = jobs
    want = str(tmp_path / "want.clips.mei.tab")
    counts, _ = M.definition_file(want, _ins_rows(bam), [n for n, _ in contigs], lib, X.JOB_A)
    got = open(paths["mei"] + ".clips.mei.tab", "rb").read()
    assert got == open(want, "rb").read()
    assert got.startswith(b"# tiddit_amd clips_mei v1 match=1 mismatch=4 gap_open=6 gap_extend=1 other=1 min_score=30 families=3 bases=1700\nSN\tqueries\t7\n")
    table = [l.split("\t") for l in got.decode().split("\n") if l and not l.startswith(("#", "SN"))]
    # CHROM POS STATUS PART QLEN FAMILY STRAND SCORE QSTART QEND FSTART FEND, as the insertions were planted
    assert [[x[0], x[1], x[3], x[4], x[5]] + x[6:13] for x in table] == [
        ["chrA", "2000", "CLOSED", "SEQ", "130", "AluX", "+", "130", "1", "130", "51", "180"],
        ["chrA", "4000", "CLOSED", "SEQ", "130", "SvaX", "-", "130", "1", "130", "101", "230"],
        ["chrA", "6000", "CLOSED", "SEQ", "250", "L1X", "+", "250", "1", "250", "301", "550"],
        ["chrA", "8000", "CLOSED", "SEQ", "250", "L1X", "-", "250", "1", "250", "601", "850"],
        ["chrA", "10000", "CLOSED", "SEQ", "250"] + ["."] * 7,
        ["chrB", "3000", "OPEN", "LEFT", "140", "L1X", "+", "140", "1", "140", "101", "240"],
        ["chrB", "3000", "OPEN", "RIGHT", "140", "L1X", "+", "140", "1", "140", "561", "700"]]
    assert [l for l in r.stdout.split("\n") if l.startswith("clips mei:")] == [M.summary_line(counts)]


def test_the_vcf_gains_the_fields_on_exactly_the_planted_records(jobs):
    bam, fa, lib, contigs, paths, r = jobs
    a = open(paths["three"] + ".clips.vcf").read().split("\n")
    b = open(paths["mei"] + ".clips.vcf").read().split("\n")
    strip = lambda ls: [l for l in ls if not l.startswith("##TIDDITcmd=")]
    want = []
    planted = {("chr" + "AB"[t], str(P - tsd)): w for t, P, tsd, s, w in X.JOB_PLANTED}
    planted[("chrB", "3000")] = ("L1X", "+", 101, 700)
    scores = {("chrA", "2000"): 130, ("chrA", "3985"): 130, ("chrA", "6000"): 250, ("chrA", "7985"): 250, ("chrB", "3000"): 140}
    for l in strip(a):
        x = l.split("\t")
        if l.startswith("##FILTER=<ID=Ambiguous"):
            want += [m for m in strip(b) if m.startswith(("##INFO=<ID=MEI",))]
        if l.startswith("##clips_vcf_junctions="):
            want.append("##clips_vcf_mei_min_score=30")
        w = planted.get((x[0], x[1])) if len(x) > 7 and x[4] == "<INS>" else None
        if w is not None:
            x[7] += ";MEI=%s;MEISTRAND=%s;MEISCORE=%d;MEISPAN=%d,%d" % (w[0], w[1], scores[(x[0], x[1])], w[2], w[3])
            l = "\t".join(x)
        want.append(l)
    assert strip(b) == want
    assert sum("MEI=" in l for l in b) == 5 and sum(l.startswith("##INFO=<ID=MEI") for l in b) == 4 and sum("<INS>" in l and not l.startswith("#") for l in b) == 6


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    bam, fa, lib, contigs, paths, r = jobs
    without, with_mei = _files(paths["three"]), _files(paths["mei"])
    assert set(with_mei) - set(without) == {".clips.mei.tab"} and set(without) <= set(with_mei) and {".clips.tab", ".clips.ins.tab", ".clips.vcf"} <= set(without)
    assert not os.path.exists(paths["three"] + ".clips.mei.tab")
    assert [k for k in without if with_mei[k] != without[k]] == [".clips.vcf"]


@pytest.mark.parametrize("env,line", [
    ({"TIDDIT_CLIPS_INS": None}, "error, TIDDIT_CLIPS_MEI={lib}: the switch names the insertions of TIDDIT_CLIPS_INS, which is not set"),
    ({"TIDDIT_CLIPS_MEI": None, "TIDDIT_CLIPS_MEI_MIN": "30"}, "error, TIDDIT_CLIPS_MEI_MIN=30: the minimum score belongs to TIDDIT_CLIPS_MEI, which is not set"),
    ({"TIDDIT_CLIPS_MEI_MIN": "11"}, "error, TIDDIT_CLIPS_MEI={lib}: TIDDIT_CLIPS_MEI_MIN=11: the minimum score is 12 ... 280"),
    ({"TIDDIT_CLIPS_MEI": "{lib}.missing"}, "error, TIDDIT_CLIPS_MEI={lib}.missing: the library FASTA cannot be read")],
    ids=["without TIDDIT_CLIPS_INS", "the minimum alone", "11", "a missing file"])
def test_the_switch_without_its_partners_and_bad_values_are_errors(jobs, env, line):
    bam, fa, lib, contigs, paths, r = jobs
    e = dict({"TIDDIT_CLIPS": C.CLIPS, "TIDDIT_CLIPS_INS": C.INS, "TIDDIT_CLIPS_MEI": lib}, **{k: v if v is None else v.format(lib=lib) for k, v in env.items()})
    bad = _job(bam, fa, paths["bad"], timeout=120, **{k: v for k, v in e.items() if v is not None})
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == [line.format(lib=lib)]
    assert not os.path.exists(paths["bad"] + "_tiddit") and not any(os.path.exists(paths["bad"] + s) for s in (".clips.tab", ".clips.ins.tab", ".clips.mei.tab"))
