"""`TIDDIT_INDELS` on the GPU: the kernels (csrc/tdt_indel.hip) on every aimed case of tests/indel_cases.py through both entries —
``tdt_indel_push`` on host columns, and ``tdt_indel_push_device`` on the batches a ``DeviceBamReader`` decodes from a small BAM written
from the case's records — against the case's claim and the struct / regex / Counter restatement: the store read out by
``tdt_indel_keys`` equals the definition's keys as a multiset (``np.array_equal`` on the sorted ``(K1, K2)`` rows), and for every minimum
support the case states ``tdt_indel_finish`` equals the definition's counter array and ``tdt_indel_rows`` its four row columns, exactly;
the handle's state, its refusals, and the switch end to end on the sv_e2e_small fixture, every job a fresh child process under its own
time limit (the first job that fails ends the fixture: nothing more is started behind a crash, a time-out or a GPU error).

The fixture holds 604 338 records: the end to end test runs ``tiddit_indels.keys_of_batch`` — the definition behind a whole-column
filter, pinned to ``events_of_read`` on every aimed case by tests/test_indel_refs_cpu.py — over the host reader's batches.  The fixture's
planted ``dM dD dM`` reads make its table non-empty; it holds no insertion: what covers the sequence path are the aimed cases.

Every test of this file fails on the parent commit: the module, the symbols and the switch do not exist there."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import indel_cases as D
from sv_e2e_common import load_fixture, materialise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("TIDDIT_VARIANTS", "TIDDIT_GENOTYPE", "TIDDIT_GENOTYPE_DEPTH", "TIDDIT_DEPTH_DIST", "TIDDIT_FORCE_DIST", "TIDDIT_COV_TRACK", "TIDDIT_CNV",
            "TIDDIT_ALLELES", "TIDDIT_ALLELES_MIN_BQ", "TIDDIT_ASCN", "TIDDIT_QC", "TIDDIT_DUPS", "TIDDIT_INDELS", "TIDDIT_HOST_INGEST",
            "TIDDIT_DIST_BACKEND", "WORLD_SIZE", "RANK", "LOCAL_RANK")
PAIRS = []                       # the (case, entry) pairs that ran and passed
READER_OK = [c for c in D.CASES if c["reader_ok"]]


# ---- the kernels --------------------------------------------------------------------------------------------------------------
def _counter(case=None, ctx=None, capacity=None, Q=None):
    from tiddit_amd import tiddit_indels
    return tiddit_indels.IndelCounter(len(D.LENGTHS), Q if Q is not None else case["Q"] if case else 20,
                                      capacity=capacity or (case and case["capacity"]) or 1 << 12, ctx=ctx)


def _same(h, want, what):
    rows, by_support = want
    k1, k2 = h.keys()
    assert k1.dtype == k2.dtype == np.uint64 and len(k1) == len(k2)
    got = D.key_rows(list(zip(k1.tolist(), k2.tolist())))
    assert got.shape == rows.shape and np.array_equal(got, rows), (what, got.shape, rows.shape)
    for S, (counts, columns) in by_support.items():
        c = h.finish(S)
        assert c.dtype == np.uint64 and c.shape == (D.SIZE,)
        assert np.array_equal(c, counts), (what, S, c.tolist(), counts.tolist())
        r = h.rows()
        assert [x.dtype for x in r] == [np.uint64, np.uint64, np.uint32, np.uint32]
        for name, x, y in zip(("K1", "K2", "SUPPORT", "REV"), r, columns):
            assert x.shape == y.shape and np.array_equal(x, y), (what, S, name, x[:8].tolist(), y[:8].tolist())


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
    b = D.build(case, padding=False)
    w = bamio.BamWriter(path, [("c%d" % t, ln) for t, ln in enumerate(case["lengths"])])
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
    assert len(D.CASES) == D.N_CASES == 53 and len(READER_OK) == 34
    assert len(set(PAIRS)) == 53 + 34, len(set(PAIRS))


def _case(name):
    return next(c for c in D.CASES if c["name"] == name)


def test_state_accumulates_between_pushes_resets_keeps_handles_apart_and_finishes_again(wanted):
    case = _case("sets forward only, reverse only and mixed; supports round 1 2 and 3")
    other = _case("shape a batch of 65 reads")
    first, second, third = D.batches(case)
    h, g = _counter(), _counter(capacity=64)
    try:
        assert h.ctx is g.ctx
        assert not h.finish(1).any() and len(h.keys()[0]) == 0 and len(h.rows()[0]) == 0
        h.push_host_batch(first)
        g.push_host_batch(D.build(other))
        part = h.finish(1)
        assert part[D.SN.index("records")] == len(first) and 0 < part[D.SN.index("distinct_events")] < 5
        h.push_host_batch(second)
        h.push_host_batch(third)
        _same(h, wanted[case["name"]], "all pushes")
        _same(h, wanted[case["name"]], "every finish again")                   # (S = 1, 2, 3 and back to 1: the store is left as it was)
        _same(g, wanted[other["name"]], "the other handle")
        h.reset()
        assert not h.finish(2).any() and len(h.keys()[0]) == 0 and len(h.rows()[0]) == 0
        _same(g, wanted[other["name"]], "the other handle after the reset")
        for b in (third, first, second):
            h.push_host_batch(b)
        _same(h, wanted[case["name"]], "after the reset, in another order")
    finally:
        h.close()
        g.close()


def test_refused_arguments_leave_the_outputs_untouched():
    from tiddit_amd import _native
    case = _case("sets an INS and a DEL at one P, two lengths at one P, two contigs")
    ctx = _native.default_context()
    lib, P = ctx.lib, _native.ptr
    assert lib.tdt_indel_sn_size() == D.SIZE
    h = ctypes.c_void_p(0x5a5a)
    assert lib.tdt_indel_create(None, 3, 20, 64, ctypes.byref(h)) == -1 and h.value == 0x5a5a
    assert lib.tdt_indel_create(ctx.handle, 3, 20, 64, None) == -1 and lib.tdt_indel_create(ctx.handle, -1, 20, 64, ctypes.byref(h)) == -1
    assert lib.tdt_indel_create(ctx.handle, (1 << 24) + 1, 20, 64, ctypes.byref(h)) == -3 and h.value == 0x5a5a           # more than 2^24 contigs
    assert lib.tdt_indel_create(ctx.handle, 3, -1, 64, ctypes.byref(h)) == -3 and lib.tdt_indel_create(ctx.handle, 3, 256, 64, ctypes.byref(h)) == -3
    assert h.value == 0x5a5a
    assert lib.tdt_indel_create(ctx.handle, 1 << 24, 20, 0, ctypes.byref(h)) == 0                                       # (2^24 contigs, no store yet)
    try:
        b = D.build(case)
        cols = [getattr(b, k) for k in D.COLUMNS]
        n = len(b)

        def push(hh, c, nn, raw, raw_len):
            return lib.tdt_indel_push(hh, *[P(x) if x is not None else None for x in c], nn, P(raw) if raw is not None else None, raw_len)
        assert push(None, cols, n, b.raw, len(b.raw)) == -1
        for k in range(5):
            assert push(h, cols[:k] + [None] + cols[k + 1:], n, b.raw, len(b.raw)) == -1
        assert push(h, cols, n, None, len(b.raw)) == -1
        assert push(h, cols, 1 << 31, b.raw, len(b.raw)) == -1
        assert push(h, cols[:4] + [np.ascontiguousarray(b.rec_off[::-1])], n, b.raw, len(b.raw)) == -1           # offsets that decrease
        assert lib.tdt_indel_push_device(None, None, 0, 0) == -1
        assert lib.tdt_indel_push_device(h, None, 5, 100) == -1
        nulls = (ctypes.c_void_p * 14)()
        assert lib.tdt_indel_push_device(h, nulls, 5, 100) == -1                                   # a batch without its columns (the batch view)
        assert lib.tdt_indel_push_device(h, nulls, 1 << 31, 100) == -1
        out = np.full(D.SIZE, 7, dtype=np.uint64)
        nr = ctypes.c_size_t(77)
        assert lib.tdt_indel_finish(None, 1, P(out), ctypes.byref(nr)) == -1 and lib.tdt_indel_finish(h, 1, None, ctypes.byref(nr)) == -1
        assert lib.tdt_indel_finish(h, 1, P(out), None) == -1
        assert lib.tdt_indel_finish(h, 0, P(out), ctypes.byref(nr)) == -3 and lib.tdt_indel_finish(h, 10 ** 6 + 1, P(out), ctypes.byref(nr)) == -3   # a bad min_support
        assert (out == 7).all() and nr.value == 77
        ms = np.full(4, 7.0)
        assert lib.tdt_indel_timing(None, P(ms)) == -1 and lib.tdt_indel_timing(h, None) == -1 and (ms == 7).all()
        st = np.full(3, 7, dtype=np.uint64)
        assert lib.tdt_indel_reserve_stats(None, P(st)) == -1 and lib.tdt_indel_reserve_stats(h, None) == -1 and (st == 7).all()
        assert lib.tdt_indel_reset(None) == -1
        cnt = ctypes.c_size_t(77)
        k1, k2 = np.full(16, 7, dtype=np.uint64), np.full(16, 7, dtype=np.uint64)
        sup, rev = np.full(16, 7, dtype=np.uint32), np.full(16, 7, dtype=np.uint32)
        assert lib.tdt_indel_keys(None, P(k1), P(k2), ctypes.byref(cnt)) == -1 and lib.tdt_indel_keys(h, P(k1), P(k2), None) == -1
        assert lib.tdt_indel_keys(h, P(k1), None, ctypes.byref(cnt)) == -1 and cnt.value == 77
        assert lib.tdt_indel_rows(None, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -1 and lib.tdt_indel_rows(h, P(k1), P(k2), P(sup), P(rev), None) == -1
        assert lib.tdt_indel_rows(h, P(k1), P(k2), None, P(rev), ctypes.byref(cnt)) == -1
        assert lib.tdt_indel_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -1 and cnt.value == 77            # no finish yet
        # nothing refused above stored anything; n = 0 is a no-op; and the handle still works
        assert push(h, [None] * 5, 0, None, 0) == 0 and lib.tdt_indel_push_device(h, None, 0, 0) == 0
        assert lib.tdt_indel_finish(h, 1, P(out), ctypes.byref(nr)) == 0 and not out.any() and nr.value == 0
        assert lib.tdt_indel_keys(h, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 0
        assert push(h, cols, n, b.raw, len(b.raw)) == 0
        cnt = ctypes.c_size_t(16)
        assert lib.tdt_indel_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -1 and cnt.value == 16            # a push since the finish
        want_keys, by_support = D.expected(case)
        assert lib.tdt_indel_finish(h, 1, P(out), ctypes.byref(nr)) == 0 and nr.value == 4
        assert np.array_equal(out, by_support[1][0])
        cnt = ctypes.c_size_t(4)                                                                   # room for 4 of the 5 keys: refused, nothing written
        assert lib.tdt_indel_keys(h, P(k1), P(k2), ctypes.byref(cnt)) == -3 and cnt.value == 4 and (k1 == 7).all() and (k2 == 7).all()
        cnt = ctypes.c_size_t(3)                                                                   # room for 3 of the 4 rows: the same
        assert lib.tdt_indel_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -3 and cnt.value == 3
        assert (k1 == 7).all() and (k2 == 7).all() and (sup == 7).all() and (rev == 7).all()
        cnt = ctypes.c_size_t(0)
        assert lib.tdt_indel_rows(h, None, None, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 4                    # the count alone
        cnt = ctypes.c_size_t(16)
        assert lib.tdt_indel_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == 0 and cnt.value == 4 and (k1[4:] == 7).all() and (rev[4:] == 7).all()
        assert all(np.array_equal(x[:4], y) for x, y in zip((k1, k2, sup, rev), by_support[1][1]))
        cnt = ctypes.c_size_t(16)
        assert lib.tdt_indel_keys(h, P(k1), P(k2), ctypes.byref(cnt)) == 0 and cnt.value == 5 and (k1[5:] == 7).all()
        assert np.array_equal(D.key_rows(list(zip(k1[:5].tolist(), k2[:5].tolist()))), want_keys)
        # a raw_len of 0: every eligible read is malformed, nothing is read; the column counters still count
        assert lib.tdt_indel_reset(h) == 0 and push(h, cols, n, None, 0) == 0
        assert lib.tdt_indel_finish(h, 1, P(out), ctypes.byref(nr)) == 0 and nr.value == 0
        assert np.array_equal(out, D.counters_of({"records": 5, "eligible": 5, "malformed": 5}, 0, 0))
    finally:
        assert lib.tdt_indel_destroy(h) == 0 and lib.tdt_indel_destroy(None) == 0


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------
def _env(**env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    return e


def _argv(bam, fa, out, fx):
    return [sys.executable, "-m", "tiddit_amd", "--sv", "--bam", bam, "--ref", fa, "-o", out, "--skip_assembly", "-s", str(fx["params"]["n_reads_stats"])]


def _job(bam, fa, out, fx, timeout=600, **env):
    return subprocess.run(_argv(bam, fa, out, fx), cwd=REPO, env=_env(**env), capture_output=True, text=True, timeout=timeout)


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
                out[rel[len(base):]] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


@pytest.fixture(scope="module")
def jobs(golden_dir, tmp_path_factory):
    """(each job is checked before the next one is started: a crash, a time-out or a GPU error ends the fixture there)"""
    fx = load_fixture(golden_dir, "sv_e2e_small.json")
    d = str(tmp_path_factory.mktemp("indels"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    paths = {n: os.path.join(d, n) for n in ("off", "on", "two", "host", "ranks", "bad")}
    _ok(_job(bam, fa, paths["off"], fx))
    r = _ok(_job(bam, fa, paths["on"], fx, TIDDIT_INDELS="1:20"))
    r2 = _ok(_job(bam, fa, paths["two"], fx, TIDDIT_INDELS="2"))
    _ok(_job(bam, fa, paths["host"], fx, TIDDIT_INDELS="1:20", TIDDIT_HOST_INGEST="1"))
    return fx, bam, fa, d, paths, r, r2


@pytest.fixture(scope="module")
def defined(jobs):
    """the definition over the host reader's batches, once: the push counters, the keys, the contig names — and the job's 50-bp coverage
    bins as the C oracle computes them from the same columns (the scan's filter: -q 5, the default)"""
    import oracle
    from tiddit_amd import bamio, tiddit_indels
    fx, bam = jobs[0], jobs[1]
    sn, keys = {}, []
    cols = {k: [] for k in ("tid", "pos", "end", "mapq", "flag")}
    rd = bamio.BamReader(bam)
    names, lengths = list(rd.references), list(rd.lengths)
    for b in rd.batches():
        keys.extend(tiddit_indels.keys_of_batch(b, sn, 20))
        for k in cols:
            cols[k].append(np.array(getattr(b, k)))
    rd.close()
    cols = {k: np.concatenate(v) for k, v in cols.items()}
    cover = {}
    for t in sorted({k1 >> 32 for k1, _ in keys}):
        m = cols["tid"] == t
        cover[names[t]] = oracle.coverage_stream(cols["pos"][m], cols["end"][m], cols["mapq"][m], cols["flag"][m], lengths[t], 50, 5)[0]
    return sn, keys, names, cover


def _rows_text(path):
    """the file split into its head (everything but the COV column of the rows) and the COV column"""
    lines = open(path).read().split("\n")
    at = lines.index("#CHROM\tPOS\tTYPE\tLEN\tSEQ\tSUPPORT\tFWD\tREV\tCOV")
    rows = [l.split("\t") for l in lines[at + 1:] if l]
    return lines[:at + 1], [r[:8] for r in rows], [r[8] for r in rows]


@pytest.mark.parametrize("which,S", [("on", 1), ("two", 2)])
def test_the_file_equals_the_definition_on_the_host_readers_batches(jobs, defined, tmp_path, which, S):
    from tiddit_amd import tiddit_indels
    fx, bam, fa, d, paths, r, r2 = jobs
    sn, keys, names, cover = defined
    counts, rows = tiddit_indels.summarise(keys, sn, S)
    v = lambda k: int(counts[D.SN.index(k)])
    assert v("records") == fx["n_records"] == 604338                                    # every record of the file, once
    assert v("malformed") == 0 and v("deletions") > 0 and v("distinct_events") > 0 and v("reported_events") == len(rows)
    if S == 1:
        assert len(rows) > 100                                                          # (the planted deletions: the table is not empty)
    got_path = paths[which] + ".indels.tab"
    head, body, cov = _rows_text(got_path)
    assert all(c != "." for c in cov)                                                    # (every contig of the fixture has bins)
    want = str(tmp_path / "want.indels.tab")
    tiddit_indels.write_file(want, counts, rows, names, cover, S, 20)
    got = open(got_path, "rb").read()
    assert len(got) > 250 and got == open(want, "rb").read()
    assert ("SN\trecords\t%d\n" % fx["n_records"]).encode() in got and got.startswith(b"# tiddit_amd indels v1 min_support=%d min_mapq=20\n" % S)
    assert len(body) == len(rows) and all(b[2] == "DEL" for b in body)
    out = (r if which == "on" else r2).stdout
    assert [l for l in out.split("\n") if l.startswith("indels:")] == [tiddit_indels.summary_line(counts)]


def test_host_ingest_writes_the_same_bytes(jobs):
    """the host-ingest job fills its bins by another path (host columns pushed per contig) and writes the same bytes; the column itself
    is compared with the oracle's bins in the test of the file above"""
    fx, bam, fa, d, paths, r, r2 = jobs
    assert open(paths["host"] + ".indels.tab", "rb").read() == open(paths["on"] + ".indels.tab", "rb").read()
    head, body, cov = _rows_text(paths["on"] + ".indels.tab")
    assert len(cov) > 100 and all(float(c) > 0 for c in cov)


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    fx, bam, fa, d, paths, r, r2 = jobs
    off, on, two, host = (_files(paths[k]) for k in ("off", "on", "two", "host"))
    assert set(on) - set(off) == {".indels.tab"} and set(off) <= set(on) and len(off) >= 5
    assert all(on[k] == off[k] for k in off), [k for k in off if on[k] != off[k]]
    assert all(two[k] == off[k] for k in off), [k for k in off if two[k] != off[k]]
    assert not os.path.exists(paths["off"] + ".indels.tab") and ".indels.tab" in host


def test_a_malformed_value_of_the_switch_is_an_error(jobs):
    fx, bam, fa, d, paths, r, r2 = jobs
    bad = _job(bam, fa, paths["bad"], fx, timeout=120, TIDDIT_INDELS="2:300")
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == ["error, TIDDIT_INDELS=2:300: the minimum MAPQ is 0 ... 255"]
    assert not os.path.exists(paths["bad"] + "_tiddit") and not os.path.exists(paths["bad"] + ".indels.tab")


def test_n_ranks_refuse_the_switch_and_write_nothing(jobs):
    """every rank ends with the refusal before the first collective (no process group is ever made) and no file is written"""
    fx, bam, fa, d, paths, r, r2 = jobs
    res = _job(bam, fa, paths["ranks"], fx, timeout=120, TIDDIT_INDELS="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29543",
               TIDDIT_DIST_BACKEND="gloo", TIDDIT_FORCE_DIST="1")
    assert res.returncode == 1, (res.returncode, res.stdout[-1000:], res.stderr[-2000:])
    errors = [l for l in res.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_INDELS is a one-process switch")
    assert not os.path.exists(paths["ranks"] + "_tiddit") and not os.path.exists(paths["ranks"] + ".indels.tab")
