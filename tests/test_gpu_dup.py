"""`TIDDIT_DUPS` on the GPU: the kernels (csrc/tdt_dup.hip) on every aimed case of tests/dup_cases.py through both entries —
``tdt_dup_push`` on host columns, and ``tdt_dup_push_device`` on the batches a ``DeviceBamReader`` decodes from a small BAM written from
the case's records — against the case's claim and the struct / Counter restatement: the store read out by ``tdt_dup_keys`` equals the
definition's keys as a multiset (``np.array_equal`` on the sorted ``(K1, K2, marked)`` rows) and ``tdt_dup_finish`` equals the
definition's counter array exactly; the handle's state, its refusals, and the switch end to end on the sv_e2e_small fixture, every job a
fresh child process under its own time limit.

The fixture holds 604 338 records: the end to end test runs ``tiddit_dup.keys_of_batch`` — the same rules on whole columns, pinned to
``key_of_read`` on every aimed case by tests/test_dup_refs_cpu.py — over the host reader's batches.  The fixture's reads carry no ``MC``
tag, so there ``pairs_no_mc == pairs``; what covers the ``MC`` walk are the aimed cases of the ``mc`` family.

Every test of this file fails on the parent commit: the symbols and the switch do not exist there."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import dup_cases as D
from sv_e2e_common import load_fixture, materialise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("TIDDIT_VARIANTS", "TIDDIT_GENOTYPE", "TIDDIT_GENOTYPE_DEPTH", "TIDDIT_DEPTH_DIST", "TIDDIT_FORCE_DIST", "TIDDIT_COV_TRACK", "TIDDIT_CNV",
            "TIDDIT_ALLELES", "TIDDIT_ALLELES_MIN_BQ", "TIDDIT_ASCN", "TIDDIT_QC", "TIDDIT_DUPS", "TIDDIT_HOST_INGEST", "TIDDIT_DIST_BACKEND", "WORLD_SIZE",
            "RANK", "LOCAL_RANK")
PAIRS = []                       # the (case, entry) pairs that ran and passed
READER_OK = [c for c in D.CASES if c["reader_ok"]]


# ---- the kernels --------------------------------------------------------------------------------------------------------------
def _counter(case=None, ctx=None, capacity=None):
    from tiddit_amd import tiddit_dup
    return tiddit_dup.DupCounter(len(D.LENGTHS), max(D.LENGTHS), capacity=capacity or (case and case["capacity"]) or 1 << 12, ctx=ctx)


def _same(h, want, what):
    rows, counts = want
    k1, k2, m = h.keys()
    assert k1.dtype == k2.dtype == np.uint64 and m.dtype == np.uint8 and len(k1) == len(k2) == len(m)
    got = D.rows_of(list(zip(k1.tolist(), k2.tolist(), m.tolist())))
    assert got.shape == rows.shape and np.array_equal(got, rows), (what, got.shape, rows.shape)
    c = h.finish()
    assert c.dtype == np.uint64 and c.shape == (D.SIZE,)
    assert np.array_equal(c, counts), (what, [(int(k), int(c[k]), int(counts[k])) for k in np.flatnonzero(c != counts)[:8]])


@pytest.fixture(scope="module")
def wanted():
    out = {}
    for c in D.CASES:
        claim, ref = D.expected(c), D.reference(c)
        assert np.array_equal(claim[0], ref[0]) and np.array_equal(claim[1], ref[1]), c["name"]
        out[c["name"]] = ref
    return out


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_push_equals_the_reference(case, wanted):
    h = _counter(case)
    try:
        for b in D.batches(case):
            h.push_host_batch(b)
        _same(h, wanted[case["name"]], case["name"])
    finally:
        h.close()
    PAIRS.append((case["name"], "push"))


def _write_bam(path, case):
    from tiddit_amd import bamio
    b = D.build(case, padding=False)
    w = bamio.BamWriter(path, [("c%d" % t, ln) for t, ln in enumerate(case["lengths"])])
    w._buf += b.raw.tobytes()                     # the case's records as they are, aux fields included
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
    assert len(D.CASES) == D.N_CASES == 45 and len(READER_OK) == 31
    assert len(set(PAIRS)) == 45 + 31, len(set(PAIRS))


def test_the_order_of_the_reads_changes_nothing(wanted):
    """the same reads in file order, reversed and shuffled: equal counters, equal key multisets"""
    case = next(c for c in D.CASES if c["name"] == "sizes sets of 1 2 63 64 65 and round DUP_HIST_MAX")
    n = len(case["reads"])
    for order in (np.arange(n), np.arange(n)[::-1], np.random.default_rng(5).permutation(n)):
        h = _counter()
        try:
            b = D.build_reads([case["reads"][k] for k in order.tolist()])
            for lo in range(0, n, 1500):
                h.push_host_batch(b.cut(lo, min(lo + 1500, n)))
            _same(h, wanted[case["name"]], "order")
        finally:
            h.close()


def test_state_accumulates_between_pushes_resets_keeps_handles_apart_and_finishes_twice(wanted):
    case = next(c for c in D.CASES if c["name"] == "carrier mates that make a fragment, records that are not eligible")
    other = next(c for c in D.CASES if c["name"] == "shape a batch of 65 reads")
    first, second, third = D.batches(case)
    h, g = _counter(), _counter(capacity=64)
    try:
        assert h.ctx is g.ctx
        assert not h.finish().any() and len(h.keys()[0]) == 0
        h.push_host_batch(first)
        g.push_host_batch(D.build(other))
        part = h.finish()
        assert part[D.SN.index("records")] == len(first) and 0 < part[D.SN.index("fragments")] < wanted[case["name"]][1][D.SN.index("fragments")]
        h.push_host_batch(second)
        h.push_host_batch(third)
        _same(h, wanted[case["name"]], "all pushes")
        _same(h, wanted[case["name"]], "a second finish")
        _same(g, wanted[other["name"]], "the other handle")
        h.reset()
        assert not h.finish().any() and len(h.keys()[0]) == 0
        _same(g, wanted[other["name"]], "the other handle after the reset")
        for b in (third, first, second):
            h.push_host_batch(b)
        _same(h, wanted[case["name"]], "after the reset, in another order")
    finally:
        h.close()
        g.close()


def test_refused_arguments_leave_the_outputs_untouched():
    from tiddit_amd import _native
    case = next(c for c in D.CASES if c["name"] == "sets pairs that differ in one field")
    ctx = _native.default_context()
    lib, P = ctx.lib, _native.ptr
    assert lib.tdt_dup_size() == D.SIZE
    h = ctypes.c_void_p(0x5a5a)
    assert lib.tdt_dup_create(None, 3, 1000, 64, ctypes.byref(h)) == -1 and h.value == 0x5a5a
    assert lib.tdt_dup_create(ctx.handle, 3, 1000, 64, None) == -1
    assert lib.tdt_dup_create(ctx.handle, -1, 1000, 64, ctypes.byref(h)) == -1 and lib.tdt_dup_create(ctx.handle, 3, -1, 64, ctypes.byref(h)) == -1
    assert lib.tdt_dup_create(ctx.handle, (1 << 24) + 1, 1000, 64, ctypes.byref(h)) == -3 and h.value == 0x5a5a           # more than 2^24 contigs
    assert lib.tdt_dup_create(ctx.handle, 1 << 24, 1000, 0, ctypes.byref(h)) == 0                                       # (2^24 contigs, no store yet)
    try:
        b = D.build(case)
        cols = [getattr(b, k) for k in ("flag", "tid", "pos", "end", "mate_tid", "mate_pos", "rec_off")]
        n = len(b)

        def push(hh, c, nn, raw, raw_len):
            return lib.tdt_dup_push(hh, *[P(x) if x is not None else None for x in c], nn, P(raw) if raw is not None else None, raw_len)
        assert push(None, cols, n, b.raw, len(b.raw)) == -1
        for k in range(7):
            assert push(h, cols[:k] + [None] + cols[k + 1:], n, b.raw, len(b.raw)) == -1
        assert push(h, cols, n, None, len(b.raw)) == -1
        assert push(h, cols, 1 << 31, b.raw, len(b.raw)) == -1
        assert push(h, cols[:6] + [np.ascontiguousarray(b.rec_off[::-1])], n, b.raw, len(b.raw)) == -1           # offsets that decrease
        assert lib.tdt_dup_push_device(None, None, 0, 0) == -1
        assert lib.tdt_dup_push_device(h, None, 5, 100) == -1
        nulls = (ctypes.c_void_p * 14)()
        assert lib.tdt_dup_push_device(h, nulls, 5, 100) == -1                                     # a batch without its columns
        assert lib.tdt_dup_push_device(h, nulls, 1 << 31, 100) == -1
        out = np.full(D.SIZE, 7, dtype=np.uint64)
        assert lib.tdt_dup_finish(None, P(out)) == -1 and lib.tdt_dup_finish(h, None) == -1 and (out == 7).all()
        ms = np.full(4, 7.0)
        assert lib.tdt_dup_timing(None, P(ms)) == -1 and lib.tdt_dup_timing(h, None) == -1 and (ms == 7).all()
        assert lib.tdt_dup_reset(None) == -1
        cnt = ctypes.c_size_t(77)
        k1, k2, m = np.full(16, 7, dtype=np.uint64), np.full(16, 7, dtype=np.uint64), np.full(16, 7, dtype=np.uint8)
        assert lib.tdt_dup_keys(None, P(k1), P(k2), P(m), ctypes.byref(cnt)) == -1 and lib.tdt_dup_keys(h, P(k1), P(k2), P(m), None) == -1
        assert lib.tdt_dup_keys(h, P(k1), None, P(m), ctypes.byref(cnt)) == -1 and cnt.value == 77
        # nothing refused above stored anything; n = 0 is a no-op; and the handle still works
        assert push(h, [None] * 7, 0, None, 0) == 0 and lib.tdt_dup_push_device(h, None, 0, 0) == 0
        assert lib.tdt_dup_finish(h, P(out)) == 0 and not out.any()
        assert lib.tdt_dup_keys(h, None, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 0
        assert push(h, cols, n, b.raw, len(b.raw)) == 0
        assert lib.tdt_dup_finish(h, P(out)) == 0
        assert np.array_equal(out, D.expected(case)[1])
        cnt = ctypes.c_size_t(8)                                                                   # room for 8 of the 9 keys: refused, nothing written
        assert lib.tdt_dup_keys(h, P(k1), P(k2), P(m), ctypes.byref(cnt)) == -3 and cnt.value == 8 and (k1 == 7).all() and (k2 == 7).all() and (m == 7).all()
        cnt = ctypes.c_size_t(16)
        assert lib.tdt_dup_keys(h, P(k1), P(k2), P(m), ctypes.byref(cnt)) == 0 and cnt.value == 9 and (k1[9:] == 7).all() and (m[9:] == 7).all()
        assert np.array_equal(D.rows_of(list(zip(k1[:9].tolist(), k2[:9].tolist(), m[:9].tolist()))), D.expected(case)[0])
        # a raw_len of 0: every fragment and carrier is malformed, nothing is read; the column counters still count
        assert lib.tdt_dup_reset(h) == 0 and push(h, cols, n, None, 0) == 0
        assert lib.tdt_dup_finish(h, P(out)) == 0
        assert np.array_equal(out, D.counters_of({"records": 9, "eligible": 9, "malformed": 9}, {}))
    finally:
        assert lib.tdt_dup_destroy(h) == 0 and lib.tdt_dup_destroy(None) == 0


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
    fx = load_fixture(golden_dir, "sv_e2e_small.json")
    d = str(tmp_path_factory.mktemp("dup"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    paths = {n: os.path.join(d, n) for n in ("off", "on", "host", "ranks", "bad")}
    _ok(_job(bam, fa, paths["off"], fx))
    r = _ok(_job(bam, fa, paths["on"], fx, TIDDIT_DUPS="1"))
    _ok(_job(bam, fa, paths["host"], fx, TIDDIT_DUPS="1", TIDDIT_HOST_INGEST="1"))
    return fx, bam, fa, d, paths, r


def test_the_file_equals_the_definition_on_the_host_readers_batches(jobs, tmp_path):
    """(the fixture's reads carry no MC tag: pairs_no_mc == pairs here, the aimed cases are what cover the MC walk)"""
    from tiddit_amd import bamio, tiddit_dup
    fx, bam, fa, d, paths, r = jobs
    sn, cols = {}, []
    rd = bamio.BamReader(bam)
    for b in rd.batches():
        cols.append(tiddit_dup.keys_of_batch(b, sn))
    rd.close()
    k1, k2 = (np.concatenate([x[k] for x in cols]) for k in range(2))
    counts = tiddit_dup.summarise_columns(k1, k2, sn)
    v = lambda k: int(counts[D.SN.index(k)])
    assert v("records") == fx["n_records"] == 604338                                    # every record of the file, once
    assert v("malformed") == 0 and v("pairs") > 100_000 and v("pairs_no_mc") == v("pairs") and v("pair_mates") > 100_000 and v("pair_sets") > 100_000
    assert v("eligible") == v("fragments") + v("pairs") + v("pair_mates")
    want = str(tmp_path / "want.dup.tab")
    tiddit_dup.write_file(want, counts)
    got = open(paths["on"] + ".dup.tab", "rb").read()
    assert len(got) > 300 and got == open(want, "rb").read()
    assert ("SN\trecords\t%d\n" % fx["n_records"]).encode() in got
    assert [l for l in r.stdout.split("\n") if l.startswith("duplicates:")] == [tiddit_dup.summary_line(counts)]
    assert open(paths["host"] + ".dup.tab", "rb").read() == got


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    fx, bam, fa, d, paths, r = jobs
    off, on, host = _files(paths["off"]), _files(paths["on"]), _files(paths["host"])
    assert set(on) - set(off) == {".dup.tab"} and set(off) <= set(on) and len(off) >= 5
    assert all(on[k] == off[k] for k in off), [k for k in off if on[k] != off[k]]
    assert not os.path.exists(paths["off"] + ".dup.tab") and ".dup.tab" in host


def test_any_other_value_of_the_switch_is_an_error(jobs):
    fx, bam, fa, d, paths, r = jobs
    bad = _job(bam, fa, paths["bad"], fx, timeout=120, TIDDIT_DUPS="2")
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == ["error, TIDDIT_DUPS=2: the switch is 1 or unset"]
    assert not os.path.exists(paths["bad"] + "_tiddit") and not os.path.exists(paths["bad"] + ".dup.tab")


def test_two_ranks_refuse_the_switch_and_write_nothing(jobs):
    """every rank ends with the refusal before the first collective (no process group is ever made) and no file is written"""
    fx, bam, fa, d, paths, r = jobs
    for env in (dict(WORLD_SIZE="2"), dict(TIDDIT_FORCE_DIST="1")):
        for rank in range(2 if "WORLD_SIZE" in env else 1):
            res = _job(bam, fa, paths["ranks"], fx, timeout=120, TIDDIT_DUPS="1", RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT="29541", TIDDIT_DIST_BACKEND="gloo", **env)
            assert res.returncode == 1, (res.returncode, res.stdout[-1000:], res.stderr[-2000:])
            errors = [l for l in res.stdout.split("\n") if l.startswith("error")]
            assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_DUPS is a one-process switch")
    assert not os.path.exists(paths["ranks"] + "_tiddit") and not os.path.exists(paths["ranks"] + ".dup.tab")
