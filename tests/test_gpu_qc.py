"""`TIDDIT_QC` on the GPU: the kernels (csrc/tdt_qc.hip) on every aimed case of tests/qc_cases.py through both entries — ``tdt_qc_push`` on
host columns, and ``tdt_qc_push_device`` on the batches a ``DeviceBamReader`` decodes from a small BAM written from the case's records —
against the case's claim and the numpy restatement (integers: ``np.array_equal`` on the whole counter array); the handle's state, its
refusals, and the switch end to end on the sv_e2e_small fixture, every job a fresh child process under its own time limit.

The fixture holds 604 338 records of 150 bases: the per-base Python loop of ``tiddit_qc.count_read`` would take minutes on it, so the end
to end test runs ``tiddit_qc.count_batch_columns`` — the same rules on whole columns, pinned to ``count_read`` on every aimed case by
tests/test_qc_refs_cpu.py — over the host reader's batches.

Every test of this file fails on the parent commit: the symbols and the switch do not exist there."""
import ctypes
import hashlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import qc_cases as QC
from sv_e2e_common import load_fixture, materialise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("TIDDIT_VARIANTS", "TIDDIT_GENOTYPE", "TIDDIT_GENOTYPE_DEPTH", "TIDDIT_DEPTH_DIST", "TIDDIT_FORCE_DIST", "TIDDIT_COV_TRACK", "TIDDIT_CNV",
            "TIDDIT_ALLELES", "TIDDIT_ALLELES_MIN_BQ", "TIDDIT_ASCN", "TIDDIT_QC", "TIDDIT_HOST_INGEST", "TIDDIT_DIST_BACKEND", "WORLD_SIZE", "RANK",
            "LOCAL_RANK")
PAIRS = []                       # the (case, entry) pairs that ran and passed
READER_OK = [c for c in QC.CASES if c["reader_ok"]]


# ---- the kernels --------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    assert got.dtype == np.uint64 and got.shape == (QC.SIZE,)
    assert np.array_equal(got, want), (what, [(int(k), int(got[k]), int(want[k])) for k in np.flatnonzero(got != want)[:8]])


@pytest.fixture(scope="module")
def wanted():
    out = {}
    for c in QC.CASES:
        claim, ref = QC.expected(c), QC.reference(c)
        assert np.array_equal(claim, ref), c["name"]
        out[c["name"]] = ref
    return out


@pytest.mark.parametrize("case", QC.CASES, ids=[c["name"] for c in QC.CASES])
def test_push_equals_the_reference(case, wanted):
    from tiddit_amd import tiddit_qc
    h = tiddit_qc.QcCounter()
    try:
        for b in QC.batches(case):
            h.push_host_batch(b)
        _same(h.counts(), wanted[case["name"]], case["name"])
    finally:
        h.close()
    PAIRS.append((case["name"], "push"))


def _write_bam(path, case):
    from tiddit_amd import bamio
    b = QC.build(case, padding=False)
    w = bamio.BamWriter(path, [("c%d" % t, ln) for t, ln in enumerate(case["lengths"])])
    w._buf += b.raw.tobytes()                     # the case's records as they are, qualities included (BamWriter.write takes none)
    w.close()


@pytest.mark.parametrize("case", READER_OK, ids=[c["name"] for c in READER_OK])
def test_push_device_from_a_small_bam_equals_the_reference(case, wanted, tmp_path):
    from tiddit_amd import bamio, tiddit_qc
    path = str(tmp_path / "case.bam")
    _write_bam(path, case)
    rd = bamio.DeviceBamReader(path)
    h = None
    try:
        h = tiddit_qc.QcCounter(ctx=rd.ctx)
        n = 0
        for b in rd.batches():
            h.push_device_batch(b)
            n += len(b)
        assert n == len(case["reads"])
        _same(h.counts(), wanted[case["name"]], case["name"])
    finally:
        if h is not None:
            h.close()
        rd.close()
    PAIRS.append((case["name"], "push_device"))


def test_the_stated_count_of_case_entry_pairs_ran():
    assert len(QC.CASES) == QC.N_CASES == 59 and len(READER_OK) == 54
    assert len(set(PAIRS)) == 59 + 54, len(set(PAIRS))


def test_state_accumulates_reads_between_pushes_resets_and_keeps_handles_apart(wanted):
    from tiddit_amd import tiddit_qc
    case = next(c for c in QC.CASES if c["name"] == "flags the combinations the rules branch on")
    other = next(c for c in QC.CASES if c["name"] == "shape a batch of 65 reads")
    first, second, third = QC.batches(case)
    part = np.zeros(QC.SIZE, dtype=np.int64)
    QC.reference_batch(part, first, None)
    part = part.astype(np.uint64)
    assert 0 < part.sum() < wanted[case["name"]].sum()
    h, g = tiddit_qc.QcCounter(), tiddit_qc.QcCounter()
    try:
        assert h.ctx is g.ctx
        assert not h.counts().any()
        h.push_host_batch(first)
        g.push_host_batch(QC.build(other))
        _same(h.counts(), part, "first push")
        h.push_host_batch(second)
        h.push_host_batch(third)
        _same(h.counts(), wanted[case["name"]], "all pushes")
        _same(g.counts(), wanted[other["name"]], "the other handle")
        h.reset()
        assert not h.counts().any()
        _same(g.counts(), wanted[other["name"]], "the other handle after the reset")
        for b in (third, first, second):
            h.push_host_batch(b)
        _same(h.counts(), wanted[case["name"]], "after the reset, in another order")
    finally:
        h.close()
        g.close()


def test_counts_device_equals_counts():
    import torch
    from tiddit_amd import tiddit_qc
    case = next(c for c in QC.CASES if c["name"] == "shape a batch of 257 reads")
    h = tiddit_qc.QcCounter()
    try:
        h.push_host_batch(QC.build(case))
        counts = h.counts()
        d_out = torch.full((QC.SIZE + 1,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert h.ctx.lib.tdt_qc_counts_device(h.handle, d_out.data_ptr()) == 0
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:QC.SIZE].view(np.uint64), counts) and got[QC.SIZE] == 7
        assert h.ctx.lib.tdt_qc_counts_device(h.handle, d_out.data_ptr() + 4) == -1
        assert h.ctx.lib.tdt_qc_counts_device(h.handle, None) == -1
        assert h.ctx.lib.tdt_qc_counts_device(None, d_out.data_ptr()) == -1
    finally:
        h.close()


def test_refused_arguments_leave_the_outputs_untouched():
    from tiddit_amd import _native
    case = next(c for c in QC.CASES if c["name"] == "cigar ops in pairs")
    ctx = _native.default_context()
    lib, P = ctx.lib, _native.ptr
    assert lib.tdt_qc_size() == QC.SIZE
    h = ctypes.c_void_p(0x5a5a)
    assert lib.tdt_qc_create(None, ctypes.byref(h)) == -1 and h.value == 0x5a5a
    assert lib.tdt_qc_create(ctx.handle, None) == -1
    assert lib.tdt_qc_create(ctx.handle, ctypes.byref(h)) == 0
    try:
        b = QC.build(case)
        cols = [getattr(b, k) for k in QC.Batch.COLUMNS]
        n = len(b)

        def push(hh, c, nn, raw, raw_len):
            return lib.tdt_qc_push(hh, *[P(x) if x is not None else None for x in c], nn, P(raw) if raw is not None else None, raw_len)
        assert push(None, cols, n, b.raw, len(b.raw)) == -1
        for k in range(7):
            assert push(h, cols[:k] + [None] + cols[k + 1:], n, b.raw, len(b.raw)) == -1
        assert push(h, cols, n, None, len(b.raw)) == -1
        assert push(h, cols, 1 << 31, b.raw, len(b.raw)) == -1
        assert push(h, cols[:6] + [np.ascontiguousarray(b.rec_off[::-1])], n, b.raw, len(b.raw)) == -1           # offsets that decrease
        assert lib.tdt_qc_push_device(None, None, 0, 0) == -1
        assert lib.tdt_qc_push_device(h, None, 5, 100) == -1
        nulls = (ctypes.c_void_p * 14)()
        assert lib.tdt_qc_push_device(h, nulls, 5, 100) == -1                                      # a batch without its columns
        assert lib.tdt_qc_push_device(h, nulls, 1 << 31, 100) == -1
        out = np.full(QC.SIZE, 7, dtype=np.uint64)
        assert lib.tdt_qc_counts(None, P(out)) == -1 and lib.tdt_qc_counts(h, None) == -1 and (out == 7).all()
        assert lib.tdt_qc_reset(None) == -1
        # nothing refused above counted anything; n = 0 is a no-op; and the handle still works
        assert push(h, [None] * 7, 0, None, 0) == 0 and lib.tdt_qc_push_device(h, None, 0, 0) == 0
        assert lib.tdt_qc_counts(h, P(out)) == 0 and not out.any()
        assert push(h, cols, n, b.raw, len(b.raw)) == 0
        assert lib.tdt_qc_counts(h, P(out)) == 0
        assert np.array_equal(out, QC.expected(case))
        # a raw_len of 0: every record of S is malformed, nothing is read; the field sections still count
        assert lib.tdt_qc_reset(h) == 0 and push(h, cols, n, None, 0) == 0
        assert lib.tdt_qc_counts(h, P(out)) == 0
        want = np.zeros(QC.SIZE, dtype=np.uint64)
        for key, v in (QC.merge(QC.plain(6), QC.sn(malformed=6), {("RL", 3): 3, ("RL", 5): 2, ("RL", 2): 1})).items():
            want[QC.index(key)] = v
        assert np.array_equal(out, want)
    finally:
        assert lib.tdt_qc_destroy(h) == 0 and lib.tdt_qc_destroy(None) == 0


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


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_ranks(bam, fa, out, fx):
    port = _port()
    procs = [subprocess.Popen(_argv(bam, fa, out, fx), cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=_env(TIDDIT_QC="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2",
                                       LOCAL_RANK=str(r), TIDDIT_HIP_DEVICE="0", TIDDIT_DIST_BACKEND="gloo", TIDDIT_INGEST_CHUNK=str(48 << 20)))
             for r in range(2)]
    res = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=600)
            res.append((p.returncode, o, e))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(r[0] == 0 for r in res), [(r[0], r[1][-1500:], r[2][-3000:]) for r in res]
    return res


@pytest.fixture(scope="module")
def jobs(golden_dir, tmp_path_factory):
    fx = load_fixture(golden_dir, "sv_e2e_small.json")
    d = str(tmp_path_factory.mktemp("qc"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    paths = {n: os.path.join(d, n) for n in ("off", "on", "host", "ranks", "bad")}
    _ok(_job(bam, fa, paths["off"], fx))
    r = _ok(_job(bam, fa, paths["on"], fx, TIDDIT_QC="1"))
    _ok(_job(bam, fa, paths["host"], fx, TIDDIT_QC="1", TIDDIT_HOST_INGEST="1"))
    ranks = _two_ranks(bam, fa, paths["ranks"], fx)
    return fx, bam, fa, d, paths, r, ranks


def test_the_file_equals_the_definition_on_the_host_readers_batches(jobs, tmp_path):
    from tiddit_amd import bamio, tiddit_qc
    fx, bam, fa, d, paths, r, ranks = jobs
    counts = np.zeros(QC.SIZE, dtype=np.int64)
    rd = bamio.BamReader(bam)
    for b in rd.batches():
        tiddit_qc.count_batch_columns(counts, b)
    rd.close()
    sn = lambda k: int(counts[QC.index(("SN", k))])
    assert sn("records") == fx["n_records"] == 604338                                   # every record of the file, once
    assert sn("malformed") == 0 and sn("bases") > 80_000_000 and sn("bases_q30") > 0 and sn("reverse") > 100_000 and sn("soft_clipped_bases") > 0
    assert counts[QC.SECTIONS["IS"][0]:QC.SECTIONS["CYC"][0]].sum() > 200_000
    want = str(tmp_path / "want.qc.tab")
    tiddit_qc.write_file(want, counts)
    got = open(paths["on"] + ".qc.tab", "rb").read()
    assert len(got) > 10_000 and got == open(want, "rb").read()
    assert ("SN\trecords\t%d\n" % fx["n_records"]).encode() in got
    line = [l for l in r.stdout.split("\n") if l.startswith("qc tables:")]
    assert line == [tiddit_qc.summary_line(counts)]


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    fx, bam, fa, d, paths, r, ranks = jobs
    off, on = _files(paths["off"]), _files(paths["on"])
    assert set(on) - set(off) == {".qc.tab"} and set(off) <= set(on) and len(off) >= 5
    assert all(on[k] == off[k] for k in off), [k for k in off if on[k] != off[k]]
    assert not os.path.exists(paths["off"] + ".qc.tab")


def test_two_ranks_and_the_host_ingest_write_the_same_file(jobs):
    fx, bam, fa, d, paths, r, ranks = jobs
    one = open(paths["on"] + ".qc.tab", "rb").read()
    assert open(paths["ranks"] + ".qc.tab", "rb").read() == one
    assert open(paths["host"] + ".qc.tab", "rb").read() == one
    line = [l for l in r.stdout.split("\n") if l.startswith("qc tables:")]
    assert [l for l in ranks[0][1].split("\n") if l.startswith("qc tables:")] == line
    assert not [l for l in ranks[1][1].split("\n") if l.startswith("qc tables:")]


def test_any_other_value_of_the_switch_is_an_error(jobs):
    fx, bam, fa, d, paths, r, ranks = jobs
    bad = _job(bam, fa, paths["bad"], fx, timeout=120, TIDDIT_QC="2")
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == ["error, TIDDIT_QC=2: the switch is 1 or unset"]
    assert not os.path.exists(paths["bad"] + "_tiddit") and not os.path.exists(paths["bad"] + ".qc.tab")
