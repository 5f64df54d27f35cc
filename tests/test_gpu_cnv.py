"""`TIDDIT_CNV` on the GPU: the two device stages of csrc/tdt_cnv.hip — the CNV bins (``tdt_cnv_bins``) and the chunked Viterbi
segmentation (``tdt_cnv_viterbi``) — against the literal references of tests/cnv_cases.py on every aimed case, each through the host
entry and again through the ``_device`` entry on caller-owned, poisoned, padded outputs; every argument refusal, outputs untouched;
the stage on made-up bins (``tiddit_cnv.main``); and the switch end to end on the sv_e2e_small fixture, every job a fresh child process
under its own time limit.  All comparisons are exact equality.

Every test of this file fails on the parent commit: the symbols, the module and the switch do not exist there."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cnv_cases as C
from sv_e2e_common import load_fixture, materialise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("TIDDIT_VARIANTS", "TIDDIT_GENOTYPE", "TIDDIT_GENOTYPE_DEPTH", "TIDDIT_DEPTH_DIST", "TIDDIT_CNV", "TIDDIT_FORCE_DIST", "TIDDIT_COV_TRACK",
            "WORLD_SIZE", "RANK", "LOCAL_RANK")
ENTRIES = ("host", "device")
PAD = 64
PAIRS = [("bins", i, e) for i in range(len(C.BINS_CASES)) for e in ENTRIES] + [("viterbi", i, e) for i in range(len(C.VITERBI_CASES)) for e in ENTRIES]


def _id(pair):
    kind, i, entry = pair
    return "%s-%s-%s" % (kind, (C.BINS_CASES if kind == "bins" else C.VITERBI_CASES)[i]["name"], entry)


def test_the_count_of_case_entry_pairs():
    assert len(PAIRS) == 2 * 18 + 2 * 57 == 150


# ---- the two stages, both entries ---------------------------------------------------------------------------------------------
def _padded(n, dtype, poison):
    """a device array of n elements inside a poisoned allocation with PAD elements either side -> (whole, view)"""
    import torch
    whole = torch.full((n + 2 * PAD,), poison, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + n]


def _untouched(whole, n, poison):
    h = whole.cpu().numpy()
    return (h[:PAD] == poison).all() and (h[PAD + n:] == poison).all()


def _bins(case, entry, ctx=None):
    import torch
    from tiddit_amd import _native, tiddit_cnv
    cov, gc, table, E = C.bins_arrays(case)
    if entry == "host":
        return tiddit_cnv.cnv_bins(cov, gc, table, E, unit=case["unit"], ctx=ctx)
    ctx = ctx or _native.default_context()
    total = sum(-(-int(r[1]) // int(r[2])) for r in table)
    d_cov, d_gc, d_E = torch.from_numpy(cov).cuda(), torch.from_numpy(gc).cuda(), torch.from_numpy(E).cuda()
    whole, d_x = _padded(total, torch.int32, -77)
    torch.cuda.synchronize()
    _native.check(ctx.lib.tdt_cnv_bins_device(ctx.handle, d_cov.data_ptr(), d_gc.data_ptr(), len(cov), _native.ptr(table), len(table), d_E.data_ptr(),
                                              case["unit"], d_x.data_ptr()))
    assert _untouched(whole, total, -77)
    return d_x.cpu().numpy()


def _viterbi(case, entry, ctx=None):
    import torch
    from tiddit_amd import _native, tiddit_cnv
    x, table = C.viterbi_arrays(case)
    if entry == "host":
        return tiddit_cnv.viterbi(x, table, ctx=ctx)
    ctx = ctx or _native.default_context()
    d_x = torch.from_numpy(x).cuda()
    whole, d_s = _padded(len(x), torch.int8, -9)
    torch.cuda.synchronize()
    _native.check(ctx.lib.tdt_cnv_viterbi_device(ctx.handle, d_x.data_ptr(), len(x), _native.ptr(table), len(table), C.UNIT, C.CAP, C.LAMBDA,
                                                 d_s.data_ptr()))
    assert _untouched(whole, len(x), -9)
    return d_s.cpu().numpy()


@pytest.mark.parametrize("pair", PAIRS, ids=[_id(p) for p in PAIRS])
def test_the_device_equals_the_reference(pair):
    kind, i, entry = pair
    if kind == "bins":
        case = C.BINS_CASES[i]
        got, want = _bins(case, entry), np.concatenate(C.bins_reference(case))
        assert got.dtype == np.int32
    else:
        case = C.VITERBI_CASES[i]
        got, want = _viterbi(case, entry), np.concatenate([s for s, _, _ in C.viterbi_reference(case)])
        assert got.dtype == np.int8
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert not len(bad), (case["name"], entry, len(bad), [(int(k), int(got[k]), int(want[k])) for k in bad[:8]])


def test_two_calls_on_one_context_and_a_context_of_its_own():
    """a long call, a short one, the long one again — on the default context and on a fresh one: the carved scratch holds nothing over"""
    from tiddit_amd import _native
    by = {c["name"]: c for c in C.VITERBI_CASES}
    big, small, multi = by["T=2L+1"], by["stay ties with jump"], by["six contigs"]
    for ctx in (None, _native.Context(_native.default_context().device)):
        for case in (big, small, multi, big):
            for entry in ENTRIES:
                assert np.array_equal(_viterbi(case, entry, ctx), np.concatenate([s for s, _, _ in C.viterbi_reference(case)])), case["name"]
        for case in (C.BINS_CASES[2], C.BINS_CASES[0], C.BINS_CASES[2]):
            for entry in ENTRIES:
                assert np.array_equal(_bins(case, entry, ctx), np.concatenate(C.bins_reference(case)))
        if ctx is not None:
            ctx.close()


def _refusals(call, good, variants, out_untouched):
    """good: the dict of arguments of a call that succeeds; variants: (changed arguments, expected code)"""
    for change, code in variants:
        args = dict(good, **change)
        assert call(**args) == code, (change, code)
        assert out_untouched(), change


@pytest.mark.parametrize("entry", ENTRIES)
def test_bins_refusals_leave_the_output_untouched(entry):
    import torch
    from tiddit_amd import _native
    ctx = _native.default_context()
    lib = ctx.lib
    case = next(c for c in C.BINS_CASES if c["family"] == "ploidy")
    cov, gc, table, E = C.bins_arrays(case)
    total = sum(-(-int(r[1]) // int(r[2])) for r in table)
    if entry == "host":
        out = np.full(total + 1, -7, dtype=np.int32)
        keep = (cov, gc, E)
        p_cov, p_gc, p_E, p_x = cov.ctypes.data, gc.ctypes.data, E.ctypes.data, out.ctypes.data
        fn, untouched, result = lib.tdt_cnv_bins, (lambda: (out == -7).all()), (lambda: out[:total])
    else:
        keep = (torch.from_numpy(cov).cuda(), torch.from_numpy(gc).cuda(), torch.from_numpy(E).cuda(), torch.full((total + 1,), -7, dtype=torch.int32, device="cuda"))
        p_cov, p_gc, p_E, p_x = (t.data_ptr() for t in keep)
        torch.cuda.synchronize()
        fn, untouched, result = lib.tdt_cnv_bins_device, (lambda: bool((keep[3] == -7).all())), (lambda: keep[3].cpu().numpy()[:total])

    def call(ctx_h, cov, gc, n, table, nseg, E, unit, x):
        return fn(ctx_h, cov, gc, n, None if table is None else _native.ptr(table), nseg, E, unit, x)

    def row(s, col, v):
        t = table.copy()
        t[s, col] = v
        return {"table": t}, -3
    good = dict(ctx_h=ctx.handle, cov=p_cov, gc=p_gc, n=len(cov), table=table, nseg=len(table), E=p_E, unit=C.UNIT, x=p_x)
    _refusals(call, good, [({"ctx_h": None}, -1), ({"cov": None}, -1), ({"gc": None}, -1), ({"table": None}, -1), ({"E": None}, -1), ({"x": None}, -1),
                           ({"cov": p_cov + 4}, -1), ({"E": p_E + 4}, -1), ({"x": p_x + 2}, -1), ({"n": -1}, -1), ({"nseg": -1}, -1), ({"unit": 0}, -1),
                           ({"unit": (1 << 20) + 1}, -1), ({"n": len(cov) - 1}, -3), row(2, 0, -1), row(2, 1, -1), row(5, 1, table[5, 1] + 1),
                           row(1, 2, 0), row(1, 2, 65), row(3, 3, 0), row(3, 3, 7), row(4, 4, table[4, 4] + 1), row(0, 4, 1),
                           ({"n": 0, "cov": None, "gc": None, "x": None}, 0), ({"nseg": 0, "table": None, "E": None, "x": None}, 0)],
              untouched)
    for change, _ in (row(2, 0, -1), row(1, 2, 65), row(4, 4, table[4, 4] + 1)):
        assert call(**dict(good, **change)) == -3 and "tdt_cnv_bins" in lib.tdt_last_error().decode()
    assert call(**good) == 0                              # (and the context is still good)
    assert np.array_equal(result(), np.concatenate(C.bins_reference(case))) and (entry == "device" or out[total] == -7)
    del keep


@pytest.mark.parametrize("entry", ENTRIES)
def test_viterbi_refusals_leave_the_output_untouched(entry):
    import torch
    from tiddit_amd import _native
    ctx = _native.default_context()
    lib = ctx.lib
    case = next(c for c in C.VITERBI_CASES if c["name"] == "six contigs")
    x, table = C.viterbi_arrays(case)
    n = len(x)
    if entry == "host":
        out = np.full(n + 1, -7, dtype=np.int8)
        keep = (x,)
        p_x, p_s = x.ctypes.data, out.ctypes.data
        fn, untouched, result = lib.tdt_cnv_viterbi, (lambda: (out == -7).all()), (lambda: out[:n])
    else:
        keep = (torch.from_numpy(x).cuda(), torch.full((n + 1,), -7, dtype=torch.int8, device="cuda"))
        p_x, p_s = (t.data_ptr() for t in keep)
        torch.cuda.synchronize()
        fn, untouched, result = lib.tdt_cnv_viterbi_device, (lambda: bool((keep[1] == -7).all())), (lambda: keep[1].cpu().numpy()[:n])

    def call(ctx_h, x, n, table, nseg, unit, cap, lam, state):
        return fn(ctx_h, x, n, None if table is None else _native.ptr(table), nseg, unit, cap, lam, state)

    def row(s, col, v):
        t = table.copy()
        t[s, col] = v
        return {"table": t}, -3
    good = dict(ctx_h=ctx.handle, x=p_x, n=n, table=table, nseg=len(table), unit=C.UNIT, cap=C.CAP, lam=C.LAMBDA, state=p_s)
    _refusals(call, good, [({"ctx_h": None}, -1), ({"x": None}, -1), ({"table": None}, -1), ({"state": None}, -1), ({"x": p_x + 2}, -1), ({"n": -1}, -1),
                           ({"nseg": -1}, -1), ({"unit": 0}, -1), ({"cap": -1}, -1), ({"lam": -1}, -1), ({"cap": (1 << 28) + 1}, -1),
                           ({"lam": (1 << 28) + 1}, -1), ({"n": n - 1}, -3), ({"n": n + 1}, -3), row(2, 0, table[2, 0] + 1), row(1, 1, -1),
                           row(5, 1, table[5, 1] + 1), row(3, 2, -1), row(3, 2, 8), ({"nseg": len(table) - 1}, -3),
                           ({"n": 0, "x": None, "state": None}, 0), ({"nseg": 0, "table": None, "x": None, "state": None}, 0)], untouched)
    assert call(**dict(good, **row(3, 2, 8)[0])) == -3 and "tdt_cnv_viterbi" in lib.tdt_last_error().decode()
    assert call(**good) == 0                              # (and the context is still good)
    assert np.array_equal(result(), np.concatenate([s for s, _, _ in C.viterbi_reference(case)])) and (entry == "device" or out[n] == -7)
    del keep


# ---- the stage on made-up bins ------------------------------------------------------------------------------------------------
def test_the_stage_on_the_planted_job(tmp_path, capsys):
    """tiddit_cnv.main on the bins of tests/cnv_cases.py's planted job: the file the literal reference writes — the two planted
    segments, the class fallback on both sides of MIN_CLASS, every reason to skip a contig"""
    from tiddit_amd import tiddit_cnv
    coverage, gcs, library, contigs, length, min_contig, W = C.planted_job()
    want, skipped, _ = C.ref_job(coverage, gcs, library, contigs, length, min_contig, W)
    prefix = str(tmp_path / "planted")
    segments = tiddit_cnv.main(coverage, gcs, dict(library), contigs, length, min_contig, W, prefix)
    got = open(prefix + ".cnv.bed").read()
    assert got == want and got.count("\n") == 5 and len(segments) == 4
    notes = [l for l in capsys.readouterr().out.split("\n") if l.startswith("note: TIDDIT_CNV skips")]
    assert notes == ["note: TIDDIT_CNV skips " + ", ".join(skipped)]
    assert any(k.startswith("CNV segmentation") for k in tiddit_cnv.STAGE_SECONDS)
    # every bin size at which K changes the layout: one 50-bp bin per CNV bin, and the largest
    for W2 in (50, 3200):
        want2 = C.ref_job(coverage, gcs, library, ["chrB", "chrC"], length, min_contig, W2)[0]
        tiddit_cnv.main(coverage, gcs, dict(library), ["chrB", "chrC"], length, min_contig, W2, prefix + str(W2))
        assert open(prefix + str(W2) + ".cnv.bed").read() == want2
    # nothing to process: the header alone
    tiddit_cnv.main(coverage, gcs, dict(library), ["tiny", "none"], length, min_contig, W, prefix + "none")
    assert open(prefix + "none.cnv.bed").read() == C.HEADER


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------
def _job(bam, fa, out, fx, timeout=600, **env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    return subprocess.run([sys.executable, "-m", "tiddit_amd", "--sv", "--bam", bam, "--ref", fa, "-o", out, "--skip_assembly", "-s",
                           str(fx["params"]["n_reads_stats"])], cwd=REPO, env=e, capture_output=True, text=True, timeout=timeout)


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


def _vcf(path):
    """the file without its ##TIDDITcmd line (which names the job's own prefix)"""
    return [l for l in open(path).read().split("\n") if not l.startswith("##TIDDITcmd=")]


DIST = dict(TIDDIT_FORCE_DIST="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1")


@pytest.fixture(scope="module")
def jobs(golden_dir, tmp_path_factory):
    fx = load_fixture(golden_dir, "sv_e2e_small.json")
    d = str(tmp_path_factory.mktemp("cnv"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    paths = {n: os.path.join(d, n) for n in ("off", "on", "w50", "var", "var_on", "dist_on")}
    _ok(_job(bam, fa, paths["off"], fx))
    _ok(_job(bam, fa, paths["on"], fx, TIDDIT_CNV="1"))
    _ok(_job(bam, fa, paths["w50"], fx, TIDDIT_CNV="50"))
    _ok(_job(bam, fa, paths["var"], fx, TIDDIT_VARIANTS="1"))
    _ok(_job(bam, fa, paths["var_on"], fx, TIDDIT_VARIANTS="1", TIDDIT_CNV="1"))
    _ok(_job(bam, fa, paths["dist_on"], fx, TIDDIT_CNV="1", MASTER_PORT="29741", **DIST))
    return fx, bam, fa, d, paths


def test_the_file_equals_the_reference_on_the_job_s_own_bins(jobs, tmp_path):
    """the bins as the job gets them — tiddit_signal.main, tiddit_gc.main and determine_ploidy in this process on the same files —
    through the literal reference"""
    from tiddit_amd import bamio, tiddit_coverage_analysis, tiddit_gc, tiddit_signal, tiddit_stats
    fx, bam, fa, d, paths = jobs
    rd = bamio.BamReader(bam)
    header = rd.header
    rd.close()
    contigs = [c["SN"] for c in header["SQ"]]
    length = {c["SN"]: c["LN"] for c in header["SQ"]}
    library = tiddit_stats.statistics(bam, fa, 5, 100000, fx["params"]["n_reads_stats"])
    prefix = str(tmp_path / "inproc")
    os.makedirs(prefix + "_tiddit/clips")
    try:
        sample = header["RG"][0]["SM"]
    except Exception:
        sample = os.path.basename(bam).split(".")[0]
    cov = tiddit_signal.main(bam, fa, prefix, 5, library["percentile_insert_size"], sample, 1, 10000, False, 60, 25)
    tiddit_signal.finish_writes()
    gc = tiddit_gc.main(fa, contigs, 1, 50, 0.5)
    library = tiddit_coverage_analysis.determine_ploidy(cov, contigs, library, 2, prefix, None, fa, 50, header, gc)
    assert open(prefix + ".ploidies.tab").read() == open(paths["on"] + ".ploidies.tab").read()
    for W, name in ((500, "on"), (50, "w50")):
        want, skipped, tracks = C.ref_job(cov, gc, library, contigs, length, 10000, W)
        got = open(paths[name] + ".cnv.bed").read()
        assert got == want and got.startswith(C.HEADER) and len(tracks) >= 1, name
    assert open(paths["var_on"] + ".cnv.bed").read() == open(paths["on"] + ".cnv.bed").read()


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    fx, bam, fa, d, paths = jobs
    off, on, w50 = _files(paths["off"]), _files(paths["on"]), _files(paths["w50"])
    for with_switch in (on, w50):
        assert set(with_switch) - set(off) == {".cnv.bed"} and set(off) <= set(with_switch)
        assert all(with_switch[k] == off[k] for k in off), [k for k in off if with_switch[k] != off[k]]
    assert not os.path.exists(paths["off"] + ".cnv.bed") and not os.path.exists(paths["var"] + ".cnv.bed")
    var, var_on = _files(paths["var"]), _files(paths["var_on"])
    assert set(var_on) - set(var) == {".cnv.bed"} and set(var) <= set(var_on)
    assert _vcf(paths["var_on"] + ".vcf") == _vcf(paths["var"] + ".vcf") and len(_vcf(paths["var"] + ".vcf")) > 20
    assert all(var_on[k] == var[k] for k in var if k != ".vcf")


def test_the_n_rank_job_writes_the_same_bytes(jobs):
    fx, bam, fa, d, paths = jobs
    assert open(paths["dist_on"] + ".cnv.bed", "rb").read() == open(paths["on"] + ".cnv.bed", "rb").read()
    assert open(paths["dist_on"] + ".candidates.tab", "rb").read() == open(paths["on"] + ".candidates.tab", "rb").read()


@pytest.mark.parametrize("value", ["0", "75", "3250", "x"])
def test_a_bad_value_is_refused_with_nothing_made(jobs, value):
    fx, bam, fa, d, paths = jobs
    out = os.path.join(d, "refused" + value)
    r = _job(bam, fa, out, fx, timeout=300, TIDDIT_CNV=value)
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    errors = [l for l in r.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_CNV=%s:" % value)
    assert not os.path.exists(out + "_tiddit") and not os.path.exists(out + ".cnv.bed") and not _files(out)
