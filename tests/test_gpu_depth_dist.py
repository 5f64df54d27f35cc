"""`TIDDIT_DEPTH_DIST=1` on the GPU: the kernel (``tdt_depth_dist``, csrc/tdt_depth_dist.hip) through ``EvidenceStore.depth_dist()``
against the numpy reference of tests/depth_dist_cases.py on every aimed case — equality is exact, these are integers — its refusals,
and the switch end to end on the sv_e2e_small fixture, every job a fresh child process under its own time limit.

Every test of this file fails on the parent commit: the symbol and the switch do not exist there."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_dist_cases as D
from sv_e2e_common import load_fixture, materialise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("TIDDIT_VARIANTS", "TIDDIT_GENOTYPE", "TIDDIT_GENOTYPE_DEPTH", "TIDDIT_DEPTH_DIST", "TIDDIT_FORCE_DIST", "TIDDIT_COV_TRACK", "WORLD_SIZE",
            "RANK", "LOCAL_RANK")


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _store(case):
    from tiddit_amd import tiddit_region
    lengths, records = case["lengths"], case["records"]
    store = tiddit_region.EvidenceStore("case", ["c%d" % t for t in range(len(lengths))], lengths, D.MIN_Q, D.MAX_INS, capacity=case["capacity"])
    cuts = [0] + list(case["batches"]) + [len(records)]
    for lo, hi in zip(cuts, cuts[1:]):
        if hi > lo:
            store.add_host_batch(D.columns(records[lo:hi]))
    return store


def test_the_case_list_is_the_one_pinned_on_the_cpu():
    assert len(D.CASES) == 11


@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_depth_dist_equals_the_reference(case):
    lengths, records = case["lengths"], case["records"]
    want = D.reference(lengths, records)
    store = _store(case)
    try:
        assert store.n == len(records)
        assert store.spans().tolist() == D.spans(lengths, records)
        table = None
        if case["order"] is not None:
            table = store.contig_table()[case["order"]]
            want = want[case["order"]]
            lengths = [lengths[i] for i in case["order"]]
        got = store.depth_dist(table=table)
        assert got.dtype == np.int64 and got.shape == want.shape == (len(lengths), D.CAP + 4)
        for t, LN in enumerate(lengths):
            assert got[t, :D.CAP + 1].sum() == LN, (case["name"], t)
            bad = np.flatnonzero(got[t] != want[t])
            assert not len(bad), (case["name"], t, [(int(k), int(got[t, k]), int(want[t, k])) for k in bad[:8]])
        if case["family"] == "state":
            # the same call again, a call with other rows in between, and again: nothing is left behind between calls
            assert np.array_equal(store.depth_dist(table=table), want)
            rev = store.contig_table()[::-1]
            assert np.array_equal(store.depth_dist(table=rev), D.reference(case["lengths"], records)[::-1])
            assert np.array_equal(store.depth_dist(table=table), want)
    finally:
        store.close()


def test_refused_arguments_leave_the_output_untouched():
    from tiddit_amd import _native
    case = next(c for c in D.CASES if c["family"] == "multi")
    store = _store(case)
    try:
        ctx, lib = store.ctx, store.ctx.lib
        good = np.ascontiguousarray(store.contig_table())
        n = len(good)
        out = np.full((n, D.CAP + 4), -7, dtype=np.int64)
        P = _native.ptr

        def call(ctx_h, store_h, tab, rows, cap, o):
            return lib.tdt_depth_dist(ctx_h, store_h, P(tab) if tab is not None else None, rows, cap, P(o) if o is not None else None)
        outside = good.copy()
        outside[2, 1] = store.n - outside[2, 0] + 1                  # one record past the end of the store
        before = good.copy()
        before[1, 0] = -1
        negative = good.copy()
        negative[3, 4] = -5
        for args, code in (((None, store.handle, good, n, D.CAP, out), -1), ((ctx.handle, None, good, n, D.CAP, out), -1),
                           ((ctx.handle, store.handle, None, n, D.CAP, out), -1), ((ctx.handle, store.handle, good, n, D.CAP, None), -1),
                           ((ctx.handle, store.handle, good, n, D.CAP - 1, out), -1), ((ctx.handle, store.handle, good, n, D.CAP + 1, out), -1),
                           ((ctx.handle, store.handle, good, -1, D.CAP, out), -1),
                           ((ctx.handle, store.handle, outside, n, D.CAP, out), -3), ((ctx.handle, store.handle, before, n, D.CAP, out), -3),
                           ((ctx.handle, store.handle, negative, n, D.CAP, out), -3),
                           ((ctx.handle, store.handle, good, 0, D.CAP, out), 0), ((ctx.handle, store.handle, None, 0, D.CAP, None), 0)):
            assert call(*args) == code, (args[3:5], code)
            assert (out == -7).all()
        with pytest.raises(_native.TdtError) as e:
            store.depth_dist(table=outside)
        assert e.value.code == -3 and "tdt_depth_dist" in str(e.value)
        assert call(ctx.handle, store.handle, good, n, D.CAP, out) == 0          # (and the store is still good)
        assert np.array_equal(out, D.reference(case["lengths"], case["records"]))
    finally:
        store.close()


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


def _host_reference(bam, min_q):
    """the table from the host-decoded columns of the file itself (bamio.BamReader), never from the store"""
    from tiddit_amd import bamio
    rd = bamio.BamReader(bam)
    names, lengths = list(rd.references), [int(x) for x in rd.lengths]
    diff = [np.zeros(n + 1, dtype=np.int64) for n in lengths]
    n_kept = 0
    for b in rd.batches():
        tid, flag = np.asarray(b.tid), np.asarray(b.flag).astype(np.int64)
        keep = (tid >= 0) & ((flag & 0x404) == 0) & (np.asarray(b.mapq) >= min_q)
        for t in np.unique(tid[keep]):
            m = keep & (tid == t)
            s = np.maximum(np.asarray(b.pos)[m].astype(np.int64), 0)
            e = np.minimum(np.asarray(b.end)[m].astype(np.int64), lengths[t])
            ok = e > s
            np.add.at(diff[t], s[ok], 1)
            np.add.at(diff[t], e[ok], -1)
            n_kept += int(ok.sum())
    rd.close()
    assert n_kept > 1000
    return names, lengths, np.stack([D._row(np.cumsum(d[:-1])) for d in diff])


@pytest.fixture(scope="module")
def jobs(golden_dir, tmp_path_factory):
    fx = load_fixture(golden_dir, "sv_e2e_small.json")
    d = str(tmp_path_factory.mktemp("depthdist"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    paths = {n: os.path.join(d, n) for n in ("off", "on", "first", "both", "all")}
    _ok(_job(bam, fa, paths["off"], fx))
    r = _ok(_job(bam, fa, paths["on"], fx, TIDDIT_DEPTH_DIST="1"))
    _ok(_job(bam, fa, paths["first"], fx, TIDDIT_VARIANTS="1"))
    _ok(_job(bam, fa, paths["both"], fx, TIDDIT_VARIANTS="1", TIDDIT_GENOTYPE=paths["first"] + ".vcf"))
    _ok(_job(bam, fa, paths["all"], fx, TIDDIT_VARIANTS="1", TIDDIT_GENOTYPE=paths["first"] + ".vcf", TIDDIT_DEPTH_DIST="1"))
    return fx, bam, fa, d, paths, r


def test_both_files_equal_the_host_reference(jobs, tmp_path):
    from tiddit_amd import tiddit_depth_dist
    fx, bam, fa, d, paths, r = jobs
    names, lengths, table = _host_reference(bam, 5)                     # (the job's default -q, the store's min_q)
    assert table[:, D.CAP + 2].max() > 5 and (table[:, :D.CAP + 1].sum(axis=1) == lengths).all()
    want = str(tmp_path / "want")
    tiddit_depth_dist.write_files(want, names, lengths, table)
    for ext in (".depth_dist.tab", ".depth_summary.tab"):
        got = open(paths["on"] + ext, "rb").read()
        assert len(got) > 50 and got == open(want + ext, "rb").read(), ext
        assert open(paths["all"] + ext, "rb").read() == got, ext


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    fx, bam, fa, d, paths, r = jobs
    off, on = _files(paths["off"]), _files(paths["on"])
    assert set(on) - set(off) == {".depth_dist.tab", ".depth_summary.tab"} and set(off) <= set(on)
    assert all(on[k] == off[k] for k in off), [k for k in off if on[k] != off[k]]
    assert not os.path.exists(paths["off"] + ".depth_dist.tab") and not os.path.exists(paths["off"] + ".depth_summary.tab")
    assert not os.path.exists(paths["both"] + ".depth_dist.tab") and not os.path.exists(paths["both"] + ".depth_summary.tab")


def test_the_store_survives_for_the_variant_and_genotype_stages(jobs):
    fx, bam, fa, d, paths, r = jobs
    both, all_ = _files(paths["both"]), _files(paths["all"])
    assert set(all_) - set(both) == {".depth_dist.tab", ".depth_summary.tab"} and set(both) <= set(all_)
    assert _vcf(paths["all"] + ".vcf") == _vcf(paths["both"] + ".vcf") and len(_vcf(paths["both"] + ".vcf")) > 20
    assert _vcf(paths["all"] + ".genotyped.vcf") == _vcf(paths["both"] + ".genotyped.vcf")
    assert all(all_[k] == both[k] for k in both if k not in (".vcf", ".genotyped.vcf"))


def test_a_bad_value_and_the_n_rank_job_are_refused_before_anything_is_made(jobs):
    fx, bam, fa, d, paths, r = jobs
    out = os.path.join(d, "refused")
    r = _job(bam, fa, out, fx, timeout=300, TIDDIT_DEPTH_DIST="2")
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    errors = [l for l in r.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_DEPTH_DIST=2")
    assert not os.path.exists(out + "_tiddit")
    r = _job(bam, fa, out, fx, timeout=300, TIDDIT_DEPTH_DIST="1", TIDDIT_FORCE_DIST="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
             MASTER_ADDR="127.0.0.1", MASTER_PORT="29733")
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    errors = [l for l in r.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_DEPTH_DIST ")
    assert "init_process_group" not in r.stderr and not os.path.exists(out + "_tiddit")
    assert not os.path.exists(out + ".depth_dist.tab")
