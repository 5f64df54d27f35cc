"""`TIDDIT_ALLELES` on the GPU: the kernel (csrc/tdt_alleles.hip) on every aimed case of tests/alleles_cases.py through both entries —
``tdt_alleles_push`` on host columns, and ``tdt_alleles_push_device`` on the batches a ``DeviceBamReader`` decodes from a small BAM
written from the case's records — against the case's claim and the numpy restatement (integers: equality is exact); the handle's
state, its refusals, and the switch end to end on the sv_e2e_small fixture, every job a fresh child process under its own time limit.

Every test of this file fails on the parent commit: the symbols and the switch do not exist there."""
import hashlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import alleles_cases as AC
from sv_e2e_common import load_fixture, materialise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("TIDDIT_VARIANTS", "TIDDIT_GENOTYPE", "TIDDIT_GENOTYPE_DEPTH", "TIDDIT_DEPTH_DIST", "TIDDIT_FORCE_DIST", "TIDDIT_COV_TRACK", "TIDDIT_CNV",
            "TIDDIT_ALLELES", "TIDDIT_ALLELES_MIN_BQ", "TIDDIT_HOST_INGEST", "TIDDIT_DIST_BACKEND", "WORLD_SIZE", "RANK", "LOCAL_RANK")
PAIRS = []                       # the (case, entry) pairs that ran and passed


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _counter(case):
    from tiddit_amd import tiddit_alleles
    pos, off = AC.table_of(case)
    return tiddit_alleles.AlleleCounter(pos, off, case["min_q"], case["min_bq"])


def _same(got, want, what):
    bad = np.argwhere(got[0] != want[0])
    assert not len(bad), (what, [(int(k), int(c), int(got[0][k, c]), int(want[0][k, c])) for k, c in bad[:8]])
    assert tuple(got[1:]) == tuple(want[1:]), (what, got[1:], want[1:])


@pytest.fixture(scope="module")
def wanted():
    out = {}
    for c in AC.CASES:
        claim, ref = AC.expected(c), AC.reference(c)
        assert np.array_equal(claim[0], ref[0]) and claim[1:] == ref[1:], c["name"]
        out[c["name"]] = ref
    return out


@pytest.mark.parametrize("case", AC.CASES, ids=[c["name"] for c in AC.CASES])
def test_push_equals_the_reference(case, wanted):
    h = _counter(case)
    try:
        for b in AC.batches(case):
            h.push_host_batch(b)
        _same(h.counts(), wanted[case["name"]], case["name"])
    finally:
        h.close()
    PAIRS.append((case["name"], "push"))


def _write_bam(path, case):
    from tiddit_amd import bamio
    b = AC.build(case, padding=False)
    w = bamio.BamWriter(path, [("c%d" % t, ln) for t, ln in enumerate(case["lengths"])])
    w._buf += b.raw.tobytes()                     # the case's records as they are, qualities included (BamWriter.write takes none)
    w.close()


@pytest.mark.parametrize("case", [c for c in AC.CASES if c["reader_ok"]], ids=[c["name"] for c in AC.CASES if c["reader_ok"]])
def test_push_device_from_a_small_bam_equals_the_reference(case, wanted, tmp_path):
    from tiddit_amd import bamio
    path = str(tmp_path / "case.bam")
    _write_bam(path, case)
    rd = bamio.DeviceBamReader(path)
    h = None
    try:
        from tiddit_amd import tiddit_alleles
        pos, off = AC.table_of(case)
        h = tiddit_alleles.AlleleCounter(pos, off, case["min_q"], case["min_bq"], ctx=rd.ctx)
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
    assert len(AC.CASES) == AC.N_CASES == 44
    assert len(set(PAIRS)) == 44 + 40, len(set(PAIRS))


def test_state_accumulates_reads_between_pushes_resets_and_keeps_handles_apart(wanted):
    case = next(c for c in AC.CASES if c["family"] == "state")
    other = next(c for c in AC.CASES if c["name"] == "contention 65 reads mixed bases")
    first, second = AC.batches(case)
    pos, off = AC.table_of(case)
    part, stats = np.zeros((len(pos), 8), dtype=np.uint32), [0, 0]
    AC.reference_batch(part, stats, pos, off, first, case["min_q"], case["min_bq"])
    assert 0 < part.sum() < wanted[case["name"]][0].sum()
    h, g = _counter(case), _counter(other)
    try:
        assert h.ctx is g.ctx
        assert not h.counts()[0].any() and h.counts()[1:] == (0, 0)
        h.push_host_batch(first)
        g.push_host_batch(AC.build(other))
        _same(h.counts(), (part, stats[0], stats[1]), "first push")
        h.push_host_batch(second)
        _same(h.counts(), wanted[case["name"]], "both pushes")
        _same(g.counts(), wanted[other["name"]], "the other handle")
        h.reset()
        assert not h.counts()[0].any() and h.counts()[1:] == (0, 0)
        _same(g.counts(), wanted[other["name"]], "the other handle after the reset")
        for b in (second, first):
            h.push_host_batch(b)
        _same(h.counts(), wanted[case["name"]], "after the reset, in the other order")
    finally:
        h.close()
        g.close()


def test_counts_device_equals_counts():
    import torch
    case = next(c for c in AC.CASES if c["name"] == "sizes a batch of 257 reads")
    h = _counter(case)
    try:
        h.push_host_batch(AC.build(case))
        table, used, bad = h.counts()
        d_out = torch.full((len(table), 8), 7, dtype=torch.int32, device="cuda")
        d_stat = torch.full((2,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert h.ctx.lib.tdt_alleles_counts_device(h.handle, d_out.data_ptr(), d_stat.data_ptr()) == 0
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), table) and d_stat.cpu().tolist() == [used, bad]
        assert h.ctx.lib.tdt_alleles_counts_device(h.handle, d_out.data_ptr() + 2, d_stat.data_ptr()) == -1
        assert h.ctx.lib.tdt_alleles_counts_device(None, d_out.data_ptr(), d_stat.data_ptr()) == -1
    finally:
        h.close()


def test_refused_arguments_leave_the_outputs_untouched():
    import ctypes
    from tiddit_amd import _native
    case = next(c for c in AC.CASES if c["name"] == "filters flags mapq tid contig")
    ctx = _native.default_context()
    lib, P = ctx.lib, _native.ptr
    pos, off = AC.table_of(case)
    n_contigs = len(off) - 1

    def create(c, sp, so, nc, mq, mbq, want):
        h = ctypes.c_void_p(0x5a5a)
        rc = lib.tdt_alleles_create(c, P(sp) if sp is not None else None, P(so) if so is not None else None, nc, mq, mbq, ctypes.byref(h))
        assert rc == want, (rc, want)
        if rc:
            assert h.value == 0x5a5a
        return h
    create(None, pos, off, n_contigs, 20, 13, -1)
    create(ctx.handle, None, off, n_contigs, 20, 13, -1)
    create(ctx.handle, pos, None, n_contigs, 20, 13, -1)
    create(ctx.handle, pos, off, -1, 20, 13, -1)
    assert lib.tdt_alleles_create(ctx.handle, P(pos), P(off), n_contigs, 20, 13, None) == -1
    create(ctx.handle, pos, off + 1, n_contigs, 20, 13, -1)                                         # offsets start at 0
    create(ctx.handle, pos, np.array([0, 2, 1], dtype=np.int64), n_contigs, 20, 13, -1)             # ... and do not decrease
    create(ctx.handle, np.array([7, 7], dtype=np.int32), np.array([0, 2, 2], dtype=np.int64), 2, 20, 13, -1)   # unique
    create(ctx.handle, np.array([8, 7], dtype=np.int32), np.array([0, 2, 2], dtype=np.int64), 2, 20, 13, -1)   # sorted
    create(ctx.handle, np.array([-1, 7], dtype=np.int32), np.array([0, 2, 2], dtype=np.int64), 2, 20, 13, -1)  # >= 0
    create(ctx.handle, pos, off, n_contigs, 20, -1, -3)
    create(ctx.handle, pos, off, n_contigs, 20, 94, -3)
    create(ctx.handle, pos, np.array([0, 1, 1 << 28], dtype=np.int64), n_contigs, 20, 13, -3)       # 2^28 sites
    empty = create(ctx.handle, None, np.zeros(3, dtype=np.int64), 2, 20, 13, 0)                     # no sites at all: a handle that counts nothing
    h = create(ctx.handle, pos, off, n_contigs, 20, 13, 0)
    try:
        b = AC.build(case)
        cols = [b.tid, b.pos, b.end, b.mapq, b.flag, b.rec_off]
        n = len(b)

        def push(hh, c, nn, raw, raw_len):
            return lib.tdt_alleles_push(hh, *[P(x) if x is not None else None for x in c], nn, P(raw) if raw is not None else None, raw_len)
        assert push(None, cols, n, b.raw, len(b.raw)) == -1
        for k in range(6):
            assert push(h, cols[:k] + [None] + cols[k + 1:], n, b.raw, len(b.raw)) == -1
        assert push(h, cols, n, None, len(b.raw)) == -1
        assert push(h, cols, 1 << 31, b.raw, len(b.raw)) == -1
        assert lib.tdt_alleles_push_device(None, None, 0, 0) == -1
        assert lib.tdt_alleles_push_device(h, None, 5, 100) == -1
        nulls = (ctypes.c_void_p * 14)()
        assert lib.tdt_alleles_push_device(h, nulls, 5, 100) == -1                                 # a batch without its columns
        out = np.full((len(pos), 8), 7, dtype=np.uint32)
        used, bad = ctypes.c_uint64(7), ctypes.c_uint64(7)
        assert lib.tdt_alleles_counts(None, P(out), ctypes.byref(used), ctypes.byref(bad)) == -1
        assert lib.tdt_alleles_counts(h, None, ctypes.byref(used), ctypes.byref(bad)) == -1
        assert (out == 7).all() and used.value == 7 and bad.value == 7
        assert lib.tdt_alleles_reset(None) == -1
        # nothing refused above counted anything; n = 0 and a handle without sites are no-ops; and the handle still works
        assert push(h, [None] * 6, 0, None, 0) == 0 and push(empty, cols, n, b.raw, len(b.raw)) == 0
        assert lib.tdt_alleles_counts(h, P(out), ctypes.byref(used), ctypes.byref(bad)) == 0
        assert not out.any() and used.value == 0 and bad.value == 0
        assert lib.tdt_alleles_counts(empty, None, ctypes.byref(used), None) == 0 and used.value == 0
        assert push(h, cols, n, b.raw, len(b.raw)) == 0
        assert lib.tdt_alleles_counts(h, P(out), None, None) == 0
        assert np.array_equal(out, AC.expected(case)[0])
        # a raw_len of 0: every read that holds a site is malformed, nothing is read
        assert lib.tdt_alleles_reset(h) == 0 and push(h, cols, n, None, 0) == 0
        assert lib.tdt_alleles_counts(h, P(out), ctypes.byref(used), ctypes.byref(bad)) == 0
        assert not out.any() and used.value == 0 and bad.value == case["used"]
    finally:
        assert lib.tdt_alleles_destroy(h) == 0 and lib.tdt_alleles_destroy(empty) == 0 and lib.tdt_alleles_destroy(None) == 0


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


def _write_sites(path, fa, contigs):
    """every 997th base of every contig, REF the reference base, ALT the next base of ACGT (a REF that is no ACGT base makes a row
    the reader skips)"""
    from tiddit_amd.fasta import FastaFile
    fasta = FastaFile(fa)
    n = 0
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for name, ln in contigs:
            seq = fasta.fetch(name).upper()
            for p in range(996, ln, 997):
                ref = seq[p]
                alt = "ACGT"[("ACGT".index(ref) + 1) % 4] if ref in "ACGT" else "A"
                f.write("%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (name, p + 1, ref, alt))
                n += 1
    return n


def _two_ranks(bam, fa, out, fx, sites):
    port = _port()
    procs = [subprocess.Popen(_argv(bam, fa, out, fx), cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=_env(TIDDIT_ALLELES=sites, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2",
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
    d = str(tmp_path_factory.mktemp("alleles"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    sites = os.path.join(d, "sites.vcf")
    n_rows = _write_sites(sites, fa, contigs)
    paths = {n: os.path.join(d, n) for n in ("off", "on", "host", "ranks")}
    _ok(_job(bam, fa, paths["off"], fx))
    r = _ok(_job(bam, fa, paths["on"], fx, TIDDIT_ALLELES=sites))
    _ok(_job(bam, fa, paths["host"], fx, TIDDIT_ALLELES=sites, TIDDIT_HOST_INGEST="1"))
    ranks = _two_ranks(bam, fa, paths["ranks"], fx, sites)
    return fx, bam, fa, d, paths, r, sites, n_rows, ranks


def test_the_file_equals_the_definition_on_the_host_readers_batches(jobs, tmp_path):
    from tiddit_amd import bamio, tiddit_alleles
    fx, bam, fa, d, paths, r, sites_path, n_rows, ranks = jobs
    rd = bamio.BamReader(bam)
    sites = tiddit_alleles.read_sites(sites_path, rd.references, rd.lengths)
    assert len(sites.rows) + sum(sites.skipped.values()) == n_rows and len(sites.rows) > 1000
    table, stats = np.zeros((len(sites), 8), dtype=np.int64), [0, 0]
    pairs = 0
    for b in rd.batches():
        # only the reads that can touch a site are walked in Python
        tid = np.asarray(b.tid).astype(np.int64)
        ok = tid >= 0
        lo, hi = np.zeros(len(tid), dtype=np.int64), np.zeros(len(tid), dtype=np.int64)
        for t in np.unique(tid[ok]):
            m = tid == t
            sp = sites.site_pos[sites.site_off[t]:sites.site_off[t + 1]]
            lo[m], hi[m] = np.searchsorted(sp, np.asarray(b.pos)[m]), np.searchsorted(sp, np.asarray(b.end)[m])
        only = np.flatnonzero(hi > lo)
        pairs += int((hi - lo)[only].sum())
        tiddit_alleles.count_batch(table, stats, sites.site_pos, sites.site_off, b, 5, 13, only=only)     # (the job's default -q)
    rd.close()
    assert 50_000 < pairs < 200_000 and stats[0] > 40_000 and stats[1] == 0
    assert table[:, :4].sum() > 40_000 and table[:, tiddit_alleles.LOWBQ].sum() > 0                    # (qualities 2 ... 40 around min_bq 13)
    want = str(tmp_path / "want.alleles.tab")
    tiddit_alleles.write_file(want, sites.rows, table)
    got = open(paths["on"] + ".alleles.tab", "rb").read()
    assert len(got) > 10_000 and got == open(want, "rb").read()
    line = [l for l in r.stdout.split("\n") if l.startswith("allele counts:")]
    assert line == [tiddit_alleles.summary_line(sites, stats[0], stats[1])]


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    fx, bam, fa, d, paths, r, sites, n_rows, ranks = jobs
    off, on = _files(paths["off"]), _files(paths["on"])
    assert set(on) - set(off) == {".alleles.tab"} and set(off) <= set(on) and len(off) >= 5
    assert all(on[k] == off[k] for k in off), [k for k in off if on[k] != off[k]]
    assert not os.path.exists(paths["off"] + ".alleles.tab")


def test_two_ranks_and_the_host_ingest_write_the_same_file(jobs):
    fx, bam, fa, d, paths, r, sites, n_rows, ranks = jobs
    one = open(paths["on"] + ".alleles.tab", "rb").read()
    assert open(paths["ranks"] + ".alleles.tab", "rb").read() == one
    assert open(paths["host"] + ".alleles.tab", "rb").read() == one
    line = [l for l in r.stdout.split("\n") if l.startswith("allele counts:")]
    assert [l for l in ranks[0][1].split("\n") if l.startswith("allele counts:")] == line
    assert not [l for l in ranks[1][1].split("\n") if l.startswith("allele counts:")]
