"""`TIDDIT_ASCN` on the GPU: the two device stages of csrc/tdt_ascn.hip — the per-bin emissions (``tdt_ascn_emissions``) and the chunked
16-state Viterbi (``tdt_hmm16_viterbi``) — against the literal references of tests/ascn_cases.py (which tests/test_ascn_refs_cpu.py
shows equal to the definition of tiddit_amd/tiddit_ascn.py) on every aimed case, each through the host entry and again through the
``_device`` entry on caller-owned, poisoned, padded outputs; every argument refusal, outputs untouched; the stage on made-up bins and
counters (``tiddit_ascn.main``); and the switch end to end on the sv_e2e_small fixture, every job a fresh child process under its own
time limit.  All comparisons are exact equality.

Every test of this file fails on the parent commit: the symbols, the module and the switch do not exist there."""
import hashlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import ascn_cases as C
import cnv_cases
from sv_e2e_common import load_fixture, materialise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("TIDDIT_VARIANTS", "TIDDIT_GENOTYPE", "TIDDIT_GENOTYPE_DEPTH", "TIDDIT_DEPTH_DIST", "TIDDIT_CNV", "TIDDIT_ASCN", "TIDDIT_ALLELES",
            "TIDDIT_ALLELES_MIN_BQ", "TIDDIT_FORCE_DIST", "TIDDIT_COV_TRACK", "TIDDIT_HOST_INGEST", "TIDDIT_DIST_BACKEND", "WORLD_SIZE", "RANK",
            "LOCAL_RANK")
ENTRIES = ("host", "device")
PAD = 64
PAIRS = [("emissions", i, e) for i in range(len(C.EMISSIONS_CASES)) for e in ENTRIES] + [("viterbi", i, e) for i in range(len(C.VITERBI_CASES)) for e in ENTRIES]
CONSTANTS = (C.UNIT, C.CAP, C.BU, C.ACAP, C.HOM, C.MIN_N)


def _id(pair):
    kind, i, entry = pair
    return "%s-%s-%s" % (kind, (C.EMISSIONS_CASES if kind == "emissions" else C.VITERBI_CASES)[i]["name"], entry)


def test_the_count_of_case_entry_pairs():
    assert len(PAIRS) == 2 * 11 + 2 * 49 == 120


# ---- the two stages, both entries ---------------------------------------------------------------------------------------------
def _padded(n, dtype, poison):
    """a device array of n elements inside a poisoned allocation with PAD elements either side -> (whole, view)"""
    import torch
    whole = torch.full((n + 2 * PAD,), poison, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + n]


def _untouched(whole, n, poison):
    h = whole.cpu().numpy()
    return (h[:PAD] == poison).all() and (h[PAD + n:] == poison).all()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _emissions(case, entry, ctx=None):
    """-> (E [total][16], nsite, sum_beta)"""
    import torch
    from tiddit_amd import _native, tiddit_ascn
    counts, pos, cols, x, table = C.emissions_arrays(case)
    if entry == "host":
        return tiddit_ascn.emissions(counts, pos, cols, x, table, ctx=ctx)
    ctx = ctx or _native.default_context()
    total = len(x)
    keep = [_dev(counts), _dev(pos), _dev(cols), _dev(x)]
    outs = [_padded(total * 16, torch.int32, -77), _padded(total, torch.int32, -78), _padded(total, torch.int32, -79)]
    torch.cuda.synchronize()
    _native.check(ctx.lib.tdt_ascn_emissions_device(ctx.handle, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), len(pos), keep[3].data_ptr(),
                                                    total, _native.ptr(table), len(table), *CONSTANTS, *[v.data_ptr() for _, v in outs]))
    for (whole, _), n, poison in zip(outs, (total * 16, total, total), (-77, -78, -79)):
        assert _untouched(whole, n, poison)
    return outs[0][1].cpu().numpy().reshape(-1, 16), outs[1][1].cpu().numpy(), outs[2][1].cpu().numpy()


def _viterbi(case, entry, ctx=None):
    import torch
    from tiddit_amd import _native, tiddit_ascn
    E, table = C.viterbi_arrays(case)
    if entry == "host":
        return tiddit_ascn.viterbi(E, table, lam=case["lam"], ctx=ctx)
    ctx = ctx or _native.default_context()
    d_E = _dev(E)
    whole, d_s = _padded(len(E), torch.int8, -9)
    torch.cuda.synchronize()
    _native.check(ctx.lib.tdt_hmm16_viterbi_device(ctx.handle, d_E.data_ptr(), len(E), _native.ptr(table), len(table), case["lam"], d_s.data_ptr()))
    assert _untouched(whole, len(E), -9)
    return d_s.cpu().numpy()


def _viterbi_want(case):
    return np.concatenate([r[0] for r in C.viterbi_reference(case)])


@pytest.mark.parametrize("pair", PAIRS, ids=[_id(p) for p in PAIRS])
def test_the_device_equals_the_reference(pair):
    kind, i, entry = pair
    if kind == "emissions":
        case = C.EMISSIONS_CASES[i]
        got, want = _emissions(case, entry), C.emissions_reference(case)
        for g, w, what in zip(got, want, ("E", "nsite", "sum_beta")):
            assert g.dtype == np.int32 and g.shape == w.shape, what
            bad = np.argwhere(g != w)
            assert not len(bad), (case["name"], entry, what, len(bad), [(tuple(int(v) for v in k), int(g[tuple(k)]), int(w[tuple(k)])) for k in bad[:8]])
        return
    case = C.VITERBI_CASES[i]
    got, want = _viterbi(case, entry), _viterbi_want(case)
    assert got.dtype == np.int8 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert not len(bad), (case["name"], entry, len(bad), [(int(k), int(got[k]), int(want[k])) for k in bad[:8]])


def test_two_calls_on_one_context_and_a_context_of_its_own():
    """a long call, a short one, the long one again, the other entry point in between — on the default context and on a fresh one: the
    carved scratch (which the two entries and the 8-state chain share) holds nothing over"""
    from tiddit_amd import _native
    by = {c["name"]: c for c in C.VITERBI_CASES}
    big, small, multi = by["T=%d" % (2 * C.L + 1)], by["stay ties with jump, state 0"], by["nine contigs"]
    em = {c["name"]: c for c in C.EMISSIONS_CASES}
    for ctx in (None, _native.Context(_native.default_context().device)):
        for case in (big, small, multi, big):
            for entry in ENTRIES:
                assert np.array_equal(_viterbi(case, entry, ctx), _viterbi_want(case)), case["name"]
            e = em["700 bins of seeded sites" if case is big else "bin edges, short last bin"]
            for entry in ENTRIES:
                assert all(np.array_equal(g, w) for g, w in zip(_emissions(e, entry, ctx), C.emissions_reference(e)))
        if ctx is not None:
            ctx.close()


def _refusals(call, good, variants, out_untouched):
    """good: the dict of arguments of a call that succeeds; variants: (changed arguments, expected code)"""
    for change, code in variants:
        args = dict(good, **change)
        assert call(**args) == code, (change, code)
        assert out_untouched(), change


@pytest.mark.parametrize("entry", ENTRIES)
def test_emissions_refusals_leave_the_outputs_untouched(entry):
    import torch
    from tiddit_amd import _native
    ctx = _native.default_context()
    lib = ctx.lib
    case = next(c for c in C.EMISSIONS_CASES if c["name"] == "contigs without sites, sites of unprocessed contigs")
    counts, pos, cols, x, table = C.emissions_arrays(case)
    total, ns = len(x), len(pos)
    sizes = (total * 16 + 1, total + 1, total + 1)
    if entry == "host":
        outs = [np.full(n, -7, dtype=np.int32) for n in sizes]
        keep = (counts, pos, cols, x)
        ptrs = [a.ctypes.data for a in keep + tuple(outs)]
        fn, untouched = lib.tdt_ascn_emissions, (lambda: all((o == -7).all() for o in outs))
        result = lambda: [o[:n - 1] for o, n in zip(outs, sizes)]
    else:
        outs = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in sizes]
        keep = (_dev(counts), _dev(pos), _dev(cols), _dev(x))
        ptrs = [t.data_ptr() for t in keep + tuple(outs)]
        torch.cuda.synchronize()
        fn, untouched = lib.tdt_ascn_emissions_device, (lambda: all(bool((o == -7).all()) for o in outs))
        result = lambda: [o.cpu().numpy()[:n - 1] for o, n in zip(outs, sizes)]
    p_counts, p_pos, p_cols, p_x, p_E, p_n, p_b = ptrs

    def call(ctx_h, counts, pos, cols, ns, x, total, table, nseg, unit, cap, bu, acap, hom, min_n, E, nsite, sum_beta):
        return fn(ctx_h, counts, pos, cols, ns, x, total, None if table is None else _native.ptr(table), nseg, unit, cap, bu, acap, hom, min_n, E,
                  nsite, sum_beta)

    def row(s, col, v):
        t = table.copy()
        t[s, col] = v
        return {"table": t}, -3
    good = dict(ctx_h=ctx.handle, counts=p_counts, pos=p_pos, cols=p_cols, ns=ns, x=p_x, total=total, table=table, nseg=len(table), unit=C.UNIT,
                cap=C.CAP, bu=C.BU, acap=C.ACAP, hom=C.HOM, min_n=C.MIN_N, E=p_E, nsite=p_n, sum_beta=p_b)
    big = 1 << 28
    _refusals(call, good, [({"ctx_h": None}, -1), ({"counts": None}, -1), ({"pos": None}, -1), ({"cols": None}, -1), ({"x": None}, -1), ({"table": None}, -1),
                           ({"E": None}, -1), ({"nsite": None}, -1), ({"sum_beta": None}, -1), ({"counts": p_counts + 2}, -1), ({"pos": p_pos + 2}, -1),
                           ({"x": p_x + 2}, -1), ({"E": p_E + 2}, -1), ({"nsite": p_n + 2}, -1), ({"sum_beta": p_b + 2}, -1), ({"ns": -1}, -1),
                           ({"total": -1}, -1), ({"nseg": -1}, -1), ({"unit": 0}, -1), ({"unit": (1 << 20) + 1}, -1), ({"cap": -1}, -1),
                           ({"cap": big + 1}, -1), ({"bu": 0}, -1), ({"bu": (1 << 15) + 1}, -1), ({"acap": -1}, -1), ({"acap": (1 << 16) + 1}, -1),
                           ({"hom": -1}, -1), ({"hom": big + 1}, -1), ({"min_n": 0}, -1), ({"total": total - 1}, -3), ({"total": total + 1}, -3),
                           ({"nseg": len(table) - 1}, -3), row(0, 0, -1), row(1, 1, ns + 1), row(1, 1, table[1, 0] - 1), row(2, 2, table[2, 2] + 1),
                           row(0, 2, 1), row(1, 3, -1), row(3, 3, table[3, 3] + 1), row(2, 4, 0), row(2, 4, 3201), ({"ns": ns - 1}, -3),
                           ({"total": 0, "x": None, "E": None, "nsite": None, "sum_beta": None}, 0),
                           ({"nseg": 0, "table": None, "x": None, "E": None, "nsite": None, "sum_beta": None}, 0)], untouched)
    if entry == "host":
        bad = cols.copy()
        bad[2, 1] = 8
        assert call(**dict(good, cols=bad.ctypes.data)) == -3 and untouched()
    assert call(**dict(good, **row(2, 4, 3201)[0])) == -3 and "tdt_ascn_emissions" in lib.tdt_last_error().decode()
    assert call(**good) == 0                              # (and the context is still good)
    want = C.emissions_reference(case)
    assert all(np.array_equal(g.reshape(w.shape), w) for g, w in zip(result(), want))
    assert all(int(o[n - 1]) == -7 for o, n in zip(outs, sizes))
    del keep


@pytest.mark.parametrize("entry", ENTRIES)
def test_viterbi_refusals_leave_the_output_untouched(entry):
    import torch
    from tiddit_amd import _native
    ctx = _native.default_context()
    lib = ctx.lib
    case = next(c for c in C.VITERBI_CASES if c["name"] == "nine contigs")
    E, table = C.viterbi_arrays(case)
    n = len(E)
    if entry == "host":
        out = np.full(n + 1, -7, dtype=np.int8)
        keep = (E,)
        p_e, p_s = E.ctypes.data, out.ctypes.data
        fn, untouched, result = lib.tdt_hmm16_viterbi, (lambda: (out == -7).all()), (lambda: out[:n])
    else:
        keep = (_dev(E), torch.full((n + 1,), -7, dtype=torch.int8, device="cuda"))
        p_e, p_s = (t.data_ptr() for t in keep)
        torch.cuda.synchronize()
        fn, untouched, result = lib.tdt_hmm16_viterbi_device, (lambda: bool((keep[1] == -7).all())), (lambda: keep[1].cpu().numpy()[:n])

    def call(ctx_h, e, n, table, nseg, lam, state):
        return fn(ctx_h, e, n, None if table is None else _native.ptr(table), nseg, lam, state)

    def row(s, col, v):
        t = table.copy()
        t[s, col] = v
        return {"table": t}, -3
    good = dict(ctx_h=ctx.handle, e=p_e, n=n, table=table, nseg=len(table), lam=C.LAMBDA, state=p_s)
    _refusals(call, good, [({"ctx_h": None}, -1), ({"e": None}, -1), ({"table": None}, -1), ({"state": None}, -1), ({"e": p_e + 2}, -1), ({"n": -1}, -1),
                           ({"nseg": -1}, -1), ({"lam": -1}, -1), ({"lam": (1 << 28) + 1}, -1), ({"n": n - 1}, -3), ({"n": n + 1}, -3),
                           row(2, 0, table[2, 0] + 1), row(1, 1, -1), row(8, 1, table[8, 1] + 1), row(3, 2, -1), row(3, 2, 16),
                           ({"nseg": len(table) - 1}, -3), ({"n": 0, "e": None, "state": None}, 0),
                           ({"nseg": 0, "table": None, "e": None, "state": None}, 0)], untouched)
    if entry == "host":
        for v in (-1, (1 << 28) + 1):
            bad = E.copy()
            bad[n // 2, 5] = v
            assert call(**dict(good, e=bad.ctypes.data)) == -3 and untouched() and "outside 0 .. 2^28" in lib.tdt_last_error().decode()
    assert call(**dict(good, **row(3, 2, 16)[0])) == -3 and "tdt_hmm16_viterbi" in lib.tdt_last_error().decode()
    assert call(**good) == 0                              # (and the context is still good)
    assert np.array_equal(result(), _viterbi_want(case)) and (entry == "device" or out[n] == -7)
    del keep


# ---- the stage on made-up bins and counters -----------------------------------------------------------------------------------
def test_the_stage_on_the_planted_job(tmp_path, capsys):
    """tiddit_cnv.bins_stage + tiddit_ascn.main on the planted job of tests/ascn_cases.py: the file the literal references write —
    the three planted segments and nothing else, a contig without sites, a skipped contig with sites — and tiddit_cnv.main's own file
    from the same two halves"""
    from tiddit_amd import tiddit_ascn, tiddit_cnv
    args, table, sites, number = C.planted_job()
    coverage, gcs, library, contigs, length, min_contig, W = args
    want, skipped, tracks, detail = C.planted_reference()
    prefix = str(tmp_path / "planted")
    bins = tiddit_cnv.bins_stage(coverage, gcs, dict(library), contigs, length, min_contig, W)
    assert bins.used == [c for c in contigs if c in tracks] and bins.skipped == skipped
    assert np.array_equal(bins.d_x.cpu().numpy(), np.concatenate([tracks[c][0] for c in bins.used]))
    segments = tiddit_ascn.main(bins, table, sites, number, length, prefix)
    got = open(prefix + ".ascn.bed").read()
    assert got == want and len(segments) == 3 and [s[3] for s in segments] == ["LOH", "DEL", "DUP"]
    assert [l for l in capsys.readouterr().out.split("\n") if l.startswith("note:")] == ["note: TIDDIT_ASCN skips tiny"]
    assert any(k.startswith("ASCN segmentation") for k in tiddit_ascn.STAGE_SECONDS) and any(k.startswith("ASCN emissions") for k in tiddit_ascn.STAGE_SECONDS)
    # the counters as the N-rank sum hands them over
    tiddit_ascn.main(bins, table.astype(np.int64), sites, number, length, prefix + "64")
    assert open(prefix + "64.ascn.bed").read() == want
    # the halves are what main runs
    tiddit_cnv.segments_stage(bins, length, prefix)
    halves = open(prefix + ".cnv.bed").read()
    keys = list(tiddit_cnv.STAGE_SECONDS)
    tiddit_cnv.main(coverage, gcs, dict(library), contigs, length, min_contig, W, prefix + "main")
    assert open(prefix + "main.cnv.bed").read() == halves == cnv_cases.ref_job(*args)[0] and list(tiddit_cnv.STAGE_SECONDS) == keys and len(keys) == 7
    # nothing to process: the header alone
    none = tiddit_cnv.bins_stage(coverage, gcs, dict(library), ["tiny"], length, min_contig, W)
    assert tiddit_ascn.main(none, table, sites, number, length, prefix + "none") == [] and open(prefix + "none.ascn.bed").read() == C.HEADER


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
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for name, ln in contigs:
            seq = fasta.fetch(name).upper()
            for p in range(996, ln, 997):
                ref = seq[p]
                alt = "ACGT"[("ACGT".index(ref) + 1) % 4] if ref in "ACGT" else "A"
                f.write("%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (name, p + 1, ref, alt))


def _two_ranks(bam, fa, out, fx, **env):
    port = _port()
    procs = [subprocess.Popen(_argv(bam, fa, out, fx), cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=_env(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r),
                                       TIDDIT_HIP_DEVICE="0", TIDDIT_DIST_BACKEND="gloo", TIDDIT_INGEST_CHUNK=str(48 << 20), **env))
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
    d = str(tmp_path_factory.mktemp("ascn"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    sites = os.path.join(d, "sites.vcf")
    _write_sites(sites, fa, contigs)
    paths = {n: os.path.join(d, n) for n in ("off", "on", "ranks")}
    _ok(_job(bam, fa, paths["off"], fx, TIDDIT_CNV="1", TIDDIT_ALLELES=sites))
    r = _ok(_job(bam, fa, paths["on"], fx, TIDDIT_CNV="1", TIDDIT_ALLELES=sites, TIDDIT_ASCN="1"))
    _two_ranks(bam, fa, paths["ranks"], fx, TIDDIT_CNV="1", TIDDIT_ALLELES=sites, TIDDIT_ASCN="1")
    return fx, bam, fa, d, paths, sites, r


def test_the_file_equals_the_definition_on_the_job_s_own_bins_and_counts(jobs, tmp_path):
    """the bins as the job gets them — tiddit_signal.main, tiddit_gc.main and determine_ploidy in this process on the same files,
    through the literal reference of the CNV bins — and the counters the job wrote into its .alleles.tab, through the definition"""
    from tiddit_amd import bamio, tiddit_ascn, tiddit_coverage_analysis, tiddit_gc, tiddit_signal, tiddit_stats
    fx, bam, fa, d, paths, sites_path, r = jobs
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
    _, skipped, tracks = cnv_cases.ref_job(cov, gc, library, contigs, length, 10000, 500)
    by = {}
    for line in open(paths["on"] + ".alleles.tab"):
        f = line.rstrip("\n").split("\t")
        if not line.startswith("#"):
            by.setdefault(f[0], {}).setdefault(int(f[1]) - 1, (int(f[12]), int(f[13])))           # (the first row of a position)
    segs, informative = [], 0
    for c in contigs:
        if c in tracks:
            pos = sorted(by.get(c, {}))
            out = tiddit_ascn.define_contig(tracks[c][0], library["contig_ploidy_" + c], 500, length[c], c, pos, [by[c][p][0] for p in pos],
                                            [by[c][p][1] for p in pos])
            informative += sum(out[1])
            segs += out[4]
    got = open(paths["on"] + ".ascn.bed").read()
    assert len(tracks) >= 20 and informative > 1000
    assert got == tiddit_ascn.text_of(segs) and got.startswith(C.HEADER)
    notes = [l for l in r.stdout.split("\n") if l.startswith("note: TIDDIT_ASCN skips")]
    assert notes == (["note: TIDDIT_ASCN skips " + ", ".join(skipped)] if skipped else [])


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    fx, bam, fa, d, paths, sites, r = jobs
    off, on = _files(paths["off"]), _files(paths["on"])
    assert set(on) - set(off) == {".ascn.bed"} and set(off) <= set(on) and {".cnv.bed", ".alleles.tab"} <= set(off)
    assert all(on[k] == off[k] for k in off), [k for k in off if on[k] != off[k]]
    assert not os.path.exists(paths["off"] + ".ascn.bed")


def test_the_two_rank_job_writes_the_same_bytes(jobs):
    fx, bam, fa, d, paths, sites, r = jobs
    for ext in (".ascn.bed", ".cnv.bed", ".alleles.tab", ".candidates.tab"):
        assert open(paths["ranks"] + ext, "rb").read() == open(paths["on"] + ext, "rb").read(), ext


@pytest.mark.parametrize("partner", ["TIDDIT_CNV", "TIDDIT_ALLELES"])
def test_the_switch_without_a_partner_is_refused_with_nothing_made(jobs, partner):
    fx, bam, fa, d, paths, sites, r = jobs
    out = os.path.join(d, "refused" + partner)
    env = {"TIDDIT_CNV": "1", "TIDDIT_ALLELES": sites, "TIDDIT_ASCN": "1"}
    del env[partner]
    r = _job(bam, fa, out, fx, timeout=300, **env)
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    errors = [l for l in r.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_ASCN=1:") and partner + " is not set" in errors[0]
    assert not os.path.exists(out + "_tiddit") and not _files(out)
