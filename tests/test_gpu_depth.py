"""TIDDIT_GENOTYPE_DEPTH on the GPU: the window-median and GC-class-median kernels (csrc/tdt_depth.hip) against the sorting references
of tests/depth_cases.py — the order statistics are compared bit for bit — and the switch end to end on sv_e2e_small with the job's
own VCF fed back in, every job a fresh child process under its own time limit."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import depth_cases as DC
from sv_e2e_common import load_fixture, materialise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("TIDDIT_VARIANTS", "TIDDIT_GENOTYPE", "TIDDIT_GENOTYPE_DEPTH", "TIDDIT_FORCE_DIST", "TIDDIT_COV_TRACK", "WORLD_SIZE", "RANK", "LOCAL_RANK")
LIMIT = int(re.search(r"^#define DP_WINDOW_LIMIT (\d+)\b", open(os.path.join(REPO, "tiddit_amd", "csrc", "tdt_depth.hip")).read(), flags=re.M).group(1))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_windows(cov, gc, table, class_med=None):
    from tiddit_amd import tiddit_depth as D
    n, lo, up = DC.window_stats(cov, gc, table, class_med)
    glo, gup, gn = D.window_medians(cov, gc, table, class_med)
    bad = np.flatnonzero((gn != n) | (_bits(glo) != _bits(lo)) | (_bits(gup) != _bits(up)))
    assert not len(bad), [(np.asarray(table).reshape(-1, 6)[i].tolist(), (gn[i], glo[i], gup[i]), (n[i], lo[i], up[i])) for i in bad[:5]]
    return n, lo, up


def _concat(cov, gc):
    bins, o = {}, 0
    for c in cov:
        bins[c] = (o, len(cov[c]))
        o += len(cov[c])
    return np.concatenate([cov[c] for c in cov]), np.concatenate([gc[c] for c in cov]), bins


# ---- window medians -----------------------------------------------------------------------------------------------------------
def test_small_contigs_and_clipped_flanks():
    """contigs of 1, 2, 5 and 41 bins; windows at the first and the last bin, flanks clipped to nothing on one or both sides"""
    from tiddit_amd import tiddit_depth as D
    sites, cov, gc = DC.small_contigs()
    c, g, bins = _concat(cov, gc)
    table = D.windows_of(sites, bins)
    assert any(r[1:5] == [-1, -1, -1, -1] for r in table[1::3].tolist()) and any(r[1] == -1 and r[3] >= 0 for r in table[1::3].tolist())
    cn, clo, cup = DC.class_stats(c, g, list(bins.values()))
    M = D.medians_of(clo, cup, cn)
    _check_windows(c, g, table, M)
    assert D.depth_fields(sites, cov, gc) == DC.depth_reference(sites, cov, gc)


def test_usable_counts_and_the_switch_to_the_long_route():
    """0, 1, 2, 63, 64 and 65 usable bins; LIMIT - 1, LIMIT and LIMIT + 1 bins as one range and as two"""
    rng = np.random.default_rng(7)
    nb = 2 * LIMIT + 200
    cov = rng.permutation(nb).astype(np.float64) / 3
    gc = rng.integers(0, 101, nb).astype(np.int8)
    rows = []
    for k in (0, 1, 2, 63, 64, 65):                            # a window of 90 bins of which k are usable
        at = 100 * len(rows)
        gc[at:at + 90] = -1
        gc[at + rng.choice(90, k, replace=False)] = 40
        rows.append([0, at, at + 89, -1, -1, -1])
    gc[700:] = np.where(rng.random(nb - 700) < 0.1, -1, gc[700:])
    for n in (LIMIT - 1, LIMIT, LIMIT + 1):
        rows.append([0, 50, 50 + n - 1, -1, -1, -1])
        rows.append([0, 50, 50 + n // 2 - 1, nb - (n - n // 2), nb - 1, -1])
        rows.append([50, 0, n - 1, -1, -1, 0])
    rows.append([0, 0, nb - 1, -1, -1, -1])                    # the whole array
    M = np.full((1, 101), np.nan)
    M[0, ::2] = rng.permutation(51) + 0.5                      # odd classes have no median
    n, lo, up = _check_windows(cov, gc, rows, M)
    assert n[:6].tolist() == [0, 1, 2, 63, 64, 65] and (n[6:] > 100).all() and (lo[6:] < up[6:]).any()


def test_values():
    """all masked, all zero, all equal; ties at the middle; values one mantissa bit apart; exact zeros among positive values"""
    tiny = np.nextafter(1.0, 2.0)
    parts = [np.full(50, 9.0), np.zeros(50), np.full(50, 2.5), np.array([1.0, 3.0, 3.0, 3.0, 3.0, 7.0]), np.array([1.0, 2.0, 2.0, 3.0]),
             np.array([tiny, 1.0, np.nextafter(tiny, 2.0), 1.0]), np.array([1.0, tiny]), np.array([0.0, 5e-300, 0.0, 1e300, 0.0, 2.0, 0.0]),
             np.array([0.0, 0.0, 4.0, 4.0]), np.array([2.0 ** -1022, 0.0, 2.0 ** -1022 * 3])]
    cov = np.concatenate(parts)
    gc = np.full(len(cov), 50, dtype=np.int8)
    gc[:50] = -1
    rows, o = [], 0
    for p in parts:
        rows.append([0, o, o + len(p) - 1, -1, -1, -1])
        o += len(p)
    rows.append([0, 0, 49, 100, 149, -1])                      # a masked range beside an equal one
    n, lo, up = _check_windows(cov, gc, rows)
    assert n[0] == 0 and (lo[1], up[1]) == (0.0, 0.0) and n[1] == 50 and (lo[2], up[2]) == (2.5, 2.5)
    assert (lo[5], up[5]) == (1.0, tiny) and (lo[6], up[6]) == (1.0, tiny) and (lo[8], up[8]) == (0.0, 4.0)
    # the same values repeated beyond the limit: the long route
    big = np.tile(parts[7], LIMIT // 7 + 3)
    _check_windows(big, np.full(len(big), 1, dtype=np.int8), [[0, 0, len(big) - 1, -1, -1, -1], [0, 0, len(big) - 2, -1, -1, -1]])
    z = np.zeros(LIMIT + 5)
    n, lo, up = _check_windows(z, np.full(len(z), -1, dtype=np.int8), [[0, 0, len(z) - 1, -1, -1, -1]])       # long and all masked
    assert n[0] == 0


# ---- GC-class medians ---------------------------------------------------------------------------------------------------------
def test_class_medians():
    """classes of 0, 1, 2, 3001 and 4000 members, a contig of one class, cov == 0 in a class of one, two contigs in one call"""
    from tiddit_amd import tiddit_depth as D
    rng = np.random.default_rng(11)
    sizes = {0: 1, 1: 2, 2: 3001, 3: 4000, 100: 2999, 57: 1}
    g1 = np.concatenate([np.full(k, g) for g, k in sizes.items()] + [np.full(500, -1)]).astype(np.int8)
    rng.shuffle(g1)
    c1 = rng.integers(1, 400, len(g1)).astype(np.float64) / 8              # many ties
    c1[np.flatnonzero(g1 == 57)] = 0.0                                     # the class of one has no covered bin
    c1[np.flatnonzero(g1 == 3)[:100]] = 0.0
    c2 = rng.random(777) + 0.25
    c2[5] = np.nextafter(c2[6], 1.0)
    g2 = np.full(777, 33, dtype=np.int8)
    cov, gc = np.concatenate([c1, c2]), np.concatenate([g1, g2])
    seg = [(0, len(c1)), (len(c1), 777), (0, len(cov)), (len(c1), 0)]
    n, lo, up = DC.class_stats(cov, gc, seg)
    assert n[0, [0, 1, 2, 3, 4, 57, 100]].tolist() == [1, 2, 3001, 3900, 0, 0, 2999] and n[1].sum() == n[1, 33] == 777 and not n[3].any()
    glo, gup, gn = D.gc_class_medians(cov, gc, seg)
    assert np.array_equal(gn, n) and np.array_equal(_bits(glo), _bits(lo)) and np.array_equal(_bits(gup), _bits(up))
    M = D.medians_of(glo, gup, gn)
    for s, (o, k) in enumerate(seg[:2]):
        want = DC.class_medians(cov[o:o + k], gc[o:o + k])
        assert {g for g in range(101) if not np.isnan(M[s, g])} == set(want)
        assert all(M[s, g].tobytes() == np.float64(want[g]).tobytes() for g in want)


# ---- the entries --------------------------------------------------------------------------------------------------------------
def test_device_entries_equal_the_host_entries():
    import torch
    from tiddit_amd import _native
    from tiddit_amd import tiddit_depth as D
    sites, cov, gc = DC.told_apart_case()
    c, g, bins = _concat(cov, gc)
    c, g = np.concatenate([c, np.arange(LIMIT + 9) / 4.0]), np.concatenate([g, np.full(LIMIT + 9, 44, dtype=np.int8)])
    seg = np.array(list(bins.values()), dtype=np.int64)
    ctx = _native.default_context()
    lo, up, n = D.gc_class_medians(c, g, seg)
    d_c, d_g = torch.from_numpy(c).cuda(), torch.from_numpy(g).cuda()
    d_lo, d_up = torch.full(lo.shape, -7.0, dtype=torch.float64, device="cuda"), torch.full(lo.shape, -7.0, dtype=torch.float64, device="cuda")
    d_n = torch.full(lo.shape, -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _native.check(ctx.lib.tdt_gc_class_medians_device(ctx.handle, d_c.data_ptr(), d_g.data_ptr(), len(c), _native.ptr(seg), len(seg),
                                                      d_lo.data_ptr(), d_up.data_ptr(), d_n.data_ptr()))
    assert np.array_equal(d_n.cpu().numpy(), n) and np.array_equal(_bits(d_lo.cpu().numpy()), _bits(lo)) and np.array_equal(_bits(d_up.cpu().numpy()), _bits(up))
    M = D.medians_of(lo, up, n)
    table = np.concatenate([D.windows_of(sites, bins), np.array([[len(c) - LIMIT - 9, 0, LIMIT + 8, -1, -1, -1]])])
    wn, wlo, wup = _check_windows(c, g, table, M)
    d_t, d_M = torch.from_numpy(table).cuda(), torch.from_numpy(np.ascontiguousarray(M)).cuda()
    out = [torch.full((len(table),), -7.0, dtype=torch.float64, device="cuda") for _ in range(2)] + [torch.full((len(table),), -7, dtype=torch.int64, device="cuda")]
    torch.cuda.synchronize()
    _native.check(ctx.lib.tdt_window_medians_device(ctx.handle, d_c.data_ptr(), d_g.data_ptr(), len(c), d_t.data_ptr(), len(table), d_M.data_ptr(),
                                                    len(M), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()))
    assert np.array_equal(out[2].cpu().numpy(), wn) and np.array_equal(_bits(out[0].cpu().numpy()), _bits(wlo))
    assert np.array_equal(_bits(out[1].cpu().numpy()), _bits(wup))
    assert D.depth_fields(sites, cov, gc) == DC.depth_reference(sites, cov, gc)
    # the device entry cannot see its table: the kernel checks it — zeros for the refused window, the others answered
    bad = table.copy()
    bad[4] = [0, 5, len(c), -1, -1, -1]
    d_t = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    rc = ctx.lib.tdt_window_medians_device(ctx.handle, d_c.data_ptr(), d_g.data_ptr(), len(c), d_t.data_ptr(), len(bad), d_M.data_ptr(), len(M),
                                           out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    assert rc == -3 and b"window 4 " in ctx.lib.tdt_last_error()
    got = out[2].cpu().numpy()
    assert got[4] == 0 and np.array_equal(np.delete(got, 4), np.delete(wn, 4))


def test_refused_arguments():
    from tiddit_amd import _native
    from tiddit_amd import tiddit_depth as D
    ctx = _native.default_context()
    cov, gc = np.arange(100.0), np.full(100, 40, dtype=np.int8)
    M = np.ones((2, 101))
    good = [10, 0, 20, 30, 40, 1]
    assert D.window_medians(cov, gc, [good], M)[2][0] == 32
    for row, code in (([10, 5, 4, -1, -1, -1], -1), ([10, 0, 5, 9, 8, -1], -1), ([10, 0, 90, -1, -1, -1], -3), ([10, 0, 5, 80, 90, -1], -3),
                      ([101, 0, 0, -1, -1, -1], -3), ([-1, 0, 5, -1, -1, -1], -3), ([0, -2, 5, -1, -1, -1], -3), ([0, 0, 5, -1, -1, 2], -3),
                      ([0, 0, 5, -1, -1, -2], -3), ([100, -1, -1, -1, -1, -1], 0)):
        if code == 0:
            assert D.window_medians(cov, gc, [good, row], M)[2].tolist() == [32, 0]
            continue
        with pytest.raises(_native.TdtError) as e:
            D.window_medians(cov, gc, [good, row], M)
        assert e.value.code == code and "window 1" in str(e.value), row
    with pytest.raises(_native.TdtError) as e:
        D.window_medians(cov, gc, [[0, 0, 5, -1, -1, 0]])     # a class row without class medians
    assert e.value.code == -3
    for seg, code in (([(0, -1)], -1), ([(0, 101)], -3), ([(-1, 5)], -3), ([(101, 0)], -3), ([(100, 0)], 0)):
        if code == 0:
            assert not D.gc_class_medians(cov, gc, seg)[2].any()
            continue
        with pytest.raises(_native.TdtError) as e:
            D.gc_class_medians(cov, gc, [(0, 100)] + seg)
        assert e.value.code == code and "segment 1" in str(e.value), seg
    # null and misaligned pointers
    t = np.array([good], dtype=np.int64)
    lo, up, n = np.zeros(1), np.zeros(1), np.zeros(1, dtype=np.int64)
    P = _native.ptr
    args = [ctx.handle, P(cov), P(gc), 100, P(t), 1, P(M), 2, P(lo), P(up), P(n)]
    assert ctx.lib.tdt_window_medians(*args) == 0
    for k in (1, 2, 4, 6, 8, 9, 10):
        a = list(args)
        a[k] = None
        assert ctx.lib.tdt_window_medians(*a) == -1 and ctx.lib.tdt_window_medians_device(*a) == -1, k
    for k in (1, 4, 6, 8, 9, 10):
        a = list(args)
        a[k] = ctypes.c_void_p(a[k].value + 4)
        assert ctx.lib.tdt_window_medians(*a) == -1 and ctx.lib.tdt_window_medians_device(*a) == -1, k
    assert ctx.lib.tdt_window_medians(None, *args[1:]) == -1
    s = np.array([[0, 100]], dtype=np.int64)
    clo, cup, cn = np.zeros(101), np.zeros(101), np.zeros(101, dtype=np.int64)
    cargs = [ctx.handle, P(cov), P(gc), 100, P(s), 1, P(clo), P(cup), P(cn)]
    assert ctx.lib.tdt_gc_class_medians(*cargs) == 0 and cn[40] == 99
    for k in (1, 2, 4, 6, 7, 8):
        a = list(cargs)
        a[k] = None
        assert ctx.lib.tdt_gc_class_medians(*a) == -1 and ctx.lib.tdt_gc_class_medians_device(*a) == -1, k
    for k in (1, 6, 7, 8):
        a = list(cargs)
        a[k] = ctypes.c_void_p(a[k].value + 4)
        assert ctx.lib.tdt_gc_class_medians(*a) == -1 and ctx.lib.tdt_gc_class_medians_device(*a) == -1, k
    # nothing asked: accepted whatever the pointers
    assert ctx.lib.tdt_window_medians(ctx.handle, None, None, 0, None, 0, None, 0, None, None, None) == 0
    assert ctx.lib.tdt_window_medians_device(ctx.handle, None, None, 0, None, 0, None, 0, None, None, None) == 0
    assert ctx.lib.tdt_gc_class_medians(ctx.handle, None, None, 0, None, 0, None, None, None) == 0
    assert D.window_medians(cov, gc, np.zeros((0, 6)))[2].shape == (0,)
    assert D.window_medians(cov, gc, [good], M)[2][0] == 32                  # (and the context is still good)


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------
def _job(bam, fa, out, fx, timeout=600, **env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    return subprocess.run([sys.executable, "-m", "tiddit_amd", "--sv", "--bam", bam, "--ref", fa, "-o", out, "--skip_assembly", "-s",
                           str(fx["params"]["n_reads_stats"])], cwd=REPO, env=e, capture_output=True, text=True, timeout=timeout)


def _ok(r):
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r


def _split(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return [l for l in lines[:-1] if l.startswith("#") and not l.startswith("##TIDDITcmd=")], [l.split("\t") for l in lines[:-1] if not l.startswith("#")]


def _files(prefix):
    d, base = os.path.split(prefix)
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            rel = os.path.relpath(os.path.join(root, f), d)
            if rel.startswith(base + ".") or rel.startswith(base + "_tiddit"):
                out[rel[len(base):]] = hashlib.sha256(open(os.path.join(root, f), "rb").read()).hexdigest()
    return out


@pytest.fixture(scope="module")
def jobs(golden_dir, tmp_path_factory):
    fx = load_fixture(golden_dir, "sv_e2e_small.json")
    d = str(tmp_path_factory.mktemp("depth"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    first, plain, depth = (os.path.join(d, n) for n in ("first", "plain", "depth"))
    _ok(_job(bam, fa, first, fx, TIDDIT_VARIANTS="1"))
    _ok(_job(bam, fa, plain, fx, TIDDIT_GENOTYPE=first + ".vcf"))
    _ok(_job(bam, fa, depth, fx, TIDDIT_GENOTYPE=first + ".vcf", TIDDIT_GENOTYPE_DEPTH="1"))
    return fx, bam, fa, contigs, d, first, plain, depth


def test_own_vcf_fed_back_in_with_the_switch(jobs):
    from tiddit_amd import tiddit_depth as D
    from tiddit_amd import tiddit_gc, tiddit_signal
    from tiddit_amd import tiddit_genotype as G
    fx, bam, fa, contigs, d, first, plain, depth = jobs
    head0, rec0 = _split(plain + ".genotyped.vcf")
    head, rec = _split(depth + ".genotyped.vcf")
    assert len(rec) == len(rec0) > 0
    assert [l for l in head if l not in head0] == list(D.FORMAT_LINES) == head[-5:-2]
    assert [l for l in head if l not in D.FORMAT_LINES] == head0
    assert head[-2].startswith("##TIDDITgenotype=") and head[-1].startswith("#CHROM")
    P = fx["params"]
    cov = tiddit_signal.scan_signals(bam, P["min_q"], fx["library"]["percentile_insert_size"], P["min_contig"], P["min_anchor_len"],
                                     P["min_clip_len"], 50)[2]
    gc = tiddit_gc.main(fa, [n for n, _ in contigs], 1, 50, 0.5)
    number = {n: i for i, (n, _) in enumerate(contigs)}
    sites, _ = G.sites_of(G.parse_vcf(first + ".vcf")[1], number, dict(contigs), fx["library"]["percentile_insert_size"])
    want = DC.depth_reference(sites, cov, gc)
    numeric = re.compile(r"[0-9]+\.[0-9]{3}")
    n_numeric = sum(all(numeric.fullmatch(x) for x in w) for w in want)
    one_contig = sum(s[0] == s[2] for s in sites)
    assert n_numeric == one_contig >= 1                        # every site on one contig of this fixture has all three values
    for i, (a, b) in enumerate(zip(rec0, rec)):
        assert b[:8] == a[:8] and a[8] == "GT:CN:COV:DV:RV:LQ:RR:DR" and b[8] == a[8] + ":DHFC:DHBFC:DHFFC" and len(b) == 10
        f = b[9].split(":")
        assert len(f) == 11 and f[:8] == a[9].split(":") and tuple(f[8:]) == want[i], (i, b[9], want[i])
    assert sum(all(numeric.fullmatch(x) for x in r[9].split(":")[8:]) for r in rec) == n_numeric
    fa_, fb = _files(plain), _files(depth)
    assert set(fa_) == set(fb) and all(fa_[k] == fb[k] for k in fa_ if k != ".genotyped.vcf")


def test_the_switch_alone_is_refused_and_a_job_without_it_is_unchanged(jobs):
    fx, bam, fa, contigs, d, first, plain, depth = jobs
    out = os.path.join(d, "refused")
    r = _job(bam, fa, out, fx, timeout=300, TIDDIT_GENOTYPE_DEPTH="1")
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    assert [l for l in r.stdout.split("\n") if l.startswith("error")] == [l for l in r.stdout.split("\n") if l.startswith("error, TIDDIT_GENOTYPE_DEPTH")]
    assert len([l for l in r.stdout.split("\n") if l.startswith("error")]) == 1
    assert not os.path.exists(out + "_tiddit") and _files(out) == {}
    off = os.path.join(d, "off")
    _ok(_job(bam, fa, off, fx))
    f = _files(off)
    assert f == {k: v for k, v in _files(plain).items() if k != ".genotyped.vcf"}

    def h(p):
        return hashlib.sha256(open(p).read().encode()).hexdigest()
    assert h(off + "_tiddit/discordants_WGS.tab") == fx["discordants_sha256"] and h(off + "_tiddit/splits_WGS.tab") == fx["splits_sha256"]
    assert h(off + "_tiddit/clips_WGS.fa") == fx["clips_sha256"] and open(off + ".ploidies.tab").read() == fx["ploidies_tab"]
    # TIDDIT_GENOTYPE without the depth switch writes the eight sub-fields, as before
    assert all(r[8] == "GT:CN:COV:DV:RV:LQ:RR:DR" and len(r[9].split(":")) == 8 for r in _split(plain + ".genotyped.vcf")[1])
    assert not any("DHFC" in l for l in _split(plain + ".genotyped.vcf")[0])
