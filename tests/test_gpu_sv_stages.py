"""GPU tests that call three device stages of `tiddit --sv` directly, on the adversarial inputs of tests/sv_stage_cases.py and
against its plain references (pinned on the CPU by test_sv_stage_refs_cpu.py):
  * library statistics (csrc/tdt_stats.hip): tdt_stats_create / _push_device / _counts / _moments and tiddit_stats._device_figures
    against the sampling rules + numpy.average / std / percentile / sort on the same list;
  * the per-read action chain and its gather (csrc/tdt_signal.hip): tiddit_signal._device_scan against sigtab_common.select_host;
  * masked medians (csrc/tdt_median.hip): tdt_masked_medians and tdt_masked_medians_parts against numpy.median per segment.
Every comparison is `==`: the project's claim is bit-identity.  Run on the MI355X box: python -m pytest tests/test_gpu_sv_stages.py -m gpu"""
import ctypes

import numpy as np
import pytest

import sigtab_common
import sv_stage_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from tiddit_amd import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def ctx(nat):
    return nat.default_context(0)


# ================================================================================================== library statistics
STATS_CASES = sc.stats_cases(large=True)
COUNTERS = ("sampled", "sum_len", "n_len", "innie", "outtie", "n_ins", "sum_ins")


def _upload(batch, dev):
    """the eight decoded columns as torch device tensors, in the order tdt_stats_push_device takes them"""
    import torch
    out = []
    for k in sc.COLS:
        a = np.ascontiguousarray(batch[k], dtype=sc._DT[k])
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        out.append(torch.from_numpy(a).to(dev))
    return out


def _counts(nat, lib, h):
    cnt = np.zeros(9, dtype=np.int64)
    nat.check(lib.tdt_stats_counts(h, nat.ptr(cnt)))
    return cnt


def _moments(nat, lib, h, mean, k0, k1):
    msd, o0, o1 = ctypes.c_double(0), ctypes.c_int32(0), ctypes.c_int32(0)
    nat.check(lib.tdt_stats_moments(h, float(mean), int(k0), int(k1), ctypes.byref(msd), ctypes.byref(o0), ctypes.byref(o1)))
    return np.float64(msd.value), o0.value, o1.value


def test_statistics_case_count():
    assert len(STATS_CASES) == 87 and sum(c["large"] for c in STATS_CASES) == 2 and sum(not c["figures"] for c in STATS_CASES) == 1


@pytest.mark.parametrize("case", STATS_CASES, ids=[c["name"] for c in STATS_CASES])
def test_library_statistics_vs_rules_and_numpy(nat, ctx, case):
    """Every batch is pushed, also those behind the one that completes the sample: `done` must turn 1 on exactly the batch where the
    reference's loop breaks, and a push after that must change no counter.  The seven counters, the two order statistics of the
    percentile (and the extreme and middle ranks), sqrt(mean squared deviation) == numpy.std, and the three figures of
    tiddit_stats._device_figures == numpy's, all with `==`.
    The case with INT32_MIN / INT32_MAX in the list asserts the counters and the order statistics only: numpy.percentile's own int32
    interpolation (numpy.subtract(b, a)) wraps beyond +-2^30, and the kernel is not bent to that."""
    import torch
    from tiddit_amd import tiddit_stats
    lib = ctx.lib
    dev = torch.device("cuda", ctx.device)
    want, ins = sc.stats_reference(case["batches"], case["n_reads"], case["min_mapq"], case["max_ins_len"])
    want_done = sc.done_flags(case["batches"], case["n_reads"])
    h = ctypes.c_void_p()
    nat.check(lib.tdt_stats_create(ctx.handle, case["n_reads"], case["min_mapq"], case["max_ins_len"], ctypes.byref(h)))
    try:
        got_done, frozen = [], None
        for b in case["batches"]:
            t = _upload(b, dev)
            torch.cuda.synchronize(dev)
            done = ctypes.c_int(-1)
            nat.check(lib.tdt_stats_push_device(h, *[x.data_ptr() for x in t], len(b["tid"]), ctypes.byref(done)))
            got_done.append(bool(done.value))
            assert done.value in (0, 1)
            if frozen is not None:                                    # a push after `done`
                assert np.array_equal(_counts(nat, lib, h), frozen)
            elif done.value:
                frozen = _counts(nat, lib, h)
        assert got_done == want_done
        cnt = _counts(nat, lib, h)
        assert dict(zip(COUNTERS, cnt[:7].tolist())) == want
        n = want["n_ins"]
        assert n == len(ins)
        if n:
            srt = np.sort(ins)
            mean = np.float64(int(cnt[6])) / n
            k0, k1 = sc.percentile_ranks(n)
            msd, o0, o1 = _moments(nat, lib, h, mean, k0, k1)
            assert (o0, o1) == (int(srt[k0]), int(srt[k1]))
            for r0, r1 in ((0, n - 1), (n // 2, n // 2), ((n - 1) // 3, (2 * n) // 3)):
                _, a, b = _moments(nat, lib, h, mean, r0, r1)
                assert (a, b) == (int(srt[r0]), int(srt[r1])), (r0, r1)
            if case["figures"]:
                assert mean == np.average(ins)
                assert np.sqrt(msd) == np.std(ins)
                state = np.zeros(6, dtype=np.int64)
                fig = tiddit_stats._device_figures(lib, h, state)
                assert fig is not None and tuple(fig) == sc.stats_figures(ins)
                assert state[:5].tolist() == [want[k] for k in COUNTERS[:5]]
        else:
            state = np.zeros(6, dtype=np.int64)
            assert tiddit_stats._device_figures(lib, h, state) is None and state[:5].tolist() == [want[k] for k in COUNTERS[:5]]
    finally:
        lib.tdt_stats_destroy(h)


# ================================================================================================== the signal scan
@pytest.fixture(scope="module")
def scan_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("scan")
    records, spans = sc.scan_records()
    files = {"main": (sc.scan_batch(records, d / "scan.bam"), len(records), spans)}
    for n in (1023, 1024, 1025):
        r = sc.scan_count_records(n)
        files[n] = (sc.scan_batch(r, d / ("count%d.bam" % n)), len(r), None)
    return files


def _compare_scan(ctx, path, chunk, split_small, P):
    """every batch of the device reader: _device_scan == select_host; -> [(first record, records, selected indices)] per batch"""
    from tiddit_amd import bamio, tiddit_signal
    rd = bamio.DeviceBamReader(path, ctx=ctx, chunk=chunk, split_small=split_small)
    big = np.array([ln >= P["min_contig"] for ln in rd.lengths], dtype=bool)
    out, o = [], 0
    try:
        for b in rd.batches():
            sel = tiddit_signal._device_scan(b, big, P["min_q"], P["max_ins"], P["min_anchor_len"], P["min_clip_len"], ctx=ctx)
            meta, raw_end, raw = sigtab_common.select_host(b, big, P["min_q"], P["max_ins"], P["min_anchor_len"], P["min_clip_len"])
            assert sel.meta.dtype == meta.dtype and len(sel.meta) == len(meta), (o, len(sel.meta), len(meta))
            for f in meta.dtype.names:
                assert np.array_equal(sel.meta[f], meta[f]), (o, f)
            assert sel.raw_end.dtype == np.uint32 and np.array_equal(sel.raw_end, raw_end)
            assert sel.raw.dtype == np.uint8 and np.array_equal(sel.raw, raw)
            assert int((sel.meta["action"] != 0).sum()) == len(meta)
            out.append((o, len(b), sel.meta["idx"].astype(np.int64)))
            o += len(b)
    finally:
        rd.close()
    return out


@pytest.mark.parametrize("chunk", [1 << 28, 1 << 16], ids=["one_batch", "small_chunks"])
@pytest.mark.parametrize("pi", range(3))
def test_signal_scan_vs_select_host(ctx, scan_files, pi, chunk):
    """the action byte, the 28-byte records (field by field), sa_rel, and the byte-exact gather of the raw records, per batch;
    parameter set 0 puts max_ins, min_clip_len and min_anchor_len exactly on the generated edge values"""
    assert len(sc.SCAN_PARAMS) == 3
    P = sc.SCAN_PARAMS[pi]
    path, n_records, spans = scan_files["main"]
    got = _compare_scan(ctx, path, chunk, chunk > 1 << 20, P)
    assert sum(n for _, n, _ in got) == n_records >= 40_000
    records, _ = sc.scan_records()
    want = np.array([sc.record_action(r, P) != 0 for r in records])
    lo, hi = spans["empty"]
    assert not want[lo:hi].any()
    for o, n, idx in got:                                             # selected reads per batch == the literal rules', none in the empty stretch
        assert len(idx) == int(want[o:o + n].sum())
        assert not ((idx + o >= lo) & (idx + o < hi)).any()
    if chunk > 1 << 20:
        assert len(got) == 1 and n_records // 4096 >= 10
    else:
        assert len(got) >= 4


@pytest.mark.parametrize("n_selected", [1023, 1024, 1025])
def test_signal_scan_selected_counts_around_the_gather_tile(ctx, scan_files, n_selected):
    path, n_records, _ = scan_files[n_selected]
    got = _compare_scan(ctx, path, 1 << 28, True, sc.SCAN_EDGE)
    assert [(o, n, len(idx)) for o, n, idx in got] == [(0, n_records, n_selected)]


def test_signal_scan_of_the_empty_stretch_selects_nothing(ctx, tmp_path):
    """a batch of more than two tiles in which no read has an action bit"""
    records, spans = sc.scan_records()
    lo, hi = spans["empty"]
    path = sc.scan_batch(records[lo:hi], tmp_path / "empty.bam")
    assert [(o, n, len(idx)) for o, n, idx in _compare_scan(ctx, path, 1 << 28, True, sc.SCAN_EDGE)] == [(0, hi - lo, 0)]


# ================================================================================================== masked medians
MEDIAN_CASES = sc.median_cases()


def _median_of(lower, upper, count):
    """lower / upper averaged the way tiddit_coverage_analysis.masked_medians does"""
    return np.array([np.mean([lower[s], upper[s]]) if count[s] else np.nan for s in range(len(count))])


def _same(a, b):
    return len(a) == len(b) and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def test_median_case_count():
    assert len(MEDIAN_CASES) == 7 == len(sc.MEDIAN_FAMILIES)


@pytest.mark.parametrize("case", MEDIAN_CASES, ids=[c[0] for c in MEDIAN_CASES])
def test_masked_medians_plain_entry_vs_numpy(nat, ctx, case):
    """tdt_masked_medians on arbitrary, overlapping segments: numpy.median of { cov > 0 and gc != -1 } per segment, NaN and count 0
    where nothing is selected"""
    name, cov, gc, seg = case
    nseg = len(seg)
    lower, upper, count = np.empty(nseg), np.empty(nseg), np.empty(nseg, dtype=np.int64)
    nat.check(ctx.lib.tdt_masked_medians(ctx.handle, nat.ptr(cov), nat.ptr(gc), nat.ptr(seg), nseg, nat.ptr(lower), nat.ptr(upper), nat.ptr(count)))
    med, cnt = sc.median_reference(cov, gc, seg)
    assert np.array_equal(count, cnt)
    got = _median_of(lower, upper, count)
    bad = np.flatnonzero(~((got == med) | (np.isnan(got) & np.isnan(med))))
    assert not len(bad), (name, bad[:5], got[bad[:5]], med[bad[:5]], seg[bad[:5]])
    sel = cnt > 0                                                     # the two middle values themselves
    for s in np.flatnonzero(sel)[:200]:
        lo, hi = seg[s]
        c, g = cov[lo:hi], gc[lo:hi]
        with np.errstate(invalid="ignore"):
            v = np.sort(c[(c > 0) & (g != -1)])
        assert (lower[s], upper[s]) == (v[(len(v) - 1) // 2], v[len(v) // 2]), (name, s)


@pytest.mark.parametrize("case", MEDIAN_CASES, ids=[c[0] for c in MEDIAN_CASES])
def test_masked_medians_parts_vs_numpy(nat, ctx, case):
    """the same data cut into parts (a 1-element part, a 2048-element part, an empty one, a 4096-element one, the rest) through
    tdt_masked_medians_parts and through tiddit_coverage_analysis.masked_medians"""
    from tiddit_amd import tiddit_coverage_analysis as ca
    name, cov, gc, _ = case
    parts, pseg = sc.median_parts(cov, gc, (1, 2049, 2049, 6145))
    assert len(parts) == 5
    med, cnt = sc.median_reference(cov, gc, pseg)
    k = len(parts)
    covs = [np.ascontiguousarray(p[0]) for p in parts]
    gcs = [np.ascontiguousarray(p[1]) for p in parts]
    cov_ptrs = (ctypes.c_void_p * k)(*[c.ctypes.data for c in covs])
    gc_ptrs = (ctypes.c_void_p * k)(*[g.ctypes.data for g in gcs])
    lens = np.array([len(c) for c in covs], dtype=np.int64)
    lower, upper, count = np.empty(k + 1), np.empty(k + 1), np.empty(k + 1, dtype=np.int64)
    nat.check(ctx.lib.tdt_masked_medians_parts(ctx.handle, cov_ptrs, gc_ptrs, nat.ptr(lens), k, nat.ptr(lower), nat.ptr(upper), nat.ptr(count)))
    assert np.array_equal(count, cnt)
    assert _same(_median_of(lower, upper, count), med), name
    per, overall = ca.masked_medians(parts, ctx=ctx)
    assert _same(np.array(per + [overall], dtype=np.float64), med), name
