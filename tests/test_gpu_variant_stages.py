"""GPU tests that call the device pieces of the native variant stage directly, on the adversarial inputs of
tests/variant_stage_cases.py and against its plain references (pinned on the CPU by test_variant_stage_refs_cpu.py):
  * the region counts (csrc/tdt_region.hip: region_counts, region_counts_packed<CHECK>, rg_lower_bound2<S>): for every query of
    every family the same seven int64 from all four entries — tdt_region_counts (host columns, span computed on the host),
    tdt_region_counts_device (device columns, span supplied), EvidenceStore.region_counts (packed, span from the pack kernel's
    atomicMax) and EvidenceStore.region_counts_device (queries and output in HBM) — each against the reference;
  * the evidence store (evidence_pack, ev_reserve): records and spans against pack_reference through the host and the device-column
    append, after every append, through both growth rules of the reserve;
  * the segment means (csrc/tdt_means.hip: seg_means) against numpy.average itself.
No tolerance anywhere: the counts are integers and the means are bit-exact by design.
Run on the MI355X box: python -m pytest tests/test_gpu_variant_stages.py -m gpu"""
import ctypes
import functools
import types
import warnings

import numpy as np
import pytest

import variant_stage_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from tiddit_amd import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def ctx(nat):
    return nat.default_context(0)


def _tensor(a, dev):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _make_store(case, capacity=0):
    from tiddit_amd import tiddit_region
    return tiddit_region.EvidenceStore(case["name"], case["names"], case["lengths"], case["min_q"], case["max_ins"], capacity=capacity)


def _append_device(store, cols):
    """the device-column append on torch tensors: the nine columns in HBM, the runs of the batch as the device reader states them"""
    import torch
    dev = torch.device("cuda", store.ctx.device)
    ten = {k: _tensor(np.ascontiguousarray(cols[k]), dev) for k in vc.COLS}
    torch.cuda.synchronize(dev)                                     # torch's copies run on its stream, the library on its own
    tid = cols["tid"]
    edges = np.flatnonzero(np.diff(tid)) + 1
    runs = [(int(tid[lo]), int(lo), int(hi)) for lo, hi in zip(np.concatenate([[0], edges]), np.concatenate([edges, [len(tid)]]))] if len(tid) else []
    store.add_device_batch(types.SimpleNamespace(runs=runs, dev={k: ten[k].data_ptr() for k in vc.COLS}))
    store.ctx.sync()                                                # (the tensors are released after the pack kernel has read them)


def _append(store, cols, device):
    if device:
        _append_device(store, cols)
    else:
        store.add_host_batch(types.SimpleNamespace(**cols))


# ================================================================================================== region counts
def test_counts_case_count():
    names = vc.counts_case_names()
    assert len(names) == 13 and names[0] == "predicate_edges" and names[-1] == "far_read"
    assert [n for n in names if n.startswith("search_n2")] == ["search_n%d" % n for n in vc.SEARCH_LARGE]


def _host_columns(nat, ctx, tab, tid, L, q, min_q, max_ins):
    out = np.full((len(q), 7), -1, dtype=np.int64)
    qs, qe, qb = (np.ascontiguousarray(q[:, j], dtype=np.int32) for j in (1, 2, 3))
    nat.check(ctx.lib.tdt_region_counts(ctx.handle, *[nat.ptr(tab[k]) for k in vc.TABLE_KEYS], len(tab["start"]), tid, L, nat.ptr(qs),
                                        nat.ptr(qe), nat.ptr(qb), len(q), min_q, max_ins, nat.ptr(out)))
    return out


def _device_columns(nat, ctx, tab, tid, span, L, q, min_q, max_ins):
    import torch
    dev = torch.device("cuda", ctx.device)
    ten = [_tensor(tab[k], dev) for k in vc.TABLE_KEYS]
    qs, qe, qb = (_tensor(np.ascontiguousarray(q[:, j], dtype=np.int32), dev) for j in (1, 2, 3))
    out = torch.full((len(q), 7), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    n = len(tab["start"])
    nat.check(ctx.lib.tdt_region_counts_device(ctx.handle, *[(x.data_ptr() if n else None) for x in ten], n, tid, span, L, qs.data_ptr(),
                                               qe.data_ptr(), qb.data_ptr(), len(q), min_q, max_ins, out.data_ptr()))
    ctx.sync()
    return out.cpu().numpy()


def _packed_device(store, q, min_q, max_ins):
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32).reshape(-1, 4)).cuda()
    out = torch.full((len(q), 7), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert dq.data_ptr() % 16 == 0
    store.region_counts_device(dq.data_ptr(), len(q), min_q, max_ins, out.data_ptr())
    return out.cpu().numpy()


@pytest.mark.parametrize("name", vc.counts_case_names())
def test_region_counts_from_all_four_entries(nat, ctx, name):
    """Every query, every entry, against get_region_numpy (== the literal loop == the C oracle on the CPU).  The store is filled
    through the host append here; its records and spans are held to pack_reference on the way."""
    case = vc.counts_case(name)
    q, min_q, max_ins, lengths = case["queries"], case["min_q"], case["max_ins"], case["lengths"]
    tabs = {t: vc.contig_table(case["cols"], t) for t in range(len(lengths))}
    want = np.array([vc.get_region_numpy(tabs[int(t)], int(t), lengths[int(t)], int(s), int(e), int(bp), min_q, max_ins) for t, s, e, bp in q])
    assert len(q) <= 5 or want[:, 1].sum() > 0
    rec, spans = vc.pack_reference(case["cols"], min_q, max_ins, len(lengths))
    # 1, 2: the per-contig kernel over columns — the span computed by the host entry, and supplied
    for t in sorted(set(q[:, 0].tolist())):
        m = q[:, 0] == t
        got = _host_columns(nat, ctx, tabs[t], t, lengths[t], q[m], min_q, max_ins)
        bad = np.flatnonzero((got != want[m]).any(axis=1))
        assert not len(bad), ("tdt_region_counts", name, q[m][bad[0]], got[bad[0]], want[m][bad[0]], len(bad))
        got = _device_columns(nat, ctx, tabs[t], t, max(1, int(spans[t])), lengths[t], q[m], min_q, max_ins)
        bad = np.flatnonzero((got != want[m]).any(axis=1))
        assert not len(bad), ("tdt_region_counts_device", name, q[m][bad[0]], got[bad[0]], want[m][bad[0]], len(bad))
    # 3, 4: one launch over the store
    store = _make_store(case)
    try:
        _append(store, case["cols"], device=False)
        assert store.n == len(rec) and np.array_equal(store.spans(), spans)
        for fn, got in (("region_counts", store.region_counts(q, min_q, max_ins)), ("region_counts_device", _packed_device(store, q, min_q, max_ins))):
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (fn, name, q[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    finally:
        store.close()


def test_far_read_is_found_through_every_span(nat, ctx):
    """the span family once more, by what it is there for: the query starting 1 before the far read's end counts it through all
    entries, and an entry told a span two short of the true one must lose exactly that read (the lower bound does use the span)"""
    case = vc.counts_case("far_read")
    tab = vc.contig_table(case["cols"], 1)
    q = case["queries"][:1]
    L, min_q, max_ins = case["lengths"][1], case["min_q"], case["max_ins"]
    true_span = int((tab["end"].astype(np.int64) - tab["start"]).max())
    want = vc.get_region_numpy(tab, 1, L, *[int(x) for x in q[0, 1:]], min_q, max_ins)
    assert np.array_equal(_device_columns(nat, ctx, tab, 1, true_span, L, q, min_q, max_ins)[0], want)
    short = _device_columns(nat, ctx, tab, 1, true_span - 2, L, q, min_q, max_ins)[0]      # (- 1 still finds it: first start >= key)
    assert short[1] == want[1] - 1 and short[0] == want[0] - 2


# ================================================================================================== the evidence store
def _capacity(nat, store):
    cap = ctypes.c_size_t(0)
    nat.check(store.ctx.lib.tdt_evstore_info(store.handle, None, ctypes.byref(cap), None))
    return cap.value


def _check_store(store, cols_so_far, case, where):
    rec, spans = vc.pack_reference(cols_so_far, case["min_q"], case["max_ins"], len(case["names"]))
    tid = cols_so_far["tid"][cols_so_far["tid"] >= 0]
    assert store.n == len(rec), where
    assert np.array_equal(store.spans(), spans), (where, store.spans(), spans)
    for t in range(len(case["names"])):
        want = rec[tid == t]
        got = store.records(t)
        assert len(got) == len(want) == store.count[t], (where, t)
        for f in ("start", "end", "mate_pos", "bits"):
            assert np.array_equal(got[f], want[f]), (where, t, f)
        assert not got["pad"].any(), (where, t)


@functools.lru_cache(maxsize=1)
def _pack_cases(large):
    return {c["name"]: c for c in vc.pack_cases(large=large)}


@pytest.mark.parametrize("device", [False, True], ids=["host_append", "device_append"])
@pytest.mark.parametrize("name", vc.PACK_SMALL + vc.PACK_LARGE)
def test_evidence_store_equals_pack_reference(nat, ctx, name, device):
    """records(t) and spans() field for field after EVERY append (so the records of the first appends are read back after each
    growth), and the capacity after every append is the one the reserve's rule gives: the floor and the x1.5 growth both run with
    records in the store"""
    case = _pack_cases(name in vc.PACK_LARGE)[name]
    store = _make_store(case, capacity=case["capacity"])
    try:
        caps, why = vc.expected_capacities(case["capacity"], [int((b["tid"] >= 0).sum()) for b in case["batches"]])
        seen = []
        for i, b in enumerate(case["batches"]):
            _append(store, b, device)
            seen.append(b)
            assert _capacity(nat, store) == caps[i], (name, i, why[i])
            _check_store(store, vc.concat_cols(seen), case, (name, "after append", i))
        if name in vc.PACK_LARGE:
            assert "x1.5" in why and "floor" in why
    finally:
        store.close()


# ================================================================================================== segment means
@pytest.mark.parametrize("family", vc.VALUE_FAMILIES)
def test_segment_means_on_aimed_kept_counts(ctx, family):
    from tiddit_amd import tiddit_region
    cov, gc, segs, masked, kept = vc.means_case(family)
    table = tiddit_region.BinTable(cov, gc)
    mean, count = tiddit_region.region_means(table, segs, masked)
    assert np.array_equal(count, kept)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, (name, s, e) in enumerate(segs):
            a = cov[name][s:e]
            if masked[i]:
                a = a[gc[name][s:e] > -1]
            assert len(a) == kept[i]
            want = np.average(a) if len(a) else np.nan
            assert (mean[i] == want and np.signbit(mean[i]) == np.signbit(want)) or (np.isnan(mean[i]) and np.isnan(want)), \
                (family, name, masked[i], mean[i], want)
