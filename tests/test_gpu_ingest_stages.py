"""The BAM ingest kernels (csrc/tdt_ingest.hip: bam_find_first, bam_find_records, bam_decode_fields and its _second, _serial and
_serial_second flavours, bam_tid_edges) on the record streams of tests/ingest_cases.py, which are AIMED at the 16 KiB segment grid, the
lane-per-record decode, batch tails, the guess-and-confirm contract, sharded seams and the edge cap.  Every case is driven directly
through tdt_ingest_create / tdt_ingest_push (tdt_ingest_push_bounded for the seams) with its own block groups; the thirteen columns,
the batch's raw bytes, the coverage-record columns, the contig runs, the record count of every push, the final carry and host_chases
are compared with the struct-walk reference of ingest_cases — `np.array_equal` throughout, no tolerance anywhere.

Routes: "wave" (the wave-per-segment decode), "serial" (TIDDIT_INGEST_HOST_CHASE=1: every batch chased on the host and decoded by the
lane-per-segment kernels), "second_binned" / "second_generic" (a second histogram attached, with and without a binned record form, and
the first column bound to a histogram with tdt_ingest_bin_for), "ahead" (spans begun through tdt_ingest_push_ahead), "sharded".
94 cases, 187 (case, route) pairs; the ledger test at the end holds the run to exactly that list."""
import ctypes
import time

import numpy as np
import pytest

import ingest_cases as ic
from tiddit_amd import _native

pytestmark = pytest.mark.gpu

RAN = set()
T0 = time.perf_counter()
_SZ = ctypes.c_size_t
NOTHING = ic.SIZE_MAX


@pytest.fixture(scope="module")
def ctx():
    return _native.default_context()


@pytest.fixture(scope="module")
def hists(ctx):
    """histograms over the cases' contigs: the first column's (bin size 50), a second one with a binned record form (100) and one without (2000)"""
    from tiddit_amd import tiddit_coverage
    return {z: tiddit_coverage.CoverageHistogram(ic.REFS, z, ctx=ctx) for z in (50, 100, 2000)}


def _host(ctx, dptr, n, dtype):
    a = np.empty(n, dtype=dtype)
    if n:
        assert dptr, "a device pointer is missing"
        _native.check(ctx.lib.tdt_copy_to_host(ctx.handle, _native.ptr(a), ctypes.c_void_p(dptr), a.nbytes))
    return a


def _fetch(ctx, h, n, second):
    """the current batch of reader h on the host: columns, raw bytes, packed column(s), edges, and the device pointers"""
    lib = ctx.lib
    ptrs = (ctypes.c_void_p * 14)()
    raw_len = _SZ(0)
    _native.check(lib.tdt_ingest_arrays(h, ptrs, ctypes.byref(raw_len)))
    G = {"dev": {k: int(ptrs[i] or 0) for i, k in enumerate(ic.COLUMNS)}}
    for i, (k, t) in enumerate(zip(ic.COLUMNS, ic.TYPES)):
        G[k] = _host(ctx, int(ptrs[i] or 0), n, t)
    G["raw"] = _host(ctx, int(ptrs[13] or 0), raw_len.value, np.uint8).tobytes()
    pk = ctypes.c_void_p()
    _native.check(lib.tdt_ingest_packed(h, ctypes.byref(pk)))
    G["packed"] = _host(ctx, int(pk.value or 0), n, np.uint64)
    if second:
        pk2 = ctypes.c_void_p()
        _native.check(lib.tdt_ingest_packed_second(h, ctypes.byref(pk2)))
        assert bool(pk2.value) == bool(n)
        G["packed2"] = _host(ctx, int(pk2.value or 0), n, np.uint64)
    edges = np.full(ic.EDGES + 2, 0xdeadbeef, dtype=np.uint32)
    tids = np.full(ic.EDGES + 2, -77, dtype=np.int32)
    ne = _SZ(0)
    _native.check(lib.tdt_ingest_edges(h, _native.ptr(edges), len(edges), ctypes.byref(ne)))
    if ne.value == NOTHING:
        G["edges"] = G["edge_tids"] = None
    else:
        _native.check(lib.tdt_ingest_edge_tids(h, _native.ptr(tids), len(tids)))
        G["edges"], G["edge_tids"] = edges[:ne.value], tids[:ne.value]
        assert np.all(edges[ne.value:] == 0xdeadbeef) and np.all(tids[ne.value:] == -77)
    return G


def _compare(name, b, G, B):
    """one batch: got G against the expectation B of ingest_cases"""
    n = B["n"]
    assert G["raw"] == B["raw"], (name, b, "the batch's bytes: carried record + inflated span")
    for k in ic.COLUMNS:
        assert np.array_equal(G[k], B[k]), (name, b, k, np.flatnonzero(G[k] != B[k])[:8])
    raw = G["raw"]
    for i in range(n):                                              # rec_off / sa_off by the bytes they point at
        o = int(G["rec_off"][i])
        assert raw[o + 4:o + 12] == B["tid"][i].tobytes() + B["pos"][i].tobytes(), (name, b, i)
    for i in np.flatnonzero(G["sa_off"] >= 0).tolist():
        s = int(G["sa_off"][i])
        assert raw[s - 3:s] == b"SAZ" and int(G["rec_off"][i]) < s < int(G["rec_off"][i]) + 4 + int.from_bytes(raw[int(G["rec_off"][i]):int(G["rec_off"][i]) + 4], "little"), (name, b, i)
    assert np.array_equal(G["packed"], B["packed"]) or "binned" in B, (name, b, "packed")
    if B["edges"] is None:
        assert G["edges"] is None, (name, b, "more than ING_EDGES runs must be reported as (size_t)-1")
    else:
        assert G["edges"] is not None and np.array_equal(G["edges"], B["edges"]) and np.array_equal(G["edge_tids"], B["edge_tids"]), (name, b, "runs")


def _binned_want(ctx, hist, G, B, n_ref):
    """what tdt_cov_pack_binned_device (or, for a histogram without a binned form, tdt_cov_pack_device) writes from the batch's arrays"""
    import torch
    n = B["n"]
    dev = torch.device("cuda", ctx.device)
    want = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    d = G["dev"]
    if not hist.has_binned():
        _native.check(ctx.lib.tdt_cov_pack_device(ctx.handle, d["pos"], d["end"], d["mapq"], d["flag"], n, want.data_ptr()))
        ctx.sync()
        return want.cpu().numpy().view(np.uint64)[:n]
    lo = np.concatenate([[0], np.flatnonzero(np.diff(B["tid"])) + 1]).astype(np.int64) if n else np.zeros(0, np.int64)
    hi = np.concatenate([lo[1:], [n]]).astype(np.int64)
    for l, h in zip(lo.tolist(), hi.tolist()):
        t = int(B["tid"][l])
        if 0 <= t < n_ref:
            hist.pack_binned_device(t, d["pos"] + 4 * l, d["end"] + 4 * l, d["mapq"] + l, d["flag"] + 2 * l, h - l, want.data_ptr() + 8 * l)
    ctx.sync()
    want = want.cpu().numpy().view(np.uint64)[:n].copy()
    out = (B["tid"] < 0) | (B["tid"] >= n_ref)                      # no contig whose bins could be packed: the INVALID shape, bin 0, the filter byte
    top = (np.minimum(B["mapq"].astype(np.uint64), 63) << np.uint64(24)) | (((B["flag"].astype(np.uint64) >> np.uint64(2)) & np.uint64(1)) << np.uint64(30)) | \
          (((B["flag"].astype(np.uint64) >> np.uint64(10)) & np.uint64(1)) << np.uint64(31))
    want[out] = ((top << np.uint64(32)) | np.uint64(3))[out]
    return want


def _run(ctx, case, route, hists, monkeypatch):
    lib = ctx.lib
    if route == "serial":
        monkeypatch.setenv("TIDDIT_INGEST_HOST_CHASE", "1")
    else:
        monkeypatch.delenv("TIDDIT_INGEST_HOST_CHASE", raising=False)
    second = route.startswith("second")
    Bs = case.batches(model=False)
    comps = [np.frombuffer(bytearray(c), dtype=np.uint8) for c in case.comp_pushes()]
    h = ctypes.c_void_p()
    _native.check(lib.tdt_ingest_create(ctx.handle, case.n_ref, ctypes.byref(h)))
    try:
        if second:
            on = ctypes.c_int(-1)
            _native.check(lib.tdt_ingest_bin_for(h, hists[50].handle, ctypes.byref(on)))
            assert on.value == 1
            h2 = hists[100 if route == "second_binned" else 2000]
            _native.check(lib.tdt_ingest_second_for(h, h2.handle, ctypes.byref(on)))
            assert on.value == (route == "second_binned") == h2.has_binned()
        if route == "ahead":
            _native.check(lib.tdt_ingest_push_ahead(h, _native.ptr(comps[0]), len(comps[0])))
        for b, (comp, B) in enumerate(zip(comps, Bs)):
            if route == "ahead" and b + 1 < len(comps):
                _native.check(lib.tdt_ingest_push_ahead(h, _native.ptr(comps[b + 1]), len(comps[b + 1])))
            n = _SZ(NOTHING)
            _native.check(lib.tdt_ingest_push(h, _native.ptr(comp), len(comp), case.skip if b == 0 else 0, ctypes.byref(n)))
            assert n.value == B["n"], (case.name, route, b, "records of the push")
            G = _fetch(ctx, h, n.value, second)
            if second:
                B = dict(B, binned=True)
            _compare(case.name, b, G, B)
            if second and n.value:
                assert np.array_equal(G["packed"], _binned_want(ctx, hists[50], G, B, case.n_ref)), (case.name, route, b, "tdt_ingest_bin_for column")
                want2 = _binned_want(ctx, h2, G, B, case.n_ref)
                assert np.array_equal(G["packed2"], want2), (case.name, route, b, "second column")
                if route == "second_generic":
                    assert np.array_equal(G["packed2"], B["packed"]), (case.name, route, b, "second column against the layout's restatement")
            c, hc = _SZ(NOTHING), _SZ(NOTHING)
            _native.check(lib.tdt_ingest_carry(h, ctypes.byref(c), ctypes.byref(hc)))
            assert c.value == B["carry"], (case.name, route, b, "carry")
        assert c.value == 0
        want_hc = sum(1 for B in Bs if B["searched"]) if route == "serial" else len(case.chased)
        assert hc.value == want_hc, (case.name, route, "host_chases", hc.value, want_hc)
    finally:
        lib.tdt_ingest_destroy(h)
    RAN.add((case.name, route))


@pytest.mark.parametrize("route", ["wave", "serial"])
@pytest.mark.parametrize("family", ["A", "B", "C", "D", "E"])
def test_legal_streams_both_decode_routes(ctx, hists, family, route, monkeypatch):
    """families A-E through the wave kernels (not one batch chased) and again through the host chase and the serial kernels"""
    for case in ic.by_family(family):
        assert case.chased == [] and route in case.routes
        _run(ctx, case, route, hists, monkeypatch)


@pytest.mark.parametrize("family", ["F", "G", "I"])
def test_decoys_refused_records_and_runs(ctx, hists, family, monkeypatch):
    """F / G: the reference's records, and exactly the batches the case states in host_chases; I: the runs at the cap"""
    for case in ic.by_family(family):
        _run(ctx, case, "wave", hists, monkeypatch)


@pytest.mark.parametrize("route", ["second_binned", "second_generic", "ahead"])
def test_second_column_and_spans_begun_ahead(ctx, hists, route, monkeypatch):
    todo = [c for c in ic.cases() if route in c.routes]
    assert len(todo) == (2 if route == "ahead" else 8)
    for case in todo:
        _run(ctx, case, route, hists, monkeypatch)


def _bounded(ctx, case, comp, skip, own, second_shard):
    lib = ctx.lib
    comp = np.frombuffer(bytearray(comp), dtype=np.uint8)
    h = ctypes.c_void_p()
    _native.check(lib.tdt_ingest_create(ctx.handle, case.n_ref, ctypes.byref(h)))
    try:
        n, fo, no = _SZ(NOTHING), _SZ(NOTHING), _SZ(NOTHING)
        _native.check(lib.tdt_ingest_push_bounded(h, _native.ptr(comp), len(comp), skip, own, ctypes.byref(n), ctypes.byref(fo),
                                                  None if second_shard else ctypes.byref(no)))
        G = _fetch(ctx, h, n.value, False)
        c, hc = _SZ(NOTHING), _SZ(NOTHING)
        _native.check(lib.tdt_ingest_carry(h, ctypes.byref(c), ctypes.byref(hc)))
        assert c.value == 0 and hc.value == 0, (case.name, c.value, hc.value)
    finally:
        lib.tdt_ingest_destroy(h)
    return n.value, fo.value, no.value, G


def test_sharded_seams(ctx, monkeypatch):
    """tdt_ingest_push_bounded twice on one device: the first shard ends at own_bytes and reports where the next record starts, the
    second starts at the block boundary with an unknown first record; a decoy at the seam shows as first_off != next_off"""
    monkeypatch.delenv("TIDDIT_INGEST_HOST_CHASE", raising=False)
    for case in ic.by_family("H"):
        e = ic.shard_expectation(case)
        R = case.reference()
        blocks, j, own = case.shard_blocks()
        eof = __import__("tiddit_amd").bamio._BGZF_EOF
        n0, fo0, no0, G0 = _bounded(ctx, case, b"".join(blocks) + eof, case.skip, own, False)
        assert (n0, fo0, no0) == (e["n0"], case.skip, e["next_off"]), (case.name, n0, fo0, no0)
        assert G0["raw"] == case.stream
        for k in ic.COLUMNS:
            assert np.array_equal(G0[k], R[k][:n0]), (case.name, "shard 0", k)
        assert np.array_equal(G0["packed"], R["packed"][:n0])
        r = ic.runs_of(R["tid"][:n0])
        assert np.array_equal(G0["edges"], r[0]) and np.array_equal(G0["edge_tids"], r[1])
        n1, fo1, _, G1 = _bounded(ctx, case, b"".join(blocks[j:]) + eof, NOTHING, NOTHING, True)
        extra = 1 if case.decoys else 0
        assert n1 == len(R["tid"]) - n0 + extra == e["model1"]["n"], (case.name, n1)
        assert G1["raw"] == case.stream[own:]
        if case.decoys:
            assert fo1 != no0, (case.name, "a decoy at the seam must show as a seam disagreement")
            assert fo1 == case.decoys[0]["off"] - own == int(G1["rec_off"][0])
        else:
            assert fo1 == no0, (case.name, fo1, no0)
        for k in ic.COLUMNS:
            want = R[k][n0:]
            if k == "rec_off":
                want = want - np.uint64(own)
            if k == "sa_off":
                want = np.where(want >= 0, want - own, want)
            assert np.array_equal(G1[k][extra:], want), (case.name, "shard 1", k)
        assert np.array_equal(G1["packed"][extra:], R["packed"][n0:])
        RAN.add((case.name, "sharded"))


def test_ledger_every_case_ran_on_every_route_it_lists():
    assert sorted(RAN) == ic.ledger() and len(RAN) == 187, sorted(set(ic.ledger()) ^ RAN)
    print("ingest stage suite: %d (case, route) pairs in %.1f s" % (len(RAN), time.perf_counter() - T0))
