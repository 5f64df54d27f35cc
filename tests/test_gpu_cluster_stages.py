"""GPU tests of the clustering kernels (csrc/tdt_dbscan.hip, tdt_dbscan_tile.h, tdt_dbscan_fused.h) on the aimed cases of
tests/cluster_stage_cases.py, against its references (pinned on the CPU by test_cluster_stage_refs_cpu.py): every case through
every entry its domain allows — tdt_dbscan_device, tdt_dbscan (as DBSCAN.main / x_coordinate_clustering call it), tdt_sort_dbscan and
tdt_cluster_columns after a shuffle inside every bucket, DBSCAN.y_coordinate_clustering on the reference's x labels for the tile
layouts — and the call-to-call state of the tile-resident pass on one context.  Equality is exact: labels are float64 holding
integers, ids int64.
Run on the MI355X box: python -m pytest tests/test_gpu_cluster_stages.py -m gpu"""
import ctypes

import numpy as np
import pytest

import cluster_stage_cases as cc

pytestmark = pytest.mark.gpu

RAN = {"cases": set(), "pairs": 0}


@pytest.fixture(scope="module")
def nat():
    from tiddit_amd import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def ctx(nat):
    return nat.default_context(0)


def _u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)).to(torch.device("cuda:0"))


def device_call(nat, ctx, x, y, off, eps, m, mode):
    """tdt_dbscan_device on columns offset to their minimum (what its callers pass) -> labels, last ids"""
    import torch
    n, nb = len(x), len(off) - 1
    tx, ty = _u32(x - (x.min() if n else 0)), _u32(y - (y.min() if n else 0))
    tl = torch.full((max(1, n),), -7.0, dtype=torch.float64, device=tx.device)
    tid = torch.full((nb,), -7, dtype=torch.int64, device=tx.device)
    torch.cuda.synchronize()
    off = np.ascontiguousarray(off, dtype=np.int64)
    nat.check(ctx.lib.tdt_dbscan_device(ctx.handle, tx.data_ptr(), ty.data_ptr(), n, nat.ptr(off), nb, int(eps), m, mode,
                                        tl.data_ptr(), tid.data_ptr()))
    ctx.sync()
    return tl.cpu().numpy()[:n], tid.cpu().numpy()


def _host(nat, ctx, c):
    data = np.ascontiguousarray(np.stack([c["x"], c["y"]], 1))
    lab, last = np.full(c["n"], -7.0), ctypes.c_int64(-7)
    nat.check(ctx.lib.tdt_dbscan(ctx.handle, nat.ptr(data), c["n"], 2, float(c["eps"]), c["m"], c["mode"], nat.ptr(lab), ctypes.byref(last)))
    return lab, np.array([last.value], dtype=np.int64)


def _sorted_reference(c, xs, ys, perm):
    """the reference on the stably sorted shuffle: the case's own labels when the order restores the case's columns (no ties in x)"""
    if np.array_equal(xs[perm], c["x"]) and np.array_equal(ys[perm], c["y"]):
        return cc.reference(c)
    return cc.reference_columns(xs[perm], ys[perm], c["off"], c["eps"], c["m"], 0, c["n"] <= cc.LITERAL_MAX)


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return None if not len(bad) else (int(bad[0]), got[bad[0]], want[bad[0]], len(bad))


def run_entry(nat, ctx, c, entry):
    want, wlast = cc.reference(c)
    name = c["name"]
    if entry == "device":
        got, last = device_call(nat, ctx, c["x"], c["y"], c["off"], c["eps"], c["m"], c["mode"])
    elif entry == "host":
        got, last = _host(nat, ctx, c)
    elif entry == "ylabels":
        from tiddit_amd import DBSCAN
        xl, xid = cc.reference(c, mode=1)
        got, cid = DBSCAN.y_coordinate_clustering(np.stack([c["x"], c["y"]], 1), c["eps"], c["m"], int(xid[0]), xl.copy())
        last = np.array([cid], dtype=np.int64)
    else:
        xs, ys, perm = cc.shuffled(c)
        want, wlast = _sorted_reference(c, xs, ys, perm)
        n, nb = c["n"], c["nb"]
        runs, last = np.full(nb, -7, dtype=np.int64), np.full(nb, -7, dtype=np.int64)
        xruns = cc.reference_columns(xs[perm], ys[perm], c["off"], c["eps"], c["m"], 1, False)[1] + 1
        if entry == "sort":
            gp, got = np.full(n, 0xffffffff, dtype=np.uint32), np.full(n, -7.0)
            nat.check(ctx.lib.tdt_sort_dbscan_ex(ctx.handle, nat.ptr(xs), nat.ptr(ys), n, nat.ptr(c["off"]), nb, float(c["eps"]), c["m"], nat.ptr(gp),
                                                 nat.ptr(got), nat.ptr(runs), nat.ptr(last)))
            assert np.array_equal(gp.astype(np.int64), perm), (name, entry, "the permutation is not the stable order")
        else:
            x32, y32 = xs.astype(np.int32), ys.astype(np.int32)
            for max_pos in (0, int(xs.max()) if n else 0):          # without and with the bound on posA that trims the sorted digits
                lab = np.full(n, -7, dtype=np.int32)
                nat.check(ctx.lib.tdt_cluster_columns(ctx.handle, nat.ptr(x32), nat.ptr(y32), n, nat.ptr(c["off"]), nb, float(c["eps"]), c["m"],
                                                      max_pos, nat.ptr(lab), nat.ptr(runs), nat.ptr(last)))
                got = lab.astype(np.float64)[perm]                   # signal order -> sorted order
                assert _first_bad(got, want) is None, (name, entry, max_pos, _first_bad(got, want))
        assert np.array_equal(runs, xruns), (name, entry, "x-run counts")
    assert got.dtype == np.float64 and _first_bad(got, want) is None, (name, entry, c["note"], c["claim"]["route"], _first_bad(got, want))
    assert np.array_equal(last, wlast), (name, entry, "last ids", _first_bad(last, wlast))


@pytest.mark.parametrize("name", cc.case_names())
def test_case_through_every_entry(nat, ctx, name):
    c = cc.get(name)
    for entry in c["entries"]:
        run_entry(nat, ctx, c, entry)
        RAN["pairs"] += 1
    RAN["cases"].add(name)


def test_every_pair_was_run():
    """(after the parametrised test above, in file order) nothing was skipped or deselected: the count is a condition"""
    assert len(RAN["cases"]) == cc.N_CASES and RAN["pairs"] == cc.N_PAIRS, (len(RAN["cases"]), RAN["pairs"])


# ================================================================================================== cross-checks without a reference
@pytest.mark.parametrize("m", cc.A_MS)
def test_one_bucket_equals_the_middle_of_three_with_empty_neighbours(nat, ctx, m):
    ran = 0
    for k in cc.a_member_counts(m):
        for o in cc.A_SEAM_OFFSETS:
            c = cc.get("a_seam_m%d_k%d_o%+d" % (m, k, o))
            for mode in (0, 1):
                one = device_call(nat, ctx, c["x"], c["y"], [0, c["n"]], c["eps"], m, mode)
                three = device_call(nat, ctx, c["x"], c["y"], [0, 0, c["n"], c["n"]], c["eps"], m, mode)
                assert np.array_equal(one[0], three[0]), (c["name"], mode, _first_bad(three[0], one[0]))
                assert three[1].tolist() == [-1, int(one[1][0]), -1], (c["name"], mode)
                ran += 1
    assert ran == 2 * len(cc.a_member_counts(m)) * len(cc.A_SEAM_OFFSETS)


@pytest.mark.parametrize("where", ["start", "end", "seam"])
def test_one_more_member_changes_the_route_and_nothing_else(nat, ctx, where):
    """128 members stay on the tile-resident pass, 129 fall through to the ballot-mask route: the two routes' verdicts side by side
    on the same points — everything outside the big cluster keeps its labels up to the renumbering of the extra sub-runs"""
    a, b = cc.get("b_switch_%s_%d" % (where, cc.DB_SMALL)), cc.get("b_switch_%s_%d" % (where, cc.DB_SMALL + 1))
    la, _ = device_call(nat, ctx, a["x"], a["y"], a["off"], a["eps"], a["m"], 0)
    lb, _ = device_call(nat, ctx, b["x"], b["y"], b["off"], b["eps"], b["m"], 0)
    at = a["claim"]["starts"][0]
    ia = np.concatenate([np.arange(at), np.arange(at + cc.DB_SMALL + (where != "end"), a["n"])])
    ib = np.where(ia < at, ia, ia + 1)
    u, v = la[ia], lb[ib]
    assert np.array_equal(u < 0, v < 0)
    pairs = set(zip(u[u >= 0].tolist(), v[v >= 0].tolist()))
    assert len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


# ================================================================================================== the host entry's domain
def test_span_limit_of_the_host_entry(nat, ctx):
    """a span of exactly 2^32 - 2 is accepted (the d_wide cases); 2^32 - 1 is refused with TDT_E_UNSUPPORTED in either column, and the
    context works afterwards"""
    ok = cc.get("d_wide_n100_eps%d" % ((1 << 32) - 1))
    for col in (0, 1):
        data = np.ascontiguousarray(np.stack([ok["x"], ok["y"]], 1))
        data[np.argmax(data[:, col]), col] += 1
        lab, last = np.full(ok["n"], -7.0), ctypes.c_int64(-7)
        rc = ctx.lib.tdt_dbscan(ctx.handle, nat.ptr(data), ok["n"], 2, float(ok["eps"]), ok["m"], 0, nat.ptr(lab), ctypes.byref(last))
        assert rc == cc.TDT_E_UNSUPPORTED, (col, rc)
        assert (lab == -7.0).all() and last.value == -7
        run_entry(nat, ctx, ok, "host")
        run_entry(nat, ctx, cc.get("a_seam_m3_k128_o-1"), "host")


# ================================================================================================== call-to-call state of route 1
def test_call_to_call_state_on_one_context(nat):
    """One fresh context, a fixed sequence of calls, every call compared with the reference: the status word re-zeroed by the next
    launch, the two group-sum arrays alternating by call parity (and left zero by the other call's finish kernel), tile_groups_max
    only growing.  Then the same sequence on a second fresh context after one extra one-bucket call: every call on the other parity."""
    seq = cc.state_sequence()
    assert [c["claim"]["groups"] for c in seq[:2]] == [3, 1] and seq[2]["claim"]["route"] == 2 and seq[4]["nb"] > 1
    assert seq[5]["n"] == 0 and seq[6]["claim"]["groups"] == 2 and seq[7]["mode"] == 1
    for prefix in ([], [cc.state_prefix()]):
        own = nat.Context(0)
        try:
            for step, c in enumerate(prefix + seq):
                want, wlast = cc.reference(c)
                got, last = device_call(nat, own, c["x"], c["y"], c["off"], c["eps"], c["m"], c["mode"])
                assert _first_bad(got, want) is None, (len(prefix), step, c["name"], _first_bad(got, want))
                assert np.array_equal(last, wlast), (len(prefix), step, c["name"])
        finally:
            own.close()


def test_callers_of_the_tile_pass_share_one_state(nat):
    """The tile-resident pass has ONE driver and ONE layout of its per-call arrays for tdt_dbscan_device and tdt_dbscan_y: what one of
    them leaves behind (codes, group sums, the status word) is what the other finds.  One fresh context, 3 * DT_T points (three tiles,
    two seams): caller-labels, several buckets, caller-labels, one bucket, one bucket falling through to route 2 (ONE cluster of all
    points), caller-labels — every call compared exactly with the reference.  Then the same on a second fresh context after one extra
    one-bucket call: every call on the other parity of the group sums."""
    n = 3 * cc.DT_T
    x, y, _, _ = cc.build_layout([("c", 100)] * (n // 101) + [("g", n % 101)], 3, seed=1)
    lab = cc._case("labels", "E", x, y, cc.EPS, 3, entries=["device"])
    cut = cc._case("buckets", "E", x, y, cc.EPS, 3, off=[0, cc.DT_T - 3, cc.DT_T - 3, 2 * cc.DT_T + 50, n], entries=["device"])
    one = cc._case("one_cluster", "E", np.arange(n), np.zeros(n), cc.EPS, 3, entries=["device"])
    assert lab["n"] == n and cut["nb"] == 4 and cc.properties(one)["largest"] > cc.DB_SMALL
    xl, xid = cc.reference(lab, mode=1)
    want = {c["name"]: cc.reference(c) for c in (lab, cut, one)}
    data = np.ascontiguousarray(np.stack([x, y], 1))

    def caller_labels(own):
        got, last = xl.copy(), ctypes.c_int64(-7)
        nat.check(own.lib.tdt_dbscan_y(own.handle, nat.ptr(data), n, 2, float(cc.EPS), 3, int(xid[0]), nat.ptr(got), ctypes.byref(last)))
        return got, np.array([last.value], dtype=np.int64)

    def device(c):
        return lambda own: device_call(nat, own, c["x"], c["y"], c["off"], c["eps"], c["m"], 0)

    calls = [("labels", caller_labels), ("buckets", device(cut)), ("labels", caller_labels), ("labels", device(lab)),
             ("one_cluster", device(one)), ("labels", caller_labels)]
    for prefix in ([], [("labels", device(lab))]):
        own = nat.Context(0)
        try:
            for step, (name, call) in enumerate(prefix + calls):
                got, last = call(own)
                assert _first_bad(got, want[name][0]) is None, (len(prefix), step, name, _first_bad(got, want[name][0]))
                assert np.array_equal(last, want[name][1]), (len(prefix), step, name, last, want[name][1])
        finally:
            own.close()


def test_too_large_cluster_after_a_caller_labels_call(nat):
    """The reduced form of what b_mixed_4095_m3 met after the caller-labels calls of family A: the members of a cluster too large for
    the tile-resident pass get no code, so its finish kernel decodes what an earlier call left in the code array before the call
    falls through — and the codes a tdt_dbscan_y call leaves say `take the caller's x label`, which this call does not have.
    One fresh context: a caller-labels call that leaves such a code on every position, then ONE cluster of all points."""
    n = 3 * cc.DT_T
    x, y, _, _ = cc.build_layout([("c", 100)] * (n // 101) + [("g", n % 101)], 3, seed=1, y_kind="equal")
    lab = cc._case("labels", "E", x, y, cc.EPS, 3, entries=["device"])
    xl, xid = cc.reference(lab, mode=1)
    want, wlast = cc.reference(lab)
    one = cc._case("one_cluster", "E", np.arange(n), np.zeros(n), cc.EPS, 3, entries=["device"])
    own = nat.Context(0)
    try:
        data, got, last = np.ascontiguousarray(np.stack([x, y], 1)), xl.copy(), ctypes.c_int64(-7)
        nat.check(own.lib.tdt_dbscan_y(own.handle, nat.ptr(data), n, 2, float(cc.EPS), 3, int(xid[0]), nat.ptr(got), ctypes.byref(last)))
        assert np.array_equal(got, want) and last.value == wlast[0]
        got, last = device_call(nat, own, one["x"], one["y"], one["off"], one["eps"], one["m"], 0)
        assert (got == 0).all() and last.tolist() == [0] and np.array_equal(got, cc.reference(one)[0])
        got, last = device_call(nat, own, lab["x"], lab["y"], lab["off"], lab["eps"], lab["m"], 0)      # and the context works afterwards
        assert np.array_equal(got, want) and np.array_equal(last, wlast)
    finally:
        own.close()
