"""GPU tests of the coverage kernels (csrc/tdt_coverage.hip, csrc/tdt_cov_record.h) on the aimed cases of
tests/coverage_stage_cases.py, against its references (pinned on the CPU by test_coverage_stage_refs_cpu.py): every case through every
entry in its `layouts` — CoverageHistogram.push, push_device, push_device_multi, tdt_cov_pack_device + push_packed_device_multi,
pack_binned_device + push_binned_device_multi — and, for bin sizes 2..128, again in a histogram created under TIDDIT_COV_MODE=0:
377 cases, 2100 (case, layout) pairs (test_coverage_stage_refs_cpu.py pins both numbers), then the call-to-call state of one
histogram (family H).  Equality is exact: float64 bins compared with np.array_equal, kept-read counts and error codes with ==.
Run on the MI355X box: python -m pytest tests/test_gpu_coverage_stages.py -m gpu"""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import coverage_stage_cases as cc

pytestmark = pytest.mark.gpu

RAN = {"cases": set(), "pairs": 0}
_HISTS = {}
_REFS = {}


@pytest.fixture(scope="module")
def nat():
    from tiddit_amd import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def ctx(nat):
    return nat.default_context(0)


@pytest.fixture(scope="module")
def cov(ctx):
    from tiddit_amd import tiddit_coverage
    yield tiddit_coverage
    while _HISTS:
        _HISTS.popitem()[1].close()


@contextmanager
def cov_mode(value):
    """TIDDIT_COV_MODE as the histogram's constructor sees it"""
    old = os.environ.pop("TIDDIT_COV_MODE", None)
    if value is not None:
        os.environ["TIDDIT_COV_MODE"] = value
    try:
        yield
    finally:
        os.environ.pop("TIDDIT_COV_MODE", None)
        if old is not None:
            os.environ["TIDDIT_COV_MODE"] = old


def histogram(cov, c, mode0):
    """one histogram per (bin size, contigs, flavour), reset between cases; the few with a 2^31 - 1 contig are not kept"""
    key = (c["z"], tuple(c["contigs"]), mode0)
    h = _HISTS.get(key)
    if h is None:
        while len(_HISTS) >= 12:
            _HISTS.pop(next(iter(_HISTS))).close()
        with cov_mode("0" if mode0 else None):
            h = cov.CoverageHistogram(c["contigs"], c["z"])
        if not c.get("big"):
            _HISTS[key] = h
    h.reset()
    return h


class DeviceColumns:
    """a case's columns on the device, every column `misalign` elements into its allocation"""

    def __init__(self, c):
        import torch
        dev, self.off, self.keep = torch.device("cuda:0"), c["misalign"], []
        self.ptr = []
        for cols in c["cols"]:
            p = []
            for a in cols:
                t = torch.empty(len(a) + self.off + 16, dtype={4: torch.int32, 1: torch.uint8, 2: torch.int16}[a.itemsize], device=dev)
                if len(a):
                    t[self.off:self.off + len(a)] = torch.from_numpy(a.view({4: np.int32, 1: np.uint8, 2: np.int16}[a.itemsize]))
                self.keep.append(t)
                p.append(t.data_ptr() + self.off * a.itemsize)
            rec = torch.zeros(len(cols[0]) + self.off + 16, dtype=torch.int64, device=dev)      # packed / binned records of this contig
            self.keep.append(rec)
            p.append(rec.data_ptr() + 8 * self.off)
            self.ptr.append(p)
        torch.cuda.synchronize()


def push(nat, ctx, h, c, dc, layout):
    q, names = c["min_q"], [n for n, _ in c["contigs"]]
    items = [(ci, lo, hi) for ci, lo, hi in c["items"]]
    P = dc.ptr
    if layout == "host":
        for ci, lo, hi in items:
            h.push(names[ci], *(a[lo:hi] for a in c["cols"][ci]), q)
    elif layout == "arrays":
        for ci, lo, hi in items:
            h.push_device(names[ci], P[ci][0] + 4 * lo, P[ci][1] + 4 * lo, P[ci][2] + lo, P[ci][3] + 2 * lo, hi - lo, q)
    elif layout == "arrays_multi":
        h.push_device_multi([(names[ci], P[ci][0] + 4 * lo, P[ci][1] + 4 * lo, P[ci][2] + lo, P[ci][3] + 2 * lo, hi - lo) for ci, lo, hi in items], q)
    elif layout == "packed":
        for ci, cols in enumerate(c["cols"]):
            nat.check(ctx.lib.tdt_cov_pack_device(ctx.handle, P[ci][0], P[ci][1], P[ci][2], P[ci][3], len(cols[0]), P[ci][4]))
        h.push_packed_device_multi([(names[ci], P[ci][4] + 8 * lo, 0 if c["null_end"] else P[ci][1] + 4 * lo, hi - lo) for ci, lo, hi in items], q)
    else:
        for ci, cols in enumerate(c["cols"]):
            h.pack_binned_device(names[ci], P[ci][0], P[ci][1], P[ci][2], P[ci][3], len(cols[0]), P[ci][4])
        h.push_binned_device_multi([(names[ci], P[ci][4] + 8 * lo, P[ci][0] + 4 * lo, P[ci][1] + 4 * lo, hi - lo) for ci, lo, hi in items], q)


def first_bad(got, want):
    """-> None, or (first differing bin, got, want, number of differing bins) of a dense result against (indices, values)"""
    idx, val = want
    nz = np.flatnonzero(got)
    if np.array_equal(nz, idx) and np.array_equal(got[nz], val):
        return None
    w = np.zeros(len(got))
    w[idx] = val
    bad = np.flatnonzero(got != w)
    return int(bad[0]), float(got[bad[0]]), float(w[bad[0]]), len(bad)


def wanted(c):
    if c["name"] not in _REFS:
        _REFS[c["name"]] = cc.reference(c)
    return _REFS[c["name"]]


def check_bins(h, c, want, where):
    assert all(v.dtype == np.float64 for _, v in want)
    names = [n for n, _ in c["contigs"]]
    allb = h.finish_all() if len(names) > 1 else None
    for ci, name in enumerate(names):
        nb = h.nbins(name)[0]
        assert nb == cc.nbins_of(c["contigs"][ci][1], c["z"]), (where, name)
        got = h.finish(name) if allb is None else allb[h.offset(name):h.offset(name) + nb]
        assert got.dtype == np.float64 and len(got) == nb
        assert first_bad(got, want[ci]) is None, (where, name, c["claim"]["flavour"], first_bad(got, want[ci]))


def run_pair(nat, ctx, cov, c, dc, layout, mode0):
    where = (c["name"], layout, "TIDDIT_COV_MODE=0" if mode0 else "")
    h = histogram(cov, c, mode0)
    try:
        code = c["expect_by_layout"].get(layout)
        if code is not None:                                       # refused at the push, nothing accumulated
            with pytest.raises(nat.TdtError) as err:
                push(nat, ctx, h, c, dc, layout)
            assert err.value.code == code, where
            assert h.kept() == 0, where
            return
        push(nat, ctx, h, c, dc, layout)
        if c["expect"] != "bins":
            with pytest.raises(nat.TdtError) as err:
                h.finish(0)
            assert err.value.code == c["expect"], where
            return
        want, kept = wanted(c)
        check_bins(h, c, want, where)
        assert h.kept() == kept, (where, h.kept(), kept)
    finally:
        ctx.sync()
        if c.get("big"):
            h.close()


@pytest.mark.parametrize("name", cc.case_names())
def test_case_through_every_layout(nat, ctx, cov, name):
    c = cc.get(name)
    dc = DeviceColumns(c)
    for mode0 in ((False, True) if c["mode0"] else (False,)):
        for layout in c["layouts"]:
            run_pair(nat, ctx, cov, c, dc, layout, mode0)
            RAN["pairs"] += 1
    RAN["cases"].add(name)


def test_every_pair_was_run():
    """(after the parametrised test above, in file order) nothing was skipped or deselected: the count is a condition"""
    assert len(RAN["cases"]) == cc.N_CASES and RAN["pairs"] == cc.N_PAIRS, (len(RAN["cases"]), RAN["pairs"])


def test_unrepresentable_overhang_quotient_is_refused_not_dropped(nat, ctx, cov):
    """What d_contig_end_z1048576 met: a read overhanging a contig whose last bin holds one base adds (z - 1) / 1 to that bin, 2^64
    fixed-point units at this bin size.  The end-bin table used to hold 0 for such an entry, so the bins came back without the
    contribution and without an error; it now holds 2^53 and `finish` answers TDT_E_INEXACT.  A contig whose quotients fit is exact."""
    c = cc.get("d_overhang_unrepresentable_z%d" % (1 << 20))
    assert cc.restatement(c)[0][0][1][-1] == 1 << 20               # the reference's own bin: (z - 1) / 1 and 1 / 1
    dc = DeviceColumns(c)
    for layout in ("arrays", "packed", "host"):
        h = cov.CoverageHistogram(c["contigs"], c["z"])
        try:
            push(nat, ctx, h, c, dc, layout)
            with pytest.raises(nat.TdtError) as err:
                h.finish(0)
            assert err.value.code == cc.TDT_E_INEXACT, layout
        finally:
            ctx.sync()
            h.close()


# ================================================================================================== H: call-to-call state
@pytest.mark.parametrize("mode0", [False, True])
def test_call_to_call_state_on_one_histogram(nat, ctx, cov, mode0):
    """push, push, finish (twice: the same bins, the same kept count); reset, then another layout; a refused push, reset, a clean result"""
    first = cc.get("h_state_a")
    with cov_mode("0" if mode0 else None):
        h = cov.CoverageHistogram(first["contigs"], first["z"])
    dcs = {}
    try:
        for step, (what, arg, layout) in enumerate(cc.state_sequence()):
            if what == "push":
                c = cc.get(arg)
                dcs.setdefault(arg, DeviceColumns(c))
                push(nat, ctx, h, c, dcs[arg], layout)
            elif what == "reset":
                h.reset()
                assert h.kept() == 0 and not h.finish(0).any(), step
            elif what == "finish_error":
                with pytest.raises(nat.TdtError) as err:
                    h.finish(0)
                assert err.value.code == arg, step
            else:
                refs = [wanted(cc.get(n)) for n in arg]
                nb = h.nbins(0)[0]
                want = sum(cc.dense(r[0][0], nb) for r in refs)          # exact: every bin is a sum of multiples of 2^-30 far below 2^53
                got = h.finish(0)
                bad = np.flatnonzero(got != want)
                assert not len(bad), (step, int(bad[0]), got[bad[0]], want[bad[0]], len(bad))
                assert h.kept() == sum(r[1] for r in refs), step
    finally:
        ctx.sync()
        h.close()


def test_cov_mode_is_read_when_the_histogram_is_created(nat, ctx, cov):
    """The flavour is fixed by tdt_cov_create: a histogram created under TIDDIT_COV_MODE=0 keeps writing the run-merged flavour's binned
    records (tdt_cov_record.h: bases_last_bin:10 | bases_first_bin:10 | 0000) after the variable is gone, and one created without it
    keeps the small-bin layout (bins_after_first:8 | bases_last_bin:8 | bases_first_bin:8) after the variable is set."""
    import torch
    z, s, e = 50, 120, 160                                         # bins 2 and 3: 30 bases in the first, 9 (one short) in the last
    c = cc.make_case("two_bin_read", "H", z, [("c", 10_000)], [cc._cols([s], [e])])
    c["claim"] = cc.model(c, "binned")
    dc = DeviceColumns(c)
    want = {True: (30 << 4) | (9 << 14), False: 30 | (9 << 8) | (1 << 16)}
    for mode0 in (True, False):
        with cov_mode("0" if mode0 else None):
            h = cov.CoverageHistogram(c["contigs"], z)
        with cov_mode(None if mode0 else "0"):
            try:
                push(nat, ctx, h, c, dc, "binned")
                ctx.sync()
                rec = int(dc.keep[4][0].item()) & 0xffffffffffffffff
                assert rec & 0xffffffff == (2 << 2) | 1 and (rec >> 32) & 0xffffff == want[mode0], (mode0, hex(rec))
                assert first_bad(h.finish(0), cc.reference(c)[0][0]) is None and h.kept() == 1
            finally:
                h.close()
