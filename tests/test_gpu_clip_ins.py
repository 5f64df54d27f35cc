"""`TIDDIT_CLIPS_INS` on the GPU: clip_ext_keys (csrc/tdt_clip.hip) on every key and consensus case of tests/clip_ins_cases.py through
both push entries — the extension store read out by ``tdt_clip_ext_keys`` equals the definition's keys as a multiset, the first store is
what it is without the extension, and behind a finish ``tdt_clip_ins`` gives the definition's counters, ``tdt_clip_ext_rows`` its
extended consensus and ``tdt_clip_ins_rows`` its pairs, exactly; the pair launches (csrc/tdt_clip_ins.hip) on every pair and closure
case through ``tdt_clip_ins_sites`` and ``tdt_clip_ins_sites_device``; every insertion length from O to 268; a store that grows from room
for 64 keys; the C-ABI refusals with poisoned outputs; and the switch end to end on a generated reference of two contigs and 20 kb with
planted insertions of 60, 130, 250 and 600 bases, every job a fresh child process under its own time limit (the first job that fails
ends the fixture: nothing more is started behind a crash, a time-out or a GPU error).

Every test of this file fails on the parent commit: the module, the symbols and the switch do not exist there."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import clip_cases as D
import clip_ins_cases as X

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = []                       # the (case, entry) pairs that ran and passed
COL_INDEX = {"tid": 0, "pos": 1, "mapq": 3, "flag": 4, "rec_off": 11, "raw": 13}          # TDT_COL_* of include/tiddit_hip.h
N_CONTIGS = 1 << 24
PUSH_CASES = X.KEY_CASES + X.CONS_CASES
K, O, M = 20, 12, 1


@pytest.fixture(scope="module")
def ctx():
    from tiddit_amd import _native
    return _native.default_context()


def _counter(ctx, case, capacity=None, ext_capacity=None):
    from tiddit_amd import tiddit_clips
    h = tiddit_clips.ClipCounter(N_CONTIGS, case["Q"], case["L"], capacity=capacity or 1 << 12, ctx=ctx)
    h.enable_ext(ext_capacity if ext_capacity is not None else case["capacity"])
    return h


class DeviceColumns:
    """a batch's columns and record bytes in device memory, exactly raw_len bytes of them, behind the pointer table of the ingest"""

    def __init__(self, b):
        import torch
        as_bytes = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
        self._keep = {k: as_bytes(getattr(b, k)) for k in D.COLUMNS}
        self._keep["raw"] = as_bytes(b.raw) if len(b.raw) else torch.zeros(1, dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        self._n, self._raw_len = len(b), len(b.raw)
        table = [None] * 14
        for k, i in COL_INDEX.items():
            table[i] = self._keep[k].data_ptr()
        self._table = (ctypes.c_void_p * 14)(*table)

    def __len__(self):
        return self._n

    def pointer_table(self):
        return self._table


@pytest.fixture(scope="module")
def wanted():
    """every push case's definition, once: the extension keys, the first store's keys, and per minimum support the extended sites and
    the pairs; the key cases checked against their claims"""
    from tiddit_amd import tiddit_clip_ins as I
    out = {}
    for c in PUSH_CASES:
        rows, sn, events = X.key_definition(c)
        if c in X.KEY_CASES:
            assert X.key_agrees_with_claim(c, rows, sn) is None, c["name"]
        by_support = {}
        for S in (c["min_support"],) if "min_support" in c else (1, 3):
            by_support[S] = I.summarise(events, sn, S, K, O, M)
            if "sites" in c:
                assert by_support[S][1] == X.literal_sites(c), c["name"]
        out[c["name"]] = (rows, D.definition(c)[0], by_support)
    return out


def _same(h, want, what):
    from tiddit_amd import tiddit_clip_ins as I
    rows, base_rows, by_support = want
    k1, k2 = h.ext_keys()
    assert k1.dtype == k2.dtype == np.uint64 and len(k1) == len(k2)
    got = D.key_rows(list(zip(k1.tolist(), k2.tolist())))
    assert got.shape == rows.shape and np.array_equal(got, rows), (what, got.shape, rows.shape)
    b1, b2 = h.keys()
    assert np.array_equal(D.key_rows(list(zip(b1.tolist(), b2.tolist()))), base_rows), what           # (the first store is what it is without the second)
    for S, (counts, sites, pairs) in by_support.items():
        h.finish(S)
        r = h.rows()
        sn = h.ins(K, O, M)
        assert sn.dtype == np.uint64 and np.array_equal(sn, counts), (what, S, sn.tolist(), counts.tolist())
        eclen, cons5 = h.ext_rows()
        w = I.site_columns(sites)
        assert np.array_equal(r[0], w[0]) and np.array_equal(r[1], w[1]), (what, S)
        assert np.array_equal(eclen, w[2]), (what, S, eclen.tolist()[:8], w[2].tolist()[:8])
        assert np.array_equal(cons5, w[3]), (what, S)
        cols, seq10 = h.ins_rows()
        wc, ws = I.pair_columns(pairs)
        assert all(np.array_equal(x, y) for x, y in zip(cols, wc)) and np.array_equal(seq10, ws), (what, S)
        assert (h.ins_timing() >= 0).all()


@pytest.mark.parametrize("entry", ["push", "push_device"])
@pytest.mark.parametrize("case", PUSH_CASES, ids=[c["name"] for c in PUSH_CASES])
def test_both_push_entries_equal_the_definition(case, entry, wanted, ctx):
    h = _counter(ctx, case)
    keep = []
    try:
        for b in D.batches(case):
            if entry == "push":
                h.push_host_batch(b)
            else:
                keep.append(DeviceColumns(b))
                h.push_device_batch(keep[-1])
        _same(h, wanted[case["name"]], case["name"])
    finally:
        h.close()
    PAIRS.append((case["name"], entry))


def test_a_store_made_for_64_keys_grows_more_than_once_and_gives_the_same(wanted, ctx):
    case = next(c for c in X.KEY_CASES if "a store made for 64 keys" in c["name"])
    assert case["capacity"] == 64
    h, big = _counter(ctx, case), _counter(ctx, case, ext_capacity=1 << 14)
    try:
        for b in D.batches(case):
            h.push_host_batch(b)
            big.push_host_batch(b)
        _same(h, wanted[case["name"]], "grown")
        _same(big, wanted[case["name"]], "never grown")
        h.reset()
        assert len(h.ext_keys()[0]) == 0 and len(h.keys()[0]) == 0
        for b in D.batches(case)[::-1]:
            h.push_host_batch(b)
        _same(h, wanted[case["name"]], "after the reset, in another order")
    finally:
        h.close()
        big.close()


# ---- the pair launches on site columns --------------------------------------------------------------------------------------------------
def _sites_entry(ctx, case, device):
    from tiddit_amd import tiddit_clip_ins as I
    counts, rows = X.pair_definition(case)
    assert X.pair_agrees_with_claim(case, counts, rows) is None, case["name"]
    sn, cols, seq10 = I.ins_sites(*I.site_columns(X.sites_of(case)), case["K"], case["O"], case["M"], ctx=ctx, device=device)
    assert np.array_equal(sn, counts), (case["name"], sn.tolist(), counts.tolist())
    wc, ws = I.pair_columns(rows)
    for name, x, y in zip(("R", "L", "TSD", "STATUS", "LEN", "MISMATCH", "CLOSURES"), cols, wc):
        assert x.dtype == np.uint32 and np.array_equal(x, y), (case["name"], name, x.tolist()[:8], y.tolist()[:8])
    assert np.array_equal(seq10, ws), case["name"]


@pytest.mark.parametrize("entry", ["sites", "sites_device"])
@pytest.mark.parametrize("case", X.PAIR_CASES, ids=[c["name"] for c in X.PAIR_CASES])
def test_both_sites_entries_equal_the_definition(case, entry, ctx):
    _sites_entry(ctx, case, entry == "sites_device")
    PAIRS.append((case["name"], entry))


def test_the_stated_count_of_case_entry_pairs_ran():
    assert len(PUSH_CASES) == X.N_KEY_CASES + len(X.CONS_CASES) == 11 + 12 and X.N_PAIR_CASES == 33
    assert len(set(PAIRS)) == 2 * 23 + 2 * 33, len(set(PAIRS))


@pytest.mark.parametrize("entry", ["sites", "sites_device"])
def test_every_length_from_O_to_268_closes_on_the_device(entry, ctx):
    _sites_entry(ctx, X.every_length_case(), entry == "sites_device")


def test_more_rows_than_a_tile_and_no_rows(ctx):
    """4100 pairs of sites 100 bases apart: the R rows of the second tile get their offsets from the first tile's count, and the pair
    whose two rows straddle the tile boundary is found; and n = 0"""
    from tiddit_amd import tiddit_clip_ins as I
    ins = X.seeded(60, 4242)
    x, y = X.flanks(ins, 40, 40)
    n = 2050
    sites = [s for k in range(n) for s in ((0, 500 + 100 * k, X.R_SIDE, 3, x), (0, 501 + 100 * k, X.L_SIDE, 3, y))] + [(1, 7, X.L_SIDE, 3, y)]
    sites = [(0, 400, X.L_SIDE, 3, y)] + sites                      # (an odd row in front: the pair of rows 4095 / 4096 straddles the tiles)
    case = {"name": "tiles", "sites": sites, "K": 20, "O": 12, "M": 1, "rows": [(2 * k + 1, 2 * k + 2, 0, X.CLOSED, 60, 0, 1, ins) for k in range(n)]}
    _sites_entry(ctx, case, False)
    _sites_entry(ctx, case, True)
    empty = [np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((0, 5), dtype=np.uint64)]
    sn, cols, seq10 = I.ins_sites(*empty, ctx=ctx)
    assert not sn.any() and all(len(c) == 0 for c in cols) and seq10.shape == (0, 10)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_outputs_untouched(ctx):
    from tiddit_amd import _native, tiddit_clip_ins as I
    lib, P = ctx.lib, _native.ptr
    case = next(c for c in X.PAIR_CASES if c["name"].startswith("pairs: two L sites"))
    k1, side, eclen, cons5 = I.site_columns(X.sites_of(case))
    n = len(k1)
    sn = np.full(I.SIZE, 7, dtype=np.uint64)
    outs = [np.full(8, 7, dtype=np.uint32) for _ in range(7)] + [np.full(80, 7, dtype=np.uint64)]
    untouched = lambda: (sn == 7).all() and all((o == 7).all() for o in outs)

    def sites(c=ctx.handle, nn=n, cols=(k1, side, eclen, cons5), kom=(20, 12, 1), s=sn, o=outs, room=8):
        cnt = ctypes.c_size_t(room or 0)
        rc = lib.tdt_clip_ins_sites(c, nn, *[P(a) if a is not None else None for a in cols], *kom, P(s) if s is not None else None,
                                    *[P(a) if a is not None else None for a in o], ctypes.byref(cnt) if room is not None else None)
        return rc, cnt.value
    assert sites(c=None)[0] == -1 and sites(s=None)[0] == -1 and sites(room=None)[0] == -1 and sites(nn=1 << 30)[0] == -1
    for k in range(4):
        assert sites(cols=[None if j == k else a for j, a in enumerate((k1, side, eclen, cons5))])[0] == -1
    for k in range(8):
        assert sites(o=[None if j == k else a for j, a in enumerate(outs)])[0] == -1              # some but not all output arrays
    assert sites(cols=(k1[::-1].copy(), side, eclen, cons5))[0] == -1                              # host sites that do not ascend
    assert sites(cols=(np.repeat(k1[:1], n), np.zeros(n, dtype=np.uint32), eclen, cons5))[0] == -1  # ... or repeat
    for kom in ((9, 12, 1), (141, 12, 1), (20, 7, 1), (20, 141, 1), (20, 12, -1), (20, 12, 9)):
        assert sites(kom=kom)[0] == -3, kom
    assert sites(room=2) == (-3, 2)                                                               # room for 2 of the 3 pairs: nothing written
    assert untouched()
    rc, cnt = sites(o=[None] * 8, room=0)                                                         # the count alone
    assert rc == 0 and cnt == 3 and sn[I.SN_INDEX["pairs"]] == 3 and all((o == 7).all() for o in outs)
    rc, cnt = sites()
    assert rc == 0 and cnt == 3 and outs[0][:3].tolist() == [1, 2, 2] and (outs[0][3:] == 7).all() and (outs[7][30:] == 7).all()
    assert sn.tolist() == [0, 0, 0, 0, 4, 2, 2, 3, 2, 1, 0]
    # the device entry: null pointers and ranges (its arrays are never touched by a refused call: nothing is launched)
    dev = lambda *a: lib.tdt_clip_ins_sites_device(*a)
    cnt = ctypes.c_size_t(8)
    one = ctypes.c_void_p(256)
    assert dev(None, 1, one, one, one, one, 20, 12, 1, one, *[None] * 8, ctypes.byref(cnt)) == -1
    assert dev(ctx.handle, 1, None, one, one, one, 20, 12, 1, one, *[None] * 8, ctypes.byref(cnt)) == -1
    assert dev(ctx.handle, 1, one, one, one, one, 20, 12, 1, None, *[None] * 8, ctypes.byref(cnt)) == -1
    assert dev(ctx.handle, 1, one, one, one, one, 20, 12, 1, one, *[None] * 8, None) == -1
    assert dev(ctx.handle, 1, one, one, one, one, 20, 12, 1, one, one, *[None] * 7, ctypes.byref(cnt)) == -1
    assert dev(ctx.handle, 1, one, one, one, one, 20, 7, 1, one, *[None] * 8, ctypes.byref(cnt)) == -3 and cnt.value == 8
    # ---- the handle
    h = ctypes.c_void_p()
    assert lib.tdt_clip_create(ctx.handle, 8, 20, 10, 64, ctypes.byref(h)) == 0
    try:
        cnt = ctypes.c_size_t(77)
        x1, x2 = np.full(16, 7, dtype=np.uint64), np.full(16, 7, dtype=np.uint64)
        res, ms3 = np.full(I.SIZE, 7, dtype=np.uint64), np.zeros(3)
        assert lib.tdt_clip_ext_keys(h, P(x1), P(x2), ctypes.byref(cnt)) == -1                    # no tdt_clip_ext_enable
        c13, nr = np.zeros(13, dtype=np.uint64), ctypes.c_size_t()
        assert lib.tdt_clip_finish(h, 1, P(c13), ctypes.byref(nr)) == 0
        assert lib.tdt_clip_ins(h, 20, 12, 1, P(res)) == -1 and (res == 7).all()                  # the same
        assert lib.tdt_clip_ext_enable(None, 64) == -1 and lib.tdt_clip_ext_enable(h, 1 << 40) == -3
        assert lib.tdt_clip_ext_enable(h, 0) == 0 and lib.tdt_clip_ext_enable(h, 64) == -1         # twice
        assert lib.tdt_clip_reset(h) == 0
        assert lib.tdt_clip_ins(h, 20, 12, 1, P(res)) == -1 and (res == 7).all()                  # no finish since the reset
        b = D.build_batch([D.rd(pos=100, trail=X.seeded(60, 1))] * 3 + [D.rd(pos=300, lead=X.seeded(60, 2))] * 3)
        cols = [getattr(b, k) for k in D.COLUMNS]
        assert lib.tdt_clip_push(h, *[P(c) for c in cols], len(b), P(b.raw), len(b.raw)) == 0
        assert lib.tdt_clip_ins(h, 20, 12, 1, P(res)) == -1 and (res == 7).all()                  # a push since the finish
        e, c5 = np.full(4, 7, dtype=np.uint32), np.full(20, 7, dtype=np.uint64)
        assert lib.tdt_clip_ext_rows(h, P(e), P(c5), ctypes.byref(cnt)) == -1 and lib.tdt_clip_ins_timing(h, P(ms3)) == -1
        assert lib.tdt_clip_finish(h, 3, P(c13), ctypes.byref(nr)) == 0 and nr.value == 2
        assert lib.tdt_clip_ext_rows(h, P(e), P(c5), ctypes.byref(cnt)) == -1                      # a finish, but no tdt_clip_ins yet
        assert lib.tdt_clip_ins(None, 20, 12, 1, P(res)) == -1 and lib.tdt_clip_ins(h, 20, 12, 1, None) == -1
        for kom in ((9, 12, 1), (20, 141, 1), (20, 12, 9)):
            assert lib.tdt_clip_ins(h, *kom, P(res)) == -3
        assert (res == 7).all()
        assert lib.tdt_clip_ins(h, 20, 12, 1, P(res)) == 0
        assert res.tolist() == [3, 3, 12, 0, 2, 1, 1, 0, 0, 0, 0]                                  # an R site at 120 and an L site at 301: no pair
        cnt = ctypes.c_size_t(1)
        assert lib.tdt_clip_ext_rows(h, P(e), P(c5), ctypes.byref(cnt)) == -3 and cnt.value == 1 and (e == 7).all() and (c5 == 7).all()
        assert lib.tdt_clip_ext_rows(h, P(e), None, ctypes.byref(cnt)) == -1 and lib.tdt_clip_ext_rows(h, P(e), P(c5), None) == -1
        cnt = ctypes.c_size_t(0)
        assert lib.tdt_clip_ext_rows(h, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 2
        cnt = ctypes.c_size_t(4)
        assert lib.tdt_clip_ext_rows(h, P(e), P(c5), ctypes.byref(cnt)) == 0 and e.tolist() == [60, 60, 7, 7] and (c5[10:] == 7).all()
        cnt = ctypes.c_size_t(8)
        assert lib.tdt_clip_ins_rows(h, *[P(o) for o in outs[:3]], None, *[P(o) for o in outs[4:]], ctypes.byref(cnt)) == -1
        assert lib.tdt_clip_ins_rows(None, *[P(o) for o in outs], ctypes.byref(cnt)) == -1 and lib.tdt_clip_ins_rows(h, *[P(o) for o in outs], None) == -1
        assert lib.tdt_clip_ins_rows(h, *[None] * 8, ctypes.byref(cnt)) == 0 and cnt.value == 0
        assert lib.tdt_clip_ins_timing(h, None) == -1 and lib.tdt_clip_ins_timing(None, P(ms3)) == -1
        cnt = ctypes.c_size_t(2)                                                                 # room for 2 of the 12 extension keys
        assert lib.tdt_clip_ext_keys(h, P(x1), P(x2), ctypes.byref(cnt)) == -3 and cnt.value == 2 and (x1 == 7).all()
        assert lib.tdt_clip_ext_keys(h, P(x1), None, ctypes.byref(cnt)) == -1 and lib.tdt_clip_ext_keys(h, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 12
        assert lib.tdt_clip_finish(h, 3, P(c13), ctypes.byref(nr)) == 0
        assert lib.tdt_clip_ins_timing(h, P(ms3)) == -1                                   # a finish since the tdt_clip_ins
    finally:
        assert lib.tdt_clip_destroy(h) == 0


# ---- the switch, end to end -------------------------------------------------------------------------------------------------------------
ALIGN, FAR = "600", "20:2"


def _job(bam, fa, out, timeout=300, **env):
    e = {k: v for k, v in os.environ.items() if not (k.startswith("TIDDIT_") and k != "TIDDIT_HIP_LIB") and k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env)
    argv = [sys.executable, "-m", "tiddit_amd", "--sv", "--bam", bam, "--ref", fa, "-o", out, "--skip_assembly"]
    return subprocess.run(argv, cwd=REPO, env=e, capture_output=True, text=True, timeout=timeout)


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
                data = open(p, "rb").read()
                if p.endswith(".vcf"):                                        # (its ##TIDDITcmd= line names the job's own prefix)
                    data = b"\n".join(l for l in data.split(b"\n") if not l.startswith(b"##TIDDITcmd="))
                out[rel[len(base):]] = hashlib.sha256(data).hexdigest()
    return out


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """the generated reference as a FASTA, the sample's reads as a sorted BAM; the jobs, each checked before the next is started"""
    from tiddit_amd import bamio
    d = str(tmp_path_factory.mktemp("clip_ins"))
    g, ins = X.job_genome()
    contigs = [("chrA", g[0].text()), ("chrB", g[1].text())]
    fa, bam = os.path.join(d, "ref.fa"), os.path.join(d, "sample.bam")
    open(fa, "wb").write(b"".join(b">" + n.encode() + b"\n" + X.fasta_raw(t) + b"\n" for n, t in contigs))
    w = bamio.BamWriter(bam, [(n, len(t)) for n, t in contigs])
    w._buf += D.build_batch(X.job_reads(g, ins)).raw.tobytes()
    w.close()
    paths = {n: os.path.join(d, n) for n in ("clips", "ins", "host", "all", "others", "bad", "ranks")}
    _ok(_job(bam, fa, paths["clips"], TIDDIT_CLIPS=X.CLIPS))
    r = _ok(_job(bam, fa, paths["ins"], TIDDIT_CLIPS=X.CLIPS, TIDDIT_CLIPS_INS=X.INS))
    return bam, fa, contigs, ins, paths, r


def test_the_file_equals_the_definitions_file_and_holds_the_planted_rows(jobs, tmp_path):
    from tiddit_amd import bamio, tiddit_clip_ins as I
    bam, fa, contigs, ins, paths, r = jobs
    events, keys, sn = [], [], {}
    rd = bamio.BamReader(bam)
    for b in rd.batches():
        I.events_of_batch_by_read(b, events, keys, sn, X.JOB_Q, X.JOB_L)
    rd.close()
    want = str(tmp_path / "want.clips.ins.tab")
    counts = I.definition_file(want, events, sn, [n for n, _ in contigs], X.JOB_S, X.JOB_K, X.JOB_O, X.JOB_M)
    got = open(paths["ins"] + ".clips.ins.tab", "rb").read()
    assert got == open(want, "rb").read()
    assert got.startswith(b"# tiddit_amd clips_ins v1 cols=140 max_tsd=32 min_cols=20 min_overlap=12 max_mismatch=1\nSN\text_left_events\t49\n")
    table = [l.split("\t") for l in got.decode().split("\n") if l and not l.startswith(("#", "SN"))]
    # CHROM POS END TSD STATUS LEN SEQ, as the insertions were planted; the 600-base one OPEN with both flanks the planted ends
    assert [[x[0], x[1], x[2], x[3], x[8], x[9], x[12]] for x in table] == X.job_expected_rows(ins)
    assert table[-1][8] == "OPEN" and table[-1][13] == ins[-1][:140] and table[-1][14] == ins[-1][-140:]
    assert [l for l in r.stdout.split("\n") if l.startswith("clips ins:")] == [I.summary_line(counts)]


def test_every_other_output_is_what_it_is_with_the_clips_alone(jobs):
    bam, fa, contigs, ins, paths, r = jobs
    alone, with_ins = _files(paths["clips"]), _files(paths["ins"])
    assert set(with_ins) - set(alone) == {".clips.ins.tab"} and set(alone) <= set(with_ins) and ".clips.tab" in alone and len(alone) >= 5
    assert all(with_ins[k] == alone[k] for k in alone), [k for k in alone if with_ins[k] != alone[k]]


def test_the_host_ingest_runs_the_same_kernel(jobs):
    bam, fa, contigs, ins, paths, r = jobs
    _ok(_job(bam, fa, paths["host"], TIDDIT_CLIPS=X.CLIPS, TIDDIT_CLIPS_INS=X.INS, TIDDIT_HOST_INGEST="1"))
    assert open(paths["host"] + ".clips.ins.tab", "rb").read() == open(paths["ins"] + ".clips.ins.tab", "rb").read()


def test_beside_the_align_and_far_stages_all_three_files_are_what_each_is_alone(jobs):
    bam, fa, contigs, ins, paths, r = jobs
    _ok(_job(bam, fa, paths["others"], TIDDIT_CLIPS=X.CLIPS, TIDDIT_CLIPS_ALIGN=ALIGN, TIDDIT_CLIPS_FAR=FAR))
    _ok(_job(bam, fa, paths["all"], TIDDIT_CLIPS=X.CLIPS, TIDDIT_CLIPS_ALIGN=ALIGN, TIDDIT_CLIPS_FAR=FAR, TIDDIT_CLIPS_INS=X.INS))
    alone, others, every = _files(paths["ins"]), _files(paths["others"]), _files(paths["all"])
    assert set(every) == set(alone) | set(others) and {".clips.ins.tab", ".clips.far.tab", ".clips.align.tab"} <= set(every)
    assert all(every[k] == alone[k] for k in alone) and all(every[k] == others[k] for k in others)


@pytest.mark.parametrize("env,line", [
    ({"TIDDIT_CLIPS_INS": "1"}, "error, TIDDIT_CLIPS_INS=1: the switch pairs the sites of TIDDIT_CLIPS, which is not set"),
    ({"TIDDIT_CLIPS": X.CLIPS, "TIDDIT_CLIPS_INS": "9"}, "error, TIDDIT_CLIPS_INS=9: the minimum extended-consensus columns are 10 ... 140"),
    ({"TIDDIT_CLIPS": X.CLIPS, "TIDDIT_CLIPS_INS": "20:7"}, "error, TIDDIT_CLIPS_INS=20:7: the minimum overlap is 8 ... 140"),
    ({"TIDDIT_CLIPS": X.CLIPS, "TIDDIT_CLIPS_INS": "20:12:9"}, "error, TIDDIT_CLIPS_INS=20:12:9: the maximum mismatches are 0 ... 8"),
    ({"TIDDIT_CLIPS": X.CLIPS, "TIDDIT_CLIPS_INS": "yes"}, "error, TIDDIT_CLIPS_INS=yes: the switch is 1, K, K:O or K:O:M (minimum extended-consensus columns "
                                                          "10 ... 140, minimum overlap 8 ... 140, maximum mismatches 0 ... 8)")],
    ids=["without TIDDIT_CLIPS", "9", "20:7", "20:12:9", "yes"])
def test_the_switch_without_its_partner_and_bad_values_are_errors(jobs, env, line):
    bam, fa, contigs, ins, paths, r = jobs
    bad = _job(bam, fa, paths["bad"], timeout=120, **env)
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == [line]
    assert not os.path.exists(paths["bad"] + "_tiddit") and not any(os.path.exists(paths["bad"] + s) for s in (".clips.tab", ".clips.ins.tab"))


def test_n_ranks_refuse_the_switch_and_write_nothing(jobs):
    """every rank ends with the refusal of TIDDIT_CLIPS before the first collective and no file is written"""
    bam, fa, contigs, ins, paths, r = jobs
    res = _job(bam, fa, paths["ranks"], timeout=120, TIDDIT_CLIPS=X.CLIPS, TIDDIT_CLIPS_INS="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29553", TIDDIT_DIST_BACKEND="gloo", TIDDIT_FORCE_DIST="1")
    assert res.returncode == 1, (res.returncode, res.stdout[-1000:], res.stderr[-2000:])
    errors = [l for l in res.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_CLIPS is a one-process switch")
    assert not os.path.exists(paths["ranks"] + "_tiddit") and not os.path.exists(paths["ranks"] + ".clips.ins.tab")
