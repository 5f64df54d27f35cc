"""`TIDDIT_CLIPS` on the GPU: the kernels (csrc/tdt_clip.hip, the shared finish of csrc/tdt_keystore.h) on every aimed case of
tests/clip_cases.py through both entries — ``tdt_clip_push`` on host columns, and ``tdt_clip_push_device`` on the same columns and
record bytes placed in device memory behind the pointer table the ingest fills — against the definition (which
tests/test_clip_refs_cpu.py pins to the cases' claims): the store read out by ``tdt_clip_keys`` equals the definition's keys as a
multiset, and for every minimum support the case states ``tdt_clip_finish`` equals the counter array and ``tdt_clip_rows`` the nine row
columns, exactly.  Then structure cases for the site launches (sizes read from the ``#define`` lines of the sources), the store's growth
and reset, the C-ABI refusals, ``tiddit_signal._scan`` on the file of tests/scan_all_cases.py at 64-KiB spans (alone, and beside the
indel and SNV counters), and the switch end to end on the sv_e2e_small fixture, every job a fresh child process under its own time limit
(the first job that fails ends the fixture: nothing more is started behind a crash, a time-out or a GPU error).

Every test of this file fails on the parent commit: the module, the symbols and the switch do not exist there."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import clip_cases as D
import scan_all_cases as C
from sv_e2e_common import load_fixture, materialise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPPED = ("TIDDIT_VARIANTS", "TIDDIT_GENOTYPE", "TIDDIT_GENOTYPE_DEPTH", "TIDDIT_DEPTH_DIST", "TIDDIT_FORCE_DIST", "TIDDIT_COV_TRACK", "TIDDIT_CNV",
            "TIDDIT_ALLELES", "TIDDIT_ALLELES_MIN_BQ", "TIDDIT_ASCN", "TIDDIT_QC", "TIDDIT_DUPS", "TIDDIT_INDELS", "TIDDIT_INDELS_NORM", "TIDDIT_SNVS",
            "TIDDIT_CLIPS", "TIDDIT_HOST_INGEST", "TIDDIT_DIST_BACKEND", "TIDDIT_INGEST_CHUNK", "TIDDIT_NO_CARRY", "WORLD_SIZE", "RANK", "LOCAL_RANK")
PAIRS = []                       # the (case, entry) pairs that ran and passed
COL_INDEX = {"tid": 0, "pos": 1, "mapq": 3, "flag": 4, "rec_off": 11, "raw": 13}          # TDT_COL_* of include/tiddit_hip.h
N_CONTIGS = 1 << 24
ROW_NAMES = ("K1", "SIDE", "SUPPORT", "REV", "SEQS", "CLEN", "CONSENSUS", "AGREE", "TOTAL")


def _define(path, name):
    text = open(os.path.join(REPO, "tiddit_amd", "csrc", path)).read()
    return int(re.search(r"^#define %s (\d+)\b" % name, text, re.M).group(1))


KS_TILE, KS_BLOCK = _define("tdt_keystore.h", "KS_TILE"), _define("tdt_keystore.h", "KS_BLOCK")
VOTE_BLOCK, K_TILE = _define("tdt_clip.hip", "CLIP_VOTE_BLOCK"), _define("tdt_clip.hip", "CLIP_K_TILE")


# ---- the kernels --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from tiddit_amd import _native
    return _native.default_context()


def _counter(ctx, case=None, capacity=None, Q=20, L=10):
    from tiddit_amd import tiddit_clips
    return tiddit_clips.ClipCounter(N_CONTIGS, case["Q"] if case else Q, case["L"] if case else L, capacity=capacity or (case and case["capacity"]) or 1 << 12,
                                    ctx=ctx)


class DeviceColumns:
    """a batch's columns and record bytes in device memory, exactly raw_len bytes of them, behind the pointer table of the ingest"""

    def __init__(self, b):
        import torch
        as_bytes = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()         # (any dtype: the bytes as they are)
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


def _same(h, want, what):
    rows, by_support = want
    k1, k2 = h.keys()
    assert k1.dtype == k2.dtype == np.uint64 and len(k1) == len(k2)
    got = D.key_rows(list(zip(k1.tolist(), k2.tolist())))
    assert got.shape == rows.shape and np.array_equal(got, rows), (what, got.shape, rows.shape)
    for S, (counts, columns) in by_support.items():
        c = h.finish(S)
        assert c.dtype == np.uint64 and c.shape == (D.SIZE,)
        assert np.array_equal(c, counts), (what, S, c.tolist(), counts.tolist())
        r = h.rows()
        assert [x.dtype for x in r] == list(D.ROW_DTYPES)
        for name, x, y in zip(ROW_NAMES, r, columns):
            assert x.shape == y.shape and np.array_equal(x, y), (what, S, name, x[:8].tolist(), y[:8].tolist())


@pytest.fixture(scope="module")
def wanted():
    """every case's definition, once, checked against the case's claim"""
    out = {}
    for c in D.CASES:
        out[c["name"]] = D.definition(c)
        assert D.agrees_with_claim(c, out[c["name"]]) is None, c["name"]
    return out


@pytest.mark.parametrize("entry", ["push", "push_device"])
@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_both_entries_equal_the_definition(case, entry, wanted, ctx):
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


def test_the_stated_count_of_case_entry_pairs_ran():
    assert len(D.CASES) == D.N_CASES == 35
    assert len(set(PAIRS)) == 2 * 35, len(set(PAIRS))


# ---- structure cases for the site launches: keys made by pushes of tiny records --------------------------------------------------
def _word(j, n):
    """the j-th word of n letters over A C G T"""
    return "".join("ACGT"[(j >> (2 * k)) & 3] for k in range(n))


def _site(pos, words, rev_every=3):
    """one trailing-clip site at pos + 4: a read of 4 matched bases per clip in ``words``"""
    return [D.rd(pos=pos, m=4, trail=w, flag=D.REV if k % rev_every == 0 else 0) for k, w in enumerate(words)]


def _structure(name):
    six = [_word(j, 6) for j in range(4 ** 6)]
    if name == "sizes":                        # sites of 1, 63, 64, 65 and 4^6 + 1 distinct sequences: below, at and above a wave's stride, and across a row tile
        reads = []
        for k, n in enumerate((1, VOTE_BLOCK - 1, VOTE_BLOCK, VOTE_BLOCK + 1)):
            reads += _site(100 + 10 * k, six[:n]) + _site(100 + 10 * k, six[:n:2])           # (every other sequence twice: counts of 1 and 2)
        reads += _site(500, six + ["ACGTACG"])
        assert 4 ** 6 + 1 == KS_TILE + 1
        return reads
    if name == "heads":                        # rows: a site of KS_TILE - 1 rows, a site of 1 row (the LAST position of tile 0), a head on the FIRST of tile 1
        return _site(100, six[:KS_TILE - 1]) + _site(200, ["GATTACA"]) * 3 + _site(300, ["CCCCCCC", "CCCCCCA"]) + _site(400, six[:5])
    if name == "singles":                      # KS_TILE + 1 sites of one row each
        return [D.rd(pos=100 + k, m=4, trail=six[k % 4096], flag=D.REV if k % 2 else 0) for k in range(KS_TILE + 1)] + _site(100, [six[0]])
    if name == "one":                          # one site holding all rows, more than a tile of them
        return _site(100, [_word(j, 7) for j in range(KS_TILE + KS_BLOCK + 3)]) + _site(100, six[:100])
    raise KeyError(name)


@pytest.mark.parametrize("name", ["sizes", "heads", "singles", "one"])
def test_structure_cases_equal_the_definition(name, ctx):
    reads = _structure(name)
    case = {"name": name, "batches": [(reads[:K_TILE + 1], 0), (reads[K_TILE + 1:], 0)], "Q": 20, "L": 6, "S": (1, 2, 3), "capacity": 1 << 14}
    want = D.definition(case)
    rows = want[1][1][1]
    if name == "sizes":
        assert sorted(rows[4].tolist()) == [1, VOTE_BLOCK - 1, VOTE_BLOCK, VOTE_BLOCK + 1, KS_TILE + 1]
    if name == "heads":
        assert rows[4].tolist() == [KS_TILE - 1, 1, 2, 5]                              # (so the heads are rows 0, KS_TILE - 1, KS_TILE and KS_TILE + 2)
    if name == "singles":
        assert len(rows[0]) == KS_TILE + 1 and (rows[4] == 1).all() and rows[2][0] == 2
    if name == "one":
        assert len(rows[0]) == 1 and rows[4][0] == KS_TILE + KS_BLOCK + 3 + 100
    h = _counter(ctx, case)
    try:
        for b in D.batches(case):
            h.push_host_batch(b)
        _same(h, want, name)
    finally:
        h.close()


def _case(start):
    return next(c for c in D.CASES if c["name"].startswith(start))


def test_a_store_made_for_64_keys_grows_more_than_once_and_gives_the_same(wanted, ctx):
    case = _case("store:")
    h, big = _counter(ctx, case), _counter(ctx, capacity=1 << 14)
    try:
        for b in D.batches(case):
            h.push_host_batch(b)
            big.push_host_batch(b)
        asks, grows, cap = h.reserve_stats()
        assert grows >= 2 and asks >= grows and cap > 64, (asks, grows, cap)
        assert big.reserve_stats() == (0, 0, 1 << 14)
        _same(h, wanted[case["name"]], "grown")
        _same(big, wanted[case["name"]], "never grown")
    finally:
        h.close()
        big.close()


def test_state_accumulates_between_pushes_resets_and_keeps_handles_apart(wanted, ctx):
    case, other = _case("store:"), _case("vote: a tie of 2 against 2")
    first, second, third = D.batches(case)
    h, g = _counter(ctx), _counter(ctx, capacity=64)
    try:
        assert not h.finish(1).any() and len(h.keys()[0]) == 0 and len(h.rows()[0]) == 0
        h.push_host_batch(first)
        g.push_host_batch(D.batches(other)[0])
        part = h.finish(1)
        assert part[D.SN.index("records")] == len(first) and 0 < part[D.SN.index("distinct_sites")] < wanted[case["name"]][1][1][0][D.SN.index("distinct_sites")]
        h.push_host_batch(second)
        h.push_host_batch(third)
        _same(h, wanted[case["name"]], "all pushes")
        _same(h, wanted[case["name"]], "every finish again")                  # (the store is left as it was)
        _same(g, wanted[other["name"]], "the other handle")
        h.reset()
        assert not h.finish(2).any() and len(h.keys()[0]) == 0 and len(h.rows()[0]) == 0
        for b in (third, first, second):
            h.push_host_batch(b)
        _same(h, wanted[case["name"]], "after the reset, in another order")
        _same(g, wanted[other["name"]], "the other handle after the reset")
    finally:
        h.close()
        g.close()


def test_refused_arguments_leave_the_outputs_untouched(ctx):
    from tiddit_amd import _native
    case = _case("support: a site with SUPPORT = S - 1")
    lib, P = ctx.lib, _native.ptr
    assert lib.tdt_clip_sn_size() == D.SIZE
    h = ctypes.c_void_p(0x5a5a)
    n = 8
    assert lib.tdt_clip_create(None, n, 20, 10, 64, ctypes.byref(h)) == -1 and h.value == 0x5a5a
    assert lib.tdt_clip_create(ctx.handle, n, 20, 10, 64, None) == -1 and lib.tdt_clip_create(ctx.handle, -1, 20, 10, 64, ctypes.byref(h)) == -1
    for args in (((1 << 24) + 1, 20, 10), (n, -1, 10), (n, 256, 10), (n, 20, 0), (n, 20, 65536)):
        assert lib.tdt_clip_create(ctx.handle, *args, 64, ctypes.byref(h)) == -3, args
    assert h.value == 0x5a5a
    assert lib.tdt_clip_create(ctx.handle, n, 20, 10, 0, ctypes.byref(h)) == 0          # (no store yet)
    try:
        b = D.batches(case)[0]
        cols = [getattr(b, k) for k in D.COLUMNS]
        nb = len(b)

        def push(hh, c, nn, raw, raw_len):
            return lib.tdt_clip_push(hh, *[P(x) if x is not None else None for x in c], nn, P(raw) if raw is not None else None, raw_len)
        assert push(None, cols, nb, b.raw, len(b.raw)) == -1
        for k in range(5):
            assert push(h, cols[:k] + [None] + cols[k + 1:], nb, b.raw, len(b.raw)) == -1
        assert push(h, cols, nb, None, len(b.raw)) == -1
        assert push(h, cols, 1 << 31, b.raw, len(b.raw)) == -1
        assert push(h, cols[:4] + [np.ascontiguousarray(b.rec_off[::-1])], nb, b.raw, len(b.raw)) == -1           # offsets that decrease
        assert lib.tdt_clip_push_device(None, None, 0, 0) == -1 and lib.tdt_clip_push_device(h, None, 5, 100) == -1
        nulls = (ctypes.c_void_p * 14)()
        assert lib.tdt_clip_push_device(h, nulls, 5, 100) == -1 and lib.tdt_clip_push_device(h, nulls, 1 << 31, 100) == -1
        out = np.full(D.SIZE, 7, dtype=np.uint64)
        nr = ctypes.c_size_t(77)
        assert lib.tdt_clip_finish(None, 1, P(out), ctypes.byref(nr)) == -1 and lib.tdt_clip_finish(h, 1, None, ctypes.byref(nr)) == -1
        assert lib.tdt_clip_finish(h, 1, P(out), None) == -1
        assert lib.tdt_clip_finish(h, 0, P(out), ctypes.byref(nr)) == -3 and lib.tdt_clip_finish(h, 10 ** 6 + 1, P(out), ctypes.byref(nr)) == -3
        assert (out == 7).all() and nr.value == 77
        ms = np.full(5, 7.0)
        assert lib.tdt_clip_timing(None, P(ms)) == -1 and lib.tdt_clip_timing(h, None) == -1 and (ms == 7).all()
        st = np.full(3, 7, dtype=np.uint64)
        assert lib.tdt_clip_reserve_stats(None, P(st)) == -1 and lib.tdt_clip_reserve_stats(h, None) == -1 and (st == 7).all()
        assert lib.tdt_clip_reset(None) == -1
        cnt = ctypes.c_size_t(77)
        k1, k2 = np.full(16, 7, dtype=np.uint64), np.full(16, 7, dtype=np.uint64)
        R = [np.full(16, 7, dtype=dt) for dt in D.ROW_DTYPES]
        rows = lambda hh, arrays, c: lib.tdt_clip_rows(hh, *[P(a) if a is not None else None for a in arrays], c)
        assert lib.tdt_clip_keys(None, P(k1), P(k2), ctypes.byref(cnt)) == -1 and lib.tdt_clip_keys(h, P(k1), P(k2), None) == -1
        assert lib.tdt_clip_keys(h, P(k1), None, ctypes.byref(cnt)) == -1 and cnt.value == 77
        assert rows(None, R, ctypes.byref(cnt)) == -1 and rows(h, R, None) == -1
        for k in range(9):
            assert rows(h, R[:k] + [None] + R[k + 1:], ctypes.byref(cnt)) == -1
        assert rows(h, R, ctypes.byref(cnt)) == -1 and cnt.value == 77                            # no finish yet
        # nothing refused above stored anything; n = 0 is a no-op; and the handle still works
        assert push(h, [None] * 5, 0, None, 0) == 0 and lib.tdt_clip_push_device(h, None, 0, 0) == 0
        assert lib.tdt_clip_finish(h, 1, P(out), ctypes.byref(nr)) == 0 and not out.any() and nr.value == 0
        assert lib.tdt_clip_keys(h, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 0
        assert push(h, cols, nb, b.raw, len(b.raw)) == 0                                         # five reads, one clip each, two sites (2 + 3)
        cnt = ctypes.c_size_t(16)
        assert rows(h, R, ctypes.byref(cnt)) == -1 and cnt.value == 16                            # a push since the finish
        assert lib.tdt_clip_finish(h, 1, P(out), ctypes.byref(nr)) == 0 and nr.value == 2
        assert out[D.SN.index("right_clips")] == 5 and out[D.SN.index("distinct_sequences")] == 2 and out[D.SN.index("distinct_sites")] == 2
        cnt = ctypes.c_size_t(4)                                                                 # room for 4 of the 5 keys: refused, nothing written
        assert lib.tdt_clip_keys(h, P(k1), P(k2), ctypes.byref(cnt)) == -3 and cnt.value == 4 and (k1 == 7).all() and (k2 == 7).all()
        cnt = ctypes.c_size_t(1)                                                                 # room for 1 of the 2 rows: the same
        assert rows(h, R, ctypes.byref(cnt)) == -3 and cnt.value == 1 and all((a == 7).all() for a in R)
        cnt = ctypes.c_size_t(0)
        assert rows(h, [None] * 9, ctypes.byref(cnt)) == 0 and cnt.value == 2                     # the count alone
        cnt = ctypes.c_size_t(16)
        assert rows(h, R, ctypes.byref(cnt)) == 0 and cnt.value == 2 and all((a[2:] == 7).all() for a in R)
        assert R[2][:2].tolist() == [2, 3] and R[1][:2].tolist() == [1, 1] and R[5][:2].tolist() == [12, 12]
        cnt = ctypes.c_size_t(16)
        assert lib.tdt_clip_keys(h, P(k1), P(k2), ctypes.byref(cnt)) == 0 and cnt.value == 5 and (k1[5:] == 7).all()
        assert lib.tdt_clip_finish(h, 3, P(out), ctypes.byref(nr)) == 0 and nr.value == 1 and out[D.SN.index("reported_sites")] == 1
        # a raw_len of 0: every eligible read is malformed, nothing is read; the column counters still count
        assert lib.tdt_clip_reset(h) == 0 and push(h, cols, nb, None, 0) == 0
        assert lib.tdt_clip_finish(h, 1, P(out), ctypes.byref(nr)) == 0 and nr.value == 0
        assert np.array_equal(out, D.push_counters({"records": 5, "eligible": 5, "malformed": 5}))
    finally:
        assert lib.tdt_clip_destroy(h) == 0 and lib.tdt_clip_destroy(None) == 0


# ---- the scan -----------------------------------------------------------------------------------------------------------------
Q, L = 20, 10
SUPPORTS = (1, 2, 3)


class Made:
    pass


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """the file of scan_all_cases and the definition over the host reader's batches"""
    from tiddit_amd import tiddit_clips
    m = Made()
    m.dir = str(tmp_path_factory.mktemp("clip_scan"))
    m.info = C.generate(m.dir)
    m.bam, m.fa, m.vcf = C.paths(m.dir)
    table = C.contigs()
    m.names, m.lengths = [n for n, _ in table], [l for _, l in table]
    m.batches = C.host_batches(m.bam)
    m.keys, m.sn = [], {}
    for b in m.batches:
        tiddit_clips.keys_of_batch_by_read(b, m.keys, m.sn, Q, L)
    m.by_support = {}
    for s in SUPPORTS:
        counts, rows = tiddit_clips.summarise(m.keys, m.sn, s)
        m.by_support[s] = (counts, D.row_columns(rows))
    return m


def _scan(m, others=False):
    """``tiddit_signal._scan`` on the module's file at 64-KiB spans with the clip counter attached (``others``: beside the left-normalising
    indel counter and the SNV counter on one resident reference) -> (store rows, {S: (counts, rows)}, indel results, snv results)"""
    from tiddit_amd import bamio, fasta, refseq, tiddit_signal as S
    tables = reference = None
    try:
        S.CLIPS = (2, Q, L)
        if others:
            reference = refseq.load_for_bam(fasta.FastaFile(m.fa), m.names, m.lengths)[0]
            S.INDELS, S.INDEL_REFERENCE = (2, C.INDEL_Q), reference
            S.SNVS, S.SNV_REFERENCE = (2, 20, 20), reference
        header, chromosomes, cov, data, splits, clips, tables = S._scan(m.bam, C.MIN_Q, C.MAX_INS, C.MIN_CONTIG, C.MIN_ANCHOR, C.MIN_CLIP, 50)
        h = S.CLIP_COUNTER
        assert h is not None
        k1, k2 = h.keys()
        by_support = {}
        for s in SUPPORTS:
            counts = h.finish(s)
            by_support[s] = (counts, h.rows())
        res = [D.key_rows(list(zip(k1.tolist(), k2.tolist()))), by_support, None, None]
        g, v = S.INDEL_COUNTER, S.SNV_COUNTER
        assert (g is not None) == others and (v is not None) == others
        if others:
            i1, i2 = g.keys()
            res[2] = (C.key_rows(list(zip(i1.tolist(), i2.tolist()))), {s: (g.finish(s), list(g.rows())) for s in C.INDEL_SUPPORTS},
                      tuple(int(x) for x in g.norm_stats()))
            v1, v2 = v.keys()
            res[3] = (C.key_rows(list(zip(v1.tolist(), v2.tolist()))), {s: (v.finish(s), list(v.rows())) for s in SUPPORTS})
        return res
    finally:
        S.CLIPS = S.SNVS = S.SNV_REFERENCE = S.INDELS = S.INDEL_REFERENCE = None
        for name in ("CLIP_COUNTER", "SNV_COUNTER", "INDEL_COUNTER"):
            if getattr(S, name) is not None:
                getattr(S, name).close()
            setattr(S, name, None)
        if tables is not None:
            tables.close()
        if reference is not None:
            reference.close()
        bamio.set_carry(None)


def _equals_the_definition(m, got):
    rows, by_support = got[0], got[1]
    assert np.array_equal(rows, D.key_rows(m.keys))
    for s in SUPPORTS:
        assert np.array_equal(by_support[s][0], m.by_support[s][0]), (s, by_support[s][0].tolist(), m.by_support[s][0].tolist())
        assert all(np.array_equal(x, y) for x, y in zip(by_support[s][1], m.by_support[s][1])), s
    assert m.sn["records"] == m.info["n_records"] and len(m.keys) >= m.info["clip_reads"] + m.info["split_reads"] > 20
    assert len(m.by_support[1][1][0]) > 20


@pytest.mark.parametrize("host_ingest", [False, True], ids=["device", "host_ingest"])
def test_the_scan_alone_equals_the_definition(made, monkeypatch, host_ingest):
    monkeypatch.setenv("TIDDIT_INGEST_CHUNK", str(1 << 16))
    if host_ingest:
        monkeypatch.setenv("TIDDIT_HOST_INGEST", "1")
    else:
        monkeypatch.delenv("TIDDIT_HOST_INGEST", raising=False)
    _equals_the_definition(made, _scan(made))


def test_the_scan_beside_the_indel_and_snv_counters_changes_none_of_the_three(made, monkeypatch):
    monkeypatch.setenv("TIDDIT_INGEST_CHUNK", str(1 << 16))
    monkeypatch.delenv("TIDDIT_HOST_INGEST", raising=False)
    got = _scan(made, others=True)
    _equals_the_definition(made, got)
    from tiddit_amd import tiddit_indels, tiddit_snvs
    host = C.host_reference()
    ikeys, isn, skeys, ssn = [], {}, [], {}
    for b in made.batches:                                                    # (the two definitions, as scan_all_cases.combine takes them)
        ikeys.extend(tiddit_indels.keys_of_batch(b, isn, C.INDEL_Q, host))
        tiddit_snvs.keys_of_batch_by_read(b, skeys, ssn, host, 20, 20)
    keys, by_support, norm = got[2]
    E = (C.key_rows(ikeys), C._indel_summary(ikeys, isn), tuple(isn.get(k, 0) for k in tiddit_indels.NORM_SN))
    assert np.array_equal(keys, E[0]) and norm == E[2] and norm[0] > 0
    for s in C.INDEL_SUPPORTS:
        assert np.array_equal(by_support[s][0], E[1][s][0]) and all(np.array_equal(x, y) for x, y in zip(by_support[s][1], E[1][s][1])), s
    keys, by_support = got[3]
    assert np.array_equal(keys, C.key_rows(skeys)) and len(skeys) > 1000
    for s in SUPPORTS:
        counts, rows = tiddit_snvs.summarise(skeys, ssn, s)
        assert np.array_equal(by_support[s][0], counts), s
        want = [np.array([r[k] for r in rows], dtype=dt) for k, dt in enumerate((np.uint64, np.uint64, np.uint32, np.uint32))]
        assert all(np.array_equal(x, y) for x, y in zip(by_support[s][1], want)), s


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------
def _job(bam, fa, out, fx, timeout=600, **env):
    e = {k: v for k, v in os.environ.items() if k not in STRIPPED}
    e.update(env)
    argv = [sys.executable, "-m", "tiddit_amd", "--sv", "--bam", bam, "--ref", fa, "-o", out, "--skip_assembly", "-s", str(fx["params"]["n_reads_stats"])]
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
def jobs(golden_dir, tmp_path_factory):
    """(each job is checked before the next one is started: a crash, a time-out or a GPU error ends the fixture there)"""
    fx = load_fixture(golden_dir, "sv_e2e_small.json")
    d = str(tmp_path_factory.mktemp("clips"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    paths = {n: os.path.join(d, n) for n in ("off", "on", "host", "ranks", "bad")}
    _ok(_job(bam, fa, paths["off"], fx))
    r = _ok(_job(bam, fa, paths["on"], fx, TIDDIT_CLIPS="2:20:12"))
    _ok(_job(bam, fa, paths["host"], fx, TIDDIT_CLIPS="2:20:12", TIDDIT_HOST_INGEST="1"))
    return fx, bam, fa, d, paths, r


def test_the_file_equals_the_definitions_file_byte_for_byte(jobs, tmp_path):
    import oracle
    from tiddit_amd import bamio, tiddit_clips
    fx, bam, fa, d, paths, r = jobs
    sn, keys = {}, []
    cols = {k: [] for k in ("tid", "pos", "end", "mapq", "flag")}
    rd = bamio.BamReader(bam)
    names, lengths = list(rd.references), list(rd.lengths)
    for b in rd.batches():
        tiddit_clips.keys_of_batch_by_read(b, keys, sn, 20, 12)
        for k in cols:
            cols[k].append(np.array(getattr(b, k)))
    rd.close()
    cols = {k: np.concatenate(v) for k, v in cols.items()}
    cover = {}
    for t in sorted({k1 >> 32 for k1, _ in keys}):                             # (the scan's filter: -q 5, the default)
        m = cols["tid"] == t
        cover[names[t]] = oracle.coverage_stream(cols["pos"][m], cols["end"][m], cols["mapq"][m], cols["flag"][m], lengths[t], 50, 5)[0]
    counts, rows = tiddit_clips.summarise(keys, sn, 2)
    v = lambda k: int(counts[D.SN.index(k)])
    assert v("records") == fx["n_records"] and v("malformed") == 0 and v("left_clips") > 0 and v("right_clips") > 0 and len(rows) == v("reported_sites") > 0
    want = str(tmp_path / "want.clips.tab")
    tiddit_clips.write_file(want, counts, rows, names, cover, 2, 20, 12)
    got = open(paths["on"] + ".clips.tab", "rb").read()
    assert got == open(want, "rb").read()
    assert got.startswith(b"# tiddit_amd clips v1 min_support=2 min_mapq=20 min_clip=12 cols=28\nSN\trecords\t%d\n" % fx["n_records"])
    assert [l for l in r.stdout.split("\n") if l.startswith("clips:")] == [tiddit_clips.summary_line(counts)]
    assert open(paths["host"] + ".clips.tab", "rb").read() == got


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    fx, bam, fa, d, paths, r = jobs
    off, on, host = (_files(paths[k]) for k in ("off", "on", "host"))
    assert set(on) - set(off) == {".clips.tab"} and set(off) <= set(on) and len(off) >= 5
    assert all(on[k] == off[k] for k in off), [k for k in off if on[k] != off[k]]
    assert not os.path.exists(paths["off"] + ".clips.tab") and ".clips.tab" in host


@pytest.mark.parametrize("value,text", [("2:300", "the minimum MAPQ is 0 ... 255"), ("0", "the minimum support is 1 ... 10^6"),
                                        ("2:20:0", "the minimum clip length is 1 ... 65535"),
                                        ("yes", "the switch is 1, S, S:Q or S:Q:L (minimum support 1 ... 10^6, minimum MAPQ 0 ... 255, minimum clip length 1 ... 65535)")])
def test_a_malformed_value_of_the_switch_is_an_error(jobs, value, text):
    fx, bam, fa, d, paths, r = jobs
    bad = _job(bam, fa, paths["bad"], fx, timeout=120, TIDDIT_CLIPS=value)
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == ["error, TIDDIT_CLIPS=%s: %s" % (value, text)]
    assert not os.path.exists(paths["bad"] + "_tiddit") and not os.path.exists(paths["bad"] + ".clips.tab")


def test_n_ranks_refuse_the_switch_and_write_nothing(jobs):
    """every rank ends with the refusal before the first collective (no process group is ever made) and no file is written"""
    fx, bam, fa, d, paths, r = jobs
    res = _job(bam, fa, paths["ranks"], fx, timeout=120, TIDDIT_CLIPS="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29551",
               TIDDIT_DIST_BACKEND="gloo", TIDDIT_FORCE_DIST="1")
    assert res.returncode == 1, (res.returncode, res.stdout[-1000:], res.stderr[-2000:])
    errors = [l for l in res.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_CLIPS is a one-process switch")
    assert not os.path.exists(paths["ranks"] + "_tiddit") and not os.path.exists(paths["ranks"] + ".clips.tab")
