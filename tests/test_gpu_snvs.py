"""`TIDDIT_SNVS` on the GPU: the kernels (csrc/tdt_snv.hip, the shared finish of csrc/tdt_keystore.h) on every aimed case of
tests/snv_cases.py through both entries — ``tdt_snv_push`` on host columns, and ``tdt_snv_push_device`` on the same columns and record
bytes placed in device memory behind the pointer table the ingest fills — against the case's claim: the store read out by
``tdt_snv_keys`` equals the claimed keys as a multiset, and for every minimum support the case states ``tdt_snv_finish`` equals the
counter array and ``tdt_snv_rows`` the four row columns, exactly.  Then the store's growth and reset, the C-ABI refusals,
``tiddit_signal._scan`` on the file of tests/scan_all_cases.py at 64-KiB spans (alone, and beside the left-normalising indel counter
that shares the reference), and the switch end to end on that file, every job a fresh child process under its own time limit (the first
job that fails ends the fixture: nothing more is started behind a crash, a time-out or a GPU error).

Every test of this file fails on the parent commit: the module, the symbols and the switch do not exist there."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_all_cases as C
import snv_cases as D

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPPED = ("TIDDIT_VARIANTS", "TIDDIT_GENOTYPE", "TIDDIT_GENOTYPE_DEPTH", "TIDDIT_DEPTH_DIST", "TIDDIT_FORCE_DIST", "TIDDIT_COV_TRACK", "TIDDIT_CNV",
            "TIDDIT_ALLELES", "TIDDIT_ALLELES_MIN_BQ", "TIDDIT_ASCN", "TIDDIT_QC", "TIDDIT_DUPS", "TIDDIT_INDELS", "TIDDIT_INDELS_NORM", "TIDDIT_SNVS",
            "TIDDIT_HOST_INGEST", "TIDDIT_DIST_BACKEND", "TIDDIT_INGEST_CHUNK", "TIDDIT_NO_CARRY", "WORLD_SIZE", "RANK", "LOCAL_RANK")
PAIRS = []                       # the (case, entry) pairs that ran and passed
COL_INDEX = {"tid": 0, "pos": 1, "mapq": 3, "flag": 4, "rec_off": 11, "raw": 13}          # TDT_COL_* of include/tiddit_hip.h


# ---- the kernels --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference():
    """the cases' reference, resident: every contig of D.LOADED packed from FASTA bytes, contig 9 left unloaded"""
    from tiddit_amd import refseq
    ref = refseq.RefSeq(D.LENGTHS)
    for t in D.LOADED:
        text = D.TEXT[t]
        raw = "".join(text[o:o + 60] + "\n" for o in range(0, len(text), 60)).encode()
        ref.load_fasta(t, np.frombuffer(raw, dtype=np.uint8), len(text), 60, 61)
    for t in D.LOADED:
        assert np.array_equal(ref.fetch(t), refseq.codes_of_bases(D.TEXT[t]))
    yield ref
    ref.close()


def _counter(reference, case=None, capacity=None, Q=20, B=20):
    from tiddit_amd import tiddit_snvs
    return tiddit_snvs.SnvCounter(len(D.LENGTHS), reference, case["Q"] if case else Q, case["B"] if case else B,
                                  capacity=capacity or (case and case["capacity"]) or 1 << 12, ctx=reference.ctx)


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
        assert [x.dtype for x in r] == [np.uint64, np.uint64, np.uint32, np.uint32]
        for name, x, y in zip(("K1", "K2", "SUPPORT", "REV"), r, columns):
            assert x.shape == y.shape and np.array_equal(x, y), (what, S, name, x[:8].tolist(), y[:8].tolist())


@pytest.fixture(scope="module")
def wanted():
    """every case's claim, checked against the definition once"""
    out = {}
    for c in D.CASES:
        claim = D.expected(c)
        assert D.same(claim, D.definition(c)), c["name"]
        out[c["name"]] = claim
    return out


@pytest.mark.parametrize("entry", ["push", "push_device"])
@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_both_entries_equal_the_claim(case, entry, wanted, reference):
    h = _counter(reference, case)
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
    assert len(D.CASES) == D.N_CASES == 26
    assert len(set(PAIRS)) == 2 * 26, len(set(PAIRS))


def _case(start):
    return next(c for c in D.CASES if c["name"].startswith(start))


def test_a_store_made_for_64_keys_grows_more_than_once_and_gives_the_same(wanted, reference):
    case = _case("store:")
    h, big = _counter(reference, case), _counter(reference, capacity=1 << 14)
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


def test_state_accumulates_between_pushes_resets_and_keeps_handles_apart(wanted, reference):
    case, other = _case("sets: one site"), _case("phase: read lengths")
    first, second, third = D.batches(case)
    h, g = _counter(reference), _counter(reference, capacity=64)
    try:
        assert not h.finish(1).any() and len(h.keys()[0]) == 0 and len(h.rows()[0]) == 0
        h.push_host_batch(first)
        g.push_host_batch(D.batches(other)[0])
        part = h.finish(1)
        assert part[D.SN.index("records")] == len(first) and 0 < part[D.SN.index("distinct_events")] <= 2
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


def test_refused_arguments_leave_the_outputs_untouched(reference):
    from tiddit_amd import _native
    case = _case("sets: one site")
    ctx = reference.ctx
    lib, P = ctx.lib, _native.ptr
    assert lib.tdt_snv_sn_size() == D.SIZE
    h = ctypes.c_void_p(0x5a5a)
    n = len(D.LENGTHS)
    assert lib.tdt_snv_create(None, n, 20, 20, 64, reference.handle, ctypes.byref(h)) == -1 and h.value == 0x5a5a
    assert lib.tdt_snv_create(ctx.handle, n, 20, 20, 64, None, ctypes.byref(h)) == -1                   # no reference
    assert lib.tdt_snv_create(ctx.handle, n, 20, 20, 64, reference.handle, None) == -1 and lib.tdt_snv_create(ctx.handle, -1, 20, 20, 64, reference.handle, ctypes.byref(h)) == -1
    for args in (((1 << 24) + 1, 20, 20), (n, -1, 20), (n, 256, 20), (n, 20, -1), (n, 20, 94)):
        assert lib.tdt_snv_create(ctx.handle, *args, 64, reference.handle, ctypes.byref(h)) == -3, args
    assert h.value == 0x5a5a
    assert lib.tdt_snv_create(ctx.handle, n, 20, 20, 0, reference.handle, ctypes.byref(h)) == 0          # (no store yet)
    try:
        b = D.batches(case)[1]
        cols = [getattr(b, k) for k in D.COLUMNS]
        nb = len(b)

        def push(hh, c, nn, raw, raw_len):
            return lib.tdt_snv_push(hh, *[P(x) if x is not None else None for x in c], nn, P(raw) if raw is not None else None, raw_len)
        assert push(None, cols, nb, b.raw, len(b.raw)) == -1
        for k in range(5):
            assert push(h, cols[:k] + [None] + cols[k + 1:], nb, b.raw, len(b.raw)) == -1
        assert push(h, cols, nb, None, len(b.raw)) == -1
        assert push(h, cols, 1 << 31, b.raw, len(b.raw)) == -1
        assert push(h, cols[:4] + [np.ascontiguousarray(b.rec_off[::-1])], nb, b.raw, len(b.raw)) == -1           # offsets that decrease
        assert lib.tdt_snv_push_device(None, None, 0, 0) == -1 and lib.tdt_snv_push_device(h, None, 5, 100) == -1
        nulls = (ctypes.c_void_p * 14)()
        assert lib.tdt_snv_push_device(h, nulls, 5, 100) == -1 and lib.tdt_snv_push_device(h, nulls, 1 << 31, 100) == -1
        out = np.full(D.SIZE, 7, dtype=np.uint64)
        nr = ctypes.c_size_t(77)
        assert lib.tdt_snv_finish(None, 1, P(out), ctypes.byref(nr)) == -1 and lib.tdt_snv_finish(h, 1, None, ctypes.byref(nr)) == -1
        assert lib.tdt_snv_finish(h, 1, P(out), None) == -1
        assert lib.tdt_snv_finish(h, 0, P(out), ctypes.byref(nr)) == -3 and lib.tdt_snv_finish(h, 10 ** 6 + 1, P(out), ctypes.byref(nr)) == -3
        assert (out == 7).all() and nr.value == 77
        ms = np.full(4, 7.0)
        assert lib.tdt_snv_timing(None, P(ms)) == -1 and lib.tdt_snv_timing(h, None) == -1 and (ms == 7).all()
        st = np.full(3, 7, dtype=np.uint64)
        assert lib.tdt_snv_reserve_stats(None, P(st)) == -1 and lib.tdt_snv_reserve_stats(h, None) == -1 and (st == 7).all()
        assert lib.tdt_snv_reset(None) == -1
        cnt = ctypes.c_size_t(77)
        k1, k2 = np.full(16, 7, dtype=np.uint64), np.full(16, 7, dtype=np.uint64)
        sup, rev = np.full(16, 7, dtype=np.uint32), np.full(16, 7, dtype=np.uint32)
        assert lib.tdt_snv_keys(None, P(k1), P(k2), ctypes.byref(cnt)) == -1 and lib.tdt_snv_keys(h, P(k1), P(k2), None) == -1
        assert lib.tdt_snv_keys(h, P(k1), None, ctypes.byref(cnt)) == -1 and cnt.value == 77
        assert lib.tdt_snv_rows(None, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -1 and lib.tdt_snv_rows(h, P(k1), P(k2), P(sup), P(rev), None) == -1
        assert lib.tdt_snv_rows(h, P(k1), P(k2), None, P(rev), ctypes.byref(cnt)) == -1
        assert lib.tdt_snv_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -1 and cnt.value == 77            # no finish yet
        # nothing refused above stored anything; n = 0 is a no-op; and the handle still works
        assert push(h, [None] * 5, 0, None, 0) == 0 and lib.tdt_snv_push_device(h, None, 0, 0) == 0
        assert lib.tdt_snv_finish(h, 1, P(out), ctypes.byref(nr)) == 0 and not out.any() and nr.value == 0
        assert lib.tdt_snv_keys(h, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 0
        assert push(h, cols, nb, b.raw, len(b.raw)) == 0                                         # five reads, one event each, three sets (1 + 3 + 1)
        cnt = ctypes.c_size_t(16)
        assert lib.tdt_snv_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -1 and cnt.value == 16            # a push since the finish
        assert lib.tdt_snv_finish(h, 1, P(out), ctypes.byref(nr)) == 0 and nr.value == 3
        assert out[D.SN.index("mismatches")] == 5 and out[D.SN.index("distinct_events")] == 3 and out[D.SN.index("aligned_bases")] == 100
        cnt = ctypes.c_size_t(4)                                                                 # room for 4 of the 5 keys: refused, nothing written
        assert lib.tdt_snv_keys(h, P(k1), P(k2), ctypes.byref(cnt)) == -3 and cnt.value == 4 and (k1 == 7).all() and (k2 == 7).all()
        cnt = ctypes.c_size_t(2)                                                                 # room for 2 of the 3 rows: the same
        assert lib.tdt_snv_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == -3 and cnt.value == 2
        assert (k1 == 7).all() and (k2 == 7).all() and (sup == 7).all() and (rev == 7).all()
        cnt = ctypes.c_size_t(0)
        assert lib.tdt_snv_rows(h, None, None, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 3                    # the count alone
        cnt = ctypes.c_size_t(16)
        assert lib.tdt_snv_rows(h, P(k1), P(k2), P(sup), P(rev), ctypes.byref(cnt)) == 0 and cnt.value == 3 and (k1[3:] == 7).all() and (rev[3:] == 7).all()
        assert sorted(sup[:3].tolist()) == [1, 1, 3]
        cnt = ctypes.c_size_t(16)
        assert lib.tdt_snv_keys(h, P(k1), P(k2), ctypes.byref(cnt)) == 0 and cnt.value == 5 and (k1[5:] == 7).all()
        # a raw_len of 0: every eligible read is malformed, nothing is read; the column counters still count
        assert lib.tdt_snv_reset(h) == 0 and push(h, cols, nb, None, 0) == 0
        assert lib.tdt_snv_finish(h, 1, P(out), ctypes.byref(nr)) == 0 and nr.value == 0
        assert np.array_equal(out, D.counters_of({"records": 5, "eligible": 5, "malformed": 5}, 0, 0))
    finally:
        assert lib.tdt_snv_destroy(h) == 0 and lib.tdt_snv_destroy(None) == 0


# ---- the scan -----------------------------------------------------------------------------------------------------------------
Q, B = 20, 20
SUPPORTS = (1, 2, 3)


class Made:
    pass


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """the file of scan_all_cases, the definition over the host reader's batches, and the resident reference"""
    from tiddit_amd import fasta, refseq, tiddit_snvs
    m = Made()
    m.dir = str(tmp_path_factory.mktemp("snv_scan"))
    m.info = C.generate(m.dir)
    m.bam, m.fa, m.vcf = C.paths(m.dir)
    table = C.contigs()
    m.names, m.lengths = [n for n, _ in table], [l for _, l in table]
    m.batches = C.host_batches(m.bam)
    m.keys, m.sn = [], {}
    host = C.host_reference()
    for b in m.batches:
        tiddit_snvs.keys_of_batch_by_read(b, m.keys, m.sn, host, Q, B)
    m.by_support = {}
    for s in SUPPORTS:
        counts, rows = tiddit_snvs.summarise(m.keys, m.sn, s)
        m.by_support[s] = (counts, D.row_columns(rows))
    m.reference = refseq.load_for_bam(fasta.FastaFile(m.fa), m.names, m.lengths)[0]
    yield m
    m.reference.close()


def _scan(m, indels):
    """``tiddit_signal._scan`` on the module's file at 64-KiB spans with the SNV counter attached (and, ``indels``, the left-normalising
    indel counter on the same reference) -> (store rows, {S: (counts, rows)}, reserve stats, indel results or None)"""
    from tiddit_amd import bamio, tiddit_signal as S
    tables = None
    try:
        S.SNVS, S.SNV_REFERENCE = (2, Q, B), m.reference
        if indels:
            S.INDELS, S.INDEL_REFERENCE = (2, C.INDEL_Q), m.reference
        header, chromosomes, cov, data, splits, clips, tables = S._scan(m.bam, C.MIN_Q, C.MAX_INS, C.MIN_CONTIG, C.MIN_ANCHOR, C.MIN_CLIP, 50)
        h = S.SNV_COUNTER
        assert h is not None and h.reference is m.reference
        k1, k2 = h.keys()
        by_support = {}
        for s in SUPPORTS:
            counts = h.finish(s)
            by_support[s] = (counts, h.rows())
        res = [D.key_rows(list(zip(k1.tolist(), k2.tolist()))), by_support, h.reserve_stats(), None]
        g = S.INDEL_COUNTER
        assert (g is not None) == indels
        if g is not None:
            assert g.reference is m.reference
            i1, i2 = g.keys()
            res[3] = (C.key_rows(list(zip(i1.tolist(), i2.tolist()))), {s: (g.finish(s), list(g.rows())) for s in C.INDEL_SUPPORTS},
                      tuple(int(v) for v in g.norm_stats()))
        return res
    finally:
        S.SNVS = S.SNV_REFERENCE = S.INDELS = S.INDEL_REFERENCE = None
        for name in ("SNV_COUNTER", "INDEL_COUNTER"):
            if getattr(S, name) is not None:
                getattr(S, name).close()
            setattr(S, name, None)
        if tables is not None:
            tables.close()
        bamio.set_carry(None)


def _equals_the_definition(m, got):
    rows, by_support = got[0], got[1]
    assert np.array_equal(rows, D.key_rows(m.keys))
    for s in SUPPORTS:
        assert np.array_equal(by_support[s][0], m.by_support[s][0]), (s, by_support[s][0].tolist(), m.by_support[s][0].tolist())
        assert all(np.array_equal(x, y) for x, y in zip(by_support[s][1], m.by_support[s][1])), s
    assert m.sn["records"] == m.info["n_records"] and len(m.keys) > 1000 and len(m.by_support[2][1][0]) > 100


@pytest.mark.parametrize("host_ingest", [False, True], ids=["device", "host_ingest"])
def test_the_scan_alone_equals_the_definition(made, monkeypatch, host_ingest):
    monkeypatch.setenv("TIDDIT_INGEST_CHUNK", str(1 << 16))
    if host_ingest:
        monkeypatch.setenv("TIDDIT_HOST_INGEST", "1")
    else:
        monkeypatch.delenv("TIDDIT_HOST_INGEST", raising=False)
    _equals_the_definition(made, _scan(made, indels=False))


def test_the_scan_beside_the_indel_counter_shares_the_reference_and_changes_neither(made, monkeypatch):
    monkeypatch.setenv("TIDDIT_INGEST_CHUNK", str(1 << 16))
    monkeypatch.delenv("TIDDIT_HOST_INGEST", raising=False)
    got = _scan(made, indels=True)
    _equals_the_definition(made, got)
    from tiddit_amd import tiddit_indels
    ikeys, isn, host = [], {}, C.host_reference()
    for b in made.batches:                                                    # (the indel definition, as scan_all_cases.combine takes it)
        ikeys.extend(tiddit_indels.keys_of_batch(b, isn, C.INDEL_Q, host))
    E = (C.key_rows(ikeys), C._indel_summary(ikeys, isn), tuple(isn.get(k, 0) for k in tiddit_indels.NORM_SN))
    keys, by_support, norm = got[3]
    assert np.array_equal(keys, E[0]) and norm == E[2] and norm[0] > 0
    for s in C.INDEL_SUPPORTS:
        assert np.array_equal(by_support[s][0], E[1][s][0]) and all(np.array_equal(x, y) for x, y in zip(by_support[s][1], E[1][s][1])), s


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------
def _job(m, out, timeout=600, **env):
    e = {k: v for k, v in os.environ.items() if k not in STRIPPED}
    e.update(env)
    argv = [sys.executable, "-m", "tiddit_amd", "--sv", "--bam", m.bam, "--ref", m.fa, "-o", out, "--skip_assembly", "-s", "20000"]
    return subprocess.run(argv, cwd=REPO, env=e, capture_output=True, text=True, timeout=timeout)


def _ok(r):
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r


def _content(path):
    """a file's bytes; of a VCF: without its ``##TIDDITcmd=`` line, which names the job's own prefix"""
    data = open(path, "rb").read()
    if path.endswith(".vcf"):
        return b"\n".join(l for l in data.split(b"\n") if not l.startswith(b"##TIDDITcmd="))
    return data


def _files(prefix):
    d, base = os.path.split(prefix)
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            rel = os.path.relpath(os.path.join(root, f), d)
            if rel.startswith(base + ".") or rel.startswith(base + "_tiddit"):
                out[rel[len(base):]] = _content(os.path.join(root, f))
    return out


@pytest.fixture(scope="module")
def jobs(made):
    """(each job is checked before the next one is started: a crash, a time-out or a GPU error ends the fixture there)"""
    paths = {n: os.path.join(made.dir, n) for n in ("off", "on", "host", "fed", "bad", "nofa", "ranks")}
    _ok(_job(made, paths["off"]))
    r = _ok(_job(made, paths["on"], TIDDIT_SNVS="2"))
    _ok(_job(made, paths["host"], TIDDIT_SNVS="2", TIDDIT_HOST_INGEST="1"))
    _ok(_job(made, paths["fed"], TIDDIT_ALLELES=paths["on"] + ".snvs.tab"))
    return paths, r


def test_the_file_equals_the_definitions_file_byte_for_byte(made, jobs, tmp_path):
    import oracle
    from tiddit_amd import tiddit_snvs
    paths, r = jobs
    cols = {k: np.concatenate([np.array(getattr(b, k)) for b in made.batches]) for k in ("tid", "pos", "end", "mapq", "flag")}
    cover = {}
    for t, (name, L) in enumerate(zip(made.names, made.lengths)):
        if L >= C.MIN_CONTIG:
            msk = cols["tid"] == t
            cover[name] = oracle.coverage_stream(cols["pos"][msk], cols["end"][msk], cols["mapq"][msk], cols["flag"][msk], L, 50, 5)[0]
    counts, columns = made.by_support[2]
    want = str(tmp_path / "want.snvs.tab")
    tiddit_snvs.write_file(want, counts, columns, made.names, cover, 2, 20, 20)
    got = open(paths["on"] + ".snvs.tab", "rb").read()
    assert len(got) > 2000 and got == open(want, "rb").read()
    assert got.startswith(b"# tiddit_amd snvs v1 min_support=2 min_mapq=20 min_bq=20\nSN\trecords\t%d\n" % made.info["n_records"])
    assert [l for l in r.stdout.split("\n") if l.startswith("snvs:")] == [tiddit_snvs.summary_line(counts)]
    assert open(paths["host"] + ".snvs.tab", "rb").read() == got


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    paths, r = jobs
    off, on, host = (_files(paths[k]) for k in ("off", "on", "host"))
    assert set(on) - set(off) == {".snvs.tab"} and set(off) <= set(on) and len(off) >= 5
    assert all(on[k] == off[k] for k in off), [k for k in off if on[k] != off[k]]
    assert not os.path.exists(paths["off"] + ".snvs.tab") and ".snvs.tab" in host


def test_the_written_file_fed_back_as_allele_sites_gives_one_line_per_row(jobs):
    paths, r = jobs
    rows = [l for l in open(paths["on"] + ".snvs.tab").read().split("\n") if l and not l.startswith(("#", "SN\t"))]
    lines = [l for l in open(paths["fed"] + ".alleles.tab").read().split("\n") if l and not l.startswith("#")]
    assert len(rows) == len(lines) > 100
    assert [l.split("\t")[:2] + l.split("\t")[3:5] for l in rows] == [l.split("\t")[:4] for l in lines]


@pytest.mark.parametrize("value,text", [("2:300", "the minimum MAPQ is 0 ... 255"), ("0", "the minimum support is 1 ... 10^6"),
                                        ("2:20:94", "the minimum base quality is 0 ... 93"),
                                        ("yes", "the switch is 1, S, S:Q or S:Q:B (minimum support 1 ... 10^6, minimum MAPQ 0 ... 255, minimum base quality 0 ... 93)")])
def test_a_malformed_value_of_the_switch_is_an_error(made, jobs, value, text):
    paths, r = jobs
    bad = _job(made, paths["bad"], timeout=120, TIDDIT_SNVS=value)
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == ["error, TIDDIT_SNVS=%s: %s" % (value, text)]
    assert not os.path.exists(paths["bad"] + "_tiddit") and not os.path.exists(paths["bad"] + ".snvs.tab")


def test_a_fasta_without_a_contig_of_the_header_is_an_error(made, jobs):
    paths, r = jobs
    text = open(made.fa).read()
    cut = text.rindex(">")
    fa = paths["nofa"] + ".fa"
    open(fa, "w").write(text[:cut])
    m = Made()
    m.bam, m.fa = made.bam, fa
    res = _job(m, paths["nofa"], timeout=120, TIDDIT_SNVS="2")
    assert res.returncode == 1, (res.returncode, res.stdout[-1000:], res.stderr[-2000:])
    errors = [l for l in res.stdout.split("\n") if l.startswith("error")]
    assert errors == ["error, TIDDIT_SNVS=2: contig %s has %d bases in the BAM header and is missing in the reference FASTA" % (made.names[-1], made.lengths[-1])]
    assert not os.path.exists(paths["nofa"] + "_tiddit") and not os.path.exists(paths["nofa"] + ".snvs.tab")


def test_n_ranks_refuse_the_switch_and_write_nothing(made, jobs):
    """every rank ends with the refusal before the first collective (no process group is ever made) and no file is written"""
    paths, r = jobs
    res = _job(made, paths["ranks"], timeout=120, TIDDIT_SNVS="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29547",
               TIDDIT_DIST_BACKEND="gloo", TIDDIT_FORCE_DIST="1")
    assert res.returncode == 1, (res.returncode, res.stdout[-1000:], res.stderr[-2000:])
    errors = [l for l in res.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_SNVS is a one-process switch")
    assert not os.path.exists(paths["ranks"] + "_tiddit") and not os.path.exists(paths["ranks"] + ".snvs.tab")
