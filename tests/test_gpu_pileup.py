"""`TIDDIT_SMALL_VCF` on the GPU: the kernels (csrc/tdt_pileup.hip) on every aimed case of tests/pileup_cases.py through both entries —
``tdt_pile_push`` on host columns, and ``tdt_pile_push_device`` on the same columns and record bytes placed in device memory behind the
pointer table the ingest fills — against the case's claim: the full depth read-out of every contig and the seven counters, exactly.
``tdt_pile_genotype`` and ``tdt_pile_genotype_device`` against the rule's literal claims.  Then reset and reuse, the C-ABI refusals on
poisoned outputs, ``tiddit_signal._scan`` on the file of tests/scan_all_cases.py at 64-KiB spans beside the SNV and indel counters, and
the switch end to end on a generated reference of about 20 kb with planted variants, every job a fresh child process under its own time
limit (the first job that fails ends the fixture: nothing more is started behind a crash, a time-out or a GPU error).

Every test of this file fails on the parent commit: the modules, the symbols and the switch do not exist there."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import pileup_cases as D
import scan_all_cases as C

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPPED = ("TIDDIT_VARIANTS", "TIDDIT_GENOTYPE", "TIDDIT_GENOTYPE_DEPTH", "TIDDIT_DEPTH_DIST", "TIDDIT_FORCE_DIST", "TIDDIT_COV_TRACK", "TIDDIT_CNV",
            "TIDDIT_ALLELES", "TIDDIT_ALLELES_MIN_BQ", "TIDDIT_ASCN", "TIDDIT_QC", "TIDDIT_DUPS", "TIDDIT_INDELS", "TIDDIT_INDELS_NORM", "TIDDIT_SNVS",
            "TIDDIT_SMALL_VCF", "TIDDIT_CLIPS", "TIDDIT_STR", "TIDDIT_PHASE", "TIDDIT_HOST_INGEST", "TIDDIT_DIST_BACKEND", "TIDDIT_INGEST_CHUNK",
            "TIDDIT_NO_CARRY", "WORLD_SIZE", "RANK", "LOCAL_RANK")
PAIRS = []                       # the (case, entry) pairs that ran and passed
COL_INDEX = {"tid": 0, "pos": 1, "mapq": 3, "flag": 4, "rec_off": 11, "raw": 13}          # TDT_COL_* of include/tiddit_hip.h


# ---- the kernels --------------------------------------------------------------------------------------------------------------
class DeviceColumns:
    """a batch's columns and record bytes in device memory, exactly raw_len bytes of them, behind the pointer table of the ingest"""

    def __init__(self, b):
        import torch
        as_bytes = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()         # (any dtype: the bytes as they are)
        self._keep = {k: as_bytes(getattr(b, k)) if len(b) else torch.zeros(8, dtype=torch.uint8).cuda() for k in D.COLUMNS}
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
def ctx():
    from tiddit_amd import _native
    return _native.default_context()


def _handle(ctx, case=None, lengths=D.LENGTHS, Q=D.Q):
    from tiddit_amd import tiddit_pileup
    return tiddit_pileup.PileupDepth(case["lengths"] if case else lengths, case["Q"] if case else Q, ctx=ctx)


def _same(h, want, what, finished=False):
    depth, counts = want
    c = h.counters() if finished else h.finish()
    assert c.dtype == np.uint64 and c.shape == (D.SIZE,)
    assert np.array_equal(c, counts), (what, c.tolist(), counts.tolist())
    for t, d in enumerate(depth):
        got = h.depth(t)
        assert got.dtype == np.uint32 and got.shape == d.shape
        if not np.array_equal(got, d):
            at = int(np.flatnonzero(got != d)[0])
            raise AssertionError((what, "contig", t, "first difference at base", at, got[max(at - 3, 0):at + 4].tolist(), d[max(at - 3, 0):at + 4].tolist()))


@pytest.fixture(scope="module")
def wanted():
    """every case's claim, checked against the definition once"""
    out = {}
    for c in D.CASES:
        claim = D.expected(c)
        assert D.same(claim, D.definition(c)), c["name"]
        out[c["name"]] = claim
    return out


def _push(h, b, entry, keep):
    if entry == "push":
        h.push_host_batch(b)
    else:
        keep.append(DeviceColumns(b))
        h.push_device_batch(keep[-1])


@pytest.mark.parametrize("entry", ["push", "push_device"])
@pytest.mark.parametrize("case", D.CASES, ids=[c["name"] for c in D.CASES])
def test_both_entries_equal_the_claim(case, entry, wanted, ctx):
    h = _handle(ctx, case)
    keep = []
    try:
        for b in D.batches(case):
            _push(h, b, entry, keep)
        _same(h, wanted[case["name"]], case["name"])
    finally:
        h.close()
    PAIRS.append((case["name"], entry))


def test_the_stated_count_of_case_entry_pairs_ran():
    assert len(D.CASES) == D.N_CASES == 18
    assert len(set(PAIRS)) == 2 * 18, len(set(PAIRS))


def _case(start):
    return next(c for c in D.CASES if c["name"].startswith(start))


@pytest.mark.parametrize("entry", ["genotype", "genotype_device"])
def test_the_genotype_entries_equal_the_rule_on_every_rule_case(entry, ctx):
    import torch
    from tiddit_amd import _native, tiddit_small_vcf
    case, k1, sup, want = D.rule_case()
    assert all(tiddit_small_vcf.genotype(alt, dp0) == cols for _, alt, dp0, cols in D.RULE)
    h = _handle(ctx, case)
    try:
        for b in D.batches(case):
            h.push_host_batch(b)
        h.finish()
        if entry == "genotype":
            got = h.genotype((k1, sup))
            assert h.timing()[3] > 0
        else:
            d_k1, d_sup = torch.from_numpy(k1.view(np.int64)).cuda(), torch.from_numpy(sup.view(np.int32)).cuda()
            d_out = torch.full((len(k1), 8), 7, dtype=torch.int32).cuda()
            torch.cuda.synchronize()
            _native.check(ctx.lib.tdt_pile_genotype_device(h.handle, ctypes.c_void_p(d_k1.data_ptr()), ctypes.c_void_p(d_sup.data_ptr()), len(k1),
                                                           ctypes.c_void_p(d_out.data_ptr())))
            ctx.sync()
            got = d_out.cpu().numpy().view(np.uint32)
        assert got.dtype == np.uint32 and got.shape == want.shape
        assert np.array_equal(got, want), [(D.RULE[i][0] if i < len(D.RULE) else D.RULE_BEHIND_THE_END[0], got[i].tolist(), want[i].tolist())
                                           for i in np.flatnonzero((got != want).any(axis=1)).tolist()]
        # ... and the whole-table form of the rule over the definition's depth says the same
        depth = D.definition(case)[0]
        rows = [(int(a), 0, int(s), 0) for a, s in zip(k1.tolist(), sup.tolist())]
        assert np.array_equal(tiddit_small_vcf.genotype_rows(rows, depth, D.LENGTHS), want)
    finally:
        h.close()


def test_state_accumulates_between_pushes_resets_and_keeps_handles_apart(wanted, ctx):
    case, other = _case("batches: seven pushes"), _case("cigar:")
    bs = D.batches(case)
    h, g = _handle(ctx), _handle(ctx)
    try:
        assert not h.counters().any()
        h.push_host_batch(bs[0])
        g.push_host_batch(D.batches(other)[0])
        assert h.counters()[0] == len(bs[0])
        for b in bs[1:]:
            h.push_host_batch(b)
        _same(h, wanted[case["name"]], "all pushes")
        _same(h, wanted[case["name"]], "a second finish changes nothing")
        _same(g, wanted[other["name"]], "the other handle")
        h.reset()
        assert not h.counters().any()
        _same(h, ([np.zeros(n, dtype=np.uint32) for n in D.LENGTHS], np.zeros(D.SIZE, dtype=np.uint64)), "empty behind the reset")
        h.reset()
        keep = []
        for b in reversed(bs):
            _push(h, b, "push_device", keep)
        _same(h, wanted[case["name"]], "after the reset, in another order, through the other entry")
        _same(g, wanted[other["name"]], "the other handle after the reset", finished=True)
    finally:
        h.close()
        g.close()


def test_refused_arguments_leave_the_outputs_untouched(ctx):
    from tiddit_amd import _native
    lib, P = ctx.lib, _native.ptr
    assert lib.tdt_pile_sn_size() == D.SIZE
    lens = np.array(D.LENGTHS, dtype=np.int64)
    n = len(lens)
    h = ctypes.c_void_p(0x5a5a)
    assert lib.tdt_pile_create(None, n, P(lens), 20, ctypes.byref(h)) == -1 and lib.tdt_pile_create(ctx.handle, n, None, 20, ctypes.byref(h)) == -1
    assert lib.tdt_pile_create(ctx.handle, n, P(lens), 20, None) == -1 and lib.tdt_pile_create(ctx.handle, -1, P(lens), 20, ctypes.byref(h)) == -1
    assert lib.tdt_pile_create(ctx.handle, 1 << 24, P(lens), 20, ctypes.byref(h)) == -3                 # (refused before a length is read)
    assert lib.tdt_pile_create(ctx.handle, n, P(lens), -1, ctypes.byref(h)) == -3 and lib.tdt_pile_create(ctx.handle, n, P(lens), 256, ctypes.byref(h)) == -3
    for bad in (1 << 31, -1):
        assert lib.tdt_pile_create(ctx.handle, 2, P(np.array([5, bad], dtype=np.int64)), 20, ctypes.byref(h)) == -3, bad
    assert h.value == 0x5a5a
    assert lib.tdt_pile_create(ctx.handle, n, P(lens), 20, ctypes.byref(h)) == 0
    try:
        b = D.batches(_case("cigar:"))[0]
        cols = [getattr(b, k) for k in D.COLUMNS]
        nb = len(b)

        def push(hh, c, nn, raw, raw_len):
            return lib.tdt_pile_push(hh, *[P(x) if x is not None else None for x in c], nn, P(raw) if raw is not None else None, raw_len)
        assert push(None, cols, nb, b.raw, len(b.raw)) == -1
        for k in range(5):
            assert push(h, cols[:k] + [None] + cols[k + 1:], nb, b.raw, len(b.raw)) == -1
        assert push(h, cols, nb, None, len(b.raw)) == -1
        assert push(h, cols, 1 << 31, b.raw, len(b.raw)) == -1
        assert push(h, cols[:4] + [np.ascontiguousarray(b.rec_off[::-1])], nb, b.raw, len(b.raw)) == -1           # offsets that decrease
        assert lib.tdt_pile_push_device(None, None, 0, 0) == -1 and lib.tdt_pile_push_device(h, None, 5, 100) == -1
        nulls = (ctypes.c_void_p * 14)()
        assert lib.tdt_pile_push_device(h, nulls, 5, 100) == -1 and lib.tdt_pile_push_device(h, nulls, 1 << 31, 100) == -1
        out = np.full(D.SIZE, 7, dtype=np.uint64)
        assert lib.tdt_pile_counters(None, P(out)) == -1 and lib.tdt_pile_counters(h, None) == -1 and (out == 7).all()
        ms = np.full(4, 7.0)
        assert lib.tdt_pile_timing(None, P(ms)) == -1 and lib.tdt_pile_timing(h, None) == -1 and (ms == 7).all()
        assert lib.tdt_pile_reset(None) == -1 and lib.tdt_pile_finish(None) == -1
        # before the finish: no depth, no genotype
        d = np.full(16, 7, dtype=np.uint32)
        k1, sup, g8 = np.array([D.B << 32 | 101], dtype=np.uint64), np.array([3], dtype=np.uint32), np.full(8, 7, dtype=np.uint32)
        assert lib.tdt_pile_depth(h, D.B, 0, 16, P(d)) == -1 and (d == 7).all()
        assert lib.tdt_pile_genotype(h, P(k1), P(sup), 1, P(g8)) == -1 and lib.tdt_pile_genotype_device(h, P(k1), P(sup), 1, P(g8)) == -1 and (g8 == 7).all()
        # nothing refused above added anything; n = 0 is a no-op
        assert push(h, [None] * 5, 0, None, 0) == 0 and lib.tdt_pile_push_device(h, None, 0, 0) == 0
        assert lib.tdt_pile_counters(h, P(out)) == 0 and not out.any()
        assert push(h, cols, nb, b.raw, len(b.raw)) == 0 and lib.tdt_pile_finish(h) == 0
        # behind the finish: a push is refused until the reset; ranges outside the contig and null pointers are refused
        assert push(h, cols, nb, b.raw, len(b.raw)) == -1 and lib.tdt_pile_push_device(h, nulls, 5, 100) == -1
        assert lib.tdt_pile_counters(h, P(out)) == 0 and out[0] == nb
        L = D.LENGTHS[D.B]
        for tid, start, cnt in ((-1, 0, 1), (n, 0, 1), (D.B, -1, 1), (D.B, 0, -1), (D.B, L - 15, 17), (D.B, L + 1, 0), (3, 1, 1), (D.B, 0, 1 << 40)):
            assert lib.tdt_pile_depth(h, tid, start, cnt, P(d)) == -3, (tid, start, cnt)
        assert lib.tdt_pile_depth(None, D.B, 0, 16, P(d)) == -1 and lib.tdt_pile_depth(h, D.B, 0, 16, None) == -1 and (d == 7).all()
        assert lib.tdt_pile_depth(h, D.B, L, 0, P(d)) == 0 and lib.tdt_pile_depth(h, D.B, 0, 0, None) == 0 and (d == 7).all()
        assert lib.tdt_pile_depth(h, D.B, 100, 16, P(d)) == 0 and d.tolist() == [1] * 15 + [0]               # (5M5=5X at base 100)
        assert lib.tdt_pile_genotype(None, P(k1), P(sup), 1, P(g8)) == -1 and lib.tdt_pile_genotype(h, None, P(sup), 1, P(g8)) == -1
        assert lib.tdt_pile_genotype(h, P(k1), None, 1, P(g8)) == -1 and lib.tdt_pile_genotype(h, P(k1), P(sup), 1, None) == -1
        assert lib.tdt_pile_genotype(h, P(k1), P(sup), 1 << 31, P(g8)) == -1 and lib.tdt_pile_genotype_device(h, None, None, 1, None) == -1
        assert (g8 == 7).all()
        assert lib.tdt_pile_genotype(h, None, None, 0, None) == 0 and lib.tdt_pile_genotype_device(h, None, None, 0, None) == 0
        assert lib.tdt_pile_genotype(h, P(k1), P(sup), 1, P(g8)) == 0 and g8.tolist() == [1, 0, 60, 9, 0, 2, 9, 1]       # (SUPPORT 3 over a depth of 1)
        # a raw_len of 0: every eligible read is malformed, nothing is read; the column counters still count
        assert lib.tdt_pile_reset(h) == 0 and push(h, cols, nb, None, 0) == 0
        assert lib.tdt_pile_counters(h, P(out)) == 0 and out.tolist() == [nb, nb, nb, 0, 0, 0, 0]
    finally:
        assert lib.tdt_pile_destroy(h) == 0 and lib.tdt_pile_destroy(None) == 0


# ---- the scan -----------------------------------------------------------------------------------------------------------------
Q, B = 20, 20


class Made:
    pass


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """the file of scan_all_cases, the definitions over the host reader's batches, and the resident reference"""
    from tiddit_amd import fasta, refseq, tiddit_indels, tiddit_pileup, tiddit_snvs
    m = Made()
    m.dir = str(tmp_path_factory.mktemp("pile_scan"))
    m.info = C.generate(m.dir)
    m.bam, m.fa, m.vcf = C.paths(m.dir)
    table = C.contigs()
    m.names, m.lengths = [n for n, _ in table], [l for _, l in table]
    m.batches = C.host_batches(m.bam)
    host = C.host_reference()
    spans, sn, skeys, ssn, ikeys, isn = [], {}, [], {}, [], {}
    for b in m.batches:
        tiddit_pileup.spans_of_batch(b, spans, sn, m.lengths, Q)
        tiddit_snvs.keys_of_batch_by_read(b, skeys, ssn, host, Q, B)
        ikeys.extend(tiddit_indels.keys_of_batch(b, isn, Q))
    m.depth, m.counts = tiddit_pileup.depth_of(spans, m.lengths), tiddit_pileup.counters_of(sn)
    m.snv, m.indel = tiddit_snvs.summarise(skeys, ssn, 2), tiddit_indels.summarise(ikeys, isn, 2)
    m.reference = refseq.load_for_bam(fasta.FastaFile(m.fa), m.names, m.lengths)[0]
    yield m
    m.reference.close()


@pytest.mark.parametrize("host_ingest", [False, True], ids=["device", "host_ingest"])
def test_the_scan_beside_the_snv_and_indel_counters_equals_the_definitions(made, monkeypatch, host_ingest):
    from tiddit_amd import bamio, tiddit_signal as S
    monkeypatch.setenv("TIDDIT_INGEST_CHUNK", str(1 << 16))
    if host_ingest:
        monkeypatch.setenv("TIDDIT_HOST_INGEST", "1")
    else:
        monkeypatch.delenv("TIDDIT_HOST_INGEST", raising=False)
    m, tables = made, None
    try:
        S.SNVS, S.SNV_REFERENCE, S.INDELS = (2, Q, B, "depth"), m.reference, (2, Q)
        header, chromosomes, cov, data, splits, clips, tables = S._scan(m.bam, C.MIN_Q, C.MAX_INS, C.MIN_CONTIG, C.MIN_ANCHOR, C.MIN_CLIP, 50)
        h = S.SNV_COUNTER.depth
        assert h is not None and h.min_mapq == Q and S.INDEL_COUNTER.depth is None and "pileup spans (push)" in S.SCAN_SECONDS
        assert m.counts[0] == m.info["n_records"] and m.counts[D.SN.index("spans")] > 10000
        _same(h, (m.depth, m.counts), "the scan")
        for counter, (counts, rows) in ((S.SNV_COUNTER, m.snv), (S.INDEL_COUNTER, m.indel)):
            assert np.array_equal(counter.finish(2), counts)
            got = counter.rows()
            assert len(rows) >= 1 and [tuple(int(v) for v in r) for r in zip(*(c.tolist() for c in got))] == [tuple(r) for r in rows]
    finally:
        S.SNVS = S.SNV_REFERENCE = S.INDELS = None
        for name in ("SNV_COUNTER", "INDEL_COUNTER"):
            if getattr(S, name) is not None:
                if getattr(S, name).depth is not None:
                    getattr(S, name).depth.close()
                getattr(S, name).close()
            setattr(S, name, None)
        if tables is not None:
            tables.close()
        bamio.set_carry(None)


def test_the_indel_counter_alone_carries_the_depth_and_without_the_setting_the_scan_makes_no_handle(made, monkeypatch):
    from tiddit_amd import bamio, tiddit_signal as S
    monkeypatch.setenv("TIDDIT_INGEST_CHUNK", str(1 << 16))
    monkeypatch.delenv("TIDDIT_HOST_INGEST", raising=False)
    for setting in ((2, Q, "depth"), (2, Q)):
        tables = None
        try:
            S.INDELS = setting
            tables = S._scan(made.bam, C.MIN_Q, C.MAX_INS, C.MIN_CONTIG, C.MIN_ANCHOR, C.MIN_CLIP, 50)[6]
            h = S.INDEL_COUNTER.depth
            assert (h is not None) == (len(setting) == 3) == ("pileup spans (push)" in S.SCAN_SECONDS) and S.SNV_COUNTER is None
            if h is not None:
                _same(h, (made.depth, made.counts), "the scan beside the indel counter alone")
            assert np.array_equal(S.INDEL_COUNTER.finish(2), made.indel[0])
        finally:
            S.INDELS = None
            if S.INDEL_COUNTER is not None:
                if S.INDEL_COUNTER.depth is not None:
                    S.INDEL_COUNTER.depth.close()
                S.INDEL_COUNTER.close()
            S.INDEL_COUNTER = None
            if tables is not None:
                tables.close()
            bamio.set_carry(None)


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------
LEN, READ = 20500, 100
HET_SNVS, HOM_SNV = (3000, 5000), 4000                              # 0-based
DEL3, INS5, INS30, DEL60 = 7000, 9000, 11000, 13000                 # the anchors' 1-based P
INS5_SEQ = "ACGTA"


def _planted_reads(text, ins30):
    """(pos, record): the reads that carry the four indels, on both strands, with bases cut from the reference"""
    from tiddit_amd import bamio
    out = []

    def add(n, P, left, ops_of, name):
        for k in range(n):
            pos, ops = P - left - k, ops_of(k)
            bases, r = [], pos
            for op, ln, ins in ops:
                if op == 0:
                    bases.append(text[r:r + ln])
                    r += ln
                elif op == 2:
                    r += ln
                else:
                    bases.append(ins)
            seq = "".join(bases)
            out.append((pos, bamio.encode_record("%s%d" % (name, k), 0x10 * (k & 1), 0, pos, 60, [(op, ln) for op, ln, _ in ops], -1, -1, 0, seq=seq,
                                                 qual=bytes([40]) * len(seq))))
    add(30, DEL3, 40, lambda k: [(0, 40 + k, None), (2, 3, None), (0, 60 - k, None)], "del3_")
    add(20, INS5, 50, lambda k: [(0, 50 + k, None), (1, 5, INS5_SEQ), (0, 45 - k, None)], "ins5_")
    add(10, INS30, 40, lambda k: [(0, 40 + k, None), (1, 30, ins30), (0, 30 - k, None)], "ins30_")
    add(10, DEL60, 40, lambda k: [(0, 40 + k, None), (2, 60, None), (0, 60 - k, None)], "del60_")
    return out


def make_file(directory):
    """one contig of LEN bases, a 30x paired bulk cut from it, the SNVs written into the bulk's plain reads (a random half of them at the
    heterozygous sites, all at the homozygous one), the bulk reads over the homozygous insertion's anchor taken out, the indel reads added
    -> (bam, fa, names, lengths)"""
    from tiddit_amd import bamio, synth_bam
    rng = np.random.default_rng(90417)
    codes, last = [], 0
    for v in rng.integers(1, 4, LEN).tolist():                       # (no two neighbours equal: an indel's placement is its own)
        last = (last + v) % 4
        codes.append(last)
    text = "".join("ACGT"[c] for c in codes)
    ins30 = "".join("ACGT"[c] for c in rng.integers(0, 4, 30).tolist())
    table = [("small1", LEN)]
    bam, fa = os.path.join(directory, "small.bam"), os.path.join(directory, "small.fa")
    seqs = {"small1": np.frombuffer(text.encode(), dtype=np.uint8)}
    C._write_fasta(fa, table, seqs)
    bulk_path = bam + ".bulk"
    synth_bam.write_wgs_sv_bam(bulk_path, table, depth=30, read_len=READ, insert=250, insert_sd=10, seed=90417, sv_per_mb=200, threads=2, ref_seqs=seqs)
    rd = bamio.BamReader(bulk_path)
    bulk = list(rd.batches())
    rd.close()
    os.remove(bulk_path)
    code = {"A": 1, "C": 2, "G": 4, "T": 8}
    records = []
    for b in bulk:
        raw = np.asarray(b.raw, dtype=np.uint8).copy()
        for i in range(len(b)):
            o = int(b.rec_off[i])
            bs, = struct.unpack_from("<I", raw, o)
            tid, pos, end = int(b.tid[i]), int(b.pos[i]), int(b.end[i])
            if tid == 0 and pos <= INS5 + 10 and end >= INS5 - 10:
                continue
            l_name, n_cig = int(raw[o + 12]), int(raw[o + 16]) | int(raw[o + 17]) << 8
            if tid == 0 and n_cig == 1 and int(b.cigar_first[i]) == READ << 4:
                for s in HET_SNVS + (HOM_SNV,):
                    if pos <= s < end and (s == HOM_SNV or rng.random() < 0.5):
                        qi, alt = s - pos, code["ACGT"[(codes[s] + 1) % 4]]
                        at = o + 36 + l_name + 4 + (qi >> 1)
                        raw[at] = (raw[at] & 0xf0) | alt if qi & 1 else (raw[at] & 0x0f) | (alt << 4)
            records.append((tid if tid >= 0 else 1 << 30, pos, len(records), raw[o:o + 4 + bs].tobytes()))
    for pos, rec in _planted_reads(text, ins30):
        records.append((0, pos, len(records), rec))
    records.sort(key=lambda r: r[:3])
    C.write_records(bam, table, [r[3] for r in records])
    return bam, fa, ["small1"], [LEN], text, ins30


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


ON = {"TIDDIT_SNVS": "2", "TIDDIT_INDELS": "2"}


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """(each job is checked before the next one is started: a crash, a time-out or a GPU error ends the fixture there)"""
    m = Made()
    m.dir = str(tmp_path_factory.mktemp("small_vcf"))
    m.bam, m.fa, m.names, m.lengths, m.text, m.ins30 = make_file(m.dir)
    paths = {n: os.path.join(m.dir, n) for n in ("off", "on", "host", "bad")}
    _ok(_job(m, paths["off"], **ON))
    r = _ok(_job(m, paths["on"], TIDDIT_SMALL_VCF="1", **ON))
    _ok(_job(m, paths["host"], TIDDIT_SMALL_VCF="1", TIDDIT_HOST_INGEST="1", **ON))
    return m, paths, r


def test_the_file_equals_the_definitions_file_byte_for_byte_and_holds_the_planted_genotypes(jobs, tmp_path):
    from tiddit_amd import bamio, refseq, tiddit_clip_vcf, tiddit_indels, tiddit_pileup, tiddit_small_vcf as V, tiddit_snvs
    m, paths, r = jobs
    rd = bamio.BamReader(m.bam)
    header, batches = rd.header, list(rd.batches())
    rd.close()
    host = refseq.HostReference({0: refseq.codes_of_bases(m.text)})
    spans, sn, skeys, ssn, ikeys, isn = [], {}, [], {}, [], {}
    for b in batches:
        tiddit_pileup.spans_of_batch(b, spans, sn, m.lengths, 20)
        tiddit_snvs.keys_of_batch_by_read(b, skeys, ssn, host, 20, 20)
        tiddit_indels.keys_of_batch_by_read(b, ikeys, isn, 20)
    depth = tiddit_pileup.depth_of(spans, m.lengths)
    srows, irows = tiddit_snvs.summarise(skeys, ssn, 2)[1], tiddit_indels.summarise(ikeys, isn, 2)[1]
    lines, above, no_ref = V.records_of(srows, V.genotype_rows(srows, depth, m.lengths), irows, V.genotype_rows(irows, depth, m.lengths), m.names, host)
    counts = V.counts_of(tiddit_pileup.counters_of(sn), above, no_ref, len(lines))
    want = str(tmp_path / "want.small.vcf")
    V.write_file(want, tiddit_clip_vcf.header_parts(header, "ALL", "3.9.5"), 20, False, counts, lines)
    got = _content(paths["on"] + ".small.vcf")
    assert len(lines) >= 7 and got == _content(want)
    assert _content(paths["host"] + ".small.vcf") == got
    assert [l for l in r.stdout.split("\n") if l.startswith("small vcf:")] == [V.summary_line(counts)]
    # the planted genotypes
    by_pos = {}
    for l in got.decode().split("\n"):
        if l and not l.startswith("#"):
            f = l.split("\t")
            by_pos.setdefault(int(f[1]), []).append(f)
    one = lambda P, typ: next(f for f in by_pos[P] if f[7].startswith("TYPE=" + typ))
    gt = lambda f: f[9].split(":")[0]
    base = lambda i: m.text[i]
    for s in HET_SNVS:
        f = one(s + 1, "SNV")
        assert (f[3], f[4], gt(f), f[6]) == (base(s), "ACGT"[("ACGT".index(base(s)) + 1) % 4], "0/1", "PASS"), f
    f = one(HOM_SNV + 1, "SNV")
    assert gt(f) == "1/1" and f[6] == "PASS" and f[9].split(":")[2].startswith("0,"), f
    f = one(DEL3, "DEL")
    assert (f[3], f[4], gt(f)) == (m.text[DEL3 - 1:DEL3 + 3], base(DEL3 - 1), "0/1") and f[7].startswith("TYPE=DEL;AS=30;FWD=15;REV=15"), f
    f = one(INS5, "INS")
    assert (f[3], f[4], gt(f)) == (base(INS5 - 1), base(INS5 - 1) + INS5_SEQ, "1/1") and f[9].startswith("1/1:20:0,20:"), f
    f = one(INS30, "INS")
    assert (f[3], f[4]) == (base(INS30 - 1), "<INS>") and f[7] == "TYPE=INS;AS=10;FWD=5;REV=5;SVLEN=30", f
    f = one(DEL60, "DEL")
    assert (f[3], f[4]) == (base(DEL60 - 1), "<DEL>") and f[7] == "TYPE=DEL;AS=10;FWD=5;REV=5;END=%d;SVLEN=-60" % (DEL60 + 60), f


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    m, paths, r = jobs
    off, on, host = (_files(paths[k]) for k in ("off", "on", "host"))
    assert set(on) - set(off) == {".small.vcf"} and set(off) <= set(on) and {".snvs.tab", ".indels.tab"} <= set(off) and len(off) >= 7
    assert all(on[k] == off[k] for k in off), [k for k in off if on[k] != off[k]]
    assert not os.path.exists(paths["off"] + ".small.vcf")
    assert host[".small.vcf"] == on[".small.vcf"] and host[".snvs.tab"] == on[".snvs.tab"] and host[".indels.tab"] == on[".indels.tab"]


@pytest.mark.parametrize("env,text", [
    ({"TIDDIT_SMALL_VCF": "2", "TIDDIT_SNVS": "2"}, "error, TIDDIT_SMALL_VCF=2: the switch is 1"),
    ({"TIDDIT_SMALL_VCF": "1"}, "error, TIDDIT_SMALL_VCF=1: the switch genotypes the rows of TIDDIT_SNVS and TIDDIT_INDELS, neither of which is set"),
    ({"TIDDIT_SMALL_VCF": "1", "TIDDIT_SNVS": "2:30", "TIDDIT_INDELS": "2"},
     "error, TIDDIT_SMALL_VCF=1: TIDDIT_SNVS and TIDDIT_INDELS have different minimum MAPQ (30 and 20): the depth is counted at one"),
    ({"TIDDIT_SMALL_VCF": "1", "TIDDIT_SNVS": "1", "RANK": "0", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29548",
      "TIDDIT_DIST_BACKEND": "gloo", "TIDDIT_FORCE_DIST": "1"}, "error, TIDDIT_SMALL_VCF is a one-process switch")],
    ids=["another value", "no partner", "two cuts", "n ranks"])
def test_a_refused_switch_is_one_error_line_before_the_scan(jobs, env, text):
    m, paths, r = jobs
    bad = _job(m, paths["bad"], timeout=120, **env)
    assert bad.returncode == 1, (bad.returncode, bad.stdout[-1000:], bad.stderr[-2000:])
    errors = [l for l in bad.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith(text) and (errors[0] == text or "one-process" in text), errors
    assert not os.path.exists(paths["bad"] + "_tiddit") and not os.path.exists(paths["bad"] + ".small.vcf") and not os.path.exists(paths["bad"] + ".snvs.tab")
