"""What the three consumers of the --sv scan that read raw record bytes (``tdt_alleles_*``, ``tdt_qc_*``, ``tdt_dup_*``) share on the host
side, pinned per consumer: the handle's own upload block through a creation, a growth and a reuse while too large (host batches of 1,
257 and 2 reads on ONE handle), a batch without record bytes on the same handle, and the pointer table of a real ``DeviceBamReader``
batch with any one column set to NULL — refused when the consumer reads the column, accepted with the reference's result when it does
not.  Every comparison is the one tests/test_gpu_{alleles,qc,dup}.py make: exact, against the case module's numpy restatement."""
import ctypes

import numpy as np
import pytest

import alleles_cases as AC
import dup_cases as D
import qc_cases as QC

pytestmark = pytest.mark.gpu

TABLE = ("tid", "pos", "end", "mapq", "flag", "mate_tid", "mate_pos", "tlen", "l_seq", "cigar_first", "cigar_last", "rec_off", "sa_off", "raw")


class _Alleles:
    M, case_name = AC, "sizes a batch of 257 reads"
    host_columns = ("tid", "pos", "end", "mapq", "flag", "rec_off")              # the arguments of tdt_alleles_push, in order
    needed = ("tid", "pos", "end", "mapq", "flag", "rec_off", "raw")
    entry, entry_device = "tdt_alleles_push", "tdt_alleles_push_device"

    @staticmethod
    def handle(case, ctx=None):
        from tiddit_amd import tiddit_alleles
        pos, off = AC.table_of(case)
        return tiddit_alleles.AlleleCounter(pos, off, case["min_q"], case["min_bq"], ctx=ctx)

    @staticmethod
    def same(h, want, what):
        got = h.counts()
        assert np.array_equal(got[0], want[0]) and tuple(got[1:]) == tuple(want[1:]), (what, got[1:], want[1:])


class _Qc:
    M, case_name = QC, "shape a batch of 257 reads"
    host_columns = QC.Batch.COLUMNS
    needed = ("flag", "mapq", "tid", "mate_tid", "tlen", "l_seq", "rec_off", "raw")
    entry, entry_device = "tdt_qc_push", "tdt_qc_push_device"

    @staticmethod
    def handle(case, ctx=None):
        from tiddit_amd import tiddit_qc
        return tiddit_qc.QcCounter(ctx=ctx)

    @staticmethod
    def same(h, want, what):
        got = h.counts()
        assert got.dtype == np.uint64 and np.array_equal(got, want), (what, [(int(k), int(got[k]), int(want[k])) for k in np.flatnonzero(got != want)[:8]])


class _Dup:
    M, case_name = D, "shape a batch of 257 reads"
    host_columns = D.Batch.COLUMNS
    needed = ("flag", "tid", "pos", "end", "mate_tid", "mate_pos", "rec_off", "raw")
    entry, entry_device = "tdt_dup_push", "tdt_dup_push_device"

    @staticmethod
    def handle(case, ctx=None):
        from tiddit_amd import tiddit_dup
        return tiddit_dup.DupCounter(len(D.LENGTHS), max(D.LENGTHS), capacity=64, ctx=ctx)

    @staticmethod
    def same(h, want, what):
        rows, counts = want
        k1, k2, m = h.keys()
        got = D.rows_of(list(zip(k1.tolist(), k2.tolist(), m.tolist())))
        assert got.shape == rows.shape and np.array_equal(got, rows), (what, got.shape, rows.shape)
        c = h.finish()
        assert np.array_equal(c, counts), (what, [(int(k), int(c[k]), int(counts[k])) for k in np.flatnonzero(c != counts)[:8]])


CONSUMERS = (_Alleles, _Qc, _Dup)
IDS = ["alleles", "qc", "dup"]


def _case(C):
    return next(c for c in C.M.CASES if c["name"] == C.case_name)


def _with_reads(case, reads, cuts):
    """the case with other reads and cuts (and none of the batches the module built for it)"""
    out = {k: v for k, v in case.items() if not (isinstance(k, tuple) and k[0] == "built")}
    out.update(reads=reads, cuts=cuts, repeat=1)
    return out


@pytest.mark.parametrize("C", CONSUMERS, ids=IDS)
def test_one_handle_through_batches_of_1_257_and_2_reads_then_one_without_record_bytes(C):
    case = _case(C)
    r = case["reads"]
    assert len(r) == 257
    # one read (the block is created), one read past a 256-thread workgroup (it grows), two reads (it is reused while too large)
    grown = _with_reads(case, r[:1] + r + r[255:], (1, 258))
    batches = C.M.batches(grown)
    assert [len(b) for b in batches] == [1, 257, 2]
    h = C.handle(case)
    try:
        for b in batches:
            h.push_host_batch(b)
        C.same(h, C.M.reference(grown), "1 + 257 + 2 reads")
        # raw_len = 0: no record is readable; what the columns alone decide still counts
        bare = _with_reads(case, r, ())
        C.M.build(bare).raw = np.zeros(0, dtype=np.uint8)
        (b,) = C.M.batches(bare)
        assert len(b) == 257 and len(b.raw) == 0
        h.reset()
        h.push_host_batch(b)
        C.same(h, C.M.reference(bare), "no record bytes")
    finally:
        h.close()


@pytest.mark.parametrize("C", CONSUMERS, ids=IDS)
def test_the_device_table_with_one_column_null_is_refused_when_the_column_is_read_and_accepted_when_not(C, tmp_path):
    from tiddit_amd import bamio
    case = _case(C)
    assert case["reader_ok"]
    path = str(tmp_path / "case.bam")
    w = bamio.BamWriter(path, [("c%d" % t, ln) for t, ln in enumerate(case["lengths"])])
    w._buf += C.M.build(case, padding=False).raw.tobytes()
    w.close()
    want = C.M.reference(case)
    rd = bamio.DeviceBamReader(path)
    h = None
    try:
        h = C.handle(case, ctx=rd.ctx)
        push = getattr(rd.ctx.lib, C.entry_device)
        seen = 0
        for b in rd.batches():                                                         # (one batch; its buffers live until the reader moves on)
            seen += 1
            assert len(b) == 257 and b._raw_len > 0
            full = [b.dev[k] or None for k in TABLE]
            assert all(full) and TABLE[:13] == tuple(k for k, _ in bamio._FIELDS)
            for k, name in enumerate(TABLE):
                table = (ctypes.c_void_p * 14)(*(full[:k] + [None] + full[k + 1:]))
                h.reset()
                rc = push(h.handle, table, len(b), b._raw_len)
                if name in C.needed:
                    assert rc == -1, name                                              # TDT_E_ARG
                else:
                    assert rc == 0, name
                    C.same(h, want, name + " NULL")
            h.reset()
            assert push(h.handle, (ctypes.c_void_p * 14)(*full), len(b), b._raw_len) == 0  # (no refused call left anything behind)
            C.same(h, want, "the full table")
        assert seen == 1
    finally:
        if h is not None:
            h.close()
        rd.close()


@pytest.mark.parametrize("C", (_Qc, _Dup), ids=["qc", "dup"])
def test_host_record_offsets_that_decrease_are_refused(C):
    """(``tdt_alleles_push`` has never made this check and is not given such a batch)"""
    from tiddit_amd import _native
    case = _case(C)
    b = C.M.build(case)
    h = C.handle(case)
    try:
        P = _native.ptr
        cols = [np.ascontiguousarray(getattr(b, k)) for k in C.host_columns]
        assert C.host_columns[-1] == "rec_off"
        push = getattr(h.ctx.lib, C.entry)
        down = np.ascontiguousarray(b.rec_off[::-1])
        assert push(h.handle, *[P(c) for c in cols[:-1]], P(down), len(b), P(b.raw), len(b.raw)) == -1
        swap = b.rec_off.copy()
        swap[[100, 101]] = swap[[101, 100]]                                            # one step down in the middle
        assert push(h.handle, *[P(c) for c in cols[:-1]], P(swap), len(b), P(b.raw), len(b.raw)) == -1
        assert push(h.handle, *[P(c) for c in cols], len(b), P(b.raw), len(b.raw)) == 0
        C.same(h, C.M.reference(case), "after the refusals")
    finally:
        h.close()
