"""`TIDDIT_INDELS_NORM` on the GPU: the resident reference (csrc/tdt_refseq.hip: ``ref_pack`` against a plain strip-and-map, through the
host entry and the device entry), then ``indel_keys<true>`` (csrc/tdt_indel.hip) on every aimed case of tests/indel_norm_cases.py through
``tdt_indel_push`` and through ``tdt_indel_push_device`` from a small BAM — keys, the eleven counters, the rows and the three new counters
exactly equal to the definition (which tests/test_indel_norm_refs_cpu.py pins to the restatement and to the cases' claims) — the handle's
state, and the switch end to end — on the sv_e2e_small fixture, and on a BAM and FASTA made from the designed reference whose reads place the
same indels at several positions — every job a fresh child process under its own time limit.

Every test of this file fails on the parent commit: the entries and the switch do not exist there."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import indel_cases as D
import indel_norm_cases as N
from sv_e2e_common import load_fixture, materialise
from test_gpu_indels import SWITCHES, _files, _ok, _rows_text

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = []                       # the (case, entry) pairs that ran and passed
READER_OK = [c for c in N.CASES if c["reader_ok"]]
LINEBASES = (1, 2, 7, 15, 16, 17, 60, 61, 64)


# ---- the resident reference ---------------------------------------------------------------------------------------------------
def _refseq(lengths=N.LENGTHS, loaded=(0, 1, 2), ctx=None, linebases=60, eol=b"\n"):
    from tiddit_amd import refseq
    ref = refseq.RefSeq(lengths, ctx=ctx)
    for t in loaded:
        raw, _ = N.contig_raw(N.TEXT[t], linebases, eol)
        ref.load_fasta(t, np.frombuffer(raw, dtype=np.uint8), len(N.TEXT[t]), linebases, linebases + len(eol))
    return ref


@pytest.fixture(scope="module")
def tile():
    ref = _refseq(loaded=())
    try:
        return ref.layout()[2]
    finally:
        ref.close()


def _texts(tile):
    every = bytes(range(256)) * 2
    unit = b"=ACMGRSVTWYHKDBN" + b"acmgrsvtwyhkdbn" + b"-*.xXuU 0189"              # (no line end inside: these are cut into lines of every length)
    letters = unit * ((2 * tile + 1) // len(unit) + 1)
    assert len(letters) > 2 * tile + 1
    texts = [b"", b"A", b"ac", every[:15], every[:16], every[:17], every, letters[:tile - 1], letters[:tile], letters[:tile + 1], letters[:2 * tile + 1],
             N.TEXT[2]]
    assert [len(t) for t in texts[7:11]] == [tile - 1, tile, tile + 1, 2 * tile + 1]   # one workgroup short of a word, exactly one, two, three
    return texts


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("eol,final", [(b"\n", True), (b"\r\n", True), (b"\n", False)])
def test_pack_equals_a_plain_strip_and_map(entry, eol, final, tile):
    """every line length and text; the text of all 256 byte values is loaded WITHOUT line ends inside it being meant as such: its bytes 10
    and 13 are bases like any other (they map to N), which a layout of one line holds"""
    import torch
    from tiddit_amd import refseq
    texts = _texts(tile)
    ran = 0
    for lb in LINEBASES:
        jobs = [(t, lb) for t in texts if b"\n" not in t and b"\r" not in t] + [(t, max(len(t), 1)) for t in texts if b"\n" in t or b"\r" in t]
        ref = refseq.RefSeq([len(t) for t, _ in jobs])
        try:
            for tid, (text, linebases) in enumerate(jobs):
                raw, tail = N.contig_raw(text, linebases, eol, final)
                poison = raw + tail + b"ACGT" * 8                  # (what follows the contig in a file is never packed)
                if entry == "host":                             # (final: the file's last line end is handed over too, nbytes counts it)
                    ref.load_fasta(tid, np.frombuffer(poison, dtype=np.uint8)[:len(raw) + len(tail)].copy(), len(text), linebases, linebases + len(eol))
                else:                                           # (into a POISONED store: the contig's own words hold 0xA5 before the load)
                    assert ref.ctx.lib.tdt_debug_refseq_fill(ref.handle, tid, 0xA5) == 0
                    d = torch.from_numpy(np.frombuffer(poison, dtype=np.uint8).copy()).cuda()
                    ref.load_fasta_device(tid, d.data_ptr(), len(raw), len(text), linebases, linebases + len(eol))
                    torch.cuda.synchronize()
            nbytes, guard, _, offs, store = ref.layout(store=True)
            assert guard >= 8 and all(int(o) % 8 == 0 for o in offs)
            used = np.zeros(nbytes, dtype=bool)
            for tid, (text, _) in enumerate(jobs):
                want = N.codes(text)
                assert np.array_equal(ref.fetch(tid), want), (lb, tid, len(text))
                if len(text) > 3:
                    assert np.array_equal(ref.fetch(tid, 1, len(text) - 2), want[1:-1]) and np.array_equal(ref.fetch(tid, len(text) - 1, 1), want[-1:])
                assert len(ref.fetch(tid, len(text), 0)) == 0
                o = int(offs[tid])
                packed = np.zeros((len(text) + 1) // 2 * 2, dtype=np.uint8)
                packed[:len(text)] = want
                assert np.array_equal(store[o:o + len(packed) // 2], packed[0::2] << 4 | packed[1::2])        # the even base in the high nibble
                used[o:o + (len(text) + 1) // 2] = True
                assert not store[o - guard:o].any() and not store[o + (len(text) + 1) // 2:o + (len(text) + 15) // 16 * 8 + guard].any()
                ran += 1
            assert not store[~used].any()                          # the guards, and everything else nothing was loaded into, read as zero
        finally:
            ref.close()
    assert ran == len(LINEBASES) * len(texts)


@pytest.mark.parametrize("entry,linebases,eol", [("host", 60, b"\n"), ("device", 61, b"\r\n"), ("host", 100000, b"\n")])
def test_the_designed_reference_packs_exactly(entry, linebases, eol):
    """the 100 000-base and the odd 49 999-base contig, many workgroups each, against the strip-and-map base by base — and the store byte by byte"""
    import torch
    from tiddit_amd import refseq
    ref = refseq.RefSeq(N.LENGTHS)
    try:
        for t in (2, 0, 1):                                     # (not in store order: a load writes its own contig's words only)
            raw, _ = N.contig_raw(N.TEXT[t], linebases, eol)
            if entry == "host":
                ref.load_fasta(t, np.frombuffer(raw, dtype=np.uint8), N.LENGTHS[t], linebases, linebases + len(eol))
            else:
                assert ref.ctx.lib.tdt_debug_refseq_fill(ref.handle, t, 0xFF) == 0           # (a poisoned store)
                d = torch.from_numpy(np.frombuffer(raw + b"\xff" * 64, dtype=np.uint8).copy()).cuda()
                ref.load_fasta_device(t, d.data_ptr(), len(raw), N.LENGTHS[t], linebases, linebases + len(eol))
                torch.cuda.synchronize()
        nbytes, guard, tile, offs, store = ref.layout(store=True)
        assert N.LENGTHS[0] > 24 * tile and N.LENGTHS[1] % 16 == 15
        want = np.zeros(nbytes, dtype=np.uint8)
        for t in range(3):
            assert np.array_equal(ref.fetch(t), N.CODES[t]), t
            c = np.zeros((N.LENGTHS[t] + 1) // 2 * 2, dtype=np.uint8)
            c[:N.LENGTHS[t]] = N.CODES[t]
            want[int(offs[t]):int(offs[t]) + len(c) // 2] = c[0::2] << 4 | c[1::2]
        assert np.array_equal(store, want)
    finally:
        ref.close()


def test_refseq_refusals_leave_the_outputs_untouched():
    from tiddit_amd import _native
    ctx = _native.default_context()
    lib, P = ctx.lib, _native.ptr
    h = ctypes.c_void_p(0x5a5a)
    lens = np.array([100, 7, 0], dtype=np.int64)
    assert lib.tdt_refseq_create(None, 3, P(lens), ctypes.byref(h)) == -1 and lib.tdt_refseq_create(ctx.handle, 3, None, ctypes.byref(h)) == -1
    assert lib.tdt_refseq_create(ctx.handle, 3, P(lens), None) == -1 and lib.tdt_refseq_create(ctx.handle, -1, P(lens), ctypes.byref(h)) == -1
    assert lib.tdt_refseq_create(ctx.handle, 2, P(np.array([5, 1 << 31], dtype=np.int64)), ctypes.byref(h)) == -1          # 2^31 bases
    assert lib.tdt_refseq_create(ctx.handle, 1, P(np.array([-1], dtype=np.int64)), ctypes.byref(h)) == -1 and h.value == 0x5a5a
    assert lib.tdt_refseq_create(ctx.handle, 3, P(lens), ctypes.byref(h)) == 0
    try:
        raw = np.frombuffer(b"ACGTACGTAC" * 10, dtype=np.uint8)
        out = np.full(16, 7, dtype=np.uint8)
        assert lib.tdt_refseq_fetch(h, 0, 0, 4, P(out)) == -1                                          # not loaded yet
        assert lib.tdt_refseq_load_fasta(None, 0, P(raw), 100, 100, 100, 101) == -1 and lib.tdt_refseq_load_fasta(h, 0, None, 100, 100, 100, 101) == -1
        assert lib.tdt_refseq_load_fasta(h, 3, P(raw), 100, 100, 100, 101) == -1 and lib.tdt_refseq_load_fasta(h, -1, P(raw), 100, 100, 100, 101) == -1
        assert lib.tdt_refseq_load_fasta(h, 0, P(raw), 99, 99, 100, 101) == -1                         # another length than at create
        assert lib.tdt_refseq_load_fasta(h, 0, P(raw), 99, 100, 100, 101) == -1                        # too few bytes
        assert lib.tdt_refseq_load_fasta(h, 0, P(raw), 100, 100, 10, 13) == -6 and lib.tdt_refseq_load_fasta(h, 0, P(raw), 100, 100, 0, 1) == -6
        assert lib.tdt_refseq_load_fasta_device(h, 0, None, 100, 100, 100, 101) == -1 and lib.tdt_refseq_load_fasta_device(h, 5, None, 0, 0, 1, 2) == -1
        assert lib.tdt_refseq_fetch(h, 0, 0, 4, P(out)) == -1                                          # nothing refused above loaded anything
        assert lib.tdt_refseq_load_fasta(h, 0, P(raw), 100, 100, 100, 101) == 0
        assert lib.tdt_refseq_load_fasta(h, 0, P(raw), 100, 100, 100, 101) == -1                       # loaded twice
        assert lib.tdt_refseq_load_fasta(h, 2, None, 0, 0, 0, 0) == 0                                  # an empty contig
        assert lib.tdt_refseq_fetch(None, 0, 0, 4, P(out)) == -1 and lib.tdt_refseq_fetch(h, 0, 0, 4, None) == -1
        assert lib.tdt_refseq_fetch(h, 3, 0, 1, P(out)) == -1 and lib.tdt_refseq_fetch(h, 1, 0, 1, P(out)) == -1
        assert lib.tdt_refseq_fetch(h, 0, 97, 4, P(out)) == -1 and lib.tdt_refseq_fetch(h, 0, -1, 4, P(out)) == -1 and lib.tdt_refseq_fetch(h, 0, 101, 0, P(out)) == -1
        assert lib.tdt_refseq_fetch(h, 2, 0, 1, P(out)) == -1 and (out == 7).all()
        assert lib.tdt_refseq_fetch(h, 0, 96, 4, P(out)) == 0 and out[:4].tolist() == [4, 8, 1, 2] and (out[4:] == 7).all()
        assert lib.tdt_debug_refseq_fill(None, 1, 0xff) == -1 and lib.tdt_debug_refseq_fill(h, 3, 0xff) == -1 and lib.tdt_debug_refseq_fill(h, 0, 0xff) == -1
        assert lib.tdt_refseq_fetch(h, 0, 96, 4, P(out)) == 0 and out[:4].tolist() == [4, 8, 1, 2]       # (a loaded contig is never filled)
        assert lib.tdt_refseq_layout(None, P(out), None, None) == -1 and lib.tdt_refseq_layout(h, None, None, None) == -1
        assert lib.tdt_indel_set_reference(None, h) == -1
        st = np.full(3, 7, dtype=np.uint64)
        assert lib.tdt_indel_norm_stats(None, P(st)) == -1 and (st == 7).all()
    finally:
        assert lib.tdt_refseq_destroy(h) == 0 and lib.tdt_refseq_destroy(None) == 0


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wanted():
    return {c["name"]: N.definition(c) for c in N.CASES}


def _counter(case, ctx=None, capacity=1 << 12):
    from tiddit_amd import tiddit_indels
    return tiddit_indels.IndelCounter(len(case["lengths"]), case["Q"], capacity=capacity, ctx=ctx)


def _same(h, want, what):
    keys, by_support, norm = want
    rows = D.key_rows(keys)
    k1, k2 = h.keys()
    got = D.key_rows(list(zip(k1.tolist(), k2.tolist())))
    assert got.shape == rows.shape and np.array_equal(got, rows), (what, got.shape, rows.shape)
    for S, (counts, columns) in by_support.items():
        c = h.finish(S)
        assert np.array_equal(c, counts), (what, S, c.tolist(), counts.tolist())
        for name, x, y in zip(("K1", "K2", "SUPPORT", "REV"), h.rows(), columns):
            assert x.shape == y.shape and np.array_equal(x, y), (what, S, name, x[:8].tolist(), y[:8].tolist())
    assert tuple(int(v) for v in h.norm_stats()) == norm, (what, h.norm_stats().tolist(), norm)


@pytest.mark.parametrize("case", N.CASES, ids=[c["name"] for c in N.CASES])
def test_push_with_a_reference_equals_the_definition(case, wanted):
    ref = _refseq(loaded=case["loaded"])
    h = _counter(case)
    try:
        h.set_reference(ref)
        for b in D.batches(case):
            h.push_host_batch(b)
        _same(h, wanted[case["name"]], case["name"])
    finally:
        h.close()
        ref.close()
    PAIRS.append((case["name"], "push"))


@pytest.mark.parametrize("case", READER_OK, ids=[c["name"] for c in READER_OK])
def test_push_device_from_a_small_bam_equals_the_definition(case, wanted, tmp_path):
    from tiddit_amd import bamio
    path = str(tmp_path / "case.bam")
    b = D.build(case, padding=False)
    w = bamio.BamWriter(path, [(N.NAMES[t], ln) for t, ln in enumerate(case["lengths"])])
    w._buf += b.raw.tobytes()                     # the case's records as they are
    w.close()
    rd = bamio.DeviceBamReader(path)
    h = ref = None
    try:
        ref = _refseq(loaded=case["loaded"], ctx=rd.ctx, linebases=61, eol=b"\r\n")
        h = _counter(case, ctx=rd.ctx)
        h.set_reference(ref)
        n = 0
        for bt in rd.batches():
            h.push_device_batch(bt)
            n += len(bt)
        assert n == len(case["reads"])
        _same(h, wanted[case["name"]], case["name"])
    finally:
        if h is not None:
            h.close()
        if ref is not None:
            ref.close()
        rd.close()
    PAIRS.append((case["name"], "push_device"))


def test_the_stated_count_of_case_entry_pairs_ran():
    assert len(N.CASES) == N.N_CASES == 41 and len(READER_OK) == 38
    assert len(set(PAIRS)) == 41 + 38, len(set(PAIRS))


def _case(family):
    return next(c for c in N.CASES if c["family"] == family)


def test_one_indel_at_three_placements_is_one_row_with_a_reference_and_three_without(wanted):
    case = _case("sets")
    ref = _refseq()
    h = _counter(case)
    try:
        for b in D.batches(case):
            h.push_host_batch(b)
        plain = N.definition(case, ref=None)
        _same(h, plain, "no reference")
        assert len(h.rows()[0]) == 0 and int(h.finish(1)[D.SN.index("distinct_events")]) == 6            # (S = 3: no row; six placements)
        h.reset()
        h.set_reference(ref)
        for b in D.batches(case):
            h.push_host_batch(b)
        _same(h, wanted[case["name"]], "reference")
        h.finish(3)
        k1, k2, sup, rev = h.rows()
        assert k1.tolist() == [D.K1(0, N.homopolymer_at(25)), D.K1(0, 6000)] and k2.tolist() == [D.DEL(2), D.INS("CA")]
        assert sup.tolist() == [3, 3] and rev.tolist() == [2, 1]
    finally:
        h.close()
        ref.close()


def test_state_across_pushes_detaching_and_two_handles(wanted):
    a, b = _case("four"), _case("ins_repeat")
    ref = _refseq()
    h, g = _counter(a), _counter(b)
    try:
        h.set_reference(ref)
        g.set_reference(ref)
        first, = D.batches(a)
        h.push_host_batch(first.cut(0, 1))
        g.push_host_batch(D.build(b))
        assert tuple(h.norm_stats()) == (4, 0, 0)
        h.push_host_batch(first.cut(1, 2))
        _same(h, wanted[a["name"]], "two pushes")
        _same(g, wanted[b["name"]], "the other handle")
        h.reset()
        assert not h.norm_stats().any()
        h.set_reference(None)                                   # detached: today's keys, and the new counters stay zero
        h.push_host_batch(first)
        _same(h, N.definition(a, ref=None), "detached")
        _same(g, wanted[b["name"]], "the other handle, still attached")
    finally:
        h.close()
        g.close()
        ref.close()


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------
def _job(bam, fa, out, fx, timeout=600, **env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES + ("TIDDIT_INDELS_NORM",)}
    e.update(env)
    argv = [sys.executable, "-m", "tiddit_amd", "--sv", "--bam", bam, "--ref", fa, "-o", out, "--skip_assembly", "-s", str(fx["params"]["n_reads_stats"])]
    return subprocess.run(argv, cwd=REPO, env=e, capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def jobs(golden_dir, tmp_path_factory):
    """(each job is checked before the next one is started: a crash, a time-out or a GPU error ends the fixture there)"""
    fx = load_fixture(golden_dir, "sv_e2e_small.json")
    d = str(tmp_path_factory.mktemp("indel_norm"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    paths = {n: os.path.join(d, n) for n in ("plain", "norm", "host", "alone", "bad", "short")}
    _ok(_job(bam, fa, paths["plain"], fx, TIDDIT_INDELS="1:20"))
    r = _ok(_job(bam, fa, paths["norm"], fx, TIDDIT_INDELS="1:20", TIDDIT_INDELS_NORM="1"))
    _ok(_job(bam, fa, paths["host"], fx, TIDDIT_INDELS="1:20", TIDDIT_INDELS_NORM="1", TIDDIT_HOST_INGEST="1"))
    return fx, bam, fa, d, paths, r


def test_the_file_equals_the_definition_with_the_reference(jobs, tmp_path):
    from tiddit_amd import bamio, fasta, refseq, tiddit_indels
    fx, bam, fa, d, paths, r = jobs
    rd = bamio.BamReader(bam)
    names = list(rd.references)
    f = fasta.FastaFile(fa)
    ref = refseq.HostReference({t: refseq.codes_of_bases(f.fetch_array(n)) for t, n in enumerate(names)})
    sn, keys = {}, []
    for b in rd.batches():
        keys.extend(tiddit_indels.keys_of_batch(b, sn, 20, ref))
    rd.close()
    counts, rows = tiddit_indels.summarise(keys, sn, 1)
    norm = [sn.get(k, 0) for k in N.NORM_SN]
    assert norm[0] > 0 and len(rows) > 100                        # (the planted deletions: some of them lie beside a base equal to their last)
    got = open(paths["norm"] + ".indels.tab").read()
    head, body, cov = _rows_text(paths["norm"] + ".indels.tab")
    assert head[0] == "# tiddit_amd indels v1 min_support=1 min_mapq=20 left_normalised=1024"
    assert head[12:15] == ["SN\t%s\t%d" % (k, v) for k, v in zip(N.NORM_SN, norm)] and len(head) == 16
    want = str(tmp_path / "want.indels.tab")
    cover = {}                                                  # (the COV column is the job's own: taken from the file, compared with the plain job's below)
    tiddit_indels.write_file(want, counts, rows, names, cover, 1, 20, norm)
    whead, wbody, _ = _rows_text(want)
    assert head == whead and body == wbody
    plain = dict(((b[0], b[1]), c) for b, c in zip(*_rows_text(paths["plain"] + ".indels.tab")[1:]))
    assert all(c != "." for c in cov) and all(plain[(b[0], b[1])] == c for b, c in zip(body, cov) if (b[0], b[1]) in plain)
    assert "indels, left-normalised: %d events shifted, %d stopped at the cap of 1024 bases, %d off the reference" % tuple(norm) in r.stdout
    assert got.count("\n") == 15 + 1 + len(rows)


def test_host_ingest_writes_the_same_bytes(jobs):
    fx, bam, fa, d, paths, r = jobs
    assert open(paths["host"] + ".indels.tab", "rb").read() == open(paths["norm"] + ".indels.tab", "rb").read()


def test_without_the_switch_nothing_changes_and_with_it_only_the_table(jobs):
    fx, bam, fa, d, paths, r = jobs
    plain, norm = _files(paths["plain"]), _files(paths["norm"])
    assert set(plain) == set(norm) and len(plain) >= 6
    assert [k for k in plain if plain[k] != norm[k]] == [".indels.tab"]
    text = open(paths["plain"] + ".indels.tab").read()
    assert "left_normalised" not in text and "shifted_events" not in text and text.split("\n")[12].startswith("#CHROM")


# ---- a job whose reads place the same indels differently ----------------------------------------------------------------------
def _plain_job(bam, fa, out, timeout=300, **env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES + ("TIDDIT_INDELS_NORM",)}
    e.update(env)
    argv = [sys.executable, "-m", "tiddit_amd", "--sv", "--bam", bam, "--ref", fa, "-o", out, "--skip_assembly"]
    return subprocess.run(argv, cwd=REPO, env=e, capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    """the designed reference as a FASTA, and a BAM of the reads of three aimed cases (placements of one indel at several positions, on
    both strands), sorted; three jobs, each checked before the next is started"""
    from tiddit_amd import bamio
    d = str(tmp_path_factory.mktemp("indel_norm_designed"))
    fa, bam = os.path.join(d, "designed.fa"), os.path.join(d, "designed.bam")
    open(fa, "wb").write(N.fasta_bytes(list(zip(N.NAMES, N.TEXT)), 60))
    reads = [r for c in N.CASES if c["family"] in ("sets", "ins_repeat") or c["name"].startswith("homopolymer of 16:") for r in c["reads"]]
    reads.sort(key=lambda r: (r["tid"], r["pos"]))
    w = bamio.BamWriter(bam, list(zip(N.NAMES, N.LENGTHS)))
    w._buf += D.build_reads(reads, padding=False).raw.tobytes()
    w.close()
    paths = {n: os.path.join(d, n) for n in ("plain", "norm", "host")}
    _ok(_plain_job(bam, fa, paths["plain"], TIDDIT_INDELS="2"))
    _ok(_plain_job(bam, fa, paths["norm"], TIDDIT_INDELS="2", TIDDIT_INDELS_NORM="1"))
    _ok(_plain_job(bam, fa, paths["host"], TIDDIT_INDELS="2", TIDDIT_INDELS_NORM="1", TIDDIT_HOST_INGEST="1"))
    return bam, fa, paths, len(reads)


def test_placements_of_one_indel_become_one_row_of_the_written_table(designed, tmp_path):
    from tiddit_amd import bamio, tiddit_indels
    bam, fa, paths, n_reads = designed
    want = {}
    for name, ref in (("plain", None), ("norm", N.host_reference())):
        rd = bamio.BamReader(bam)
        sn, keys = {}, []
        for b in rd.batches():
            keys.extend(tiddit_indels.keys_of_batch(b, sn, 20, ref))
        rd.close()
        counts, rows = tiddit_indels.summarise(keys, sn, 2)
        assert int(counts[D.SN.index("records")]) == n_reads == 6 + 66 + 16
        path = str(tmp_path / (name + ".tab"))
        tiddit_indels.write_file(path, counts, rows, list(N.NAMES), {}, 2, 20, None if ref is None else [sn.get(k, 0) for k in N.NORM_SN])
        want[name] = _rows_text(path)[:2]
        assert _rows_text(paths[name] + ".indels.tab")[:2] == want[name], name
    # the table without the reference: every placement a key of its own; only the three placements that two cases share reach a support of 2
    assert want["plain"][1] == [["c0", "6004", "INS", "2", "CA", "2", "1", "1"], ["c0", "6011", "INS", "2", "AC", "2", "2", "0"],
                                ["c0", "6040", "INS", "2", "CA", "2", "2", "0"]]
    # with it: the 2-base deletion of the 25-A run once, SUPPORT 3 = FWD 1 + REV 2; the CA unit of both CA runs once each; the 16-A run's base
    h25, h16 = N.homopolymer_at(25), N.homopolymer_at(16)
    assert want["norm"][1] == [["c0", str(h16), "DEL", "1", ".", "16", "16", "0"], ["c0", str(h25), "DEL", "2", ".", "3", "1", "2"],
                               ["c0", "6000", "INS", "2", "CA", "44", "43", "1"], ["c1", "300", "INS", "4", "CACA", "25", "25", "0"]]
    assert open(paths["host"] + ".indels.tab", "rb").read() == open(paths["norm"] + ".indels.tab", "rb").read()
    plain, norm = _files(paths["plain"]), _files(paths["norm"])
    assert set(plain) == set(norm) and [k for k in plain if plain[k] != norm[k]] == [".indels.tab"]


def test_the_switch_without_its_partner_a_bad_value_and_a_short_fasta_are_errors(jobs):
    fx, bam, fa, d, paths, r = jobs
    for name, env, line in (("alone", {"TIDDIT_INDELS_NORM": "1"}, "error, TIDDIT_INDELS_NORM=1: the switch left-normalises the events of TIDDIT_INDELS: TIDDIT_INDELS not set"),
                            ("bad", {"TIDDIT_INDELS": "1", "TIDDIT_INDELS_NORM": "yes"}, "error, TIDDIT_INDELS_NORM=yes: the switch is 1")):
        res = _job(bam, fa, paths[name], fx, timeout=120, **env)
        assert res.returncode == 1 and [l for l in res.stdout.split("\n") if l.startswith("error")] == [line]
        assert not os.path.exists(paths[name] + "_tiddit") and not os.path.exists(paths[name] + ".indels.tab")
    short = os.path.join(d, "short.fa")
    lines = open(fa).read().rstrip("\n").split("\n")
    open(short, "w").write("\n".join(lines[:-1]) + "\n")           # the last contig loses its last line
    res = _job(bam, short, paths["short"], fx, timeout=120, TIDDIT_INDELS="1", TIDDIT_INDELS_NORM="1")
    errors = [l for l in res.stdout.split("\n") if l.startswith("error")]
    assert res.returncode == 1 and len(errors) == 1 and errors[0].startswith("error, TIDDIT_INDELS_NORM=1: contig ") and "bases in the BAM header" in errors[0]
    assert not os.path.exists(paths["short"] + "_tiddit") and not os.path.exists(paths["short"] + ".indels.tab")
