"""`TIDDIT_CLIPS_FAR` on the GPU: the launches of csrc/tdt_clip_far.hip on every aimed case of tests/clip_far_cases.py through both
entries — ``tdt_clip_far_sites`` on host columns, ``tdt_clip_far_sites_device`` on the same columns in caller-owned device memory with
poisoned, padded outputs — against the definition (which tests/test_clip_far_refs_cpu.py pins to the restatement and to the cases'
claims), exactly; the two large references (dispersed duplications beyond 2^20 bases on 2.2 Mb, windows over the grid's stride); through
the clip counter's handle (push, finish, ``tdt_clip_far`` on the rows where they lie, ``tdt_clip_far_rows``); the C-ABI refusals; and the
switch end to end on a generated reference of three contigs and 30 kb with a planted translocation, a dispersed duplication and a
mobile-element-like sequence present five times, every job a fresh child process under its own time limit (the first job that fails
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
import clip_far_cases as C

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = []                       # the (case, entry) pairs that ran and passed
POISON, PADDING = 0x5a, 16
NAMES6 = ("status", "contig", "PARTNER", "strand", "mismatches", "HITS")


@pytest.fixture(scope="module")
def ctx():
    from tiddit_amd import _native
    return _native.default_context()


def _refseq(case, ctx=None):
    from tiddit_amd import refseq
    ref = refseq.RefSeq(case["lengths"], ctx=ctx)
    for t, text in enumerate(case["contigs"]):
        if text is not None:
            ref.load_fasta(t, np.frombuffer(C.fasta_raw(text), dtype=np.uint8), len(text), 60, 61)
    return ref


@pytest.fixture(scope="module")
def wanted():
    """every case's definition, once, checked against the case's claim"""
    out = {}
    for c in C.CASES:
        out[c["name"]] = C.definition(c)
        assert C.agrees_with_claim(c, out[c["name"]][0], out[c["name"]][2]) is None, c["name"]
    return out


def _columns_of(placed):
    return tuple(np.array([p[k] for p in placed], dtype=np.uint32) for k in range(6))


def _sites_device(ctx, ref, case):
    """the device entry on torch-owned memory: the outputs are PADDING entries longer than the sites and filled with POISON"""
    import torch
    cols = C.columns(case)
    n = len(cols[0])
    as_bytes = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy() if len(a) else np.zeros(8, dtype=np.uint8)).cuda()
    ins = [as_bytes(a) for a in cols]
    outs = [torch.full(((n + PADDING) * 4,), POISON, dtype=torch.uint8).cuda() for _ in range(6)]
    torch.cuda.synchronize()
    rc = ctx.lib.tdt_clip_far_sites_device(ctx.handle, ref.handle, n, *[ctypes.c_void_p(t.data_ptr()) for t in ins], case["K"], case["M"],
                                           *[ctypes.c_void_p(t.data_ptr()) for t in outs])
    assert rc == 0, rc
    got = [t.cpu().numpy().view(np.uint32) for t in outs]
    assert all((g[n:] == 0x5a5a5a5a).all() for g in got)                       # nothing behind the last site is written
    return tuple(g[:n].copy() for g in got)


def _equal(case, got, placed):
    for name, x, y in zip(NAMES6, got, _columns_of(placed)):
        assert x.dtype == np.uint32 and x.shape == y.shape and np.array_equal(x, y), (case["name"], name, np.flatnonzero(x != y)[:8].tolist())


@pytest.mark.parametrize("entry", ["sites", "sites_device"])
@pytest.mark.parametrize("case", C.CASES, ids=[c["name"] for c in C.CASES])
def test_both_entries_equal_the_definition(case, entry, wanted, ctx):
    from tiddit_amd import tiddit_clip_far as F
    ref = _refseq(case, ctx)
    try:
        if C.first_nibble(case["lengths"], 1) != 2 * int(ref.layout()[3][1]):   # (the cases aim at store nibbles: the layout they assume is the store's)
            raise AssertionError("the store's layout is not the cases'")
        got = F.far_sites(ref, *C.columns(case), case["K"], case["M"]) if entry == "sites" else _sites_device(ctx, ref, case)
    finally:
        ref.close()
    _equal(case, got, wanted[case["name"]][0])
    PAIRS.append((case["name"], entry))


def test_the_stated_count_of_case_entry_pairs_ran():
    assert len(C.CASES) == C.N_CASES == 43
    assert len(set(PAIRS)) == 2 * 43, len(set(PAIRS))


def test_the_large_references_equal_the_definition(ctx):
    from tiddit_amd import tiddit_clip_far as F
    for case in C.big_cases():
        placed, counts, rows = C.definition(case)
        assert C.agrees_with_claim(case, placed, rows) is None, case["name"]
        ref = _refseq(case, ctx)
        try:
            got = F.far_sites(ref, *C.columns(case), case["K"], case["M"])
        finally:
            ref.close()
        _equal(case, got, placed)


# ---- through the handle -------------------------------------------------------------------------------------------------------------
def _event_case():
    return next(c for c in C.CASES if c["name"] == "events: a translocation with 5 bases of microhomology")


def _handle_reads(case):
    """clipped reads over the case's two junction sites (and its decoy), their clips cut from the case's reference where its sites say
    the clipped bases lie; a site whose clips are too short to be searched; a site whose clips are random"""
    seqs = [C.Seq(t) for t in case["contigs"]]
    reads = []
    for x in case["sites"]:
        g, q = seqs[x["claim"]["ptid"]], x["claim"]["partner"]
        for k in (30, 34, 41):
            if x["side"] == C.R_SIDE:
                reads.append(D.rd(tid=x["tid"], pos=x["P"] - 40, m=40, trail=g.get(q, q + k - 1), flag=D.REV * (k == 34)))
            else:
                reads.append(D.rd(tid=x["tid"], pos=x["P"] - 1, m=40, lead=g.get(q - k + 1, q)))
    reads += [D.rd(tid=1, pos=100, m=30, trail=seqs[0].get(1000, 1011)) for _ in range(3)]           # CLEN 12 < K
    reads += [D.rd(tid=0, pos=100, m=30, trail=C.seeded(30, 9)) for _ in range(2)]                   # nowhere in the reference
    return sorted(reads, key=lambda r: (r["tid"], r["pos"]))


def test_the_handle_places_the_rows_of_its_finish_where_they_lie(ctx):
    from tiddit_amd import tiddit_clip_far as F, tiddit_clips
    case = _event_case()
    K, M = 20, 2
    ref = _refseq(case, ctx)
    h = tiddit_clips.ClipCounter(len(case["lengths"]), 20, 10, capacity=1 << 10, ctx=ctx)
    try:
        h.push_host_batch(D.build_batch(_handle_reads(case)))
        counts = h.finish(2)
        rows = h.rows()
        assert len(rows[0]) == 5 == int(counts[D.SN.index("reported_sites")])
        sn, got, ms = F.far_counter(h, ref, K, M)
        host = C.host_reference(case)
        placed = [F.place_site(host, int(k1) >> 32, int(k1) & 0xffffffff, int(s), int(cl), int(co), K, M) for k1, s, cl, co in zip(rows[0], rows[1], rows[5], rows[6])]
        want_sn, want_rows = F.summarise(list(zip(rows[0].tolist(), rows[1].tolist(), rows[2].tolist(), rows[5].tolist())), placed, M)
        for name, x, y in zip(NAMES6, got, _columns_of(placed)):
            assert x.dtype == np.uint32 and np.array_equal(x, y), (name, x.tolist(), y.tolist())
        assert sn[F.SN_INDEX["mated"]] == 0 and np.array_equal(sn[:10], want_sn[:10]), (sn.tolist(), want_sn.tolist())
        # five sites: one short, the junction's two mated, the decoy placed and unmated, the random clip unplaced
        assert want_sn.tolist() == [5, 1, 0, 4, 3, 0, 1, 0, 3, 0, 2]
        assert [(r[0], r[1], r[2], r[10], r[12], r[13], r[14]) for r in want_rows if r[12] is not None] == [(0, 405, 1, "BND", 1, 601, 5), (1, 601, 0, "BND", 0, 405, 5)]
        assert ms.shape == (4,) and (ms >= 0.0).all()
        again = h.rows()
        assert all(np.array_equal(x, y) for x, y in zip(rows, again))                   # tdt_clip_rows is what it was
        # a second call, other parameters: the columns follow; a push invalidates them
        sn2, got2, _ = F.far_counter(h, ref, 28, 0)
        assert sn2[F.SN_INDEX["short_consensus"]] == 1 and sn2[F.SN_INDEX["searched"]] == 4 and sn2[F.SN_INDEX["placed"]] == 3
        h.push_host_batch(D.build_batch(_handle_reads(case)[:1]))
        n = ctypes.c_size_t(0)
        assert ctx.lib.tdt_clip_far_rows(h.handle, None, None, None, None, None, None, ctypes.byref(n)) == -1
    finally:
        h.close()
        ref.close()


def test_refused_arguments_leave_the_outputs_untouched(ctx):
    from tiddit_amd import _native, refseq, tiddit_clips
    lib, P = ctx.lib, _native.ptr
    case = _event_case()
    ref = _refseq(case, ctx)
    other = refseq.RefSeq([100, 100, 100], ctx=ctx)                                      # another contig count than the handle's
    h = tiddit_clips.ClipCounter(len(case["lengths"]), 20, 10, capacity=1 << 10, ctx=ctx)
    try:
        k1, side, clen, cons = C.columns(case)
        n = len(k1)
        outs = [np.full(n, 7, dtype=np.uint32) for _ in range(6)]
        ins = [k1, side, clen, cons]
        bad_km = ((15, 2), (29, 2), (20, -1), (20, 13), (0, 0))

        def sites(fn, c, r, nn, i, km, o):
            return fn(c, r, nn, *[P(a) if a is not None else None for a in i], *km, *[P(a) if a is not None else None for a in o])
        for fn in (lib.tdt_clip_far_sites, lib.tdt_clip_far_sites_device):                # (refused before any pointer is followed)
            assert sites(fn, None, ref.handle, n, ins, (20, 2), outs) == -1 and sites(fn, ctx.handle, None, n, ins, (20, 2), outs) == -1
            for k in range(4):
                assert sites(fn, ctx.handle, ref.handle, n, ins[:k] + [None] + ins[k + 1:], (20, 2), outs) == -1
            for k in range(6):
                assert sites(fn, ctx.handle, ref.handle, n, ins, (20, 2), outs[:k] + [None] + outs[k + 1:]) == -1
            assert sites(fn, ctx.handle, ref.handle, 1 << 31, ins, (20, 2), outs) == -1
            assert sites(fn, ctx.handle, ref.handle, 1 << 29, ins, (20, 2), outs) == -3                    # two entries per site: the sort's limit
            for km in bad_km:
                assert sites(fn, ctx.handle, ref.handle, n, ins, km, outs) == -3, km
            assert sites(fn, ctx.handle, ref.handle, 0, [None] * 4, (20, 2), [None] * 6) == 0             # no site: a no-op
        assert all((o == 7).all() for o in outs)
        sn = np.full(11, 7, dtype=np.uint64)
        cnt = ctypes.c_size_t(77)
        ms = np.full(4, 7.0)
        rows = lambda hh, arrays, c: lib.tdt_clip_far_rows(hh, *[P(a) if a is not None else None for a in arrays], c)
        assert lib.tdt_clip_far(None, ref.handle, 20, 2, P(sn)) == -1 and lib.tdt_clip_far(h.handle, None, 20, 2, P(sn)) == -1
        assert lib.tdt_clip_far(h.handle, ref.handle, 20, 2, None) == -1
        assert lib.tdt_clip_far(h.handle, ref.handle, 20, 2, P(sn)) == -1                                  # no finish yet
        assert rows(h.handle, outs, ctypes.byref(cnt)) == -1 and lib.tdt_clip_far_timing(h.handle, P(ms)) == -1
        h.push_host_batch(D.build_batch(_handle_reads(case)))
        assert lib.tdt_clip_far(h.handle, ref.handle, 20, 2, P(sn)) == -1                                  # a push, and still no finish
        h.finish(2)
        assert lib.tdt_clip_far(h.handle, other.handle, 20, 2, P(sn)) == -1                                # another contig count
        for km in bad_km:
            assert lib.tdt_clip_far(h.handle, ref.handle, *km, P(sn)) == -3, km
        assert rows(h.handle, outs, ctypes.byref(cnt)) == -1                                               # a finish, and no search since
        assert lib.tdt_clip_far_timing(h.handle, P(ms)) == -1 and lib.tdt_clip_far_timing(None, P(ms)) == -1
        assert lib.tdt_clip_far_timing(h.handle, None) == -1
        assert (sn == 7).all() and cnt.value == 77 and (ms == 7.0).all() and all((o == 7).all() for o in outs)
        # and the handle still works
        assert lib.tdt_clip_far(h.handle, ref.handle, 20, 2, P(sn)) == 0 and sn.tolist() == [5, 1, 0, 4, 3, 0, 1, 0, 3, 0, 0]
        assert rows(None, outs, ctypes.byref(cnt)) == -1 and rows(h.handle, outs, None) == -1
        for k in range(6):
            assert rows(h.handle, outs[:k] + [None] + outs[k + 1:], ctypes.byref(cnt)) == -1
        cnt = ctypes.c_size_t(4)                                                                           # room for 4 of the 5 rows
        assert rows(h.handle, outs, ctypes.byref(cnt)) == -3 and cnt.value == 4 and all((o == 7).all() for o in outs)
        cnt = ctypes.c_size_t(0)
        assert rows(h.handle, [None] * 6, ctypes.byref(cnt)) == 0 and cnt.value == 5                       # the count alone
        big = [np.full(8, 7, dtype=np.uint32) for _ in range(6)]
        cnt = ctypes.c_size_t(8)
        assert rows(h.handle, big, ctypes.byref(cnt)) == 0 and cnt.value == 5 and all((o[5:] == 7).all() for o in big)
        assert sorted(big[0][:5].tolist()) == [0, 2, 2, 2, 2]
        assert lib.tdt_clip_far_timing(h.handle, P(ms)) == 0 and (ms >= 0.0).all() and (ms != 7.0).all()
        h.reset()
        assert rows(h.handle, big, ctypes.byref(cnt)) == -1
    finally:
        h.close()
        other.close()
        ref.close()


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------------
READ, CLIPS, FAR, ALIGN = 100, "3:20:10", "20:2", "600"
LEN_A, LEN_B, LEN_C = 15000, 10000, 5000
TA, TB = 4000, 7000                            # the sample joins A[... TA] to B[TB + 1 ...]
DA, DB, DC = 3000, 3399, 9000                  # A[DA ... DB] lies a second time behind A[DC]
ME, ME_LEN = 6000, 300                         # a 300-bp element (five copies in the reference) is inserted behind A[ME]
ME_AT = ((0, 1000), (0, 12000), (1, 2000), (1, 8000), (2, 1000))


def _genome():
    a, b, c = C.Seq(C.seeded(LEN_A, 911)), C.Seq(C.seeded(LEN_B, 912)), C.Seq(C.seeded(LEN_C, 913))
    g = (a, b, c)
    me = C.seeded(ME_LEN, 914)
    for t, q in ME_AT:
        g[t].put(q, me)
    # no base of homology at any junction: an aligner clips exactly there
    C._differ(a, TA + 1, b[TB + 1]), C._differ(b, TB, a[TA])
    a.differ(DC + 1, DA), a.differ(DA - 1, DC), a.differ(DB + 1, DC + 1), a.differ(DC, DB)
    C._differ(a, ME + 1, me[0]), C._differ(a, ME, me[-1])
    return g, me


def _sample_reads(g, me):
    """100-bp reads tiled over the junctions' sides, clipped where the sample leaves the reference (30 ... 70 clipped bases on either
    side), and plain reads every 50 bases of every contig"""
    a, b, c = g
    reads = []

    def left(t, end, clip):                     # aligned on contig t up to `end`, then the clip
        m = READ - len(clip)
        reads.append(D.rd(tid=t, pos=end - m, m=m, trail=clip, seq=g[t].get(end - m + 1, end) + clip, flag=D.REV * (len(clip) % 2)))

    def right(t, start, clip):                  # the clip, then aligned on contig t from `start` on
        m = READ - len(clip)
        reads.append(D.rd(tid=t, pos=start - 1, m=m, lead=clip, seq=clip + g[t].get(start, start + m - 1), flag=D.REV * (len(clip) % 2)))
    for k in range(30, 71, 5):
        left(0, TA, b.get(TB + 1, TB + k)), right(1, TB + 1, a.get(TA - k + 1, TA))                  # the translocation, from both sides
        left(0, DC, a.get(DA, DA + k - 1)), right(0, DA, a.get(DC - k + 1, DC))                      # the copy's first junction
        left(0, DB, a.get(DC + 1, DC + k)), right(0, DC + 1, a.get(DB - k + 1, DB))                  # ... and its second
        left(0, ME, me[:k]), right(0, ME + 1, me[-k:])                                               # the element's two ends
    for t, s in enumerate(g):
        n = len(s.b)
        for p in range(1, n - READ, 50):
            reads.append(D.rd(tid=t, pos=p - 1, m=READ, seq=s.get(p, p + READ - 1), flag=D.REV * (p % 100 == 1)))
    return sorted(reads, key=lambda r: (r["tid"], r["pos"]))


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
    d = str(tmp_path_factory.mktemp("clip_far"))
    g, me = _genome()
    contigs = [("chrA", g[0].text()), ("chrB", g[1].text()), ("chrC", g[2].text())]
    fa, bam = os.path.join(d, "ref.fa"), os.path.join(d, "sample.bam")
    open(fa, "wb").write(b"".join(b">" + n.encode() + b"\n" + C.fasta_raw(t) + b"\n" for n, t in contigs))
    w = bamio.BamWriter(bam, [(n, len(t)) for n, t in contigs])
    w._buf += D.build_batch(_sample_reads(g, me)).raw.tobytes()
    w.close()
    paths = {n: os.path.join(d, n) for n in ("clips", "far", "align", "both", "bad")}
    _ok(_job(bam, fa, paths["clips"], TIDDIT_CLIPS=CLIPS))
    r = _ok(_job(bam, fa, paths["far"], TIDDIT_CLIPS=CLIPS, TIDDIT_CLIPS_FAR=FAR))
    return bam, fa, contigs, paths, r


def test_the_file_equals_the_definitions_file_and_names_the_planted_junctions(jobs, tmp_path):
    from tiddit_amd import bamio, refseq, tiddit_clip_far as F, tiddit_clips
    bam, fa, contigs, paths, r = jobs
    sn, keys = {}, []
    rd = bamio.BamReader(bam)
    for b in rd.batches():
        tiddit_clips.keys_of_batch_by_read(b, keys, sn, 20, 10)
    rd.close()
    _, rows = tiddit_clips.summarise(keys, sn, 3)
    host = refseq.HostReference({t: refseq.codes_of_bases(text) for t, (_, text) in enumerate(contigs)})
    K, M = 20, 2
    placed = [F.place_site(host, k1 >> 32, k1 & 0xffffffff, side, clen, cons, K, M) for k1, side, _, _, _, clen, cons, _, _ in rows]
    counts, out = F.summarise([(x[0], x[1], x[2], x[5]) for x in rows], placed, M)
    want = str(tmp_path / "want.clips.far.tab")
    F.write_file(want, counts, out, [n for n, _ in contigs], K, M)
    got = open(paths["far"] + ".clips.far.tab", "rb").read()
    assert got == open(want, "rb").read()
    assert got.startswith(b"# tiddit_amd clips_far v1 seed=16 min_cols=20 max_mismatch=2\nSN\tsites\t8\n")
    # eight sites, all placed; the element's two ends place five times each; the translocation's two on another contig; six rows mated
    assert counts.tolist() == [8, 0, 0, 8, 8, 2, 0, 6, 2, 0, 6]
    table = [l.split("\t") for l in got.decode().split("\n") if l and not l.startswith(("#", "SN"))]
    # CHROM POS SIDE SUPPORT CLEN PCHROM PARTNER STRAND MISMATCH HITS TYPE LEN MATE_CHROM MATE HOM, as the junctions were planted
    assert table == [
        ["chrA", "3000", "L", "9", "28", "chrA", "9000", "+", "0", "1", "DUP", "6001", "chrA", "9000", "0"],
        ["chrA", "3399", "R", "9", "28", "chrA", "9001", "+", "0", "1", "DEL", "5601", "chrA", "9001", "0"],
        ["chrA", "4000", "R", "9", "28", "chrB", "7001", "+", "0", "1", "BND", ".", "chrB", "7001", "0"],
        ["chrA", "6000", "R", "9", "28", "chrA", "1000", "+", "0", "5", "DUP", "5001", ".", ".", "."],
        ["chrA", "6001", "L", "9", "28", "chrA", "1299", "+", "0", "5", "DEL", "4701", ".", ".", "."],
        ["chrA", "9000", "R", "9", "28", "chrA", "3000", "+", "0", "1", "DUP", "6001", "chrA", "3000", "0"],
        ["chrA", "9001", "L", "9", "28", "chrA", "3399", "+", "0", "1", "DEL", "5601", "chrA", "3399", "0"],
        ["chrB", "7001", "L", "9", "28", "chrA", "4000", "+", "0", "1", "BND", ".", "chrA", "4000", "0"]]
    assert [l for l in r.stdout.split("\n") if l.startswith("clips far:")] == [F.summary_line(counts)]


def test_every_other_output_is_what_it_is_with_the_clips_alone(jobs):
    bam, fa, contigs, paths, r = jobs
    alone, far = _files(paths["clips"]), _files(paths["far"])
    assert set(far) - set(alone) == {".clips.far.tab"} and set(alone) <= set(far) and ".clips.tab" in alone and len(alone) >= 5
    assert all(far[k] == alone[k] for k in alone), [k for k in alone if far[k] != alone[k]]


def test_with_the_local_stage_also_set_both_files_are_what_each_is_alone(jobs):
    bam, fa, contigs, paths, r = jobs
    _ok(_job(bam, fa, paths["align"], TIDDIT_CLIPS=CLIPS, TIDDIT_CLIPS_ALIGN=ALIGN))
    _ok(_job(bam, fa, paths["both"], TIDDIT_CLIPS=CLIPS, TIDDIT_CLIPS_ALIGN=ALIGN, TIDDIT_CLIPS_FAR=FAR))
    far, align, both = _files(paths["far"]), _files(paths["align"]), _files(paths["both"])
    assert set(both) == set(far) | set(align) and {".clips.far.tab", ".clips.align.tab"} <= set(both)
    assert all(both[k] == far[k] for k in far) and all(both[k] == align[k] for k in align)


@pytest.mark.parametrize("env,line", [
    ({"TIDDIT_CLIPS_FAR": "1"}, "error, TIDDIT_CLIPS_FAR=1: the switch places the sites of TIDDIT_CLIPS, which is not set"),
    ({"TIDDIT_CLIPS": CLIPS, "TIDDIT_CLIPS_FAR": "15"}, "error, TIDDIT_CLIPS_FAR=15: the minimum consensus columns are 16 ... 28"),
    ({"TIDDIT_CLIPS": CLIPS, "TIDDIT_CLIPS_FAR": "20:13"}, "error, TIDDIT_CLIPS_FAR=20:13: the maximum mismatches are 0 ... 12")],
    ids=["without TIDDIT_CLIPS", "15", "20:13"])
def test_the_switch_without_its_partner_and_bad_values_are_errors(jobs, env, line):
    bam, fa, contigs, paths, r = jobs
    bad = _job(bam, fa, paths["bad"], timeout=120, **env)
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == [line]
    assert not os.path.exists(paths["bad"] + "_tiddit") and not any(os.path.exists(paths["bad"] + s) for s in (".clips.tab", ".clips.far.tab"))
