"""`TIDDIT_CLIPS_ALIGN` on the GPU: the kernel (csrc/tdt_clip_align.hip) on every aimed case of tests/clip_align_cases.py through both
entries — ``tdt_clip_align_sites`` on host columns, ``tdt_clip_align_sites_device`` on the same columns in caller-owned device memory
with poisoned, padded outputs — against the definition (which tests/test_clip_align_refs_cpu.py pins to the restatement and to the
cases' claims), exactly; one site with a window of 2^20 against the restatement; through the clip counter's handle (push, finish,
``tdt_clip_align`` on the rows where they lie, ``tdt_clip_align_rows``); the C-ABI refusals; and the switch end to end on a generated
reference of 23 kb with a planted deletion, tandem duplication and inversion, every job a fresh child process under its own time limit
(the first job that fails ends the fixture: nothing more is started behind a crash, a time-out or a GPU error).

Every test of this file fails on the parent commit: the module, the symbols and the switch do not exist there."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import clip_align_cases as C
import clip_cases as D

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = []                       # the (case, entry) pairs that ran and passed
POISON, PADDING = 0x5a, 16
NAMES5 = ("status", "PARTNER", "strand", "mismatches", "HITS")


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
    return tuple(np.array([p[k] for p in placed], dtype=np.uint32) for k in range(5))


def _sites_device(ctx, ref, case):
    """the device entry on torch-owned memory: the outputs are PADDING entries longer than the sites and filled with POISON"""
    import torch
    cols = C.columns(case)
    n = len(cols[0])
    as_bytes = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    ins = [as_bytes(a) for a in cols]
    outs = [torch.full(((n + PADDING) * 4,), POISON, dtype=torch.uint8).cuda() for _ in range(5)]
    torch.cuda.synchronize()
    rc = ctx.lib.tdt_clip_align_sites_device(ctx.handle, ref.handle, n, *[ctypes.c_void_p(t.data_ptr()) for t in ins], case["W"], case["K"], case["M"],
                                             *[ctypes.c_void_p(t.data_ptr()) for t in outs])
    assert rc == 0, rc
    got = [t.cpu().numpy().view(np.uint32) for t in outs]
    assert all((g[n:] == 0x5a5a5a5a).all() for g in got)                       # nothing behind the last site is written
    return tuple(g[:n].copy() for g in got)


@pytest.mark.parametrize("entry", ["sites", "sites_device"])
@pytest.mark.parametrize("case", C.CASES, ids=[c["name"] for c in C.CASES])
def test_both_entries_equal_the_definition(case, entry, wanted, ctx):
    from tiddit_amd import tiddit_clip_align as A
    ref = _refseq(case, ctx)
    try:
        got = A.align_sites(ref, *C.columns(case), case["W"], case["K"], case["M"]) if entry == "sites" else _sites_device(ctx, ref, case)
    finally:
        ref.close()
    want = _columns_of(wanted[case["name"]][0])
    for name, x, y in zip(NAMES5, got, want):
        assert x.dtype == np.uint32 and x.shape == y.shape and np.array_equal(x, y), (case["name"], name, np.flatnonzero(x != y)[:8].tolist())
    PAIRS.append((case["name"], entry))


def test_the_stated_count_of_case_entry_pairs_ran():
    assert len(C.CASES) == C.N_CASES == 32
    assert len(set(PAIRS)) == 2 * 32, len(set(PAIRS))


def test_a_window_of_2_to_the_20_equals_the_restatement(ctx):
    from test_clip_align_refs_cpu import restate_rows, restate_sites
    from tiddit_amd import tiddit_clip_align as A
    case = C.big_case()
    want = restate_sites(case)
    assert C.agrees_with_claim(case, want, restate_rows(case, want)[1]) is None
    ref = _refseq(case, ctx)
    try:
        got = A.align_sites(ref, *C.columns(case), case["W"], case["K"], case["M"])
    finally:
        ref.close()
    assert [tuple(int(g[0]) for g in got)] == want


# ---- through the handle -------------------------------------------------------------------------------------------------------------
def _event_case():
    return next(c for c in C.CASES if c["name"] == "events: a 200-bp deletion with 5 bases of microhomology")


def _handle_reads(case):
    """clipped reads over the case's two junction sites, their clips cut from the case's reference where its sites say the clipped bases
    lie; a site whose clips are too short to be searched; a site whose clips are random"""
    g = C.Seq(case["contigs"][1])
    r_site, l_site = case["sites"]
    reads = []
    for k in (30, 34, 41):
        q = r_site["claim"]["partner"]
        reads.append(D.rd(tid=1, pos=r_site["P"] - 40, m=40, trail=g.get(q, q + k - 1), flag=D.REV * (k == 34)))
        q = l_site["claim"]["partner"]
        reads.append(D.rd(tid=1, pos=l_site["P"] - 1, m=40, lead=g.get(q - k + 1, q)))
    reads += [D.rd(tid=1, pos=900, m=30, trail=g.get(1000, 1011)) for _ in range(3)]                # CLEN 12 < K
    reads += [D.rd(tid=1, pos=100, m=30, trail=C.seeded(30, 9)) for _ in range(2)]                  # nothing like it within W
    reads += [D.rd(tid=0, pos=2, m=20, trail=case["contigs"][0][25:37]) for _ in range(2)]          # on the short contig in front
    return reads


def test_the_handle_aligns_the_rows_of_its_finish_where_they_lie(ctx):
    from tiddit_amd import tiddit_clip_align as A, tiddit_clips
    case = _event_case()
    W, K, M = 300, 20, 2
    ref = _refseq(case, ctx)
    h = tiddit_clips.ClipCounter(len(case["lengths"]), 20, 10, capacity=1 << 10, ctx=ctx)
    try:
        h.push_host_batch(D.build_batch(_handle_reads(case)))
        counts = h.finish(2)
        rows = h.rows()
        assert len(rows[0]) == 5 == int(counts[D.SN.index("reported_sites")])
        sn, got, ms = A.align_counter(h, ref, W, K, M)
        host = C.host_reference(case)
        placed = [A.place_site(host, int(k1) >> 32, int(k1) & 0xffffffff, int(s), int(cl), int(co), W, K, M) for k1, s, cl, co in zip(rows[0], rows[1], rows[5], rows[6])]
        want_sn, want_rows = A.summarise(list(zip(rows[0].tolist(), rows[1].tolist(), rows[2].tolist(), rows[5].tolist())), placed, M)
        for name, x, y in zip(NAMES5, got, _columns_of(placed)):
            assert x.dtype == np.uint32 and np.array_equal(x, y), (name, x.tolist(), y.tolist())
        assert sn[A.SN_INDEX["mated"]] == 0 and np.array_equal(sn[:11], want_sn[:11]), (sn.tolist(), want_sn.tolist())
        assert want_sn.tolist() == [5, 2, 0, 3, 2, 0, 1, 0, 2, 0, 0, 2]                 # two short, the pair of the deletion mated, the random clip unaligned
        assert [(r[1], r[2], r[9], r[10], r[11], r[12]) for r in want_rows if r[9]] == [(405, 1, "DEL", 200, 601, 5), (601, 0, "DEL", 200, 405, 5)]
        assert ms >= 0.0
        again = h.rows()
        assert all(np.array_equal(x, y) for x, y in zip(rows, again))                   # tdt_clip_rows is what it was
        # a second call, other parameters: the columns follow; a push invalidates them
        sn2, got2, _ = A.align_counter(h, ref, 100, 12, 0)
        assert sn2[A.SN_INDEX["short_consensus"]] == 0 and sn2[A.SN_INDEX["searched"]] == 5 and sn2[A.SN_INDEX["aligned"]] == 2
        h.push_host_batch(D.build_batch(_handle_reads(case)[:1]))
        n = ctypes.c_size_t(0)
        assert ctx.lib.tdt_clip_align_rows(h.handle, None, None, None, None, None, ctypes.byref(n)) == -1
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
        outs = [np.full(n, 7, dtype=np.uint32) for _ in range(5)]
        ins = [k1, side, clen, cons]

        def sites(fn, c, r, nn, i, wkm, o):
            return fn(c, r, nn, *[P(a) if a is not None else None for a in i], *wkm, *[P(a) if a is not None else None for a in o])
        for fn in (lib.tdt_clip_align_sites, lib.tdt_clip_align_sites_device):            # (refused before any pointer is followed)
            assert sites(fn, None, ref.handle, n, ins, (300, 20, 2), outs) == -1 and sites(fn, ctx.handle, None, n, ins, (300, 20, 2), outs) == -1
            for k in range(4):
                assert sites(fn, ctx.handle, ref.handle, n, ins[:k] + [None] + ins[k + 1:], (300, 20, 2), outs) == -1
            for k in range(5):
                assert sites(fn, ctx.handle, ref.handle, n, ins, (300, 20, 2), outs[:k] + [None] + outs[k + 1:]) == -1
            assert sites(fn, ctx.handle, ref.handle, 1 << 31, ins, (300, 20, 2), outs) == -1
            for wkm in ((0, 20, 2), ((1 << 20) + 1, 20, 2), (300, 0, 2), (300, 29, 2), (300, 20, -1), (300, 20, 28)):
                assert sites(fn, ctx.handle, ref.handle, n, ins, wkm, outs) == -3, wkm
            assert sites(fn, ctx.handle, ref.handle, 0, [None] * 4, (300, 20, 2), [None] * 5) == 0        # no site: a no-op
        assert all((o == 7).all() for o in outs)
        sn = np.full(12, 7, dtype=np.uint64)
        cnt = ctypes.c_size_t(77)
        ms = ctypes.c_double(7.0)
        rows = lambda hh, arrays, c: lib.tdt_clip_align_rows(hh, *[P(a) if a is not None else None for a in arrays], c)
        assert lib.tdt_clip_align(None, ref.handle, 300, 20, 2, P(sn)) == -1 and lib.tdt_clip_align(h.handle, None, 300, 20, 2, P(sn)) == -1
        assert lib.tdt_clip_align(h.handle, ref.handle, 300, 20, 2, None) == -1
        assert lib.tdt_clip_align(h.handle, ref.handle, 300, 20, 2, P(sn)) == -1                           # no finish yet
        assert rows(h.handle, outs, ctypes.byref(cnt)) == -1 and lib.tdt_clip_align_timing(h.handle, ctypes.byref(ms)) == -1
        h.push_host_batch(D.build_batch(_handle_reads(case)))
        assert lib.tdt_clip_align(h.handle, ref.handle, 300, 20, 2, P(sn)) == -1                           # a push, and still no finish
        h.finish(2)
        assert lib.tdt_clip_align(h.handle, other.handle, 300, 20, 2, P(sn)) == -1                         # another contig count
        for wkm in ((0, 20, 2), ((1 << 20) + 1, 20, 2), (300, 0, 2), (300, 29, 2), (300, 20, -1), (300, 20, 28)):
            assert lib.tdt_clip_align(h.handle, ref.handle, *wkm, P(sn)) == -3, wkm
        assert rows(h.handle, outs, ctypes.byref(cnt)) == -1                                               # a finish, and no align since
        assert lib.tdt_clip_align_timing(h.handle, ctypes.byref(ms)) == -1 and lib.tdt_clip_align_timing(None, ctypes.byref(ms)) == -1
        assert (sn == 7).all() and cnt.value == 77 and ms.value == 7.0 and all((o == 7).all() for o in outs)
        # and the handle still works
        assert lib.tdt_clip_align(h.handle, ref.handle, 300, 20, 2, P(sn)) == 0 and sn.tolist() == [5, 2, 0, 3, 2, 0, 1, 0, 2, 0, 0, 0]
        assert rows(None, outs, ctypes.byref(cnt)) == -1 and rows(h.handle, outs, None) == -1
        for k in range(5):
            assert rows(h.handle, outs[:k] + [None] + outs[k + 1:], ctypes.byref(cnt)) == -1
        cnt = ctypes.c_size_t(4)                                                                           # room for 4 of the 5 rows
        assert rows(h.handle, outs, ctypes.byref(cnt)) == -3 and cnt.value == 4 and all((o == 7).all() for o in outs)
        cnt = ctypes.c_size_t(0)
        assert rows(h.handle, [None] * 5, ctypes.byref(cnt)) == 0 and cnt.value == 5                       # the count alone
        big = [np.full(8, 7, dtype=np.uint32) for _ in range(5)]
        cnt = ctypes.c_size_t(8)
        assert rows(h.handle, big, ctypes.byref(cnt)) == 0 and cnt.value == 5 and all((o[5:] == 7).all() for o in big)
        assert sorted(big[0][:5].tolist()) == [0, 0, 2, 2, 2]
        assert lib.tdt_clip_align_timing(h.handle, ctypes.byref(ms)) == 0 and ms.value >= 0.0 and ms.value != 7.0
        h.reset()
        assert rows(h.handle, big, ctypes.byref(cnt)) == -1
    finally:
        h.close()
        other.close()
        ref.close()


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------------
READ, CLIPS, ALIGN = 100, "3:20:10", "600"
DEL_A, DEL_B = 3000, 3300                      # bases 3001 ... 3300 are deleted
DUP_A, DUP_B = 8000, 8399                      # bases 8000 ... 8399 are there twice
INV_A, INV_B = 13000, 13499                    # bases 13000 ... 13499 are inverted


def _genome():
    g = C.Seq(C.seeded(20000, 901))
    g.differ(DEL_A, DEL_B), g.differ(DEL_A + 1, DEL_B + 1)                 # no base of homology at any junction: an aligner clips exactly there
    g.differ(DUP_B + 1, DUP_A), g.differ(DUP_A - 1, DUP_B)
    if g[INV_A] == C.rc(g[INV_B]):
        g.put(INV_A, C.other(g[INV_A]))
    return g


def _sample_reads(g):
    """100-bp reads tiled over the six junction sides, clipped where the sample leaves the reference (the longer part aligned is not asked
    for: 30 ... 70 clipped bases on either side), and plain reads every 50 bases"""
    reads = []

    def left(end, clip):                        # aligned up to `end`, then the clip
        m = READ - len(clip)
        reads.append(D.rd(tid=0, pos=end - m, m=m, trail=clip, seq=g.get(end - m + 1, end) + clip, flag=D.REV * (len(clip) % 2)))

    def right(start, clip):                     # the clip, then aligned from `start` on
        m = READ - len(clip)
        reads.append(D.rd(tid=0, pos=start - 1, m=m, lead=clip, seq=clip + g.get(start, start + m - 1), flag=D.REV * (len(clip) % 2)))
    for k in range(30, 71, 5):
        left(DEL_A, g.get(DEL_B + 1, DEL_B + k)), right(DEL_B + 1, g.get(DEL_A - k + 1, DEL_A))
        left(DUP_B, g.get(DUP_A, DUP_A + k - 1)), right(DUP_A, g.get(DUP_B - k + 1, DUP_B))
        left(INV_A - 1, C.rc(g.get(INV_B - k + 1, INV_B))), right(INV_B + 1, C.rc(g.get(INV_A, INV_A + k - 1)))
    for p in range(1, 20000 - READ, 50):
        reads.append(D.rd(tid=0, pos=p - 1, m=READ, seq=g.get(p, p + READ - 1), flag=D.REV * (p % 100 == 1)))
    reads += [D.rd(tid=1, pos=p, m=READ, seq=C.seeded(3000, 902)[p:p + READ]) for p in range(0, 2900, 100)]
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
    """the generated reference as a FASTA, the sample's reads as a sorted BAM; two jobs, each checked before the next is started"""
    from tiddit_amd import bamio
    d = str(tmp_path_factory.mktemp("clip_align"))
    g = _genome()
    contigs = [("chrA", g.text()), ("chrB", C.seeded(3000, 902))]
    fa, bam = os.path.join(d, "ref.fa"), os.path.join(d, "sample.bam")
    open(fa, "wb").write(b"".join(b">" + n.encode() + b"\n" + C.fasta_raw(t) + b"\n" for n, t in contigs))
    w = bamio.BamWriter(bam, [(n, len(t)) for n, t in contigs])
    w._buf += D.build_batch(_sample_reads(g)).raw.tobytes()
    w.close()
    paths = {n: os.path.join(d, n) for n in ("clips", "align", "bad")}
    _ok(_job(bam, fa, paths["clips"], TIDDIT_CLIPS=CLIPS))
    r = _ok(_job(bam, fa, paths["align"], TIDDIT_CLIPS=CLIPS, TIDDIT_CLIPS_ALIGN=ALIGN))
    return bam, fa, contigs, paths, r


def test_the_file_equals_the_definitions_file_and_names_the_three_events(jobs, tmp_path):
    from tiddit_amd import bamio, refseq, tiddit_clip_align as A, tiddit_clips
    bam, fa, contigs, paths, r = jobs
    sn, keys = {}, []
    rd = bamio.BamReader(bam)
    for b in rd.batches():
        tiddit_clips.keys_of_batch_by_read(b, keys, sn, 20, 10)
    rd.close()
    _, rows = tiddit_clips.summarise(keys, sn, 3)
    host = refseq.HostReference({t: refseq.codes_of_bases(text) for t, (_, text) in enumerate(contigs)})
    W, K, M = 600, 20, 2
    placed = [A.place_site(host, k1 >> 32, k1 & 0xffffffff, side, clen, cons, W, K, M) for k1, side, _, _, _, clen, cons, _, _ in rows]
    counts, out = A.summarise([(x[0], x[1], x[2], x[5]) for x in rows], placed, M)
    want = str(tmp_path / "want.clips.align.tab")
    A.write_file(want, counts, out, [n for n, _ in contigs], W, K, M)
    got = open(paths["align"] + ".clips.align.tab", "rb").read()
    assert got == open(want, "rb").read()
    assert got.startswith(b"# tiddit_amd clips_align v1 window=600 min_cols=20 max_mismatch=2\nSN\tsites\t6\n")
    assert counts.tolist() == [6, 0, 0, 6, 6, 0, 0, 0, 2, 2, 2, 4]
    table = [l.split("\t") for l in got.decode().split("\n") if l and not l.startswith(("#", "SN"))]
    # POS SIDE SUPPORT CLEN PARTNER STRAND MISMATCH HITS TYPE LEN MATE HOM, as the events were planted
    assert [l[1:] for l in table] == [
        ["3000", "R", "9", "28", "3301", "+", "0", "1", "DEL", "300", "3301", "0"], ["3301", "L", "9", "28", "3000", "+", "0", "1", "DEL", "300", "3000", "0"],
        ["8000", "L", "9", "28", "8399", "+", "0", "1", "DUP", "400", "8399", "0"], ["8399", "R", "9", "28", "8000", "+", "0", "1", "DUP", "400", "8000", "0"],
        ["12999", "R", "9", "28", "13499", "-", "0", "1", "INV", "500", ".", "."], ["13500", "L", "9", "28", "13000", "-", "0", "1", "INV", "500", ".", "."]]
    assert all(l[0] == "chrA" for l in table)
    assert [l for l in r.stdout.split("\n") if l.startswith("clips align:")] == [A.summary_line(counts)]


def test_every_other_output_is_what_it_is_with_the_clips_alone(jobs):
    bam, fa, contigs, paths, r = jobs
    alone, align = _files(paths["clips"]), _files(paths["align"])
    assert set(align) - set(alone) == {".clips.align.tab"} and set(alone) <= set(align) and ".clips.tab" in alone and len(alone) >= 5
    assert all(align[k] == alone[k] for k in alone), [k for k in alone if align[k] != alone[k]]


@pytest.mark.parametrize("env,line", [
    ({"TIDDIT_CLIPS_ALIGN": "1"}, "error, TIDDIT_CLIPS_ALIGN=1: the switch realigns the sites of TIDDIT_CLIPS, which is not set"),
    ({"TIDDIT_CLIPS": CLIPS, "TIDDIT_CLIPS_ALIGN": "0"}, "error, TIDDIT_CLIPS_ALIGN=0: the window is 1 ... 2^20"),
    ({"TIDDIT_CLIPS": CLIPS, "TIDDIT_CLIPS_ALIGN": "5:40"}, "error, TIDDIT_CLIPS_ALIGN=5:40: the minimum consensus columns are 1 ... 28")],
    ids=["without TIDDIT_CLIPS", "0", "5:40"])
def test_the_switch_without_its_partner_and_bad_values_are_errors(jobs, env, line):
    bam, fa, contigs, paths, r = jobs
    bad = _job(bam, fa, paths["bad"], timeout=120, **env)
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == [line]
    assert not os.path.exists(paths["bad"] + "_tiddit") and not any(os.path.exists(paths["bad"] + s) for s in (".clips.tab", ".clips.align.tab"))
