"""`TIDDIT_CLIPS_VCF` on the GPU: both C entries of the boundary support (``tdt_junction_support`` / ``tdt_junction_support_device``,
csrc/tdt_junction.hip) against the definition of tiddit_amd/tiddit_clip_vcf.py and the literal claims of tests/clip_vcf_cases.py on every
kernel case — equality is exact, these are integers — their refusals, the handle path on a store filled on the device, and the switch end
to end on a generated reference of 25 kb with six planted events, every job a fresh child process under its own time limit.

Every test of this file fails on the parent commit: the entries, the module and the switch do not exist there."""
import hashlib
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import clip_align_cases as C
import clip_cases as D
import clip_vcf_cases as X

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = []                       # the (case, entry) pairs that ran and passed
MIN_Q, MAX_INS = 20, 1000
COLS = ("tid", "pos", "end", "mapq", "flag", "mate_tid", "mate_pos", "tlen", "sa_off")
TYPES = (np.int32, np.int32, np.int32, np.uint8, np.uint16, np.int32, np.int32, np.int32, np.int64)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _columns(case):
    """the nine columns the pack kernel reads, chosen so that it packs exactly the case's (start, end, bits)"""
    rows = [(t, s, e, b) for t, (_, recs) in enumerate(case["contigs"]) for s, e, b in recs]
    tid, start, end, bits = (np.array([r[k] for r in rows], dtype=np.int64).reshape(len(rows)) for k in range(4))
    cols = {"tid": tid, "pos": start, "end": end, "mapq": np.where(bits & X.LOW_Q, 0, 60),
            "flag": (bits & (X.UNMAPPED | X.MATE_UNMAPPED)) | np.where(bits & X.DUPLICATE, 0x400, 0), "mate_tid": np.where(bits & X.DISCORDANT, tid + 1, tid),
            "mate_pos": np.full(len(rows), -1), "tlen": np.zeros(len(rows)), "sa_off": np.where(bits & X.HAS_SA, 0, -1)}
    return {k: np.ascontiguousarray(cols[k], dtype=dt) for k, dt in zip(COLS, TYPES)}


def _store(case, device=False):
    from tiddit_amd import tiddit_region
    lengths = [ln for ln, _ in case["contigs"]]
    cols = _columns(case)
    store = tiddit_region.EvidenceStore("case", ["c%d" % t for t in range(len(lengths))], lengths, MIN_Q, MAX_INS, capacity=max(len(cols["tid"]), 1))
    if len(cols["tid"]) and not device:
        store.add_host_batch(types.SimpleNamespace(**cols))
    elif len(cols["tid"]):
        import torch
        dev = torch.device("cuda", store.ctx.device)
        ten = {k: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).to(dev) for k, v in cols.items()}
        torch.cuda.synchronize(dev)                                     # torch's copies run on its stream, the library on its own
        tid = cols["tid"]
        edges = np.flatnonzero(np.diff(tid)) + 1
        runs = [(int(tid[lo]), int(lo), int(hi)) for lo, hi in zip(np.concatenate([[0], edges]), np.concatenate([edges, [len(tid)]]))]
        store.add_device_batch(types.SimpleNamespace(runs=runs, dev={k: ten[k].data_ptr() for k in COLS}))
        store.ctx.sync()                                                # (the tensors are released after the pack kernel has read them)
    return store


def _device_entry(store, tab, bounds, F):
    """``tdt_junction_support_device`` on torch copies of the boundaries -> (return code, int64[nb][4])"""
    import torch
    from tiddit_amd import _native
    q = np.ascontiguousarray(np.asarray(bounds, dtype=np.int32).reshape(-1, 2))
    dev = torch.device("cuda", store.ctx.device)
    dq = torch.from_numpy(q.reshape(-1).copy() if q.size else np.zeros(2, dtype=np.int32)).to(dev)
    dout = torch.full((max(len(q), 1) * 4,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    rc = store.ctx.lib.tdt_junction_support_device(store.ctx.handle, store.handle, _native.ptr(tab), len(tab), dq.data_ptr(), len(q), F, dout.data_ptr())
    return rc, dout.cpu().numpy().reshape(-1, 4)[:len(q)]


def _definition(case):
    from tiddit_amd import tiddit_clip_vcf as V
    tab, recs = X.table(case), X.records(case)
    out = []
    for row, b in case["boundaries"]:
        o, n, _, _, ln = (int(v) for v in tab[row])
        r = recs[o:o + n]
        out.append(V.boundary_support(zip(r["start"].tolist(), r["end"].tolist(), r["bits"].tolist()), ln, b, case["F"]))
    return out


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("case", X.KERNEL_CASES + [dict(X.SITE_CASE, name="sites: a deletion's two boundaries")], ids=[c["name"] for c in X.KERNEL_CASES] + ["sites: a deletion's two boundaries"])
def test_both_entries_equal_the_definition_and_the_claim(case, entry):
    want = _definition(case)
    assert want == [tuple(e) for e in case["expect"]]
    store = _store(case)
    try:
        tab = X.table(case)
        if not case["span"]:
            assert np.array_equal(store.contig_table(), tab)                     # (the pack kernel's spans are the table's)
        for t in range(len(tab)):
            got = store.records(t)
            o, n = int(tab[t, 0]), int(tab[t, 1])
            assert np.array_equal(got["start"], X.records(case)["start"][o:o + n]) and np.array_equal(got["bits"], X.records(case)["bits"][o:o + n])
        if entry == "host":
            got = store.junction_support(case["boundaries"], case["F"], table=tab)
            assert got.dtype == np.int64 and got.shape == (len(want), 4)
        else:
            rc, got = _device_entry(store, tab, case["boundaries"], case["F"])
            assert rc == 0
        assert [tuple(r) for r in got.tolist()] == want, case.get("claims", case["name"])
        assert store.junction_ms() >= 0.0
    finally:
        store.close()
    PAIRS.append((case["name"], entry))


def test_the_stated_count_of_case_entry_pairs_ran():
    assert X.N_KERNEL_CASES == 30 and len(PAIRS) == len(set(PAIRS)) == 2 * (X.N_KERNEL_CASES + 1)


def test_the_handle_path_on_a_store_filled_on_the_device():
    """``EvidenceStore.junction_support`` with its own table on a store that ``add_device_batch`` filled"""
    case = next(c for c in X.KERNEL_CASES if c["name"] == "search: ranges of 64, 4096 and 5000 records")
    store = _store(case, device=True)
    try:
        assert store.n == 64 + 4096 + 5000
        got = store.junction_support(case["boundaries"], case["F"])
        assert [tuple(r) for r in got.tolist()] == case["expect"]
        assert store.junction_support([], 10).shape == (0, 4)
    finally:
        store.close()


def test_refused_arguments_leave_a_poisoned_output_untouched():
    import torch
    from tiddit_amd import _native
    case = next(c for c in X.KERNEL_CASES if c["name"] == "search: three contigs with an empty one in the middle")
    store = _store(case)
    try:
        ctx, lib, P = store.ctx, store.ctx.lib, _native.ptr
        good = np.ascontiguousarray(store.contig_table())
        q = np.ascontiguousarray(np.array(case["boundaries"], dtype=np.int32))
        nb, n = len(q), len(good)
        out = np.full((nb, 4), -7, dtype=np.int64)
        odd_q = np.zeros(2 * nb + 1, dtype=np.int32)[1:]                          # 4 bytes off an 8-byte boundary
        odd_out = np.zeros(32 * nb + 8, dtype=np.uint8)[4:4 + 32 * nb].view(np.int64)
        assert odd_q.ctypes.data % 8 == 4 and odd_out.ctypes.data % 8 == 4
        outside = good.copy()
        outside[2, 1] = store.n - outside[2, 0] + 1                               # one record past the end of the store
        negative = good.copy()
        negative[1, 4] = -5
        bad_row, neg_row = q.copy(), q.copy()
        bad_row[1, 0], neg_row[2, 0] = n, -1
        H, S = ctx.handle, store.handle
        for args, code in (((None, S, good, n, q, nb, 10, out), -1), ((H, None, good, n, q, nb, 10, out), -1), ((H, S, None, n, q, nb, 10, out), -1),
                           ((H, S, good, n, None, nb, 10, out), -1), ((H, S, good, n, q, nb, 10, None), -1), ((H, S, good, n, odd_q, nb, 10, out), -1),
                           ((H, S, good, n, q, nb, 10, odd_out), -1), ((H, S, good, -1, q, nb, 10, out), -1), ((H, S, good, n, q, 2 ** 31, 10, out), -1),
                           ((H, S, good, n, q, nb, 0, out), -1), ((H, S, good, n, q, nb, X.JS_MAX_FLANK + 1, out), -1), ((H, S, good, n, q, nb, -3, out), -1),
                           ((H, S, outside, n, q, nb, 10, out), -3), ((H, S, negative, n, q, nb, 10, out), -3), ((H, S, good, n, bad_row, nb, 10, out), -3),
                           ((H, S, good, n, neg_row, nb, 10, out), -3), ((H, S, good, 0, q, nb, 10, out), -3),
                           ((H, S, good, n, q, 0, 10, out), 0), ((H, S, None, 0, None, 0, 10, None), 0)):
            a = [P(x) if isinstance(x, np.ndarray) else x for x in args]
            assert lib.tdt_junction_support(*a) == code, (args[3], args[5:7], code)
            assert (out == -7).all() and (odd_out == 0).all()
        with pytest.raises(_native.TdtError) as e:
            store.junction_support(bad_row, 10)
        assert e.value.code == -3 and "boundary 1 names contig 3 of 3" in str(e.value)
        # the device entry: the same refusals before the launch ...
        dev = torch.device("cuda", ctx.device)
        dq = torch.from_numpy(q.reshape(-1).copy()).to(dev)
        dout = torch.full((4 * 4 + 1,), -7, dtype=torch.int64, device=dev)          # (room for the four boundaries below, and a guard word)
        torch.cuda.synchronize(dev)
        Q, O = dq.data_ptr(), dout.data_ptr()
        for args, code in (((None, S, P(good), n, Q, nb, 10, O), -1), ((H, None, P(good), n, Q, nb, 10, O), -1), ((H, S, None, n, Q, nb, 10, O), -1),
                           ((H, S, P(good), n, None, nb, 10, O), -1), ((H, S, P(good), n, Q, nb, 10, None), -1), ((H, S, P(good), n, Q + 4, nb - 1, 10, O), -1),
                           ((H, S, P(good), n, Q, nb, 10, O + 4), -1), ((H, S, P(good), n, Q, nb, 0, O), -1), ((H, S, P(good), n, Q, nb, 1001, O), -1),
                           ((H, S, P(outside), n, Q, nb, 10, O), -3), ((H, S, P(negative), n, Q, nb, 10, O), -3), ((H, S, P(good), n, Q, 0, 10, O), 0)):
            assert lib.tdt_junction_support_device(*args) == code, (args[3], args[5:7], code)
            assert (dout.cpu().numpy() == -7).all()
        # ... and a boundary that names no row, which only the kernel sees: zeros for it, the others counted, the first one named
        dbad = torch.from_numpy(np.array([[0, 150], [3, 150], [2, 150], [-1, 150]], dtype=np.int32).reshape(-1).copy()).to(dev)
        torch.cuda.synchronize(dev)
        assert lib.tdt_junction_support_device(H, S, P(good), n, dbad.data_ptr(), 4, 10, O) == -3
        assert "boundary 1 names contig 3 of 3" in lib.tdt_last_error().decode()
        assert dout.cpu().numpy().tolist() == [2, 2, 2, 0] + [0] * 4 + [3, 3, 3, 0] + [0] * 4 + [-7]
        assert lib.tdt_junction_support(H, S, P(good), n, P(q), nb, 10, P(out)) == 0          # (and the store is still good)
        assert [tuple(r) for r in out.tolist()] == case["expect"]
    finally:
        store.close()


# ---- the switch, end to end ---------------------------------------------------------------------------------------------------------
READ, FLANK = 150, 10
CLIPS, ALIGN, FAR, INS = "3:20:10", "600", "20:2", "20:12:1"
LEN_A, LEN_B = 17000, 8000
HET_A, HET_B = 2000, 2300                      # chrA 2001 ... 2300 deleted on one allele: reads over both breakpoints as well as clipped ones
HOM_A, HOM_B = 5000, 5300                      # chrA 5001 ... 5300 deleted on both: no read crosses either breakpoint
DUP_A, DUP_B = 8000, 8399                      # chrA 8000 ... 8399 twice in tandem, on one allele
TRA_A, TRA_B = 11000, 3000                     # the sample joins chrA[... 11000] to chrB[3001 ...], on one allele
INS_CLOSED = (0, 14000, 60)                    # 60 bases behind chrA 14000, on both alleles
INS_OPEN = (1, 5000, 600)                      # 600 bases behind chrB 5000 (longer than the two flanks reach), on one allele
EVENT_CLIPS = (30, 60, 90, 120)                # the clipped bases of the reads over each side of a DEL / DUP / BND junction
INS_CLIPS = (30, 60, 90, 120, 140, 140, 140)   # ... and of an insertion (three reads reach all 140 columns)
# (contig, b, reads that cross it intact): the twelve boundaries, 0-based, b bases left of the cut
CROSSED = ((0, HET_A, 6), (0, HET_B, 6), (0, HOM_A, 0), (0, HOM_B, 0), (0, DUP_B, 8), (0, DUP_A - 1, 8), (0, TRA_A, 4), (1, TRA_B, 4),
           (0, INS_CLOSED[1], 0), (1, INS_OPEN[1], 5))


def _genome():
    a, b = C.Seq(C.seeded(LEN_A, 941)), C.Seq(C.seeded(LEN_B, 942))
    ins = [C.seeded(INS_CLOSED[2], 943), C.seeded(INS_OPEN[2], 944)]
    for lo, hi in ((HET_A, HET_B), (HOM_A, HOM_B)):                            # no base of homology at any junction: an aligner clips exactly there
        a.differ(lo, hi), a.differ(lo + 1, hi + 1)
    a.differ(DUP_B + 1, DUP_A), a.differ(DUP_A - 1, DUP_B)
    if a[TRA_A + 1] == b[TRA_B + 1]:
        a.put(TRA_A + 1, C.other(b[TRA_B + 1]))
    if a[TRA_A] == b[TRA_B]:
        b.put(TRA_B, C.other(a[TRA_A]))
    for (t, P, _), s in zip((INS_CLOSED, INS_OPEN), ins):
        g = (a, b)[t]
        if g[P + 1] == s[0]:
            g.put(P + 1, C.other(s[0]))
        if g[P] == s[-1]:
            g.put(P, C.other(s[-1]))
    return (a, b), ins


def _sample_reads(g, ins):
    """150-bp reads: over every junction side the clipped ones, clipped where the sample leaves the reference; over every boundary of
    ``CROSSED`` that many plain reads that hold 40 bases or more on both sides; and plain reads every 50 bases of both contigs, except those
    that would hold a boundary in their inside"""
    reads = []

    def left(t, end, clip):                     # aligned up to `end`, then the clip
        m = READ - len(clip)
        reads.append(D.rd(tid=t, pos=end - m, m=m, trail=clip, seq=g[t].get(end - m + 1, end) + clip, flag=D.REV * (len(reads) % 2)))

    def right(t, start, clip):                  # the clip, then aligned from `start` on
        m = READ - len(clip)
        reads.append(D.rd(tid=t, pos=start - 1, m=m, lead=clip, seq=clip + g[t].get(start, start + m - 1), flag=D.REV * (len(reads) % 2)))
    A, B = g
    for k in EVENT_CLIPS:
        for lo, hi in ((HET_A, HET_B), (HOM_A, HOM_B)):
            left(0, lo, A.get(hi + 1, hi + k)), right(0, hi + 1, A.get(lo - k + 1, lo))
        left(0, DUP_B, A.get(DUP_A, DUP_A + k - 1)), right(0, DUP_A, A.get(DUP_B - k + 1, DUP_B))
        left(0, TRA_A, B.get(TRA_B + 1, TRA_B + k)), right(1, TRA_B + 1, A.get(TRA_A - k + 1, TRA_A))
    for (t, P, _), s in zip((INS_CLOSED, INS_OPEN), ins):
        for k in INS_CLIPS:
            left(t, P, (s + g[t].get(P + 1, P + READ))[:k]), right(t, P + 1, (g[t].get(P - READ, P) + s)[-k:])
    for t, b, n in CROSSED:
        for j in range(n):
            p = b - 75 + 5 * j                                                  # 0-based start: 40 ... 75 bases left of the cut, the rest right of it
            reads.append(D.rd(tid=t, pos=p, m=READ, seq=g[t].get(p + 1, p + READ)))
    for t, s in enumerate(g):
        for p in range(0, len(s.b) - READ, 50):
            if not any(bt == t and p < b < p + READ for bt, b, _ in CROSSED):
                reads.append(D.rd(tid=t, pos=p, m=READ, seq=s.get(p + 1, p + READ), flag=D.REV * (p % 100 == 0)))
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


FOUR = {"TIDDIT_CLIPS": CLIPS, "TIDDIT_CLIPS_ALIGN": ALIGN, "TIDDIT_CLIPS_FAR": FAR, "TIDDIT_CLIPS_INS": INS}


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """the generated reference as a FASTA, the sample's reads as a sorted BAM; two jobs, each checked before the next is started"""
    from tiddit_amd import bamio
    d = str(tmp_path_factory.mktemp("clip_vcf"))
    g, ins = _genome()
    contigs = [("chrA", g[0].text()), ("chrB", g[1].text())]
    fa, bam = os.path.join(d, "ref.fa"), os.path.join(d, "sample.bam")
    open(fa, "wb").write(b"".join(b">" + n.encode() + b"\n" + C.fasta_raw(t) + b"\n" for n, t in contigs))
    w = bamio.BamWriter(bam, [(n, len(t)) for n, t in contigs])
    w._buf += D.build_batch(_sample_reads(g, ins)).raw.tobytes()
    w.close()
    paths = {n: os.path.join(d, n) for n in ("four", "vcf", "bad", "ranks")}
    _ok(_job(bam, fa, paths["four"], **FOUR))
    r = _ok(_job(bam, fa, paths["vcf"], TIDDIT_CLIPS_VCF=str(FLANK), **FOUR))
    return bam, fa, contigs, ins, paths, r


def _definition_file(bam, contigs, path):
    """``{o}.clips.vcf`` from the definitions alone: the host reader's batches through tiddit_clips, the three stages' definitions, and the
    records of a store built from the file -> the counters"""
    from tiddit_amd import bamio, refseq, tiddit_clip_align as A, tiddit_clip_far as Fa, tiddit_clip_ins as I, tiddit_clip_vcf as V, tiddit_clips, tiddit_region
    names, lengths = [n for n, _ in contigs], [len(t) for _, t in contigs]
    sn, keys, events, ext_keys, ext_sn = {}, [], [], [], {}
    rd = bamio.BamReader(bam)
    for b in rd.batches():
        tiddit_clips.keys_of_batch_by_read(b, keys, sn, 20, 10)
        I.events_of_batch_by_read(b, events, ext_keys, ext_sn, 20, 10)
    rd.close()
    _, rows = tiddit_clips.summarise(keys, sn, 3)
    host = refseq.HostReference({t: refseq.codes_of_bases(text) for t, (_, text) in enumerate(contigs)})
    sites = [(x[0], x[1], x[2], x[5]) for x in rows]
    placed = [A.place_site(host, k1 >> 32, k1 & 0xffffffff, side, clen, cons, 600, 20, 2) for k1, side, _, _, _, clen, cons, _, _ in rows]
    _, align_rows = A.summarise(sites, placed, 2)
    placed = [Fa.place_site(host, k1 >> 32, k1 & 0xffffffff, side, clen, cons, 20, 2) for k1, side, _, _, _, clen, cons, _, _ in rows]
    _, far_rows = Fa.summarise(sites, placed, 2)
    _, isites, pairs = I.summarise(events, ext_sn, 3, 20, 12, 1)
    k1, _, eclen, cons5 = I.site_columns(isites)
    cols, seq10 = I.pair_columns(pairs)
    ins_rows = I.file_rows(k1, [s[2] for s in isites], eclen, cons5, cols, seq10)
    store = tiddit_region.build_store(bam, 5, 100000)
    try:
        recs = [store.records(t) for t in range(len(names))]
    finally:
        store.close()
    of = lambda t: zip(recs[t]["start"].tolist(), recs[t]["end"].tolist(), recs[t]["bits"].tolist())
    parts = V.header_parts({"SQ": [{"SN": n, "LN": ln} for n, ln in zip(names, lengths)]}, "sample", "3.9.5")
    return V.definition_file(path, parts, names, lengths, FLANK, of, align_rows, far_rows, ins_rows)


def _strip(data):
    return [l for l in data.decode().split("\n") if not l.startswith("##TIDDITcmd=")]


def test_the_file_equals_the_definitions_file_and_names_the_six_events(jobs, tmp_path):
    from tiddit_amd import tiddit_clip_vcf as V
    bam, fa, contigs, ins, paths, r = jobs
    want = str(tmp_path / "want.clips.vcf")
    counts = _definition_file(bam, contigs, want)
    got = open(paths["vcf"] + ".clips.vcf", "rb").read()
    assert _strip(got) == _strip(open(want, "rb").read())
    assert sum(l.startswith(b"##TIDDITcmd=") for l in got.split(b"\n")) == 1
    assert counts == {"junctions": 4, "both_sources": 3, "sources_disagree": 0, "one_sided": 0, "not_mutual": 0, "inv_rows": 0, "ins_rows": 2, "ins_explained": 0,
                      "records": 7, "ambiguous": 0}
    body = [l.split("\t") for l in got.decode().split("\n") if l and not l.startswith("#")]
    info = [dict(kv.split("=") for kv in l[7].split(";")) for l in body]
    # CHROM POS ID ALT FILTER and the genotype, as the events were planted
    assert [[l[0], l[1], l[2], l[4], l[6], l[9].split(":")[0]] for l in body] == [
        ["chrA", "2000", "CLIP_1", "<DEL>", "PASS", "0/1"], ["chrA", "5000", "CLIP_2", "<DEL>", "PASS", "1/1"], ["chrA", "7999", "CLIP_3", "<DUP>", "PASS", "0/1"],
        ["chrA", "11000", "CLIP_4_1", "N[chrB:3001[", "PASS", "0/1"], ["chrA", "14000", "CLIP_5", "<INS>", "PASS", "1/1"],
        ["chrB", "3001", "CLIP_4_2", "]chrA:11000]N", "PASS", "0/1"], ["chrB", "5000", "CLIP_6", "<INS>", "PASS", "0/1"]]
    assert [(i.get("END"), i.get("SVLEN"), i["SRC"]) for i in info] == [("2300", "-300", "align,far"), ("5300", "-300", "align,far"), ("8399", "400", "align,far"),
                                                                       (None, None, "far"), ("14000", "60", "ins"), (None, None, "far"), ("5000", None, "ins")]
    assert info[4]["SVINSSEQ"] == ins[0] and info[6]["LEFT_SVINSSEQ"] == ins[1][:140] and info[6]["RIGHT_SVINSSEQ"] == ins[1][-140:]
    # RV and RR as planted: four (seven) clipped reads per site, and the reads of CROSSED over the two boundaries
    assert [l[9].split(":")[1:3] for l in body] == [["4,4", "6,6"], ["4,4", "0,0"], ["4,4", "8,8"], ["4,4", "4,4"], ["7,7", "0,0"], ["4,4", "4,4"], ["7,7", "5,5"]]
    assert [l for l in r.stdout.split("\n") if l.startswith("clips vcf:")] == [V.summary_line(counts)]


def test_every_other_output_is_what_it_is_without_the_switch(jobs):
    bam, fa, contigs, ins, paths, r = jobs
    four, vcf = _files(paths["four"]), _files(paths["vcf"])
    assert set(vcf) - set(four) == {".clips.vcf"} and set(four) <= set(vcf) and len(four) >= 8
    assert {".clips.tab", ".clips.align.tab", ".clips.far.tab", ".clips.ins.tab"} <= set(four)
    assert all(vcf[k] == four[k] for k in four), [k for k in four if vcf[k] != four[k]]


@pytest.mark.parametrize("env,line", [
    ({"TIDDIT_CLIPS_VCF": "1"}, "error, TIDDIT_CLIPS_VCF=1: the switch joins the rows of TIDDIT_CLIPS, which is not set"),
    ({"TIDDIT_CLIPS": CLIPS, "TIDDIT_CLIPS_VCF": "1"}, "error, TIDDIT_CLIPS_VCF=1: the switch joins the rows of TIDDIT_CLIPS_ALIGN, TIDDIT_CLIPS_FAR and TIDDIT_CLIPS_INS, "
                                                      "none of which is set"),
    (dict(FOUR, TIDDIT_CLIPS_VCF="0"), "error, TIDDIT_CLIPS_VCF=0: the switch is 1 or F (the flank a read covers on both sides of a breakpoint, 2 ... 1000; 1 means 10)"),
    (dict(FOUR, TIDDIT_CLIPS_VCF="1001"), "error, TIDDIT_CLIPS_VCF=1001: the flank is 2 ... 1000 (1 means 10)"),
    (dict(FOUR, TIDDIT_CLIPS_VCF="yes"), "error, TIDDIT_CLIPS_VCF=yes: the switch is 1 or F (the flank a read covers on both sides of a breakpoint, 2 ... 1000; 1 means 10)")],
    ids=["without TIDDIT_CLIPS", "without a stage", "0", "1001", "yes"])
def test_the_switch_without_its_partners_and_bad_values_are_errors(jobs, env, line):
    bam, fa, contigs, ins, paths, r = jobs
    bad = _job(bam, fa, paths["bad"], timeout=120, **env)
    assert bad.returncode == 1
    assert [l for l in bad.stdout.split("\n") if l.startswith("error")] == [line]
    assert not os.path.exists(paths["bad"] + "_tiddit") and not any(os.path.exists(paths["bad"] + s) for s in (".clips.tab", ".clips.vcf"))


def test_n_ranks_refuse_the_switch_and_write_nothing(jobs):
    """every rank ends with the refusal of TIDDIT_CLIPS before the first collective and no file is written"""
    bam, fa, contigs, ins, paths, r = jobs
    res = _job(bam, fa, paths["ranks"], timeout=120, TIDDIT_CLIPS_VCF="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29554",
               TIDDIT_DIST_BACKEND="gloo", TIDDIT_FORCE_DIST="1", **FOUR)
    assert res.returncode == 1, (res.returncode, res.stdout[-1000:], res.stderr[-2000:])
    errors = [l for l in res.stdout.split("\n") if l.startswith("error")]
    assert len(errors) == 1 and errors[0].startswith("error, TIDDIT_CLIPS is a one-process switch")
    assert not os.path.exists(paths["ranks"] + "_tiddit") and not os.path.exists(paths["ranks"] + ".clips.vcf")
