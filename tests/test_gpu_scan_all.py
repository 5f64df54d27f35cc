"""The ``--sv`` scan with EVERY consumer on one pass — what production runs and no other module does: each other ``test_gpu_*.py`` attaches
one consumer to a batch and strips every other switch from its jobs.

Part A runs ``tiddit_signal._scan`` itself, in process, on the file of tests/scan_all_cases.py (something in every 256 KiB of it for every
consumer; every expectation from the definitions over the host reader's batches): all eleven consumers attached at 64-KiB spans — dozens of
batches, records straddling every span, the three pinned result slots, the row thread a batch behind, the key stores' reserve -> ask ->
grow with a span inflating ahead and four keyed consumers on one stream (the STR counter with a column the others do not need, ``end``,
and its counter left in a tap, not in a module global), ONE resident reference shared by the left-normalisation, the SNV
counter and the clip placements —, and behind that scan the clip chain on the live objects: ``tiddit_clips.main`` with the align, far, ins
and mei stages on the counter where its rows lie, then ``tiddit_clip_vcf.main`` on ``tiddit_variant.LIVE_STORE`` in place, every row and
every file against the definitions', and ``tiddit_str.main`` on the live STR counter, its ``.str.tab`` byte for byte the definitions'.
The same at 1-MiB spans and at the default chunk, every consumer alone against the all-on run, the
statistics pass's carried batches replayed to every consumer (with and without a usable second coverage column), the six stores grown
mid-scan from room for 64 items, host ingest for the four keyed consumers together, and an allocation refused mid-scan through the
library's own hook.  Every comparison is exact.  tests/test_gpu_scan_random.py runs the same pass, with this module's ``_scan``, ``_collect``
and comparison, over the random legal records of tests/scan_random_cases.py.

Part B runs `tiddit --sv` on the sv_e2e_small fixture as fresh child processes, each under its own time limit and checked before the next
is started: one job per switch family, then every switch in ONE job — at the default chunk and at 4-MiB spans — whose files must be the
owning family job's, byte for byte.  What those files must contain is pinned by each family's own module; this part shows that company
changes nothing."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import scan_all_cases as C
from sv_e2e_common import load_fixture, materialise
from test_gpu_indels import SWITCHES, _files, _ok

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what every attachable consumer drives in tiddit_signal: its switches, then the counter the scan leaves (beside the 50-bp histogram and the
# signal predicates, which every scan runs).  ``_scan`` sets and resets exactly these; tests/test_scan_all_refs_cpu.py holds the table
# against tiddit_signal's globals, so that the next consumer cannot be left out silently.
DRIVES = {"track": ("COV_TRACK",), "store": ("KEEP_EVIDENCE",), "alleles": ("ALLELES", "ALLELE_COUNTER"), "qc": ("QC", "QC_COUNTER"),
          "dups": ("DUPS", "DUP_COUNTER"), "indels": ("INDELS", "INDEL_REFERENCE", "INDEL_COUNTER"), "snvs": ("SNVS", "SNV_REFERENCE", "SNV_COUNTER"),
          "clips": ("CLIPS", "CLIPS_INS", "CLIP_COUNTER"), "str": ("STR",)}        # (STR: a tiddit_str.ScanTap, the counter inside it)
ATTACHABLE = tuple(DRIVES)
OFF = {"KEEP_EVIDENCE": False, "CLIPS_INS": False}                          # (every other switch is off as None)
STAGES = ("align", "far", "ins", "mei")
SPAN = str(1 << 16)


# ---- part A: the real driver, in process -----------------------------------------------------------------------------------------
class Made:
    pass


def make(directory, generate=C.generate):
    """``generate(directory)`` writes the file and what lies beside it -> the file, the definitions' results and files, the sites, the
    loci and the resident reference (the caller closes ``reference``)"""
    from tiddit_amd import fasta, refseq, tiddit_str
    m = Made()
    m.dir = directory
    m.info = generate(m.dir)
    m.bam, m.fa, m.vcf = C.paths(m.dir)
    m.library = C.library_path(m.dir)
    parts = C.partials(m.dir)
    m.E = C.combine(parts)
    C.write_definition_files(os.path.join(m.dir, "want"), parts, m.E, m.library)
    m.files = {ext: _content(os.path.join(m.dir, "want") + ext) for ext in C.STAGE_FILES + (C.STR_FILE,)}
    m.sites = C.sites_table(m.dir)
    table = C.contigs()
    m.names, m.lengths = [n for n, _ in table], [l for _, l in table]
    m.loci = tiddit_str.read_loci(C.str_path(m.dir), m.names, m.lengths)
    assert m.loci.rows == C.str_loci().rows and not any(m.loci.skipped.values())
    m.reference = refseq.load_for_bam(fasta.FastaFile(m.fa), m.names, m.lengths)[0]
    return m


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """the file of scan_all_cases with everything :func:`make` gives (one resident reference for every scan of the module)"""
    m = make(str(tmp_path_factory.mktemp("scan_all")))
    yield m
    m.reference.close()


def _keyed(h, supports):
    """a keyed counter's store as a sorted multiset, and its counters and rows at every support"""
    k1, k2 = h.keys()
    by_support = {}
    for s in supports:
        counts = h.finish(s)
        by_support[s] = (counts, list(h.rows()))
    return C.key_rows(list(zip(k1.tolist(), k2.tolist()))), by_support


def _chain(m, S, cov):
    """the clip chain behind the scan as ``__main__`` runs it, on the live objects: the counter where its rows lie, the shared reference,
    the evidence store in place -> the rows the stages kept and every file they wrote (under a prefix of their own)"""
    from tiddit_amd import tiddit_clip_mei, tiddit_clip_vcf, tiddit_clips, tiddit_variant
    prefix = os.path.join(tempfile.mkdtemp(dir=m.dir), "live")
    keep = {}
    counter, S.CLIP_COUNTER = S.CLIP_COUNTER, None                             # (tiddit_clips.main closes it, whatever happens)
    tiddit_clips.main(counter, prefix, cov, m.names, C.CLIP_S, align=(m.reference,) + C.ALIGN, far=(m.reference,) + C.FAR, ins=C.INS, keep=keep,
                      mei=(m.library, C.MEI_MIN))
    assert counter.handle is None and sorted(keep) == sorted(STAGES)
    tiddit_clip_vcf.main(tiddit_variant.LIVE_STORE, prefix, m.names, C.FLANK, C.header_parts(), keep["align"], keep["far"], keep["ins"],
                         mei=(C.MEI_MIN, keep["mei"], tiddit_clip_mei.library_index(m.library)[1]))
    return {"rows": {k: [tuple(r) for r in keep[k]] for k in STAGES}, "files": {ext: _content(prefix + ext) for ext in C.STAGE_FILES}}


def _collect(m, S, tables, data, splits, clips, cov, seen):
    """everything one scan left behind, in the shapes of scan_all_cases.combine"""
    from tiddit_amd import tiddit_variant
    R = {"batches": len(seen), "records": sum(seen), "cov": cov}
    if S.SNV_COUNTER is not None:
        R["snvs"] = _keyed(S.SNV_COUNTER, C.SNV_SUPPORTS)
        R["snv_reserve"] = S.SNV_COUNTER.reserve_stats()
    if S.CLIP_COUNTER is not None:
        e1, e2 = S.CLIP_COUNTER.ext_keys()
        R["clips"] = _keyed(S.CLIP_COUNTER, C.CLIP_SUPPORTS) + (C.key_rows(list(zip(e1.tolist(), e2.tolist()))),)
        R["clip_reserve"] = S.CLIP_COUNTER.reserve_stats()
        if tiddit_variant.LIVE_STORE is not None:
            # (in front of everything below: the junction support reads the store in place, and what the store holds is collected behind it)
            R["chain"] = _chain(m, S, cov)
    if tables is not None:
        data, splits = tables.rows()
        text = {n: tables.clips(t) for t, n in enumerate(tables.names)}
    else:
        text = {n: b"".join(S._clip_bytes(e) for e in v) for n, v in clips.items()}
    R["signals"] = (data, splits, text)
    if S.COV_TRACK_BINS is not None:
        R["track"] = S.COV_TRACK_BINS
    store = tiddit_variant.LIVE_STORE
    if store is not None:
        n, cap = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert store.ctx.lib.tdt_evstore_info(store.handle, ctypes.byref(n), ctypes.byref(cap), None) == 0
        R["store"] = ({t: C.store_fields(store.records(t)) for t in range(len(store.references))}, store.spans().astype(np.int64))
        R["store_capacity"] = cap.value
        assert n.value == store.n == int(store.count.sum())
    if S.ALLELE_COUNTER is not None:
        R["alleles"] = S.ALLELE_COUNTER.counts()
    if S.QC_COUNTER is not None:
        R["qc"] = S.QC_COUNTER.counts()
    if S.DUP_COUNTER is not None:
        k1, k2, mk = S.DUP_COUNTER.keys()
        R["dups"] = (C.key_rows(list(zip(k1.tolist(), k2.tolist(), mk.tolist()))) if len(k1) else np.zeros((0, 3), dtype=np.uint64), S.DUP_COUNTER.finish())
    h = S.INDEL_COUNTER
    if h is not None:
        k1, k2 = h.keys()
        by_support = {}
        for s in C.INDEL_SUPPORTS:
            counts = h.finish(s)
            by_support[s] = (counts, list(h.rows()))
        R["indels"] = (C.key_rows(list(zip(k1.tolist(), k2.tolist()))), by_support)
        if h.reference is not None:
            R["indels"] += (tuple(int(v) for v in h.norm_stats()),)
        R["indel_reserve"] = h.reserve_stats()
    if S.STR is not None and S.STR.counter is not None:
        R["str"] = _str(m, S.STR, R)
    return R


def _str(m, tap, R):
    """the counter the scan left in the tap: its store, counters and rows, then the stage behind the scan as ``__main__`` runs it, on that
    live counter under a prefix of its own -> (sorted key rows, counters, row columns, the table at ``STR_S``, the file it wrote)"""
    from tiddit_amd import tiddit_str
    h = tap.counter                                                            # (left in the tap until the stage takes it: ``_scan`` closes what is there)
    k1, k2 = h.keys()
    counts = h.finish()
    rows = h.rows()
    R["str_reserve"] = h.reserve_stats()
    prefix = os.path.join(tempfile.mkdtemp(dir=m.dir), "live")
    tap.counter = None
    try:
        again = tiddit_str.main(h, tap.loci, prefix, C.STR_CUTS)
    finally:
        h.close()                                                              # (tiddit_str.main closes it behind its last read; whatever happens, it is closed here)
    assert h.handle is None and np.array_equal(again, counts)
    return (C.key_rows(list(zip(k1.tolist(), k2.tolist()))), counts, rows, tiddit_str.summarise(tap.loci, rows, C.STR_S), _content(prefix + C.STR_FILE))


def _scan(m, on, norm=True):
    """``tiddit_signal._scan`` on the module's file with the consumers ``on`` attached -> what it left behind (:func:`_collect`); the
    module globals, the counters, the store, the tables and a carry nobody took are closed and reset whatever happens"""
    from tiddit_amd import bamio, tiddit_signal as S, tiddit_str, tiddit_variant
    assert set(on) <= set(ATTACHABLE)
    assert all(getattr(S, n) is OFF.get(n) for names in DRIVES.values() for n in names)
    seen = []
    real = S._device_scan

    def counting(batch, *a, **k):
        seen.append(len(batch))
        return real(batch, *a, **k)
    tables = None
    try:
        S._device_scan = counting
        S.COV_TRACK = C.TRACK if "track" in on else None
        S.KEEP_EVIDENCE = "store" in on
        S.ALLELES = (m.sites.site_pos, m.sites.site_off, C.MIN_BQ) if "alleles" in on else None
        S.QC = True if "qc" in on else None
        S.DUPS = True if "dups" in on else None
        S.INDELS = (2, C.INDEL_Q) if "indels" in on else None
        S.INDEL_REFERENCE = m.reference if "indels" in on and norm else None
        S.SNVS = (C.SNV_SUPPORTS[0], C.SNV_Q, C.SNV_BQ) if "snvs" in on else None
        S.SNV_REFERENCE = m.reference if "snvs" in on else None                # (the one handle the indel counter holds)
        S.CLIPS = (C.CLIP_S, C.CLIP_Q, C.CLIP_L) if "clips" in on else None
        S.CLIPS_INS = "clips" in on                                            # (clips always with the extension store)
        if "str" in on:
            assert tiddit_str.attach(m.loci, C.STR_CUTS) is S.STR              # (as __main__ attaches it: a tap the scan leaves its counter in)
        header, chromosomes, cov, data, splits, clips, tables = S._scan(m.bam, C.MIN_Q, C.MAX_INS, C.MIN_CONTIG, C.MIN_ANCHOR, C.MIN_CLIP, 50)
        assert chromosomes == [n for n, l in zip(m.names, m.lengths) if l >= C.MIN_CONTIG]
        return _collect(m, S, tables, data, splits, clips, cov, seen)
    finally:
        S._device_scan = real
        if S.STR is not None and S.STR.counter is not None:                    # (a counter a scan left in the tap and nobody took)
            S.STR.counter.close()
        tiddit_str.detach()
        for name in (n for names in DRIVES.values() for n in names):
            if name.endswith("_COUNTER") and getattr(S, name) is not None:
                getattr(S, name).close()
            setattr(S, name, OFF.get(name))
        S.COV_TRACK_BINS = None
        if tiddit_variant.LIVE_STORE is not None:
            tiddit_variant.LIVE_STORE.close()
            tiddit_variant.LIVE_STORE = None
        if tables is not None:
            tables.close()
        bamio.set_carry(None)


PARTS = ("cov", "signals", "track", "store", "alleles", "qc", "dups", "indels", "snvs", "clips", "chain", "str")


def _differing(a, b, parts=PARTS):
    return [k for k in parts if not C._eq(a[k], b[k])]


@pytest.fixture(scope="module")
def all_on(made):
    """every consumer attached, left-normalisation on, 64-KiB spans: the run the others are compared with"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TIDDIT_INGEST_CHUNK", SPAN)
        mp.delenv("TIDDIT_HOST_INGEST", raising=False)
        return _scan(made, ATTACHABLE)


def _as_run(E, files):
    """the definitions' results in the shapes an all-on run leaves them (:func:`_collect`): what a run that is right returns"""
    R = {k: E[k] for k in ("records", "cov", "track", "store", "alleles", "qc", "dups", "snvs")}
    R["indels"] = E["indels_norm"]
    R["clips"] = E["clips"] + (E["clip_ext"],)
    R["chain"] = {"rows": {k: E["clip_chain"][k][1] for k in STAGES}, "files": {ext: files[ext] for ext in C.STAGE_FILES}}
    R["str"] = E["str"] + (files[C.STR_FILE],)
    return R


def _same_keyed(name, got, want, supports):
    """a keyed consumer's store and, per support, its counters and row columns; every failure names the part"""
    assert np.array_equal(got[0], want[0]), "%s: the keys" % name
    for s in supports:
        assert np.array_equal(got[1][s][0], want[1][s][0]), "%s: the counters at support %d: %s, %s" % (name, s, got[1][s][0].tolist(), want[1][s][0].tolist())
        assert len(got[1][s][1]) == len(want[1][s][1])
        for c, (x, y) in enumerate(zip(got[1][s][1], want[1][s][1])):
            assert np.array_equal(x, y), "%s: row column %d at support %d" % (name, c, s)


def _equals_definitions(R, E, files):
    """every consumer's result of an all-on run against scan_all_cases.expected, and the clip chain's rows and files against the
    definitions' (``files``: scan_all_cases.write_definition_files)"""
    assert R["records"] == E["records"]
    assert list(R["cov"]) == list(E["cov"]) and list(R["track"]) == list(E["track"])
    # piece by piece, so that a failure names what differs ...
    keys, by_support, norm = R["indels"]
    wkeys, wby, wnorm = E["indels_norm"]
    assert np.array_equal(keys, wkeys) and norm == wnorm and norm[0] > 0
    for s in C.INDEL_SUPPORTS:
        assert np.array_equal(by_support[s][0], wby[s][0]), (s, by_support[s][0].tolist(), wby[s][0].tolist())
        assert all(np.array_equal(x, y) for x, y in zip(by_support[s][1], wby[s][1])), s
    assert np.array_equal(R["dups"][0], E["dups"][0]) and np.array_equal(R["dups"][1], E["dups"][1])
    assert np.array_equal(R["qc"], E["qc"])
    assert np.array_equal(R["alleles"][0], E["alleles"][0]) and R["alleles"][1:] == E["alleles"][1:] and R["alleles"][1] > 0
    for n in E["cov"]:
        assert R["cov"][n].dtype == np.float64 and np.array_equal(R["cov"][n], E["cov"][n]), n
    for n in E["track"]:
        assert np.array_equal(R["track"][n], E["track"][n]), n
    assert np.array_equal(R["store"][1], E["store"][1])
    for t in E["store"][0]:
        assert all(np.array_equal(x, y) for x, y in zip(R["store"][0][t], E["store"][0][t])), t
    _same_keyed("snvs", R["snvs"], E["snvs"], C.SNV_SUPPORTS)
    _same_keyed("clips", R["clips"], E["clips"], C.CLIP_SUPPORTS)
    assert np.array_equal(R["clips"][2], E["clip_ext"]) and len(E["clip_ext"]) > 0, "clips: the extension keys"
    for stage in STAGES:
        got, want = R["chain"]["rows"][stage], E["clip_chain"][stage][1]
        assert len(got) == len(want) > 0, "chain: the number of %s rows: %d, %d" % (stage, len(got), len(want))
        for c, (x, y) in enumerate(zip(zip(*got), zip(*want))):
            assert x == y, "chain: column %d of the %s rows" % (c, stage)
    assert sorted(R["chain"]["files"]) == sorted(C.STAGE_FILES) and sorted(files) == sorted(C.STAGE_FILES + (C.STR_FILE,))
    for ext in C.STAGE_FILES:
        assert R["chain"]["files"][ext] == files[ext], "chain: the file %s" % ext
    keys, counts, cols, table, text = R["str"]
    wkeys, wcounts, wcols, wtable = E["str"]
    assert np.array_equal(keys, wkeys), "str: the keys"
    assert np.array_equal(counts, wcounts), "str: the counters: %s, %s" % (counts.tolist(), wcounts.tolist())
    assert len(cols) == len(wcols) == 4
    for c, (x, y) in enumerate(zip(cols, wcols)):
        assert np.array_equal(x, y), "str: row column %d" % c
    assert len(table) == len(wtable)
    for k, (x, y) in enumerate(zip(table, wtable)):
        assert x == y, "str: the table's row of locus %d: %s, %s" % (k, x, y)
    assert text == files[C.STR_FILE], "str: the file %s" % C.STR_FILE
    # ... and each as a whole: shapes, dtypes, nothing more and nothing less than the definition gives
    for name, want in (("indels", "indels_norm"), ("dups", "dups"), ("qc", "qc"), ("alleles", "alleles"), ("cov", "cov"), ("track", "track"), ("store", "store"),
                       ("snvs", "snvs")):
        assert C._eq(R[name], E[want]), name
    assert C._eq(R["clips"], E["clips"] + (E["clip_ext"],)), "clips"
    assert C._eq(R["chain"], _as_run(E, files)["chain"]), "chain"
    assert C._eq(R["str"], _as_run(E, files)["str"]), "str"


def test_all_on_at_64k_spans_every_consumer_equals_its_definition(made, all_on):
    assert all_on["batches"] >= 24 and all_on["records"] == made.info["n_records"] and list(all_on["track"]) == made.names
    _equals_definitions(all_on, made.E, made.files)
    # the chain ran on something: every class of event the file holds (tests/test_scan_all_refs_cpu.py pins the definitions' counts)
    vcf = all_on["chain"]["files"][".clips.vcf"]
    assert vcf.count(b"SVTYPE=DEL") >= 3 and vcf.count(b"SVTYPE=BND") >= 6 and vcf.count(b";MEI=") >= 3
    assert all_on["snv_reserve"][2] > 64 and all_on["clip_reserve"][2] > 64 and all_on["str_reserve"][2] > 64
    assert len(all_on["str"][0]) > 0 and sum(1 for t in all_on["str"][3] if t[2] is not None) > 0       # (STR keys, and loci genotyped from them)


def test_all_on_signal_rows_clips_and_bins_equal_a_host_ingest_scan_with_nothing_attached(made, all_on, monkeypatch):
    monkeypatch.setenv("TIDDIT_HOST_INGEST", "1")
    H = _scan(made, ())
    assert H["batches"] == 0                                                   # (no device batch: the literal Python rows)
    data, splits, text = H["signals"]
    assert sum(len(v) for v in data.values()) >= 100 and sum(len(v) for v in splits.values()) >= 100 and sum(t.count(b">") for t in text.values()) >= 100
    assert _differing(all_on, H, ("cov", "signals")) == []


@pytest.mark.parametrize("chunk", [str(1 << 20), None], ids=["1MiB", "default"])
def test_span_size_does_not_matter(made, all_on, monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("TIDDIT_INGEST_CHUNK", raising=False)
    else:
        monkeypatch.setenv("TIDDIT_INGEST_CHUNK", chunk)
    R = _scan(made, ATTACHABLE)
    assert 1 <= R["batches"] < all_on["batches"] and R["records"] == all_on["records"]
    assert _differing(R, all_on) == []


@pytest.mark.parametrize("alone", ATTACHABLE)
def test_company_does_not_matter(made, all_on, monkeypatch, alone):
    monkeypatch.setenv("TIDDIT_INGEST_CHUNK", SPAN)
    R = _scan(made, (alone,))
    assert R["batches"] == all_on["batches"]
    assert [k for k in PARTS if k in R] == ["cov", "signals", alone]
    assert _differing(R, all_on, ("cov", "signals", alone)) == []


def test_alone_nothing_attached_and_indels_without_the_reference(made, all_on, monkeypatch):
    monkeypatch.setenv("TIDDIT_INGEST_CHUNK", SPAN)
    R = _scan(made, ())
    assert [k for k in PARTS if k in R] == ["cov", "signals"] and _differing(R, all_on, ("cov", "signals")) == []
    P = _scan(made, ("indels",), norm=False)
    assert len(P["indels"]) == 2 and C._eq(P["indels"], made.E["indels"])
    assert len(P["indels"][1][1][1][0]) > len(all_on["indels"][1][1][1][0])   # one row per placement without the reference


def _carried_scan(made, monkeypatch, track_bin, on=ATTACHABLE):
    """the statistics pass keeps its batches in HBM, the scan takes them -> (the scan's result, the batches that were carried)"""
    from tiddit_amd import bamio, tiddit_stats
    monkeypatch.setenv("TIDDIT_INGEST_CHUNK", SPAN)
    monkeypatch.delenv("TIDDIT_NO_CARRY", raising=False)
    try:
        tiddit_stats.statistics(made.bam, made.fa, C.MIN_Q, 100000, 5000, carry=True, track_bin_size=track_bin)
        c = bamio._CARRY
        assert c is not None and c.hist2 is not None and c.hist2.bin_size == track_bin
        held = list(c.batches)
        assert all(getattr(b, "_retained", None) and b._live for b in held)
    except BaseException:
        bamio.set_carry(None)
        raise
    return _scan(made, on), held


@pytest.mark.parametrize("track_bin", [C.TRACK[0], C.OTHER_TRACK_BIN], ids=["its own track column", "a column for another bin size"])
def test_carried_batches_reach_every_consumer_and_are_gone_afterwards(made, all_on, monkeypatch, track_bin):
    from tiddit_amd import _native
    ctx = _native.default_context()
    R, held = _carried_scan(made, monkeypatch, track_bin)
    assert 3 <= len(held) < all_on["batches"]                                  # (at least 3 and fewer than all batches were retained)
    assert R["batches"] == all_on["batches"] and R["records"] == all_on["records"]
    assert _differing(R, all_on) == []
    _equals_definitions(R, made.E, made.files)
    assert all(b._retained is None and not b._live for b in held)
    assert ctx.lib.tdt_device_cache_bytes(ctx.handle) > 0                      # (their buffers and the reader's went to the ingest cache)
    _native.check(ctx.lib.tdt_device_cache_flush(ctx.handle, None))
    assert ctx.lib.tdt_device_cache_bytes(ctx.handle) == 0


def _tiny(monkeypatch, dup_class=None):
    """the six stores of the scan start with room for 64 items (the names as ``_scan`` looks them up)"""
    from tiddit_amd import tiddit_clips, tiddit_dup, tiddit_indels, tiddit_region, tiddit_snvs, tiddit_str

    def small(cls):
        class Tiny(cls):
            def __init__(self, *a, capacity=None, **k):
                super().__init__(*a, capacity=64, **k)
        return Tiny
    monkeypatch.setattr(tiddit_dup, "DupCounter", small(dup_class or tiddit_dup.DupCounter))
    monkeypatch.setattr(tiddit_indels, "IndelCounter", small(tiddit_indels.IndelCounter))
    monkeypatch.setattr(tiddit_region, "EvidenceStore", small(tiddit_region.EvidenceStore))
    monkeypatch.setattr(tiddit_snvs, "SnvCounter", small(tiddit_snvs.SnvCounter))
    monkeypatch.setattr(tiddit_str, "StrCounter", small(tiddit_str.StrCounter))

    class TinyClips(small(tiddit_clips.ClipCounter)):
        def enable_ext(self, capacity=None):
            super().enable_ext(capacity=64)
    monkeypatch.setattr(tiddit_clips, "ClipCounter", TinyClips)


def _grown(R):
    asks, grows, cap = R["indel_reserve"]
    assert asks >= 1 and grows >= 1 and cap > 64, R["indel_reserve"]
    # (the dup store has no accessor for its capacity: it holds more keys than it had room for, and its kernel never writes past its room)
    assert len(R["dups"][0]) > 64 and R["store_capacity"] > 64
    for name in ("snv_reserve", "clip_reserve", "str_reserve"):
        asks, grows, cap = R[name]
        assert asks >= 1 and grows >= 1 and cap > 64, (name, R[name])
    assert len(R["clips"][2]) > 64                                             # (the extension store has no accessor either)


def test_the_stores_grow_mid_scan(made, all_on, monkeypatch):
    monkeypatch.setenv("TIDDIT_INGEST_CHUNK", SPAN)
    _tiny(monkeypatch)
    R = _scan(made, ATTACHABLE)
    assert R["batches"] == all_on["batches"] and _differing(R, all_on) == []
    _equals_definitions(R, made.E, made.files)                                 # (the junction support among it: the evidence store it read had grown)
    _grown(R)
    assert all_on["indel_reserve"][1] == all_on["snv_reserve"][1] == all_on["clip_reserve"][1] == 0       # (the all-on run's stores were made large enough: nothing grew there)


KEYED = ("indels", "snvs", "clips", "str")


def test_host_ingest_with_the_four_keyed_consumers_together(made, all_on, monkeypatch):
    """``TIDDIT_HOST_INGEST=1``: the host reader's batches through ``push_host_batch`` of the indel, the SNV, the clip and the STR counter,
    which share one upload block per handle (the STR counter with a column more: ``end``)"""
    monkeypatch.setenv("TIDDIT_HOST_INGEST", "1")
    H = _scan(made, KEYED)
    assert H["batches"] == 0 and H["records"] == 0                             # (no device batch)
    assert [k for k in PARTS if k in H] == ["cov", "signals"] + list(KEYED)
    assert _differing(H, all_on, KEYED) == []
    assert len(H["snvs"][0]) > 0 and len(H["clips"][0]) > 0 and len(H["clips"][2]) > 0 and len(H["str"][0]) > 0


def test_an_allocation_refused_mid_scan_is_retried_behind_the_cache_flush(made, all_on, monkeypatch):
    """the library's own hook makes the next device allocation fail once, as the driver would — immediately before the first push of the
    duplicate store, which has to grow (room for 64) while the statistics pass's batches are held in HBM; nothing faults, the refused
    call is simply made again behind the flush of the ingest's buffer cache"""
    from tiddit_amd import _native, tiddit_dup
    lib = _native.default_context().lib
    armed = []

    class Refused(tiddit_dup.DupCounter):
        def push_device_batch(self, b):
            if not armed:
                armed.append(len(b))
                lib.tdt_debug_fail_next_malloc(1)
            super().push_device_batch(b)
    _tiny(monkeypatch, Refused)
    try:
        R, held = _carried_scan(made, monkeypatch, C.TRACK[0])
    finally:
        lib.tdt_debug_fail_next_malloc(0)
    assert len(armed) == 1 and len(held) >= 3
    assert R["batches"] == all_on["batches"] and _differing(R, all_on) == []
    _equals_definitions(R, made.E, made.files)
    _grown(R)


# ---- part B: every switch in one job ----------------------------------------------------------------------------------------------
ALL_SWITCHES = tuple(SWITCHES) + ("TIDDIT_INDELS_NORM", "TIDDIT_INGEST_CHUNK", "TIDDIT_NO_CARRY", "TIDDIT_SNVS", "TIDDIT_CLIPS", "TIDDIT_CLIPS_ALIGN",
                                  "TIDDIT_CLIPS_FAR", "TIDDIT_CLIPS_INS", "TIDDIT_CLIPS_VCF", "TIDDIT_CLIPS_MEI", "TIDDIT_CLIPS_MEI_MIN", "TIDDIT_STR", "TIDDIT_STR_CUTS")
NOT_SCAN_SWITCHES = ()          # a switch of the package's docstrings that the jobs need not strip would be named here; today there is none
SUMMARIES = ("qc tables:", "duplicates:", "indels:", "indels, left-normalised:", "allele counts:", "note: TIDDIT_CNV skips", "note: TIDDIT_ASCN skips",
             "snvs:", "clips:", "clips align:", "clips far:", "clips ins:", "clips mei:", "clips vcf:", "str:")
# the files of each family (everything else is written by every job); .vcf and .genotyped.vcf carry one line that names the job's own prefix,
# ``##TIDDITcmd=`` (the command line): they are compared without exactly that line
OWNED = {"qc": (".qc.tab",), "dups": (".dup.tab",), "indels": (".indels.tab",), "acn": (".alleles.tab", ".cnv.bed", ".ascn.bed"), "track": (".bed",),
         "variants": (".vcf", ".depth_dist.tab", ".depth_summary.tab"), "genotype": (".genotyped.vcf",), "snvs": (".snvs.tab",),
         "clips": (".clips.tab", ".clips.align.tab", ".clips.far.tab", ".clips.ins.tab", ".clips.mei.tab", ".clips.vcf"),
         "str": (".str.tab",)}
STR_CUTS = "5:3:20"
HOMOPOLYMER, DINUCLEOTIDE = 8, 5          # the catalogue of the fixture: every homopolymer run of 8 or more bases, every dinucleotide run of 5 or more units


def _job(bam, fa, out, fx, timeout=600, **env):
    e = {k: v for k, v in os.environ.items() if k not in ALL_SWITCHES}
    e.update(env)
    argv = [sys.executable, "-m", "tiddit_amd", "--sv", "--bam", bam, "--ref", fa, "-o", out, "--skip_assembly", "-s", str(fx["params"]["n_reads_stats"])]
    return subprocess.run(argv, cwd=REPO, env=e, capture_output=True, text=True, timeout=timeout)


def _write_sites(path, fa, contigs):
    """every 997th base of every contig, REF the reference base, ALT the next base of ACGT"""
    from tiddit_amd.fasta import FastaFile
    fasta = FastaFile(fa)
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for name, ln in contigs:
            seq = fasta.fetch(name).upper()
            for p in range(996, ln, 997):
                ref = seq[p]
                f.write("%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (name, p + 1, ref, "ACGT"[("ACGT".index(ref) + 1) % 4] if ref in "ACGT" else "A"))


def _write_loci(path, fa, contigs):
    """the STR catalogue of the fixture's own reference: every run of ``HOMOPOLYMER`` or more equal bases and every run of ``DINUCLEOTIDE``
    or more units of two different bases, with both neighbour bases inside the contig, a run that touches the one in front left out
    -> the number of rows"""
    import re
    from tiddit_amd.fasta import FastaFile
    fasta = FastaFile(fa)
    n = 0
    with open(path, "w") as f:
        for name, ln in contigs:
            seq = fasta.fetch(name).upper()
            runs = [(m.start(), m.end(), m.group(1)) for m in re.finditer(r"([ACGT])\1{%d,}" % (HOMOPOLYMER - 1), seq)]
            runs += [(m.start(), m.end(), m.group(1)) for m in re.finditer(r"([ACGT]{2})\1{%d,}" % (DINUCLEOTIDE - 1), seq) if m.group(1)[0] != m.group(1)[1]]
            last = 0
            for s, e, unit in sorted(runs):
                if s >= max(1, last + 1) and e <= ln - 1:
                    f.write("%s\t%d\t%d\t%s\t%s_%d\n" % (name, s, e, unit, name, s))
                    last = e
                    n += 1
    return n


def _write_library(path, fa, contigs):
    """three families: pieces of the fixture's own reference (an inserted copy of one of them is a dispersed duplication, which the
    mei stage names) — the first as it stands, the second reverse-complemented, the third with every 50th base changed"""
    from tiddit_amd.fasta import FastaFile
    fasta = FastaFile(fa)
    name, ln = max(contigs, key=lambda c: c[1])
    seq = "".join(c if c in "ACGT" else "A" for c in fasta.fetch(name).upper())
    cut = lambda i, n: seq[(i * ln) // 4:(i * ln) // 4 + n]
    third = list(cut(3, 400))
    third[::50] = ["ACGT"[("ACGT".index(c) + 1) % 4] for c in third[::50]]
    families = (("FamOne", cut(1, 300)), ("FamTwo", cut(2, 500)[::-1].translate(str.maketrans("ACGT", "TGCA"))), ("FamThree", "".join(third)))
    with open(path, "w") as f:
        for n, t in families:
            f.write(">%s\n" % n + "".join(t[o:o + 60] + "\n" for o in range(0, len(t), 60)))


@pytest.fixture(scope="module")
def jobs(golden_dir, tmp_path_factory):
    """(each job is checked before the next one is started: a crash, a time-out or a GPU error ends the fixture there)"""
    fx = load_fixture(golden_dir, "sv_e2e_small.json")
    d = str(tmp_path_factory.mktemp("scan_all_jobs"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    sites = os.path.join(d, "sites.vcf")
    _write_sites(sites, fa, contigs)
    library = os.path.join(d, "families.fa")
    _write_library(library, fa, contigs)
    loci = os.path.join(d, "loci.bed")
    assert _write_loci(loci, fa, contigs) >= 1
    paths = {n: os.path.join(d, n) for n in tuple(OWNED) + ("all", "all4m")}
    family = {"qc": dict(TIDDIT_QC="1"), "dups": dict(TIDDIT_DUPS="1"), "indels": dict(TIDDIT_INDELS="1:20", TIDDIT_INDELS_NORM="1"),
              "acn": dict(TIDDIT_ALLELES=sites, TIDDIT_CNV="1", TIDDIT_ASCN="1"), "track": dict(TIDDIT_COV_TRACK="500"),
              "variants": dict(TIDDIT_VARIANTS="1", TIDDIT_DEPTH_DIST="1"), "snvs": dict(TIDDIT_SNVS="2"),
              "clips": dict(TIDDIT_CLIPS="2", TIDDIT_CLIPS_ALIGN="1", TIDDIT_CLIPS_FAR="1", TIDDIT_CLIPS_INS="1", TIDDIT_CLIPS_VCF="1", TIDDIT_CLIPS_MEI=library),
              "str": dict(TIDDIT_STR=loci, TIDDIT_STR_CUTS=STR_CUTS)}
    out = {}
    for name, env in family.items():
        out[name] = _ok(_job(bam, fa, paths[name], fx, **env))
    family["genotype"] = dict(TIDDIT_GENOTYPE=paths["variants"] + ".vcf")
    out["genotype"] = _ok(_job(bam, fa, paths["genotype"], fx, **family["genotype"]))
    every = {k: v for env in family.values() for k, v in env.items()}
    assert len(every) == sum(len(env) for env in family.values()) == 20
    out["all"] = _ok(_job(bam, fa, paths["all"], fx, **every))
    out["all4m"] = _ok(_job(bam, fa, paths["all4m"], fx, TIDDIT_INGEST_CHUNK=str(4 << 20), **every))
    assert os.path.getsize(bam) > 5 * (4 << 20)                                # (the small-span job sees more than five spans)
    return paths, out


def _content(path):
    """a file's bytes; of a VCF: without its ``##TIDDITcmd=`` line, which names the job's own prefix"""
    data = open(path, "rb").read()
    if path.endswith(".vcf"):
        lines = data.split(b"\n")
        assert sum(l.startswith(b"##TIDDITcmd=") for l in lines) == 1
        return b"\n".join(l for l in lines if not l.startswith(b"##TIDDITcmd="))
    return data


def _summaries(r):
    return [l for l in r.stdout.split("\n") if l.startswith(SUMMARIES)]


def test_the_all_on_job_writes_the_union_of_the_family_jobs_files(jobs):
    paths, out = jobs
    sets = {n: set(_files(paths[n])) for n in paths}
    common = set.intersection(*(sets[n] for n in OWNED))
    assert len(common) >= 5
    for n, owned in OWNED.items():
        assert sets[n] - common == set(owned), (n, sorted(sets[n] - common))
    assert sets["all"] == set.union(*(sets[n] for n in OWNED)) == sets["all4m"]
    assert len(sets["all"]) == len(common) + sum(len(v) for v in OWNED.values())


def test_every_file_of_the_all_on_job_is_the_owning_jobs_file(jobs):
    paths, out = jobs
    rel = sorted(_files(paths["all"]))
    owner = {ext: n for n, owned in OWNED.items() for ext in owned}
    for k in rel:
        for n in ([owner[k]] if k in owner else list(OWNED)):                   # (a file every job writes: the same in each of them)
            assert _content(paths["all"] + k) == _content(paths[n] + k), (k, n)
    for ext in owner:
        assert len(_content(paths["all"] + ext)) > 50, ext


def test_the_str_family_job_genotypes_loci_of_the_fixtures_own_repeats(jobs):
    """(the catalogue at runs of 8 bases and 5 units: 272 loci of the fixture's reference, 271 of them genotyped by the definition)"""
    paths, out = jobs
    rows = [l.split("\t") for l in open(paths["str"] + ".str.tab").read().split("\n") if l and not l.startswith(("#", "SN\t"))]
    assert len(rows) >= 1 and all(len(r) == 16 for r in rows)
    assert sum(1 for r in rows if r[11] != ".") >= 1                            # GT: at least one locus with S or more spanning reads
    assert open(paths["str"] + ".str.tab").read().startswith("# tiddit_amd str v1 flank=5 min_reads=3 min_mapq=20\n")


def test_the_summary_lines_are_the_owning_jobs(jobs):
    paths, out = jobs
    want = [l for n in OWNED for l in _summaries(out[n])]
    got = _summaries(out["all"])
    assert sorted(got) == sorted(want) and len(got) >= 5
    assert {l.split(":")[0].split(",")[0] for l in got} >= {"qc tables", "duplicates", "indels", "allele counts", "snvs", "clips", "clips align", "clips far",
                                                            "clips ins", "clips mei", "clips vcf", "str"}


def test_the_all_on_job_at_4_mib_spans_writes_the_same_bytes(jobs):
    paths, out = jobs
    a, b = _files(paths["all"]), _files(paths["all4m"])
    assert set(a) == set(b)
    for k in sorted(a):
        assert _content(paths["all"] + k) == _content(paths["all4m"] + k), k
    assert _summaries(out["all4m"]) == _summaries(out["all"])
