"""The native variant stage on the GPU: the evidence store the scan fills (tdt_evstore_*), the one-launch region counts over it
(tdt_region_counts_packed) against the oracle and the per-contig kernel, and `TIDDIT_VARIANTS=1 tiddit --sv` against the VCF of
the compiled reference (tests/golden/sv_vcf*.json, tests/golden/make_golden_vcf.py)."""
import hashlib
import json
import os
import sys
import types

import numpy as np
import pytest

import oracle
from sv_e2e_common import load_fixture, materialise

pytestmark = pytest.mark.gpu

PAIRS = {"sv_vcf_small.json": "sv_e2e_small.json", "sv_vcf.json": "sv_e2e.json", "sv_vcf_grch38.json": "sv_e2e_grch38.json"}


def _bits(c, min_q, max_ins, tid):
    from tiddit_amd import tiddit_region as R
    f = c["flag"].astype(np.int64)
    b = np.where(f & 0x4, R.EV_UNMAPPED, 0) | np.where(f & 0x8, R.EV_MATE_UNMAPPED, 0) | np.where(f & 0x400, R.EV_DUPLICATE, 0)
    b |= np.where(c["has_sa"] != 0, R.EV_HAS_SA, 0) | np.where(c["mapq"].astype(np.int64) < min_q, R.EV_LOW_Q, 0)
    b |= np.where((np.abs(c["tlen"].astype(np.int64)) > max_ins) | (c["mate_tid"] != tid), R.EV_DISCORDANT, 0)
    return b.astype(np.uint8)


@pytest.fixture(scope="module")
def files(golden_dir, tmp_path_factory):
    out = {}
    for name in ("sv_e2e_small.json", "sv_e2e_grch38.json"):
        fx = load_fixture(golden_dir, name)
        d = str(tmp_path_factory.mktemp("store"))
        bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
        out[name] = (fx, bam, fa, contigs)
    return out


@pytest.mark.parametrize("name", ["sv_e2e_small.json", "sv_e2e_grch38.json"])
@pytest.mark.parametrize("host", [False, True])
def test_store_equals_read_table(files, name, host, monkeypatch):
    """every contig's packed records = ReadTable's columns (bits included), max span reduced on the device, the tid = -1 tail left out"""
    from tiddit_amd import tiddit_region
    fx, bam, fa, contigs = files[name]
    if host:
        monkeypatch.setenv("TIDDIT_HOST_INGEST", "1")
    min_q, max_ins = fx["params"]["min_q"], int(fx["library"]["percentile_insert_size"])
    store = tiddit_region.build_store(bam, min_q, max_ins)
    try:
        monkeypatch.delenv("TIDDIT_HOST_INGEST", raising=False)
        table = tiddit_region.ReadTable(bam)
        spans = store.spans()
        total = 0
        for t in range(len(table.references)):
            c = table.contigs[t]
            got = store.records(t)
            assert len(got) == len(c["start"]) == store.count[t], table.references[t]
            total += len(got)
            assert np.array_equal(got["start"], c["start"]) and np.array_equal(got["end"], c["end"])
            assert np.array_equal(got["mate_pos"], c["mate_pos"])
            assert np.array_equal(got["bits"], _bits(c, min_q, max_ins, t)), table.references[t]
            assert not got["pad"].any()
            want_span = int((c["end"].astype(np.int64) - c["start"]).max()) if len(got) else 0
            assert spans[t] == want_span
        assert total == store.n
        if name == "sv_e2e_grch38.json":
            assert store.n < fx["n_records"]                      # (the unplaced tail is not in the store)
    finally:
        store.close()


def _synthetic_store(min_q, max_ins):
    """three contigs: empty; one read; many reads with one longer than every other — through the host-upload path"""
    from tiddit_amd import tiddit_region
    rng = np.random.default_rng(3)
    lengths = [50_000, 40_000, 200_000]
    cols = {k: [] for k in ("tid", "pos", "end", "mapq", "flag", "mate_tid", "mate_pos", "tlen", "sa_off")}

    def add(t, pos, end, mapq, flag, mtid, mpos, tlen, sa):
        for k, v in zip(cols, (t, pos, end, mapq, flag, mtid, mpos, tlen, sa)):
            cols[k].append(np.asarray(v))
    add([1], [20_000], [20_150], [60], [0x1 | 0x2], [1], [20_300], [450], [-1])
    n = 20_000
    pos = np.sort(rng.integers(0, lengths[2] - 200, n))
    end = pos + rng.integers(1, 151, n)
    end[n // 2] = pos[n // 2] + 9_000                              # the longest read by far
    flag = rng.choice([0x1, 0x3, 0x11, 0x401, 0x9, 0x5, 0x801], n, p=[.4, .3, .1, .05, .05, .05, .05])
    mtid = np.where(rng.random(n) < 0.05, 0, 2)
    mpos = np.clip(pos + rng.integers(-2000, 2000, n), 0, None)
    tlen = rng.integers(-3000, 3000, n)
    sa = np.where(rng.random(n) < 0.03, 100, -1)
    add(np.full(n, 2), pos, end, rng.integers(0, 61, n), flag, mtid, mpos, tlen, sa)
    add([-1, -1], [-1, -1], [0, 0], [0, 0], [4, 4], [-1, -1], [-1, -1], [0, 0], [-1, -1])      # unplaced tail
    dt = {"tid": np.int32, "pos": np.int32, "end": np.int32, "mapq": np.uint8, "flag": np.uint16, "mate_tid": np.int32, "mate_pos": np.int32,
          "tlen": np.int32, "sa_off": np.int64}
    b = types.SimpleNamespace(**{k: np.concatenate(v).astype(dt[k]) for k, v in cols.items()})
    store = tiddit_region.EvidenceStore("synthetic", ["c0", "c1", "c2"], lengths, min_q, max_ins, capacity=1000)     # (grows)
    half = 7_000                                                    # two batches, contig 2 spanning both
    b1 = types.SimpleNamespace(**{k: getattr(b, k)[:half] for k in cols})
    b2 = types.SimpleNamespace(**{k: getattr(b, k)[half:] for k in cols})
    store.add_host_batch(b1)
    store.add_host_batch(b2)
    per = {}
    for t in range(3):
        m = b.tid == t
        per[t] = {"start": b.pos[m], "end": b.end[m], "mapq": b.mapq[m], "flag": b.flag[m], "mate_tid": b.mate_tid[m], "mate_pos": b.mate_pos[m],
                  "tlen": b.tlen[m], "has_sa": (b.sa_off[m] >= 0).astype(np.uint8)}
    return store, lengths, per


def test_packed_counts_equal_oracle_and_device_kernel():
    from tiddit_amd import _native
    min_q, max_ins = 20, 600
    store, lengths, per = _synthetic_store(min_q, max_ins)
    try:
        assert store.n == 20_001 and list(store.count) == [0, 1, 20_000]
        rng = np.random.default_rng(9)
        q = []
        for t in range(3):
            L = lengths[t]
            for _ in range(300):
                s = int(rng.integers(0, L))
                e = s + int(rng.integers(0, 3000))
                q.append((t, s, e, int(rng.integers(s - 100, e + 100))))
            q += [(t, L - 50, L + 10, L - 20),          # q_end clamped at the contig end
                  (t, L + 5, L + 20, L),               # q_start >= q_end: the fallback q_end - 10
                  (t, 0, 100, 3), (t, 0, 0, 0),        # bp near 0
                  (t, 19_990, 20_200, 20_100)]
        q = np.array(q, dtype=np.int64)
        got = store.region_counts(q, min_q, max_ins)
        ctx = _native.default_context()
        for i, (t, s, e, bp) in enumerate(q):
            c = per[int(t)]
            want = oracle.get_region_counts(c, int(t), lengths[t], int(s), int(e), int(bp), min_q, max_ins)
            assert np.array_equal(got[i], want), (i, q[i], got[i], want)
        for t in range(3):                              # the per-contig kernel of tdt_region.hip on the same queries
            sel = q[q[:, 0] == t]
            c = {k: np.ascontiguousarray(v) for k, v in per[t].items()}
            out = np.zeros((len(sel), 7), dtype=np.int64)
            qs, qe, qb = (np.ascontiguousarray(sel[:, j], dtype=np.int32) for j in (1, 2, 3))
            _native.check(ctx.lib.tdt_region_counts(ctx.handle, *[_native.ptr(c[k]) for k in ("start", "end", "mapq", "flag", "mate_tid",
                                                                                               "mate_pos", "tlen", "has_sa")],
                                                    len(c["start"]), t, lengths[t], _native.ptr(qs), _native.ptr(qe), _native.ptr(qb), len(sel),
                                                    min_q, max_ins, _native.ptr(out)))
            assert np.array_equal(out, got[q[:, 0] == t])
    finally:
        store.close()


def test_packed_counts_refuse_other_parameters():
    from tiddit_amd import _native
    store, lengths, per = _synthetic_store(20, 600)
    try:
        q = np.array([(2, 1000, 2000, 1500)], dtype=np.int64)
        for mq, mi in ((19, 600), (20, 601)):
            with pytest.raises(_native.TdtError) as e:
                store.region_counts(q, mq, mi)
            assert e.value.code == -1
        with pytest.raises(_native.TdtError):
            store.region_counts(np.array([(3, 0, 10, 5)]), 20, 600)        # no such contig row
    finally:
        store.close()


# ---- the CLI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["sv_vcf_small.json", "sv_vcf.json", "sv_vcf_grch38.json"])
def cli_run(request, golden_dir, tmp_path_factory):
    from tiddit_amd import __main__ as cli
    vfx = json.load(open(os.path.join(golden_dir, request.param)))
    fx = load_fixture(golden_dir, PAIRS[request.param])
    d = str(tmp_path_factory.mktemp("vcf"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    out = os.path.join(d, "run")
    argv = ["--sv", "--bam", bam, "--ref", fa, "-o", out, "--skip_assembly", "-s", str(fx["params"]["n_reads_stats"])]
    os.environ["TIDDIT_VARIANTS"] = "1"
    try:
        cli.main(argv)
        cmd = '##TIDDITcmd="' + " ".join(sys.argv) + '"'
    finally:
        del os.environ["TIDDIT_VARIANTS"]
    return vfx, fx, bam, fa, out, argv, cmd


def _check_vcf(path, vfx, cmd):
    lines = [l for l in open(path).read().split("\n")]
    assert [l for l in lines if l.startswith("##TIDDITcmd=")] == [cmd]
    lines = [l for l in lines if not l.startswith("##TIDDITcmd=")]
    i = next(k for k, l in enumerate(lines) if l.startswith("#CHROM"))
    head = lines[:i + 1]
    assert [l for l in head if not l.startswith("##contig=")] == vfx["vcf_header_other_lines"]
    assert hashlib.sha256("\n".join(head).encode()).hexdigest() == vfx["vcf_header_sha256"]
    assert "\n".join(lines[i + 1:]) == _body(vfx)


def _body(vfx):
    return "".join(l + "\n" for l in vfx["vcf_records"])


def _candidate_rows(fx):
    return [[r[0], str(r[3]), r[1], str(r[4]), str(r[2])] + [str(x) for x in r[5:]] for r in fx["candidates"]]


def test_cli_vcf_equals_reference(cli_run):
    from tiddit_amd import __main__ as cli
    from tiddit_amd import tiddit_variant
    vfx, fx, bam, fa, out, argv, cmd = cli_run
    _check_vcf(out + ".vcf", vfx, cmd)
    rows = [l.rstrip("\n").split("\t") for l in open(out + ".candidates.tab") if not l.startswith("#")]
    assert rows == _candidate_rows(fx)
    assert "variant typing (native)" in cli.STAGE_SECONDS
    assert tiddit_variant.LIVE_STORE is None                    # (the store was freed with the stage)


def test_drop_in_main_without_a_live_store(cli_run):
    """tiddit_variant.main called on its own builds its store with one ingest pass over the file: the same VCF"""
    import argparse
    from tiddit_amd import tiddit_cluster, tiddit_gc, tiddit_signal, tiddit_variant, tiddit_vcf_header
    from tiddit_amd.bamio import BamReader
    vfx, fx, bam, fa, out, argv, cmd = cli_run
    if fx["params"]["total_mb"] > 8:
        pytest.skip("the drop-in path runs on the small fixture")
    P = fx["params"]
    lib = dict(vfx["meta"]["library"])
    max_ins = vfx["meta"]["max_ins_len"]
    r = BamReader(bam, batch_bytes=1 << 20)
    header = r.header
    r.close()
    names = [c["SN"] for c in header["SQ"]]
    cov = tiddit_signal.scan_signals(bam, P["min_q"], max_ins, P["min_contig"], P["min_anchor_len"], P["min_clip_len"], 50)[2]
    gc = tiddit_gc.main(fa, names, 1, 50, 0.5)
    cand = tiddit_cluster.main(out, names, {c["SN"]: c["LN"] for c in header["SQ"]}, ["WGS"], lib["mp"], fx["epsilon"], P["m"], max_ins,
                               P["min_contig"], True, P["min_reads"])
    args = argparse.Namespace(**dict(vfx["meta"]["args"], bam=bam, ref=fa, o=out))
    assert tiddit_variant.LIVE_STORE is None
    variants = tiddit_variant.main(bam, cand, args, lib, P["min_q"], ["WGS"], cov, {n: i for i, n in enumerate(names)}, max_ins, gc)
    assert "evidence store (one ingest pass)" in tiddit_variant.STAGE_SECONDS
    assert tiddit_variant.vcf_body(names, variants) == _body(vfx)
    assert tiddit_vcf_header.main(header, lib, "WGS", vfx["meta"]["version"]).split("\n")[-1].startswith("#CHROM")


def test_host_ingest_and_switch_off(golden_dir, tmp_path, monkeypatch):
    """small fixture: TIDDIT_HOST_INGEST=1 fills the store from the host columns, same VCF; without the switch no .vcf is written"""
    from tiddit_amd import __main__ as cli
    vfx = json.load(open(os.path.join(golden_dir, "sv_vcf_small.json")))
    fx = load_fixture(golden_dir, "sv_e2e_small.json")
    bam, fa, contigs = materialise(fx, str(tmp_path), threads=min(16, os.cpu_count() or 1))
    base = ["--sv", "--bam", bam, "--ref", fa, "--skip_assembly", "-s", str(fx["params"]["n_reads_stats"])]
    monkeypatch.setenv("TIDDIT_HOST_INGEST", "1")
    monkeypatch.setenv("TIDDIT_VARIANTS", "1")
    out = str(tmp_path / "host")
    cli.main(base + ["-o", out])
    _check_vcf(out + ".vcf", vfx, '##TIDDITcmd="' + " ".join(sys.argv) + '"')
    monkeypatch.delenv("TIDDIT_HOST_INGEST")
    monkeypatch.delenv("TIDDIT_VARIANTS")
    out = str(tmp_path / "off")
    cli.main(base + ["-o", out])
    assert not os.path.exists(out + ".vcf")
    rows = [l.rstrip("\n").split("\t") for l in open(out + ".candidates.tab") if not l.startswith("#")]
    assert rows == _candidate_rows(fx)
    assert not any(k.startswith("variant typing") for k in cli.STAGE_SECONDS)
