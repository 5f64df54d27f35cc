"""The native variant stage on N ranks on the GPU: the evidence stores of byte-range shards of a file add up to the whole file's store
(records and every get_region count), the device-query counts entry (tdt_region_counts_packed_device) equals the host one, and
`TIDDIT_VARIANTS=1 tiddit --sv` on 2 / 3 ranks (gloo, one GPU) and over real RCCL (one rank) writes the VCF of the compiled
reference (tests/golden/sv_vcf*.json)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from sv_e2e_common import load_fixture, materialise
from test_gpu_variant import PAIRS, _body, _candidate_rows, _check_vcf, _synthetic_store

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ["_tiddit/discordants_WGS.tab", "_tiddit/splits_WGS.tab", "_tiddit/clips_WGS.fa", ".ploidies.tab", ".candidates.tab"]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _without_cmd(path):
    return [l for l in open(path).read().split("\n") if not l.startswith("##TIDDITcmd=")]


# ---- 1. shard additivity ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stores(golden_dir, tmp_path_factory):
    """the whole-file store and the k = 2, 3 shard stores of the small and the GRCh38-shaped file"""
    from tiddit_amd import tiddit_region
    out = {}
    made = []
    try:
        for vname in ("sv_vcf_small.json", "sv_vcf_grch38.json"):
            vfx = json.load(open(os.path.join(golden_dir, vname)))
            fx = load_fixture(golden_dir, PAIRS[vname])
            bam, fa, contigs = materialise(fx, str(tmp_path_factory.mktemp("shards")), threads=min(16, os.cpu_count() or 1))
            min_q, max_ins = vfx["meta"]["min_mapq"], int(vfx["meta"]["max_ins_len"])
            whole = tiddit_region.build_store(bam, min_q, max_ins)
            made.append(whole)
            shards = {}
            for k in (2, 3):
                shards[k] = [tiddit_region.build_store(bam, min_q, max_ins, shard=(r, k)) for r in range(k)]
                made += shards[k]
            out[vname] = (vfx, whole, shards, min_q, max_ins)
        yield out
    finally:
        for s in made:
            s.close()


def _summed(shards, rows, min_q, max_ins):
    return sum(s.region_counts(rows, min_q, max_ins) for s in shards)


@pytest.mark.parametrize("vname", ["sv_vcf_small.json", "sv_vcf_grch38.json"])
@pytest.mark.parametrize("k", [2, 3])
def test_shard_stores_add_up_to_the_whole_file(stores, vname, k):
    from tiddit_amd import tiddit_variant
    vfx, whole, shards, min_q, max_ins = stores[vname]
    parts = shards[k]
    assert sum(s.n for s in parts) == whole.n and max(s.n for s in parts) < whole.n
    assert np.array_equal(sum(s.count for s in parts), whole.count)
    # the seams as dist.check_seams reads them: every non-empty shard starts where the chain of the one before it ends
    expect = None
    for fo, no, empty in (s.seam for s in parts):
        if empty:
            continue
        assert expect is None or fo == expect
        expect = no
    # every get_region call of the reference's run, from the summed counts of the shards
    calls = vfx["get_region_calls"]
    assert all(c[4] == min_q and int(c[5]) == max_ins for c in calls)
    rows = np.array([(whole.tid[c[0]], c[1], c[2], c[3]) for c in calls], dtype=np.int64)
    got = _summed(parts, rows, min_q, max_ins)
    assert np.array_equal(got, whole.region_counts(rows, min_q, max_ins))
    for i, c in enumerate(calls):
        assert tiddit_variant.region_tuple(got[i], c[1], c[2]) == tuple(c[6]), c
    # random windows on the contigs with reads, and windows across every seam that falls inside a contig
    rng = np.random.default_rng(k)
    q = []
    for t in np.flatnonzero(whole.count)[:40]:
        L = whole.lengths[t]
        for _ in range(25):
            s = int(rng.integers(0, L))
            e = s + int(rng.integers(0, 4000))
            q.append((t, s, e, int(rng.integers(s - 100, e + 100))))
        q += [(t, L - 50, L + 10, L - 20), (t, L + 5, L + 20, L)]      # clamped; q_start >= q_end
    seams = 0
    for a, b in zip(parts, parts[1:]):
        for t in np.flatnonzero((a.count > 0) & (b.count > 0)):
            x = int(b.records(int(t))["start"][0])                  # the first record of the next shard on a contig both hold
            seams += 1
            q += [(t, x - 300, x + 300, x), (t, x - 5, x + 5, x - 1), (t, x, x, x), (t, max(0, x - 2000), x - 1, x - 30), (t, x + 1, x + 900, x + 450)]
    assert seams >= 1
    q = np.array(q, dtype=np.int64)
    assert np.array_equal(_summed(parts, q, min_q, max_ins), whole.region_counts(q, min_q, max_ins))


# ---- 2. the device-query entry ------------------------------------------------------------------------------------------------------
def _device_counts(store, rows, min_q, max_ins):
    import torch
    q = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)).cuda()
    out = torch.full((len(q), 7), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    err = None
    try:
        store.region_counts_device(q.data_ptr(), len(q), min_q, max_ins, out.data_ptr())
    except Exception as e:
        err = e
    return out.cpu().numpy(), err


def test_device_entry_equals_host_entry():
    from tiddit_amd import _native
    min_q, max_ins = 20, 600
    store, lengths, per = _synthetic_store(min_q, max_ins)
    try:
        rng = np.random.default_rng(11)
        q = []
        for t in range(3):                                 # empty contig, one read, a contig split over two batches
            L = lengths[t]
            for _ in range(200):
                s = int(rng.integers(0, L))
                e = s + int(rng.integers(0, 3000))
                q.append((t, s, e, int(rng.integers(s - 100, e + 100))))
            q += [(t, L - 50, L + 10, L - 20), (t, L + 5, L + 20, L), (t, 0, 0, 0), (t, 19_990, 20_200, 20_100)]
        q = np.array(q, dtype=np.int64)
        want = store.region_counts(q, min_q, max_ins)
        got, err = _device_counts(store, q, min_q, max_ins)
        assert err is None and np.array_equal(got, want)
        assert want[:, 1].sum() > 0
        # bad contig rows: zeros there, the other queries answered, TDT_E_RANGE naming the first bad query
        bad = q.copy()
        bad[17, 0], bad[5, 0], bad[300, 0] = 3, -1, 1 << 20
        got, err = _device_counts(store, bad, min_q, max_ins)
        assert isinstance(err, _native.TdtError) and err.code == -3 and "query 5 " in str(err), err
        ok = np.ones(len(q), dtype=bool)
        ok[[5, 17, 300]] = False
        assert np.array_equal(got[ok], want[ok]) and not got[~ok].any()
        # the store's min_q / max_ins only
        for mq, mi in ((19, 600), (20, 601)):
            got, err = _device_counts(store, q[:4], mq, mi)
            assert isinstance(err, _native.TdtError) and err.code == -1
        # nq = 0 (null pointers allowed); null or misaligned pointers with queries
        store.region_counts_device(None, 0, min_q, max_ins, None)
        lib, ctx = store.ctx.lib, store.ctx
        tab = np.ascontiguousarray(store.contig_table())
        import torch
        dq = torch.from_numpy(np.ascontiguousarray(q[:8], dtype=np.int32)).cuda()
        dout = torch.zeros((8, 7), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for qp, op in ((None, dout.data_ptr()), (dq.data_ptr(), None), (dq.data_ptr() + 4, dout.data_ptr()), (dq.data_ptr(), dout.data_ptr() + 4)):
            assert lib.tdt_region_counts_packed_device(ctx.handle, store.handle, _native.ptr(tab), len(tab), qp, 8, min_q, max_ins, op) == -1
        assert lib.tdt_region_counts_packed_device(None, store.handle, _native.ptr(tab), len(tab), dq.data_ptr(), 8, min_q, max_ins, dout.data_ptr()) == -1
        assert lib.tdt_region_counts_packed_device(ctx.handle, None, _native.ptr(tab), len(tab), dq.data_ptr(), 8, min_q, max_ins, dout.data_ptr()) == -1
        assert lib.tdt_region_counts_packed_device(ctx.handle, store.handle, None, len(tab), dq.data_ptr(), 8, min_q, max_ins, dout.data_ptr()) == -1
        assert lib.tdt_region_counts_packed_device(ctx.handle, store.handle, _native.ptr(tab), len(tab), dq.data_ptr(), 8, min_q, max_ins,
                                                   dout.data_ptr()) == 0
        assert np.array_equal(dout.cpu().numpy(), want[:8])
        big = tab.copy()
        big[2, 1] += 1                                                  # a row past the end of the store: refused on the host
        assert lib.tdt_region_counts_packed_device(ctx.handle, store.handle, _native.ptr(big), len(big), dq.data_ptr(), 8, min_q, max_ins,
                                                   dout.data_ptr()) == -3
    finally:
        store.close()


# ---- 3-6. the CLI on N ranks ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["sv_vcf_small.json", "sv_vcf.json", "sv_vcf_grch38.json"])
def one(request, golden_dir, tmp_path_factory):
    """the one-process run with the switch on, and the size of the store its variant stage used"""
    from tiddit_amd import __main__ as cli
    from tiddit_amd import tiddit_region
    vfx = json.load(open(os.path.join(golden_dir, request.param)))
    fx = load_fixture(golden_dir, PAIRS[request.param])
    d = str(tmp_path_factory.mktemp("one"))
    bam, fa, contigs = materialise(fx, d, threads=min(16, os.cpu_count() or 1))
    out = os.path.join(d, "one")
    argv = ["--sv", "--bam", bam, "--ref", fa, "--skip_assembly", "-s", str(fx["params"]["n_reads_stats"])]
    sizes = []
    real = tiddit_region.EvidenceStore.close

    def close(self):
        if getattr(self, "handle", None):
            sizes.append(self.n)
        real(self)
    tiddit_region.EvidenceStore.close = close
    os.environ["TIDDIT_VARIANTS"] = "1"
    try:
        cli.main(argv + ["-o", out])
    finally:
        del os.environ["TIDDIT_VARIANTS"]
        tiddit_region.EvidenceStore.close = real
    assert len(sizes) == 1
    return request.param, vfx, fx, bam, fa, contigs, out, argv, sizes[0]


def _vcf_rank(rank, world, port, q, argv, env):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      TIDDIT_HIP_DEVICE="0", TIDDIT_DIST_BACKEND="gloo", TIDDIT_INGEST_CHUNK=str(48 << 20), TIDDIT_VARIANTS="1", **env)
    try:
        import torch.distributed as dist
        from tiddit_amd import __main__ as cli, tiddit_region, tiddit_variant
        sizes = []
        real = tiddit_region.EvidenceStore.close

        def close(self):
            if getattr(self, "handle", None):
                sizes.append(self.n)
            real(self)
        tiddit_region.EvidenceStore.close = close
        cli.main(argv)
        q.put((rank, {"cmd": '##TIDDITcmd="' + " ".join(sys.argv) + '"', "sizes": sizes, "live_none": tiddit_variant.LIVE_STORE is None,
                      "stages": sorted(tiddit_variant.STAGE_SECONDS)}))
        if dist.is_initialized():
            dist.destroy_process_group()
    except BaseException:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def _spawn(target, world, args):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=900) for _ in procs)
    finally:
        for p in procs:
            p.join(120)
            if p.is_alive():
                p.kill()
    return res


def _check_ranks(one, world, nout, res):
    vname, vfx, fx, bam, fa, contigs, out, argv, n_one = one
    assert all(isinstance(v, dict) for v in res.values()), res
    _check_vcf(nout + ".vcf", vfx, res[0]["cmd"])
    assert _without_cmd(nout + ".vcf") == _without_cmd(out + ".vcf")
    for rel in OUTPUTS + ["_tiddit/clips/%s.fa" % n for n, ln in contigs if ln >= fx["params"]["min_contig"]]:
        assert open(nout + rel, "rb").read() == open(out + rel, "rb").read(), rel
    rows = [l.rstrip("\n").split("\t") for l in open(nout + ".candidates.tab") if not l.startswith("#")]
    assert rows == _candidate_rows(fx)
    for r in range(world):
        assert res[r]["live_none"], r
        assert len(res[r]["sizes"]) == 1, (r, res[r]["sizes"])          # one store per rank: its scan's, taken by the stage
        assert "region counts (N ranks: broadcast, one launch per rank, reduce)" in res[r]["stages"]
    shares = [res[r]["sizes"][0] for r in range(world)]
    assert sum(shares) == n_one and max(shares) < n_one, (shares, n_one)


@pytest.mark.parametrize("world", [2, 3])
def test_cli_vcf_on_n_ranks(one, tmp_path, world):
    vname = one[0]
    if (vname, world) not in (("sv_vcf_small.json", 2), ("sv_vcf_small.json", 3), ("sv_vcf.json", 2), ("sv_vcf_grch38.json", 3)):
        pytest.skip("the other fixture / world pairs cover it")
    nout = str(tmp_path / "ranks")
    res = _spawn(_vcf_rank, world, (one[7] + ["-o", nout], {}))
    _check_ranks(one, world, nout, res)


def test_cli_vcf_on_two_ranks_without_preingest(one, tmp_path):
    if one[0] != "sv_vcf_small.json":
        pytest.skip("the small fixture covers it")
    nout = str(tmp_path / "nopre")
    res = _spawn(_vcf_rank, 2, (one[7] + ["-o", nout], {"TIDDIT_DIST_PREINGEST": "0"}))
    _check_ranks(one, 2, nout, res)


def test_cli_vcf_over_real_rccl_with_one_rank(one, tmp_path):
    """TIDDIT_FORCE_DIST=1, WORLD_SIZE=1, backend nccl: the queries arrive by an RCCL broadcast into a device tensor, the device entry
    answers them, the counts leave by an RCCL reduce"""
    vname, vfx, fx, bam, fa, contigs, out, argv, n_one = one
    if vname == "sv_vcf.json":
        pytest.skip("the small and the GRCh38-shaped files cover it")
    nout = str(tmp_path / "rccl1")
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()), TIDDIT_FORCE_DIST="1",
               TIDDIT_INGEST_CHUNK=str(48 << 20), TIDDIT_VARIANTS="1")
    env.pop("TIDDIT_DIST_BACKEND", None)
    r = subprocess.run([sys.executable, "-m", "tiddit_amd"] + argv + ["-o", nout], cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    cmd = [l for l in open(nout + ".vcf").read().split("\n") if l.startswith("##TIDDITcmd=")]
    assert len(cmd) == 1
    _check_vcf(nout + ".vcf", vfx, cmd[0])
    assert _without_cmd(nout + ".vcf") == _without_cmd(out + ".vcf")


def _drop_in_rank(rank, world, port, q, one_args):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), TIDDIT_HIP_DEVICE="0",
                      TIDDIT_INGEST_CHUNK=str(1 << 20))
    import argparse
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tiddit_amd import tiddit_cluster, tiddit_gc, tiddit_signal, tiddit_variant
        from tiddit_amd.bamio import BamReader
        vfx, fx, bam, fa, out = one_args
        P = fx["params"]
        lib = dict(vfx["meta"]["library"])
        max_ins = vfx["meta"]["max_ins_len"]
        r = BamReader(bam, batch_bytes=1 << 20)
        header = r.header
        r.close()
        names = [c["SN"] for c in header["SQ"]]
        cand = cov = gc = args = None
        if rank == 0:                                               # (rank 0's inputs only: the other ranks hand in None)
            cov = tiddit_signal.scan_signals(bam, P["min_q"], max_ins, P["min_contig"], P["min_anchor_len"], P["min_clip_len"], 50)[2]
            gc = tiddit_gc.main(fa, names, 1, 50, 0.5)
            cand = tiddit_cluster.main(out, names, {c["SN"]: c["LN"] for c in header["SQ"]}, ["WGS"], lib["mp"], fx["epsilon"], P["m"], max_ins,
                                       P["min_contig"], True, P["min_reads"])
            args = argparse.Namespace(**dict(vfx["meta"]["args"], bam=bam, ref=fa, o=out))
        live = tiddit_variant.LIVE_STORE is None
        variants = tiddit_variant.main_sharded(bam, cand, args, lib if rank == 0 else None, P["min_q"], ["WGS"], cov,
                                               {n: i for i, n in enumerate(names)}, max_ins, gc)
        q.put((rank, {"live_none_before": live, "body": None if variants is None else tiddit_variant.vcf_body(names, variants),
                      "stages": sorted(tiddit_variant.STAGE_SECONDS)}))
    except BaseException:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_main_sharded_without_a_live_store(one):
    """tiddit_variant.main_sharded called on its own: every rank builds the store of its shard with one pass (seams checked)"""
    vname, vfx, fx, bam, fa, contigs, out, argv, n_one = one
    if vname != "sv_vcf_small.json":
        pytest.skip("the drop-in path runs on the small fixture")
    res = _spawn(_drop_in_rank, 2, ((vfx, fx, bam, fa, out),))
    assert all(isinstance(v, dict) for v in res.values()), res
    assert res[0]["body"] == _body(vfx) and res[1]["body"] is None
    for r in range(2):
        assert res[r]["live_none_before"]
        assert "evidence store (one ingest pass over this rank's shard)" in res[r]["stages"]
