"""`TIDDIT_COV_TRACK=Z[:Q[:bed|wig]]` on the GPU: `tiddit --sv` writes, from its own scan of the file, the coverage file that
`tiddit --cov -z Z -q Q [-w]` writes for the same BAM.  The partner of every comparison is `--cov` through ``run_cov`` — whose bytes are
pinned to the compiled reference in tests/test_gpu_pipeline.py and tests/test_gpu_parity.py — never the code under test alone; every
comparison is exact (bytes or sha256).  Below the file level, the second coverage-record column the ingest kernel writes is compared
record for record with ``tdt_cov_pack_binned_device`` / ``tdt_cov_pack_device`` on the same batch's field arrays.

``test_track_equals_cov_and_the_scan_is_undisturbed`` is the test that fails without the feature: the parent commit writes no
``{o}.bed`` / ``{o}.wig`` from ``--sv``."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cluster_oracle

from sv_e2e_common import load_fixture, materialise
from test_gpu_variant import PAIRS, _candidate_rows, _check_vcf

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ["_tiddit/discordants_WGS.tab", "_tiddit/splits_WGS.tab", "_tiddit/clips_WGS.fa", ".ploidies.tab", ".candidates.tab"]
# the default everyone uses; the small-bin kernel flavour with no mapq cut, as wig; a bin size without a binned form (generic packed
# records); the scan's own parameters (two histograms with the same spec)
TRACKS = ["500", "100:0:wig", "2000:20", "50:5"]
VCF_OF = {e: v for v, e in PAIRS.items()}


def sha(data):
    return hashlib.sha256(data if isinstance(data, bytes) else data.encode()).hexdigest()


def _port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spec(track):
    from tiddit_amd.__main__ import parse_cov_track
    return parse_cov_track(track)


class Files:
    """one fixture's BAM + FASTA, and the files `--cov` writes for it (made once per parameter set)"""

    def __init__(self, fx, name, directory):
        self.fx, self.name, self.dir = fx, name, directory
        self.bam, self.fa, self.contigs = materialise(fx, directory, threads=min(16, os.cpu_count() or 1))
        self._cov = {}
        self.n = 0

    def sv_argv(self, out, extra=()):
        return ["--sv", "--bam", self.bam, "--ref", self.fa, "-o", out, "--skip_assembly", "-s", str(self.fx["params"]["n_reads_stats"])] + list(extra)

    def fresh(self, tag):
        self.n += 1
        return os.path.join(self.dir, "%s%d" % (tag, self.n))

    def cov_bytes(self, track):
        """the bytes of `--cov -z Z -q Q [-w] -o other` (run_cov, in this process) for the track's parameters"""
        z, q, fmt = _spec(track)
        if (z, q, fmt) not in self._cov:
            from tiddit_amd import __main__ as cli
            assert "TIDDIT_COV_TRACK" not in os.environ
            other = self.fresh("cov")
            cli.main(["--cov", "--bam", self.bam, "-o", other, "-z", str(z), "-q", str(q)] + (["-w"] if fmt == "wig" else []))
            data = open(other + "." + fmt, "rb").read()
            assert len(data) > 100 and not os.path.exists(other + (".bed" if fmt == "wig" else ".wig"))
            self._cov[(z, q, fmt)] = data
        return self._cov[(z, q, fmt)]


_FILES = {}          # fixture name -> Files: made once per session, whichever parametrisation asks for it


@pytest.fixture(scope="module", params=["sv_e2e_small.json", "sv_e2e.json", "sv_e2e_grch38.json"])
def files(request, golden_dir, tmp_path_factory):
    """the 3-Mb, the 24-Mb and the GRCh38-shaped end-to-end fixtures (a test that names its own files parametrises this fixture indirectly)"""
    if request.param not in _FILES:
        _FILES[request.param] = Files(load_fixture(golden_dir, request.param), request.param, str(tmp_path_factory.mktemp("covtrack")))
    return _FILES[request.param]


def _track_path(out, track):
    return out + "." + _spec(track)[2]


def _check_sv_outputs(F, out):
    """what tests/test_gpu_sv_e2e.py compares of a `--sv` run, against the fixture: signal tables, clips, ploidy table, candidates"""
    from tiddit_amd import tiddit_cluster
    fx, P = F.fx, F.fx["params"]
    assert sha(open(out + "_tiddit/discordants_WGS.tab").read()) == fx["discordants_sha256"]
    assert sha(open(out + "_tiddit/splits_WGS.tab").read()) == fx["splits_sha256"]
    assert sha(open(out + "_tiddit/clips_WGS.fa").read()) == fx["clips_sha256"]
    assert open(out + ".ploidies.tab").read() == fx["ploidies_tab"]
    rows = [l.rstrip("\n").split("\t") for l in open(out + ".candidates.tab") if not l.startswith("#")]
    assert rows == _candidate_rows(fx)
    cand = tiddit_cluster.main(out, [n for n, _ in F.contigs], dict(F.contigs), ["WGS"], fx["library"]["mp"], fx["epsilon"], P["m"],
                               fx["library"]["percentile_insert_size"], P["min_contig"], True, P["min_reads"])
    assert cluster_oracle.summary(cand) == fx["candidates"]
    assert sha(cluster_oracle.canonical(cand)) == fx["candidates_sha256"]


# ---- 1, 2, 6: one process -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track", TRACKS)
def test_track_equals_cov_and_the_scan_is_undisturbed(files, track, monkeypatch):
    """`--sv --skip_assembly` with the switch on: the track file is the file `--cov` writes, byte for byte; and every output the
    end-to-end test compares still equals the fixture.  (Fails on the parent commit: no such file is written there.)"""
    from tiddit_amd import __main__ as cli, tiddit_signal
    F = files
    want = F.cov_bytes(track)
    out = F.fresh("sv")
    monkeypatch.setenv("TIDDIT_COV_TRACK", track)
    cli.main(F.sv_argv(out))
    assert os.path.exists(_track_path(out, track)), "--sv wrote no coverage track"
    got = open(_track_path(out, track), "rb").read()
    assert sha(got) == sha(want) and got == want
    assert not os.path.exists(out + (".wig" if _spec(track)[2] == "bed" else ".bed"))
    assert tiddit_signal.COV_TRACK is None and tiddit_signal.COV_TRACK_BINS is None          # (the request does not outlive the job)
    assert any(k.startswith("coverage track") for k in cli.STAGE_SECONDS)
    assert any("coverage track push" in k for k in cli.STAGE_SECONDS)
    _check_sv_outputs(F, out)


@pytest.mark.parametrize("track", TRACKS)
def test_library_level_scan_keeps_the_50bp_bins_and_leaves_the_track_bins(files, track, tmp_path):
    """a caller who drives the modules himself: ``tiddit_signal.COV_TRACK = (Z, Q)`` before the scan, the bins in
    ``tiddit_signal.COV_TRACK_BINS`` behind it — formatted by print_coverage they are `--cov`'s file; the 50-bp coverage of every
    contig keeps the fixture's sha (the second histogram does not disturb the first)"""
    from tiddit_amd import tiddit_coverage, tiddit_signal
    F = files
    fx, P = F.fx, F.fx["params"]
    z, q, fmt = _spec(track)
    want = F.cov_bytes(track)
    tiddit_signal.COV_TRACK = (z, q)
    try:
        header, chroms, cov, data, splits, clips = tiddit_signal.scan_signals(F.bam, P["min_q"], fx["library"]["percentile_insert_size"],
                                                                              P["min_contig"], P["min_anchor_len"], P["min_clip_len"], 50)
    finally:
        tiddit_signal.COV_TRACK = None
    assert list(cov) == list(fx["coverage_sha256"])
    for c in cov:
        assert sha(cov[c].astype("<f8").tobytes()) == fx["coverage_sha256"][c], c
    bins = tiddit_signal.COV_TRACK_BINS
    assert bins is not None and list(bins) == [n for n, _ in F.contigs]
    path = str(tmp_path / ("lib." + fmt))
    tiddit_coverage.print_coverage(bins, header, z, fmt, path)
    assert open(path, "rb").read() == want
    # ... and a scan without the request leaves none
    tiddit_signal.scan_signals(F.bam, P["min_q"], fx["library"]["percentile_insert_size"], P["min_contig"], P["min_anchor_len"], P["min_clip_len"], 50)
    assert tiddit_signal.COV_TRACK_BINS is None and not any("track" in k for k in tiddit_signal.SCAN_SECONDS)


def test_switch_unset_writes_no_track(files, monkeypatch):
    from tiddit_amd import __main__ as cli, tiddit_signal
    F = files
    monkeypatch.delenv("TIDDIT_COV_TRACK", raising=False)
    out = F.fresh("off")
    cli.main(F.sv_argv(out))
    assert not os.path.exists(out + ".bed") and not os.path.exists(out + ".wig")
    assert not any("track" in k for k in cli.STAGE_SECONDS) and tiddit_signal.COV_TRACK is None
    assert sha(open(out + "_tiddit/discordants_WGS.tab").read()) == F.fx["discordants_sha256"]


# ---- 3: together with the variant stage --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track", ["500", "100:0:wig"])
def test_track_beside_the_vcf(files, track, golden_dir, monkeypatch):
    from tiddit_amd import __main__ as cli
    F = files
    vfx = json.load(open(os.path.join(golden_dir, VCF_OF[F.name])))
    want = F.cov_bytes(track)
    out = F.fresh("vcf")
    monkeypatch.setenv("TIDDIT_COV_TRACK", track)
    monkeypatch.setenv("TIDDIT_VARIANTS", "1")
    cli.main(F.sv_argv(out))
    _check_vcf(out + ".vcf", vfx, '##TIDDITcmd="' + " ".join(sys.argv) + '"')
    assert open(_track_path(out, track), "rb").read() == want


# ---- 5: the head of the file, consumed by the statistics pass and carried into the scan ---------------------------------------------
@pytest.mark.parametrize("track", ["500", "2000:20"])
@pytest.mark.parametrize("mode", ["fixture -s, short spans", "small -s, short spans", "fixture -s"])
def test_batches_carried_from_the_statistics_pass_reach_the_track(files, track, mode, monkeypatch):
    """the statistics pass keeps the batches it sampled (carry=True) and the scan starts from them: they carry the second column, written
    for the track's histogram, and the track equals `--cov`'s file — with the file in one span's worth of batches and cut into many
    short spans, with the fixture's -s and with a small one"""
    from tiddit_amd import __main__ as cli, bamio
    F = files
    want = F.cov_bytes(track)
    z = _spec(track)[0]
    seen = []
    real = bamio.take_carry

    def spy(*a, **k):
        c = real(*a, **k)
        if c is not None:
            seen.append((len(c.batches), c.hist2 is not None and c.hist2.bin_size == z,
                         all(b.second_for is c.hist2 and b.dev.get("packed2") for b in c.batches)))
        return c
    monkeypatch.setattr(bamio, "take_carry", spy)
    monkeypatch.setenv("TIDDIT_COV_TRACK", track)
    if "short spans" in mode:
        monkeypatch.setenv("TIDDIT_INGEST_CHUNK", str(1 << 20))
    out = F.fresh("carry")
    argv = F.sv_argv(out)
    if mode.startswith("small -s"):
        argv[argv.index("-s") + 1] = "20000"
    cli.main(argv)
    assert len(seen) == 1 and seen[0][0] >= 1 and seen[0][1] and seen[0][2], seen
    assert open(_track_path(out, track), "rb").read() == want


def test_a_carry_without_the_second_column_still_reaches_the_track(files, tmp_path):
    """library level: a statistics pass that was not told about the track leaves batches with no second column; the scan pushes those
    through their field arrays — same bins"""
    from tiddit_amd import bamio, tiddit_coverage, tiddit_signal, tiddit_stats
    F = files
    fx, P = F.fx, F.fx["params"]
    want = F.cov_bytes("500")
    os.environ["TIDDIT_INGEST_CHUNK"] = str(1 << 20)
    try:
        lib = tiddit_stats.statistics(F.bam, F.fa, P["min_q"], 100000, P["n_reads_stats"], carry=True)
        tiddit_signal.COV_TRACK = (500, 20)
        header = tiddit_signal.scan_signals(F.bam, P["min_q"], lib["percentile_insert_size"], P["min_contig"], P["min_anchor_len"], P["min_clip_len"], 50)[0]
    finally:
        os.environ.pop("TIDDIT_INGEST_CHUNK", None)
        tiddit_signal.COV_TRACK = None
        bamio.set_carry(None)
    path = str(tmp_path / "nocol.bed")
    tiddit_coverage.print_coverage(tiddit_signal.COV_TRACK_BINS, header, 500, "bed", path)
    assert open(path, "rb").read() == want


# ---- 4: N ranks ---------------------------------------------------------------------------------------------------------------------
def _track_rank(rank, world, port, q, argv, env):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      TIDDIT_HIP_DEVICE="0", TIDDIT_DIST_BACKEND="gloo", TIDDIT_INGEST_CHUNK=str(48 << 20), **env)
    try:
        import torch.distributed as dist
        from tiddit_amd import __main__ as cli, tiddit_coverage
        written = []
        real = tiddit_coverage.print_coverage

        def spy(coverage_data, bam_header, bin_size, file_type, outfile):
            written.append(outfile)
            return real(coverage_data, bam_header, bin_size, file_type, outfile)
        tiddit_coverage.print_coverage = spy
        cli.main(argv)
        q.put((rank, {"written": written, "notes": dict(cli.STAGE_NOTES)}))
        if dist.is_initialized():
            dist.destroy_process_group()
    except BaseException:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def _spawn(world, args, timeout=600):
    """fresh child processes, one per rank; every wait has its own time limit and the first failure ends the test"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_track_rank, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=timeout) for _ in procs)
    finally:
        for p in procs:
            p.join(120)
            if p.is_alive():
                p.kill()
    return res


RANK_CASES = [("sv_e2e_small.json", t) for t in TRACKS] + [("sv_e2e.json", "500"), ("sv_e2e_grch38.json", "500"), ("sv_e2e_grch38.json", "2000:20")]


@pytest.mark.parametrize("files,track", RANK_CASES, indirect=["files"])
def test_track_on_two_ranks_sharing_the_gpu(files, track):
    """two ranks over gloo on the one GPU: byte-range shards, the track's bins through the same exact all-reduce as the 50-bp bins, the
    file written by rank 0 only — `--cov`'s bytes; the ranks other than 0 start from batches they ingested beside rank 0's statistics"""
    F = files
    want = F.cov_bytes(track)
    nout = F.fresh("ranks")
    res = _spawn(2, (F.sv_argv(nout), {"TIDDIT_COV_TRACK": track}))
    assert all(isinstance(v, dict) for v in res.values()), res
    assert res[0]["written"] == [_track_path(nout, track)] and res[1]["written"] == []
    assert open(_track_path(nout, track), "rb").read() == want
    assert sha(open(nout + "_tiddit/discordants_WGS.tab").read()) == F.fx["discordants_sha256"]
    assert open(nout + ".ploidies.tab").read() == F.fx["ploidies_tab"]


@pytest.mark.parametrize("files", ["sv_e2e_small.json", "sv_e2e_grch38.json"], indirect=True)
def test_track_on_two_ranks_with_the_vcf(files):
    F = files
    want = F.cov_bytes("500")
    nout = F.fresh("ranksvcf")
    res = _spawn(2, (F.sv_argv(nout), {"TIDDIT_COV_TRACK": "500", "TIDDIT_VARIANTS": "1"}))
    assert all(isinstance(v, dict) for v in res.values()), res
    assert open(nout + ".bed", "rb").read() == want and os.path.exists(nout + ".vcf")
    rows = [l.rstrip("\n").split("\t") for l in open(nout + ".candidates.tab") if not l.startswith("#")]
    assert rows == _candidate_rows(F.fx)


@pytest.mark.parametrize("track", ["500", "100:0:wig"])
def test_track_over_real_rccl_with_one_rank(files, track):
    """TIDDIT_FORCE_DIST=1, WORLD_SIZE=1, backend nccl: the N-rank path with the all-reduce of the track's bins a real RCCL call"""
    F = files
    want = F.cov_bytes(track)
    nout = F.fresh("rccl")
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()), TIDDIT_FORCE_DIST="1",
               TIDDIT_INGEST_CHUNK=str(48 << 20), TIDDIT_COV_TRACK=track)
    env.pop("TIDDIT_DIST_BACKEND", None)
    r = subprocess.run([sys.executable, "-m", "tiddit_amd"] + F.sv_argv(nout), cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(_track_path(nout, track), "rb").read() == want
    assert sha(open(nout + "_tiddit/splits_WGS.tab").read()) == F.fx["splits_sha256"]


# ---- the record layout, below the file level ------------------------------------------------------------------------------------------
_FIRST_COLUMN = {}       # fixture name -> the first column of every batch, decoded with no second histogram attached


@pytest.mark.parametrize("z", [100, 128, 129, 500, 1023, 1, 1024, 2000])
def test_second_column_record_for_record(files, z):
    """decode the fixture's BAM with a second histogram attached: the second column equals, record for record, what
    tdt_cov_pack_binned_device writes for that histogram from the batch's start / end / mapq / flag arrays (bin sizes of both kernel
    flavours: <= 128 and 129..1023) or — a bin size without a binned form — what tdt_cov_pack_device writes; the first column is what
    it is with nothing attached"""
    import torch
    from tiddit_amd import _native, bamio, tiddit_coverage
    F = files
    chunk = 8 << 20

    def read(second):
        rd = bamio.DeviceBamReader(F.bam, chunk=chunk, split_small=False)
        h50 = tiddit_coverage.CoverageHistogram(rd.header, 50, ctx=rd.ctx)
        h2 = tiddit_coverage.CoverageHistogram(rd.header, z, ctx=rd.ctx) if second else None
        assert rd.bin_for(h50)
        if second:
            assert rd.second_for(h2) == (2 <= z < 1024) == h2.has_binned()
        try:
            for b in rd.batches():
                yield rd, h2, b
        finally:
            rd.close()
            h50.close()
            if h2 is not None:
                h2.close()

    if F.name not in _FIRST_COLUMN:             # (the same for every z: read once per file)
        _FIRST_COLUMN[F.name] = []
        for rd, _, b in read(False):
            assert "packed2" not in b.dev and b.second_for is None
            _FIRST_COLUMN[F.name].append(b.packed.copy())
    first = _FIRST_COLUMN[F.name]
    assert len(first) >= 2
    dev = torch.device("cuda", _native.default_context().device)
    k, unplaced = 0, 0
    for rd, h2, b in read(True):
        n, d = len(b), b.dev
        assert d["packed2"] and b.second_for is h2 and b.second_binned == h2.has_binned()
        assert np.array_equal(b.packed, first[k]), "the first column changed with a second histogram attached"
        k += 1
        got = b.packed2
        want = torch.zeros(n, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        if h2.has_binned():
            for t, lo, hi in b.runs:
                if t >= 0:
                    h2.pack_binned_device(t, d["pos"] + 4 * lo, d["end"] + 4 * lo, d["mapq"] + lo, d["flag"] + 2 * lo, hi - lo, want.data_ptr() + 8 * lo)
        else:
            _native.check(rd.ctx.lib.tdt_cov_pack_device(rd.ctx.handle, d["pos"], d["end"], d["mapq"], d["flag"], n, want.data_ptr()))
        rd.ctx.sync()
        want = want.cpu().numpy().view(np.uint64)
        for t, lo, hi in b.runs:
            if t >= 0 or not h2.has_binned():
                assert np.array_equal(got[lo:hi], want[lo:hi]), (z, t, lo, hi)
            else:
                # unplaced reads have no contig whose bins could be packed: the kernel writes the INVALID shape, bin 0, and the filter byte
                unplaced += hi - lo
                top = (np.minimum(b.mapq[lo:hi].astype(np.uint64), 63) << np.uint64(24)) | \
                      (((b.flag[lo:hi].astype(np.uint64) >> np.uint64(2)) & np.uint64(1)) << np.uint64(30)) | \
                      (((b.flag[lo:hi].astype(np.uint64) >> np.uint64(10)) & np.uint64(1)) << np.uint64(31))
                assert np.array_equal(got[lo:hi], (top << np.uint64(32)) | np.uint64(3)), (z, lo, hi)
    assert k == len(first)
    if F.name == "sv_e2e_grch38.json":
        assert unplaced > 0 or not (2 <= z < 1024)
