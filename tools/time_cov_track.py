"""What the coverage track of `tiddit --sv` (TIDDIT_COV_TRACK) costs the job, and what it saves: `tiddit --sv --skip_assembly` with the
switch off and on, interleaved, in one process — the scan stage's wall, the whole job's wall, the scan's time in the second
histogram's push and the time to write the file — and what a user pays for the same file today: a separate `tiddit --cov` on the same
BAM, in this process (warm library, warm buffers) and, with --child, as a fresh `python -m tiddit_amd --cov` process (interpreter,
imports and the device's first touch included).  The track of the last "on" run is compared with `--cov`'s file, byte for byte.
One JSON line.

usage: python tools/time_cov_track.py (--bam WGS.bam --ref ref.fa | --mb 240) [--track 500] [--reps 3] [--child]
(--mb: bench.py's synthetic file of that genome size, made at $TIDDIT_BENCH_TMP/tiddit_bench_sv_<mb>/ when it is not there)"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def bench_file(mb):
    from tiddit_amd import synth_bam
    d = os.path.join(os.environ.get("TIDDIT_BENCH_TMP", "/tmp"), "tiddit_bench_sv_%d" % mb)
    bam, fa = os.path.join(d, "WGS.bam"), os.path.join(d, "ref.fa")
    if not (os.path.exists(bam) and os.path.exists(fa)):
        os.makedirs(d, exist_ok=True)
        contigs = synth_bam.wgs_contigs(mb)
        seqs = synth_bam.write_fasta(fa, contigs)
        synth_bam.write_wgs_sv_bam(bam + ".tmp", contigs, threads=min(16, os.cpu_count() or 1), ref_seqs=seqs)
        os.replace(bam + ".tmp", bam)
    return bam, fa


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--track", default="500")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", action="store_true", help="also time a fresh `python -m tiddit_amd --cov` process per repetition")
    a = ap.parse_args()
    if a.mb:
        a.bam, a.ref = bench_file(a.mb)
    if not a.bam or not a.ref:
        ap.error("--bam and --ref, or --mb")
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native, tiddit_signal
    z, q, fmt = cli.parse_cov_track(a.track)
    cov_argv = ["--cov", "--bam", a.bam, "-z", str(z), "-q", str(q)] + (["-w"] if fmt == "wig" else [])
    ctx = _native.default_context()
    runs = {"off": [], "on": [], "cov": [], "cov_child": []}
    same = None
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode in ("off", "on", "cov") + (("cov_child",) if a.child else ()):
                out = os.path.join(d, "r%d%s" % (i, mode))
                os.environ.pop("TIDDIT_COV_TRACK", None)
                rec = {}
                t0 = time.perf_counter()
                if mode in ("off", "on"):
                    if mode == "on":
                        os.environ["TIDDIT_COV_TRACK"] = a.track
                    with contextlib.redirect_stdout(io.StringIO()):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                    rec["wall"] = time.perf_counter() - t0
                    S = cli.STAGE_SECONDS
                    rec["scan stage"] = S.get("signal extraction + coverage")
                    rec["library statistics"] = S.get("library statistics")
                    rec["scan: coverage push"] = tiddit_signal.SCAN_SECONDS.get("coverage push")
                    rec["scan: coverage track push"] = tiddit_signal.SCAN_SECONDS.get("coverage track push (second histogram)")
                    rec["track file written"] = next((v for k, v in S.items() if k.startswith("coverage track")), None)
                elif mode == "cov":
                    cli.main(cov_argv + ["-o", out])
                    ctx.sync()
                    rec["wall"] = time.perf_counter() - t0
                else:
                    env = dict(os.environ)
                    env.pop("TIDDIT_COV_TRACK", None)
                    r = subprocess.run([sys.executable, "-m", "tiddit_amd"] + cov_argv + ["-o", out], cwd=REPO, env=env, capture_output=True,
                                       text=True, timeout=900)
                    if r.returncode != 0:
                        raise RuntimeError("the --cov child failed: " + r.stderr[-2000:])
                    rec["wall"] = time.perf_counter() - t0
                os.environ.pop("TIDDIT_COV_TRACK", None)
                if i:
                    runs[mode].append(rec)
            if i == a.reps:
                same = open(os.path.join(d, "r%don.%s" % (i, fmt)), "rb").read() == open(os.path.join(d, "r%dcov.%s" % (i, fmt)), "rb").read()
                assert not os.path.exists(os.path.join(d, "r%doff.%s" % (i, fmt)))

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    out = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "track": a.track, "reps": a.reps, "track_equals_cov_file": same,
           "median_s": {"scan stage, off": med("off", "scan stage"), "scan stage, on": med("on", "scan stage"),
                        "job wall, off": med("off", "wall"), "job wall, on": med("on", "wall"),
                        "separate --cov, in process": med("cov", "wall"), "separate --cov, fresh process": med("cov_child", "wall"),
                        "on: scan's time in the second push": med("on", "scan: coverage track push"),
                        "on: track file written": med("on", "track file written")},
           "runs": runs}
    print(json.dumps(out))
    if not same:
        raise SystemExit("the track differs from --cov's file")


if __name__ == "__main__":
    main()
