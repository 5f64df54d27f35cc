"""What the depth distributions of `tiddit --sv` (TIDDIT_DEPTH_DIST=1) cost the job: `tiddit --sv --skip_assembly` with the switch off
and on, interleaved, in one process — the stage's seconds (the launch and the text apart), the scan stage's wall (the store is packed
only with the switch on) and the whole job's wall.  Writes the record to profiles/depth_dist_<mb>mb.md (or --out) and prints one JSON
line.  With --profile nothing is written: one warm-up and one run each way, for a `rocprofv3 --kernel-trace --stats -- python
tools/time_depth_dist.py ... --profile` run whose kernel table goes beside the record.

usage: python tools/time_depth_dist.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--profile] [--out FILE.md]
(--mb: bench.py's synthetic file of that genome size, made at $TIDDIT_BENCH_TMP/tiddit_bench_sv_<mb>/ when it is not there)"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from time_cov_track import bench_file  # noqa: E402  (the same synthetic file)

STAGE = "depth distribution ({o}.depth_dist.tab, {o}.depth_summary.tab)"
LAUNCH = "  depth distribution launch (device, one launch over all contigs)"
TEXT = "  depth distribution text (host)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="one warm-up and one run each way, no record written (for rocprofv3)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mb:
        a.bam, a.ref = bench_file(a.mb)
    if not a.bam or not a.ref:
        ap.error("--bam and --ref, or --mb")
    if a.profile:
        a.reps = 1
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native
    ctx = _native.default_context()
    runs = {"off": [], "on": []}
    summary = None
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode in ("off", "on"):
                out = os.path.join(d, "r%d%s" % (i, mode))
                os.environ.pop("TIDDIT_DEPTH_DIST", None)
                if mode == "on":
                    os.environ["TIDDIT_DEPTH_DIST"] = "1"
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(io.StringIO()):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    os.environ.pop("TIDDIT_DEPTH_DIST", None)
                S = cli.STAGE_SECONDS
                rec = {"wall": time.perf_counter() - t0, "scan stage": S.get("signal extraction + coverage"), "stage": S.get(STAGE),
                       "launch": S.get(LAUNCH), "text": S.get(TEXT)}
                assert os.path.exists(out + ".depth_dist.tab") == (mode == "on")
                if i:
                    runs[mode].append(rec)
                if mode == "on" and i == a.reps:
                    summary = open(out + ".depth_summary.tab").read().rstrip("\n").split("\n")[-1]

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "total row of the summary": summary,
           "median_s": {"job wall, off": med("off", "wall"), "job wall, on": med("on", "wall"), "scan stage, off": med("off", "scan stage"),
                        "scan stage, on": med("on", "scan stage"), "on: stage": med("on", "stage"), "on: launch": med("on", "launch"),
                        "on: text": med("on", "text")},
           "runs": runs}
    print(json.dumps(res))
    if a.profile:
        return
    path = a.out or os.path.join(REPO, "profiles", "depth_dist_%dmb.md" % a.mb if a.mb else "depth_dist.md")
    rows = [("whole job, switch off", "off", "wall"), ("whole job, switch on", "on", "wall"),
            ("scan stage (\"signal extraction + coverage\"), switch off", "off", "scan stage"),
            ("scan stage, switch on (packs the evidence store)", "on", "scan stage"), ("on: the depth-distribution stage", "on", "stage"),
            ("on: its launch (`tdt_depth_dist`, synchronised)", "on", "launch"), ("on: its text (the two files)", "on", "text")]
    with open(path, "w") as f:
        f.write("# The depth distributions of `tiddit --sv` (`TIDDIT_DEPTH_DIST=1`)\n\n")
        f.write("File: `%s` (%.0f MB).  `tools/time_depth_dist.py`: one process, after one warm-up round %d rounds of { `--sv --skip_assembly` "
                "switch off, the same with the switch on }, interleaved.  Wall seconds; no budget was fixed in advance, this is what was "
                "measured.\n\n" % (os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for label, mode, key in rows:
            f.write("| %s | %s | %.4f |\n" % (label, " | ".join("%.4f" % r[key] for r in runs[mode]), med(mode, key)))
        f.write("\nThe `total` row of the last run's `depth_summary.tab` (length, sum of depths, mean, min, max): `%s`\n" % summary)


if __name__ == "__main__":
    main()
