"""What the copy-number segments of `tiddit --sv` (TIDDIT_CNV) cost the job: `tiddit --sv --skip_assembly` with the switch off, with
W = 500 and with W = 50, interleaved, in one process — the stage's seconds and its parts (medians, upload, expected depth, the bins
launch, the five segmentation launches, segments, text) beside the whole job's wall.  Writes the record to profiles/cnv_<mb>mb.md (or
--out) and prints one JSON line.  With --profile nothing is written: one warm-up and one run each way, for a `rocprofv3 --kernel-trace
--stats -- python tools/time_cnv.py ... --profile` run of its own; --kernels FILE_kernel_stats.csv then puts that run's rows of the
cnv_* kernels into the record.  No threshold is set here: the record is what was measured.

usage: python tools/time_cnv.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--profile] [--kernels FILE.csv] [--out FILE.md]
(--mb: bench.py's synthetic file of that genome size, made at $TIDDIT_BENCH_TMP/tiddit_bench_sv_<mb>/ when it is not there)"""
import argparse
import contextlib
import csv
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

STAGE = "copy-number segments ({o}.cnv.bed)"
MODES = (("off", None), ("W=500", "500"), ("W=50", "50"))
KERNELS = ("cnv_bins_kernel", "cnv_chunk_matrices", "cnv_carry", "cnv_backpointers", "cnv_chunk_ends", "cnv_backtrace")


def kernel_rows(path):
    """the cnv_* rows of a rocprofv3 kernel_stats.csv -> [(name, calls, total ns, average ns)]"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            k = next((k for k in KERNELS if k in name), None)
            if k:
                rows.append((k, r.get("Calls"), r.get("TotalDurationNs"), r.get("AverageNs")))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="one warm-up and one run each way, no record written (for rocprofv3)")
    ap.add_argument("--kernels", help="a rocprofv3 kernel_stats.csv of a --profile run: its cnv_* rows go into the record")
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
    runs = {m: [] for m, _ in MODES}
    parts = []
    lines = {}
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode, value in MODES:
                out = os.path.join(d, "r%d%s" % (i, mode.replace("=", "")))
                os.environ.pop("TIDDIT_CNV", None)
                if value:
                    os.environ["TIDDIT_CNV"] = value
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(io.StringIO()):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    os.environ.pop("TIDDIT_CNV", None)
                S = cli.STAGE_SECONDS
                rec = {"wall": time.perf_counter() - t0, "stage": S.get(STAGE)}
                rec.update({k.strip(): v for k, v in S.items() if k.startswith("  CNV ")})
                assert os.path.exists(out + ".cnv.bed") == (value is not None)
                if i:
                    runs[mode].append(rec)
                if value and i == a.reps:
                    lines[mode] = open(out + ".cnv.bed").read().count("\n") - 1
                    parts = [k for k in rec if k.startswith("CNV ")]

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "segments": lines,
           "median_s": {m: {k: med(m, k) for k in ["wall", "stage"] + parts} for m, _ in MODES}, "runs": runs}
    print(json.dumps(res))
    if a.profile:
        return
    path = a.out or os.path.join(REPO, "profiles", "cnv_%dmb.md" % a.mb if a.mb else "cnv.md")
    with open(path, "w") as f:
        f.write("# The copy-number segments of `tiddit --sv` (`TIDDIT_CNV`)\n\n")
        f.write("File: `%s` (%.0f MB).  `tools/time_cnv.py`: one process, after one warm-up round %d rounds of { `--sv --skip_assembly` switch "
                "off, `TIDDIT_CNV=500`, `TIDDIT_CNV=50` }, interleaved.  Wall seconds; no budget was fixed in advance, this is what was "
                "measured.\n\n" % (os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode, _ in MODES:
            keys = ["wall"] if mode == "off" else ["wall", "stage"] + parts
            for key in keys:
                label = "whole job" if key == "wall" else "the stage" if key == "stage" else key
                f.write("| %s: %s | %s | %.4f |\n" % (mode, label, " | ".join("%.4f" % r[key] for r in runs[mode]), med(mode, key)))
        f.write("\nSegments written in the last round: %s\n" % ", ".join("%s: %d" % kv for kv in sorted(lines.items())))
        if a.kernels:
            f.write("\nKernels (`rocprofv3 --kernel-trace --stats`, a run of its own: one warm-up and one run each of off / W=500 / W=50, so two calls "
                    "at each bin size):\n\n| kernel | calls | total ns | average ns |\n|---|---|---|---|\n")
            for row in kernel_rows(a.kernels):
                f.write("| `%s` | %s | %s | %s |\n" % row)


if __name__ == "__main__":
    main()
