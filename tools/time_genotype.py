"""What genotyping known sites (TIDDIT_GENOTYPE) adds to a `TIDDIT_VARIANTS=1 tiddit --sv --skip_assembly` job: the job with and
without the switch, interleaved, every run a fresh process on the same box, the sites being the job's own VCF.  Reported: the scan
stage's seconds of both (nothing new is enqueued during the scan: it must stay inside the spread of the interleaved runs), the job's
wall, and the new stage split into sites / links handle (upload + sort) / counts launches / column text; with --profile also
`rocprofv3 --kernel-trace --stats` of one more run with the switch, in a run of its own, for the new kernels.  Writes a markdown file.
--depth: what TIDDIT_GENOTYPE_DEPTH=1 adds instead — both columns run with TIDDIT_GENOTYPE, the second with the depth switch too;
the default output is profiles/genotype_depth_240mb.md and the kernel statistics are those of csrc/tdt_depth.hip and the medians.

usage: python tools/time_genotype.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--profile] [--depth] [--out profiles/genotype_240mb.md]
(--mb: bench.py's synthetic file of that genome size, made at $TIDDIT_BENCH_TMP/tiddit_bench_sv_<mb>/ when it is not there)"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
KERNELS = ("links_count", "lk_make_keys", "lk_pack", "rs_onesweep", "rs_hist_all", "region_counts_packed")
DEPTH_KERNELS = ("dp_windows_short", "dp_windows_long", "dp_class_medians", "med_hist", "med_pick", "seg_means")


def one(a):
    """the child: one job in this process, its stage seconds as JSON"""
    from tiddit_amd import __main__ as cli
    t0 = time.perf_counter()
    cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", a.o, "--skip_assembly", "--force_overwrite"])
    json.dump({"wall": time.perf_counter() - t0, "stages": cli.STAGE_SECONDS, "notes": cli.STAGE_NOTES}, open(a.one, "w"))


def child(a, out, sites, front=(), depth=False):
    env = dict(os.environ, TIDDIT_VARIANTS="1")
    env.pop("TIDDIT_GENOTYPE", None)
    env.pop("TIDDIT_GENOTYPE_DEPTH", None)
    if sites:
        env["TIDDIT_GENOTYPE"] = sites
    if depth:
        env["TIDDIT_GENOTYPE_DEPTH"] = "1"
    res = out + ".json"
    t0 = time.perf_counter()
    r = subprocess.run(list(front) + [sys.executable, os.path.abspath(__file__), "--one", res, "--bam", a.bam, "--ref", a.ref, "-o", out], cwd=REPO,
                       env=env, capture_output=True, text=True, timeout=1100)
    if r.returncode != 0:
        raise RuntimeError("the job failed: " + r.stdout[-1000:] + r.stderr[-3000:])
    rec = json.load(open(res))
    rec["process wall"] = time.perf_counter() - t0
    return rec


def main():
    from tools.time_cov_track import bench_file
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--depth", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--one")
    ap.add_argument("-o")
    a = ap.parse_args()
    if a.one:
        return one(a)
    if a.mb:
        a.bam, a.ref = bench_file(a.mb)
    if not a.bam or not a.ref:
        ap.error("--bam and --ref, or --mb")
    a.out = a.out or os.path.join(REPO, "profiles", "genotype_depth_240mb.md" if a.depth else "genotype_240mb.md")
    kernels = DEPTH_KERNELS if a.depth else KERNELS
    runs = {"off": [], "on": []}
    lines = []
    with tempfile.TemporaryDirectory() as d:
        first = os.path.join(d, "first")
        child(a, first, None)                             # (warms the page cache; its VCF is the sites file)
        sites = first + ".vcf"
        n_sites = sum(1 for l in open(sites) if not l.startswith("#"))
        for i in range(a.reps):
            for mode in ("off", "on"):
                runs[mode].append(child(a, os.path.join(d, "r%d%s" % (i, mode)), sites if a.depth or mode == "on" else None,
                                        depth=a.depth and mode == "on"))
        body = [[l for l in open(os.path.join(d, "r0%s.vcf" % m)) if not l.startswith("#")] for m in ("on", "off")]
        assert body[0] == body[1]                         # (the variant stage in front of the genotyping is what it was)
        stats = None
        rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        if a.profile and os.path.exists(rocprof):
            pd = os.path.join(d, "prof")
            child(a, os.path.join(d, "profiled"), sites, front=[rocprof, "--kernel-trace", "--stats", "-d", pd, "--output-format", "csv", "--"],
                  depth=a.depth)
            stats = []
            for path in glob.glob(os.path.join(pd, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    if any(k in row.get("Name", "") for k in kernels):
                        stats.append(row)

    def col(mode, key):
        return [r["stages"].get(key) for r in runs[mode] if r["stages"].get(key) is not None]

    def fmt(v):
        return "-" if not v else "%.4f (%.4f .. %.4f)" % (statistics.median(v), min(v), max(v))
    new = [k for k in runs["on"][0]["stages"] if k not in runs["off"][0]["stages"]]
    what = ("TIDDIT_GENOTYPE_DEPTH", "`TIDDIT_VARIANTS=1 TIDDIT_GENOTYPE={its own VCF} tiddit --sv --skip_assembly` with and without "
            "`TIDDIT_GENOTYPE_DEPTH=1`") if a.depth else ("TIDDIT_GENOTYPE", "`TIDDIT_VARIANTS=1 tiddit --sv --skip_assembly` with and without "
                                                          "`TIDDIT_GENOTYPE={its own VCF}`")
    lines += ["# %s on the %s job (tools/time_genotype.py)" % (what[0], os.path.basename(os.path.dirname(a.bam) or a.bam)), "",
              "%s, %d interleaved runs each, every run a "
              "fresh process; BAM %.0f MB, %d sites.  Seconds: median (min .. max)." % (what[1], a.reps, os.path.getsize(a.bam) / 1e6, n_sites), "",
              "| | without the switch | with the switch |", "|---|---|---|"]
    for key in ("library statistics", "signal extraction + coverage", "clustering", "variant typing (native)") + \
            (("genotyping of known sites ({o}.genotyped.vcf)",) if a.depth else ()):
        lines.append("| %s | %s | %s |" % (key, fmt(col("off", key)), fmt(col("on", key))))
    lines.append("| job wall (inside the process) | %s | %s |" % (fmt([r["wall"] for r in runs["off"]]), fmt([r["wall"] for r in runs["on"]])))
    lines.append("| process wall (interpreter, imports, first touch of the device) | %s | %s |" % (fmt([r["process wall"] for r in runs["off"]]),
                                                                                                  fmt([r["process wall"] for r in runs["on"]])))
    lines += ["", "The new stage:", "", "| | seconds |", "|---|---|"]
    for key in new:
        lines.append("| %s | %s |" % (key.replace("  ", "&nbsp;&nbsp;"), fmt(col("on", key))))
    lines += ["", "notes of the last run with the switch: `%s`" % json.dumps(runs["on"][-1]["notes"]), ""]
    if stats is not None:
        lines += ["`rocprofv3 --kernel-trace --stats`, one more run with the switch (a run of its own):", ""]
        if stats:
            keys = [k for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in stats[0]]
            lines += ["| " + " | ".join(keys) + " |", "|" + "---|" * len(keys)]
            lines += ["| " + " | ".join(str(r[k])[:90] for k in keys) + " |" for r in stats]
        else:
            lines.append("(no kernel statistics were found in the profiler's output)")
        lines.append("")
    open(a.out, "w").write("\n".join(lines))
    print(json.dumps({"out": a.out, "sites": n_sites, "runs": runs}))


if __name__ == "__main__":
    main()
