"""What the allele counts of `tiddit --sv` (TIDDIT_ALLELES) cost the job: `tiddit --sv --skip_assembly` with the switch off, with one
site per 1000 bp and with one site per 100 bp, interleaved, in one process — the whole job's wall, the scan stage, the new stage timer
(the pushes' host side), the host's reading of the sites file and the read-out beside them.  The yardstick is the same job without the
switch in the same process, never an absolute number.  Writes the record to profiles/alleles_<mb>mb.md (or --out) and prints one JSON
line.  With --profile nothing is written: one warm-up and one run each way, for a `rocprofv3 --kernel-trace --stats -- python
tools/time_alleles.py ... --profile` run of its own; --kernels FILE_kernel_stats.csv then puts that run's rows of the counting kernel
and of the scan's largest kernels into the record.

usage: python tools/time_alleles.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--profile] [--kernels FILE.csv] [--out FILE.md]
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

MODES = (("off", 0), ("1/1000", 1000), ("1/100", 100))
KEYS = (("sites", "allele sites (host, before the scan)"), ("scan", "signal extraction + coverage"), ("push", "allele counts (push)"), ("ingest wait", "ingest (inflate + decode, device)"),
        ("file", "allele counts ({o}.alleles.tab)"), ("read-out", "allele counters to the host"), ("text", "allele table text (host)"))


def write_sites(path, contigs, step):
    """one row every `step` bases of every contig (REF A, ALT C: the kernel's work does not depend on the letters)"""
    n = 0
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n")
        for name, ln in contigs:
            f.write("".join("%s\t%d\t.\tA\tC\n" % (name, p) for p in range(step, ln + 1, step)))
            n += len(range(step, ln + 1, step))
    return n


def kernel_rows(path, top=6):
    """the al_count row and the `top` largest rows of a rocprofv3 kernel_stats.csv -> [(name, calls, total ns, average ns)]"""
    with open(path) as f:
        rows = [(r.get("Name", ""), r.get("Calls"), r.get("TotalDurationNs"), r.get("AverageNs")) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: -int(r[2] or 0))
    keep = [r for i, r in enumerate(rows) if i < top or "al_count" in r[0]]
    return [(r[0].split("(")[0][:60],) + r[1:] for r in keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam")
    ap.add_argument("--ref")
    ap.add_argument("--mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="one warm-up and one run each way, no record written (for rocprofv3)")
    ap.add_argument("--kernels", help="a rocprofv3 kernel_stats.csv of a --profile run: its rows go into the record")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mb:
        a.bam, a.ref = bench_file(a.mb)
    if not a.bam or not a.ref:
        ap.error("--bam and --ref, or --mb")
    if a.profile:
        a.reps = 1
    from tiddit_amd import __main__ as cli
    from tiddit_amd import _native, bamio
    ctx = _native.default_context()
    rd = bamio.BamReader(a.bam, batch_bytes=1 << 20)
    contigs = list(zip(rd.references, rd.lengths))
    rd.close()
    runs = {m: [] for m, _ in MODES}
    notes = {}
    with tempfile.TemporaryDirectory() as d:
        sites = {}
        for mode, step in MODES:
            if step:
                sites[mode] = os.path.join(d, "sites_%d.vcf" % step)
                notes[mode] = {"rows": write_sites(sites[mode], contigs, step)}
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode, step in MODES:
                out = os.path.join(d, "r%d_%d" % (i, step))
                os.environ.pop("TIDDIT_ALLELES", None)
                if step:
                    os.environ["TIDDIT_ALLELES"] = sites[mode]
                buf = io.StringIO()
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(buf):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    os.environ.pop("TIDDIT_ALLELES", None)
                S = {k.strip(): v for k, v in cli.STAGE_SECONDS.items()}
                rec = {"wall": time.perf_counter() - t0}
                rec.update({short: S[key] for short, key in KEYS if key in S})
                assert os.path.exists(out + ".alleles.tab") == bool(step)
                if i:
                    runs[mode].append(rec)
                if step and i == a.reps:
                    notes[mode]["summary"] = next(l for l in buf.getvalue().split("\n") if l.startswith("allele counts:"))

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    keys = ["wall"] + [short for short, _ in KEYS]
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "notes": notes,
           "median_s": {m: {k: med(m, k) for k in keys} for m, _ in MODES}, "runs": runs}
    print(json.dumps(res))
    if a.profile:
        return
    path = a.out or os.path.join(REPO, "profiles", "alleles_%dmb.md" % a.mb if a.mb else "alleles.md")
    with open(path, "w") as f:
        f.write("# The allele counts of `tiddit --sv` (`TIDDIT_ALLELES`)\n\n")
        f.write("File: `%s` (%.0f MB).  `tools/time_alleles.py`: one process, after one warm-up round %d rounds of { `--sv --skip_assembly` switch "
                "off, one site per 1000 bp, one site per 100 bp }, interleaved.  Wall seconds; the yardstick is the off job of the same "
                "process; no budget was fixed in advance, this is what was measured.  `wall` includes the host reading the sites file before "
                "the scan (Python, row by row).\n\n" % (os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam),
                                                       os.path.getsize(a.bam) / 1e6, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        labels = {"wall": "whole job", "sites": "sites file read on the host (before the scan)", "scan": "scan stage", "push": "new stage timer (pushes, host side)", "ingest wait": "scan: waited for the ingest",
                  "file": "counters off the device + file", "read-out": "counters to the host", "text": "file text"}
        for mode, _ in MODES:
            for key in keys:
                if med(mode, key) is None:
                    continue
                f.write("| %s: %s | %s | %.4f |\n" % (mode, labels[key], " | ".join("%.4f" % r[key] for r in runs[mode]), med(mode, key)))
        off = [r["scan"] for r in runs["off"]]
        f.write("\nScan stage, off runs: spread %.4f s (min %.4f, max %.4f).  Scan stage against the off median: %s.\n" % (
            max(off) - min(off), min(off), max(off),
            ", ".join("%s %+.4f s" % (m, med(m, "scan") - med("off", "scan")) for m, s in MODES if s)))
        for mode, _ in MODES:
            if mode in notes:
                f.write("\n%s: %d rows; %s\n" % (mode, notes[mode]["rows"], notes[mode].get("summary", "")))
        if a.kernels:
            f.write("\nKernels (`rocprofv3 --kernel-trace --stats`, a run of its own: one warm-up and one run each of off / 1/1000 / 1/100, so "
                    "`al_count` ran for four jobs' batches; the largest kernels of the six jobs beside it):\n\n"
                    "| kernel | calls | total ns | average ns |\n|---|---|---|---|\n")
            for row in kernel_rows(a.kernels):
                f.write("| `%s` | %s | %s | %s |\n" % row)


if __name__ == "__main__":
    main()
