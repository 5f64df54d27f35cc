"""What the allele-specific copy number of `tiddit --sv` (TIDDIT_ASCN) costs the job: `tiddit --sv --skip_assembly` with
`TIDDIT_CNV=1 TIDDIT_ALLELES=<one site per 1000 bp>` and the switch off and on, interleaved, in one process — the whole job's wall, the
stage's seconds and its parts (upload of the counter table, the emissions launch, the five segmentation launches, segments, text),
and the CNV stage beside them.  The yardstick is the same job without the switch in the same process, never an absolute number; the
spread of the off runs is stated.  Writes the record to profiles/ascn_<mb>mb.md (or --out) and prints one JSON line.  With --profile
nothing is written: one warm-up and one run each way, for a `rocprofv3 --kernel-trace --stats -- python tools/time_ascn.py ...
--profile` run of its own; --kernels FILE_kernel_stats.csv then puts that run's rows of the new kernels, and of the five 8-state
launches of TIDDIT_CNV over the same bins, into the record.  No threshold is set here: the record is what was measured.

usage: python tools/time_ascn.py (--bam WGS.bam --ref ref.fa | --mb 240) [--reps 3] [--profile] [--kernels FILE.csv] [--out FILE.md]
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

from time_alleles import write_sites  # noqa: E402
from time_cov_track import bench_file  # noqa: E402  (the same synthetic file)

STAGE = "allele-specific copy number ({o}.ascn.bed)"
CNV_STAGE = "copy-number segments ({o}.cnv.bed)"
MODES = (("off", None), ("on", "1"))
KERNELS = ("ascn_emissions_kernel", "h16_chunk_matrices", "h16_carry", "h16_backpointers", "h16_chunk_ends", "h16_backtrace",
           "cnv_chunk_matrices", "cnv_carry", "cnv_backpointers", "cnv_chunk_ends", "cnv_backtrace")


def kernel_rows(path):
    """the rows of the new kernels and of the 8-state chain in a rocprofv3 kernel_stats.csv -> [(name, calls, total ns, average ns)]"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            k = next((k for k in KERNELS if k in r.get("Name", "")), None)
            if k:
                rows.append((k, r.get("Calls"), r.get("TotalDurationNs"), r.get("AverageNs")))
    return sorted(rows, key=lambda r: KERNELS.index(r[0]))


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
    rd = bamio.BamReader(a.bam, batch_bytes=1 << 20)
    contigs = [(c["SN"], c["LN"]) for c in rd.header["SQ"]]
    rd.close()
    ctx = _native.default_context()
    runs = {m: [] for m, _ in MODES}
    parts, lines, bins = [], {}, None
    switches = ("TIDDIT_CNV", "TIDDIT_ALLELES", "TIDDIT_ASCN")
    with tempfile.TemporaryDirectory() as d:
        sites = os.path.join(d, "sites.vcf")
        n_sites = write_sites(sites, contigs, 1000)
        for i in range(a.reps + 1):                       # (the first round warms up: page cache, device buffers, code objects)
            for mode, value in MODES:
                out = os.path.join(d, "r%d%s" % (i, mode))
                os.environ.update(TIDDIT_CNV="1", TIDDIT_ALLELES=sites)
                if value:
                    os.environ["TIDDIT_ASCN"] = value
                t0 = time.perf_counter()
                try:
                    with contextlib.redirect_stdout(io.StringIO()):
                        cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", out, "--skip_assembly", "--force_overwrite"])
                    ctx.sync()
                finally:
                    for k in switches:
                        os.environ.pop(k, None)
                S = cli.STAGE_SECONDS
                rec = {"wall": time.perf_counter() - t0, "stage": S.get(STAGE), "CNV stage": S.get(CNV_STAGE)}
                rec.update({k.strip(): v for k, v in S.items() if k.startswith("  ASCN ")})
                assert os.path.exists(out + ".ascn.bed") == (value is not None) and os.path.exists(out + ".cnv.bed")
                if i:
                    runs[mode].append(rec)
                if value and i == a.reps:
                    lines = {"ascn.bed": open(out + ".ascn.bed").read().count("\n") - 1, "cnv.bed": open(out + ".cnv.bed").read().count("\n") - 1}
                    parts = [k for k in rec if k.startswith("ASCN ")]
                    bins = sum(-(-ln // 500) for _, ln in contigs)

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    off = [r["wall"] for r in runs["off"]]
    res = {"bam": a.bam, "bam_MB": round(os.path.getsize(a.bam) / 1e6, 1), "reps": a.reps, "sites": n_sites, "segments": lines,
           "off_spread_s": [min(off), max(off)],
           "median_s": {m: {k: med(m, k) for k in ["wall", "stage", "CNV stage"] + parts} for m, _ in MODES}, "runs": runs}
    print(json.dumps(res))
    if a.profile:
        return
    path = a.out or os.path.join(REPO, "profiles", "ascn_%dmb.md" % a.mb if a.mb else "ascn.md")
    with open(path, "w") as f:
        f.write("# The allele-specific copy number of `tiddit --sv` (`TIDDIT_ASCN`)\n\n")
        f.write("File: `%s` (%.0f MB), %d sites (one per 1000 bp), at most %d CNV bins of 500 bp.  `tools/time_ascn.py`: one process, after one "
                "warm-up round %d rounds of { `--sv --skip_assembly` with `TIDDIT_CNV=1 TIDDIT_ALLELES=sites.vcf`, the same with `TIDDIT_ASCN=1` }, "
                "interleaved.  Wall seconds; the yardstick is the off job; no budget was fixed in advance, this is what was measured.\n\n"
                % (os.path.basename(os.path.dirname(a.bam)) + "/" + os.path.basename(a.bam), os.path.getsize(a.bam) / 1e6, n_sites, bins or 0, a.reps))
        f.write("| | " + " | ".join("run %d" % (k + 1) for k in range(a.reps)) + " | median |\n|---|" + "---|" * (a.reps + 1) + "\n")
        for mode, _ in MODES:
            keys = ["wall", "CNV stage"] if mode == "off" else ["wall", "CNV stage", "stage"] + parts
            for key in keys:
                label = "whole job" if key == "wall" else "the stage" if key == "stage" else key
                f.write("| %s: %s | %s | %.4f |\n" % (mode, label, " | ".join("%.4f" % r[key] for r in runs[mode]), med(mode, key)))
        f.write("\nThe off runs spread over %.4f ... %.4f s (%.4f s); the medians of the whole job differ by %+.4f s.\n"
                % (min(off), max(off), max(off) - min(off), med("on", "wall") - med("off", "wall")))
        f.write("\nSegments written in the last round: %s\n" % ", ".join("%s: %d" % kv for kv in sorted(lines.items())))
        if a.kernels:
            f.write("\nKernels (`rocprofv3 --kernel-trace --stats`, a run of its own: one warm-up and one run each of off / on — the `cnv_*` launches "
                    "run four times, the new ones twice, all over the same bins):\n\n| kernel | calls | total ns | average ns |\n|---|---|---|---|\n")
            for row in kernel_rows(a.kernels):
                f.write("| `%s` | %s | %s | %s |\n" % row)


if __name__ == "__main__":
    main()
