"""Wall of `tiddit --sv --skip_assembly` with and without the native variant stage (TIDDIT_VARIANTS=1), in one process, runs
interleaved: the variant stage's own seconds (and its parts), the scan's time in the evidence store's pack launches, and the
scan stage with the switch on against off.  One JSON line.

usage: python tools/time_variants.py --bam WGS.bam --ref ref.fa [--reps 3]
(bench.py leaves its 240-Mb file at $TIDDIT_BENCH_TMP/tiddit_bench_sv_240/)"""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam", required=True)
    ap.add_argument("--ref", required=True)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from tiddit_amd import __main__ as cli
    from tiddit_amd import tiddit_signal
    runs = {"off": [], "on": []}
    with tempfile.TemporaryDirectory() as d:
        for i in range(a.reps + 1):                       # (the first pair warms up)
            for mode in ("off", "on"):
                if mode == "on":
                    os.environ["TIDDIT_VARIANTS"] = "1"
                else:
                    os.environ.pop("TIDDIT_VARIANTS", None)
                cli.main(["--sv", "--bam", a.bam, "--ref", a.ref, "-o", os.path.join(d, "r%d%s" % (i, mode)), "--skip_assembly", "--force_overwrite"])
                rec = dict(cli.STAGE_SECONDS)
                rec["scan: evidence store (pack)"] = tiddit_signal.SCAN_SECONDS.get("evidence store (pack)")
                if i:
                    runs[mode].append(rec)
        os.environ.pop("TIDDIT_VARIANTS", None)
        n_vcf = sum(1 for l in open(os.path.join(d, "r1on.vcf")) if not l.startswith("#"))

    def med(mode, key):
        v = [r[key] for r in runs[mode] if r.get(key) is not None]
        return statistics.median(v) if v else None
    keys = sorted(set(k for r in runs["on"] for k in r))
    out = {"bam": a.bam, "reps": a.reps, "vcf_records": n_vcf,
           "scan_s_off": med("off", "signal extraction + coverage"), "scan_s_on": med("on", "signal extraction + coverage"),
           "on_median_s": {k: med("on", k) for k in keys}, "runs": runs}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
